"""The CPU oracle against an INDEPENDENT float64 formulation (tests/f64_reference.py): plane intersection + Gram-system
barycentrics over all triangles instead of the oracle's fused fp32 Möller–Trumbore / BVH, numpy transcendental functions,
exact-digit Halton.  Tolerances, not bits: the two sides share no arithmetic.

This tightens the oracle's pin as far as the environment allows (VERDICT r1 "weak 1"); parity against the Metal renderer
itself stays UNPINNED — the reference has no fixtures and cannot run here."""
import numpy as np
import pytest

import f64_reference as F


def _random_rays(rng, n, lo, hi):
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2 + 1e-3
    o = c + rng.normal(size=(n, 3)) * r * 1.5
    t = lo + rng.random((n, 3)) * (hi - lo)
    d = t - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = np.inf
    return rays


@pytest.mark.parametrize("name", ["plane", "plane-back", "sphere", "train", "treefir", "teapot"])
def test_oracle_intersector_matches_float64_plane_formulation(orc, mrt, name):
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name=name, position=[0.1, -0.2, 0.3], rotation=[0.2, 0.5, -0.1], scale=1.3)]
    sc = S((8, 8))
    flat = mrt.flatten_scene(sc)
    osc = orc.OracleScene(flat, sc.lights)
    tris = F.Triangles(flat)
    assert len(tris) == osc.triangles
    w = np.concatenate([tris.v0, tris.v1, tris.v2])
    rays = _random_rays(np.random.default_rng(11), 600 if name != "teapot" else 250, w.min(0), w.max(0))
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    t, u, v, ti, t2 = tris.intersect(o, d, np.full(len(o), np.inf))
    for brute in (True, False):
        h = osc.intersect_closest(rays, brute=brute)
        hit64 = ti >= 0
        # a ray is "decided" when it is clear of triangle edges and of a second surface at the same distance
        edge = np.where(hit64, np.minimum(np.minimum(u, v), 1 - u - v), 1.0)
        with np.errstate(invalid="ignore"):
            sep = np.where(hit64, (t2 - t) / np.maximum(t, 1e-9), 1.0)
        decided = (edge > 1e-4) & (sep > 1e-4)
        assert decided.mean() > 0.9
        # misses in float64 that graze an edge may be hits in fp32 and vice versa: only decided rays must agree on hit / miss
        agree = (h["type"] == 1) == hit64
        assert agree[decided].all(), f"{(~agree & decided).sum()} decided rays disagree on hit/miss"
        assert agree.mean() > 0.995
        m = decided & hit64
        assert m.sum() > 20
        assert np.allclose(h["distance"][m], t[m], rtol=2e-5, atol=1e-6)
        assert np.abs(h["u"][m] - u[m]).max() < 5e-4 and np.abs(h["v"][m] - v[m]).max() < 5e-4
        ids = tris.ids[ti[m]]
        assert np.array_equal(h["instance_id"][m], ids[:, 0]) and np.array_equal(h["geometry_id"][m], ids[:, 1]) and np.array_equal(h["primitive_id"][m], ids[:, 2])
    # any-hit with a finite tmax
    rays[:, 7] = 2.0
    t, u, v, ti, t2 = tris.intersect(o, d, np.full(len(o), 2.0))
    a = osc.intersect_any(rays, brute=True)
    edge = np.where(ti >= 0, np.minimum(np.minimum(u, v), 1 - u - v), 1.0)
    near_tmax = np.abs(t - 2.0) < 1e-4
    ok = (edge > 1e-4) & ~near_tmax
    # any-hit is a boolean over ALL triangles: a grazing hit elsewhere may flip it, so allow a few
    assert ((a == 1) == (ti >= 0))[ok].mean() > 0.995


def test_oracle_image_matches_float64_restatement_on_a_cornell_crop(orc, mrt):
    """trace_pixel in float64 (brute force over all 4 910 triangles) for a 16x16 block of the 64x64 Cornell frame,
    two accumulated frames, against the oracle's fp32 image."""
    W = H = 64
    sc = mrt.CornellScene((W, H))
    flat = mrt.flatten_scene(sc)
    osc = orc.OracleScene(flat, sc.lights)
    r = orc.OracleRenderer(osc, W, H, seed=1, max_bounces=3, camera=sc.camera)
    r.render(1); img0 = r.accumulation().copy()
    r.render(1); img1 = r.accumulation().copy()
    tris = F.Triangles(flat)
    seeds = np.array([orc.seed_hash(1, i) for i in range(W * H)], np.int64).reshape(H, W)
    assert seeds.max() < (1 << 20)
    pix = [(x, y) for y in range(20, 36) for x in range(24, 40)]       # covers the sphere's silhouette, its shadow and the floor
    f0, m0 = F.render_frame(tris, sc.lights, sc.camera, W, H, seeds, 0, pix)
    f1, m1 = F.render_frame(tris, sc.lights, sc.camera, W, H, seeds, 1, pix)
    ref0 = f0
    ref1 = (f1 + f0 * 1.0) / 2.0                                       # Raytracing.metal:394-401 with frameIndex = 1
    ys, xs = np.array([p[1] for p in pix]), np.array([p[0] for p in pix])
    for img, ref, margin in ((img0, ref0, m0), (img1, ref1, np.minimum(m0, m1))):
        got = img[ys, xs, :3].astype(np.float64)
        assert np.all(img[ys, xs, 3] == 1.0)
        d = np.abs(got - ref).max(1)
        safe = margin > 1e-3                                           # paths that stayed clear of every discrete decision boundary
        assert safe.mean() > 0.7
        # measured: max 2.5e-6 over all 256 pixels, median 7e-8 (fp32 rounding of radiance values up to 3.4)
        assert (d[safe] <= 2e-5).mean() >= 0.97, f"{(d[safe] > 2e-5).sum()} of {safe.sum()} safe pixels differ by more than 2e-5 (max {d[safe].max():.3g})"
        assert np.median(d) < 1e-6
        assert ref.max() > 0.5 and (ref.sum(1) > 0).mean() > 0.5       # the crop is lit: the comparison is not vacuous


def _crop_against_f64(orc, mrt, sc, W, H, x0, y0, frames=2, side=16, materials=False, max_bounces=3, image=None):
    """The oracle's fp32 image of `sc` against tests/f64_reference.render_frame on a side x side block, `frames` accumulated frames; the tolerance rule of the
    Cornell crop above, scaled with the radiance range.  `materials`: the extension of docs/HISTORY.md §10 on both sides.  `image(f)`: the (H, W, 4) accumulation after
    frame f from another renderer of the same definition (the GPU's) in place of the oracle's.
    Returns (f64 radiance of frame 0, margin, triangles, pixels, per-path branch tally summed over the frames) for the callers' own checks."""
    flat = mrt.flatten_scene(sc)
    tris = F.Triangles(flat)
    if image is None:
        osc = orc.OracleScene(flat, sc.lights)
        r = orc.OracleRenderer(osc, W, H, seed=1, max_bounces=max_bounces, camera=sc.camera)
        r.set_materials(materials)
        assert len(tris) == osc.triangles
        def image(f):
            r.render(1)
            return r.accumulation().copy()
    seeds = np.array([orc.seed_hash(1, i) for i in range(W * H)], np.int64).reshape(H, W)
    pix = [(x, y) for y in range(y0, y0 + side) for x in range(x0, x0 + side)]
    ys, xs = np.array([p[1] for p in pix]), np.array([p[0] for p in pix])
    ref, margin, first, tally = None, np.full(len(pix), np.inf), None, 0
    for f in range(frames):
        img = image(f)
        ff, m, t = F.render_frame(tris, sc.lights, sc.camera, W, H, seeds, f, pix, max_bounces=max_bounces, materials=materials, tally=True)
        first = ff if first is None else first
        ref = ff if f == 0 else (ff + ref * float(f)) / float(f + 1)          # Raytracing.metal:394-401
        margin = np.minimum(margin, m); tally = tally + t
        got = img[ys, xs, :3].astype(np.float64)
        assert np.all(img[ys, xs, 3] == 1.0)
        d = np.abs(got - ref).max(1)
        safe = margin > 1e-3
        scale = max(1.0, float(ref.max()))
        print(f"crop ({x0}, {y0}) frame {f}: safe {safe.mean():.3f}, max over safe pixels {d[safe].max():.3g}, median {np.median(d):.3g}, scale {scale:.3g}")
        assert safe.mean() > 0.5, safe.mean()
        # measured with materials on the Cornell box of tests/material_scenes.py (glass + gold-like spheres, 4 bounces): max 1.6e-6 over the safe pixels of the WHOLE
        # 64 x 48 frame, scale 2.5 — curved glass does not need a wider bound than the plain crops
        assert (d[safe] <= 2e-5 * scale).mean() >= 0.97, f"frame {f}: {(d[safe] > 2e-5 * scale).sum()} of {safe.sum()} safe pixels differ by more than {2e-5 * scale:.1e} (max {d[safe].max():.3g})"
        assert np.median(d) < 2e-6 * scale
    return first, margin, tris, pix, tally


def _without_light(lights, k):
    """the same lights (same count: the same light is picked for every sample) with light k's colour zeroed"""
    import copy
    out = [copy.copy(l) for l in lights]
    z = type(lights[k].color)()
    z.x = z.y = z.z = 0.0
    out[k].color = z
    return out


def test_oracle_image_matches_float64_on_a_dragonscene_crop_spot_light_rotated_trs_six_submeshes(orc, mrt):
    """DragonScene (Scene.swift:21-30 lights: area + SPOT; DragonScene.swift:14-22 transforms) with the 871 K-triangle dragon replaced by train.obj at the dragon's own
    position / ROTATION / scale x 0.3 — a rotated, scaled, translated instance of a SIX-submesh mesh where the dragon stands, in the spot light's cone — on a 16 x 16 crop that
    holds both trains, the fir and both planes.  Pins the oracle's spot-light branch (Raytracing.metal:292-316), M * n for a rotated TRS (:266-268) and the per-submesh colour
    lookup (:262-269) against a formulation that shares none of its arithmetic."""
    W, H = 96, 54

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            full = mrt.DragonScene(size).models
            dr = [mo for mo in full if mo.name == "dragon"][0]
            self.models = [mo if mo.name != "dragon" else mrt.Model(name="train", position=dr.position, rotation=dr.rotation, scale=0.3 * dr.scale) for mo in full]
    sc = S((W, H))
    assert [l.type for l in sc.lights] == [4, 2] and sc.models[1].rotation[1] != 0
    f0, margin, tris, pix, _ = _crop_against_f64(orc, mrt, sc, W, H, 40, 12)
    # not vacuous: the spot light carries a visible part of the crop, and the crop sees many submeshes of both trains
    seeds = np.array([orc.seed_hash(1, i) for i in range(W * H)], np.int64).reshape(H, W)
    dark, _ = F.render_frame(tris, _without_light(sc.lights, 1), sc.camera, W, H, seeds, 0, pix)
    assert ((f0 - dark).max(1) > 0.02).mean() > 0.1, ((f0 - dark).max(1) > 0.02).mean()
    cam = sc.camera
    f3 = lambda v: np.array([v.x, v.y, v.z], np.float64)
    px = np.array(pix, np.float64) + 0.5
    uv = px / np.array([W, H]) * 2 - 1
    d = uv[:, :1] * f3(cam.right) + uv[:, 1:] * f3(cam.up) + f3(cam.forward); d /= np.linalg.norm(d, axis=1, keepdims=True)
    _, _, _, ti, _ = tris.intersect(np.broadcast_to(f3(cam.position), d.shape), d, np.full(len(d), np.inf))
    seen = {tuple(tris.ids[k][:2]) for k in ti if k >= 0}
    assert len({g for i, g in seen if i == 0}) >= 4 and len({g for i, g in seen if i == 1}) >= 4, seen      # (instance, geometry): >= 4 submeshes of each train


def test_oracle_image_matches_float64_on_a_garden_crop_sun_and_spot(orc, mrt):
    """BASELINE.json configs[3]'s lights — SPOT + SUN (Scene.swift:82-106; metal-raytracing_amd/scene.py GardenScene) — on the garden's floor, back wall, one teapot
    (15 704 triangles, GENERATED normals, rotation 7.0 rad about y, scale 0.008) and two firs, 16 x 16 crop over the teapot's silhouette and shadow.  Pins the oracle's
    sun branch (Raytracing.metal:323-327: infinite light distance, no falloff) and the spot branch at another geometry."""
    W, H = 96, 54

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            g = mrt.GardenScene(size)
            keep = [("plane", None), ("plane-back", None), ("teapot", (0.8, 0.0, 2.0)), ("treefir", (0.8, 0.0, -1.2)), ("treefir", (-0.8, 0.0, 0.4))]
            self.models = [mo for mo in g.models if any(mo.name == n and (p is None or tuple(mo.position) == p) for n, p in keep)]
            self.lights = g.lights
    sc = S((W, H))
    assert [l.type for l in sc.lights] == [2, 1] and len(sc.models) == 5
    f0, margin, tris, pix, _ = _crop_against_f64(orc, mrt, sc, W, H, 50, 7)
    seeds = np.array([orc.seed_hash(1, i) for i in range(W * H)], np.int64).reshape(H, W)
    for k in (0, 1):          # each of the two lights carries a visible part of the crop
        dark, _ = F.render_frame(tris, _without_light(sc.lights, k), sc.camera, W, H, seeds, 0, pix)
        assert ((f0 - dark).max(1) > 0.02).mean() > 0.1, (k, ((f0 - dark).max(1) > 0.02).mean())


def test_oracle_image_matches_float64_on_a_cornell_crop_with_point_and_spot_lights(orc, mrt):
    """The Cornell box lit by a POINT light (Raytracing.metal:317-322) and a spot light whose cone edge crosses the crop (the comparison `spot > cos(coneAngle)`, :306)."""
    W = H = 64
    sc = mrt.CornellScene((W, H))
    sc.lights = [mrt.Light.pointLight(position=[0.3, 1.6, 0.4], color=[2.0, 1.5, 1.0]),
                 mrt.Light.spotLight(position=[-0.6, 1.8, 0.8], direction=[0.5, -1.0, -0.6], coneAngle=np.float32(18.0 / 180.0 * np.pi), color=[5, 5, 6])]
    assert [l.type for l in sc.lights] == [3, 2]
    f0, margin, tris, pix, _ = _crop_against_f64(orc, mrt, sc, W, H, 24, 20)
    seeds = np.array([orc.seed_hash(1, i) for i in range(W * H)], np.int64).reshape(H, W)
    for k in (0, 1):
        dark, _ = F.render_frame(tris, _without_light(sc.lights, k), sc.camera, W, H, seeds, 0, pix)
        assert ((f0 - dark).max(1) > 0.02).mean() > 0.1, (k, ((f0 - dark).max(1) > 0.02).mean())


# ---------------------------------------------------------------- the materials extension (docs/HISTORY.md §10)
MATERIAL_CROPS = [(16, 8), (28, 8)]          # 64 x 48 frame: over the right half of the glass sphere and its silhouette; over the gold-like sphere's top and left silhouette


def materials_crop_is_not_vacuous(tally):
    """the crop holds paths through every kind of event the extension adds (the float64 side knows what each of its paths did)"""
    t = dict(zip(F.BRANCHES, tally.sum(0)))
    assert t["reflect"] >= 3 and t["refract"] >= 50 and t["specular"] >= 30 and t["emitter"] >= 3 and t["diffuse"] >= 500 and t["absorbed"] >= 1, t


@pytest.mark.parametrize("x0,y0", MATERIAL_CROPS)
def test_oracle_materials_match_float64_physics_on_a_cornell_crop(orc, mrt, x0, y0):
    """The oracle's `if (materials)` against the float64 restatement of docs/HISTORY.md §10 (Householder reflection, refraction by angles, the lobe through arccos):
    Cornell box with a glass sphere (dissolve 0.15, Ni 1.5), a gold-like sphere (Ks 0.8 / Ns 96) and an emissive panel, 4 bounces, two accumulated frames."""
    from material_scenes import cornell_with_materials
    W, H = 64, 48
    sc = cornell_with_materials(mrt, (W, H))
    _, margin, _, _, tally = _crop_against_f64(orc, mrt, sc, W, H, x0, y0, materials=True, max_bounces=4)
    materials_crop_is_not_vacuous(tally)


# pure-function checks of the float64 helpers: what the restatement is itself pinned by
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _incident(rng, n, lo_deg=3.0, hi_deg=87.0):
    """unit normals and unit directions arriving at them (d.n < 0) at angles of incidence in [lo, hi] degrees"""
    nn = _unit(rng, n)
    t = _unit(rng, n); t -= (t * nn).sum(1, keepdims=True) * nn; t /= np.linalg.norm(t, axis=1, keepdims=True)
    th = np.radians(rng.uniform(lo_deg, hi_deg, n))
    return nn, -np.cos(th)[:, None] * nn + np.sin(th)[:, None] * t, th


def test_f64_reflection_is_the_mirror_image():
    rng = np.random.default_rng(21)
    n, d, th = _incident(rng, 200)
    r = F.householder(n, d)
    assert np.allclose((r * n).sum(1), -(d * n).sum(1), atol=1e-14) and np.allclose(r - (r * n).sum(1, keepdims=True) * n, d - (d * n).sum(1, keepdims=True) * n, atol=1e-14)
    assert np.allclose(np.linalg.norm(r, axis=1), 1.0, atol=1e-14) and np.allclose(F.householder(-n, d), r, atol=1e-15) and np.allclose(F.householder(n, r), d, atol=1e-14)
    assert np.allclose(F.householder([[0.0, 1.0, 0.0]], [[0.6, -0.8, 0.0]]), [[0.6, 0.8, 0.0]], atol=1e-16)


@pytest.mark.parametrize("ni", [1.5, 2.4, 1.0, 0.67])
def test_f64_refraction_obeys_snell_and_stays_in_the_plane_of_incidence(ni):
    rng = np.random.default_rng(22)
    n, d, th = _incident(rng, 400)
    for flip in (False, True):                       # entering (d.n < 0, eta = 1 / ni) and leaving (the same rays against -n, eta = ni)
        r = F.dielectric(d, -n if flip else n, ni)
        eta = ni if flip else 1.0 / ni
        assert (r["entering"] != flip).all() and np.allclose(r["eta"], eta) and np.allclose(r["theta_i"], th, atol=1e-13)
        assert np.array_equal(r["tir"], eta * np.sin(th) >= 1.0)
        ok = ~r["tir"]
        assert ok.sum() > 50                             # leaving a medium of index 2.4: only below the critical angle of 24.6 degrees
        t = r["refracted"][ok]
        assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() < 1e-12
        sin_t = np.linalg.norm(np.cross(t, n[ok]), axis=1)
        assert np.abs(sin_t - eta * np.sin(th[ok])).max() < 1e-12                                        # Snell
        assert np.abs(np.einsum("ki,ki->k", np.cross(d[ok], n[ok]), t)).max() < 1e-12                  # coplanar with d and n
        assert ((t * n[ok]).sum(1) < 0).all()                                                          # goes on through the surface ...
        tang = lambda v: v - (v * n[ok]).sum(1, keepdims=True) * n[ok]
        assert ((tang(t) * tang(d[ok])).sum(1) > 0).all()                                              # ... on the same side of the normal
        if ni == 1.0:
            assert np.abs(t - d[ok]).max() < 1e-12 and np.abs(r["F"][ok] - (1.0 - np.cos(th[ok])) ** 5).max() < 1e-12                    # Ni 1 bends nothing


def test_f64_refraction_in_and_out_through_parallel_faces_returns_the_direction():
    rng = np.random.default_rng(23)
    for ni in (1.5, 2.4, 0.67, 1.0):
        n, d, th = _incident(rng, 300)
        a = F.dielectric(d, n, ni)
        ok = ~a["tir"]
        b = F.dielectric(a["refracted"][ok], -n[ok], ni)             # the far face of a slab: its normal points out of the medium, the other way
        assert not b["entering"].any() and not b["tir"].any()
        assert np.abs(b["refracted"] - d[ok]).max() < 1e-12
        assert np.abs(b["F"] - a["F"][ok]).max() < 1e-12               # §10: the transmitted cosine when leaving == the incident cosine when entering


def test_f64_schlick_limits():
    n = np.array([[0.0, 1.0, 0.0]])
    for ni in (1.5, 2.4, 0.67):
        r0 = ((1 - ni) / (1 + ni)) ** 2
        assert abs(F.dielectric([[0.0, -1.0, 0.0]], n, ni)["F"][0] - r0) < 1e-15                        # normal incidence, entering
        assert abs(F.dielectric([[0.0, 1.0, 0.0]], n, ni)["F"][0] - r0) < 1e-15                         # and leaving
        th = np.radians(np.array([30.0, 60.0, 80.0, 89.0, 89.9, 89.999]))
        r = F.dielectric(np.c_[np.sin(th), -np.cos(th), 0 * th], np.repeat(n, len(th), 0), ni)
        f = r["F"]
        if ni > 1.0:
            assert (np.diff(f) > 0).all() and f[0] > r0 and 1.0 - f[-1] < 1e-3 and (f <= 1.0).all()     # tends to 1 at grazing incidence
        else:                                            # into a thinner medium: total internal reflection beyond arcsin(0.67) = 42 degrees
            assert r["tir"].tolist() == [False] + [True] * 5 and r0 < f[0] < 1.0 and (f[1:] == 1.0).all()
    c = 0.5 ** 0.5
    assert abs(F.dielectric([[c, -c, 0.0]], n, 1.5)["F"][0] - (0.04 + 0.96 * (1 - c) ** 5)) < 1e-15


def test_f64_specular_half_vector_distribution():
    """theta = arccos sqrt((1 - v) / (1 + (a2 - 1) v)) inverts the GGX cumulative: v = 0 is the normal itself, v -> 1 grazing, the median half angle has tan^2 = a2; the frame is the diffuse branch's."""
    rng = np.random.default_rng(24)
    nw = _unit(rng, 50)
    u = rng.random(50)
    for Ns in (0.01, 30.0, 1e6):
        a2 = 2.0 / (Ns + 2.0)
        h0 = F.specular_half_vector(u, np.zeros(50), Ns, nw)
        assert np.abs(h0 - nw).max() < 1e-12
        hm = F.specular_half_vector(u, np.full(50, 0.5), Ns, nw)
        cos2 = (hm * nw).sum(1) ** 2
        assert np.abs((1 - cos2) / cos2 - a2).max() < 1e-9 * max(1.0, a2) and np.abs(np.linalg.norm(hm, axis=1) - 1).max() < 1e-12
    y = np.array([[0.0, 1.0, 0.0]])
    h = F.specular_half_vector(np.array([0.0]), np.array([0.5]), 0.0, y)[0]       # Ns = 0: a2 = 1, cos^2 = 1 - v; phi = 0 lies along `right` = normalize(y x (0.0072, 1, 0.0034))
    right = np.cross(y[0], [0.0072, 1.0, 0.0034]); right /= np.linalg.norm(right)
    assert np.allclose(h, np.sqrt(0.5) * right + np.sqrt(0.5) * y[0], atol=1e-15)
