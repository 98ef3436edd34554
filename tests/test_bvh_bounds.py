"""Every box the 8-wide build emits, audited exactly (tests/bvh_audit.py), on scenes made to put triangles on the edges of their boxes: walls that lie
exactly on x = +-1, y = 0 and z = -1, a "stadium" (a ground quad 2000 units across under ~200 meshes of 1e-3 ... 1e-1 near the origin and at the
ground's corners and edges), both again 1.3e4 units from the origin, and the walls at 1e-4 scale where the absolute pad dominates.  Every builder,
leaf size and pre-split setting; three refits of a 20 K-triangle mesh; two-level scenes under skewed, mirrored, near-singular, far and tiny
instance transforms, before and after a TLAS-only update.  Then rays aimed where the audit says the boxes are tightest, axis-aligned rays on the
decoded planes and in the walls' planes against the oracle's brute force (no BVH, no TLAS culling) bit for bit, and telephoto images.

Known gaps, kept as strict xfail tests with the failing ray recorded (KNOWN): rays 1e3 ... 1e4 units away lose hits to the box tests, since the
triangle test's rounding grows with the distance to the ray origin while the boxes are padded by the size of their coordinates; any-hit limits one
float past the hit still lose a few hits; two-level BLAS walks take a farther triangle for a few near-parallel rays; the two-level telephoto image
differs from the oracle.  The box tests' limit is widened by 4 ulp like their far side, which settles the any-hit edge and ties on t elsewhere.
Depth: builder = 0 reaches wide_depth 4 over coincident keys and 19 over clustered ones; nothing here goes past WIDE_DEPTH_REBUILD (48)."""
import numpy as np
import pytest

import bvh_audit as A
from test_fuzz_geometry import _Raw, _fan
from test_gpu_parity import assert_parity

FAR = np.array([1.3e4, -2.7e3, 7.1e3])
BUILDS = [dict(builder=b, max_leaf=m, presplit=p) for b in (0, 1, 2) for m in (1, 4) for p in (0, None)]


def _opts(d):
    return {k: v for k, v in d.items() if v is not None}


# ------------------------------------------------------------------------------------------------ geometry
def _quad(c, u, v, n=1):
    """an n x n tessellated parallelogram c + s u + t v, s, t in [-1, 1]"""
    g = np.linspace(-1, 1, n + 1)
    s, t = np.meshgrid(g, g)
    pos = (np.asarray(c, np.float64) + s.reshape(-1, 1) * u + t.reshape(-1, 1) * v).astype(np.float32)
    idx = np.array([[r * (n + 1) + k, r * (n + 1) + k + 1, (r + 1) * (n + 1) + k + 1, (r + 1) * (n + 1) + k] for r in range(n) for k in range(n)], np.uint32)
    return pos, np.vstack([idx[:, [0, 1, 2]], idx[:, [0, 2, 3]]])


def _cube(c=(0, 0, 0), h=1.0):
    p = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64) + c
    f = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    idx = np.array([[a, b, c_] for q in f for a, b, c_ in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint32)
    return p.astype(np.float32), idx


def _axis_parts():
    X, Y, Z = np.eye(3)
    return [_quad((1, 1, 0), Y, Z, 3), _quad((-1, 1, 0), Y, Z, 1), _quad((0, 0, 0), X, Z, 4), _quad((0, 1, -1), X, Y, 2),
            _cube((0.2, 0.4, 0.1), 0.25)] + [_quad((0.1 * k, 0.5, 0.05 * k), 0.3 * X, 0.3 * Z) for k in range(5)]      # five stacked coplanar quads at y = 0.5


class _Scene:
    """mrt.Scene stand-in built from (name, pos, idx, position, scale[, xf]) entries"""
    def __new__(cls, mrt, size, entries):
        sc = mrt.Scene(size)
        models = []
        for k, e in enumerate(entries):
            name, pos, idx, position, scale = e[:5]
            m = _Raw(mrt, name, pos, idx, (0.3 + 0.1 * (k % 5), 0.5, 0.7 - 0.1 * (k % 4)), position, [0, 0, 0], scale, share=e[6] if len(e) > 6 else None)
            if len(e) > 5 and e[5] is not None:
                m.meshes[0].transform = np.asarray(e[5], np.float32)
            models.append(m)
        sc.models = models
        return sc


def axis_scene(mrt, size, offset=(0, 0, 0), scale=1.0):
    parts = _axis_parts()
    return _Scene(mrt, size, [(f"wall{k}", p, i, offset, scale) for k, (p, i) in enumerate(parts)])


def stadium_scene(mrt, size, offset=(0, 0, 0), n=200, seed=5):
    rng = np.random.default_rng(seed)
    X, Z = np.eye(3)[0], np.eye(3)[2]
    ents = [("ground", *_quad((0, 0, 0), 1e3 * X, 1e3 * Z), offset, 1.0)]
    cube = _cube((0, 0, 0), 1.0); fan = _fan(rng, 20)
    for k in range(n):
        site = k % 4
        if site == 0:
            c = rng.uniform(-1, 1, 3) * [1, 0.5, 1] + [0, 0.5, 0]
        elif site == 1:
            c = np.array([rng.choice([-1e3, 1e3]), rng.uniform(0, 1), rng.choice([-1e3, 1e3])])
        else:
            c = np.array([rng.uniform(-1e3, 1e3), rng.uniform(0, 1), rng.choice([-1e3, 1e3])])[[0, 1, 2] if site == 2 else [2, 1, 0]]
        p, i = cube if k % 2 else fan
        ents.append((f"m{k}", p, i, np.asarray(offset) + c, float(10 ** rng.uniform(-3, -1))))
    return _Scene(mrt, size, ents)


def _xf(A3, t=(0, 0, 0)):
    """column-major 4x4 of p -> A3 p + t"""
    T = np.eye(4); T[:3, :3] = np.asarray(A3, np.float64).T; T[3, :3] = t
    return T.astype(np.float32)


def _rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]); Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


TRANSFORMS = {
    "identity": (np.eye(3), (0, 0, 0)),
    "rot_scale": (1.7 * _rot(0.3, 1.1, -0.4), (3, 0, 0)),
    "mirror": (np.diag([-1.0, 1, 1]) @ _rot(0.2, -0.5, 0.9), (-3, 0, 0)),
    "aniso": (_rot(0.4, 0.7, 0.1) @ np.diag([40.0, 1, 0.025]), (0, 3, 0)),
    "shear": (np.array([[1.0, 200, 0], [0, 1, 0], [0, 0, 1]]), (0, -3, 0)),
    "near_singular": (_rot(0.9, 0.2, 0.6) @ np.diag([1.0, 1.0, 1e-6]), (0, 0, 3)),
    "far": (_rot(0.1, 0.2, 0.3), (1e4, 0, 0)),
    "tiny": (1e-3 * np.eye(3), (0, 0, -3)),
}


def two_level_scene(mrt, size, names=tuple(TRANSFORMS)):
    import metal_raytracing_amd.scene as S
    sph = S.load_obj(S.find_resource("sphere"))
    sph_pos, sph_idx = sph[0], np.vstack([s.indices for s in sph[2]])
    meshes = [("cube", *_cube()), ("sphere", sph_pos, sph_idx), ("fan", *_fan(np.random.default_rng(9), 300))]
    sc = mrt.Scene(size)
    models, first = [], {}
    for mname, pos, idx in meshes:
        for k, tn in enumerate(names):
            A3, t = TRANSFORMS[tn]
            src = first.get(mname)
            m = _Raw(mrt, mname, pos, idx, (0.2 + 0.2 * k % 3, 0.6, 0.4), [0, 0, 0], [0, 0, 0], 1.0, share=src)
            m.meshes[0].transform = _xf(A3, np.asarray(t, np.float64) + [0, 0, 6.0 * len(models) / len(names)])
            first.setdefault(mname, m)
            models.append(m)
    sc.models = models
    return sc


# ------------------------------------------------------------------------------------------------ audit helpers
def _audit(ds, presplit, num_tris=None):
    lay = A.layout_of(ds)
    st = ds.stats
    assert int(lay["header"][3]) == st.wide_depth
    rep = A.audit(lay, presplit=presplit, num_tris=num_tris)
    rep.check()
    return rep, lay


# ------------------------------------------------------------------------------------------------ probes
def _oracle(orc, mrt, sc, two):
    return orc.OracleScene(mrt.flatten_scene(sc, share=two), sc.lights, instancing=two)


def _compare(ds_list, osc, rays, what, edge=False):
    """closest (both GPU paths) and any-hit against the oracle's brute force, bit for bit; returns the hit count.  Any-hit limits: 1.001 x the
    closest hit, or (edge) the next float past it."""
    ref = osc.intersect_closest(rays, brute=True)
    zero_min = rays[:, 3] == 0
    for name, ds in ds_list:
        got = ds.intersect_closest(rays)
        for f in ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v"):
            bad = np.nonzero(got[f].view(np.uint32) != ref[f].view(np.uint32))[0]
            assert len(bad) == 0, f"{what} {name} intersect_closest {f}: {len(bad)} rays differ, first ray {rays[bad[0]].tolist()}: gpu {got[bad[0]]} oracle {ref[bad[0]]}"
        if zero_min.all() and ds.stats.wide_layout:
            gs = ds.intersect_stream(rays)
            for f in ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v"):
                bad = np.nonzero(gs[f].view(np.uint32) != ref[f].view(np.uint32))[0]
                assert len(bad) == 0, f"{what} {name} intersect_stream {f}: {len(bad)} rays differ, first ray {rays[bad[0]].tolist()}: gpu {gs[bad[0]]} oracle {ref[bad[0]]}"
    r2 = rays.copy()
    fin = np.isfinite(ref["distance"]) & (ref["type"] == 1)
    r2[fin, 7] = np.nextafter(ref["distance"][fin], np.float32(np.inf)) if edge else ref["distance"][fin] * np.float32(1.001)      # (open rays as they are)
    ra = osc.intersect_any(r2, brute=True)
    for name, ds in ds_list:
        ga = ds.intersect_any(r2)
        bad = np.nonzero(ga != ra)[0]
        assert len(bad) == 0, f"{what} {name} intersect_any: {len(bad)} rays differ, first ray {r2[bad[0]].tolist()}: gpu {ga[bad[0]]} oracle {ra[bad[0]]}"
        if (r2[:, 3] == 0).all() and ds.stats.wide_layout:
            gsa = ds.intersect_stream(r2, any_hit=True)["type"]
            bad = np.nonzero(gsa != ra)[0]
            assert len(bad) == 0, f"{what} {name} intersect_stream any: {len(bad)} rays differ, first ray {r2[bad[0]].tolist()}"
    return int((ref["type"] == 1).sum())


def _world_of(lay, pk):
    """two-level: object -> world maps (3x4, float64) of one instance per packet's BLAS; None for flattened scenes"""
    if not int(lay["header"][2]):
        return None
    inst = A.decode_instances(lay["instances"])
    out = []
    for p in pk:
        i = int(np.nonzero((inst["packet_base"] <= p) & (p < inst["packet_base"] + inst["ntri"]))[0][0])
        R = inst["w2o"][i]; M = np.linalg.inv(R[:, :3])
        out.append(np.c_[M, -M @ R[:, 3]])
    return np.array(out)


RANGES = {"shadow": lambda rng, n, ext: ext * 10 ** rng.uniform(-4, -2, n), "mid": lambda rng, n, ext: 10 ** rng.uniform(0, 1, n),
          "far": lambda rng, n, ext: 10 ** rng.uniform(3, 4, n)}


def thin_rays(rep, lay, extent, rng, k=2000, ranges=("shadow", "mid")):
    """rays at the vertex / edge point that touches the tightest plane of the k thinnest packets, from the given distance ranges (RANGES: 1e-4 ...
    1e-2 of the extent, 1 ... 10, 1e3 ... 1e4), including directions nearly parallel to that plane"""
    pk, ax, side = A.thinnest(rep, lay, k)
    V, _ = A.decode_packets(lay["wpackets"])
    n = len(pk)
    if n == 0:
        return np.zeros((0, 8), np.float32)
    v = V[pk]                                                          # (n, 3, 3)
    key = v[np.arange(n)[:, None], np.arange(3)[None, :], ax[:, None]] * np.where(side == 0, 1, -1)[:, None]
    o3 = np.argsort(key, 1)
    vert = v[np.arange(n), o3[:, 0]]
    edge = 0.5 * (v[np.arange(n), o3[:, 0]] + v[np.arange(n), o3[:, 1]])
    M = _world_of(lay, pk)
    rays = []
    for target in (vert, edge):
        for dist in [RANGES[g](rng, n, extent) for g in ranges]:
            for parallel in (False, True):
                d = rng.normal(size=(n, 3))
                if parallel:      # along the plane, a little into it
                    d[np.arange(n), ax] = 0.0
                    d /= np.linalg.norm(d, axis=1, keepdims=True)
                    d[np.arange(n), ax] = np.where(side == 0, 1, -1) * 10 ** rng.uniform(-6, -2, n)
                d /= np.linalg.norm(d, axis=1, keepdims=True)
                t = target
                if M is not None:
                    t = np.einsum("nij,nj->ni", M[:, :, :3], target) + M[:, :, 3]
                    d = np.einsum("nij,nj->ni", M[:, :, :3], d); d /= np.linalg.norm(d, axis=1, keepdims=True)
                r = np.zeros((n, 8), np.float32)
                r[:, 0:3] = t - d * dist[:, None]; r[:, 4:7] = d; r[:, 7] = np.inf
                rays.append(r)
    return np.vstack(rays)


def axis_rays(lay, walls, rng, n=3000):
    """directions with exact zero components; origins on decoded plane values and on the walls' planes; rays inside the walls' planes"""
    D = A.decode_nodes(lay["wnodes"])
    occ = D["qlo"] <= D["qhi"]
    planes = [np.unique(np.float32(np.r_[D["lo"][..., a][occ[..., a]], D["hi"][..., a][occ[..., a]]])) for a in range(3)]
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, 1], [1, 0, -1], [0.6, 0, 0.8], [0, 0.8, -0.6]], np.float32)
    lo, hi = D["lo"][0][occ[0].all(1)].min(0), D["hi"][0][occ[0].all(1)].max(0)
    out = []
    for _ in range(n):
        d = dirs[rng.integers(len(dirs))].copy()
        o = rng.uniform(lo, hi)
        a = rng.integers(3)
        if rng.random() < 0.5:
            o[a] = rng.choice(planes[a])                               # on a decoded plane
        else:
            o[a] = rng.choice(walls[a]) if len(walls[a]) else o[a]    # on a wall's plane
            if rng.random() < 0.5:
                d[a] = 0.0                                              # in the wall's plane
                if not d.any():
                    d[(a + 1) % 3] = 1.0
        back = rng.uniform(0.5, 3.0) * max(1.0, float(np.abs(hi - lo).max()))
        nz = d != 0
        o2 = o.copy(); o2[nz] = o[nz] - d[nz] * back                 # step back along the non-zero components only: the zero ones stay on the plane
        out.append(np.r_[o2, 0.0, d, np.inf])
    r = np.array(out, np.float32)
    r[:, 4:7] /= np.linalg.norm(r[:, 4:7], axis=1, keepdims=True)
    r[:, 4:7][np.abs(r[:, 4:7]) < 1e-30] = 0.0
    return r


def _limited(rays, rng):
    r = rays.copy()
    r[:, 3] = np.float32(rng.uniform(1e-4, 0.5, len(r)))
    r[:, 7] = np.float32(rng.uniform(1.0, 6.0, len(r)))
    return r


def telephoto(mrt, sc_extent, centre, w, h, dist=1e3):
    d = np.array([0.3, 0.45, 0.84]); d /= np.linalg.norm(d)
    right = np.cross(d, [0, 1, 0]); right /= np.linalg.norm(right); up = np.cross(right, d)
    half = 0.6 * sc_extent / (dist * sc_extent)
    cam = mrt.Camera()
    pos = np.asarray(centre) + d * dist * sc_extent
    cam.position = mrt.Float3(*pos); cam.forward = mrt.Float3(*(-d)); cam.right = mrt.Float3(*(right * half * w / h)); cam.up = mrt.Float3(*(up * half))
    return cam


WALKS = {      # render walk -> (scene options, renderer options)
    "tl_pairs1": ({}, {"tl_pairs": 1}),
    "tl_pairs0": ({}, {"tl_pairs": 0}),
    "rope": ({"rope": 1}, {"wide_bounce": 0, "primary_wide": 0}),
}


def render_parity(mrt, orc, ctx, sc, cam, two, walk, w=96, h=64):
    """one walk's 2-frame, 3-bounce image and ray counts against the oracle, bit for bit"""
    osc = _oracle(orc, mrt, sc, two)
    ref = orc.OracleRenderer(osc, w, h, seed=1, max_bounces=3, camera=cam); ref.render(2)
    sopt, ropt = WALKS[walk]
    sc.camera = cam
    with mrt.Renderer((w, h), sc, ctx=ctx, max_bounces=3, seed=1, scene_options={**({"instancing": 1} if two else {}), **sopt}) as r:
        for k, v in ropt.items():
            r.set_option(k, v)
        r.set_camera(cam)
        r.draw(2, wait=True)
        assert_parity(r.accumulation(), ref.accumulation(), exact_frac=1.0)
        assert (r.stats.closest_rays, r.stats.shadow_rays) == ref.counters(), walk
    osc.close()


# ------------------------------------------------------------------------------------------------ tests
SCENES = {
    "axis": lambda mrt: axis_scene(mrt, (96, 64)),
    "axis_far": lambda mrt: axis_scene(mrt, (96, 64), offset=FAR),
    "axis_tiny": lambda mrt: axis_scene(mrt, (96, 64), scale=1e-4),
    "stadium": lambda mrt: stadium_scene(mrt, (96, 64)),
    "stadium_far": lambda mrt: stadium_scene(mrt, (96, 64), offset=FAR),
}
MARGINS = {}

# Probes that still find lost hits in the box tests of the query kernels (known gaps, kept visible: strict, so each flips to a failure once fixed).
# The recorded ray is the first one that differs; the cause is described in the module docstring.
FAR_RAY = "rays 1e3 ... 1e4 units away lose hits to the box tests (their triangle test errs with the distance; the pads do not): "
KNOWN = {
    ("axis_tiny", "far"): FAR_RAY + "ray (3685.81, 1612.94, -0.6017) dir (-0.9161, -0.4009, 1.495e-4): no hit, brute force hits id 12 at 4023.277",
    ("stadium", "far"): FAR_RAY + "ray (4861.18, -0.1059, 6777.31) dir (-0.6004, 7.12e-5, -0.7997): no hit, brute force hits mesh 151 at 9725.108",
    ("stadium", "edge"): "any-hit limit one float past the hit: ray (0.17546, 3.59658, 5.71664) dir (0.004146, -0.42732, -0.90409) limit 6.645884 reports no hit",
    ("refit0", "far"): FAR_RAY + "ray (-3.1147, 1177.49, 1522.51) dir (0.001472, -0.61172, -0.79107): hit at 1923.7228, brute force 1923.6761",
    ("refit0", "edge"): "any-hit limit one float past the hit: ray (-3.30503, 0.246261, 1.31030) dir (0.85078, 0.20987, -0.48179) limit 2.3702846 reports no hit",
    ("refit1", "edge"): "any-hit limit one float past the hit: ray (-1.23728, -0.395237, 0.666638) dir (0.82203, 0.21248, -0.52832) limit 2.9268341 reports no hit",
    ("two_level_built", "near"): "near-parallel ray (-1.46991, -1.00073, 8.31616) dir (0.53583, 2.669e-4, -0.84432) at the identity sphere: hit at 2.7432141, per-instance brute force 2.7432005",
    ("two_level_built", "far"): FAR_RAY + "ray (-1868.75, -1.17448, 1025.53) dir (0.87785, 8.196e-5, -0.47893): hit at 2128.7651, brute force 2128.7632",
    ("two_level_built", "edge"): "as two_level_built near: ray (-1.46991, -1.00073, 8.31616) takes a farther triangle",
    ("two_level_updated", "near"): "axis-aligned ray (-22480.98, -22481.51, 16.9126) dir (0.70711, 0.70711, 0): no hit, per-instance brute force hits instance 20 at 31789.1",
    ("two_level_updated", "far"): FAR_RAY + "ray (-508.105, -1660.58, -239.337) dir (0.28995, 0.94675, 0.13998): hit at 1752.7981, brute force 1752.7979",
    ("two_level_updated", "edge"): "as two_level_updated near: ray (-22480.98, -22481.51, 16.9126) finds no hit",
    ("image_two_level", "tl_pairs1"): "two-level telephoto image from 1.2e4 units: rmse 4.8e-3 against the oracle",
    ("image_two_level", "tl_pairs0"): "two-level telephoto image from 1.2e4 units: rmse 4.8e-3 against the oracle",
    ("image_two_level", "rope"): "two-level telephoto image from 1.2e4 units: rmse 4.8e-3 against the oracle",
}


def _known(*key):
    why = KNOWN.get(key)
    return [pytest.mark.xfail(strict=True, raises=AssertionError, reason=why)] if why else []


def _walls(scene):
    off = FAR if "far" in scene else np.zeros(3)
    s = 1e-4 if "tiny" in scene else 1.0
    return [np.float32(off[0] + s * np.array([1.0, -1.0])), np.float32(off[1] + s * np.array([0.0, 0.5])), np.float32(off[2] + s * np.array([-1.0]))]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_every_box_encloses_its_triangles(mrt, gpu_ctx, scene):
    """every builder x leaf size x pre-split setting: the exact audit, zero-margin containment and half a pad to spare"""
    sc = SCENES[scene](mrt)
    T = sc.triangleCount
    split = {}
    for b in BUILDS:
        ds = mrt.DeviceScene(gpu_ctx, sc, _opts(b))
        try:
            rep, _ = _audit(ds, presplit=b["presplit"] is None, num_tris=T)
        except AssertionError as e:
            raise AssertionError(f"{scene} {b}: {e}") from None
        if b["presplit"] is None:
            split[b["builder"], b["max_leaf"]] = rep.counts["split_triangles"]
        MARGINS[(scene, str(b))] = (rep.summary(), rep.counts.get("split_triangles", 0))
        ds.close()
    print(scene, {k: v for k, v in MARGINS.items() if k[0] == scene}, "pre-split triangles per (builder, max_leaf):", split)


def _probe_scene(mrt, orc, gpu_ctx, scene):
    sc = SCENES[scene](mrt)
    wide = mrt.DeviceScene(gpu_ctx, sc, {"max_leaf": 1})
    rope = mrt.DeviceScene(gpu_ctx, sc, {"max_leaf": 1, "wide": 0})
    rep, lay = _audit(wide, presplit=True, num_tris=sc.triangleCount)
    D = A.decode_nodes(lay["wnodes"]); occ = (D["qlo"][0] <= D["qhi"][0]).all(1)
    ext = float((D["hi"][0][occ].max(0) - D["lo"][0][occ].min(0)).max())
    return sc, wide, rope, rep, lay, ext, _oracle(orc, mrt, sc, False)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_rays_at_the_tightest_planes(mrt, orc, gpu_ctx, scene):
    """rays from 1e-4 ... 1e-2 extents and 1 ... 10 units aimed at the planes the audit found tightest, and axis-aligned rays on decoded planes
    and walls: 8-wide and rope builds against the oracle's brute force, bit for bit"""
    rng = np.random.default_rng(11)
    sc, wide, rope, rep, lay, ext, osc = _probe_scene(mrt, orc, gpu_ctx, scene)
    rays = thin_rays(rep, lay, ext, rng, k=1500)
    hits = _compare([("wide", wide), ("rope", rope)], osc, rays, f"{scene} thin")
    ar = axis_rays(lay, _walls(scene), rng)
    hits_a = _compare([("wide", wide), ("rope", rope)], osc, ar, f"{scene} axis")
    hits_l = _compare([("wide", wide), ("rope", rope)], osc, _limited(ar, rng), f"{scene} axis limited")
    print(f"{scene}: thin rays {len(rays)} hit {hits}; axis rays {len(ar)} hit {hits_a}, limited {hits_l}")
    assert hits > 0.05 * len(rays)
    osc.close(); wide.close(); rope.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,probe", [pytest.param(s, p, marks=_known(s, p)) for s in SCENES for p in ("far", "edge")])
def test_far_rays_and_tight_any_hit_limits(mrt, orc, gpu_ctx, scene, probe):
    """far: rays from 1e3 ... 1e4 units at the tightest planes; edge: any-hit limits one float past the closest hit (thin and axis-aligned rays)"""
    rng = np.random.default_rng(13)
    sc, wide, rope, rep, lay, ext, osc = _probe_scene(mrt, orc, gpu_ctx, scene)
    try:
        if probe == "far":
            rays = thin_rays(rep, lay, ext, rng, k=1500, ranges=("far",))
            hits = _compare([("wide", wide), ("rope", rope)], osc, rays, f"{scene} far", edge=False)
        else:
            rays = np.vstack([thin_rays(rep, lay, ext, rng, k=1500), axis_rays(lay, _walls(scene), rng)])
            hits = _compare([("wide", wide), ("rope", rope)], osc, rays, f"{scene} edge", edge=True)
        print(f"{scene} {probe}: rays {len(rays)} hit {hits}")
    finally:
        osc.close(); wide.close(); rope.close()


@pytest.mark.gpu
@pytest.mark.parametrize("instancing,probe", [pytest.param(i, p, marks=_known(f"refit{i}", p)) for i in (0, 1) for p in ("near", "far", "edge")])
def test_three_refits_keep_every_box(mrt, orc, gpu_ctx, instancing, probe):
    """a 19 602-triangle sheet displaced by up to 20 % of its extent three times, some vertices pushed past the old root box: the audit after each
    refit, then rays at the tightest planes (near: 1e-4 ... 1e-2 extents and 1 ... 10 units; far: 1e3 ... 1e4; edge: any-hit limits one float past
    the hit) against the brute force"""
    X, Z = np.eye(3)[0], np.eye(3)[2]
    pos, idx = _quad((0, 0, 0), X, Z, 99)
    rng = np.random.default_rng(3)
    sc = _Scene(mrt, (96, 64), [("sheet", pos, idx, (0, 0.5, 0), 1.0), ("cube", *_cube((0, 0, 0), 0.2), (1.5, 0.3, 0), 1.0)])
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": instancing})
    _audit(ds, presplit=not instancing, num_tris=sc.triangleCount)
    p = pos.astype(np.float64)
    for k in range(3):
        q = p + rng.uniform(-0.2, 0.2, p.shape) * 2.0 * rng.random((len(p), 1))
        out = rng.random(len(p)) < 0.01
        q[out] *= 1.25                                                        # past the old root box
        q = q.astype(np.float32)
        nrm = np.tile(np.float32([0, 1, 0]), (len(q), 1))
        ds.update_mesh(0, q, nrm); ds.commit()
        assert ds.refits == k + 1
        rep, lay = _audit(ds, presplit=not instancing, num_tris=sc.triangleCount)
        sc.models[0].meshes[0].positions = q; sc.models[0].meshes[0].normals = nrm
    osc = _oracle(orc, mrt, sc, bool(instancing))
    try:
        rays = thin_rays(rep, lay, 3.0, rng, k=500, ranges=("far",) if probe == "far" else ("shadow", "mid"))
        _compare([("refit", ds)], osc, rays, f"refit instancing={instancing} {probe}", edge=probe == "edge")
    finally:
        osc.close(); ds.close()


def _two_level_pair(mrt, gpu_ctx, sc):
    return mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1}), mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1, "wide": 0})


def _update_all_transforms(sc, scenes):
    """every instance turned and moved a little: a TLAS-only update of each scene"""
    for i, m in enumerate(sc.meshes):
        A3 = np.asarray(m.transform, np.float64)[:3, :3].T @ _rot(0.05 * i, -0.03 * i, 0.02)
        t = np.asarray(m.transform, np.float64)[3, :3] + [0.1, -0.2, 0.05 * i]
        m.transform = _xf(A3, t)
        for ds in scenes:
            ds.set_instance_transform(i, m.transform)
    for ds in scenes:
        ds.commit()


@pytest.mark.gpu
def test_two_level_boxes_under_hostile_transforms(mrt, gpu_ctx):
    """cube, sphere and fan under eight transforms: the audit including the TLAS and the instance boxes, then every transform changed (TLAS-only
    update) and audited again"""
    sc = two_level_scene(mrt, (96, 64))
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    rep, _ = _audit(ds, presplit=False)
    print("two-level margins", rep.summary())
    _update_all_transforms(sc, [ds])
    rep, _ = _audit(ds, presplit=False)
    print("two-level margins after the TLAS update", rep.summary())
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("phase,probe", [pytest.param(ph, p, marks=_known("two_level_" + ph, p)) for ph in ("built", "updated") for p in ("near", "far", "edge")])
def test_two_level_rays_at_the_tightest_planes(mrt, orc, gpu_ctx, phase, probe):
    """the eight-transform scene (as built, and after a TLAS-only update): rays at the tightest BLAS planes taken into world space by their instance,
    and axis-aligned rays on the TLAS planes; 8-wide (query and stream) and wide = 0 builds against the per-instance brute force, bit for bit"""
    sc = two_level_scene(mrt, (96, 64))
    ds, rope = _two_level_pair(mrt, gpu_ctx, sc)
    if phase == "updated":
        _update_all_transforms(sc, [ds, rope])
    rep, lay = _audit(ds, presplit=False)
    rng = np.random.default_rng(19)
    osc = _oracle(orc, mrt, sc, True)
    try:
        rays = thin_rays(rep, lay, 3.0, rng, k=300, ranges=("far",) if probe == "far" else ("shadow", "mid"))
        if probe != "far":
            rays = np.vstack([rays, axis_rays(lay, [[], [], []], rng, n=1000)])
        hits = _compare([("wide", ds), ("rope", rope)], osc, rays, f"two-level {phase} {probe}", edge=probe == "edge")
        print(f"two-level {phase} {probe}: rays {len(rays)} hit {hits}")
    finally:
        osc.close(); ds.close(); rope.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,walk", [pytest.param(s, w, marks=_known("image_" + s, w)) for s in ("two_level", "stadium") for w in WALKS if s == "two_level" or w != "tl_pairs0"])
def test_far_telephoto_images(mrt, orc, gpu_ctx, scene, walk):
    """96 x 64, 2 frames, 3 bounces from ~1e3 extents away, forward long against right and up: every walk against the oracle bit for bit, ray counts
    included (the stadium is flattened: tl_pairs does not apply)"""
    if scene == "two_level":
        sc = two_level_scene(mrt, (96, 64))
        cam = telephoto(mrt, 12.0, (0, 0, 3), 96, 64)
    else:
        sc = stadium_scene(mrt, (96, 64))
        cam = telephoto(mrt, 2e3, (0, 0, 0), 96, 64)
    sc.lights = [mrt.Light.sunLight([-0.3, -1.0, -0.2], [3, 3, 3]), mrt.Light.pointLight([0.5, 3.0, 2.0], [20, 20, 20])]
    render_parity(mrt, orc, gpu_ctx, sc, cam, scene == "two_level", walk)


@pytest.mark.gpu
@pytest.mark.parametrize("keys", ["coincident", "clustered"])
def test_builder0_depth_on_degenerate_keys(mrt, orc, gpu_ctx, keys):
    """builder = 0 over 4096 coincident triangles (one Morton key), and over 4096 triangles in 64 clusters 1e-6 wide at wildly different scales of
    the scene: the depth it reaches, the audit, and an image against the oracle"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32) + [-0.5, 0.3, -0.2]
    if keys == "coincident":
        pos = np.tile(tri, (4096, 1))
    else:
        rng = np.random.default_rng(23)
        centres = np.r_[[[-0.5, 0.3, -0.2]], rng.uniform(-1, 1, (63, 3)) * 10.0 ** rng.uniform(-6, 0, (63, 1))]
        c = np.repeat(centres, 64, 0) + rng.normal(size=(4096, 3)) * 1e-6
        pos = (c[:, None, :] + np.array([[0, 0, 0], [0.3, 0, 0], [0, 0.3, 0]])[None]).reshape(-1, 3).astype(np.float32)
    idx = np.arange(3 * 4096, dtype=np.uint32).reshape(-1, 3)
    sc = _Scene(mrt, (64, 48), [("dups", pos, idx, (0, 0, 0), 1.0)])
    ds = mrt.DeviceScene(gpu_ctx, sc, {"builder": 0, "max_leaf": 1})
    rep, _ = _audit(ds, presplit=True, num_tris=4096)
    print(f"builder 0 over 4096 {keys} triangles: wide_depth", ds.stats.wide_depth, "real depth", rep.depth)
    ds.close()
    osc = _oracle(orc, mrt, sc, False)
    ref = orc.OracleRenderer(osc, 64, 48, seed=1, max_bounces=2, camera=sc.camera); ref.render(1)
    with mrt.Renderer((64, 48), sc, ctx=gpu_ctx, max_bounces=2, seed=1, scene_options={"builder": 0, "max_leaf": 1}) as r:
        r.draw(1, wait=True)
        assert_parity(r.accumulation(), ref.accumulation(), exact_frac=1.0)
    osc.close()
