"""The ray families of tests/special_rays.py — axis-parallel directions with both zero signs, denormal and clamp-sized components, origins on vertex coordinates and in
the floor's plane, intervals that end on the hit, instances that turn a +0 into a -0 — through every entry that takes caller rays, on the flattened 8-wide layout, on
a two-level scene and on a scene without the 8-wide layout; and renders whose shadow rays are made of such directions (a sun straight overhead).  Every field of every
record must have the bits of the oracle's brute force, and on the rays float64 can decide also match tests/f64_reference.py within test_independent_f64.py's figures.
tests/test_special_rays_cpu.py checks the reference side and the preconditions without a GPU.

What this found (docs/HISTORY.md §21): the 8-wide node test took the near / far planes by `d < 0`, which is false for -0, and the reciprocal from copysign, which is
-1e20 for -0: every ray with a -0 direction component missed everything on the 8-wide layouts."""
import numpy as np
import pytest

import special_rays as S
from test_query_device import LAYOUTS
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

FAMILIES = ("F1", "F2", "F3", "F4")
TWO_LEVEL = {"two_level": {"instancing": 1}, "two_level_rope": {"instancing": 1, "wide": 0}}
TMIN_INERT = np.float32(1e-30)          # a positive min_distance that changes nothing (asserted on the oracle): it only sends the ray to the one-ray-per-lane kernel
ALL_ONES = 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(got, want, what, tags):
    for f in S.FIELDS:
        bad = np.flatnonzero(_bits(got[f]) != _bits(want[f]))
        assert len(bad) == 0, f"{what} {f}: {len(bad)} of {len(want)} records differ from the oracle's brute force, first {bad[0]} ({tags[bad[0]]}): {got[bad[0]]} != {want[bad[0]]}"


def _records(mrt, t):
    return t.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(t.shape[:-1])


def _subset(j, idx):
    return {k: v[idx] for k, v in j.items()}


class _Family:
    """one family of one case, or the part `idx` of it: rays, tags and the three reference answers side by side"""
    def __init__(self, c, name, idx=None):
        fam = c.families[name]
        idx = np.arange(len(fam.rays)) if idx is None else idx
        self.c, self.name, self.idx, self.rays, self.tags = c, name, idx, np.array(fam.rays[idx]), fam.tags[idx]
        self.closest, self.occluded, self.judged = c.closest[name][idx], c.occluded[name][idx], _subset(c.judged[name], idx)
        self.may_judge = S.judged_mask(name, fam)[idx]

    def check_closest(self, rec, what):
        _assert_bits(rec, self.closest, f"{what} {self.name}", self.tags)
        S.assert_matches_f64(self.c.tris, self.judged, rec, f"{what} {self.name}", self.may_judge)

    def check_any(self, occ, what):
        bad = np.flatnonzero(np.asarray(occ) != self.occluded)
        assert len(bad) == 0, f"{what} {self.name}: {len(bad)} any-hit answers differ from the oracle's brute force, first {bad[0]} ({self.tags[bad[0]]})"
        m = self.judged["decided"] & self.may_judge
        assert np.array_equal(np.asarray(occ)[m] == 1, self.judged["hit"][m]), f"{what} {self.name}: any-hit against float64"

    def without_min(self):
        """the rays the stream kernels can take (min_distance == 0): all, but of F4 the cases that need none"""
        if self.name != "F4": return self
        return _Family(self.c, self.name, np.flatnonzero(np.isin(self.c.families[self.name].tags, S.F4_NO_MIN)))

    def with_inert_min(self):
        """the same rays with min_distance = TMIN_INERT and, by the oracle's brute force, the same answers"""
        g = _Family(self.c, self.name, self.without_min().idx)
        g.rays[:, 3] = TMIN_INERT
        o = self.c.oracle.intersect_closest(g.rays, brute=True)
        for fld in S.FIELDS:
            assert np.array_equal(_bits(o[fld]), _bits(g.closest[fld])), "precondition: the inert min_distance changes no answer"
        return g


def _case_of(mrt, orc, layout, family):
    if family == "F5": return S.case_f5(mrt, orc)
    return S.case(mrt, orc, layout.startswith("two_level"))


def _options(layout):
    return {**LAYOUTS, **TWO_LEVEL}[layout]


def _cases():
    out = [(layout, fam) for layout in LAYOUTS for fam in FAMILIES]
    return out + [(layout, "F5") for layout in TWO_LEVEL]


@pytest.fixture(scope="module")
def scenes(mrt, gpu_ctx):
    """one DeviceScene per layout and scene for the whole module: never modified, closed at the end"""
    made = {}
    def get(layout, f5):
        if (layout, f5) not in made:
            sc = S.f5_scene(mrt) if f5 else S._scene(mrt, S.SIZE, S.SEED)
            made[layout, f5] = mrt.DeviceScene(gpu_ctx, sc, _options(layout))
            assert made[layout, f5].stats.wide_layout == (0 if "rope" in layout else 1)
        return made[layout, f5]
    yield get
    for ds in made.values(): ds.close()


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", ctx.device))


@pytest.mark.parametrize("layout,family", _cases())
def test_host_entries(mrt, orc, scenes, layout, family):
    """intersect_closest / intersect_any (one ray per lane, any interval) and intersect_stream (the render kernels' walk; min_distance 0)"""
    c = _case_of(mrt, orc, layout, family)
    ds = scenes(layout, family == "F5")
    f = _Family(c, family)
    f.check_closest(ds.intersect_closest(f.rays), f"{layout} intersect_closest")
    f.check_any(ds.intersect_any(f.rays), f"{layout} intersect_any")
    if ds.stats.wide_layout:
        z = f.without_min()
        z.check_closest(ds.intersect_stream(z.rays), f"{layout} intersect_stream")
        z.check_any(ds.intersect_stream(z.rays, any_hit=True)["type"], f"{layout} intersect_stream(any_hit)")
    if not layout.startswith("two_level"):          # the diagnostics walk (walk_wide / walk_rope with counters): the id of the hit it ends with
        st = ds.traversal_stats(f.rays)
        gid = np.where(f.closest["type"] == 1, _global_ids(c.tris, f.closest), 0xFFFFFFFF)
        assert np.array_equal(st[:, 3], gid.astype(np.uint32)), f"{layout} traversal_stats {family}"


def _global_ids(tris, rec):
    """(instance, geometry, primitive) -> the flattened scene's triangle number, which is tests/f64_reference.Triangles' row"""
    key = {tuple(r): k for k, r in enumerate(tris.ids.tolist())}
    return np.array([key.get((int(r["instance_id"]), int(r["geometry_id"]), int(r["primitive_id"])), 0xFFFFFFFF) for r in rec], np.int64)


@pytest.mark.parametrize("layout,family", _cases())
def test_device_entries(mrt, orc, gpu_ctx, scenes, layout, family):
    """intersect_closest_device / intersect_any_device: the family as it is (min_distance 0 takes the stream kernel on the 8-wide layouts; F4's positive ones the lane
    kernel, ray by ray), with a count word, with an all-ones mask, and once more with an inert positive min_distance on every ray (the lane kernel)"""
    import torch
    c = _case_of(mrt, orc, layout, family)
    ds = scenes(layout, family == "F5")
    f = _Family(c, family)
    for g, how in ((f, "as given"), (f.with_inert_min(), "inert min_distance")):
        d = _t(g.rays, gpu_ctx)
        word = torch.tensor([len(g.rays)], dtype=torch.int32, device=d.device)
        for kw, form in (({}, ""), ({"count": word}, " counted"), ({"mask": ALL_ONES}, " masked")):
            rc = ds.intersect_closest_device(d, **kw); ra = ds.intersect_any_device(d, **kw)
            torch.cuda.synchronize()
            g.check_closest(_records(mrt, rc), f"{layout} intersect_closest_device{form} ({how})")
            g.check_any(ra.cpu().numpy(), f"{layout} intersect_any_device{form} ({how})")
            assert (rc[:, 7] == 0).all().item()


@pytest.mark.parametrize("layout,family", [(l, f) for l, f in _cases() if not l.startswith("two_level")])          # intersect_all_device: flattened scenes (its docstring)
def test_all_hits_entry(mrt, orc, gpu_ctx, scenes, layout, family):
    """intersect_all_device, max_hits = 4, unmasked and with an all-ones mask: row 0 is the closest record, hit_counts > 0 is any-hit, every row ascends in (distance, id)"""
    import torch
    K = 4
    c = _case_of(mrt, orc, layout, family)
    ds = scenes(layout, False)
    f = _Family(c, family)
    d = _t(f.rays, gpu_ctx)
    for kw, form in (({}, ""), ({"mask": ALL_ONES}, " masked")):
        h, n = ds.intersect_all_device(d, K, **kw)
        torch.cuda.synchronize()
        rec, n = _records(mrt, h), n.cpu().numpy()
        what = f"{layout} intersect_all_device{form}"
        f.check_closest(np.ascontiguousarray(rec[:, 0]), what + " row 0")
        f.check_any((n > 0).astype(np.int32), what + " hit_counts > 0")
        assert ((rec["type"] == 1) == (np.arange(K)[None, :] < n[:, None])).all(), what + ": hit records first, then miss records"
        gid = np.stack([_global_ids(c.tris, rec[:, k]) for k in range(K)], 1)
        for k in range(K - 1):
            both = n > k + 1
            t0, t1 = rec["distance"][both, k], rec["distance"][both, k + 1]
            assert ((t0 < t1) | ((t0 == t1) & (gid[both, k] < gid[both, k + 1]))).all(), what + f": rows {k}, {k + 1} out of order"
        lo, hi = f.rays[:, 3], f.rays[:, 7]
        inside = (rec["distance"] >= lo[:, None]) & (rec["distance"] <= hi[:, None])
        assert inside[rec["type"] == 1].all(), what + ": a hit outside [min_distance, max_distance]"
    if family == "F1":          # precondition, by float64: the -0 rays have lists to order, not single hits
        assert (np.isfinite(f.judged["t2"]) & S.carries_neg_zero(f.rays)).sum() >= 300


# ---------------------------------------------------------------- renders
def _sun_scene(mrt, sun, sphere=True):
    class Sc(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="plane", position=[0, 0, 0], scale=10)] + ([mrt.Model(name="sphere", position=[0.3, 0.7, 0.2], scale=1.0)] if sphere else [])
            self.lights = [mrt.Light.sunLight(sun, [1.0, 0.9, 0.8])]
    return Sc(S.SIZE)


def _oracle_image(mrt, orc, sc, two_level, frames=2):
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=two_level), sc.lights, instancing=two_level)
    r = orc.OracleRenderer(osc, *S.SIZE, seed=1, max_bounces=3, camera=sc.camera)
    r.render(frames)
    img, cnt = r.accumulation().copy(), r.counters()
    r.close(); osc.close()
    return img, cnt


# scene options, renderer options.  A two-level scene of up to 64 instances takes its bounce and shadow rays through a TLAS pass without a tree (rope_box_hit per instance) by
# default; tl_pairs = 0 is the one loop over both levels, tl_pairs = 2 the TLAS pass as a walk of the 8-wide TLAS: the walks a larger scene gets.  megakernel = 1: one launch per
# frame (megakernel.h), flattened scenes only.
RENDERS = {"flat": (None, {}), "flat_megakernel": (None, {"megakernel": 1}), "rope": ({"wide": 0}, {}), "two_level": ({"instancing": 1}, {}), "two_level_one_loop": ({"instancing": 1}, {"tl_pairs": 0}),
           "two_level_tlas_walk": ({"instancing": 1}, {"tl_pairs": 2}), "two_level_rope": ({"instancing": 1, "wide": 0}, {})}


def _render(mrt, gpu_ctx, sc, how, frames=2):
    sopt, ropt = RENDERS[how]
    with mrt.Renderer(S.SIZE, sc, ctx=gpu_ctx, seed=1, max_bounces=3, scene_options=sopt) as r:
        assert r.device_scene.stats.wide_layout == (0 if "rope" in how else 1)
        for k, v in ropt.items(): r.set_option(k, v)
        r.draw(frames, wait=True)
        return r.accumulation().copy(), (r.stats.closest_rays, r.stats.shadow_rays)


@pytest.mark.parametrize("layout", list(RENDERS))
@pytest.mark.parametrize("sun", [(0.0, -1.0, 0.0), (0.3, -1.0, 0.0)], ids=["overhead", "tilted_in_xy"])
def test_sun_light_casts_its_shadow(mrt, orc, gpu_ctx, layout, sun):
    """eval_light negates the sun's direction: every shadow ray of sunLight([0, -1, 0]) is (-0, +1, -0), of sunLight([0.3, -1, 0]) (-0.29, +0.96, -0)"""
    two_level = layout.startswith("two_level")
    sc = _sun_scene(mrt, sun)
    ref, counters = _oracle_image(mrt, orc, sc, two_level)
    bare, _ = _oracle_image(mrt, orc, _sun_scene(mrt, sun, sphere=False), two_level)
    assert (_bits(ref) != _bits(bare)).any(-1).mean() >= 0.05, "precondition: the sphere and its shadow are in the picture"
    assert counters[1] > 100
    img, rays = _render(mrt, gpu_ctx, sc, layout)
    assert_parity(img, ref, exact_frac=1.0)
    assert rays == counters


@pytest.mark.parametrize("layout", [k for k in RENDERS if k.startswith("two_level")])
def test_render_of_the_rotated_instances(mrt, orc, gpu_ctx, layout):
    """a guard: F5's scene under a point light straight above it and a sun, through the renderer's own two-level walks"""
    lights = [mrt.Light.pointLight(position=[0.2, 3.0, 0.6], color=[8.0, 8.0, 8.0]), mrt.Light.sunLight([0.0, -1.0, 0.0], [0.6, 0.6, 0.6])]
    sc = S.f5_scene(mrt, lights=lights)
    ref, counters = _oracle_image(mrt, orc, sc, True)
    assert counters[1] > 100
    img, rays = _render(mrt, gpu_ctx, sc, layout)
    assert_parity(img, ref, exact_frac=1.0)
    assert rays == counters
