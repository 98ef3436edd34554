"""The tree figures that steer refits — MRTSceneStats.wide_cost / wide_cost_built, leaf_growth, sah_cost, bvh_nodes, bvh_leaves, max_depth, wide_depth, scene_bytes and
the 12 words of mrt_debug_wide_histogram — against tests/tree_stats_reference.py: every expected value is recounted from the layout the SAME DeviceScene dumps after the
same build or refit (nothing depends on which tree a builder chose or on how the nodes of a level are numbered).

Tolerances (derived in tree_stats_reference.py and DESIGN.md §10l, none taken from the library's output):
  emulation   wide_cost within 2 float32 ulp (the order of the float64 atomic additions may move the final rounding across a tie), leaf_growth after k chained
              refits within 2k ulp, sah_cost after a build bit-equal (k_refit's recurrence is deterministic given the emitted tree), integers equal;
  meaning     the exact float64 value within the bound the reference computes for that scene; for scenes with |coordinate| <= 8 that bound must stay below
              1e-3 relative, or the check says nothing (the scene offset by (1.3e4, -2.7e3, 7.1e3) is exempt from the cap, not from the bound).
Every test prints its margins ("MARGIN case figure ulp bound"): the table of DESIGN.md §10l."""
import math

import numpy as np
import pytest

import bvh_audit as A
import rope_audit as R
import tree_stats_reference as T
from test_build_sizes import _soup
from test_fuzz_geometry import _Raw, _fan, _sheets

pytestmark = pytest.mark.gpu

F32 = np.float32
CAP = 1e-3


# ------------------------------------------------------------------------------------------------ scenes under the identity
def _scene(mrt, meshes, extra=()):
    """meshes: [(name, positions, indices)], each one model under the identity transform: the world vertices are the input floats bit for bit"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [_Raw(mrt, name, pos, idx, (0.6, 0.6, 0.6), [0, 0, 0], [0, 0, 0], 1.0) for name, pos, idx in meshes]
            for name, src, position in extra:          # further instances of an earlier mesh (two-level scenes: the same BLAS)
                self.models.append(_Raw(mrt, name, None, None, None, position, [0, 0, 0], 1.0, share=self.models[src]))
    sc = S((64, 64))
    for m in sc.meshes[:len(meshes)]:
        assert np.array_equal(np.asarray(m.transform, np.float64), np.eye(4)), "the identity, exactly"
    return sc


def _layout(ds):
    hdr = ds.read_layout("header")
    lay = dict(header=hdr, wnodes=ds.read_layout("wnodes"), rope_nodes=ds.read_layout("rope_nodes"), rope_packets=ds.read_layout("rope_packets"))
    lay["wpackets"] = ds.read_layout("wpackets") if hdr[0] else np.zeros((0, 12), np.uint32)
    if hdr[2]:
        lay["instances"] = ds.read_layout("instances"); lay["tlas_nodes"] = ds.read_layout("tlas_nodes")
    return lay


def _histogram(mrt, ds):
    out = np.zeros(12, np.uint32)
    mrt._ffi.check(mrt.lib.mrt_debug_wide_histogram(ds.handle, mrt._ffi.ptr(out)))
    return out


def _bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


def _finite(st):
    for f in ("wide_cost", "wide_cost_built", "leaf_growth", "sah_cost"):
        assert math.isfinite(getattr(st, f)), f


def _margin(case, figure, ulp, bound_rel=None):
    print(f"MARGIN {case} {figure} ulp={ulp}" + ("" if bound_rel is None else f" bound={bound_rel:.2e}"))


def _check_cost(case, st_cost, cost, near, ulps=2):
    """a reported wide_cost against the reference's Cost: emulation within `ulps`, meaning within the scene's own bound (capped for scenes near the origin)"""
    u = T.ulps32(st_cost, cost.emu)
    rel = cost.bound / cost.exact if cost.exact > 0 else 0.0
    _margin(case, "wide_cost", u, rel)
    assert u <= ulps, (case, st_cost, cost.emu)
    assert abs(float(st_cost) - cost.exact) <= cost.bound, (case, st_cost, cost.exact, cost.bound)
    assert (not near) or rel < CAP, (case, rel)


def _check_build(mrt, case, ds, opts, triangles, vertices, near=True, instances=1):
    """every figure of a flattened scene after a BUILD"""
    st, lay = ds.stats, _layout(ds)
    hdr = lay["header"].astype(np.int64)
    wide = opts.get("wide", 1) != 0
    rope = (not wide) or opts.get("rope", 0) == 1
    _finite(st)
    assert (st.triangles, st.vertices, st.instances, st.refits) == (triangles, vertices, instances, 0)
    assert st.wide_layout == (1 if wide else 0) and (hdr[0] > 0) == wide and hdr[2] == 0
    assert st.max_leaf_tris == 4, "scene option max_leaf as it stands (scene_device.h)"
    assert st.leaf_growth == 1.0 and st.wide_cost == st.wide_cost_built
    cost, _ = T.scene_wide_cost(lay)
    hist = _histogram(mrt, ds)
    assert np.array_equal(hist, T.histogram(lay["wnodes"])), (hist, T.histogram(lay["wnodes"]))
    refs = int(hdr[4]) if wide else len(lay["rope_packets"])
    assert refs >= triangles
    if wide:
        _check_cost(case, st.wide_cost, cost, near)
        assert st.wide_cost > 0
        assert st.wide_depth == T.wide_depth(lay) == hdr[3], "the LDS stack is sized from it: 320 B per wave and level it overstates"
        assert st.bvh_nodes == hdr[0] and st.max_depth == st.wide_depth, "with the 8-wide layout: its nodes and its levels"
        assert hist[11] == refs and hist[:9].sum() == hdr[0] and hist[9] == hdr[0] - 1, "references; every node but the root is some node's internal child"
        assert 1 <= st.bvh_leaves <= refs and st.sah_cost > 0
    else:
        assert st.wide_cost == 0 and st.wide_depth == 0 and not hist.any()
    assert (len(lay["rope_nodes"]) > 0) == rope
    if rope:
        b = T.binary_figures(lay["rope_nodes"], 1.0, 1.0, st.max_leaf_tris)
        assert not b.violations, b.violations
        assert b.nodes == len(lay["rope_nodes"]) and len(lay["rope_packets"]) == refs
        assert st.bvh_leaves == b.leaves and b.largest_leaf <= st.max_leaf_tris
        assert _bits(st.sah_cost) == _bits(b.sah32), (case, st.sah_cost, b.sah32)
        rel = abs(float(st.sah_cost) / b.sah64 - 1)
        _margin(case, "sah_cost", 0, (b.depth + 3) * 2.0 ** -23)
        assert rel <= (b.depth + 3) * 2.0 ** -23, "a sum of non-negative terms, one rounding per level, the area's and the division's"
        if not wide:
            assert st.bvh_nodes == b.nodes and st.max_depth == b.depth, "without the 8-wide layout: the binary tree's nodes and its depth in edges"
    assert st.scene_bytes == T.scene_bytes(hdr, st, len(lay["rope_nodes"]), len(lay["rope_packets"]))
    return st, lay


OPTIONS = {"default": {}, "rope": {"rope": 1}, "binary": {"wide": 0}}


@pytest.mark.parametrize("n", [1, 2, 9, 65, 1025, 3000])
@pytest.mark.parametrize("layout", list(OPTIONS))
@pytest.mark.parametrize("builder", [0, 1, 2])
def test_flat_build(mrt, gpu_ctx, builder, layout, n):
    """1, 2, 9: one node with empty slots; 65: not a multiple of a wave; 1025: three waves of k_wide_cost's workgroup (256 threads) and a level of more than 64 nodes;
    3000: two workgroups"""
    pos, idx = _soup(np.random.default_rng(31 * n + builder), n)
    opts = dict(OPTIONS[layout], builder=builder)
    ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("soup", pos, idx)]), opts)
    st, lay = _check_build(mrt, f"flat/b{builder}/{layout}/{n}", ds, opts, n, 3 * n)
    if layout != "binary" and n >= 1025:          # (the shapes this test is about, not figures of the library: 1025 fills more than two waves of k_wide_cost, 3000 more than one workgroup)
        widest = max(len(lv) for lv in T.wide_levels(A.decode_nodes(lay["wnodes"]), 0))
        assert lay["header"][0] > (256 if n == 3000 else 128) and widest > 64, (lay["header"][0], widest)
    ds.close()


def _slivers():
    """the pre-split scene of test_build_sizes.test_presplit_build_at_the_tail_boundary"""
    pos, idx = _soup(np.random.default_rng(5), 1000)
    tri = pos.reshape(-1, 3, 3)
    tri[::9, 1] = tri[::9, 0] + [2.5, 0.0, 0.01]
    tri[::9, 2] = tri[::9, 0] + [0.0, 0.02, 0.0]
    return tri.reshape(-1, 3).astype(np.float32), idx


def _edge(name):
    if name == "sheet":          # coplanar and axis-aligned: one extent is the pad alone, everywhere
        pos, idx = _sheets(12)
        return pos, idx, {}, True
    if name == "point":          # every triangle the same point: the root's area is at its minimum, two pads a side
        pos = np.tile(np.array([[0.001, -0.002, 0.0005]], np.float32), (60, 1))
        return pos, np.arange(60, dtype=np.uint32).reshape(-1, 3), {}, True
    if name.startswith("slivers"):
        pos, idx = _slivers()
        return pos, idx, {"presplit": int(name[7:])}, True
    pos, idx = _soup(np.random.default_rng(77), 700)          # "far": float32 plane decoding at its coarsest
    return (pos + np.array([1.3e4, -2.7e3, 7.1e3], np.float32)).astype(np.float32), idx, {}, False


@pytest.mark.parametrize("layout", ["default", "rope"])
@pytest.mark.parametrize("name", ["sheet", "point", "slivers0", "slivers4", "far"])
def test_edge_geometry(mrt, gpu_ctx, name, layout):
    pos, idx, opts, near = _edge(name)
    opts = dict(opts, **OPTIONS[layout])
    ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [(name, pos, idx)]), opts)
    st, lay = _check_build(mrt, f"edge/{name}/{layout}", ds, opts, len(idx), len(pos), near=near)
    assert st.wide_cost > 1.0 and st.sah_cost > 0, "0 only for a root without area (wide_tree_cost, finish_tree): the pads give every box one"
    if name == "slivers4":
        assert lay["header"][4] > len(idx), "pre-splitting made references"
    if name == "slivers0":
        assert lay["header"][4] == len(idx)
    if name == "far":
        cost, _ = T.scene_wide_cost(lay)
        print(f"MARGIN edge/far/{layout} emulation-against-meaning ulp={T.ulps32(cost.emu, F32(cost.exact))}")
    ds.close()


# ------------------------------------------------------------------------------------------------ flat refits
def _moved(pos, step):
    pos = np.asarray(pos, np.float32)
    return (pos + np.float32(0.05) * np.sin(7.0 * pos[:, [2, 0, 1]] + step)).astype(np.float32)


def _two_meshes(seed=11):
    rng = np.random.default_rng(seed)
    fan = _fan(rng, 300)
    soup = _soup(rng, 900)
    return [("fan", *fan), ("soup", *soup)]


def _boxes(meshes, new=None):
    """k_flatten's padded boxes of every triangle of the flattened scene, by global triangle id (meshes in order; one submesh each), and the mesh of every triangle"""
    tri = np.concatenate([np.asarray((new or {}).get(k, pos), F32)[idx.astype(np.int64)] for k, (_, pos, idx) in enumerate(meshes)])
    owner = np.concatenate([np.full(len(idx), k) for k, (_, pos, idx) in enumerate(meshes)])
    lo, hi = T.padded_boxes(tri)
    return lo, hi, owner


def _t(a, gpu_ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.device("cuda", gpu_ctx.device))


def _deform(ds, gpu_ctx, mesh_id, pos, nrm, device):
    if device:
        import torch
        ds.update_mesh_device(mesh_id, _t(pos, gpu_ctx), _t(nrm, gpu_ctx)); ds.refit_device()
        torch.cuda.synchronize()
    else:
        ds.update_mesh(mesh_id, pos, nrm); ds.commit()


def _check_refit(case, ds, st0, lay_before, meshes, new, moved_meshes, prev, steps, near=True):
    """the figures after one refit of a flattened scene with the 8-wide layout; returns the stats, the layout and the reference's chained leaf_growth"""
    st, lay = ds.stats, _layout(ds)
    _finite(st)
    assert st.refits == steps and ds.refits == steps
    cost, _ = T.scene_wide_cost(lay)
    _check_cost(case, st.wide_cost, cost, near)
    assert st.wide_cost_built == st0.wide_cost_built
    assert _bits(st.sah_cost) == _bits(F32(st0.sah_cost) * (F32(st.wide_cost) / F32(st.wide_cost_built))), "the build's figure scaled by wide_cost / wide_cost_built in float32"
    lo, hi, owner = _boxes(meshes, new)
    g = T.leaf_growth(lay_before["wnodes"], lay["wnodes"], lay["wpackets"][:, 3], lo, hi, np.isin(owner, list(moved_meshes)), previous=prev)
    u = T.ulps32(st.leaf_growth, g.emu)
    _margin(case, "leaf_growth", u, g.rel_bound)
    assert u <= 2 * steps, (case, st.leaf_growth, g.emu)
    assert abs(float(g.ratio32) / g.ratio_exact - 1) <= g.rel_bound and ((not near) or g.rel_bound < CAP), (g.ratio32, g.ratio_exact, g.rel_bound)
    for f in ("bvh_nodes", "bvh_leaves", "max_depth", "wide_depth", "scene_bytes", "wide_layout", "max_leaf_tris"):
        assert getattr(st, f) == getattr(st0, f), f
    assert st.wide_depth == T.wide_depth(lay)
    return st, lay, g


@pytest.mark.parametrize("device", [False, True], ids=["commit", "stream"])
@pytest.mark.parametrize("layout", ["default", "rope"])
def test_flat_refit_chain(mrt, gpu_ctx, layout, device):
    """two deformations of the fan beside a soup that stays: only the fan's leaves enter the growth sums, the second step chains on the first"""
    meshes = _two_meshes()
    sc = _scene(mrt, meshes)
    nrm = [m.normals for m in sc.meshes]
    ds = mrt.DeviceScene(gpu_ctx, sc, OPTIONS[layout])
    case = f"refit/{layout}/{'stream' if device else 'commit'}"
    st0, lay = _check_build(mrt, case + "/build", ds, OPTIONS[layout], 1200, 301 + 2700, instances=2)
    prev, lay_build = F32(1), lay
    for step in range(2):
        new = {0: _moved(meshes[0][1], step)}
        _deform(ds, gpu_ctx, 0, new[0], nrm[0], device)
        st_b, lay_next, g = _check_refit(f"{case}/{step}", ds, st0, lay, meshes, new, {0}, prev, step + 1)
        assert g.emu > 1.0, "the deformation loosens the fan's leaves"
        # the wrong moved set — the soup's unmoved leaves counted too — is another number: the library agrees with the right one only
        lo, hi, owner = _boxes(meshes, new)
        wrong = T.leaf_growth(lay["wnodes"], lay_next["wnodes"], lay_next["wpackets"][:, 3], lo, hi, np.ones(1200, bool), previous=prev)
        assert T.ulps32(wrong.emu, st_b.leaf_growth) > 1000 and wrong.slots > g.slots
        n, bad, _ = T.unmoved_leaf_excess(lay["wnodes"], lay_next["wnodes"], lay_next["wpackets"][:, 3], lo, hi, owner == 0)
        assert n > 0 and not bad, bad
        prev, lay = g.emu, lay_next
    if layout == "rope":
        R.links_kept(lay_build, lay).check()
    ds.close()


@pytest.mark.parametrize("device", [False, True], ids=["commit", "stream"])
def test_refit_with_unchanged_vertices(mrt, gpu_ctx, device):
    meshes = _two_meshes(12)
    sc = _scene(mrt, meshes)
    ds = mrt.DeviceScene(gpu_ctx, sc, {})
    st0, lay0 = ds.stats, _layout(ds)
    _deform(ds, gpu_ctx, 0, meshes[0][1], sc.meshes[0].normals, device)
    st, lay = ds.stats, _layout(ds)
    assert st.refits == 1
    assert st.leaf_growth == 1.0, "every leaf of the fan has the box it had"
    assert _bits(st.wide_cost) == _bits(st0.wide_cost) and _bits(st.sah_cost) == _bits(st0.sah_cost)
    g = T.leaf_growth(lay0["wnodes"], lay["wnodes"], lay["wpackets"][:, 3], *_boxes(meshes)[:2], _boxes(meshes)[2] == 0)
    assert g.emu == 1.0 and g.g_old == g.g_new > 0 and g.slots > 0
    ds.close()


def test_refit_beside_a_presplit_wall(mrt, gpu_ctx):
    """the slivers (pre-split: several clipped references each) stay, the fan beside them moves: the unmoved clipped leaves keep their boxes and stay out of the sums"""
    rng = np.random.default_rng(21)
    meshes = [("slivers", *_slivers()), ("fan", *_fan(rng, 300))]
    sc = _scene(mrt, meshes)
    ds = mrt.DeviceScene(gpu_ctx, sc, {"presplit": 4})
    st0, lay0 = _check_build(mrt, "refit/presplit/build", ds, {"presplit": 4}, 1300, 3000 + 301, instances=2)
    assert lay0["header"][4] > 1300
    new = {1: _moved(meshes[1][1], 0)}
    _deform(ds, gpu_ctx, 1, new[1], sc.meshes[1].normals, False)
    st, lay, g = _check_refit("refit/presplit/0", ds, st0, lay0, meshes, new, {1}, F32(1), 1)
    lo, hi, owner = _boxes(meshes, new)
    n, bad, clipped = T.unmoved_leaf_excess(lay0["wnodes"], lay["wnodes"], lay["wpackets"][:, 3], lo, hi, owner == 1)
    assert n > 0 and not bad, bad
    assert clipped > 50, "leaves whose box is smaller than their triangles': the clipped references"
    ds.close()


def test_refit_of_the_binary_layout_alone(mrt, gpu_ctx):
    """wide = 0: the figures of the 8-wide layout stay what the header says of a scene without it — cost 0, growth 1 — and sah_cost the build's"""
    meshes = _two_meshes(13)
    sc = _scene(mrt, meshes)
    ds = mrt.DeviceScene(gpu_ctx, sc, {"wide": 0})
    st0, lay0 = _check_build(mrt, "refit/binary/build", ds, {"wide": 0}, 1200, 3001, instances=2)
    _deform(ds, gpu_ctx, 0, _moved(meshes[0][1], 0), sc.meshes[0].normals, False)
    st = ds.stats
    assert st.refits == 1 and st.leaf_growth == 1.0 and st.wide_cost == 0 and st.wide_cost_built == 0
    assert _bits(st.sah_cost) == _bits(st0.sah_cost) and (st.bvh_nodes, st.bvh_leaves, st.max_depth) == (st0.bvh_nodes, st0.bvh_leaves, st0.max_depth)
    ds.close()


# ------------------------------------------------------------------------------------------------ two-level scenes
def _three(seed=41):
    rng = np.random.default_rng(seed)
    small = _soup(rng, 40)
    return [("fan", *_fan(rng, 300)), ("soup", *_soup(rng, 1025)), ("small", small[0] * np.float32(0.5), small[1])]


def _two_level_figures(mrt, case, ds, lay, built=None):
    """the scene's figures from its layout; built: (per-BLAS sah at the build, per-BLAS Cost at the build) once refits have happened"""
    st = ds.stats
    hdr = lay["header"].astype(np.int64)
    _finite(st)
    cost, per = T.scene_wide_cost(lay)
    _check_cost(case, st.wide_cost, cost, True)
    trees = T.rope_trees(lay)
    figs = [T.binary_figures(rows, 1.0, 1.0, st.max_leaf_tris) for _, rows in trees]
    assert len(figs) == len(per) == 3
    assert st.bvh_leaves == sum(f.leaves for f in figs)
    assert st.wide_depth == T.wide_depth(lay) == hdr[3] and hdr[5] == max(len(T.wide_levels(A.decode_nodes(lay["wnodes"]), f)) for _, f, n in T.blas_ranges(lay))
    top = T.binary_figures(lay["tlas_nodes"], 1.0, 1.0, 2)
    assert st.bvh_nodes == top.nodes == len(lay["tlas_nodes"]) and st.max_depth == top.depth + 1, "two-level scenes: the rope TLAS's nodes and its levels"
    assert st.wide_layout == 1 and st.max_leaf_tris == 4
    assert st.scene_bytes == T.scene_bytes(hdr, st, len(lay["rope_nodes"]), len(lay["rope_packets"]))
    assert np.array_equal(_histogram(mrt, ds), T.histogram(lay["wnodes"])), "all nodes of the array: the TLAS slots (the unused ones count as nodes without children) and every BLAS"
    if built is None:
        for f in figs:
            assert not f.violations, f.violations
        assert st.wide_cost == st.wide_cost_built and st.leaf_growth == 1.0 and st.refits == 0
        assert _bits(st.sah_cost) == _bits(T.mean_sah([f.sah32 for f in figs], [c.emu for c in per], [c.emu for c in per])), "the mean over the BLASes in double"
        _margin(case, "sah_cost", 0)
    else:
        sah0, per0 = built
        want = T.mean_sah(sah0, [c.emu for c in per], [c.emu for c in per0])
        u = T.ulps32(st.sah_cost, want)
        _margin(case, "sah_cost", u)
        assert u <= 2, "each BLAS's build-time figure scaled by its own wide_cost ratio (either within an ulp of the recount), the mean in double"
    return st, per, figs


@pytest.mark.parametrize("device", [False, True], ids=["commit", "stream"])
def test_two_level_build_and_refit(mrt, gpu_ctx, device):
    """three BLASes of different size and cost (and a second instance of the first: 4 instances, 3 BLASes), the largest one deformed twice"""
    meshes = _three()
    sc = _scene(mrt, meshes, extra=[("fan2", 0, [2.5, 0.0, 0.5])])
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    case = f"two-level/{'stream' if device else 'commit'}"
    lay = _layout(ds)
    st0, per0, figs0 = _two_level_figures(mrt, case + "/build", ds, lay)
    assert (st0.triangles, st0.instances) == (2 * 300 + 1025 + 40, 4), "instanced triangles: the fan counts twice"
    costs = sorted(float(c.emu) for c in per0)
    assert costs[2] > 1.05 * costs[0], "BLASes of clearly different cost: a mean over the wrong ranges is another number"
    sah0 = [f.sah32 for f in figs0]
    ranges = T.blas_ranges(lay)
    b_first, b_count = [(f, n) for b, f, n in ranges if b == 1][0]
    prev = F32(1)
    for step in range(2):
        new = _moved(meshes[1][1], step)
        if device:
            import torch
            ds.update_blas_device(1, _t(new, gpu_ctx), _t(sc.meshes[1].normals, gpu_ctx)); ds.refit_blas_device()
            torch.cuda.synchronize()
        else:
            ds.update_mesh(1, new, sc.meshes[1].normals); ds.commit()
        lay_next = _layout(ds)
        st, per, figs = _two_level_figures(mrt, f"{case}/{step}", ds, lay_next, built=(sah0, per0))
        assert st.refits == step + 1 and st.wide_cost_built == st0.wide_cost_built and st.bvh_leaves == st0.bvh_leaves and st.wide_depth == st0.wide_depth
        lo, hi = T.padded_boxes(new[meshes[1][2].astype(np.int64)])
        g = T.leaf_growth(lay["wnodes"], lay_next["wnodes"], lay_next["wpackets"][:, 3], lo, hi, np.ones(len(lo), bool), previous=prev, first=b_first, count=b_count)
        worst = max(F32(1), g.emu)          # (fold_blas_stats: the other BLASes stand at 1)
        u = T.ulps32(st.leaf_growth, worst)
        _margin(f"{case}/{step}", "leaf_growth", u, g.rel_bound)
        assert u <= 2 * (step + 1) and g.emu > 1.0 and g.rel_bound < CAP
        assert abs(float(g.ratio32) / g.ratio_exact - 1) <= g.rel_bound
        prev, lay = g.emu, lay_next
    ds.close()


# ------------------------------------------------------------------------------------------------ the policy
@pytest.mark.parametrize("two_level", [False, True], ids=["flat", "two-level"])
def test_refit_max_cost_ratio_flips_where_the_reference_says(mrt, gpu_ctx, two_level):
    """refit_max_cost_ratio acts on max(wide_cost / wide_cost_built, leaf_growth): half a percent above the reference's value of it the commit refits, half a percent
    below it builds again.  (The margin keeps both settings off a float32 tie; the agreement asserted above is at the ulp level.)"""
    meshes = _three(43) if two_level else _two_meshes(15)
    which = 1 if two_level else 0
    base = {"instancing": 1} if two_level else {}
    sc = _scene(mrt, meshes)
    new = _moved(meshes[which][1], 0)
    nrm = sc.meshes[which].normals
    probe = mrt.DeviceScene(gpu_ctx, sc, base)
    lay0 = _layout(probe)
    c0, _ = T.scene_wide_cost(lay0)
    probe.update_mesh(which, new, nrm); probe.commit()
    assert probe.refits == 1
    lay1 = _layout(probe)
    c1, _ = T.scene_wide_cost(lay1)
    if two_level:
        first, count = [(f, n) for b, f, n in T.blas_ranges(lay0) if b == which][0]
        lo, hi = T.padded_boxes(new[meshes[which][2].astype(np.int64)])
        g = T.leaf_growth(lay0["wnodes"], lay1["wnodes"], lay1["wpackets"][:, 3], lo, hi, np.ones(len(lo), bool), first=first, count=count)
    else:
        lo, hi, owner = _boxes(meshes, {which: new})
        g = T.leaf_growth(lay0["wnodes"], lay1["wnodes"], lay1["wpackets"][:, 3], lo, hi, owner == which)
    probe.close()
    m = max(float(c1.emu) / float(c0.emu), float(g.emu), 1.0)
    assert m * 0.995 >= 1.0, "the option takes values from 1"
    above = mrt.DeviceScene(gpu_ctx, sc, dict(base, refit_max_cost_ratio=m * 1.005))
    above.update_mesh(which, new, nrm); above.commit()
    st = above.stats
    assert above.refits == 1 and st.refits == 1 and st.leaf_growth > 1.0, "inside the ratio: refitted"
    above.close()
    below = mrt.DeviceScene(gpu_ctx, sc, dict(base, refit_max_cost_ratio=m * 0.995))
    below.update_mesh(which, new, nrm); below.commit()
    st = below.stats
    assert below.refits == 0 and st.refits == 0 and st.leaf_growth == 1.0 and st.wide_cost == st.wide_cost_built, "beyond the ratio: built again"
    cb, _ = T.scene_wide_cost(_layout(below))
    assert T.ulps32(st.wide_cost, cb.emu) <= 2
    below.close()
