"""The stages of the device build against what they are defined to make (tests/build_reference.py): is this the tree the builder promises, not merely a valid one?

  morton + sort   builder 0: the leaf order is the stable sort of k_morton's keys, recomputed bit for bit in float32 from the leaf boxes (which are k_flatten's
                  padded boxes of the input triangles, bit for bit); every inner node is the radix-tree node of its range.
  PLOC            builder 1: the dumped tree is the tree of the rounds as k_ploc_nn / k_ploc_merge / k_ploc_tail define them, for every radius.
  collapse        the 8-wide layout is a collapse of the binary tree dumped beside it (every child a binary subtree, matched by triangle ids), and its cost in the
                  DP's own metric lies within the float32 error of the optimum computed in float64; the greedy collapse (wide_collapse = 0) is a collapse too
                  and costs no less.
Option sets that make the dumps complete: build_reference.py's docstring.  Every case is one small build and a numpy check.  Nothing here pins node numbers or
byte images: numbering inside a level follows atomics.

Bounds.  Order, radix tree and PLOC topology are exact.  The collapse: eps = (1 + 2^-24)^(3 D + 8) - 1 for a binary tree of depth D (build_reference.epsilon: one
addition, one product and one addition per level behind a device-side table entry, eight roundings for box_area and the leaf term); the device chooses by costs
perturbed by at most eps either way, so what it chose costs at most (1 + eps) / (1 - eps) times the optimum C*, and nothing costs less than C*:
C* (1 - eps) / (1 + eps) <= cost <= C* (1 + eps) / (1 - eps).  Every case prints its excess ("EXCESS case cost / C* - 1") and the greedy collapse's ratio."""
import numpy as np
import pytest

import build_reference as B
import rope_audit as R
import tree_stats_reference as T
from bvh_audit import decode_instances
from test_build_sizes import _soup
from test_bvh_bounds import _quad
from test_tree_stats import _scene

pytestmark = pytest.mark.gpu

F32 = np.float32
FULL = {"max_leaf": 1, "presplit": 0, "wide": 0}          # the rope layout alone, nothing collapsed: the complete binary tree of the build


# ------------------------------------------------------------------------------------------------ geometry
def _soup_mesh(n, seed):
    return _soup(np.random.default_rng(seed), n)


def _sheet_mesh():
    """288 axis-aligned coplanar triangles at y = 0.5: every centre has the same y, that axis has no extent"""
    return _quad((0, 0.5, 0), np.eye(3)[0], np.eye(3)[2], 12)


def _grid_mesh():
    """a regular 24 x 24 grid of equal quads on a sheared plane (y = 0.3 x): the two triangles of a quad have one box, so one key — 576 pairs of equal keys — and
    the unions of neighbouring boxes tie along the rows"""
    return _quad((0, 1, 0), np.eye(3)[0] + 0.3 * np.eye(3)[1], np.eye(3)[2], 24)


def _coincident_mesh():
    """67 copies of one triangle (test_rope_audit's shape): one Morton key; the radix tree splits by position, PLOC makes a chain"""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32) + F32([-0.5, 0.3, -0.2])
    pos = np.tile(tri, (67, 1))
    return pos, np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)


SHAPES = {"sheet": _sheet_mesh, "grid": _grid_mesh, "coincident": _coincident_mesh}


def _mesh(case):
    return SHAPES[case]() if case in SHAPES else _soup_mesh(case, 13 * case + 1)


def _dumped_tree(mrt, gpu_ctx, pos, idx, opts):
    """build, dump parts 8 and 9, decode; the leaves' boxes by triangle id must be k_flatten's padded boxes of the input (identity transform), bit for bit"""
    ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("mesh", pos, idx)]), opts)
    assert ds.stats.wide_layout == (0 if opts.get("wide", 1) == 0 else 1)
    tree = B.binary_tree(ds.read_layout("rope_nodes"), ds.read_layout("rope_packets"))
    ds.close()
    lo, hi = B.leaf_boxes(tree)
    want_lo, want_hi = T.padded_boxes(np.asarray(pos, F32)[np.asarray(idx, np.int64)])
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), "a leaf's box is not k_flatten's padded box of its triangle"
    return tree, lo, hi


# ------------------------------------------------------------------------------------------------ morton + sort + radix tree
@pytest.mark.parametrize("case", [1, 2, 3, 65, 4095, 4096, 4097, 70001, "sheet", "grid", "coincident"])
def test_morton_order_and_radix_tree(mrt, gpu_ctx, case):
    """4095, 4096, 4097: one sort tile of 16 x 256 keys and the first size that needs two; 70 001: 18 tiles"""
    pos, idx = _mesh(case)
    tree, lo, hi = _dumped_tree(mrt, gpu_ctx, pos, idx, dict(FULL, builder=0))
    assert tree.n == len(idx)
    keys, q = B.morton_keys(lo, hi)
    srt = B.check_sorted_order(tree, keys)
    rad = B.check_radix_tree(tree, keys)
    print(f"STAGES morton {case}: {tree.n} leaves, depth {tree.depth}, {srt.counts['equal_pairs']} adjacent equal keys, {len(np.unique(keys))} distinct")
    srt.check(); rad.check()
    if isinstance(case, int) and case >= 2:          # the clamp at both ends, on every axis: exercised, not assumed
        assert (q.min(0) == 0).all() and (q.max(0) == 2097151).all(), (q.min(0), q.max(0))
    if case == "sheet":
        assert (q[:, 1] == 0).all() and q[:, 0].max() == 2097151 and q[:, 2].max() == 2097151, "the axis without extent takes the ext > 0 ? ... : 0 branch"
    if case == "grid":
        assert srt.counts["equal_pairs"] >= 576
    if case == "coincident":
        assert len(np.unique(keys)) == 1 and np.array_equal(tree.order, np.arange(67)), "one key: the order is the ids', the tree splits by position"


# ------------------------------------------------------------------------------------------------ PLOC
def _ploc_case(mrt, gpu_ctx, case, radius=None):
    pos, idx = _mesh(case)
    opts = dict(FULL, builder=1)
    if radius is not None:
        opts["ploc_radius"] = radius
    tree, lo, hi = _dumped_tree(mrt, gpu_ctx, pos, idx, opts)
    keys, _ = B.morton_keys(lo, hi)
    rep = B.check_ploc(tree, lo, hi, B.morton_order(keys), 16 if radius is None else radius)
    print(f"STAGES ploc {case} radius {radius or 16}: {tree.n} leaves, depth {tree.depth}, {rep.counts['rounds']} rounds")
    rep.check()
    return tree


@pytest.mark.parametrize("case", [2, 3, 65, 1023, 1024, 1025, 2049, 4097, 16385, "grid", "coincident"])
def test_ploc_rounds(mrt, gpu_ctx, case):
    """1024, 1025: the tail kernel alone, and one batch of four rounds in front of it; 2049, 4097, 16 385: several batches; the grid: ties decide; 67 coincident
    triangles: every round has one mutual pair, a chain"""
    tree = _ploc_case(mrt, gpu_ctx, case)
    if case == "coincident":
        assert tree.depth == 66


@pytest.mark.parametrize("radius", [1, 4, 256])
@pytest.mark.parametrize("n", [1025, 4097])
def test_ploc_radius_is_followed(mrt, gpu_ctx, n, radius):
    tree = _ploc_case(mrt, gpu_ctx, n, radius)
    if n == 4097 and radius == 1:
        other = _ploc_case(mrt, gpu_ctx, n)
        assert not np.array_equal(B.canonical(tree)[0], B.canonical(other)[0]), "radius 1 and radius 16 give one tree: the option is not followed"


# ------------------------------------------------------------------------------------------------ the 8-wide collapse
def _check_collapse(case, tree, wide_opt, wide_greedy, max_leaf, c_node=1.0, c_tri=0.5):
    """the optimal layout within the bound, the greedy one a collapse that costs no less; returns (excess, greedy ratio, eps)"""
    opt = B.optimal_collapse(tree, c_node, c_tri, max_leaf)
    eps = B.epsilon(tree.depth)
    lo, hi = opt.cost * (1 - eps) / (1 + eps), opt.cost * (1 + eps) / (1 - eps)
    rep = B.match_collapse(tree, wide_opt, max_leaf, c_node, c_tri)
    rep.check()
    g = B.match_collapse(tree, wide_greedy, max_leaf, c_node, c_tri)
    g.check()
    print(f"EXCESS {case}: cost / C* - 1 = {rep.cost / opt.cost - 1:+.3e} (eps {eps:.2e}, depth {tree.depth}, C* {opt.cost:.6g}, {rep.counts['wide_nodes']} wide nodes, "
          f"largest leaf {rep.counts['largest_leaf']}); greedy / C* = {g.cost / opt.cost:.4f} ({g.counts['wide_nodes']} wide nodes)")
    assert lo <= rep.cost <= hi, (case, rep.cost, opt.cost, eps)
    assert g.cost >= lo, (case, g.cost, opt.cost)
    return rep.cost / opt.cost - 1, g.cost / opt.cost, eps


def _flat_layouts(mrt, gpu_ctx, pos, idx, opts):
    out = []
    for wc in (1, 0):
        ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("mesh", pos, idx)]), dict(opts, wide_collapse=wc))
        assert ds.stats.wide_layout == 1
        tree = B.binary_tree(ds.read_layout("rope_nodes"), ds.read_layout("rope_packets"))          # (refuses a leaf of more than one reference)
        out.append((tree, B.wide_of(ds.read_layout("wnodes"), ds.read_layout("wpackets"))))
        ds.close()
    (tree, wide_opt), (tree0, wide_greedy) = out
    assert np.array_equal(B.canonical(tree)[0], B.canonical(tree0)[0]) and np.array_equal(tree.order, tree0.order), "wide_collapse changed the binary tree"
    return tree, wide_opt, wide_greedy


COLLAPSE = {"rope": 1, "presplit": 0, "cost_isect": 1e6}          # both layouts of one build: the full binary tree, and its collapse


@pytest.mark.parametrize("max_leaf", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 9, 65, 1025, 3000])
@pytest.mark.parametrize("builder", [0, 1, 2])
def test_collapse_is_optimal(mrt, gpu_ctx, builder, n, max_leaf):
    """n = 3000 with builder 1 (seed 31 * 3000 + 1 of _soup): the greedy collapse is visibly dearer than the bound allows the optimal one to be"""
    pos, idx = _soup_mesh(n, 31 * n + builder)
    tree, wide_opt, wide_greedy = _flat_layouts(mrt, gpu_ctx, pos, idx, dict(COLLAPSE, builder=builder, max_leaf=max_leaf))
    assert tree.n == n
    excess, ratio, eps = _check_collapse(f"b{builder}/n{n}/leaf{max_leaf}", tree, wide_opt, wide_greedy, max_leaf)
    if n == 3000 and builder == 1:
        assert ratio > (1 + eps) / (1 - eps), "the metric does not separate the greedy collapse from the optimal one"


@pytest.mark.parametrize("costs", [(1.0, 0.3), (1.0, 1.0), (2.0, 0.5)])
@pytest.mark.parametrize("max_leaf", [1, 2, 4])
@pytest.mark.parametrize("builder", [0, 1, 2])
def test_collapse_follows_its_cost_constants(mrt, gpu_ctx, builder, max_leaf, costs):
    n = 1025
    pos, idx = _soup_mesh(n, 31 * n + builder)
    opts = dict(COLLAPSE, builder=builder, max_leaf=max_leaf, wide_cost_node=costs[0], wide_cost_tri=costs[1])
    tree, wide_opt, wide_greedy = _flat_layouts(mrt, gpu_ctx, pos, idx, opts)
    _check_collapse(f"b{builder}/n{n}/leaf{max_leaf}/costs{costs}", tree, wide_opt, wide_greedy, max_leaf, *costs)


def test_collapse_of_every_blas_of_a_two_level_scene(mrt, gpu_ctx):
    """two BLASes of 300 and 1 025 triangles, three instances: the BLAS builds are driven from two_level.hip; parts 8 and 9 hold every BLAS's tree with indices relative
    to its instances' node_base / packet_base, part 0 its 8-wide nodes from wroot on (absolute), the packets' ids are local to the mesh"""
    meshes = [("a", *_soup_mesh(300, 77)), ("b", *_soup_mesh(1025, 78))]
    layouts = []
    for wc in (1, 0):
        sc = _scene(mrt, meshes, extra=[("a2", 0, [2.5, 0.0, 0.5])])
        ds = mrt.DeviceScene(gpu_ctx, sc, dict(COLLAPSE, instancing=1, wide_collapse=wc))
        assert ds.stats.wide_layout == 1 and ds.stats.instances == 3
        lay = dict(R.layout_of(ds), wnodes=ds.read_layout("wnodes"), wpackets=ds.read_layout("wpackets"))
        ds.close()
        inst = decode_instances(lay["instances"])
        ends = {root: end for name, root, end, pb, nt in R.trees_of(lay)}
        per = {}
        for i in range(3):
            nb, pb, nt = int(inst["node_base"][i]), int(inst["packet_base"][i]), int(inst["ntri"][i])
            per.setdefault(int(inst["blas"][i]), (B.binary_tree(lay["rope_nodes"][nb:ends[nb]], lay["rope_packets"][pb:pb + nt]), B.wide_of(lay["wnodes"], lay["wpackets"], int(inst["wroot"][i]))))
        layouts.append(per)
    assert sorted(t.n for t, w in layouts[0].values()) == [300, 1025]
    for b, (tree, wide_opt) in layouts[0].items():
        _check_collapse(f"two-level/BLAS{b}/n{tree.n}", tree, wide_opt, layouts[1][b][1], 4)


# ------------------------------------------------------------------------------------------------ options no other test names
def test_cost_trav_and_cost_isect_steer_the_binary_leaf_collapse(mrt, gpu_ctx):
    """scene options cost_trav / cost_isect: the emitted binary tree obeys k_refit's collapse rule under the constants given (tree_stats_reference.binary_figures
    recounts it from the dump: no inner node the rule would have made a leaf, sah_cost bit-equal), and cheap triangle tests give larger leaves than the default"""
    pos, idx = _soup_mesh(1025, 5)
    leaves = {}
    for ct, ci in ((1.0, 1.0), (2.0, 0.7), (1.0, 1e6)):
        ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("mesh", pos, idx)]), {"rope": 1, "presplit": 0, "cost_trav": ct, "cost_isect": ci})
        b = T.binary_figures(ds.read_layout("rope_nodes"), ct, ci, 4)
        assert not b.violations, b.violations
        assert np.asarray(ds.stats.sah_cost, F32).view(np.uint32) == np.asarray(b.sah32, F32).view(np.uint32), (ct, ci, ds.stats.sah_cost, b.sah32)
        leaves[(ct, ci)] = b.leaves
        ds.close()
    print(f"STAGES cost constants: leaves {leaves}")
    assert leaves[(2.0, 0.7)] < leaves[(1.0, 1.0)] < leaves[(1.0, 1e6)] == 1025


def test_validate_changes_nothing_but_the_check(mrt, gpu_ctx):
    """scene option validate: 0 and 1 give the same 8-wide nodes (as sets: numbering inside a level follows atomics; everything of a node but its child / packet
    base); any other value is refused"""
    pos, idx = _soup_mesh(3000, 9)
    def nodes(v):
        ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("mesh", pos, idx)]), {"validate": v})
        wn = ds.read_layout("wnodes")
        ds.close()
        rows = np.ascontiguousarray(wn[:, [0, 1, 2, 3] + list(range(6, 20))])
        return rows[np.lexsort(rows.T[::-1])]
    a, b = nodes(0), nodes(1)
    assert len(a) > 100 and np.array_equal(a, b)
    ds = mrt.DeviceScene(gpu_ctx, _scene(mrt, [("mesh", pos[:9], idx[:3])]))
    for bad in (2.0, -1.0, 0.5):
        assert mrt.lib.mrt_scene_set_option(ds.handle, b"validate", bad) == mrt._ffi.MRT_ERR_INVALID_ARGUMENT
    ds.close()
