"""tests/tree_stats_reference.py on hand-made layouts (no GPU): the recount of wide_cost, the histogram, the depth, leaf_growth and the binary tree's figures
gives what the same trees give worked out by hand, its emulation and its exact value part where float32 decoding is coarse (and the bound covers the gap), and
every planted defect — a dropped slot, a flipped imask bit, a raised count, a node k_refit would have collapsed — changes the figure it should."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import tree_stats_reference as T
from test_bvh_audit_cpu import _encode_node, _get_byte, _set_byte

F32 = np.float32


def f32(x):
    """one rounding of a Python float (a double) to float32 — independent of numpy's float32 arithmetic"""
    return struct.unpack("f", struct.pack("f", x))[0]


# ------------------------------------------------------------------------------------------------ a dyadic 8-wide tree
# node 0 (grid step 2^-6 from the origin): slot 0 -> node 1 over A = [1, 2]^3; slot 2: leaf B of 2 triangles, [0, 0, 0] .. [1, .5, .5]; slot 5: leaf C of 1, [2, 2, 2] .. [3, 3, 2]
# node 1 (grid step 2^-8 from (1, 1, 1)): slot 1: leaf D of 3, [1, 1, 1] .. [1.5, 1.5, 1.25]; slot 6: leaf E of 1, [1.5, 1.25, 1] .. [1.75, 1.75, 1.5]
A_, B_, C_ = ((1, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, .5, .5)), ((2, 2, 2), (3, 3, 2))
D_, E_ = ((1, 1, 1), (1.5, 1.5, 1.25)), ((1.5, 1.25, 1), (1.75, 1.75, 1.5))


def _tree():
    n0 = _encode_node((0, 0, 0), (255 / 64,) * 3, [("node", *A_, 0, 0), None, ("leaf", *B_, 2, 0), None, None, ("leaf", *C_, 1, 2), None, None], 1, 0)
    n1 = _encode_node((1, 1, 1), (1 + 255 / 256,) * 3, [None, ("leaf", *D_, 3, 0), None, None, None, None, ("leaf", *E_, 1, 3), None], 0, 3)
    return np.stack([n0, n1])


def test_the_hand_made_tree():
    wn = _tree()
    D = T.decode_nodes(wn)
    assert np.array_equal(D["ex"], [[-6] * 3, [-8] * 3])
    assert np.array_equal(D["lo"][0, 5], C_[0]) and np.array_equal(D["hi"][1, 6], E_[1]), "dyadic boxes decode to themselves"
    # areas 2 (xy + yz + zx): A 6, B 2.5, C 2 (flat), D 1, E 1; the root's children span [0, 0, 0] .. [3, 3, 2]: 42
    # sum = 1 x 6 + .5 x 2 x 2.5 + .5 x 1 x 2 + .5 x 3 x 1 + .5 x 1 x 1 = 11.5;  cost = (1 x 42 + 11.5) / 42
    c = T.wide_cost(wn, 0, 2, 0, 1.0, 0.5)
    assert c.sum32 == 11.5 and c.sum64 == 11.5 and c.area_root == 42.0
    assert c.emu == F32(53.5 / 42) and c.exact == 53.5 / 42
    assert abs(float(c.emu) - c.exact) <= c.bound <= 8 * T.U * c.exact, "every plane is exact here: the bound is the seven float32 operations' roundings and the final one"
    # other constants: (2 x 42 + 2 x 6 + .25 x (5 + 2 + 3 + 1)) / 42
    assert T.wide_cost(wn, 0, 2, 0, 2.0, 0.25).emu == F32((84 + 12 + 2.75) / 42)
    # the subtree at node 1 alone: children span [1, 1, 1] .. [1.75, 1.75, 1.5]: 2 (.5625 + .375 + .375) = 2.625; (2.625 + 1.5 + .5) / 2.625
    assert T.wide_cost(wn, 1, 1, 1, 1.0, 0.5).emu == F32(4.625 / 2.625)
    assert T.histogram(wn).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 4, 7]
    lay = dict(header=np.array([2, 0, 0, 2, 7, 0, 0, 3], np.uint32), wnodes=wn)
    assert T.wide_depth(lay) == 2
    assert [lv.tolist() for lv in T.wide_levels(D, 0)] == [[0], [1]]
    cost, per = T.scene_wide_cost(lay)
    assert cost.emu == c.emu and len(per) == 1
    assert T.scene_wide_cost(dict(header=np.zeros(8, np.uint32), wnodes=wn[:0]))[0].emu == 0


def _drop_slot(wn):          # node 0 slot 5: empty box, no count
    for w in (8, 10, 12):
        _set_byte(wn, 0, w + 1, 1, 255)
    for w in (14, 16, 18):
        _set_byte(wn, 0, w + 1, 1, 0)
    _set_byte(wn, 0, 7, 1, 0)


def _flip_imask(wn):         # node 0 slot 5 becomes an internal child: weight c_node instead of c_tri x 1
    wn[0, 3] ^= np.uint32(1 << (24 + 5))


def _raise_count(wn):        # node 0 slot 5: 1 -> 2 triangles
    _set_byte(wn, 0, 7, 1, _get_byte(wn, 0, 7, 1) + (1 << 5))


@pytest.mark.parametrize("mutate,cost,hist", [
    (_drop_slot, (24 + 10.5) / 24, [0, 0, 2, 0, 0, 0, 0, 0, 0, 1, 3, 6]),          # the root's children now span [0, 2]^3: area 24; the sum loses .5 x 1 x 2
    (_flip_imask, (42 + 12.5) / 42, [0, 0, 1, 0, 1, 0, 0, 0, 0, 2, 4, 7]),          # (the histogram counts the slot twice, as k_wide_histogram does: its mask bit and its count)
    (_raise_count, (42 + 12.5) / 42, [0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 4, 8]),
], ids=["drop_slot", "flip_imask", "raise_count"])
def test_mutations_change_the_figures(mutate, cost, hist):
    wn = _tree()
    good = T.wide_cost(wn, 0, 2, 0).emu
    mutate(wn)
    c = T.wide_cost(wn, 0, 2, 0)
    assert c.emu != good and c.emu == F32(cost)
    assert T.histogram(wn).tolist() == hist


def test_round_sum32_is_one_rounding():
    rng = np.random.default_rng(3)
    a = np.r_[rng.uniform(-2e4, 2e4, 400).astype(F32).astype(np.float64), [1.3e4] * 3, [F32(1.3e4)] * 256]
    q = np.r_[rng.integers(0, 256, 403), np.arange(256)].astype(np.float64)
    e = np.r_[rng.integers(-40, 4, 403), [-14] * 256]
    b = q * np.ldexp(1.0, e)
    got = T.round_sum32(a, b)
    twice = 0
    for x, y, g in zip(a, b, got):
        exact = Fraction(float(x)) + Fraction(float(y))
        lo, hi = F32(np.nextafter(g, F32(-np.inf))), F32(np.nextafter(g, F32(np.inf)))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == (Fraction(float(hi)) - Fraction(float(g))) / 2 or err == (Fraction(float(g)) - Fraction(float(lo))) / 2:
            assert int(g.view(np.uint32)) & 1 == 0, "a tie goes to the even neighbour"
        twice += F32(x + y) != g
    # the case a plain float64 sum gets wrong: 2^24 + 1 + 2^-40 lies above the tie, its float64 sum on it
    assert F32(2.0 ** 24 + (1 + 2.0 ** -40)) == F32(2.0 ** 24) and T.round_sum32(2.0 ** 24, 1 + 2.0 ** -40) == F32(2.0 ** 24 + 2)


def test_a_far_node_with_a_step_below_its_origins_ulp():
    """origin 1.3e4 (float32 ulp 2^-10), grid step 2^-14: the traversal's float32 planes fall on multiples of 2^-10, the exact ones do not"""
    org = float(F32(1.3e4))
    step = 2.0 ** -14
    wn = _encode_node((org,) * 3, (org + 255 * 2.0 ** -10,) * 3, [("leaf", (org,) * 3, (org + 2.0 ** -10,) * 3, 1, 0)] + [None] * 7, 0, 0)[None, :].copy()
    wn[0, 3] = (int(wn[0, 3]) & 0xFF000000) | 0xF2F2F2          # exponents -14
    for sl, (a, b, cnt) in enumerate([(0, 40, 1), (37, 200, 2), (90, 255, 3)]):
        for ax in range(3):
            _set_byte(wn, 0, 8 + 2 * ax + sl // 4, sl % 4, a); _set_byte(wn, 0, 14 + 2 * ax + sl // 4, sl % 4, b)
        _set_byte(wn, 0, 6 + sl // 4, sl % 4, cnt << 5)
    D = T.decode_nodes(wn)
    assert np.array_equal(D["lo"][0, 1], [org + 37 * step] * 3) and D["ex"][0, 0] == -14
    c = T.wide_cost(wn, 0, 1, 0)
    # float32 planes are the exact ones rounded to multiples of 2^-10 = 16 grid steps (round_sum32, checked against fractions above)
    r = lambda k: float(T.round_sum32(org, k * step)) - org
    ext = [(r(b) - r(a)) for a, b in ((0, 40), (37, 200), (90, 255))]
    assert all(x == round(x * 1024) / 1024 for x in ext)
    s = sum(6 * x * x * 0.5 * n for x, n in zip(ext, (1, 2, 3)))
    A = 6 * (r(255) - r(0)) ** 2
    assert c.emu == F32((A + s) / A)
    xs = sum(6 * ((b - a) * step) ** 2 * 0.5 * n for (a, b), n in zip(((0, 40), (37, 200), (90, 255)), (1, 2, 3)))
    assert c.exact == pytest.approx((6 * (255 * step) ** 2 + xs) / (6 * (255 * step) ** 2), rel=1e-15)
    assert T.ulps32(c.emu, F32(c.exact)) > 1000, "emulation and meaning part here"
    assert abs(float(c.emu) - c.exact) <= c.bound < np.inf


# ------------------------------------------------------------------------------------------------ leaf_growth
def test_leaf_growth_by_hand():
    # one node, grid step 2^-6: slot 0 = triangle 0 in [0, 1]^3 (x y + y z + z x = 3), slot 3 = triangle 1 in [2, 3]^3 (3)
    wn = _encode_node((0, 0, 0), (255 / 64,) * 3, [("leaf", (0, 0, 0), (1, 1, 1), 1, 0), None, None, ("leaf", (2, 2, 2), (3, 3, 3), 1, 1)] + [None] * 4, 0, 0)[None, :]
    gids = np.array([0, 1])
    # triangle 0 now reaches x = 1.49: rounded outwards onto the old grid 96 / 64 = 1.5 -> 1.5 + 1 + 1.5 = 4
    lo = np.array([[0, 0, 0], [2, 2, 2]], F32); hi = np.array([[1.49, 1, 1], [3, 3, 3]], F32)
    g = T.leaf_growth(wn, wn, gids, lo, hi, [True, False], previous=1.5)
    assert (g.g_old, g.g_new, g.slots) == (3.0, 4.0, 1)
    assert g.ratio32 == F32(4 / 3) and g.emu == F32(f32(1.5 * f32(4 / 3))) and g.ratio_exact == 4 / 3
    assert abs(float(g.ratio32) / g.ratio_exact - 1) <= g.rel_bound < 2e-6          # (half an ulp of coordinates below 4 on either end of extents of 1, two extents per product, old and new)
    both = T.leaf_growth(wn, wn, gids, lo, hi, [True, True], previous=1.5)
    assert (both.g_old, both.g_new) == (6.0, 7.0) and both.emu != g.emu, "an unmoved leaf in the sums changes the figure"
    none = T.leaf_growth(wn, wn, gids, lo, hi, [False, False], previous=1.5)
    assert none.emu == F32(1.5) and none.slots == 0
    # a box that collapses to nothing contributes nothing, and its old area neither (the node's new sum is 0)
    flat = T.leaf_growth(wn, wn, gids, np.array([[1, 1, 1], [2, 2, 2]], F32), np.array([[1, 1, 1], [3, 3, 3]], F32), [True, False])
    assert flat.emu == F32(1) and (flat.g_old, flat.g_new) == (0.0, 0.0)
    # links changed between the dumps: refused
    other = wn.copy(); other[0, 5] = 7
    with pytest.raises(AssertionError, match="tri_base"):
        T.leaf_growth(wn, other, gids, lo, hi, [True, False])


def test_unmoved_leaves_keep_their_boxes():
    before = _encode_node((0, 0, 0), (255 / 64,) * 3, [("leaf", (0, 0, 0), (1, 1, 1), 1, 0), ("leaf", (2, 2, 2), (3, 3, 3), 1, 1)] + [None] * 6, 0, 0)[None, :]
    # the sibling grew, the node's grid is coarser (step 2^-5): slot 0 holds a clipped reference — its triangle's box reaches to x = 3 — and keeps [0, 1]^3
    after = _encode_node((0, 0, 0), (255 / 32,) * 3, [("leaf", (0, 0, 0), (1, 1, 1), 1, 0), ("leaf", (2, 2, 2), (6, 6, 6), 1, 1)] + [None] * 6, 0, 0)[None, :]
    lo = np.array([[0, 0, 0], [2, 2, 2]], F32); hi = np.array([[3, 1, 1], [6, 6, 6]], F32)
    n, bad, clipped = T.unmoved_leaf_excess(before, after, np.array([0, 1]), lo, hi, [False, True])
    assert (n, bad, clipped) == (1, [], 1)
    # had slot 0 been given its whole triangle's box, the audit names the plane
    grown = _encode_node((0, 0, 0), (255 / 32,) * 3, [("leaf", (0, 0, 0), (3, 1, 1), 1, 0), ("leaf", (2, 2, 2), (6, 6, 6), 1, 1)] + [None] * 6, 0, 0)[None, :]
    n, bad, clipped = T.unmoved_leaf_excess(before, grown, np.array([0, 1]), lo, hi, [False, True])
    assert n == 1 and len(bad) == 1 and "slot 0 axis x hi" in bad[0]
    # an unsplit triangle's leaf is cut to the triangle's own box: [0.25, 1] on x here, not the [0, 1] it had
    tight = _encode_node((0, 0, 0), (255 / 32,) * 3, [("leaf", (0.25, 0, 0), (1, 1, 1), 1, 0), ("leaf", (2, 2, 2), (6, 6, 6), 1, 1)] + [None] * 6, 0, 0)[None, :]
    lo2 = np.array([[0.25, 0, 0], [2, 2, 2]], F32); hi2 = np.array([[1, 1, 1], [6, 6, 6]], F32)
    assert T.unmoved_leaf_excess(before, tight, np.array([0, 1]), lo2, hi2, [False, True]) == (1, [], 0)
    n, bad, _ = T.unmoved_leaf_excess(before, tight, np.array([0, 1]), lo, hi, [False, True])
    assert len(bad) == 1 and "slot 0 axis x lo" in bad[0], "a plane inside the box to keep"


def test_padded_boxes_by_hand():
    tri = np.array([[[1, 2, -4], [0.5, 2, 3], [1, -8, 0]], [[1.3e4, -2.7e3, 7.1e3], [1.3e4 + 1, -2.7e3, 7.1e3], [1.3e4, -2.7e3 + 1, 7.1e3 + 0.5]]], F32)
    lo, hi = T.padded_boxes(tri)
    k5, k6 = f32(1e-5), f32(1e-6)
    for t in range(2):
        for ax in range(3):
            mn, mx = float(tri[t, :, ax].min()), float(tri[t, :, ax].max())
            e = f32(f32(k5 * max(abs(mn), abs(mx))) + k6)          # (products and sums of float32 values in double are exact or round once more harmlessly: 48 bits)
            assert float(lo[t, ax]) == f32(mn - e) and float(hi[t, ax]) == f32(mx + e), (t, ax)
    assert float(lo[0, 0]) == f32(0.5 - f32(f32(k5 * 1.0) + k6)) and float(hi[0, 1]) == f32(2 + f32(f32(k5 * 8.0) + k6))


# ------------------------------------------------------------------------------------------------ the rope tree
def _rope(lo, hi, a, b):
    w = np.zeros(16, np.uint32)
    w[0:3] = np.asarray(lo, F32).view(np.uint32); w[4:7] = np.asarray(hi, F32).view(np.uint32)
    w[3], w[7] = a, b
    w[8:16] = 0xFFFFFFFF
    return w


def _rope_tree(nt4=4):
    L = T.NODE_LEAF
    return np.stack([_rope((0, 0, 0), (4, 2, 1), 1, 2 | (0x0F << 24)),          # root: area 2 (8 + 2 + 4) = 28
                     _rope((0, 0, 0), (1, 1, 1), L | 0, 2),                      # leaf of 2: area 6 -> 12
                     _rope((2, 0, 0), (4, 2, 1), 3, 4),                          # inner: area 2 (4 + 2 + 2) = 16
                     _rope((2, 0, 0), (3, 1, 1), L | 2, 1),                      # leaf of 1: area 6 -> 6
                     _rope((3, 0, 0), (4, 2, 1), L | 3, nt4)])                   # leaf of 4: area 2 (2 + 2 + 1) = 10 -> 40


def test_binary_figures_by_hand():
    b = T.binary_figures(_rope_tree())
    assert (b.nodes, b.leaves, b.depth, b.largest_leaf) == (5, 3, 2, 4)
    # node 2: 16 + 6 + 40 = 62 (5 references: no leaf); root: 28 + 12 + 62 = 102
    assert b.cost_root32 == 102 and b.area_root32 == 28 and b.sah32 == F32(102 / 28) and b.sah64 == 102 / 28
    assert not b.violations
    # other constants: leaves ci x area x nt = 36 / 18 / 120, node 2: 2 x 16 + 18 + 120 = 170, root: 2 x 28 + 36 + 170 = 262
    assert T.binary_figures(_rope_tree(), ct=2.0, ci=3.0).sah32 == F32(262 / 28)
    # node 2 over 1 + 1 references: as a leaf 16 x 2 = 32 against 16 + 6 + 10 = 32 as emitted — k_refit collapses at <=
    bad = T.binary_figures(_rope_tree(nt4=1))
    assert len(bad.violations) == 1 and "inner node 2" in bad.violations[0] and "collapses" in bad.violations[0]
    assert [v[:11] for v in T.binary_figures(_rope_tree(nt4=1), max_leaf=1).violations] == ["leaf node 1"], "two references do not fit a leaf of one: node 2 stays, leaf 1 is too large"
    big = T.binary_figures(_rope_tree(nt4=5))
    assert big.largest_leaf == 5 and len(big.violations) == 1 and "leaf node 4" in big.violations[0]


def test_scene_bytes_and_mean_sah():
    class S: triangles, vertices, instances, max_submeshes = 10, 30, 2, 3
    flat = np.array([4, 0, 0, 2, 12, 0, 0, 3])
    assert T.scene_bytes(flat, S, 0, 0) == 160 + 480 + 120 + 128 + 320 + 576
    assert T.scene_bytes(flat, S, 7, 12) == 160 + 480 + 120 + 128 + 320 + 576 + 448 + 576
    assert T.scene_bytes(np.array([0, 0, 0, 0, 0, 0, 0, 3]), S, 7, 12) == 160 + 480 + 120 + 128 + 448 + 576
    two = np.array([9, 2, 2, 4, 10, 2, 2, 3])
    assert T.scene_bytes(two, S, 7, 10) == 448 + 480 + 720 + 480 + 160 + 480 + 2 * (144 + 60)
    assert T.mean_sah([2.0, 4.0], [3.0, 5.0], [3.0, 4.0]) == F32((2.0 + float(F32(4) * (F32(5) / F32(4)))) / 2)
    assert T.mean_sah([2.0, 4.0], [3.0, 5.0], [0.0, 5.0]) == F32(3.0)
