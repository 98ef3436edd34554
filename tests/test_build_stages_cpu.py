"""tests/build_reference.py has teeth before it judges a device build (test_build_stages.py): its optimal collapse against exhaustive enumeration, its PLOC
rounds on cases small enough to do by hand, its radix-tree and sort checks on a hand-built tree, and one planted defect per check — each must be flagged by the
check meant for it, by name.  No GPU."""
import functools

import numpy as np
import pytest

import build_reference as B

F32 = np.float32


# ------------------------------------------------------------------------------------------------ helpers
def _boxes(rng, n):
    """n small boxes strung along a jittered line: neighbours in rank are neighbours in space, sizes vary by a decade"""
    c = np.c_[np.arange(n) * 0.3, np.zeros(n), np.zeros(n)] + rng.uniform(-0.25, 0.25, (n, 3))
    e = 10.0 ** rng.uniform(-1.5, -0.5, (n, 3))
    return (c - e).astype(F32), (c + e).astype(F32)


def _tree_of_shape(shape, rng):
    """a Tree from a nested-tuple shape (None = leaf), random boxes by rank, the leaves' ids a random permutation"""
    left, right = [], []
    def walk(s):
        me = len(left); left.append(-1); right.append(-1)
        if s is not None:
            left[me] = walk(s[0]); right[me] = walk(s[1])
        return me
    walk(shape)
    left, right = np.array(left), np.array(right)
    leaves = np.nonzero(left < 0)[0]          # (preorder numbering: the leaves come in rank order)
    n = len(leaves)
    lo = np.zeros((len(left), 3), F32); hi = np.zeros((len(left), 3), F32)
    lo[leaves], hi[leaves] = _boxes(rng, n)
    gid = np.full(len(left), -1); gid[leaves] = rng.permutation(n)
    return B.make_tree(left, right, 0, gid, lo, hi)


@functools.lru_cache(maxsize=None)
def _shapes(n):
    if n == 1:
        return (None,)
    return tuple((l, r) for k in range(1, n) for l in _shapes(k) for r in _shapes(n - k))


def _exhaustive(tree, c_node, c_tri, limit):
    """the least cost over EVERY valid collapse: a node is a leaf (<= limit references) or a wide node whose children are any cut of its subtree with 2 .. 8 members,
    each child collapsed in every way in turn; cuts are enumerated outright (cuts(n) = {n} or any cut of the left with any cut of the right)"""
    cn, ct = float(F32(c_node)), float(F32(c_tri))
    A = B.areas(tree); nt = tree.last - tree.first + 1
    cuts, best = {}, {}
    def cuts_of(v):
        if v not in cuts:
            out = [(v,)]
            if tree.left[v] >= 0:
                out += [a + b for a in cuts_of(int(tree.left[v])) for b in cuts_of(int(tree.right[v])) if len(a) + len(b) <= B.WIDE_N]
            cuts[v] = out
        return cuts[v]
    def cost(v):
        if v not in best:
            c = A[v] * nt[v] * ct if nt[v] <= limit else np.inf
            if tree.left[v] >= 0:
                c = min(c, A[v] * cn + min(sum(cost(x) for x in cut) for cut in cuts_of(v) if len(cut) >= 2))
            best[v] = c
        return best[v]
    return cost(int(tree.levels[0][0]))


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


# ------------------------------------------------------------------------------------------------ the optimal collapse
@pytest.mark.parametrize("max_leaf", [1, 2, 4])
def test_optimal_collapse_against_every_collapse_of_every_shape(max_leaf):
    """every ordered binary tree shape of 1 .. 9 leaves (2 056 of them; 9 leaves: the cut of all leaves no longer fits one node), random boxes: the table's optimum
    is the exhaustive minimum, the collapse unfolded from its decisions is valid (collapse_of, matched by ids) and costs exactly that"""
    rng = np.random.default_rng(100 + max_leaf)
    shapes = 0
    for n in range(1, 10):
        for shape in _shapes(n):
            tree = _tree_of_shape(shape, rng)
            c_node, c_tri = ((1.0, 0.5), (1.0, 0.3), (1.0, 1.0), (2.0, 0.5))[shapes % 4]
            opt = B.optimal_collapse(tree, c_node, c_tri, max_leaf)
            want = _exhaustive(tree, c_node, c_tri, min(max_leaf, 4))
            assert _close(opt.cost, want), (shape, opt.cost, want)
            col = B.unfold(tree, opt)
            assert _close(B.collapse_cost(tree, col, c_node, c_tri), want), shape
            rep = B.match_collapse(tree, B.as_wide(tree, col), max_leaf, c_node, c_tri)
            assert not rep.failures and _close(rep.cost, want), (shape, rep.failures, rep.cost, want)
            assert all(len(ch) <= 8 for _, ch in col) and rep.counts["largest_leaf"] <= min(max_leaf, 4)
            shapes += 1
    assert shapes == 2056


def _host_sah_tree(mrt, lo, hi):
    n = len(lo)
    lo4 = np.zeros((n, 4), F32); hi4 = np.zeros((n, 4), F32); lo4[:, :3] = lo; hi4[:, :3] = hi
    order = np.zeros(n, np.uint32); left = np.zeros(n - 1, np.uint32); right = np.zeros(n - 1, np.uint32); parent = np.zeros(2 * n - 1, np.uint32)
    mrt._ffi.check(mrt.lib.mrt_debug_host_sah(mrt._ffi.ptr(lo4), mrt._ffi.ptr(hi4), n, mrt._ffi.ptr(order), mrt._ffi.ptr(left), mrt._ffi.ptr(right), mrt._ffi.ptr(parent)))
    N = 2 * n - 1          # internal i -> i, leaf j -> n - 1 + j holding reference order[j]
    L = np.full(N, -1, np.int64); R = np.full(N, -1, np.int64); L[:n - 1] = left; R[:n - 1] = right
    gid = np.full(N, -1, np.int64); gid[n - 1:] = order
    blo = np.zeros((N, 3), F32); bhi = np.zeros((N, 3), F32); blo[n - 1:] = lo[order]; bhi[n - 1:] = hi[order]
    return B.make_tree(L, R, int(np.nonzero(parent == 0xFFFFFFFF)[0][0]), gid, blo, bhi)


def test_optimal_collapse_beats_the_greedy_collapse_on_a_host_sah_tree(mrt):
    """1 025 boxes, the topology of the host's binned-SAH builder (no device): optimum <= the greedy collapse's cost in the same metric, strictly here"""
    from tree_stats_reference import padded_boxes
    from test_build_sizes import _soup
    pos, _ = _soup(np.random.default_rng(5), 1025)
    tree = _host_sah_tree(mrt, *padded_boxes(pos.reshape(-1, 3, 3)))
    for max_leaf in (1, 4):
        opt = B.optimal_collapse(tree, 1.0, 0.5, max_leaf)
        col = B.unfold(tree, opt)
        rep = B.match_collapse(tree, B.as_wide(tree, col), max_leaf)
        assert not rep.failures and _close(rep.cost, opt.cost)
        greedy = B.greedy_collapse(tree)
        g = B.match_collapse(tree, B.as_wide(tree, greedy), max_leaf)
        assert not g.failures and _close(g.cost, B.collapse_cost(tree, greedy))
        print(f"host SAH 1025, max_leaf {max_leaf}: optimum {opt.cost:.6f}, greedy {g.cost:.6f}, ratio {g.cost / opt.cost:.4f}; wide nodes {rep.counts['wide_nodes']} against {g.counts['wide_nodes']}")
        assert opt.cost < g.cost


# ------------------------------------------------------------------------------------------------ PLOC by hand
def _row(xs, w=1.0):
    xs = np.asarray(xs, np.float64)
    lo = np.c_[xs, np.zeros(len(xs)), np.zeros(len(xs))]
    return lo.astype(F32), (lo + [w, 1.0, 1.0]).astype(F32)


def _ploc(lo, hi, radius):
    counts, seq, rounds = B.ploc_topology(lo, hi, np.arange(len(lo)), radius)
    return counts.tolist(), seq.tolist(), rounds.tolist()


def test_ploc_two_boxes():
    assert _ploc(*_row([0, 5]), 16) == ([2, 1, 1], [0, 1], [0, -1, -1])
    assert _ploc(*_row([3]), 16) == ([1], [0], [-1])


def test_ploc_three_boxes_with_a_tie_the_lowest_position_wins():
    """A, B, C evenly spaced: B is as near to A as to C; strict < from the lowest position up gives A.  ((A, B), C), never (A, (B, C))"""
    for radius in (1, 16):
        assert _ploc(*_row([0, 2, 4]), radius) == ([3, 2, 1, 1, 1], [0, 1, 2], [1, 0, -1, -1, -1])


def test_ploc_radius_one_and_two_give_different_trees():
    """positions 0 .. 3 at x = 0, 10, 0.5, 10.75: with radius 2 the near boxes find each other across a position, with radius 1 the middle pair merges first"""
    lo, hi = _row([0, 10, 0.5, 10.75])
    assert _ploc(lo, hi, 2) == ([4, 2, 1, 1, 2, 1, 1], [0, 2, 1, 3], [1, 0, -1, -1, 0, -1, -1])
    assert _ploc(lo, hi, 1) == ([4, 3, 1, 2, 1, 1, 1], [0, 1, 2, 3], [2, 1, -1, 0, -1, -1, -1])


def test_ploc_a_row_of_equal_boxes_is_a_chain():
    """every area ties: every cluster names the lowest position but itself, (0, 1) is the one mutual pair of every round"""
    for radius in (1, 3, 16):
        counts, seq, rounds = _ploc(*_row([1, 1, 1, 1, 1]), radius)
        assert counts == [5, 4, 3, 2, 1, 1, 1, 1, 1] and seq == [0, 1, 2, 3, 4] and rounds == [3, 2, 1, 0, -1, -1, -1, -1, -1]


def _ploc_tree(lo, hi, order, radius, redirect=None):
    """a Tree as a dump of a PLOC build would give it (reference rounds, optionally with a planted defect)"""
    n = len(order)
    left, right, made, root = B.ploc_rounds(lo[order], hi[order], radius, redirect)
    gid = np.full(2 * n - 1, -1, np.int64); gid[:n] = order
    blo = np.zeros((2 * n - 1, 3), F32); bhi = np.zeros((2 * n - 1, 3), F32); blo[:n] = lo[order]; bhi[:n] = hi[order]
    return B.make_tree(left, right, root, gid, blo, bhi), left, made


def test_check_ploc_flags_one_merge_redirected_to_the_second_nearest_neighbour():
    rng = np.random.default_rng(8)
    c = rng.uniform(-1, 1, (300, 3)); e = 10.0 ** rng.uniform(-2, -1, (300, 3))
    lo, hi = (c - e).astype(F32), (c + e).astype(F32)
    keys, _ = B.morton_keys(lo, hi)
    order = B.morton_order(keys)
    good, left, made = _ploc_tree(lo, hi, order, 16)
    assert not B.check_ploc(good, lo, hi, order, 16).failures
    assert B.check_ploc(good, lo, hi, order, 15).failures or B.check_ploc(good, lo, hi, order, 1).failures, "another radius is another tree"
    # the merges of round 0 (their left members are leaves: id = position).  A redirected pair often merges one round later into the same tree: the first
    # redirection that changes the tree is the planted defect
    same = B.canonical(good)
    for node in np.nonzero((left >= 0) & (made == 0))[0]:
        bad, _, _ = _ploc_tree(lo, hi, order, 16, redirect=(0, int(left[node])))
        if not (np.array_equal(B.canonical(bad)[0], same[0]) and np.array_equal(bad.order, good.order)):
            break
    else:
        raise AssertionError("no redirection changed the tree")
    rep = B.check_ploc(bad, lo, hi, order, 16)
    assert rep.failures and rep.failures[0].startswith("ploc: preorder position") and "merged in round" in rep.failures[0], rep.failures


# ------------------------------------------------------------------------------------------------ radix tree and sort, by hand
def _radix_tree(keys, ids, move_split=None):
    """top-down, independent of k_karras' searches: the range [a, b] of the sorted (key, position) pairs splits where their highest differing bit turns 1.
    keys: sorted; ids: the triangle id at every position.  move_split (a, b, by): that one range splits `by` positions further right — a planted defect."""
    aug = [(int(k) << 32) | p for p, k in enumerate(keys)]
    left, right, gid = [], [], []
    def build(a, b):
        me = len(left); left.append(-1); right.append(-1); gid.append(-1)
        if a == b:
            gid[me] = int(ids[a]); return me
        bit = (aug[a] ^ aug[b]).bit_length() - 1
        s = max(p for p in range(a, b) if not (aug[p] >> bit) & 1)
        if move_split is not None and move_split[:2] == (a, b):
            s += move_split[2]
        left[me] = build(a, s); right[me] = build(s + 1, b)
        return me
    build(0, len(keys) - 1)
    N = len(left)
    return B.make_tree(left, right, 0, gid, np.zeros((N, 3), F32), np.ones((N, 3), F32))


def test_radix_and_sort_checks_on_a_hand_built_tree():
    # by hand: keys 000, 001, 001, 100 — the root splits after rank 2 (bit 2), [0, 2] after rank 0 (bit 0), the equal keys at ranks 1, 2 by position (01 | 10)
    ids = np.array([3, 0, 2, 1])
    keys_by_id = np.zeros(4, np.uint64); keys_by_id[ids] = [0b000, 0b001, 0b001, 0b100]
    t = _radix_tree([0b000, 0b001, 0b001, 0b100], ids)
    assert B.canonical(t)[0].tolist() == [4, 3, 1, 2, 1, 1, 1] and t.order.tolist() == [3, 0, 2, 1]
    assert not B.check_sorted_order(t, keys_by_id).failures and not B.check_radix_tree(t, keys_by_id).failures
    # larger, with runs of equal keys (one of five: split by position over three levels) and keys that differ in the top bit of the 63
    rng = np.random.default_rng(3)
    ks = np.sort(np.concatenate([rng.integers(0, 1 << 62, 40), np.full(5, 77), np.full(2, 1 << 62), [0, 0, (1 << 63) - 1]]).astype(np.uint64))
    n = len(ks)
    ids = np.lexsort((np.arange(n), rng.permutation(ks)))          # some permutation and its keys, stably sorted
    keys_by_id = np.zeros(n, np.uint64); keys_by_id[ids] = ks
    assert np.array_equal(ids, B.morton_order(keys_by_id))
    t = _radix_tree(ks, ids)
    assert not B.check_sorted_order(t, keys_by_id).failures
    rep = B.check_radix_tree(t, keys_by_id)
    assert not rep.failures and rep.counts["inner"] == n - 1
    # planted: two leaves swapped inside the run of equal keys — the tree over the same sorted keys is the same radix tree; the sort was not stable
    run = np.nonzero(ks == 77)[0]
    swapped = ids.copy(); swapped[[run[1], run[2]]] = swapped[[run[2], run[1]]]
    rep = B.check_sorted_order(_radix_tree(ks, swapped), keys_by_id)
    assert rep.failures and "not stable" in rep.failures[0], rep.failures
    assert not B.check_radix_tree(_radix_tree(ks, swapped), keys_by_id).failures
    # planted: a key out of order (a sort pass that lost a digit)
    lost = ids.copy(); lost[[3, 30]] = lost[[30, 3]]
    rep = B.check_sorted_order(_radix_tree(ks, lost), keys_by_id)
    assert rep.failures and "lost a digit" in rep.failures[0], rep.failures
    # planted: one split moved by one
    a, b = int(t.first[t.left[0]]), int(t.last[t.left[0]])
    assert b - a >= 3
    s = int(t.last[t.left[t.left[0]]])
    moved = _radix_tree(ks, ids, move_split=(a, b, 1 if s + 1 < b else -1))
    assert not B.check_sorted_order(moved, keys_by_id).failures
    rep = B.check_radix_tree(moved, keys_by_id)
    assert rep.failures and rep.failures[0].startswith("radix: node") and f"the radix tree splits after {s}" in rep.failures[0], rep.failures


def test_morton_keys_clamp_and_degenerate_axis():
    """the centre at the upper bound gives n = 1, s = 2^21: clamped to 2 097 151; an axis of no extent gives cell 0; the axes interleave x, y, z from the top"""
    lo = np.array([[0, 0, 5], [1, 2, 5], [0.5, 2, 5]], F32)
    keys, q = B.morton_keys(lo, lo + F32(1))
    assert q.tolist() == [[0, 0, 0], [2097151, 2097151, 0], [1048576, 2097151, 0]]
    assert int(keys[0]) == 0 and int(keys[1]) == 0x6DB6DB6DB6DB6DB6 and int(keys[2]) == (1 << 62) | 0x2492492492492492
    assert B._clz64(np.array([0, 1, 1 << 62, (1 << 64) - 1], np.uint64)).tolist() == [64, 63, 1, 0]


# ------------------------------------------------------------------------------------------------ the dumps' decoders, and the collapse's planted defects
def _encode_rope(tree):
    """rope nodes (N, 16) and packets (n, 12) as k_emit_nodes / k_emit_packets write them (boxes, a / b words, the id in packet word 3); escape links left 0"""
    N = len(tree.left)
    pre = B.preorder(tree)          # rows in preorder: the root is row 0
    wn = np.zeros((N, 16), np.uint32)
    wn[pre, 0:3] = tree.lo.view(np.uint32); wn[pre, 4:7] = tree.hi.view(np.uint32)
    leaf = tree.left < 0
    wn[pre, 3] = np.where(leaf, B.NODE_LEAF | tree.first, pre[tree.left]); wn[pre, 7] = np.where(leaf, 1, pre[tree.right])
    wp = np.zeros((tree.n, 12), np.uint32); wp[:, 3] = tree.order
    return wn, wp


def _encode_wide(wide):
    """8-wide nodes (W, 20) and packets as wide_of reads them: imask, child_base, tri_base and the meta bytes; boxes are not needed.  Children of a node get
    consecutive indices (wide_of's list is breadth first); packets are written in arrival order."""
    W = len(wide)
    wn = np.zeros((W, 20), np.uint32)
    ids = []
    for k, ch in enumerate(wide):
        inner = [c for leaf, c in ch if not leaf]
        if inner:
            assert inner == list(range(inner[0], inner[0] + len(inner)))
            wn[k, 4] = inner[0]
        wn[k, 5] = len(ids)
        off, imask = 0, 0
        meta = np.zeros(8, np.uint8)
        for sl, (leaf, c) in enumerate(ch):
            if leaf:
                meta[sl] = (len(c) << 5) | off; off += len(c); ids.extend(int(x) for x in c)
            else:
                imask |= 1 << sl
        wn[k, 3] = imask << 24
        wn[k, 6:8] = meta.view(np.uint32)
    wp = np.zeros((len(ids), 12), np.uint32); wp[:, 3] = ids
    return wn, wp


def _collapse_case():
    rng = np.random.default_rng(21)
    n = 60
    lo, hi = _boxes(rng, n)
    keys, _ = B.morton_keys(lo, hi)
    tree, _, _ = _ploc_tree(lo, hi, B.morton_order(keys), 16)
    return tree, B.optimal_collapse(tree, 1.0, 0.5, 4)


def test_the_decoders_read_what_the_layouts_hold():
    tree, opt = _collapse_case()
    wn, wp = _encode_rope(tree)
    back = B.binary_tree(wn, wp)
    assert np.array_equal(B.canonical(back)[0], B.canonical(tree)[0]) and np.array_equal(back.order, tree.order)
    wn[np.nonzero(wn[:, 3] & B.NODE_LEAF)[0][0], 7] = 2
    with pytest.raises(AssertionError, match="a leaf of 2 references"):
        B.binary_tree(wn, wp)
    col = B.unfold(tree, opt)
    wide = B.wide_of(*_encode_wide(B.as_wide(tree, col)))
    rep = B.match_collapse(tree, wide, 4)
    assert rep.cost == B.collapse_of(tree, *_encode_wide(B.as_wide(tree, col)), 4).cost
    assert not rep.failures and _close(rep.cost, opt.cost) and rep.counts["wide_nodes"] == len(col)


def test_collapse_of_prices_a_wide_node_that_opens_a_different_child():
    """valid, not optimal: the root's wide node opens one more child than the table decided (or, with all eight slots taken, keeps two siblings closed)"""
    tree, opt = _collapse_case()
    ch = B.unfold_node(tree, opt, int(tree.levels[0][0]), True)
    k = next(k for k, (leaf, c) in enumerate(ch) if tree.left[c] >= 0)
    c = ch[k][1]
    if len(ch) < 8:
        other = ch[:k] + [(bool(opt.dec[x, 1]), int(x)) for x in (tree.left[c], tree.right[c])] + ch[k + 1:]
    else:
        pairs = [(i, j) for i in range(8) for j in range(8) if i != j and any(tree.left[p] == ch[i][1] and tree.right[p] == ch[j][1] for p in range(len(tree.left)))]
        i, j = pairs[0]
        p = next(p for p in range(len(tree.left)) if tree.left[p] == ch[i][1] and tree.right[p] == ch[j][1])
        other = [x for q, x in enumerate(ch) if q not in (i, j)] + [(False, p)]
    assert sorted(x[1] for x in other) != sorted(x[1] for x in ch)
    col = B.unfold(tree, opt, root_children=other)
    rep = B.collapse_of(tree, *_encode_wide(B.as_wide(tree, col)), 4)
    assert not rep.failures, rep.failures
    eps = B.epsilon(tree.depth)
    assert rep.cost > opt.cost * (1 + eps) / (1 - eps), "the optimality bound of test_build_stages.py refuses it"
    assert _close(rep.cost, B.collapse_cost(tree, col))


def test_collapse_of_names_a_child_that_straddles_two_binary_subtrees():
    tree, opt = _collapse_case()
    col = B.unfold(tree, opt)
    wide = B.as_wide(tree, col)
    spans = {(int(a), int(b)) for a, b in zip(tree.first, tree.last)}
    for k, (f, ch) in enumerate(col):
        lv = sorted((int(tree.first[c]), int(tree.last[c]), j) for j, (leaf, c) in enumerate(ch) if leaf)
        hit = next(((x, y) for x, y in zip(lv, lv[1:]) if x[1] + 1 == y[0] and (x[0], y[1]) not in spans and y[1] - x[0] + 1 <= 4), None)
        if hit:
            break
    assert hit, "no two adjacent leaf children of different subtrees in this case"
    (a0, a1, i), (b0, b1, j) = hit
    merged = (True, np.concatenate([wide[k][i][1], wide[k][j][1]]))
    wide[k] = [merged if q == i else x for q, x in enumerate(wide[k]) if q != j]
    rep = B.match_collapse(tree, wide, 4)
    # (named where it is; the node that holds it then no longer covers its binary node, which is said too)
    assert len(rep.failures) == 2 and rep.failures[0].startswith(f"collapse child: wide node {k} child") and rep.failures[1].startswith(f"collapse partition: wide node {k} ") and rep.cost is None, rep.failures
    # and the two other failures, collected together: a leaf over five references, a node that lost a child
    cheap = B.optimal_collapse(tree, 1.0, 0.05, 4)          # triangle tests almost free: leaves of several references
    wide = B.as_wide(tree, B.unfold(tree, cheap))
    assert not B.match_collapse(tree, wide, 4, 1.0, 0.05).failures
    k, j = next((k, j) for k, ch in enumerate(wide) for j, (leaf, c) in enumerate(ch) if leaf and len(c) > 1)
    wide[k] = [x for q, x in enumerate(wide[k]) if q != j]
    rep = B.match_collapse(tree, wide, 1, 1.0, 0.05)
    assert any(f.startswith(f"collapse partition: wide node {k} ") for f in rep.failures) and rep.cost is None, rep.failures
    assert any(f.startswith("collapse leaf:") and "min(max_leaf, 4) = 1" in f for f in rep.failures), rep.failures
