"""The rope audit (tests/rope_audit.py) on trees made here, in host memory: random valid trees pass; one wrong word in one node of a copy is reported
with that node named.  The generator gets its escape links another way than the audit's parent / child rule: for every octant it walks the tree
depth first in that octant's order and notes, for each node, the node visited after its subtree.  Nothing here is ever given to a kernel."""
import re
import time

import numpy as np
import pytest

import bvh_audit as A
import rope_audit as R

LEAF, TERM, MASK = R.NODE_LEAF, R.NODE_TERM, R.NODE_INDEX_MASK


# ------------------------------------------------------------------------------------------------ generator
def _below(x):
    """the largest float32 <= x (float64), per element"""
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def _above(x):
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def _topology(rng, leaves, shape):
    """left / right child per node (-1: leaf), nodes numbered at random with the root at 0"""
    left, right = [-1], [-1]
    open_ = [0]
    while len(open_) < leaves:          # (the open nodes are the leaves so far)
        k = len(open_) - 1 if shape == "chain" else int(rng.integers(len(open_)))
        nd = open_.pop(k)
        left[nd], right[nd] = len(left), len(left) + 1
        left += [-1, -1]; right += [-1, -1]
        new = [left[nd], right[nd]]
        if shape == "chain":
            new = new[::-1] if rng.random() < 0.5 else new          # the chain goes on under either child
        open_ += new
    n = len(left)
    perm = np.r_[0, 1 + rng.permutation(n - 1)] if n > 1 else np.zeros(1, np.int64)
    L, Rr = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for old in range(n):
        if left[old] >= 0:
            L[perm[old]], Rr[perm[old]] = perm[left[old]], perm[right[old]]
    return L, Rr


def _escapes(L, Rr, mask):
    """per node and octant: the node an ordered depth-first walk visits after the node's subtree (TERM after the last)"""
    n = len(L)
    esc = np.full((n, 8), TERM, np.uint32)
    for o in range(8):
        order, stack = [], [0]
        while stack:
            nd = stack.pop()
            order.append(nd)
            if L[nd] >= 0:
                near, far = (Rr[nd], L[nd]) if (mask[nd] >> o) & 1 else (L[nd], Rr[nd])
                stack += [far, near]
        where = np.empty(n, np.int64); where[order] = np.arange(n)
        size = np.ones(n, np.int64)
        for nd in reversed(order):                # a preorder reversed: children before parents
            if L[nd] >= 0:
                size[nd] += size[L[nd]] + size[Rr[nd]]
        after = where + size
        order = np.array(order)
        esc[:, o] = np.where(after < n, order[np.minimum(after, n - 1)], TERM)
    return esc


def make_tree(seed, leaves, shape="random", max_leaf=3):
    """a valid flattened rope layout: dict(header, rope_nodes, rope_packets) and num_tris"""
    rng = np.random.default_rng(seed)
    L, Rr = _topology(rng, leaves, shape)
    n = len(L)
    is_leaf = L < 0
    lv = np.nonzero(is_leaf)[0]
    cnt = rng.integers(1, max_leaf + 1, len(lv))
    T = int(cnt.sum())
    first = np.zeros(len(lv), np.int64)
    slot = rng.permutation(len(lv))                                  # the leaves' ranges in an order of their own
    first[slot] = np.cumsum(cnt[slot]) - cnt[slot]
    # triangles: float32 v0, e1, e2 near a centre per leaf, at scales from 1e-3 to 1e3
    c = rng.uniform(-1, 1, (len(lv), 3)) * 10.0 ** rng.uniform(-3, 3, (len(lv), 1))
    pk = np.zeros((T, 12), np.uint32)
    gids = rng.permutation(T)
    lo = np.zeros((n, 3), np.float32); hi = np.zeros((n, 3), np.float32)
    for k, nd in enumerate(lv):
        rows = np.arange(first[k], first[k] + cnt[k])
        v0 = (c[k] + rng.normal(size=(cnt[k], 3)) * np.abs(c[k]).max() * 0.1).astype(np.float32)
        e = (rng.normal(size=(cnt[k], 2, 3)) * np.abs(c[k]).max() * 0.1).astype(np.float32)
        pk[rows, 0:3] = v0.view(np.uint32); pk[rows, 3] = gids[rows]
        pk[rows, 4:7] = e[:, 0].view(np.uint32); pk[rows, 8:11] = e[:, 1].view(np.uint32)
        V = np.stack([v0.astype(np.float64), v0.astype(np.float64) + e[:, 0], v0.astype(np.float64) + e[:, 1]], 1)
        tlo, thi = V.min(1), V.max(1)
        pad = A.pad_of(np.maximum(np.abs(tlo), np.abs(thi)))
        lo[nd] = _below((tlo - pad).min(0)); hi[nd] = _above((thi + pad).max(0))
    mask = rng.integers(0, 256, n)
    depth_order, stack = [], [0]
    while stack:
        nd = stack.pop(); depth_order.append(nd)
        if L[nd] >= 0: stack += [L[nd], Rr[nd]]
    for nd in reversed(depth_order):
        if L[nd] >= 0:
            lo[nd] = np.minimum(lo[L[nd]], lo[Rr[nd]]); hi[nd] = np.maximum(hi[L[nd]], hi[Rr[nd]])
    wn = np.zeros((n, 16), np.uint32)
    wn[:, 0:3] = lo.view(np.uint32); wn[:, 4:7] = hi.view(np.uint32)
    wn[lv, 3] = LEAF | first.astype(np.uint32); wn[lv, 7] = cnt
    inner = np.nonzero(~is_leaf)[0]
    wn[inner, 3] = L[inner]; wn[inner, 7] = (mask[inner].astype(np.uint32) << 24) | Rr[inner].astype(np.uint32)
    wn[:, 8:16] = _escapes(L, Rr, mask)
    return dict(header=np.zeros(8, np.uint32), rope_nodes=wn, rope_packets=pk), T


def _copy(lay):
    return {k: np.array(v) for k, v in lay.items()}


def _f32(word):
    return np.array([word], np.uint32).view(np.float32)[0]


def _u32(value):
    return np.array([value], np.float32).view(np.uint32)[0]


def _named(rep, check, *names):
    """some failure of that check names every one of the given things ("node 7", "packet 3", "octant 2")"""
    hits = [f for f in rep.failures if f.startswith(check) and all(re.search(rf"\b{re.escape(n)}\b", f) for n in names)]
    assert hits, f"no '{check}' failure naming {names} among:\n" + "\n".join(rep.failures[:20])
    return hits


def _inner(lay):
    return np.nonzero((lay["rope_nodes"][:, 3] & LEAF) == 0)[0]


def _leaves(lay):
    return np.nonzero((lay["rope_nodes"][:, 3] & LEAF) != 0)[0]


def _subtree(lay, nd):
    out, stack = [], [int(nd)]
    while stack:
        x = stack.pop(); out.append(x)
        if not lay["rope_nodes"][x, 3] & LEAF:
            stack += [int(lay["rope_nodes"][x, 3]), int(lay["rope_nodes"][x, 7] & MASK)]
    return out


# ------------------------------------------------------------------------------------------------ clean trees
@pytest.mark.parametrize("leaves,shape", [(1, "random"), (2, "random"), (3, "random"), (17, "random"), (200, "random"), (60, "chain"), (200, "chain")])
def test_clean_trees_pass(leaves, shape):
    for seed in range(4):
        lay, T = make_tree(100 * leaves + seed, leaves, shape)
        rep = R.audit(lay, presplit=False, num_tris=T)
        rep.check()
        n = len(lay["rope_nodes"])
        assert n == 2 * leaves - 1 and rep.counts == dict(nodes=n, leaves=leaves, packets=T, trees=1, pad_excused=0)
        assert rep.margins["pad"]["min_pad_frac"] >= 0.5
        R.links_kept(lay, _copy(lay)).check()


def test_the_one_leaf_tree_is_a_root_with_eight_terminal_links():
    lay, T = make_tree(1, 1)
    assert len(lay["rope_nodes"]) == 1 and lay["rope_nodes"][0, 3] & LEAF and (lay["rope_nodes"][0, 8:16] == TERM).all()
    R.audit(lay, num_tris=T).check()
    m = _copy(lay); m["rope_nodes"][0, 8 + 5] = 0
    _named(R.audit(m, num_tris=T), "escape", "node 0", "octant 5")


def test_the_chain_is_as_deep_as_it_has_leaves():
    lay, T = make_tree(7, 120, "chain")
    depth, nd = 1, 0
    while not lay["rope_nodes"][nd, 3] & LEAF:
        a, b = int(lay["rope_nodes"][nd, 3]), int(lay["rope_nodes"][nd, 7] & MASK)
        nd = a if not lay["rope_nodes"][a, 3] & LEAF else b
        depth += 1
    assert depth == 120


def test_a_large_tree_audits_quickly():
    lay, T = make_tree(3, 20000)
    t0 = time.perf_counter()
    rep = R.audit(lay, num_tris=T)
    dt = time.perf_counter() - t0
    rep.check()
    print(f"{rep.counts} audited in {dt:.2f} s")
    assert rep.counts["nodes"] == 39999 and dt < 10.0          # (about a second; the bound only guards against a quadratic step)


def test_the_empty_layout_is_reported():
    lay = dict(header=np.zeros(8, np.uint32), rope_nodes=np.zeros((0, 16), np.uint32), rope_packets=np.zeros((0, 12), np.uint32))
    assert R.audit(lay).failures == ["structure: no rope layout"]


# ------------------------------------------------------------------------------------------------ mutations: one word of one node of a copy
CASES = [(seed, leaves, shape) for seed, (leaves, shape) in enumerate([(2, "random"), (3, "random"), (9, "random"), (40, "random"), (200, "random"), (30, "chain")])]


@pytest.fixture(params=CASES, ids=lambda c: f"{c[1]}{c[2]}")
def tree(request):
    seed, leaves, shape = request.param
    lay, T = make_tree(900 + seed, leaves, shape)
    R.audit(lay, num_tris=T).check()
    return lay, T, np.random.default_rng(seed)


def test_an_escape_link_to_another_valid_node(tree):
    lay, T, rng = tree
    n = len(lay["rope_nodes"])
    for _ in range(8):
        m = _copy(lay)
        nd, o = int(rng.integers(1, n)), int(rng.integers(8))
        other = [x for x in range(n) if x != m["rope_nodes"][nd, 8 + o]]
        m["rope_nodes"][nd, 8 + o] = other[int(rng.integers(len(other)))]
        rep = R.audit(m, num_tris=T)
        _named(rep, "escape", f"node {nd}", f"octant {o}")
        assert all(f.startswith("escape") and f"octant {o}" in f for f in rep.failures), rep.failures
        _named(R.links_kept(lay, m), "links_kept", f"node {nd}", f"octant {o}")


def test_an_escape_link_into_the_node_s_own_subtree(tree):
    """a cycle for the rays of that octant: reported, and the audit returns"""
    lay, T, rng = tree
    for nd in _inner(lay)[:6]:
        m = _copy(lay)
        o = int(rng.integers(8))
        sub = _subtree(lay, nd)
        m["rope_nodes"][nd, 8 + o] = sub[int(rng.integers(len(sub)))]
        _named(R.audit(m, num_tris=T), "escape", f"node {nd}", f"octant {o}")


def test_a_child_link_back_to_an_ancestor(tree):
    """a cycle in the tree itself: the walk expands no node twice"""
    lay, T, rng = tree
    nd = int(_inner(lay)[-1])
    m = _copy(lay)
    m["rope_nodes"][nd, 3] = 0
    rep = R.audit(m, num_tris=T)
    _named(rep, "structure", "node 0", "reached 2 times")


def test_a_parent_box_one_ulp_low_on_its_high_side(tree):
    lay, T, rng = tree
    for nd in rng.permutation(_inner(lay))[:6]:
        for ax in range(3):
            m = _copy(lay)
            m["rope_nodes"][nd, 4 + ax] = _u32(np.nextafter(_f32(lay["rope_nodes"][nd, 4 + ax]), np.float32(-np.inf)))
            rep = R.audit(m, num_tris=T)
            _named(rep, "union", f"node {nd}", f"axis {'xyz'[ax]} hi")
            assert all(f.startswith("union") for f in rep.failures), rep.failures          # (its own parent may notice too; nothing else does)
            R.links_kept(lay, m).check()                                                     # boxes are the refit's to write


@pytest.mark.parametrize("step", [1, -1])
def test_a_leaf_count_off_by_one(tree, step):
    lay, T, rng = tree
    for nd in rng.permutation(_leaves(lay))[:6]:
        m = _copy(lay)
        m["rope_nodes"][nd, 7] = int(lay["rope_nodes"][nd, 7]) + step
        _named(R.audit(m, num_tris=T), "structure", f"node {nd}")
        _named(R.links_kept(lay, m), "links_kept", f"node {nd}", "word 7")


def test_a_packet_referenced_by_two_leaves(tree):
    lay, T, rng = tree
    x, y = rng.permutation(_leaves(lay))[:2]
    m = _copy(lay)
    m["rope_nodes"][x, 3] = lay["rope_nodes"][y, 3]; m["rope_nodes"][x, 7] = 1
    shared = int(lay["rope_nodes"][y, 3] & 0x7FFFFFFF)
    _named(R.audit(m, num_tris=T), "structure", f"packet {shared}", f"node {x}", f"node {y}", "referenced by 2 leaves")


def test_a_child_index_beyond_the_array(tree):
    lay, T, rng = tree
    n = len(lay["rope_nodes"])
    for nd in rng.permutation(_inner(lay))[:4]:
        for word, value in ((3, n), (3, MASK), (7, (int(lay["rope_nodes"][nd, 7]) & ~MASK) | (n + 5))):
            m = _copy(lay)
            m["rope_nodes"][nd, word] = value
            _named(R.audit(m, num_tris=T), "structure", f"node {nd}", "child index")


def test_a_triangle_id_missing(tree):
    lay, T, rng = tree
    m = _copy(lay)
    j, k = rng.permutation(T)[:2]
    gone, twice = int(lay["rope_packets"][j, 3]), int(lay["rope_packets"][k, 3])
    m["rope_packets"][j, 3] = twice
    rep = R.audit(m, presplit=False, num_tris=T)
    _named(rep, "structure", f"triangle {gone}", "referenced by no packet")
    _named(rep, "structure", f"triangle {twice}", "referenced by 2 packets")
    _named(rep, "pad", "excused")                                   # nothing may be excused from the pad check without pre-splitting
    _named(R.audit(m, presplit=True, num_tris=T), "structure", f"triangle {gone}")
    _named(R.links_kept(lay, m), "links_kept", f"packet {j}")
    # the last id missing when the audit is not told how many triangles there are: the duplicate still gives it away
    assert R.audit(m, presplit=False).failures


def test_a_leaf_box_one_ulp_inside_its_triangle(tree):
    lay, T, rng = tree
    V, gid = A.decode_packets(lay["rope_packets"])
    for nd in rng.permutation(_leaves(lay))[:6]:
        first, cnt = int(lay["rope_nodes"][nd, 3] & 0x7FFFFFFF), int(lay["rope_nodes"][nd, 7])
        for ax in range(3):
            for side, word in (("lo", ax), ("hi", 4 + ax)):
                tv = V[first:first + cnt, :, ax]
                j = first + int(np.argmin(tv.min(1)) if side == "lo" else np.argmax(tv.max(1)))
                edge = tv.min() if side == "lo" else tv.max()
                f = np.float32(edge)                                   # the first float32 strictly inside the triangle's extreme
                if side == "lo" and not f > edge: f = np.nextafter(f, np.float32(np.inf))
                if side == "hi" and not f < edge: f = np.nextafter(f, np.float32(-np.inf))
                m = _copy(lay)
                m["rope_nodes"][nd, word] = _u32(f)
                _named(R.audit(m, num_tris=T), "contain", f"packet {j}", f"node {nd}", f"axis {'xyz'[ax]} {side}")


def test_a_leaf_box_that_lost_its_pad(tree):
    """exactly on the triangle: contained, and reported by the pad check"""
    lay, T, rng = tree
    V, gid = A.decode_packets(lay["rope_packets"])
    nd = int(_leaves(lay)[0])
    first, cnt = int(lay["rope_nodes"][nd, 3] & 0x7FFFFFFF), int(lay["rope_nodes"][nd, 7])
    m = _copy(lay)
    m["rope_nodes"][nd, 0] = _u32(_below(V[first:first + cnt, :, 0].min()))
    rep = R.audit(m, num_tris=T)
    _named(rep, "pad", f"node {nd}", "axis x lo")
    assert not [f for f in rep.failures if f.startswith("contain")]


def test_a_mask_bit_changed_with_the_links_left_as_they_were(tree):
    lay, T, rng = tree
    for nd in rng.permutation(_inner(lay))[:6]:
        o = int(rng.integers(8))
        m = _copy(lay)
        m["rope_nodes"][nd, 7] ^= np.uint32(1 << (24 + o))
        rep = R.audit(m, num_tris=T)
        _named(rep, "escape", f"node {nd}", f"octant {o}")
        assert all(f.startswith("escape") and f"octant {o}" in f and re.search(rf"\bnode {nd}\b", f) for f in rep.failures), rep.failures
        _named(R.links_kept(lay, m), "links_kept", f"node {nd}", "word 7")


# ------------------------------------------------------------------------------------------------ two-level form and pre-split references
def _two_level(seed):
    """three BLASes behind each other (the middle one a single leaf), five instances; indices inside a BLAS relative to its bases"""
    parts = [make_tree(seed + k, leaves) for k, leaves in enumerate((5, 1, 12))]
    nodes = np.vstack([p[0]["rope_nodes"] for p in parts]); packets = np.vstack([p[0]["rope_packets"] for p in parts])
    nb = np.cumsum([0] + [len(p[0]["rope_nodes"]) for p in parts]); pb = np.cumsum([0] + [p[1] for p in parts])
    rows = np.zeros((5, 20), np.uint32)
    for i, bl in enumerate((0, 1, 2, 0, 2)):
        rows[i, 12], rows[i, 13], rows[i, 17], rows[i, 18] = nb[bl], pb[bl], parts[bl][1], bl
    hdr = np.zeros(8, np.uint32); hdr[2] = 5
    return dict(header=hdr, rope_nodes=nodes, rope_packets=packets, instances=rows), nb, pb


def test_a_two_level_layout_is_one_tree_per_blas_with_relative_indices():
    lay, nb, pb = _two_level(40)
    rep = R.audit(lay)
    rep.check()
    assert rep.counts == dict(nodes=int(nb[-1]), leaves=18, packets=int(pb[-1]), trees=3, pad_excused=0)
    # a child index written absolute in the last BLAS
    nd = int(nb[2] + _inner(dict(rope_nodes=lay["rope_nodes"][nb[2]:]))[0])
    m = _copy(lay); m["rope_nodes"][nd, 3] += np.uint32(nb[2])
    assert any("BLAS 2" in f for f in R.audit(m).failures)
    # an escape link that leaves its BLAS
    m = _copy(lay); m["rope_nodes"][nb[0] + 1, 8] = np.uint32(nb[1])
    _named(R.audit(m), "escape", "BLAS 0", f"node {nb[0] + 1}", "octant 0")
    # two instances of one BLAS naming different roots
    m = _copy(lay); m["instances"][3, 12] = 1
    _named(R.audit(m), "structure", "BLAS 0", "node_base")
    # a packet id of the neighbouring BLAS's numbering
    m = _copy(lay); m["rope_packets"][pb[1], 3] = 3
    _named(R.audit(m), "structure", "BLAS 1", f"packet {pb[1]}")
    # a node no BLAS reaches: the part is longer than the trees
    m = _copy(lay); m["rope_nodes"] = np.vstack([lay["rope_nodes"], lay["rope_nodes"][-1:]])
    _named(R.audit(m), "structure", f"node {nb[-1]}", "never reached")


def _presplit_pair():
    """one long triangle as two references in two leaves, each box the padded clipped piece (as k_split_emit makes them), and an ordinary third leaf"""
    v = np.array([[0, 0, 0], [8, 0.5, 0], [0, 1, 0.25]], np.float32)
    other = np.array([[1, 2, 1], [2, 2, 1], [1, 3, 1.5]], np.float32)
    pk = np.zeros((3, 12), np.uint32)
    for j, (t, g) in enumerate(((v, 0), (v, 0), (other, 1))):
        pk[j, 0:3] = t[0].view(np.uint32); pk[j, 3] = g; pk[j, 4:7] = (t[1] - t[0]).view(np.uint32); pk[j, 8:11] = (t[2] - t[0]).view(np.uint32)
    wn = np.zeros((5, 16), np.uint32)
    boxes = [A._clip_extent(v.astype(np.float64), 0, 0.0, 3.0), A._clip_extent(v.astype(np.float64), 0, 3.0, 8.0), (other.min(0).astype(np.float64), other.max(0).astype(np.float64))]
    for nd, j in ((2, 0), (3, 1), (4, 2)):
        lo, hi = boxes[j]
        pad = A.pad_of(np.maximum(np.abs(lo), np.abs(hi)))
        wn[nd, 0:3] = _below(lo - pad).view(np.uint32); wn[nd, 4:7] = _above(hi + pad).view(np.uint32)
        wn[nd, 3] = LEAF | j; wn[nd, 7] = 1
    f = lambda nd, w: wn[nd, w:w + 3].view(np.float32)
    for nd, (l, r) in ((1, (2, 3)), (0, (1, 4))):          # node 0 = {node 1 = {2, 3}, 4}, every mask 0: left first
        wn[nd, 0:3] = np.minimum(f(l, 0), f(r, 0)).view(np.uint32); wn[nd, 4:7] = np.maximum(f(l, 4), f(r, 4)).view(np.uint32)
        wn[nd, 3] = l; wn[nd, 7] = r
    wn[:, 8:16] = np.array([TERM, 4, 3, 4, TERM], np.uint32)[:, None]
    return dict(header=np.zeros(8, np.uint32), rope_nodes=wn, rope_packets=pk)


def test_pre_split_references_are_checked_by_their_clipped_piece():
    lay = _presplit_pair()
    rep = R.audit(lay, presplit=True, num_tris=2)
    rep.check()
    assert rep.counts["pad_excused"] == 2 and "split" in rep.margins
    off = R.audit(lay, presplit=False, num_tris=2)
    _named(off, "structure", "triangle 0", "referenced by 2 packets")
    _named(off, "pad", "2 packets excused")
    # the second reference's box pulled in past its share of the triangle
    m = _copy(lay)
    m["rope_nodes"][3, 0] = _u32(np.float32(3.5))
    _named(R.audit(m, presplit=True, num_tris=2), "split", "triangle 0")
    # ... and its far end short of the triangle's
    m = _copy(lay)
    m["rope_nodes"][3, 4] = _u32(np.float32(7.5))
    assert [f for f in R.audit(m, presplit=True, num_tris=2).failures if f.startswith("split")]


def test_bvh_audit_s_own_split_check_is_what_it_was():
    """check_split was factored out of bvh_audit.audit for both audits to use: same verdicts and words on a hand-made pair of references"""
    rep = A.Report()
    v = np.array([[0, 0, 0], [8, 0.5, 0], [0, 1, 0.25]], np.float64)
    lo = np.array([[-0.1, -0.1, -0.1], [2.9, -0.1, -0.1]]); hi = np.array([[3.1, 1.1, 0.3], [8.1, 1.1, 0.3]])
    chain = lambda j: (((10 + j, j), lo[j], hi[j]),)
    name = lambda tag: f"node {tag[0]} slot {tag[1]}"
    A.check_split(rep, 5, np.array([20, 21]), v, lo, hi, chain, name)
    assert not rep.failures and rep.margins["split"]["where"].startswith("triangle 5 packet 2")
    lo3 = lo.copy(); lo3[1, 1] = 0.4
    rep = A.Report()
    A.check_split(rep, 5, np.array([20, 21]), v, lo3, hi, lambda j: (((10 + j, j), lo3[j], hi[j]),), name)
    assert len(rep.failures) == 1 and re.match(r"split: triangle 5 clipped to reference packet 21's share of axis x leaves node 11 slot 1 on axis y by ", rep.failures[0])
