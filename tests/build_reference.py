"""What the device build is DEFINED to make, in numpy: the stages of bvh_build.hip stated as properties and exact references, checked against the layouts the same
scene dumps (DeviceScene.read_layout; decoders of rope_audit.py and bvh_audit.py).  No device code, no oracle.  The audits say a tree is valid and its figures
truthful; this says it is the tree the builder's comments promise.  Nothing here depends on how nodes are numbered.

What makes a dump complete.  rope = 1, max_leaf = 1, presplit = 0: parts 8 and 9 hold the whole binary tree of the build (k_refit collapses nothing), k_emit_nodes
writes every box unrounded with the left child first, the packets lie in leaf order with the triangle id in word 3, and every leaf's box is k_flatten's padded box of
its triangle.  rope = 1 with cost_isect = 1e6 keeps the full binary tree under any max_leaf (ci * A * nt <= ct * A + ... never holds for boxes that do not coincide)
while the 8-wide layout beside it is the collapse of that very tree.

    tree = binary_tree(rope_nodes, rope_packets)        the ordered tree: per node leaf-rank range [first, last], children, box; order = triangle id per leaf rank
    keys, q = morton_keys(leaf_lo, leaf_hi)             k_morton + k_flatten's cbounds in float32, bit for bit (by triangle id)
    check_sorted_order(tree, keys)                      the leaf order is np.lexsort((id, key)): what a stable LSD radix sort over vals[gid] = gid gives
    check_radix_tree(tree, keys)                        builder 0: every inner node is the radix-tree node of its range (k_karras; equal keys augmented by position)
    ploc_topology(leaf_lo, leaf_hi, order, radius)      builder 1: the rounds of k_ploc_nn / k_ploc_merge / k_ploc_compact / k_ploc_tail -> (preorder leaf counts, leaf sequence, round per node)
    check_ploc(tree, leaf_lo, leaf_hi, order, radius)   the dumped tree is that tree
    opt = optimal_collapse(tree, c_node, c_tri, max_leaf)   the table C(n, 0..7) of the comment block "optimal 8-wide collapse" in float64; opt.cost = C(root, 1)
    greedy_collapse(tree)                               the greedy collapse of k_wide_level<false> (largest area first) over a tree whose leaves hold one reference
    wide_of(wnodes, wpackets, root)                     the emitted 8-wide tree as [(children)], a child = (True, ids) or (False, index of its wide node)
    collapse_of(tree, wnodes, wpackets, max_leaf, c_node, c_tri, root)   every wide child matched to a binary node by ids -> Report with .cost in the DP's metric
    match_collapse(tree, wide, ...)                     the same on wide_of's form (unfold / greedy_collapse through as_wide: how the CPU tests plant defects)
    epsilon(depth)                                      the float32 error of a device-side C entry: (1 + 2^-24)^(3 depth + 8) - 1

The DP's metric.  C(n, 1) = min(C_leaf, C_node), C_leaf = area * triangles * c_tri, C_node = area * c_node + the children's entries; area = 2 (dx dy + dy dz + dz dx).
A collapse costs the sum over wide nodes of area * c_node plus the sum over leaf children of area * nt * c_tri, areas in float64 from the binary tree's float32
boxes.  One convention: C(root, 1) may be C_leaf(root) — the whole scene one leaf (k_wide_level: "the whole scene is one leaf").  The layout still needs a node to hold
that leaf; the metric does not charge it, exactly as the table does not: a root node whose only child is a leaf over every reference costs C_leaf(root).
The constants are taken as the float32 values the library holds (0.3 is not a float32).
"""
from collections import namedtuple

import numpy as np

from bvh_audit import Report, decode_nodes
from rope_audit import NODE_INDEX_MASK, NODE_LEAF

F32 = np.float32
WIDE_N = 8
LEAF_LIMIT = 4          # a wide node addresses its leaf triangles with a 32-bit mask: min(max_leaf, 4)

Tree = namedtuple("Tree", "n left right first last lo hi order levels leaf_node depth")
Optimum = namedtuple("Optimum", "cost C dec limit")


# ------------------------------------------------------------------------------------------------ the ordered binary tree
def make_tree(left, right, root, gid, lo, hi):
    """An ordered binary tree from child arrays: left / right (N,) with -1 at leaves, gid (N,) the triangle id of a leaf, lo / hi (N, 3) float32 boxes (an inner
    node's row is overwritten with the union of its children's).  Nodes are renumbered nowhere; row `root` is the root.  Refuses a tree that is not one."""
    left = np.asarray(left, np.int64); right = np.asarray(right, np.int64); gid = np.asarray(gid, np.int64)
    lo = np.array(lo, F32).reshape(-1, 3); hi = np.array(hi, F32).reshape(-1, 3)
    N = len(left)
    leaf = left < 0
    levels, front, seen = [], np.array([root], np.int64), 0
    while len(front):
        seen += len(front)
        assert seen <= N, "a cycle or a shared child in the binary tree"
        levels.append(front)
        inner = front[~leaf[front]]
        front = np.concatenate([left[inner], right[inner]])
        assert np.all((front >= 0) & (front < N)), "a child index outside the tree"
    assert seen == N, f"{N - seen} nodes not reached from the root"
    first = np.zeros(N, np.int64); last = np.zeros(N, np.int64)
    # leaf ranks: the leaves in left-to-right order.  size = leaves below; rank of the first leaf from the parent's
    cnt = np.zeros(N, np.int64)
    for lv in reversed(levels):
        cnt[lv[leaf[lv]]] = 1
        I = lv[~leaf[lv]]
        cnt[I] = cnt[left[I]] + cnt[right[I]]
        lo[I] = np.minimum(lo[left[I]], lo[right[I]]); hi[I] = np.maximum(hi[left[I]], hi[right[I]])
    for lv in levels:
        I = lv[~leaf[lv]]
        first[left[I]] = first[I]; first[right[I]] = first[I] + cnt[left[I]]
    last = first + cnt - 1
    n = int(cnt[root])
    leaf_node = np.zeros(n, np.int64)
    L = np.nonzero(leaf)[0]
    leaf_node[first[L]] = L
    return Tree(n, left, right, first, last, lo, hi, gid[leaf_node], levels, leaf_node, len(levels) - 1)


def binary_tree(rope_nodes, rope_packets):
    """The ordered tree of one dumped rope tree (root = row 0, indices relative to it; a flattened scene's parts 8 and 9, or one BLAS's rows of them): per node its
    leaf-rank range [first, last], its children (left first, as k_emit_nodes writes them) and its box; order = the triangle id at every leaf rank (packet word 3).
    Refuses a tree with a leaf of more than one reference — the precondition of every check here — and one whose leaves' packet ranges are not its leaf ranks."""
    wn = np.ascontiguousarray(rope_nodes, np.uint32).reshape(-1, 16)
    wp = np.ascontiguousarray(rope_packets, np.uint32).reshape(-1, 12)
    a, b = wn[:, 3].astype(np.int64), wn[:, 7].astype(np.int64)
    leaf = (a & NODE_LEAF) != 0
    assert np.all(b[leaf] == 1), f"a leaf of {int(b[leaf].max())} references: the binary tree was collapsed (build with max_leaf = 1, or cost_isect = 1e6)"
    left = np.where(leaf, -1, a); right = np.where(leaf, -1, b & NODE_INDEX_MASK)
    pk = np.where(leaf, a & 0x7FFFFFFF, 0)
    assert np.all(pk[leaf] < len(wp)), "a leaf's packet outside the packets"
    gid = np.where(leaf, wp[np.minimum(pk, len(wp) - 1), 3].astype(np.int64), -1)
    t = make_tree(left, right, 0, gid, wn[:, 0:3].view(F32), wn[:, 4:7].view(F32))
    assert t.n == len(wp) and np.array_equal(pk[t.leaf_node], np.arange(t.n)), "the packets do not lie in the leaf order of the tree"
    assert np.all(t.lo == wn[:, 0:3].view(F32)) and np.all(t.hi == wn[:, 4:7].view(F32)), "an inner box that is not the union of its children's (rope_audit's check)"
    return t


def leaf_boxes(tree):
    """the leaves' boxes by triangle id (ids must be 0 .. n - 1, once each): k_flatten's padded boxes when the tree was built without pre-splitting"""
    assert np.array_equal(np.sort(tree.order), np.arange(tree.n)), "the ids of the leaves are not 0 .. n - 1, once each"
    lo = np.zeros((tree.n, 3), F32); hi = np.zeros((tree.n, 3), F32)
    lo[tree.order] = tree.lo[tree.leaf_node]; hi[tree.order] = tree.hi[tree.leaf_node]
    return lo, hi


def preorder(tree):
    """the preorder position of every node, the left subtree first (a subtree of c leaves has 2c - 1 nodes)"""
    pre = np.zeros(len(tree.left), np.int64)
    cnt = tree.last - tree.first + 1
    for lv in tree.levels:
        I = lv[tree.left[lv] >= 0]
        pre[tree.left[I]] = pre[I] + 1
        pre[tree.right[I]] = pre[I] + 2 * cnt[tree.left[I]]
    return pre


def canonical(tree):
    """(preorder list of subtree leaf counts, DFS leaf sequence as triangle ids): fixes an ordered binary tree whatever the node ids"""
    out = np.zeros(len(tree.left), np.int64)
    out[preorder(tree)] = tree.last - tree.first + 1
    return out, tree.order.copy()


# ------------------------------------------------------------------------------------------------ morton keys and the sort
def _spread21(x):
    x = x & np.uint64(0x1fffff)
    for s, m in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(s))) & np.uint64(m)
    return x


def morton_keys(leaf_lo, leaf_hi):
    """k_morton over k_flatten's centroid bounds, in float32 with one rounding per operation (the library is built with -ffp-contract=off): c = 0.5f * (lo + hi)
    of the padded box, cbounds = min / max of c, n = ext > 0 ? (c - mn) / ext : 0, s = n * 2097152 clamped to [0, 2097151], truncated, spread21, x << 2 | y << 1 | z.
    Returns (keys uint64 (n,), q int64 (n, 3) the 21-bit cells per axis)."""
    lo = np.asarray(leaf_lo, F32).reshape(-1, 3); hi = np.asarray(leaf_hi, F32).reshape(-1, 3)
    c = F32(0.5) * (lo + hi)
    mn, mx = c.min(0), c.max(0)
    ext = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(ext > 0, (c - mn) / ext, F32(0)).astype(F32)
    s = nrm * F32(2097152.0)
    s = np.minimum(np.maximum(s, F32(0)), F32(2097151.0))
    q = s.astype(np.int64)          # (uint64_t) s: truncation of a value in [0, 2097151]
    u = q.astype(np.uint64)
    keys = (_spread21(u[:, 0]) << np.uint64(2)) | (_spread21(u[:, 1]) << np.uint64(1)) | _spread21(u[:, 2])
    return keys, q


def morton_order(keys):
    """the order a stable sort by key leaves over vals[gid] = gid: by key, equal keys by ascending id"""
    return np.lexsort((np.arange(len(keys)), np.asarray(keys, np.uint64)))


def check_sorted_order(tree, keys):
    """The leaf order of the tree is np.lexsort((id, key)): keys non-decreasing, equal keys in ascending id order.  keys: by triangle id."""
    rep = Report()
    keys = np.asarray(keys, np.uint64)
    want = morton_order(keys)
    rep.counts.update(leaves=tree.n, equal_pairs=int((np.diff(np.sort(keys)) == 0).sum()))
    if np.array_equal(tree.order, want):
        return rep
    ks = keys[tree.order]
    for r in np.nonzero(ks[1:] < ks[:-1])[0][:5]:
        rep.fail(f"sorted: leaf ranks {r}, {r + 1} (ids {tree.order[r]}, {tree.order[r + 1]}): key {int(ks[r]):#x} before the smaller key {int(ks[r + 1]):#x}: a sort pass lost a digit")
    for r in np.nonzero((ks[1:] == ks[:-1]) & (tree.order[1:] < tree.order[:-1]))[0][:5]:
        rep.fail(f"sorted: leaf ranks {r}, {r + 1}: equal keys {int(ks[r]):#x} with id {tree.order[r]} before id {tree.order[r + 1]}: the sort is not stable")
    if not rep.failures:
        r = int(np.nonzero(tree.order != want)[0][0])
        rep.fail(f"sorted: leaf rank {r} holds id {tree.order[r]}, the sorted order has id {want[r]} there")
    return rep


def _clz64(x):
    """leading zeros of uint64 values (64 for 0)"""
    x = np.asarray(x, np.uint64).copy()
    n = np.zeros(x.shape, np.int64)
    zero = x == 0
    for s in (32, 16, 8, 4, 2, 1):
        m = x < (np.uint64(1) << np.uint64(64 - s))
        n += s * m
        x = np.where(m, x << np.uint64(s), x)
    return np.where(zero, 64, n)


def _delta(ks, i, j):
    """k_karras' delta_kr: common prefix length of the keys at sorted positions i, j; equal keys: 64 + that of the positions as 32-bit words"""
    a, b = ks[i], ks[j]
    eq = a == b
    pos = _clz64((np.asarray(i, np.int64) ^ np.asarray(j, np.int64)).astype(np.uint64)) - 32
    return np.where(eq, 64 + pos, _clz64(a ^ b))


def check_radix_tree(tree, keys):
    """Every inner node of a builder = 0 tree is the node of the binary radix tree over the position-augmented keys: spanning leaf ranks [a, b] and splitting after
    s, the common prefix of (s, s + 1) is exactly that of (a, b) — in sorted distinct keys that holds at one position of the range only, the one where the first
    differing bit turns from 0 to 1.  The root spans [0, n - 1].  keys: by triangle id."""
    rep = Report()
    ks = np.asarray(keys, np.uint64)[tree.order]
    I = np.nonzero(tree.left >= 0)[0]
    rep.counts.update(inner=int(len(I)))
    root = tree.levels[0][0]
    if (tree.first[root], tree.last[root]) != (0, tree.n - 1):
        rep.fail(f"radix: the root spans leaf ranks [{tree.first[root]}, {tree.last[root]}], not [0, {tree.n - 1}]")
    if not len(I):
        return rep
    a, b, s = tree.first[I], tree.last[I], tree.last[tree.left[I]]
    gap = tree.first[tree.right[I]] != s + 1
    for k in np.nonzero(gap)[0][:5]:
        rep.fail(f"radix: node {I[k]} [{a[k]}, {b[k]}]: its children do not meet (left ends at {s[k]}, right starts at {tree.first[tree.right[I[k]]]})")
    d_node, d_split = _delta(ks, a, b), _delta(ks, s, s + 1)
    for k in np.nonzero((d_node != d_split) & ~gap)[0][:10]:
        seg = np.arange(a[k], b[k])
        where = seg[_delta(ks, seg, seg + 1) == d_node[k]]
        rep.fail(f"radix: node {I[k]} over leaf ranks [{a[k]}, {b[k]}] splits after {s[k]} (common prefix {d_split[k]} bits there); the range shares {d_node[k]} bits"
                 + (f" and the radix tree splits after {where[0]}" if len(where) else ""))
    return rep


# ------------------------------------------------------------------------------------------------ PLOC
BIG = F32(3.0e38)


def ploc_rounds(lo, hi, radius, redirect=None):
    """The rounds of k_ploc_nn / k_ploc_merge / k_ploc_compact (and k_ploc_tail: "same rounds, same pairs, same order") over clusters lo / hi (m, 3) float32 in
    Morton order.  Each round: every cluster finds within +-radius positions the neighbour of least (dx*dy + dy*dz) + dz*dx of the union box, float32, strict <
    from the lowest position up (ties: the lowest position); mutual pairs merge, the lower position becomes the left child and keeps the place; survivors are
    compacted in order.  Leaves are nodes 0 .. m - 1 (positions), inner nodes m ...: returns (left, right, round_made, root).
    redirect (round, position): that cluster takes its second-nearest neighbour in that round — a planted defect for the tests of this module."""
    lo = np.array(lo, F32).reshape(-1, 3); hi = np.array(hi, F32).reshape(-1, 3)
    n = len(lo)
    left = np.full(2 * n - 1, -1, np.int64); right = np.full(2 * n - 1, -1, np.int64); made = np.zeros(2 * n - 1, np.int64)
    cid = np.arange(n)
    nxt, rnd = n, 0
    while len(cid) > 1:
        m = len(cid)
        best = np.full(m, BIG, F32); nn = np.full(m, -1, np.int64)
        R = min(int(radius), m - 1)
        area = {}
        for d in range(1, R + 1):
            dx = np.maximum(hi[:-d], hi[d:]) - np.minimum(lo[:-d], lo[d:])
            area[d] = (dx[:, 0] * dx[:, 1] + dx[:, 1] * dx[:, 2]) + dx[:, 2] * dx[:, 0]
        for d in list(range(-R, 0)) + list(range(1, R + 1)):          # j = i + d, from the lowest position up
            a = area[abs(d)]
            i = np.arange(-d, m) if d < 0 else np.arange(0, m - d)
            up = a < best[i]
            best[i] = np.where(up, a, best[i]); nn[i] = np.where(up, i + d, nn[i])
        if redirect is not None and redirect[0] == rnd:
            p = redirect[1]
            b2, j2 = BIG, -1
            for j in range(max(p - R, 0), min(p + R, m - 1) + 1):
                if j not in (p, nn[p]):
                    a = area[abs(j - p)][min(j, p)]
                    if a < b2:
                        b2, j2 = a, j
            if j2 >= 0:
                nn[p] = j2
        ok = nn >= 0
        mutual = ok & (nn[np.where(ok, nn, 0)] == np.arange(m))
        create = np.nonzero(mutual & (np.arange(m) < nn))[0]
        assert len(create), "PLOC made no progress: no mutual pair (boxes that compare false with everything)"
        j = nn[create]
        ids = nxt + np.arange(len(create))
        left[ids] = cid[create]; right[ids] = cid[j]; made[ids] = rnd
        nxt += len(create)
        lo[create] = np.minimum(lo[create], lo[j]); hi[create] = np.maximum(hi[create], hi[j])
        cid = cid.copy(); cid[create] = ids
        keep = ~(mutual & (np.arange(m) > nn))
        cid, lo, hi = cid[keep], lo[keep], hi[keep]
        rnd += 1
    return left, right, made, int(cid[0])


def ploc_topology(leaf_lo, leaf_hi, order, radius, redirect=None):
    """The PLOC tree over boxes leaf_lo / leaf_hi (by triangle id) taken in `order` (the Morton order).  Returns (preorder list of subtree leaf counts, DFS leaf
    sequence as triangle ids, preorder list of the round in which each inner node was made, -1 at leaves)."""
    order = np.asarray(order, np.int64)
    lo = np.asarray(leaf_lo, F32).reshape(-1, 3)[order]; hi = np.asarray(leaf_hi, F32).reshape(-1, 3)[order]
    n = len(order)
    if n == 1:
        return np.array([1]), order.copy(), np.array([-1])
    left, right, made, root = ploc_rounds(lo, hi, radius, redirect)
    gid = np.full(2 * n - 1, -1, np.int64); gid[:n] = order
    t = make_tree(left, right, root, gid, np.zeros((2 * n - 1, 3), F32), np.zeros((2 * n - 1, 3), F32))
    counts, seq = canonical(t)
    rounds = np.full(2 * n - 1, -1, np.int64)
    rounds[preorder(t)] = np.where(left >= 0, made, -1)
    return counts, seq, rounds


def check_ploc(tree, leaf_lo, leaf_hi, order, radius):
    """The dumped builder = 1 tree is ploc_topology's.  On a mismatch: the first differing preorder position, with the round in which the reference made that merge."""
    rep = Report()
    counts, seq, rounds = ploc_topology(leaf_lo, leaf_hi, order, radius)
    got_counts, got_seq = canonical(tree)
    rep.counts.update(leaves=tree.n, rounds=int(rounds.max()) + 1)
    if len(got_counts) != len(counts):
        rep.fail(f"ploc: the tree has {len(got_counts)} nodes, the reference {len(counts)}"); return rep
    bad = np.nonzero(got_counts != counts)[0]
    if len(bad):
        p = int(bad[0])
        rep.fail(f"ploc: preorder position {p}: a subtree of {got_counts[p]} leaves where the rounds as defined make one of {counts[p]}"
                 + (f" (merged in round {rounds[p]} of {int(rounds.max()) + 1})" if rounds[p] >= 0 else " (a leaf)") + f"; {len(bad)} positions differ")
    bad = np.nonzero(got_seq != seq)[0]
    if len(bad):
        r = int(bad[0])
        rep.fail(f"ploc: leaf rank {r} holds id {got_seq[r]}, the reference tree has id {seq[r]} there; {len(bad)} ranks differ")
    return rep


# ------------------------------------------------------------------------------------------------ the optimal 8-wide collapse
def areas(tree):
    """box_area of every node in float64 from the float32 boxes: 2 (dx dy + dy dz + dz dx)"""
    d = tree.hi.astype(np.float64) - tree.lo.astype(np.float64)
    return 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])


def epsilon(depth):
    """How far a device-side C entry may lie from its exact value, relatively: every entry is a sum of positive terms, and the longest chain of float32 roundings
    behind one has K = 3 depth + 8 steps — per level of the binary tree one addition (cl[k] + cr[i - k]), one product (area * c_node) and one addition, and for the
    leaf term and box_area the constant.  eps = (1 + 2^-24)^K - 1.  The device chooses by such costs: what it chose costs at most (1 + eps) / (1 - eps) times the
    optimum, and no collapse costs less than the optimum."""
    return (1.0 + 2.0 ** -24) ** (3 * depth + 8) - 1.0


def optimal_collapse(tree, c_node=1.0, c_tri=0.5, max_leaf=4):
    """The table of the comment block "optimal 8-wide collapse" (bvh_build.hip), float64: C[n, i], i = 1 .. 7, the least cost of n's subtree as a forest of at most
    i wide-BVH roots; C[n, 0] = C_node(n), the cost with n itself a wide node (inf at leaves).
        C(n, 1) = min(C_leaf, C_node), C_leaf = area * triangles * c_tri for subtrees of <= min(max_leaf, 4) triangles, C_node = area * c_node + min_k C(l, k) + C(r, 8 - k)
        C(n, i) = min(C(n, i - 1), min_k C(l, k) + C(r, i - k))
    dec keeps the arg-mins as wide_dp_node does (dec[n, 0] = k of C_node, dec[n, 1] = 1: the leaf, dec[n, i] = k or 0 for "i - 1 roots do as well").
    Returns Optimum(cost = C[root, 1], C, dec, limit)."""
    cn, ct = float(F32(c_node)), float(F32(c_tri))
    limit = min(int(max_leaf), LEAF_LIMIT)
    N = len(tree.left)
    A = areas(tree)
    nt = tree.last - tree.first + 1
    C = np.full((N, WIDE_N), np.inf); dec = np.zeros((N, WIDE_N), np.int64)
    for lv in reversed(tree.levels):
        L = lv[tree.left[lv] < 0]
        C[L, 1:] = (A[L] * ct)[:, None]; dec[L, 1] = 1
        I = lv[tree.left[lv] >= 0]
        if not len(I):
            continue
        cl, cr = C[tree.left[I]], C[tree.right[I]]
        def split(i):          # min over k = 1 .. i - 1 of cl[k] + cr[i - k], first arg-min
            cand = np.stack([cl[:, k] + cr[:, i - k] for k in range(1, i)], 1)
            k = cand.argmin(1)
            return cand[np.arange(len(I)), k], k + 1
        best, bk = split(WIDE_N)
        c_int = A[I] * cn + best
        c_leaf = np.where(nt[I] <= limit, A[I] * nt[I] * ct, np.inf)
        C[I, 0] = c_int; dec[I, 0] = bk
        C[I, 1] = np.minimum(c_leaf, c_int); dec[I, 1] = c_leaf <= c_int
        for i in range(2, WIDE_N):
            b, k = split(i)
            better = b < C[I, i - 1]
            C[I, i] = np.where(better, b, C[I, i - 1]); dec[I, i] = np.where(better, k, 0)
    return Optimum(float(C[tree.levels[0][0], 1]), C, dec, limit)


def _wide_from_children(tree, children_of_root_fn):
    """breadth first: [(binary node of the wide node, [(is_leaf, binary node)])] from a function giving a wide node's children"""
    root = int(tree.levels[0][0])
    out, queue = [], [root]
    while queue:
        f = queue.pop(0)
        ch = children_of_root_fn(f, f == root)
        out.append((f, ch))
        queue.extend(c for leaf, c in ch if not leaf)
    return out


def unfold_node(tree, opt, f, is_root=False):
    """the children of binary node f as a wide node, by the table's decisions: [(is_leaf, binary child)] (k_wide_level<true>'s stack of (node, roots allowed))"""
    dec = opt.dec
    if tree.left[f] < 0 or (is_root and dec[f, 1]):
        return [(True, f)]          # the whole scene is one leaf
    out = []
    stack = [(int(tree.right[f]), WIDE_N - int(dec[f, 0])), (int(tree.left[f]), int(dec[f, 0]))]
    while stack:
        c, b = stack.pop()
        while b > 1 and dec[c, b] == 0:
            b -= 1
        if b == 1:
            out.append((bool(dec[c, 1]), c))
        else:
            k = int(dec[c, b])
            stack.append((int(tree.right[c]), b - k)); stack.append((int(tree.left[c]), k))
    return out


def unfold(tree, opt, root_children=None):
    """The collapse the table's decisions stand for: [(binary node, [(is_leaf, binary child)])], the root's wide node first.  root_children: other children for
    the root's wide node (the nodes below still follow the table) — how the tests of this module plant a collapse that is valid and not optimal."""
    return _wide_from_children(tree, lambda f, is_root: root_children if (is_root and root_children is not None) else unfold_node(tree, opt, f, is_root))


def greedy_collapse(tree):
    """k_wide_level<false> over a binary tree whose leaves hold one reference each: open inner children, the largest float32 box_area first (the first of equals),
    until eight children or none left to open."""
    d = tree.hi - tree.lo
    a32 = F32(2) * ((d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0])
    def children(f, is_root):
        if tree.left[f] < 0:
            return [(True, f)]
        ch = [int(tree.left[f]), int(tree.right[f])]
        while len(ch) < WIDE_N:
            best, ba = -1, F32(-1)
            for k, c in enumerate(ch):
                if tree.left[c] >= 0 and a32[c] > ba:
                    ba, best = a32[c], k
            if best < 0:
                break
            c = ch[best]
            ch[best] = int(tree.left[c]); ch.append(int(tree.right[c]))
        return [(tree.left[c] < 0, c) for c in ch]
    return _wide_from_children(tree, children)


def collapse_cost(tree, collapse, c_node=1.0, c_tri=0.5):
    """the cost of a collapse given on binary nodes ([(binary node, [(is_leaf, binary child)])]) in the DP's metric (module docstring)"""
    cn, ct = float(F32(c_node)), float(F32(c_tri))
    A = areas(tree); nt = tree.last - tree.first + 1
    root = int(tree.levels[0][0])
    total = 0.0
    for f, ch in collapse:
        if not (f == root and len(ch) == 1 and ch[0] == (True, root)):
            total += A[f] * cn
        total += sum(A[c] * nt[c] * ct for leaf, c in ch if leaf)
    return float(total)


def as_wide(tree, collapse):
    """a collapse on binary nodes in wide_of's form: [(children)], a child = (True, ids) or (False, index of its wide node)"""
    index = {f: k for k, (f, ch) in enumerate(collapse)}
    return [[(True, tree.order[tree.first[c]:tree.last[c] + 1].copy()) if leaf else (False, index[c]) for leaf, c in ch] for f, ch in collapse]


def wide_of(wnodes, wpackets, root=0):
    """The emitted 8-wide tree under node `root` (a flattened scene's node 0, a BLAS's wroot): a list of wide nodes, the root's first, each a list of children in
    slot order — (True, triangle ids of its packets) for a leaf child, (False, index into this list) for an inner one.  Child nodes are child_base + rank among the
    set bits of imask; a leaf child's packets are tri_base + (meta & 31) .. + (meta >> 5), their ids word 3 of the packet.  Packets lie in arrival order."""
    D = decode_nodes(wnodes)
    wp = np.ascontiguousarray(wpackets, np.uint32)
    gid = wp[:, 3].astype(np.int64)
    index, nodes, out = {int(root): 0}, [int(root)], []
    k = 0
    while k < len(nodes):
        nd = nodes[k]; k += 1
        assert k <= D["n"], "a cycle in the 8-wide tree"
        ch, rank = [], 0
        for sl in range(8):
            m = int(D["meta"][nd, sl])
            if (int(D["imask"][nd]) >> sl) & 1:
                c = int(D["child_base"][nd]) + rank; rank += 1
                assert 0 <= c < D["n"] and c not in index, f"wide node {nd} slot {sl}: child {c} outside the array or reached twice"
                index[c] = len(nodes); nodes.append(c)
                ch.append((False, index[c]))
            elif m >> 5:
                p = int(D["tri_base"][nd]) + (m & 31)
                assert p + (m >> 5) <= len(gid), f"wide node {nd} slot {sl}: packets outside the array"
                ch.append((True, gid[p:p + (m >> 5)].copy()))
        out.append(ch)
    return out


def collapse_of(tree, wnodes, wpackets, max_leaf=4, c_node=1.0, c_tri=0.5, root=0):
    """match_collapse of the emitted 8-wide tree under node `root` of the dumped wnodes / wpackets (wide_of)"""
    return match_collapse(tree, wide_of(wnodes, wpackets, root), max_leaf, c_node, c_tri)


def match_collapse(tree, wide, max_leaf=4, c_node=1.0, c_tri=0.5):
    """Match every child of every wide node (wide_of's form) to a node of the binary tree — a leaf child through the ids of its packets, an inner child through the
    ids of everything below it — never by position.  Failures are collected (Report.failures):
      child      a child whose id set is not exactly one binary node's leaf set;
      partition  a wide node whose children do not partition its own binary node (the root's: the binary root);
      leaf       a leaf child over more than min(max_leaf, 4) references.
    Report.cost: the cost of the emitted collapse in the DP's metric (module docstring), float64 on the binary boxes; None when a child could not be matched.
    Report.counts: wide nodes, leaf children, the references of the largest leaf child."""
    rep = Report()
    rep.cost = None
    cn, ct = float(F32(c_node)), float(F32(c_tri))
    limit = min(int(max_leaf), LEAF_LIMIT)
    A = areas(tree)
    rank_of = np.full(int(tree.order.max()) + 1, -1, np.int64); rank_of[tree.order] = np.arange(tree.n)
    node_at = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(tree.first, tree.last))}
    W = len(wide)
    ids = [None] * W
    for k in range(W - 1, -1, -1):          # (children come after their parents in wide_of's list)
        parts = [c if leaf else ids[c] for leaf, c in wide[k]]
        ids[k] = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    def match(s):
        s = np.asarray(s, np.int64)
        if not len(s) or s.min() < 0 or s.max() >= len(rank_of) or (rank_of[s] < 0).any():
            return None
        r = rank_of[s]
        if len(np.unique(r)) != len(r) or r.max() - r.min() + 1 != len(r):
            return None
        return node_at.get((int(r.min()), int(r.max())))
    root = int(tree.levels[0][0])
    own = [None] * W; own[0] = root
    cost, ok = 0.0, True
    leaves = largest = 0
    for k, ch in enumerate(wide):
        nodes = []
        for j, (leaf, c) in enumerate(ch):
            s = c if leaf else ids[c]
            b = match(s)
            if b is None:
                rep.fail(f"collapse child: wide node {k} child {j} ({'leaf' if leaf else 'inner'}, {len(s)} ids, e.g. {np.sort(np.asarray(s))[:6].tolist()}): its ids are not the leaf set of one binary node")
                ok = False; continue
            nodes.append(b)
            if leaf:
                leaves += 1; largest = max(largest, len(s))
                if len(s) > limit:
                    rep.fail(f"collapse leaf: wide node {k} child {j}: a leaf over {len(s)} references, more than min(max_leaf, 4) = {limit}")
                cost += A[b] * len(s) * ct
            else:
                own[c] = b
        if own[k] is None:
            continue          # (its parent could not match it: reported there)
        me = own[k]
        spans = sorted((int(tree.first[b]), int(tree.last[b])) for b in nodes)
        covered = len(nodes) == len(ch) and len(spans) > 0 and spans[0][0] == tree.first[me] and spans[-1][1] == tree.last[me] and all(x[1] + 1 == y[0] for x, y in zip(spans, spans[1:]))
        if not covered:
            rep.fail(f"collapse partition: wide node {k} stands for binary node {me} (leaf ranks [{tree.first[me]}, {tree.last[me]}]); its children cover {spans}")
            ok = False
        if not (k == 0 and len(ch) == 1 and ch[0][0] and len(nodes) == 1 and nodes[0] == root):
            cost += A[me] * cn
    rep.counts.update(wide_nodes=W, leaf_children=leaves, largest_leaf=largest)
    if ok:
        rep.cost = float(cost)
    return rep
