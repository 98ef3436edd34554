"""Recount, in numpy, of the tree figures MRTSceneStats reports and the refit policy acts on — from the layout the same scene dumps
(DeviceScene.read_layout; decoders of bvh_audit.py and rope_audit.py).  No device code, no oracle.

Every figure comes twice:
  emulation   the device's own operations in the device's precision and order (float32 with one rounding per operation: the library is built with
              -ffp-contract=off; an fma is ONE rounding of the exact p + q * 2^e).  What stays free is the order of the float64 atomic additions
              (relative 1e-16 per term), which can move a final float32 rounding across a tie: the library must agree within an ulp or two.
  meaning     exact float64 arithmetic on the exactly decoded planes, with a rigorous bound on how far the float32 evaluation may lie from it:
              half a float32 ulp of the coordinate per decoded plane, one rounding per float32 operation, propagated through area and sum.

    wide_cost(wnodes, first, count, root, c_node, c_tri)      k_wide_cost + wide_tree_cost (bvh_refit.hip)            -> Cost(emu, exact, bound)
    scene_wide_cost(lay, c_node, c_tri)                       flat: the tree at node 0; two-level: mean over the BLASes -> Cost, [Cost per BLAS]
    leaf_growth(before, after, gids, lo, hi, moved, previous) k_refit_wide_level's growth sums + k_refit_fold              -> Growth(emu, ratio_exact, rel_bound)
    unmoved_leaf_excess(before, after, gids, lo, hi, moved)   a leaf none of whose triangles moved keeps its (possibly clipped) box      -> slots, failures, clipped
    padded_boxes(tri)                                         k_flatten's leaf boxes under the identity (build_common.h)
    histogram(wnodes)                                         the 12 words of k_wide_histogram
    wide_depth(lay)                                           levels actually present (two-level: TLAS levels + 1 + the deepest BLAS)
    binary_figures(rope_nodes, ct, ci, max_leaf)              k_refit / k_assign / k_build_summary on one rope tree      -> Binary
    scene_bytes(header, stats, rope_nodes, rope_packets)      the sums of bvh_build.hip finish_tree / emit_wide / emit_rope and two_level.hip build_two_level
Nothing here depends on which tree a builder chose or on how the nodes of a level are numbered."""
import math
from collections import namedtuple

import numpy as np

from bvh_audit import decode_instances, decode_nodes
from rope_audit import NODE_INDEX_MASK, NODE_LEAF

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32

Cost = namedtuple("Cost", "emu exact bound sum32 sum64 area_root")          # emu: float32 as the library computes it; exact: float64; bound: |float32 evaluation - exact| <=
Growth = namedtuple("Growth", "emu ratio32 ratio_exact rel_bound g_old g_new slots")
Binary = namedtuple("Binary", "nodes leaves depth largest_leaf sah32 sah64 violations cost_root32 area_root32")


# ------------------------------------------------------------------------------------------------ float32 building blocks
def round_sum32(a, b):
    """float32(a + b) with ONE rounding of the exact sum, a and b float64 arrays (what a float32 fma leaves when b is an exact product).  A plain float64 sum
    rounds twice when the exponents are far apart; here the float64 sum is made round-to-odd from its exact remainder (TwoSum) first, after which the
    rounding to 24 bits is that of the exact value (53 >= 24 + 2)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    odd = (s.view(np.int64) & 1) != 0
    toward = np.where(err > 0, np.inf, -np.inf)
    t = np.where((err != 0) & ~odd, np.nextafter(s, toward), s)
    return t.astype(F32)


def ulps32(a, b):
    """distance of two float32 values in units in the last place (ordered bit patterns)"""
    def o(x):
        u = np.asarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return int(abs(o(a) - o(b)))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def area32(dx, dy, dz):
    """dx * dy + dy * dz + dz * dx in float32, left to right, one rounding per operation"""
    dx, dy, dz = (np.asarray(v, F32) for v in (dx, dy, dz))
    return (dx * dy + dy * dz) + dz * dx


def padded_boxes(tri):
    """k_flatten's leaf boxes of world triangles tri (T, 3, 3) float32: min / max of the three vertices, then e = 1e-5f * m + 1e-6f in float32 (build_common.h)"""
    tri = np.asarray(tri, F32)
    lo, hi = tri.min(1), tri.max(1)
    m = np.maximum(np.abs(lo), np.abs(hi))
    e = F32(1e-5) * m + F32(1e-6)
    return (lo - e).astype(F32), (hi + e).astype(F32)


# ------------------------------------------------------------------------------------------------ the 8-wide layout
def _planes(D, rows):
    """per node of rows and slot: float32 planes as the traversal decodes them (one fma), the exact float64 ones, and per plane the bound on their difference"""
    org = D["origin"][rows][:, None, :]
    st = np.ldexp(1.0, D["ex"][rows])[:, None, :]
    out = {}
    for k, q in (("lo", D["qlo"][rows]), ("hi", D["qhi"][rows])):
        b = q * st
        exact = org + b
        bb = exact - org
        assert np.all(((org - (exact - bb)) + (b - bb)) == 0), "a plane p + q * 2^e that float64 does not hold exactly"
        out[k + "32"] = round_sum32(np.broadcast_to(org, b.shape), b)
        out[k] = exact
        out["d" + k] = np.where(out[k + "32"].astype(np.float64) == exact, 0.0, 0.5 * ulp32(exact))
    return out


def occupied(D):
    cnt = D["meta"] >> 5
    inner = ((D["imask"][:, None] >> np.arange(8)[None, :]) & 1) != 0
    return inner, cnt, inner | (cnt > 0)


def wide_cost(wnodes, first, count, root, c_node=1.0, c_tri=0.5):
    """Cost of the 8-wide subtree in nodes [first, first + count) rooted at node root, per unit of the root's area: (c_node * A + sum) / A."""
    D = decode_nodes(wnodes)
    if count == 0:
        return Cost(F32(0), 0.0, 0.0, 0.0, 0.0, 0.0)
    rows = np.arange(first, first + count)
    inner, cnt, occ = (x[rows] for x in occupied(D))
    P = _planes(D, rows)
    w = np.where(inner, float(F32(c_node)), float(F32(c_tri)) * cnt)          # (double) c_node | (double) c_tri * (double) cnt
    # emulation: float32 extents and area, float64 weights and sum
    d32 = np.maximum(P["hi32"] - P["lo32"], F32(0))
    a32 = F32(2) * area32(d32[..., 0], d32[..., 1], d32[..., 2])
    sum32 = math.fsum((a32.astype(np.float64) * w)[occ])
    r = root - first
    ro = occ[r]
    rlo, rhi = P["lo32"][r][ro].min(0), P["hi32"][r][ro].max(0)
    rd = np.maximum(F32(0), rhi - rlo).astype(np.float64)          # (the host subtracts in float32, then widens)
    A = 2.0 * (rd[0] * rd[1] + rd[1] * rd[2] + rd[2] * rd[0])
    emu = F32((float(F32(c_node)) * A + sum32) / A) if A > 0 else F32(0)
    # meaning: exact planes, float64 throughout (the sum by fsum)
    d = np.maximum(P["hi"] - P["lo"], 0.0)
    a = 2.0 * (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])
    sum64 = math.fsum((a * w)[occ])
    xd = np.maximum(P["hi"][r][ro].max(0) - P["lo"][r][ro].min(0), 0.0)
    Ax = 2.0 * (xd[0] * xd[1] + xd[1] * xd[2] + xd[2] * xd[0])
    exact = (float(F32(c_node)) * Ax + sum64) / Ax if Ax > 0 else 0.0
    # bound: every extent off by the two planes' errors and the subtraction's rounding; the area's five operations; the final rounding
    dd = P["dlo"] + P["dhi"]
    dd = dd + U * (d + dd)
    up = d + dd
    a_hi = 2.0 * (up[..., 0] * up[..., 1] + up[..., 1] * up[..., 2] + up[..., 2] * up[..., 0]) * (1 + U) ** 5
    dS = math.fsum(((a_hi - a) * w)[occ]) + 2.0 ** -50 * sum64
    rdd = (P["dlo"][r][ro].max(0) + P["dhi"][r][ro].max(0)); rdd = rdd + U * (xd + rdd)
    xu = xd + rdd
    dA = 2.0 * (xu[0] * xu[1] + xu[1] * xu[2] + xu[2] * xu[0]) * (1 + 2.0 ** -50) - Ax
    if Ax > dA > -1:
        bound = (dS + (sum64 / Ax) * dA) / (Ax - dA) + U * abs(exact) * 1.0001
    else:
        bound = math.inf
    return Cost(emu, exact, bound, sum32, sum64, A)


def blas_ranges(lay):
    """[(blas, first wide node, count)] of a two-level layout, in node order: a BLAS's 8-wide nodes start at its instances' wroot and end where the next one's begin"""
    hdr = np.asarray(lay["header"], np.int64)
    inst = decode_instances(lay["instances"])
    roots = {}
    for i in range(len(inst["blas"])):
        roots.setdefault(int(inst["blas"][i]), (int(inst["wroot"][i]), int(inst["ntri"][i])))
    order = sorted(roots.items(), key=lambda kv: kv[1][0])
    out = []
    for k, (b, (wr, nt)) in enumerate(order):
        end = order[k + 1][1][0] if k + 1 < len(order) else int(hdr[0])
        out.append((b, wr, end - wr if nt else 0))
    return out


def scene_wide_cost(lay, c_node=1.0, c_tri=0.5):
    """MRTSceneStats.wide_cost of a layout: the flat tree at node 0, or the mean over the BLASes in double (0 without the 8-wide layout)"""
    hdr = np.asarray(lay["header"], np.int64)
    if hdr[0] == 0:
        return Cost(F32(0), 0.0, 0.0, 0.0, 0.0, 0.0), []
    if not hdr[2]:
        c = wide_cost(lay["wnodes"], 0, int(hdr[0]), 0, c_node, c_tri)
        return c, [c]
    per = [wide_cost(lay["wnodes"], f, n, f, c_node, c_tri) for _, f, n in blas_ranges(lay)]
    B = len(per)
    emu = F32(math.fsum(float(c.emu) for c in per) / B)
    exact = math.fsum(c.exact for c in per) / B
    bound = math.fsum(c.bound for c in per) / B + U * abs(exact) * 1.0001
    return Cost(emu, exact, bound, 0.0, 0.0, 0.0), per


def mean_sah(sah_built, cost_now, cost_built):
    """fold_blas_stats: the mean in double of the BLASes' build-time SAH figures, each scaled by its own wide_cost / wide_cost_built in float32"""
    terms = [float(F32(s) * (F32(c) / F32(b))) if F32(b) > 0 else float(F32(s)) for s, c, b in zip(sah_built, cost_now, cost_built)]
    return F32(math.fsum(terms) / len(terms))


def histogram(wnodes):
    """the 12 words of k_wide_histogram over all nodes of the array: [c] = nodes with c children (c = 0 .. 8), [9] internal children, [10] leaf children, [11] triangles"""
    D = decode_nodes(wnodes)
    out = np.zeros(12, np.int64)
    if D["n"] == 0:
        return out
    cnt = D["meta"] >> 5
    inner = np.array([bin(int(m)).count("1") for m in D["imask"]], np.int64)
    leaves = (cnt > 0).sum(1)
    out[:9] = np.bincount(inner + leaves, minlength=9)[:9]
    out[9], out[10], out[11] = inner.sum(), leaves.sum(), cnt.sum()
    return out


def wide_levels(D, root):
    """the levels of the 8-wide tree under root: arrays of node indices, the root's first.  Children of a node: child_base + rank of its imask bits."""
    pop = np.array([bin(int(m)).count("1") for m in D["imask"]], np.int64)
    levels, front = [], np.array([root], np.int64)
    while len(front):
        assert len(levels) <= D["n"], "a cycle in the 8-wide tree"
        levels.append(front)
        c = pop[front]
        start = np.repeat(D["child_base"][front], c)
        rank = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        front = start + rank
        assert np.all((front >= 0) & (front < D["n"])), "a child index outside the array"
    return levels


def wide_depth(lay):
    """MRTSceneStats.wide_depth: the levels present under node 0; two-level: TLAS levels + 1 + the deepest BLAS"""
    hdr = np.asarray(lay["header"], np.int64)
    if hdr[0] == 0:
        return 0
    D = decode_nodes(lay["wnodes"])
    top = len(wide_levels(D, 0))
    if not hdr[2]:
        return top
    return top + 1 + max(len(wide_levels(D, f)) for _, f, n in blas_ranges(lay) if n)


def leaf_slots(D, first, count, npackets):
    """the leaf slots of nodes [first, first + count): node, slot, first packet, count"""
    rows = np.arange(first, first + count)
    inner, cnt, _ = (x[rows] for x in occupied(D))
    nd, sl = np.nonzero(~inner & (cnt > 0))
    m = D["meta"][rows][nd, sl]
    pk = D["tri_base"][rows][nd] + (m & 31)
    c = m >> 5
    assert np.all(pk + c <= npackets)
    return rows[nd], sl, pk, c


def leaf_growth(before_wnodes, after_wnodes, gids, new_lo, new_hi, moved, previous=1.0, first=0, count=None):
    """MRTSceneStats.leaf_growth after one refit (k_refit_wide_level, k_refit_fold).  before / after: the 8-wide nodes dumped before and after the refit (the
    refit must have kept every link: checked); gids: the packets' triangle ids (word 3 of wpackets); new_lo / new_hi: the padded boxes of ALL triangles as they
    are now (padded_boxes), by id; moved: per triangle, whether its instance was updated; previous: the figure before this refit.  For every leaf slot with a
    moved triangle: had = its box decoded from the BEFORE planes, now = the union of its triangles' new boxes rounded outwards onto the OLD grid; areas
    x*y + y*z + z*x in float32; two float64 sums, a node whose new sum is 0 contributing nothing; result float32(previous * float32(g_new / g_old))."""
    D = decode_nodes(before_wnodes)
    D1 = decode_nodes(after_wnodes)
    count = D["n"] - first if count is None else count
    for k in ("imask", "child_base", "tri_base", "meta"):          # (of the refitted range: a commit of a two-level scene builds the TLAS slots in front of it again)
        assert np.array_equal(D[k][first:first + count], D1[k][first:first + count]), f"the refit changed {k}"
    gids = np.asarray(gids, np.int64); moved = np.asarray(moved, bool)
    new_lo = np.asarray(new_lo, F32); new_hi = np.asarray(new_hi, F32)
    nd, sl, pk, c = leaf_slots(D, first, count, len(gids))
    BIG = F32(3.0e38)
    lo = np.full((len(nd), 3), BIG, F32); hi = np.full((len(nd), 3), -BIG, F32); mv = np.zeros(len(nd), bool)
    for r in range(int(c.max()) if len(c) else 0):
        on = c > r
        g = gids[pk[on] + r]
        lo[on] = np.minimum(lo[on], new_lo[g]); hi[on] = np.maximum(hi[on], new_hi[g]); mv[on] |= moved[g]
    nd, sl, lo, hi = nd[mv], sl[mv], lo[mv], hi[mv]
    org32 = D["origin"][nd].astype(F32); org = D["origin"][nd]
    st = np.ldexp(1.0, D["ex"][nd]); st32 = st.astype(F32)
    ql, qh = D["qlo"][nd, sl].astype(np.float64), D["qhi"][nd, sl].astype(np.float64)
    had_lo, had_hi = round_sum32(org, ql * st), round_sum32(org, qh * st)
    kl = np.floor((lo - org32) / st32); kh = np.ceil((hi - org32) / st32)          # float32 subtraction and division (by a power of two), floorf / ceilf
    now_lo, now_hi = round_sum32(org, kl.astype(np.float64) * st), round_sum32(org, kh.astype(np.float64) * st)
    o = np.maximum(had_hi - had_lo, F32(0)); n = np.maximum(now_hi - now_lo, F32(0))
    a_old = area32(o[:, 0], o[:, 1], o[:, 2]).astype(np.float64); a_new = area32(n[:, 0], n[:, 1], n[:, 2]).astype(np.float64)
    per_old = np.zeros(D["n"]); per_new = np.zeros(D["n"])
    np.add.at(per_old, nd, a_old); np.add.at(per_new, nd, a_new)          # (per node in slot order: nd, sl come sorted from np.nonzero)
    live = per_new > 0
    g0, g1 = math.fsum(per_old[live]), math.fsum(per_new[live])
    ratio32 = F32(g1 / g0) if g0 > 0 else F32(1)
    emu = F32(previous) * ratio32
    # meaning: the same boxes in exact float64 — the old planes as they decode, the new box on the old grid with floor / ceil of the exact quotient
    xl, xh = org + ql * st, org + qh * st
    fl = (lo.astype(np.float64) - org) / st; fh = (hi.astype(np.float64) - org) / st
    yl, yh = org + np.floor(fl) * st, org + np.ceil(fh) * st
    xo = np.maximum(xh - xl, 0.0); yo = np.maximum(yh - yl, 0.0)
    e_old = xo[:, 0] * xo[:, 1] + xo[:, 1] * xo[:, 2] + xo[:, 2] * xo[:, 0]
    e_new = yo[:, 0] * yo[:, 1] + yo[:, 1] * yo[:, 2] + yo[:, 2] * yo[:, 0]
    keep = live[nd]
    G0, G1 = math.fsum(e_old[keep]), math.fsum(e_new[keep])
    ratio_exact = G1 / G0 if G0 > 0 else 1.0
    # bound: half an ulp per plane (the fma's rounding); a whole grid step where the float32 quotient may fall on the other side of an integer; the
    # subtraction's rounding; the area's five operations
    def near(f):          # (the float32 subtraction's rounding is relative to its result, the division by a power of two exact: the quotient is off by at most U |f|)
        return (f != np.rint(f)) & (np.abs(f - np.rint(f)) <= 2 * U * np.maximum(1.0, np.abs(f)))          # (an exact integer below 2^24: the subtraction is exact too)
    d_old = 0.5 * (ulp32(xl) + ulp32(xh)); d_old = d_old + U * (xo + d_old)
    d_new = 0.5 * (ulp32(yl) + ulp32(yh)) + st * (near(fl) + 0.0) + st * (near(fh) + 0.0); d_new = d_new + U * (yo + d_new)
    def spread(x, dx, e):
        up = x + dx
        return math.fsum(((up[:, 0] * up[:, 1] + up[:, 1] * up[:, 2] + up[:, 2] * up[:, 0]) * (1 + U) ** 5 - e)[keep])
    rel = (spread(xo, d_old, e_old) / G0 + spread(yo, d_new, e_new) / G1 + 4 * U) if G0 > 0 and G1 > 0 else 0.0
    return Growth(emu, ratio32, ratio_exact, rel, g0, g1, int(len(nd)))


def unmoved_leaf_excess(before_wnodes, after_wnodes, gids, new_lo, new_hi, moved, first=0, count=None):
    """A leaf slot none of whose triangles moved keeps its box (k_refit_wide_level): what it had — decoded from the BEFORE planes in float32 — cut to its triangles'
    own boxes, then rounded outwards onto the node's NEW grid: the AFTER planes must contain that box and lie less than two new grid steps outside it (one for the
    rounding, one for the quantiser's correction when the rounded plane fell inside).  A pre-split reference thus stays clipped: it never grows to its triangle's box.
    Returns (slots checked, failures as strings, slots whose triangles' box reaches more than a step beyond what the slot had: the clipped references)."""
    D, D1 = decode_nodes(before_wnodes), decode_nodes(after_wnodes)
    count = D["n"] - first if count is None else count
    gids = np.asarray(gids, np.int64); moved = np.asarray(moved, bool)
    new_lo = np.asarray(new_lo, F32); new_hi = np.asarray(new_hi, F32)
    nd, sl, pk, c = leaf_slots(D, first, count, len(gids))
    mv = np.zeros(len(nd), bool)
    lo = np.full((len(nd), 3), F32(3.0e38), F32); hi = np.full((len(nd), 3), F32(-3.0e38), F32)
    for r in range(int(c.max()) if len(c) else 0):
        on = c > r
        g = gids[pk[on] + r]
        lo[on] = np.minimum(lo[on], new_lo[g]); hi[on] = np.maximum(hi[on], new_hi[g]); mv[on] |= moved[g]
    nd, sl, lo, hi = nd[~mv], sl[~mv], lo[~mv].astype(np.float64), hi[~mv].astype(np.float64)
    st0, st1 = np.ldexp(1.0, D["ex"][nd]), np.ldexp(1.0, D1["ex"][nd])
    had_lo = round_sum32(D["origin"][nd], D["qlo"][nd, sl] * st0).astype(np.float64); had_hi = round_sum32(D["origin"][nd], D["qhi"][nd, sl] * st0).astype(np.float64)
    keep_lo, keep_hi = np.maximum(lo, had_lo), np.minimum(hi, had_hi)
    clipped = int(((lo < had_lo - st0) | (hi > had_hi + st0)).any(1).sum())
    bad = []
    # (the AFTER planes as the traversal decodes them, one fma in float32: that is what the quantiser checked against the box)
    got_lo = round_sum32(D1["origin"][nd], D1["qlo"][nd, sl] * st1).astype(np.float64); got_hi = round_sum32(D1["origin"][nd], D1["qhi"][nd, sl] * st1).astype(np.float64)
    for name, want, got, sign in (("lo", keep_lo, got_lo, 1.0), ("hi", keep_hi, got_hi, -1.0)):
        gap = sign * (want - got)          # >= 0: the new plane is outside the box to keep
        for k, ax in list(zip(*np.nonzero((gap < 0) | (gap >= 2 * st1))))[:10]:
            bad.append(f"node {nd[k]} slot {sl[k]} axis {'xyz'[ax]} {name}: keeps {want[k, ax]!r}, plane at {got[k, ax]!r} (new grid step {st1[k, ax]!r})")
    return int(len(nd)), bad, clipped


# ------------------------------------------------------------------------------------------------ the rope layout
def binary_figures(rope_nodes, ct=1.0, ci=1.0, max_leaf=4):
    """One rope tree (root = row 0, indices relative to it: a flattened scene's part, or one BLAS's rows): node and leaf counts, depth in edges from the root
    (k_assign), the largest leaf, the SAH cost by k_refit's recurrence in float32 — leaf: ci * area * nt; inner: ct * area + left + right, the left child first;
    divided by the root's box_area — and in float64, and the violations of the collapse rule: an emitted inner node with nt <= max_leaf whose leaf cost
    ci * area * nt does not exceed its emitted subtree's cost (k_refit would have made it a leaf), and a leaf of more than max_leaf references."""
    wn = np.ascontiguousarray(rope_nodes, np.uint32).reshape(-1, 16)
    lo, hi = wn[:, 0:3].view(F32), wn[:, 4:7].view(F32)
    a, b = wn[:, 3].astype(np.int64), wn[:, 7].astype(np.int64)
    leaf = (a & NODE_LEAF) != 0
    N = len(wn)
    levels, front, seen = [], np.array([0], np.int64), 0
    while len(front):
        seen += len(front)
        assert seen <= N, "a cycle or a shared child in the rope tree"
        levels.append(front)
        inner = front[~leaf[front]]
        front = np.concatenate([a[inner], b[inner] & NODE_INDEX_MASK])
        assert np.all((front >= 0) & (front < N)), "a child index outside the tree"
    d = hi - lo          # box_area: no clamp
    ar32 = F32(2) * area32(d[:, 0], d[:, 1], d[:, 2])
    d64 = hi.astype(np.float64) - lo.astype(np.float64)
    ar64 = 2.0 * (d64[:, 0] * d64[:, 1] + d64[:, 1] * d64[:, 2] + d64[:, 2] * d64[:, 0])
    ct32, ci32 = F32(ct), F32(ci)
    c32 = np.zeros(N, F32); c64 = np.zeros(N); nt = np.zeros(N, np.int64)
    violations = []
    for lv in reversed(levels):
        L = lv[leaf[lv]]
        nt[L] = b[L]
        c32[L] = (ci32 * ar32[L]) * nt[L].astype(F32)
        c64[L] = float(ci32) * ar64[L] * nt[L]
        I = lv[~leaf[lv]]
        l, r = a[I], b[I] & NODE_INDEX_MASK
        nt[I] = nt[l] + nt[r]
        c32[I] = ((ct32 * ar32[I]) + c32[l]) + c32[r]
        c64[I] = float(ct32) * ar64[I] + c64[l] + c64[r]
        as_leaf = (ci32 * ar32[I]) * nt[I].astype(F32)
        for k in np.nonzero((nt[I] <= max_leaf) & (as_leaf <= c32[I]))[0][:10]:
            violations.append(f"inner node {I[k]}: {nt[I[k]]} references, leaf cost {as_leaf[k]!r} <= subtree cost {c32[I[k]]!r}: k_refit collapses it")
        for k in np.nonzero(nt[L] > max_leaf)[0][:10]:
            violations.append(f"leaf node {L[k]}: {nt[L[k]]} references, more than max_leaf {max_leaf}")
    reached = np.concatenate(levels)
    sah32 = c32[0] / ar32[0] if ar32[0] > 0 else F32(0)
    sah64 = c64[0] / ar64[0] if ar64[0] > 0 else 0.0
    return Binary(int(len(reached)), int(leaf[reached].sum()), len(levels) - 1, int(b[reached][leaf[reached]].max()), F32(sah32), float(sah64), violations, c32[0], ar32[0])


def rope_trees(lay):
    """the rope trees of a layout as row slices: one for a flattened scene, one per BLAS (rope_audit.trees_of)"""
    from rope_audit import trees_of
    return [(name, np.asarray(lay["rope_nodes"])[root:end]) for name, root, end, pb, nt in trees_of(lay)]


# ------------------------------------------------------------------------------------------------ bytes
def scene_bytes(header, stats, rope_nodes, rope_packets):
    """MRTSceneStats.scene_bytes from the counts of the layout.  Flattened (bvh_build.hip finish_tree, emit_wide, emit_rope): 16 B per triangle (shading record) and
    per vertex (normal), 20 B per instance and submesh slot, 64 B per instance; 80 B per 8-wide node and 48 B per packet when the 8-wide layout is kept; 64 B per
    rope node and 48 B per packet when the rope layout is.  Two-level (two_level.hip build_two_level): 64 B per BLAS rope node and 48 B per packet, the 8-wide
    nodes (TLAS slots included) at 80 B and the packets again when every BLAS has the layout, 16 B per triangle and vertex, 80 + 64 + 20 x submesh slots per instance."""
    hdr = np.asarray(header, np.int64)
    T, V, I, S = int(stats.triangles), int(stats.vertices), int(stats.instances), int(stats.max_submeshes)
    NW, npk = int(hdr[0]), int(hdr[4])
    if hdr[2]:
        return rope_nodes * 64 + rope_packets * 48 + (NW * 80 + rope_packets * 48 if NW else 0) + rope_packets * 16 + V * 16 + I * (80 + 64 + S * 20)
    if T == 0:
        return 0
    return T * 16 + V * 16 + I * S * 20 + I * 64 + (NW * 80 + npk * 48 if NW else 0) + rope_nodes * 64 + rope_packets * 48
