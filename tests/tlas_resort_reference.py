"""What mrt_scene_rebuild_tlas_device computes on the device (csrc/tlas_rebuild.hip), restated in numpy float32: the full recursive median order of the
instance ids, level by level.  A range [first, first + count) is split at count // 2, so where the ranges lie depends on the count alone; within a range of two or more
the axis is the widest extent of 0.5f * (lo + hi) over its members (axis 0, then 1 if strictly wider, then 2 if strictly wider) and every member moves to first + its rank
under (lo + hi on that axis, id)."""
import numpy as np

LEAF = 0x80000000


def ranges_of_level(n, level):
    """the ranges of one level, root = level 0: (first, count) pairs, count // 2 down from (0, n); a range of one stays"""
    out = [(0, n)]
    for _ in range(level):
        nxt = []
        for first, count in out:
            if count < 2: nxt.append((first, count)); continue
            half = count // 2
            nxt += [(first, half), (first + half, count - half)]
        out = nxt
    return out


def median_order(lo, hi, start):
    """lo, hi: (N, 3) float32 boxes by instance id; start: any permutation of the live ids.  Returns ids, the full median order."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    ids = np.array(start, np.uint32)
    n = len(ids)
    s = lo + hi          # float32: the builders' sort key
    assert s.dtype == np.float32
    level = 0
    while True:
        ranges = [r for r in ranges_of_level(n, level) if r[1] >= 2]
        if not ranges: return ids
        for first, count in ranges:
            m = ids[first:first + count]
            c = np.float32(0.5) * s[m]
            ext = c.max(axis=0) - c.min(axis=0)
            ax = 0
            if ext[1] > ext[ax]: ax = 1
            if ext[2] > ext[ax]: ax = 2
            ids[first:first + count] = m[np.lexsort((m, s[m, ax]))]          # rank under (key, id): keys first, ties by id
        level += 1


def host_build(lib, lo, hi):
    """mrt_debug_tlas_host_build on (n, 3) boxes -> dict(rope_order, rope_links (nodes, 4) {a, b, escape, depth}, wide_order, wide_pos, rope_levels, wide_levels)"""
    from metal_raytracing_amd._ffi import ptr
    n = len(lo)
    lo4 = np.zeros((n, 4), np.float32); hi4 = np.zeros((n, 4), np.float32)
    lo4[:, :3] = lo; hi4[:, :3] = hi
    rope_order, wide_order, wide_pos = (np.zeros(n, np.uint32) for _ in range(3))
    links = np.zeros((2 * n - 1, 4), np.uint32); counts = np.zeros(68, np.uint32)
    rc = lib.mrt_debug_tlas_host_build(ptr(lo4), ptr(hi4), n, ptr(rope_order), ptr(links), ptr(wide_order), ptr(wide_pos), ptr(counts))
    assert rc == 0, lib.mrt_last_error().decode()
    return dict(rope_order=rope_order, rope_links=links[:int(counts[0])], wide_order=wide_order, wide_pos=wide_pos,
                rope_levels=counts[4:4 + int(counts[1])].copy(), wide_levels=counts[36:36 + int(counts[3])].copy(), wide_nodes=int(counts[2]))


def rope_leaves(links):
    """(first, count) of every leaf of the rope TLAS, from its link words"""
    return [(int(a & 0x7FFFFFFF), int(b)) for a, b, _, _ in links if a & LEAF]
