"""The box audit of tests/bvh_audit.py on a hand-encoded two-level 8-wide layout (no GPU): it passes on a correct tree and names each planted
defect — a plane moved one step inwards, a dropped packet, a child index past the end, a depth above the claimed one, a shrunk instance box."""
import numpy as np
import pytest

import bvh_audit as A


def _f32_words(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _encode_node(lo, hi, slots, child_base, tri_base):
    """one 8-wide node (20 uint32) over the box [lo, hi]: slots = 8 entries of None (empty) or (kind, box_lo, box_hi, count, offset), kind
    'node' or 'leaf'; planes rounded outwards in float64 on the node's power-of-two grid, as k_wide_level does."""
    lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
    ex = np.array([int(np.ceil(np.log2(max(float(hi[a]) - float(lo[a]), 1e-30) / 255.0))) for a in range(3)])
    step = np.ldexp(1.0, ex)
    qlo = np.full((8, 3), 255, np.int64); qhi = np.zeros((8, 3), np.int64)
    meta = np.zeros(8, np.uint32); imask = 0
    for sl, s in enumerate(slots):
        if s is None:
            continue
        kind, blo, bhi, cnt, off = s
        qlo[sl] = np.clip(np.floor((np.asarray(blo, np.float64) - lo.astype(np.float64)) / step), 0, 255)
        qhi[sl] = np.clip(np.ceil((np.asarray(bhi, np.float64) - lo.astype(np.float64)) / step), 0, 255)
        if kind == "node":
            imask |= 1 << sl
        else:
            meta[sl] = (cnt << 5) | off
    w = np.zeros(20, np.uint32)
    w[0:3] = _f32_words(lo)
    w[3] = (int(ex[0]) & 0xFF) | ((int(ex[1]) & 0xFF) << 8) | ((int(ex[2]) & 0xFF) << 16) | (imask << 24)
    w[4], w[5] = child_base, tri_base
    w[6] = meta[0] | (meta[1] << 8) | (meta[2] << 16) | (meta[3] << 24)
    w[7] = meta[4] | (meta[5] << 8) | (meta[6] << 16) | (meta[7] << 24)
    for k, arr in enumerate((qlo[:, 0], qlo[:, 1], qlo[:, 2], qhi[:, 0], qhi[:, 1], qhi[:, 2])):
        b = arr.astype(np.uint8)
        w[8 + 2 * k] = int(b[0]) | int(b[1]) << 8 | int(b[2]) << 16 | int(b[3]) << 24
        w[9 + 2 * k] = int(b[4]) | int(b[5]) << 8 | int(b[6]) << 16 | int(b[7]) << 24
    return w


def _padded(v):
    lo, hi = v.min(0), v.max(0)
    e = A.pad_of(np.maximum(np.abs(lo), np.abs(hi)))
    return lo - e, hi + e


def _layout():
    """Two instances of one 4-triangle BLAS.  Nodes: 0 = TLAS root (two instance leaves), 1 = unused TLAS slot (tlas_wcap = 2), 2 = BLAS root
    (an internal child + a leaf of two packets), 3 = its child (two leaves of one packet)."""
    tris = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
                     [[1.0, 1.003, 0.0], [1.2, 1.003, 0.3], [1.0, 1.4, 0.1]],
                     [[-1.0, 0.5, 1.0], [-0.5, 0.5, 1.0], [-1.0, 0.9, 1.25]],
                     [[-0.25, -0.75, -0.5], [0.0, -0.5, -0.5], [-0.25, -0.5, 0.0]]], np.float32)
    # packets: node 2's leaf (triangles 2, 3) first, then node 3's (0, 1)
    order = [2, 3, 0, 1]
    wp = np.zeros((4, 12), np.uint32)
    for p, t in enumerate(order):
        v = tris[t]
        wp[p, 0:3] = _f32_words(v[0]); wp[p, 3] = t
        wp[p, 4:7] = _f32_words(v[1] - v[0]); wp[p, 8:11] = _f32_words(v[2] - v[0])
    V, _ = A.decode_packets(wp)
    boxes = [_padded(V[p]) for p in range(4)]
    u = lambda bs: (np.min([b[0] for b in bs], 0), np.max([b[1] for b in bs], 0))
    n3 = u(boxes[2:4]); leaf2 = u(boxes[0:2]); n2 = u([n3, leaf2])
    node3 = _encode_node(*n3, [("leaf", *boxes[2], 1, 0), ("leaf", *boxes[3], 1, 1)] + [None] * 6, 0, 2)
    node2 = _encode_node(*n2, [("node", *n3, 0, 0), None, None, ("leaf", *leaf2, 2, 0)] + [None] * 4, 3, 0)
    # instances: a translation, and a rotation with a scale of 2
    c, s = np.cos(0.7), np.sin(0.7)
    xfs = [np.array([[1, 0, 0, 5], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64),
           np.array([[2 * c, -2 * s, 0, -3], [2 * s, 2 * c, 0, 1], [0, 0, 2, 0.5]], np.float64)]
    inst = np.zeros((2, 20), np.uint32); ibox = np.zeros((2, 16), np.float32)
    for i, xf in enumerate(xfs):
        Ai = np.linalg.inv(xf[:, :3])
        rows = np.c_[Ai, -Ai @ xf[:, 3]].astype(np.float32)
        inst[i, 0:12] = rows.reshape(-1).view(np.uint32)
        inst[i, 13] = 0; inst[i, 17] = 4; inst[i, 18] = 0; inst[i, 19] = 2       # packet_base, ntri, blas, wroot
        olo, ohi = n2[0].astype(np.float32), n2[1].astype(np.float32)
        grown_lo, grown_hi = olo - 1e-4, ohi + 1e-4
        cg = np.array([[(grown_hi if (k >> a) & 1 else grown_lo)[a] for a in range(3)] for k in range(8)])
        img = cg @ xf[:, :3].T + xf[:, 3]
        m = np.abs(img).max(0)
        wlo = (img.min(0) - (4e-5 * m + 4e-6)).astype(np.float32); whi = (img.max(0) + (4e-5 * m + 4e-6)).astype(np.float32)
        ibox[i, 0:3], ibox[i, 4:7], ibox[i, 8:11], ibox[i, 12:15] = olo, ohi, wlo, whi
    wb = [(ibox[i, 8:11].astype(np.float64), ibox[i, 12:15].astype(np.float64)) for i in range(2)]
    node0 = _encode_node(*u(wb), [("leaf", *wb[0], 1, 0), ("leaf", *wb[1], 1, 1)] + [None] * 6, 0, 0)
    wn = np.stack([node0, np.zeros(20, np.uint32), node2, node3])
    hdr = np.array([4, 2, 2, 4, 4, 2, 2, 3], np.uint32)
    return dict(header=hdr, wnodes=wn, wpackets=wp, instances=inst, inst_box=ibox, wtlas_index=np.array([0, 1], np.uint32)), xfs


def _set_byte(wn, node, word, byte, value):
    w = int(wn[node, word])
    wn[node, word] = (w & ~(0xFF << (8 * byte))) | ((value & 0xFF) << (8 * byte))


def _get_byte(wn, node, word, byte):
    return (int(wn[node, word]) >> (8 * byte)) & 0xFF


def test_audit_passes_on_a_correct_tree():
    lay, _ = _layout()
    rep = A.audit(lay)
    rep.check()
    assert rep.depth == 4
    assert set(rep.margins) >= {"contain", "pad", "tlas_leaf", "obj_box", "world_box"}
    assert rep.margins["pad"]["min_pad_frac"] >= 0.5
    assert rep.counts["nodes_reached"] == 3


def test_decode_is_exact_and_empty_slots_are_empty():
    lay, _ = _layout()
    D = A.decode_nodes(lay["wnodes"])
    step = np.ldexp(1.0, D["ex"][2])
    assert np.array_equal(D["lo"][2, 0], D["origin"][2] + D["qlo"][2, 0] * step)
    assert (D["qlo"][2, 1] == 255).all() and (D["qhi"][2, 1] == 0).all() and D["meta"][2, 1] == 0 and not (D["imask"][2] >> 1) & 1


# (description, mutation, text the failure must contain)
def _qhi_down(lay):        # node 3 slot 0, qhi_x (word 14, byte 0) one step lower
    _set_byte(lay["wnodes"], 3, 14, 0, _get_byte(lay["wnodes"], 3, 14, 0) - 1)


def _qlo_up(lay):          # node 3 slot 1, qlo_y (word 10, byte 1) one step higher
    _set_byte(lay["wnodes"], 3, 10, 1, _get_byte(lay["wnodes"], 3, 10, 1) + 1)


def _drop_packet(lay):     # node 2 slot 3 names one packet instead of two
    _set_byte(lay["wnodes"], 2, 6, 3, (1 << 5) | 0)


def _child_past_end(lay):
    lay["wnodes"][2, 4] = 99


def _depth_understated(lay):
    lay["header"][3] = 3


def _instance_box_shrunk(lay, xfs):
    """instance 1's world box cut back to the exact image of its object box: the fma-chain bound delta no longer fits"""
    ib = lay["inst_box"]
    R = lay["instances"][1, 0:12].view(np.float32).astype(np.float64).reshape(3, 4)
    M = np.linalg.inv(R[:, :3])
    olo, ohi = ib[1, 0:3].astype(np.float64), ib[1, 4:7].astype(np.float64)
    corners = np.array([[(ohi if (k >> a) & 1 else olo)[a] for a in range(3)] for k in range(8)])
    img = (corners - R[:, 3]) @ M.T
    ib[1, 12] = np.float32(img[:, 0].max())


MUTATIONS = [
    ("qhi lowered", _qhi_down, "node 3 slot 0 axis x hi"),
    ("qlo raised", _qlo_up, "node 3 slot 1 axis y lo"),
    ("packet dropped", _drop_packet, "packet 1 (id 3): referenced by no leaf slot"),
    ("child past the end", _child_past_end, "node 2 slot 0: child index 99 outside wnodes"),
    ("depth understated", _depth_understated, "real depth 4 exceeds the claimed wide_depth 3"),
    ("instance box shrunk", None, "world_box: instance 1"),
]


@pytest.mark.parametrize("name,mutate,expect", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_audit_reports_each_mutation(name, mutate, expect):
    lay, xfs = _layout()
    if mutate is None:
        _instance_box_shrunk(lay, xfs)
    else:
        mutate(lay)
    rep = A.audit(lay)
    assert rep.failures, f"{name}: not reported"
    assert any(expect in f for f in rep.failures), f"{name}: expected '{expect}' in {rep.failures}"
    with pytest.raises(AssertionError):
        rep.check()


def test_split_references_must_cover_the_triangle():
    """A flattened layout with one long triangle in two references: covered as built; a gap between the two slabs is reported."""
    v = np.array([[0.0, 0.0, 0.0], [8.0, 0.5, 0.0], [0.0, 1.0, 0.25]], np.float32)
    wp = np.zeros((2, 12), np.uint32)
    for p in range(2):
        wp[p, 0:3] = _f32_words(v[0]); wp[p, 3] = 0; wp[p, 4:7] = _f32_words(v[1] - v[0]); wp[p, 8:11] = _f32_words(v[2] - v[0])
    V, _ = A.decode_packets(wp)
    lo, hi = _padded(V[0])

    def piece(a, b):
        ext = A._clip_extent(V[0], 0, a, b)
        e = A.pad_of(np.maximum(np.abs(ext[0]), np.abs(ext[1])))
        return np.maximum(ext[0] - e, lo), np.minimum(ext[1] + e, hi)

    def lay_of(cut_a, cut_b):
        p0, p1 = piece(lo[0], cut_a), piece(cut_b, hi[0])
        node = _encode_node(lo, hi, [("leaf", *p0, 1, 0), ("leaf", *p1, 1, 1)] + [None] * 6, 0, 0)
        return dict(header=np.array([1, 0, 0, 1, 2, 0, 0, 3], np.uint32), wnodes=node[None, :], wpackets=wp)

    rep = A.audit(lay_of(4.0, 4.0), presplit=True, num_tris=1)
    rep.check()
    assert rep.counts["split_triangles"] == 1 and "split" in rep.margins
    rep = A.audit(lay_of(3.0, 5.0), presplit=True, num_tris=1)
    assert any(f.startswith("split: triangle 0") for f in rep.failures), rep.failures
    rep = A.audit(lay_of(4.0, 4.0), presplit=False, num_tris=1)
    assert any("referenced 2 times" in f for f in rep.failures), rep.failures
