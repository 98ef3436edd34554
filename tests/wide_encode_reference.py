"""What csrc/wide_encode.h and csrc/instance_math.h compute, restated for tests that need no GPU.

The encoder of the 8-wide node in numpy float32 (every operation rounded to float32, none fused, as the library is built): per axis the power-of-two grid
(sdiv = extent / 255, exponent rounded up, kept to 1 .. 254, step and 1 / step built from bits), per child floor / ceil onto the grid, the clamp to 0 .. 255 and one more
step where the float32 decode origin + q * step fails to enclose the child, (255, 0) for an empty slot; words 0, 2, 3 and 4 of the 80-byte node.  The node box is the union
of the occupied children, as a refit takes it.

The world->object rows of an instance in Python floats (IEEE double, one operation at a time, in the order of instance_math.h), rounded to float32 once; and the world_box
condition of bvh_audit.audit for one instance."""
import math

import numpy as np

from bvh_audit import GAMMA4

F = np.float32


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _f32(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def encode(clo, chi, occ, imask):
    """clo, chi: (N, 8, 3) float32 child boxes; occ: (N, 8) bool, at least one per node; imask: (N,) -> (N, 20) uint32, word 1 .. 7 of a node zero but for the planes"""
    clo, chi = np.asarray(clo, np.float32), np.asarray(chi, np.float32)
    occ = np.asarray(occ, bool)
    n = clo.shape[0]
    big = F(3.0e38)
    nl = np.where(occ[:, :, None], clo, big).min(axis=1)
    nh = np.where(occ[:, :, None], chi, -big).max(axis=1)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):          # (what an empty slot's stale box gives is masked below)
        sdiv = (nh - nl) / F(255.0)
        bits = _u32(sdiv)
        e = (bits >> 23) + ((bits & 0x7FFFFF) != 0)
        e = np.clip(e, 1, 254).astype(np.uint32)
        step = _f32(e << 23)[:, None, :]
        inv_step = _f32((np.uint32(254) - e) << 23)[:, None, :]
        o = nl[:, None, :]
        fl = np.floor((clo - o) * inv_step)
        fh = np.ceil((chi - o) * inv_step)
        fl = np.minimum(np.maximum(fl, F(0)), F(255)); fh = np.minimum(np.maximum(fh, F(0)), F(255))
        fl = np.where((o + fl * step > clo) & (fl > 0), fl - F(1), fl)
        fh = np.where((o + fh * step < chi) & (fh < 255), fh + F(1), fh)
    assert fl.dtype == np.float32 and fh.dtype == np.float32 and sdiv.dtype == np.float32
    ql = np.where(occ[:, :, None], fl, F(255)).astype(np.uint32)          # (N, 8, 3)
    qh = np.where(occ[:, :, None], fh, F(0)).astype(np.uint32)
    out = np.zeros((n, 20), np.uint32)
    out[:, 0:3] = _u32(nl)
    eu = (e - np.uint32(127)) & 0xFF
    out[:, 3] = eu[:, 0] | (eu[:, 1] << 8) | (eu[:, 2] << 16) | (np.asarray(imask, np.uint32) << 24)
    sh = (8 * (np.arange(8) & 3)).astype(np.uint32)
    for a in range(3):
        for half in range(2):
            s = slice(4 * half, 4 * half + 4)
            out[:, 8 + 2 * a + half] = np.bitwise_or.reduce(ql[:, s, a] << sh[s], axis=1)
            out[:, 14 + 2 * a + half] = np.bitwise_or.reduce(qh[:, s, a] << sh[s], axis=1)
    return out


def rows_reference(xf):
    """xf: 16 float32, column-major -> (3, 4) float32 rows of [A^-1 | -A^-1 t], or None for a matrix that is not taken"""
    a00, a10, a20, a01, a11, a21, a02, a12, a22 = (float(xf[k]) for k in (0, 1, 2, 4, 5, 6, 8, 9, 10))
    tx, ty, tz = float(xf[12]), float(xf[13]), float(xf[14])
    c = [[a11 * a22 - a12 * a21, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11],
         [a12 * a20 - a10 * a22, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12],
         [a10 * a21 - a11 * a20, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10]]
    det = a00 * c[0][0] + a01 * c[1][0] + a02 * c[2][0]
    if not (abs(det) > 0.0 and math.isfinite(det)):
        return None
    rows = np.zeros((3, 4), np.float32)
    for r in range(3):
        i0, i1, i2 = c[r][0] / det, c[r][1] / det, c[r][2] / det
        rows[r] = [F(i0), F(i1), F(i2), F(-(i0 * tx + i1 * ty + i2 * tz))]
    return rows


def world_box_margin(rows, obj_lo, obj_hi, wlo, whi):
    """bvh_audit.audit's world_box check for one instance: the smallest distance, over the six planes, by which the world box contains the exact image, under the float64
    inverse of the stored float32 rows, of the object box grown by delta_k = gamma_4 (sum_j |R_kj| max|X_j| + |w_k|), X over the world box.  Negative: it does not."""
    R = np.asarray(rows, np.float32).astype(np.float64)
    A, w = R[:, :3], R[:, 3]
    M = np.linalg.inv(A)
    wlo, whi = np.asarray(wlo, np.float32).astype(np.float64), np.asarray(whi, np.float32).astype(np.float64)
    X = np.maximum(np.abs(wlo), np.abs(whi))
    delta = GAMMA4 * (np.abs(A) @ X + np.abs(w))
    olo, ohi = np.asarray(obj_lo, np.float32).astype(np.float64) - delta, np.asarray(obj_hi, np.float32).astype(np.float64) + delta
    corners = np.array([[(ohi if (c >> k) & 1 else olo)[k] for k in range(3)] for c in range(8)])
    img = (corners - w) @ M.T          # x = A^-1 (p - w)
    return float(np.minimum(img.min(0) - wlo, whi - img.max(0)).min())
