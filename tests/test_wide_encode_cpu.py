"""The shared writers of the two-level and 8-wide formats without a GPU: the 8-wide node encoder (csrc/wide_encode.h: the build, both refits and the host TLAS build call
it) through mrt_debug_wide_encode, and the instance arithmetic (csrc/instance_math.h: the host's update_tlas and the device's instance moves call it) through
mrt_debug_instance_box.  Bit equality with the restatements of wide_encode_reference.py, and the geometric conditions decoded exactly in float64 by bvh_audit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bvh_audit as A
import wide_encode_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mrt_debug_wide_encode", "mrt_debug_instance_box")
FAMILIES = ("unit", "far", "thin", "huge", "tiny", "flat", "single", "identical")
NODES = 500


def _family(kind):
    """(clo, chi (NODES, 8, 3) float32, occ (NODES, 8) bool, imask (NODES,)): slot 0 always has a child"""
    rng = np.random.default_rng(1000 + FAMILIES.index(kind))
    c = rng.uniform(-4.0, 4.0, (NODES, 8, 3))
    h = rng.uniform(0.01, 1.5, (NODES, 8, 3))
    occ = rng.random((NODES, 8)) < 0.6
    if kind == "far": c = c + 1e4; h = h * 1e-3
    elif kind == "thin": h[:, :, 0] *= 1e-6
    elif kind == "huge": c = c * 1e28; h = h * 1e28
    elif kind == "tiny": c = c * 1e-30; h = h * 1e-30
    elif kind == "flat": h[:, :, 1] = 0.0; c[:, :, 1] = c[:, :1, 1]
    elif kind == "single": occ[:] = False
    elif kind == "identical": c[:] = c[:, :1]; h[:] = h[:, :1]; occ[:] = True
    occ[:, 0] = True
    c, h = c.astype(np.float32), h.astype(np.float32)
    with np.errstate(over="ignore"):
        clo, chi = (c - h).astype(np.float32), (c + h).astype(np.float32)
    assert np.isfinite(clo).all() and np.isfinite(chi).all() and (clo <= chi).all()
    imask = (rng.integers(0, 256, NODES) & (occ * (1 << np.arange(8))).sum(axis=1)).astype(np.uint32)          # any subset of the occupied slots
    return clo, chi, occ, imask


def _encode(lib, clo, chi, occ, imask):
    from metal_raytracing_amd._ffi import ptr
    n = clo.shape[0]
    lo4 = np.zeros((n, 8, 4), np.float32); hi4 = np.zeros((n, 8, 4), np.float32)
    lo4[:, :, :3] = clo; hi4[:, :, :3] = chi
    masks = (occ * (1 << np.arange(8))).sum(axis=1)
    out = np.full((n, 20), 0xDEADBEEF, np.uint32)
    for i in range(n):
        rc = lib.mrt_debug_wide_encode(ptr(lo4[i]), ptr(hi4[i]), int(masks[i]), int(imask[i]), ptr(out[i]))
        assert rc == 0, lib.mrt_last_error().decode()
    return out


@pytest.mark.parametrize("kind", FAMILIES)
def test_encoder_matches_the_restatement_and_encloses(mrt, kind):
    clo, chi, occ, imask = _family(kind)
    got = _encode(mrt.lib, clo, chi, occ, imask)
    want = R.encode(clo, chi, occ, imask)
    assert (got[:, 4:8] == 0).all(), "word 1 is written as zeros"
    for w in (0, 2, 3, 4):
        assert np.array_equal(got[:, 4 * w:4 * w + 4], want[:, 4 * w:4 * w + 4]), f"word {w} differs from the float32 restatement"
    D = A.decode_nodes(got)
    assert np.array_equal(D["imask"], imask), "imask comes back in bits 24 .. 31"
    o3 = occ[:, :, None]
    assert (D["qlo"][~occ] == A.EMPTY_LO).all() and (D["qhi"][~occ] == A.EMPTY_HI).all(), "empty slots hold (255, 0) on every axis"
    lo64, hi64 = clo.astype(np.float64), chi.astype(np.float64)
    assert (~o3 | ((D["lo"] <= lo64) & (D["hi"] >= hi64))).all(), "every occupied slot encloses its child with zero margin"
    step = np.ldexp(1.0, D["ex"])[:, None, :]
    free_lo = o3 & (D["qlo"] != 0) & (D["qlo"] != 255)
    free_hi = o3 & (D["qhi"] != 0) & (D["qhi"] != 255)
    slack_lo, slack_hi = (lo64 - D["lo"]) / step, (D["hi"] - hi64) / step
    print(kind, "largest slack in steps:", float(np.where(free_lo, slack_lo, 0).max()), float(np.where(free_hi, slack_hi, 0).max()))
    assert (~free_lo | (slack_lo <= 1.0)).all() and (~free_hi | (slack_hi <= 1.0)).all(), "a plane lies at most one grid step beyond the child unless its byte is clamped"
    nl = np.where(o3, lo64, np.inf).min(axis=1); nh = np.where(o3, hi64, -np.inf).max(axis=1)
    assert np.array_equal(D["origin"], nl), "the origin is the union's lower corner"
    per_step = (nh - nl) / 255.0
    grid = np.ldexp(1.0, D["ex"])
    assert (grid >= per_step).all(), "2^e >= extent / 255"
    clamped = (D["ex"] <= -126) | (D["ex"] >= 127)
    assert (clamped | (grid / 2 < per_step)).all(), "the exponent is minimal unless clamped"


def _xf(m3, t=(0.0, 0.0, 0.0)):
    xf = np.zeros(16, np.float32)
    m3 = np.asarray(m3, np.float64)
    for c in range(3): xf[4 * c:4 * c + 3] = m3[:, c]
    xf[12:15] = t; xf[15] = 1.0
    return xf


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


OBJ_LO, OBJ_HI = np.array([-1.0, -0.5, -2.0], np.float32), np.array([1.5, 0.75, 0.25], np.float32)
MATRICES = {
    "identity": _xf(np.eye(3)),
    "rotation_scale_half": _xf(0.5 * _rot((1.0, 2.0, 3.0), 0.7), (0.3, -1.2, 2.5)),
    "non_uniform_scale": _xf(np.diag([1.0, 3.0, 0.2]), (1.0, 2.0, 3.0)),
    "shear": _xf([[1.0, 0.8, 0.0], [0.0, 1.0, -0.4], [0.3, 0.0, 1.0]], (-2.0, 0.5, 0.0)),
    "translation_1e4": _xf(_rot((0.0, 1.0, 0.2), 1.1), (1.0e4, -1.0e4, 1.0e4)),
    "scale_1e-3": _xf(1e-3 * _rot((1.0, 0.0, 1.0), 2.0), (0.1, 0.2, 0.3)),
}
REFUSED = {
    "singular": _xf([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 0.0, 1.0]]),
    "infinite_determinant": _xf(np.diag([np.inf, 1.0, 1.0])),
}


def _instance_box(lib, xf):
    from metal_raytracing_amd._ffi import ptr
    rows = np.full((3, 4), np.nan, np.float32); box = np.full(6, np.nan, np.float32)
    rc = lib.mrt_debug_instance_box(ptr(xf), ptr(OBJ_LO), ptr(OBJ_HI), ptr(rows), ptr(box))
    return rc, rows, box


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_instance_rows_and_world_box(mrt, name):
    xf = MATRICES[name]
    rc, rows, box = _instance_box(mrt.lib, xf)
    assert rc == 0, mrt.lib.mrt_last_error().decode()
    want = R.rows_reference(xf)
    assert want is not None and np.array_equal(rows.view(np.uint32), want.view(np.uint32)), "the rows are the float64 restatement's, rounded once"
    assert np.isfinite(box).all() and (box[:3] < box[3:]).all()
    margin = R.world_box_margin(rows, OBJ_LO, OBJ_HI, box[:3], box[3:])
    print(name, "world_box margin:", margin)
    assert margin >= 0.0, "bvh_audit's world_box condition for this one instance"
    rc2, rows2, box2 = _instance_box(mrt.lib, xf)
    assert rc2 == 0 and rows2.tobytes() == rows.tobytes() and box2.tobytes() == box.tobytes(), "a second call gives identical bytes"


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_instance_box_refuses_what_invert_affine_does_not_take(mrt, name):
    assert R.rows_reference(REFUSED[name]) is None
    rc, rows, box = _instance_box(mrt.lib, REFUSED[name])
    assert rc == 1 and "mrt_debug_instance_box" in mrt.lib.mrt_last_error().decode()          # MRT_ERR_INVALID_ARGUMENT
    assert np.isnan(rows).all() and np.isnan(box).all(), "nothing is written"


def test_entries_check_their_arguments(mrt):
    f = (C.c_float * 32)(); u = (C.c_uint32 * 20)()
    for call in (lambda: mrt.lib.mrt_debug_wide_encode(None, f, 1, 0, u), lambda: mrt.lib.mrt_debug_wide_encode(f, f, 1, 0, None),
                 lambda: mrt.lib.mrt_debug_wide_encode(f, f, 0, 0, u), lambda: mrt.lib.mrt_debug_wide_encode(f, f, 256, 0, u), lambda: mrt.lib.mrt_debug_wide_encode(f, f, 1, 2, u)):
        assert call() == 1 and "mrt_debug_wide_encode" in mrt.lib.mrt_last_error().decode()
    for call in (lambda: mrt.lib.mrt_debug_instance_box(None, f, f, f, f), lambda: mrt.lib.mrt_debug_instance_box(f, f, f, None, f), lambda: mrt.lib.mrt_debug_instance_box(f, f, f, f, None)):
        assert call() == 1 and "mrt_debug_instance_box" in mrt.lib.mrt_last_error().decode()


def test_header_and_ffi_declare_the_entries(mrt):
    from metal_raytracing_amd import _ffi
    P, U32 = C.c_void_p, C.c_uint32
    dbg = open(os.path.join(ROOT, "include", "mrt_debug.h")).read()
    for name in ENTRIES:
        assert re.search(rf"^int {name}\(", dbg, re.M)
    assert _ffi.SIGNATURES["mrt_debug_wide_encode"] == (C.c_int, [P, P, U32, U32, P])
    assert _ffi.SIGNATURES["mrt_debug_instance_box"] == (C.c_int, [P, P, P, P, P])
    assert mrt.lib.mrt_abi_version() == 3
