"""The variance-guided a-trous filter on device buffers and the sample image of its moments (mrt_context_moments_sample_device, mrt_context_denoise_variance_device;
DESIGN.md §10t) as far as they can be checked without a GPU: the yardstick of the GPU tests (tests/variance_reference.py) against answers known exactly, the switch
between the two variance estimates, coverage and NaN, the moments through two reprojection calls against the running average, nine mistakes each failing a named check,
the header, the ctypes mirror and the C++ one, every refusal that needs no device — each reached with a NULL context, which is refused last —, the resources of the
kernels of variance.hip, and the direction of the quality gain against the oracle."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as D
import path_state_reference as PS
import temporal_cases as TC
import temporal_reference as T
import variance_cases as VC
import variance_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
SAMPLE, FILTER = "mrt_context_moments_sample_device", "mrt_context_denoise_variance_device"
f32 = np.float32
SIGMAS = (f32(4.0), f32(0.25), f32(0.25))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


class NotTheCase(Exception):
    """a check's set-up does not hold: the case is not what its docstring says.  Not an AssertionError, so that a mistake which breaks a set-up is not counted as caught."""


def _given(condition, *what):
    if not condition: raise NotTheCase(*what)


def _entries(c, **kw):
    """the working entries of the first level of a case: (I, v, normal | depth)"""
    I, v, _, _ = V.prepass(c["image"], c["moments"], c["normal_depth"], c["albedo"], **kw)
    return I, v, c["normal_depth"]


# ---------------------------------------------------------------- known answers that are exact, each also the named check of a mistake
def check_flat_image(mistake=None):
    """a constant image with v = 1, len = 32, one iteration: all weights are the dyadic h.  Interior: I' = I and v' = (sum b^2)^2 = (70/256)^2 = 4900/65536 to the bit,
    wsum = 1.  Corner (0, 0): the taps dx, dy in {0, 1, 2}, sum b = 11/16, sum b^2 = 53/256: v' = (2809/65536) / (121/256)^2.  Edge x = 0: (53 * 70 / 65536) / (11/16)^2."""
    I, v, nd = _entries(VC.flat(12, 11), mistake=mistake)
    _given((v == 1).all())
    I2, v2 = V.level(I, v, nd, 1, *SIGMAS, mistake=mistake)
    assert np.array_equal(_bits(I2), _bits(I))
    assert _bits(v2[5, 5]) == _bits(f32(4900.0 / 65536.0)) and (v2[2:-2, 2:-2] == v2[5, 5]).all()
    corner = f32(2809.0 / 65536.0) / (f32(121.0 / 256.0) * f32(121.0 / 256.0))
    edge = f32(3710.0 / 65536.0) / (f32(11.0 / 16.0) * f32(11.0 / 16.0))
    assert _bits(v2[0, 0]) == _bits(corner) and _bits(v2[10, 11]) == _bits(corner) and _bits(v2[5, 0]) == _bits(edge) and _bits(v2[0, 6]) == _bits(edge)
    assert _bits(v2[0, 0]) == _bits(VC.scalar_level(I, v, nd, 0, 0, 1)[1]) and _bits(v2[1, 1]) == _bits(VC.scalar_level(I, v, nd, 1, 1, 1)[1])
    out = VC.run(VC.flat(12, 11), iterations=1, mistake=mistake)
    assert np.array_equal(_bits(out[..., 0:3]), _bits(VC.flat(12, 11)["image"][..., 0:3])) and (out[..., 3] == 1).all()


def check_two_halves(mistake=None):
    """two constant halves: with v = 0 den is 1e-6 and rejects the other half — every pixel comes back to the bit at every iteration count; with a large v they blend"""
    c = VC.halves(12, 9)
    for it in (1, 2, 3, 5):
        assert np.array_equal(_bits(VC.run(c, iterations=it, mistake=mistake)[..., 0:3]), _bits(c["image"][..., 0:3])), it
    big = VC.halves(12, 9, variance=100.0)
    out = VC.run(big, iterations=1, mistake=mistake)
    assert (out[:, 4:8, 0] < f32(0.5)).all() and (out[:, 4:8, 0] > f32(0.25)).all() and np.array_equal(_bits(out[:, 0:4, 0:3]), _bits(big["image"][:, 0:4, 0:3]))


def check_g_is_the_gaussian_of_the_neighbours(mistake=None):
    """one pixel of variance 0 among pixels of variance 1, beside the edge of two halves: g = 3/4 (the centre's quarter is missing), so it blends with the other half;
    with g = v_p it would reject it"""
    c = VC.halves(12, 9, variance=1.0); c["moments"][4, 5, 1] = f32(0.0)
    I, v, nd = _entries(c, mistake=mistake)
    _given(v[4, 5] == 0 and v.sum() == 12 * 9 - 1)
    want, want_v, g = VC.scalar_level(I, v, nd, 5, 4, 1)
    _given(g == f32(0.75))
    I2, v2 = V.level(I, v, nd, 1, *SIGMAS, mistake=mistake)
    assert np.array_equal(_bits(I2[4, 5]), _bits(want)) and _bits(v2[4, 5]) == _bits(want_v) and f32(0.25) < I2[4, 5, 0] < f32(0.5)


def check_g_is_taken_at_distance_1(mistake=None):
    """at step 2, variance 1 on the eight adjacent pixels only: g = 3/4 from distance 1; at distance 2 it would be 0 and reject the other half"""
    c = VC.halves(12, 9, variance=0.0); c["moments"][3:6, 4:7, 1] = f32(1.0); c["moments"][4, 5, 1] = f32(0.0)
    I, v, nd = _entries(c, mistake=mistake)
    want, want_v, g = VC.scalar_level(I, v, nd, 5, 4, 2)
    _given(g == f32(0.75))
    I2, v2 = V.level(I, v, nd, 2, *SIGMAS, mistake=mistake)
    assert np.array_equal(_bits(I2[4, 5]), _bits(want)) and _bits(v2[4, 5]) == _bits(want_v) and f32(0.25) < I2[4, 5, 0] < f32(0.5)


def check_g_is_renormalised_at_the_image_edge(mistake=None):
    """the corner's g over its four taps inside is (9/16 v) / (9/16) = v exactly; unnormalised it is 9/16 v and the colour term a quarter tighter"""
    c = VC.halves(4, 3, variance=1.0)
    I, v, nd = _entries(c, mistake=mistake)
    want, want_v, g = VC.scalar_level(I, v, nd, 1, 0, 1)
    _given(g == 1)
    I2, v2 = V.level(I, v, nd, 1, *SIGMAS, mistake=mistake)
    assert np.array_equal(_bits(I2[0, 1]), _bits(want)) and _bits(v2[0, 1]) == _bits(want_v) and f32(0.25) < I2[0, 1, 0] < f32(0.5)


def check_sigma_color_is_not_divided_by_the_step(mistake=None):
    c = VC.halves(16, 9, variance=0.01)
    I, v, nd = _entries(c, mistake=mistake)
    for step in (2, 4):
        want, want_v, _ = VC.scalar_level(I, v, nd, 7, 4, step)
        I2, v2 = V.level(I, v, nd, step, *SIGMAS, mistake=mistake)
        assert np.array_equal(_bits(I2[4, 7]), _bits(want)) and _bits(v2[4, 7]) == _bits(want_v), step
    # den = 4 * 0.1 + 1e-6 against a luminance step of 0.25: accepted at every level; divided by a step of 4 it is 0.1 and rejects
    assert f32(0.25) < V.level(I, v, nd, 4, *SIGMAS, mistake=mistake)[0][4, 7, 0] < f32(0.5)


def check_the_boost(mistake=None):
    """the spatial estimate of a two-valued pattern — m1 = m2 in {0, 1/2} on a chessboard, every k = 1 — is exact: an interior pixel's window holds 25 and 24 of the two
    values, M1 = M2 = 12/49 (or 12.5/49), and v = (M2 - M1^2) * 4 / len"""
    c = VC.known_answer_cases()[9][1]
    _given(VC.known_answer_cases()[9][0] == "two_valued_moments")
    for ln, boost in ((1.0, 4.0), (2.0, 2.0), (3.0, f32(4.0) / f32(3.0)), (0.5, 4.0), (np.nan, 4.0)):
        c["moments"][..., 3] = f32(ln)
        _, v, _ = _entries(c, mistake=mistake)
        for (y, x) in ((5, 5), (5, 4)):
            halfs = 24 if (x + y) % 2 == 0 else 25          # how many of the window's 49 hold 1/2
            M = f32(halfs * 0.5) / f32(49.0)
            want = (M - M * M) * f32(boost)
            assert _bits(v[y, x]) == _bits(want) and _bits(v[y, x]) == _bits(VC.scalar_spatial(c, x, y)), (ln, y, x, v[y, x], want)
        assert _bits(v[0, 0]) == _bits(VC.scalar_spatial(c, 0, 0)) and _bits(v[10, 3]) == _bits(VC.scalar_spatial(c, 3, 10))          # 16 and 28 taps inside


def check_the_switch_between_the_estimates(mistake=None):
    """len = 4 takes the pixel's own moments, len = 3.999 its neighbourhood's"""
    c = VC.known_answer_cases()[9][1]
    c["moments"][..., 3] = f32(3.999); c["moments"][5, 5, 3] = f32(4.0); c["moments"][5, 7, 3] = f32(4.5)
    info = {}
    I, v, A, cov = V.prepass(c["image"], c["moments"], c["normal_depth"], c["albedo"], mistake=mistake, info=info)
    m1 = c["moments"][..., 0]
    assert info["long_history"].sum() == 2 and _bits(v[5, 5]) == _bits(m1[5, 5] - m1[5, 5] * m1[5, 5]) and _bits(v[5, 7]) == _bits(m1[5, 7] - m1[5, 7] * m1[5, 7])
    assert _bits(v[5, 6]) == _bits(VC.scalar_spatial(c, 6, 5)) and v[5, 6] != v[5, 5]


def check_uncovered_pixels_and_nan(mistake=None):
    """pixels that are not covered pass through to the bit at every iteration count and a NaN behind them — image, moments, guide — or outside reaches no covered output"""
    c = VC.nan_behind_uncovered()
    un = c["albedo"][..., 3] == 0
    for it in (1, 2, 3, 4, 5):
        out = VC.run(c, iterations=it, mistake=mistake)
        assert np.array_equal(_bits(out[un][:, 0:3]), _bits(c["image"][un][:, 0:3])) and (out[..., 3] == 1).all(), it
        assert np.isfinite(out[~un]).all(), it
        assert np.array_equal(_bits(out[~un][:, 0:3]), _bits(c["image"][~un][:, 0:3])), it          # (a flat image: every covered pixel is its own value again)
    r = VC.random_case((33, 17), 5)
    un = r["albedo"][..., 3] == 0
    out = VC.run(r, mistake=mistake)
    _given(un.sum() > 40 and np.isnan(r["moments"][un]).all())
    assert np.isfinite(out[~un]).all() and np.array_equal(_bits(out[un][:, 0:3]), _bits(r["image"][un][:, 0:3]))
    # a pixel of variance 0 is covered: it is filtered and is a tap
    z = VC.halves(12, 9, variance=100.0); z["moments"][4, 5, 1] = f32(0.0)
    assert f32(0.25) < VC.run(z, iterations=1, mistake=mistake)[4, 5, 0] < f32(0.5)


CHECK_OF = {"w_not_squared": check_flat_image, "wsum_not_squared": check_flat_image, "g_is_v_p": check_g_is_the_gaussian_of_the_neighbours, "g_at_step": check_g_is_taken_at_distance_1,
            "no_boost": check_the_boost, "history_gt": check_the_switch_between_the_estimates, "sentinel_eq_0": check_uncovered_pixels_and_nan,
            "sigma_over_step": check_sigma_color_is_not_divided_by_the_step, "g_not_renormalised": check_g_is_renormalised_at_the_image_edge}


def test_flat_image_interior_corner_and_edge(): check_flat_image()
def test_two_halves_reject_at_variance_0_and_blend_at_a_large_one(): check_two_halves()
def test_g_is_the_gaussian_of_the_neighbours_not_the_pixels_own_variance(): check_g_is_the_gaussian_of_the_neighbours()
def test_g_is_taken_at_distance_1_at_every_level(): check_g_is_taken_at_distance_1()
def test_g_is_renormalised_at_the_image_edge(): check_g_is_renormalised_at_the_image_edge()
def test_sigma_color_is_in_standard_deviations_at_every_level(): check_sigma_color_is_not_divided_by_the_step()
def test_the_boost_and_the_exact_spatial_estimate(): check_the_boost()
def test_the_switch_between_the_two_estimates_is_at_4(): check_the_switch_between_the_estimates()
def test_uncovered_pixels_pass_through_and_no_nan_reaches_a_covered_output(): check_uncovered_pixels_and_nan()


CHECKS = {f.__name__[6:]: f for f in (check_flat_image, check_two_halves, check_g_is_the_gaussian_of_the_neighbours, check_g_is_taken_at_distance_1,
                                      check_g_is_renormalised_at_the_image_edge, check_sigma_color_is_not_divided_by_the_step, check_the_boost,
                                      check_the_switch_between_the_estimates, check_uncovered_pixels_and_nan)}
# DESIGN.md §10t's table: under each mistake exactly these checks fail, each at a comparison of the filter's result — a set-up that no longer holds raises NotTheCase
FAILS_UNDER = {"w_not_squared": {"flat_image", "g_is_the_gaussian_of_the_neighbours", "g_is_renormalised_at_the_image_edge", "sigma_color_is_not_divided_by_the_step"},
               "wsum_not_squared": {"flat_image", "g_is_the_gaussian_of_the_neighbours", "g_is_renormalised_at_the_image_edge", "sigma_color_is_not_divided_by_the_step"},
               "g_is_v_p": {"g_is_the_gaussian_of_the_neighbours", "g_is_taken_at_distance_1", "uncovered_pixels_and_nan"},
               "g_at_step": {"g_is_taken_at_distance_1"},
               "no_boost": {"the_boost", "the_switch_between_the_estimates"},
               "history_gt": {"the_switch_between_the_estimates"},
               "sentinel_eq_0": {"uncovered_pixels_and_nan", "g_is_the_gaussian_of_the_neighbours", "g_is_taken_at_distance_1"},
               "sigma_over_step": {"sigma_color_is_not_divided_by_the_step", "g_is_taken_at_distance_1"},
               "g_not_renormalised": {"g_is_renormalised_at_the_image_edge"}}


@pytest.mark.parametrize("mistake", V.MISTAKES)
def test_each_mistake_fails_its_named_check(mistake):
    """the named check fails at one of its comparisons (NotTheCase, a broken set-up, would not count), and the set of checks that fail is the recorded one"""
    assert set(CHECK_OF) == set(V.MISTAKES) == set(FAILS_UNDER) and CHECK_OF[mistake].__name__[6:] in FAILS_UNDER[mistake]
    with pytest.raises(AssertionError):
        CHECK_OF[mistake](mistake)
    failed = set()
    for name, check in CHECKS.items():
        try: check(mistake)
        except AssertionError: failed.add(name)
    assert failed == FAILS_UNDER[mistake], (mistake, sorted(failed))


@pytest.mark.parametrize("size", [(16, 8), (17, 17), (33, 17), (64, 64), (15, 33), (1, 1), (63, 1), (64, 1), (65, 1), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_images_hold_every_feature(size):
    """the random images of the GPU test are not vacuous; float64 agrees with float32 to rounding"""
    c = VC.random_case(size, 100 + size[0])
    info = {}
    out = VC.run(c, info=info)
    un = c["albedo"][..., 3] == 0
    assert out.dtype == np.float32 and np.isfinite(out[~un]).all()
    if size[0] * size[1] >= 128:
        assert un.any() and info["long_history"].any() and info["short_history"].any() and (info["v"][~un] == 0).any() and (info["v"][~un] > 1).any()
        assert not np.array_equal(out[~un][:, 0:3], c["image"][~un][:, 0:3])
    if size == (33, 17):
        # dtype=np.float64 evaluates the same expressions in double precision.  On this image the two are not comparable pixel by pixel — a variance that is exactly 0
        # in float32 (m2 == m1 * m1 rounded) is 1e-8 in float64 and den = 1e-6 turns that into another set of taps —; on an image without such a pixel they agree to
        # rounding: five levels of at most 200 roundings of 2^-24 each, on values of at most 1/2
        wide = VC.run(c, dtype=np.float64)
        assert wide.dtype == np.float64 and np.isfinite(wide[~un]).all()
        smooth = VC.halves(12, 9, variance=100.0)
        assert np.abs(VC.run(smooth, dtype=np.float64) - VC.run(smooth)).max() <= 5 * 200 * 2.0 ** -24 * 0.5
        assert np.isnan(c["moments"][~un][:, 3]).any() and np.isnan(c["normal_depth"][un]).any()
        for kw in (dict(iterations=1), dict(iterations=3, sigma_color=1.0), dict(demodulate=0)):
            assert not np.array_equal(VC.run(c, **kw)[~un], out[~un]), kw


# ---------------------------------------------------------------- the moments
def test_moments_sample_is_the_luminance_of_the_demodulated_sample():
    rng = np.random.default_rng(1)
    s = (rng.random((40, 4)) * 3).astype(f32); a = rng.random((40, 4)).astype(f32)
    a[0:10, 3] = 0; a[10:15, 0:3] = f32(1e-4); s[:, 3] = np.nan
    out = V.moments_sample(s, a)
    A = np.where((a[:, 3:4] != 0), np.maximum(a[:, 0:3], f32(1e-3)), f32(1))
    l = np.array([VC.lum(s[i, 0:3] / A[i]) for i in range(40)], f32)
    assert out.dtype == np.float32 and np.array_equal(_bits(out[:, 0]), _bits(l)) and np.array_equal(_bits(out[:, 1]), _bits(l * l)) and not out[:, 2:4].any()
    plain = V.moments_sample(s, a, demodulate=0)
    assert np.array_equal(_bits(plain[:, 0]), _bits(np.array([VC.lum(s[i]) for i in range(40)], f32))) and np.array_equal(_bits(plain[0:10]), _bits(out[0:10]))


def test_moments_through_two_reprojection_calls_are_the_running_averages():
    """moments_sample + temporal_reference.reproject twice over a still world, frames 0 .. 5: m1 is the running average of l and m2 that of l * l, bit for bit against
    path_state_reference.fold_sample, with the colour's length in .w"""
    from test_temporal_cpu import _still_world
    size = (21, 13)
    n = size[0] * size[1]
    cam, s = _still_world(size, 1)
    nd, ids = T.guides_of(s)
    on = s["type"] == 1
    rng = np.random.default_rng(2)
    alb = rng.random((n, 4)).astype(f32); alb[:, 3] = on
    hist = np.zeros((n, 4), f32); mom = np.zeros((n, 4), f32)
    accum = np.full((n, 4), np.nan, f32)
    for f in range(6):
        sample = (rng.random((n, 4)) * 3.0).astype(f32)
        ms = V.moments_sample(sample, alb)
        hist = T.reproject(size, cam, cam, s, sample, nd, ids, hist, max_history=7.0)
        mom = T.reproject(size, cam, cam, s, ms, nd, ids, mom, max_history=7.0)
        _, accum = PS.fold_sample(ms, accum, f)
        assert np.array_equal(_bits(mom[on, 0:2]), _bits(accum[on, 0:2])) and not mom[on, 2].any(), f
        assert np.array_equal(_bits(mom[:, 3]), _bits(hist[:, 3])) and (mom[on, 3] == f + 1).all()
    assert (mom[on, 1] >= mom[on, 0] * mom[on, 0] * f32(0.999)).all() and on.sum() > 200


# ---------------------------------------------------------------- ABI, ffi and the C++ mirror
P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32
SAMPLE_ARGS = ["ctx", "width", "height", "d_sample", "d_albedo", "demodulate", "d_out", "hip_stream"]
FILTER_ARGS = ["ctx", "width", "height", "d_image", "d_moments", "d_normal_depth", "d_albedo", "d_workspace", "workspace_bytes", "d_out", "params", "hip_stream"]


def test_header_declares_the_entries_and_states_the_definition():
    raw = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", raw, re.M)
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, want in ((SAMPLE, SAMPLE_ARGS), (FILTER, FILTER_ARGS)):
        m = re.search(r"^(\w+) " + name + r"\((.*?)\);", code, re.M | re.S)
        assert m and m.group(1) == "int", f"{name} is not declared in include/mrt_abi.h"
        args = [" ".join(a.split()) for a in m.group(2).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == want
    assert args[0] == "MRTContext ctx" and args[3:7] == ["const void *d_image", "const void *d_moments", "const void *d_normal_depth", "const void *d_albedo"]
    assert args[7:] == ["void *d_workspace", "size_t workspace_bytes", "void *d_out", "const MRTDenoiseParams *params", "void *hip_stream"]
    assert re.search(r"^#define MRT_VARIANCE_MIN_HISTORY\s+4\.0f", raw, re.M) and re.search(r"^#define MRT_VARIANCE_EPSILON\s+1e-6f", raw, re.M)
    assert re.search(r"^#define MRT_VARIANCE_MAX_HEIGHT\s+524280\b", raw, re.M) and 524280 == 65535 * 8
    assert V.MIN_HISTORY == 4.0 and V.EPSILON == 1e-6
    start = raw.index("Variance-guided a-trous filter on DEVICE buffers")
    assert start > raw.index("} MRTReprojectParams;") and start < raw.index("device group (multi-GPU")          # after the reprojection block
    block = " ".join(re.sub(r"\n \*", "\n", raw[start:raw.index("#define MRT_VARIANCE_MIN_HISTORY")]).split())
    for words in ("k(x) = max(0, 1 - x)", "correctly rounded sqrt", "no fused multiply-add", "DEFINED as a second call of mrt_context_reproject_device", "d_out_p = {l, l * l, 0, 0}",
                  "A tap is skipped iff its v < 0 or it lies outside the image", "v = -1", "len_p >= MRT_VARIANCE_MIN_HISTORY: v_p = max(0, m2 - m1 * m1)", "a NaN len counts as shorter",
                  "7 x 7 window at distance 1, row-major from (-3, -3)", "w = k(xn)^2 * k(xz)^2", "the centre takes w = 1", "s1 += w * m1_q; s2 += w * m2_q; sw += w",
                  "v_p = max(0, M2 - M1 * M1) * (4 / max(len_p, 1))", "at distance 1 at every level", "1/4 centre, 1/8 edges, 1/16 corners", "g = gs / gw",
                  "den = sigma_color * sqrt(g) + MRT_VARIANCE_EPSILON", "w = ((h * k(xn)^2) * k(xz)^2) * k(xc)^2, the centre takes w = h", "sum += w * I_q; vs += (w * w) * v_q; wsum += w",
                  "I'_p = sum / wsum, v'_p = vs / (wsum * wsum)", "{I' * A_p, 1}", "IN STANDARD DEVIATIONS and is not divided by the step", "never multiplied by 0",
                  "height > MRT_VARIANCE_MAX_HEIGHT", "Renderer.draw does neither", "no stage makes d_prev_position", "not fed back into the colour history"):
        assert words in block, words


def test_ffi_matches_the_header(mrt):
    from metal_raytracing_amd import _ffi
    res, args = _ffi.SIGNATURES[SAMPLE]
    assert res is C.c_int and args == [P, I32, I32, P, P, I32, P, P]
    res, args = _ffi.SIGNATURES[FILTER]
    assert res is C.c_int and args == [P, I32, I32, P, P, P, P, P, SZ, P, C.POINTER(_ffi.DenoiseParams), P] and len(args) == len(FILTER_ARGS)
    for name in (SAMPLE, FILTER):
        fn = getattr(mrt.lib, name)                                                                    # the export
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert mrt.lib.mrt_abi_version() == 3 and _ffi.DENOISE_DEFAULTS == D.DEFAULTS
    assert list(inspect.signature(mrt.DeviceScene.moments_sample_device).parameters) == ["self", "sample", "albedo", "size", "demodulate", "out", "stream"]
    assert list(inspect.signature(mrt.DeviceScene.denoise_variance_device).parameters) == ["self", "image", "moments", "normal_depth", "albedo", "size", "iterations", "sigma_color",
                                                                                            "sigma_normal", "sigma_depth", "demodulate", "out", "workspace", "stream"]
    for fn, words in ((mrt.DeviceScene.moments_sample_device, ("l * l", "reproject_device", "prev_history")), (mrt.DeviceScene.denoise_variance_device, ("standard deviations", "7 x 7", "workspace"))):
        assert all(w in fn.__doc__ for w in words + ("copied or synchronised", "stream: as intersect_closest_device takes it")), fn.__name__


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use_variance.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*sample)(MRTContext, int, int, const void *, const void *, bool, void *, void *) = &mrt::Scene::momentsSampleDevice;\n"
                   "void (*filter)(MRTContext, int, int, const void *, const void *, const void *, const void *, void *, size_t, void *, const MRTDenoiseParams *, void *) =\n"
                   "    &mrt::Scene::denoiseVarianceDevice;\n"
                   "void (mrt::Renderer::*msample)(const void *, const void *, bool, void *, void *) = &mrt::Renderer::momentsSampleDevice;\n"
                   "void (mrt::Renderer::*mfilter)(const void *, const void *, const void *, const void *, void *, size_t, void *, const MRTDenoiseParams *, void *) =\n"
                   "    &mrt::Renderer::denoiseVarianceDevice;\n"
                   "static_assert(MRT_VARIANCE_MIN_HISTORY == 4.0f && MRT_VARIANCE_EPSILON == 1e-6f, \"\");\n"
                   "void use(MRTContext ctx, mrt::Renderer &r, void *img, void *mom, void *nd, void *al, void *work, void *out, void *stream) {\n"
                   "    MRTDenoiseParams p = {3, 2.0f, MRT_DENOISE_DEFAULT_SIGMA_NORMAL, MRT_DENOISE_DEFAULT_SIGMA_DEPTH, 1, {0, 0, 0}};\n"
                   "    mrt::Scene::momentsSampleDevice(ctx, 8, 8, img, al, true, mom, stream);\n"
                   "    mrt::Scene::denoiseVarianceDevice(ctx, 8, 8, img, mom, nd, al, work, mrt::Scene::denoiseWorkspaceBytes(8, 8), out, &p, stream);\n"
                   "    r.momentsSampleDevice(img, al, false, mom, nullptr);\n"
                   "    r.denoiseVarianceDevice(img, mom, nd, al, work, r.denoiseWorkspaceBytes(), out, nullptr, nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


# ---------------------------------------------------------------- refusals that need no device
def test_arguments_are_refused_before_the_context(mrt):
    """One assertion per refusal rule.  Every device pointer is a plausible address that is never dereferenced: each call returns before the context is looked at, and the
    call with nothing wrong is refused for its NULL context alone."""
    from metal_raytracing_amd._ffi import DenoiseParams
    lib = mrt.lib
    A, B, D_, E, W, O = (0x1000000 * k for k in (1, 2, 3, 4, 5, 7))                                     # 16-byte aligned, 16 MiB apart (the workspace has 32)
    w, h = 64, 48
    img = w * h * 16

    def refused(rc, *words):
        msg = lib.mrt_last_error().decode()
        return rc == INVALID and all(x in msg for x in words)

    # ---- the sample image
    def sample(width=w, height=h, smp=A, al=B, demodulate=1, out=O):
        return lib.mrt_context_moments_sample_device(None, width, height, smp, al, demodulate, out, None)

    assert refused(sample(), SAMPLE, "ctx is NULL") and refused(sample(demodulate=0), "ctx is NULL") and refused(sample(demodulate=7), "ctx is NULL")
    assert refused(sample(width=0), "width") and refused(sample(width=-3), "width") and refused(sample(height=0), "height") and refused(sample(width=2 ** 15, height=2 ** 15), "2^30")
    for kw, word in (("smp", "d_sample"), ("al", "d_albedo"), ("out", "d_out")):
        assert refused(sample(**{kw: None}), word, "NULL"), kw
        for off in (4, 8, 12): assert refused(sample(**{kw: dict(smp=A, al=B, out=O)[kw] + off}), word, "16-byte"), (kw, off)
    for kw, word, base in (("smp", "d_sample", A), ("al", "d_albedo", B)):
        for at in (base, base + img - 16, base - img + 16): assert refused(sample(out=at), "d_out overlaps " + word), (kw, hex(at))
        assert refused(sample(out=base + img), "ctx is NULL") and refused(sample(out=base - img), "ctx is NULL"), kw          # back to back is apart
    assert refused(sample(smp=A, al=A), "ctx is NULL")                                                  # inputs may share

    # ---- the filter
    def call(width=w, height=h, image=A, mom=B, nd=D_, al=E, work=W, nbytes=2 * img, out=O, params=None):
        return lib.mrt_context_denoise_variance_device(None, width, height, image, mom, nd, al, work, nbytes, out, params, None)

    def par(iterations=5, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.25, demodulate=1):
        return C.byref(DenoiseParams(iterations, sigma_color, sigma_normal, sigma_depth, demodulate))

    assert refused(call(), FILTER, "ctx is NULL") and refused(call(params=par()), "ctx is NULL") and refused(call(params=par(8, 1e30, 1e-30, 7.0, 0)), "ctx is NULL")
    assert refused(call(nbytes=2 * img + 5), "ctx is NULL")
    assert refused(call(width=0), "width") and refused(call(width=-3), "width") and refused(call(height=0), "height") and refused(call(height=-1), "height")
    assert refused(call(width=2 ** 15, height=2 ** 15), "2^30")
    assert refused(call(width=1, height=524281, out=2 ** 40), "height", "524280") and refused(call(width=1, height=2 ** 20, out=2 ** 40), "height", "524280")
    assert refused(call(width=1, height=524280, nbytes=2 ** 25, work=2 ** 41, out=2 ** 40), "ctx is NULL")                            # 65535 workgroups of 8 rows: the tallest image
    assert refused(call(params=par(iterations=0)), "iterations") and refused(call(params=par(iterations=9)), "iterations")
    for key in ("sigma_color", "sigma_normal", "sigma_depth"):
        for bad in (0.0, -1.0, float("nan"), float("inf")): assert refused(call(params=par(**{key: bad})), key), (key, bad)
    assert refused(call(params=par(demodulate=2)), "demodulate") and refused(call(params=par(demodulate=-1)), "demodulate")
    names = dict(image="d_image", mom="d_moments", nd="d_normal_depth", al="d_albedo", work="d_workspace", out="d_out")
    base = dict(image=A, mom=B, nd=D_, al=E, work=W, out=O)
    for kw, word in names.items():
        assert refused(call(**{kw: None}), word, "NULL"), kw
        for off in (4, 8, 12): assert refused(call(**{kw: base[kw] + off}), word, "16-byte"), (kw, off)
    assert refused(call(nbytes=2 * img - 1), "workspace_bytes") and refused(call(nbytes=0), "workspace_bytes")
    for kw in ("image", "mom", "nd", "al"):
        word = names[kw]
        for at in (base[kw], base[kw] + img - 16, base[kw] - img + 16): assert refused(call(out=at), "d_out overlaps " + word), (kw, hex(at))
        for at in (base[kw], base[kw] + img - 16, base[kw] - 2 * img + 16): assert refused(call(work=at, out=0x20000000), "d_workspace overlaps " + word), (kw, hex(at))
        assert refused(call(out=base[kw] + img), "ctx is NULL") and refused(call(work=base[kw] - 2 * img, out=0x20000000), "ctx is NULL"), kw
    for at in (W, W + 2 * img - 16, W - img + 16): assert refused(call(out=at), "d_out overlaps d_workspace"), hex(at)
    assert refused(call(out=W + 2 * img), "ctx is NULL") and refused(call(out=W - img), "ctx is NULL")
    assert refused(call(image=A, mom=A, nd=A, al=A), "ctx is NULL")                                     # inputs may share: nothing writes them


# ---------------------------------------------------------------- kernel resources
VGPR_CEILING = {"k_moments_sample": 13, "k_var_prepass": 49, "k_var_atrous_tileILi1ELb1E": 31, "k_var_atrous_tileILi1ELb0E": 44, "k_var_atrous_tileILi2ELb1E": 31,
                "k_var_atrous_tileILi2ELb0E": 34, "k_var_atrousILb1E": 48, "k_var_atrousILb0E": 50}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_variance_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed); the figures are the ones the compiler writes into the code object's metadata.  Eight kernels, 256 threads, no
    scratch; the tile kernels hold 20^2 * 32 and 24^2 * 32 bytes of LDS, the others none.  The VGPR ceilings are the recorded figures: a register
    regression fails here, not on a GPU."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert line.split()[-1] == "variance.o", "variance.o is the last object linked"
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "variance.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "variance.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in ("private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size", "vgpr_count"))
    assert len(kernels) == len(VGPR_CEILING), sorted(kernels)
    for key, ceiling in VGPR_CEILING.items():
        (name, (scratch, lds, threads, vgprs)), = [(n, k) for n, k in kernels.items() if key in n]
        print(f"{key}: {vgprs} VGPRs, {lds} B of LDS, {scratch} B of scratch")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert lds == (20 * 20 * 32 if "tileILi1" in key else 24 * 24 * 32 if "tileILi2" in key else 0), (name, lds)
        assert threads == 256, (name, threads)
        assert vgprs <= ceiling, (name, vgprs)
    src = open(os.path.join(CSRC, "variance.hip")).read()
    assert re.findall(r'#include "(\w+\.h)"', src) == ["variance.h"]
    assert re.findall(r'#include "(\w+\.h)"', open(os.path.join(CSRC, "variance.h")).read()) == ["scene_device.h"]


# ---------------------------------------------------------------- the direction of the quality gain
def _quality(frames, converged, size, sigma_color=None):
    hist, mom, nd, alb = VC.accumulate(frames, size)
    img = lambda a: VC.as_image(a, size)
    plain = D.denoise_reference(img(hist), img(nd), img(alb)).reshape(-1, 4)
    new = V.denoise_variance(img(hist), img(mom), img(nd), img(alb), sigma_color=sigma_color).reshape(-1, 4)
    return TC.rmse(hist, converged), TC.rmse(plain, converged), TC.rmse(new, converged)


def test_the_variance_guided_filter_beats_the_unfiltered_accumulation(mrt, orc):
    """The moved sequences of §10r — CornellScene 64 x 64, three steps of the camera; the two-level scene of test_instancing 64 x 48, a step every frame —, the oracle's
    one-frame samples, colour and moments reprojected by the reference, against 512 frames at the last camera.  RMSE measured when the default was confirmed (DESIGN.md
    §10t) — the reprojected accumulation, denoise_reference on it, the new filter: Cornell 0.0752 / 0.0652 / 0.0567, two-level 0.1107 / 0.1061 / 0.0970.  Only the
    direction against the unfiltered accumulation is asserted."""
    for name, (frames, converged), size in (("cornell", TC.quality_frames(mrt, orc), TC.QUALITY["size"]), ("two-level", VC.two_level_frames(mrt, orc), VC.QUALITY_TWO_LEVEL["size"])):
        e_hist, e_plain, e_new = _quality(frames, converged, size)
        print(f"RMSE {name}: reprojected {e_hist:.4f}, denoise_reference {e_plain:.4f}, variance-guided {e_new:.4f}")
        assert e_new < e_hist, (name, e_new, e_hist)
