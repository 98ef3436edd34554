"""Temporal reprojection on device buffers (mrt_context_reproject_device) as far as it can be checked without a GPU: the yardstick of the GPU tests
(tests/temporal_reference.py) against answers known exactly, one case per rejection rule, the two identities with the running average, the direction of the quality gain
against the oracle and the composed six-frame sequence in its CPU form; then the header, the ctypes mirror and the C++ one, every refusal that needs no device — each
reached with a NULL context, which is refused last — and the resources of the kernels of temporal.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import path_state_reference as PS
import temporal_cases as TC
import temporal_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
NAME = "mrt_context_reproject_device"
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- the reference against answers known exactly
@pytest.mark.parametrize("c", TC.known_answer_cases() + TC.rejection_cases(), ids=lambda c: c["name"])
def test_known_answers_and_rejections(c):
    """every checked pixel blends exactly the taps the case names, with their exact weights in the stated order — or restarts at its sample"""
    info = {}
    out = TC.run_reference(c, info=info)
    assert out.dtype == np.float32 and out.shape == (TC.W * TC.H, 4) and c["checks"]
    for pixel, taps in c["checks"].items():
        want = TC.blend(c, pixel, taps)
        assert np.array_equal(_bits(out[pixel]), _bits(want)), (c["name"], pixel, out[pixel], want)
        assert np.isfinite(out[pixel]).all(), (c["name"], pixel, out[pixel])
        assert int(info["valid"][:, pixel].sum()) == len(taps), (c["name"], pixel)
    if c["name"].startswith(("still", "one_pixel", "half_pixel", "quarter")): assert info["kept"].sum() >= 24          # the blocks' inner pixels go on


def test_the_exact_camera_projects_pixel_centres_exactly():
    for z in (1.0, 2.0):
        px, py, d2, ok = T.project(TC.EXACT_CAMERA, TC.grid_points(z=z), TC.W, TC.H)
        p = np.arange(TC.W * TC.H)
        assert ok.all() and np.array_equal(px, p % TC.W + f32(0.5)) and np.array_equal(py, p // TC.W + f32(0.5))
    # projection inverts the ray generation for a basis that is neither aligned nor orthogonal: pixel + jitter comes back to a few ulps of the image size
    rng = np.random.default_rng(3)
    cam = TC.tilted_camera(2)
    size = (33, 17)
    fx = rng.random(500).astype(f32) * f32(33); fy = rng.random(500).astype(f32) * f32(17)
    px, py, d2, ok = T.project(cam, TC.unproject(cam, fx, fy, rng.random(500).astype(f32) * f32(5) + f32(0.5), size), *size)
    assert ok.all() and np.abs(px - fx).max() < 1e-4 and np.abs(py - fy).max() < 1e-4
    behind = TC.unproject(cam, fx, fy, -np.ones(500, f32), size)
    assert not T.project(cam, behind, *size)[3].any()


@pytest.mark.parametrize("size", [(16, 8), (33, 17), (64, 64), (1, 1), (63, 1), (64, 1), (65, 1), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_images_hold_every_feature(size):
    """the random images of the GPU test are not vacuous, and nothing a rejection leaves unread reaches an output"""
    c = TC.random_case(size, 100 + size[0])
    info = {}
    out = TC.run_reference(c, info=info)
    assert np.isfinite(out).all(), "a word behind a rejection leaked"
    assert np.isnan(c["prev_history"]).any() or size[0] * size[1] < 8
    if size == (33, 17):
        on = info["on"] & info["projected"]
        live = on[None] & info["read"]
        assert (~info["on"]).any() and info["kept"].sum() > 100 and (on & ~info["kept"]).sum() > 20
        for k in ("inside", "ids", "normal", "depth", "length"): assert (live & ~info[k]).any() and (live & info[k]).any(), k
        assert (info["valid"].sum(0) == 4).any() and (info["valid"].sum(0) == 1).any()          # full bilinear fetches, and partial ones
        lens = np.unique(out[:, 3])
        assert lens.min() == 1.0 and lens.max() == 32.0 and ((lens > 1) & (lens < 32) & (lens != np.round(lens))).any()
        assert np.abs(info["fx"] - np.arange(33 * 17) % 33)[info["on"]].max() > 2.5


# ---------------------------------------------------------------- the two identities
def _still_world(size, seed):
    """a still image of surfaces and misses under one camera, per-frame samples, and this frame's ids as the previous frame's"""
    w, h = size
    n = w * h
    rng = np.random.default_rng(seed)
    cam = TC.tilted_camera(0)
    p = np.arange(n)
    depth = f32(2.0) + rng.random(n).astype(f32)
    q = TC.unproject(cam, (p % w).astype(f32) + rng.random(n).astype(f32), (p // w).astype(f32) + rng.random(n).astype(f32), depth, size)
    nrm = rng.standard_normal((n, 3)).astype(f32)
    nrm = nrm / np.sqrt(T._dot(nrm, nrm))[:, None]
    s = T.surfaces_of(q, nrm, instance=rng.integers(0, 5, n), geometry=rng.integers(0, 3, n), primitive=p, distance=np.sqrt(T._dot(q - cam[0], q - cam[0])))
    s["type"][rng.random(n) < 0.1] = 0
    return cam, s


def test_a_still_world_is_the_running_average_bit_for_bit():
    """equal cameras, no previous position, max_history above the frame count: frames 0 .. 5 give fold_sample's accumulation in rgb, every bit, on surfaces; a miss
    restarts at its sample every frame"""
    size = (21, 13)
    n = size[0] * size[1]
    cam, s = _still_world(size, 1)
    nd, ids = T.guides_of(s)
    on = s["type"] == 1
    rng = np.random.default_rng(2)
    hist = np.zeros((n, 4), f32)
    accum = np.full((n, 4), np.nan, f32)
    for f in range(6):
        sample = (rng.random((n, 4)) * 3.0).astype(f32)
        hist = T.reproject(size, cam, cam, s, sample, nd, ids, hist, max_history=7.0)
        _, accum = PS.fold_sample(sample, accum, f)
        assert np.array_equal(_bits(hist[on, 0:3]), _bits(accum[on, 0:3])), f
        assert (hist[on, 3] == f + 1).all() and np.array_equal(_bits(hist[~on]), _bits(np.concatenate([sample[~on, 0:3], np.ones(((~on).sum(), 1), f32)], 1)))
    assert on.sum() > 200 and (~on).sum() > 10


def test_a_clamped_history_is_the_exponential_average():
    size = (21, 13)
    n = size[0] * size[1]
    cam, s = _still_world(size, 4)
    nd, ids = T.guides_of(s)
    on = s["type"] == 1
    rng = np.random.default_rng(5)
    M = 4
    hist = np.zeros((n, 4), f32)
    for f in range(9):
        sample = (rng.random((n, 4)) * 3.0).astype(f32)
        new = T.reproject(size, cam, cam, s, sample, nd, ids, hist, max_history=float(M))
        if f >= M:
            want = (sample[:, 0:3] + hist[:, 0:3] * f32(M - 1)) / f32(M)
            assert np.array_equal(_bits(new[on, 0:3]), _bits(want[on])) and (new[on, 3] == M).all(), f
        else:
            assert (new[on, 3] == f + 1).all()
        hist = new
    # clamped before the blend, not after: max_history 1 keeps nothing of the history
    one = T.reproject(size, cam, cam, s, sample, nd, ids, hist, max_history=1.0)
    assert np.array_equal(_bits(one[:, 0:3]), _bits(sample[:, 0:3])) and (one[:, 3] == 1).all()


# ---------------------------------------------------------------- ABI, ffi and the C++ mirror
P, SZ, I32, U32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32
ARGS = ["ctx", "width", "height", "camera", "prev_camera", "d_surfaces", "d_prev_position", "d_prev_normal_depth", "d_prev_ids", "d_prev_history", "d_sample", "d_out", "params",
        "hip_stream"]


def _header_text():
    return open(os.path.join(ROOT, "include", "mrt_abi.h")).read()


def test_header_declares_the_entry_and_states_the_definition():
    raw = _header_text()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", raw, re.M)
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"^(\w+) " + NAME + r"\((.*?)\);", code, re.M | re.S)
    assert m and m.group(1) == "int", f"{NAME} is not declared in include/mrt_abi.h"
    args = [a.strip() for a in m.group(2).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert args[0] == "MRTContext ctx" and args[1] == "int32_t width" and args[2] == "int32_t height" and args[3] == "const MRTCamera *camera" and args[4] == "const MRTCamera *prev_camera"
    assert all(a.startswith("const void *") for a in args[5:11]) and args[11] == "void *d_out" and args[12] == "const MRTReprojectParams *params" and args[13] == "void *hip_stream"
    s = re.search(r"typedef struct \{([^}]*)\} MRTReprojectParams;", code)
    assert s and re.findall(r"(\w+)\s+(\w+);", s.group(1)) == [("float", "max_history"), ("float", "min_cos_normal"), ("float", "depth_tolerance"), ("int32_t", "_pad")]
    for macro, value in (("MAX_HISTORY", "32.0f"), ("MIN_COS_NORMAL", "0.9f"), ("DEPTH_TOLERANCE", "0.1f")):
        assert re.search(rf"^#define MRT_REPROJECT_DEFAULT_{macro}\s+{re.escape(value)}", raw, re.M), macro
    assert T.DEFAULTS == dict(max_history=32.0, min_cos_normal=0.9, depth_tolerance=0.1)
    # the definition is written into the header: the expressions the reference and the kernel follow
    block = " ".join(re.sub(r"\n \*", "\n", raw[raw.index("Temporal reprojection of the accumulated image"):raw.index("} MRTReprojectParams;")]).split())
    for words in ("nx = cross(up, forward), ny = cross(forward, right), nz = cross(right, up), det = dot(right, nx)", "fails unless c > 0", "px = ((a / c + 1) * 0.5) * (float)width",
                  "fx = (float)x + (P0.px - P1.px)", "(0,0), (1,0), (0,1), (1,1)", "w = (i ? ax : 1 - ax) * (j ? ay : 1 - ay)", "A tap of weight 0 is not read",
                  "decided before any conversion to an integer", "dot(prev_n, cur.normal) >= min_cos_normal", "fabs(t_prev * t_prev - P0.d2) <= depth_tolerance * P0.d2",
                  "history.w >= 1", "the primitive is not compared", "sw += w; sc += w * history.rgb; sl += w * history.w", "len = min(sl / sw + 1, max_history)",
                  "out = {(sample.rgb + hist * (len - 1)) / len, len}", "no fused multiply-add", "no square root"):
        assert words in block, words


def test_ffi_matches_the_header(mrt):
    import inspect
    from metal_raytracing_amd import _ffi
    res, args = _ffi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == len(ARGS)
    assert args[0] is P and args[1] is I32 and args[2] is I32 and args[3] is C.POINTER(_ffi.Camera) and args[4] is C.POINTER(_ffi.Camera)
    assert all(a is P for a in args[5:12]) and args[12] is C.POINTER(_ffi.ReprojectParams) and args[13] is P
    fn = getattr(mrt.lib, NAME)                                                                        # the export
    assert fn.restype is res and list(fn.argtypes) == args
    assert C.sizeof(_ffi.ReprojectParams) == 16 and [(n, t) for n, t in _ffi.ReprojectParams._fields_] == [("max_history", C.c_float), ("min_cos_normal", C.c_float),
                                                                                                          ("depth_tolerance", C.c_float), ("_pad", C.c_int32)]
    assert [getattr(_ffi.ReprojectParams, n).offset for n, _ in _ffi.ReprojectParams._fields_] == [0, 4, 8, 12]
    assert _ffi.REPROJECT_DEFAULTS == T.DEFAULTS and mrt.ReprojectParams is _ffi.ReprojectParams
    assert mrt.lib.mrt_abi_version() == 3
    assert list(inspect.signature(mrt.DeviceScene.reproject_device).parameters) == ["self", "surfaces", "sample", "prev_normal_depth", "prev_ids", "prev_history", "size", "camera",
                                                                                     "prev_camera", "prev_position", "max_history", "min_cos_normal", "depth_tolerance", "out", "stream"]
    doc = mrt.DeviceScene.reproject_device.__doc__
    assert all(w in doc for w in ("fold_guides_device", "prev_position", "max_history", "nothing is allocated", "stream: as intersect_closest_device takes it"))


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use_temporal.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*reproject)(MRTContext, int, int, const mrt::Camera &, const mrt::Camera &, const void *, const void *, const void *, const void *, const void *, const void *, void *,\n"
                   "                  const MRTReprojectParams *, void *) = &mrt::Scene::reprojectDevice;\n"
                   "void (mrt::Renderer::*member)(const mrt::Camera &, const mrt::Camera &, const void *, const void *, const void *, const void *, const void *, const void *, void *,\n"
                   "                              const MRTReprojectParams *, void *) = &mrt::Renderer::reprojectDevice;\n"
                   "static_assert(sizeof(MRTReprojectParams) == 16, \"\");\n"
                   "void use(MRTContext ctx, mrt::Renderer &r, const mrt::Camera &a, const mrt::Camera &b, void *s, void *nd, void *ids, void *hist, void *smp, void *out, void *stream) {\n"
                   "    MRTReprojectParams p = {MRT_REPROJECT_DEFAULT_MAX_HISTORY, MRT_REPROJECT_DEFAULT_MIN_COS_NORMAL, MRT_REPROJECT_DEFAULT_DEPTH_TOLERANCE, 0};\n"
                   "    mrt::Scene::reprojectDevice(ctx, 8, 8, a, b, s, nullptr, nd, ids, hist, smp, out, &p, stream);\n"
                   "    r.reprojectDevice(a, b, s, s, nd, ids, hist, smp, out, nullptr, nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "temporal_host.cpp")])


# ---------------------------------------------------------------- refusals that need no device
def test_arguments_are_refused_before_the_context(mrt):
    """One assertion per refusal rule.  Every device pointer is a plausible address that is never dereferenced: each call returns before the context is looked at, and the
    call with nothing wrong is refused for its NULL context alone."""
    from metal_raytracing_amd._ffi import Camera, ReprojectParams
    lib = mrt.lib
    A, B, D_, E, F, G, O = (0x1000000 * k for k in range(1, 8))                                         # 16-byte aligned, 16 MiB apart
    w, h = 64, 48
    img = w * h * 16
    cam = Camera()

    def refused(rc, *words):
        msg = lib.mrt_last_error().decode()
        return rc == INVALID and all(x in msg for x in words)

    def call(width=w, height=h, camera=cam, prev_camera=cam, surf=A, pos=B, nd=D_, ids=E, hist=F, sample=G, out=O, params=None):
        cp = lambda c: None if c is None else C.byref(c)
        return lib.mrt_context_reproject_device(None, width, height, cp(camera), cp(prev_camera), surf, pos, nd, ids, hist, sample, out, params, None)

    def par(max_history=32.0, min_cos_normal=0.9, depth_tolerance=0.1):
        return C.byref(ReprojectParams(max_history, min_cos_normal, depth_tolerance, 0))

    assert refused(call(), NAME, "ctx is NULL")                                                         # NULL = the defaults
    assert refused(call(pos=None), "ctx is NULL")                                                       # the geometry did not move
    assert refused(call(params=par()), "ctx is NULL")
    assert refused(call(params=par(1.0, -1.0, 0.0)), "ctx is NULL") and refused(call(params=par(1e30, float("inf"), float("inf"))), "ctx is NULL")
    assert refused(call(width=2 ** 24 - 1, height=1, out=2 ** 40), "ctx is NULL") and refused(call(width=1, height=2 ** 24 - 1, out=2 ** 40), "ctx is NULL")          # (256 MiB images)
    assert refused(call(width=0), "width") and refused(call(width=-3), "width") and refused(call(height=0), "height") and refused(call(height=-1), "height")
    assert refused(call(width=2 ** 24, height=1), "width", "2^24") and refused(call(width=1, height=2 ** 24), "height", "2^24")
    assert refused(call(width=2 ** 15, height=2 ** 15), "2^30")
    assert refused(call(camera=None), " camera is NULL") and refused(call(prev_camera=None), "prev_camera is NULL")
    for bad in (0.5, 0.0, -1.0, float("nan"), float("inf")):
        assert refused(call(params=par(max_history=bad)), "max_history"), bad
    assert refused(call(params=par(min_cos_normal=float("nan"))), "min_cos_normal")
    assert refused(call(params=par(depth_tolerance=float("nan"))), "depth_tolerance") and refused(call(params=par(depth_tolerance=-0.01)), "depth_tolerance")
    names = dict(surf="d_surfaces", pos="d_prev_position", nd="d_prev_normal_depth", ids="d_prev_ids", hist="d_prev_history", sample="d_sample", out="d_out")
    base = dict(surf=A, pos=B, nd=D_, ids=E, hist=F, sample=G, out=O)
    for kw, word in names.items():
        if kw != "pos": assert refused(call(**{kw: None}), word, "NULL"), kw
        for off in (4, 8, 12): assert refused(call(**{kw: base[kw] + off}), word, "16-byte"), (kw, off)
    # d_out against every input, byte ranges: the last row of one on the first of the other, both ways round
    for kw, word in names.items():
        if kw == "out": continue
        size = 4 * img if kw == "surf" else img
        for at in (base[kw], base[kw] + size - 16, base[kw] - img + 16):
            assert refused(call(out=at), "d_out overlaps " + word), (kw, hex(at))
        assert refused(call(out=base[kw] + size, **({"pos": None} if kw == "surf" else {})), "ctx is NULL") and refused(call(out=base[kw] - img), "ctx is NULL"), kw          # back to back is apart
    assert refused(call(pos=None, out=B), "ctx is NULL")
    assert refused(call(nd=A, ids=A, hist=A, sample=A, pos=A), "ctx is NULL")                           # inputs may share: nothing writes them


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_temporal_kernels_use_no_scratch_no_lds_and_16_byte_accesses(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed); the figures are the ones the compiler writes into the code object's metadata.  Two kernels — with and without
    a previous position —, 256 threads, no scratch, no LDS, no atomics; every access to memory is 16 bytes wide but the surface row's, of which the compiler may leave out
    the words the stage does not use; one store.  The VGPR ceilings are the recorded figures: a register regression fails here, not on a GPU."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "temporal.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "temporal.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "temporal.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in ("private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size", "vgpr_count"))
    assert len(kernels) == 2 and all("k_reproject" in k for k in kernels) and sum("ILb1E" in k for k in kernels) == 1, sorted(kernels)
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S)}
    assert set(bodies) == set(kernels)
    for name, (scratch, lds, threads, vgprs) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert threads == 256, f"{name}: {threads} threads per workgroup"
        assert vgprs <= VGPR_CEILING["ILb1E" in name], (name, vgprs)
        body = bodies[name]
        assert not re.search(r"^\s*(?:ds_|global_atomic|flat_atomic|buffer_atomic|scratch_)", body, re.M), f"{name}: LDS, atomics or scratch"
        stores = re.findall(r"^\s*(?:global|flat|buffer)_store_(\w+)", body, re.M)
        assert stores and set(stores) == {"dwordx4"}, (name, stores)
        loads = re.findall(r"^\s*(?:global|flat|buffer)_load_(\w+)", body, re.M)
        narrow = [l for l in loads if l != "dwordx4"]
        # four taps x (ids, normal | depth, history), the sample, the row's normal | type, MOVED the previous position: one 16-byte load each; what is narrower is the
        # surface row's position and ids groups, of which the stage uses three and two words
        assert loads.count("dwordx4") == 14 + ("ILb1E" in name) and 2 <= len(narrow) <= 3, (name, loads)
        assert not re.search(r"v_sqrt_f32|v_rsq_f32", body), f"{name}: a square root"
    src = open(os.path.join(CSRC, "temporal.hip")).read()
    assert re.findall(r'#include "(\w+\.h)"', src) == ["temporal.h", "device_math.h"]
    assert re.findall(r'#include "(\w+\.h)"', open(os.path.join(CSRC, "temporal.h")).read()) == ["scene_device.h"]


VGPR_CEILING = {False: 52, True: 54}          # [MOVED]: DESIGN.md §10r


# ---------------------------------------------------------------- the direction of the quality gain, and the composed sequence in its CPU form
def test_reprojection_beats_one_sample_and_a_restart_at_every_move(mrt, orc):
    """A short camera move over CornellScene 64 x 64 (eight frames, a step before frames 2, 4 and 6), the oracle's one-frame samples, against 512 frames at the last
    camera.  Measured when the defaults were confirmed: RMSE of the last sample 0.1232, of the average restarted at every move 0.0925, of the
    reprojected accumulation 0.0752.  Only the direction is asserted."""
    frames, converged = TC.quality_frames(mrt, orc)
    hist, restart, sample = TC.quality_run(frames)
    e_hist, e_restart, e_sample = TC.rmse(hist, converged), TC.rmse(restart, converged), TC.rmse(sample, converged)
    print(f"RMSE: last sample {e_sample:.4f}, restarted average {e_restart:.4f}, reprojected {e_hist:.4f}")
    assert e_hist < e_sample and e_hist < e_restart, (e_hist, e_restart, e_sample)


def test_the_composed_sequence_on_the_cpu_is_not_vacuous(mrt, orc):
    """Six frames of a two-level scene at 48 x 32 with the camera moving a little each frame and one instance moving (tests/temporal_cases.py cpu_sequence: the oracle's
    queries, the reference modules' rows) — the sequence tests/test_temporal_device.py composes from the stage entries.  The motion is chosen so that the reference
    alone shows every effect: from frame 1 on at least half of the surface pixels keep their history, and some lose it to each of leaving the image, another surface at
    the moving instance's silhouette, and the depth test."""
    frames = TC.cpu_sequence(mrt, orc)
    assert len(frames) == 6 and (frames[0]["out"][:, 3] == 1).all()
    for k, c in enumerate(frames[1:], 1):
        L = TC.sequence_losses(c)
        on = c["surfaces"]["type"] == 1
        assert on.sum() > 500 and (~on).sum() > 300 and ((c["surfaces"]["instance_id"] == TC.SEQUENCE["mover"]) & on).sum() >= 10, k
        assert (c["out"][on, 3] > 1).sum() * 2 >= on.sum(), (k, (c["out"][on, 3] > 1).sum(), on.sum())
        for why in ("outside", "ids", "depth"): assert L[why].any(), (k, why)
        assert not np.array_equal(c["camera"], c["prev_camera"]) and not np.array_equal(c["prev_position"][:, 0:3], c["surfaces"]["position"])
        assert c["out"][:, 3].max() > k and np.isfinite(c["out"]).all()
