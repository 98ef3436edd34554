"""The path-state entries (mrt_context_reset_paths_device / _advance_paths_device / _deposit_light_device / _fold_sample_device) as far as they can be
checked without a GPU: the header, the ctypes mirror and the C++ one, every refusal that needs no device — each reached with a NULL context, which is refused last — the
resources of the kernels of paths.hip, and the yardstick of the GPU tests (tests/path_state_reference.py) pinned to the oracle's image through a frame composed on queues."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import path_state_reference as PS
import stages_materials_reference as M
import stages_reference as R
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
RESET, ADVANCE, DEPOSIT, FOLD = ("mrt_context_reset_paths_device", "mrt_context_advance_paths_device", "mrt_context_deposit_light_device", "mrt_context_fold_sample_device")
P, SZ, I32, U32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32
WANT = {RESET: [P, SZ, "pointer", "pointer", "pointer", SZ, "pointer"],
        ADVANCE: [P, SZ] + ["pointer"] * 7 + [SZ, "pointer", "pointer", "pointer"],
        DEPOSIT: [P, SZ] + ["pointer"] * 6 + [SZ, "pointer"],
        FOLD: [P, SZ, "pointer", "pointer", U32, I32, "pointer"]}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrt_abi.h")).read(), flags=re.S)


def _ctype_of(arg):
    arg = arg.strip()
    if "*" in arg: return "pointer"
    return {"size_t": SZ, "int32_t": I32, "uint32_t": U32, "MRTContext": P}[arg.split()[0]]


def _declared(name):
    m = re.search(r"^(\w+) " + name + r"\((.*?)\);", _header(), re.M | re.S)
    assert m, f"{name} is not declared in include/mrt_abi.h"
    return m.group(1), [_ctype_of(a) for a in m.group(2).split(",")], [a.split()[-1].lstrip("*") for a in m.group(2).split(",")]


# ---------------------------------------------------------------- ABI, ffi and the C++ mirror
def test_header_declares_the_four_functions():
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", open(os.path.join(ROOT, "include", "mrt_abi.h")).read(), re.M)
    for name, want in WANT.items():
        res, args, _ = _declared(name)
        assert res == "int" and args == want, name
    assert _declared(ADVANCE)[2] == ["ctx", "n", "d_count", "d_surfaces", "d_lobes", "d_light", "d_throughput", "d_pixel", "d_radiance", "npixels", "d_keep_shadow", "d_keep_path", "hip_stream"]
    assert _declared(DEPOSIT)[2] == ["ctx", "n", "d_count", "d_occluded", "d_light", "d_throughput", "d_pixel", "d_radiance", "npixels", "hip_stream"]
    assert _declared(RESET)[2] == ["ctx", "n", "d_throughput", "d_pixel", "d_radiance", "npixels", "hip_stream"]
    assert _declared(FOLD)[2] == ["ctx", "npixels", "d_sample", "d_accum", "frame_index", "clear_sample", "hip_stream"]


def test_ffi_matches_the_header(mrt):
    import inspect
    from metal_raytracing_amd import _ffi
    for name in WANT:
        res, args, _ = _declared(name)
        fres, fargs = _ffi.SIGNATURES[name]
        assert fres is C.c_int and len(fargs) == len(args), name
        for have, want in zip(fargs, args):
            assert have is (P if want == "pointer" else want), (name, have, want)
        fn = getattr(mrt.lib, name)
        assert fn.restype is fres and list(fn.argtypes) == fargs
    assert mrt.lib.mrt_abi_version() == 3
    sig = lambda m: list(inspect.signature(getattr(mrt.DeviceScene, m)).parameters)
    assert sig("reset_paths_device") == ["self", "n", "radiance", "out", "stream"]
    assert sig("advance_paths_device") == ["self", "light", "throughput", "pixel", "radiance", "surfaces", "lobes", "count", "keep_path", "out", "stream"]
    assert sig("deposit_light_device") == ["self", "occluded", "light", "throughput", "pixel", "radiance", "count", "stream"]
    assert sig("fold_sample_device") == ["self", "sample", "accum", "frame_index", "clear_sample", "stream"]


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use_paths.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*reset)(MRTContext, size_t, void *, void *, void *, size_t, void *) = &mrt::Scene::resetPathsDevice;\n"
                   "void (*advance)(MRTContext, size_t, const void *, const void *, const void *, const void *, void *, const void *, void *, size_t, void *, void *, void *) =\n"
                   "    &mrt::Scene::advancePathsDevice;\n"
                   "void (*deposit)(MRTContext, size_t, const void *, const void *, const void *, const void *, const void *, void *, size_t, void *) = &mrt::Scene::depositLightDevice;\n"
                   "void (*fold)(MRTContext, size_t, void *, void *, uint32_t, bool, void *) = &mrt::Scene::foldSampleDevice;\n"
                   "void use(MRTContext ctx, void *a, void *b, void *c, void *d, void *e, void *stream) {\n"
                   "    mrt::Scene::resetPathsDevice(ctx, 16, a, b, c, 16, stream);\n"
                   "    mrt::Scene::advancePathsDevice(ctx, 16, nullptr, d, nullptr, e, a, nullptr, nullptr, 0, b, nullptr, stream);\n"
                   "    mrt::Scene::depositLightDevice(ctx, 16, d, e, a, a, b, c, 16, stream);\n"
                   "    mrt::Scene::foldSampleDevice(ctx, 16, c, d, 3, true, nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


# ---------------------------------------------------------------- refusals that need no device
def test_arguments_are_refused_before_the_context(mrt):
    """One assertion per refusal rule.  Every pointer is a plausible address that is never dereferenced: each call returns before the context is looked at, and the call
    with nothing wrong is refused for its NULL context alone."""
    lib = mrt.lib
    A, B, D, E, F, G, H, K = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000          # 16-byte aligned, all different

    def last():
        return lib.mrt_last_error().decode()

    def refused(rc, *words):
        msg = last()
        return rc == INVALID and all(w in msg for w in words)

    # ---- reset
    def reset(n=100, thr=A, pix=B, rad=D, npix=100):
        return lib.mrt_context_reset_paths_device(None, n, thr, pix, rad, npix, None)

    assert refused(reset(), RESET, "ctx is NULL")
    assert refused(reset(rad=None), "ctx is NULL")                                                      # the image may be left out
    assert refused(reset(n=0, thr=None, pix=None, rad=None, npix=0), "ctx is NULL")
    assert refused(reset(thr=None), "d_throughput", "NULL")
    assert refused(reset(pix=None), "d_pixel", "NULL")
    assert refused(reset(thr=A + 8), "d_throughput", "16-byte")
    assert refused(reset(pix=B + 2), "d_pixel", "4-byte")
    assert refused(reset(pix=B + 4), "ctx is NULL")                                                     # 4-byte alignment is enough for an index word
    assert refused(reset(rad=D + 4), "d_radiance", "16-byte")
    assert refused(reset(n=2 ** 31), RESET, "n must be below 2^31")
    assert refused(reset(npix=2 ** 31), "npixels", "2^31")
    assert refused(reset(n=2 ** 31 - 1, npix=2 ** 31 - 1), "ctx is NULL")

    # ---- advance
    def advance(n=100, cnt=K, surf=E, lobes=None, light=F, thr=A, pix=B, rad=D, npix=100, ks=G, kp=H):
        return lib.mrt_context_advance_paths_device(None, n, cnt, surf, lobes, light, thr, pix, rad, npix, ks, kp, None)

    assert refused(advance(), ADVANCE, "ctx is NULL")
    assert refused(advance(surf=None, lobes=E), "ctx is NULL")                                          # the materials form
    assert refused(advance(cnt=None, kp=None, pix=None, rad=None), "ctx is NULL")                       # no count, no second mask; the diffuse form reads no image
    assert refused(advance(n=0, cnt=None, surf=None, light=None, thr=None, pix=None, rad=None, ks=None, kp=None), "ctx is NULL")
    assert refused(advance(lobes=E + 0x100), "both", "d_surfaces", "d_lobes")
    assert refused(advance(surf=None), "neither", "d_surfaces", "d_lobes")
    assert refused(advance(surf=None, lobes=E, pix=None), "d_pixel", "NULL", "materials")
    assert refused(advance(surf=None, lobes=E, rad=None), "d_radiance", "NULL", "materials")
    assert refused(advance(light=None), "d_light", "NULL")
    assert refused(advance(thr=None), "d_throughput", "NULL")
    assert refused(advance(ks=None), "d_keep_shadow", "NULL")
    assert refused(advance(cnt=K + 2), "d_count", "4-byte")
    assert refused(advance(surf=E + 8), "d_surfaces", "16-byte")
    assert refused(advance(surf=None, lobes=E + 4), "d_lobes", "16-byte")
    assert refused(advance(light=F + 8), "d_light", "16-byte")
    assert refused(advance(thr=A + 12), "d_throughput", "16-byte")
    assert refused(advance(pix=B + 1), "d_pixel", "4-byte")
    assert refused(advance(rad=D + 8), "d_radiance", "16-byte")
    assert refused(advance(ks=G + 1, kp=H + 3), "ctx is NULL")                                          # masks are bytes
    assert refused(advance(n=2 ** 31), ADVANCE, "n must be below 2^31")
    assert refused(advance(npix=2 ** 31), "npixels", "2^31")

    # ---- deposit
    def deposit(n=100, cnt=K, occ=E, light=F, thr=A, pix=B, rad=D, npix=100):
        return lib.mrt_context_deposit_light_device(None, n, cnt, occ, light, thr, pix, rad, npix, None)

    assert refused(deposit(), DEPOSIT, "ctx is NULL")
    assert refused(deposit(cnt=None), "ctx is NULL")
    assert refused(deposit(n=0, cnt=None, occ=None, light=None, thr=None, pix=None, rad=None), "ctx is NULL")
    for kw, word in (({"occ": None}, "d_occluded"), ({"light": None}, "d_light"), ({"thr": None}, "d_throughput"), ({"pix": None}, "d_pixel"), ({"rad": None}, "d_radiance")):
        assert refused(deposit(**kw), word, "NULL"), kw
    for kw, word, size in (({"cnt": K + 1}, "d_count", "4-byte"), ({"occ": E + 2}, "d_occluded", "4-byte"), ({"light": F + 4}, "d_light", "16-byte"),
                           ({"thr": A + 8}, "d_throughput", "16-byte"), ({"pix": B + 3}, "d_pixel", "4-byte"), ({"rad": D + 4}, "d_radiance", "16-byte")):
        assert refused(deposit(**kw), word, size), kw
    assert refused(deposit(occ=E + 4, pix=B + 12), "ctx is NULL")
    assert refused(deposit(n=2 ** 31), DEPOSIT, "n must be below 2^31")
    assert refused(deposit(npix=2 ** 31), "npixels", "2^31")

    # ---- fold
    def fold(npix=100, sample=A, accum=D, frame=0, clear=0):
        return lib.mrt_context_fold_sample_device(None, npix, sample, accum, frame, clear, None)

    assert refused(fold(), FOLD, "ctx is NULL")
    assert refused(fold(frame=2 ** 32 - 2, clear=1), "ctx is NULL")
    assert refused(fold(npix=0, sample=None, accum=None), "ctx is NULL")
    assert refused(fold(frame=2 ** 32 - 1), "frame_index")
    assert refused(fold(accum=A), "d_sample", "d_accum")
    assert refused(fold(sample=None), "d_sample", "NULL")
    assert refused(fold(accum=None), "d_accum", "NULL")
    assert refused(fold(sample=A + 8), "d_sample", "16-byte")
    assert refused(fold(accum=D + 4), "d_accum", "16-byte")
    assert refused(fold(npix=2 ** 31), "npixels", "2^31")


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_path_kernels_use_no_scratch_and_no_lds(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed); the figures are the ones the compiler writes into the code object's metadata.  These kernels are nothing but
    traffic: a spill would add traffic of its own, and they share nothing between threads."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "paths.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "paths.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "paths.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)), int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
                         int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1)))
    # reset, advance x {diffuse, materials} x {one mask, two}, deposit, fold x {keep, clear}
    assert len(kernels) == 8 and sum("k_paths_advance" in k for k in kernels) == 4 and sum("k_paths_fold" in k for k in kernels) == 2, sorted(kernels)
    assert any("k_paths_reset" in k for k in kernels) and any("k_paths_deposit" in k for k in kernels)
    for name, (scratch, lds, threads) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert threads == 256, f"{name}: {threads} threads per workgroup"
    # no traversal, shading or builder code is compiled in this translation unit
    src = open(os.path.join(CSRC, "paths.hip")).read()
    assert re.findall(r'#include "(\w+\.h)"', src) == ["paths.h"]
    assert re.findall(r'#include "(\w+\.h)"', open(os.path.join(CSRC, "paths.h")).read()) == ["scene_device.h"]


# ---------------------------------------------------------------- the reference against the oracle's image: a frame composed on queues, on the CPU
def _same(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint32).reshape(a.shape[0], -1) != b.view(np.uint32).reshape(b.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {a.shape[0]} rows differ; first at {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


CPU_CASES = [(name, False) for name in R.CASES] + [(M.CORNELL, True)]


def _oracle_frames(orc, c, materials, frames):
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=M.MAX_BOUNCES if materials else 3, camera=c["scene"].camera)
    if materials: orr.set_materials(True)
    out = []
    for _ in range(frames):
        orr.render(1)
        out.append(orr.accumulation().reshape(-1, 4).copy())
    orr.close()
    return out


@pytest.mark.parametrize("name,materials", CPU_CASES)
def test_a_frame_composed_on_queues_equals_the_oracles_image(mrt, orc, name, materials):
    """reset -> per bounce: closest, resolve, scatter, advance, the two compactions, any, deposit -> fold: the oracle's accumulation at frame 0 and after three frames,
    every bit of it, the fourth component included.  The queues are no pretence: paths end after bounce 0, and the materials scene emits and holds every lobe that goes on."""
    c = (M if materials else R).scene_case(mrt, orc, name)
    bounces = M.MAX_BOUNCES if materials else 3
    n = c["w"] * c["h"]
    want = _oracle_frames(orc, c, materials, 3)
    accum = np.full((n, 4), np.nan, np.float32)                                                     # frame 0 reads no accumulation
    samples = []
    for f in range(3):
        info = {}
        sample = PS.composed_frame(orc, c, f, bounces, materials=materials, info=info)
        assert not sample[:, 3].any()                                                               # only .rgb is ever changed
        if f == 0:
            counts = info["counts"]
            assert len(counts) == bounces - 1 and 0 < counts[-1] < n and all(a >= b for a, b in zip([n] + counts, counts)), counts
            if name in ("cornell", "two_level", M.CORNELL): assert counts[0] < n, counts               # the scenes of the GPU test (elsewhere every primary ray hits)
            if materials: assert info["emitted"] and {1, 2, 3, 4} <= info["lobes"], info
        cleared, accum = PS.fold_sample(sample, accum, f, clear_sample=True)
        assert not cleared.view(np.uint32).any()
        samples.append(sample[:, 0:3])
        if f == 0:
            _same(accum, want[0], f"{name}: frame 0")
            assert accum[:, 0:3].any()
    _same(accum, want[2], f"{name}: three frames folded")
    _same(accum[:, 0:3], R.running_average(samples), f"{name}: the fold is the reference's own")


def test_the_reference_leaves_tails_and_unnamed_pixels_alone():
    """the contract of the count word and of the pixel word, on the reference itself: small rows written by hand"""
    rng = np.random.default_rng(2)
    n, npix = 9, 12
    thr = rng.random((n, 4)).astype(np.float32); light = rng.random((n, 4)).astype(np.float32); light[::2, 3] = 1.0
    lobes = np.zeros(n, M.LOBE_DTYPE)
    lobes["weight"] = rng.random((n, 3)); lobes["emission"] = rng.random((n, 3)); lobes["lobe"] = [0, 1, 2, 3, 4, 5, 1, 2 ** 30, 1]
    pix = np.array([3, 0, 11, 12, 7, -1, 5, 2 ** 30, 1], np.int32)                                    # 12 = npixels and -1 = 0xFFFFFFFF lie outside
    rad = rng.random((npix, 4)).astype(np.float32)
    a = PS.advance_paths(thr, light, lobes=lobes, pixel=pix, radiance=rad, count=7, keep_shadow=np.full(n, 9, np.uint8), keep_path=np.full(n, 9, np.uint8))
    assert a["keep_path"].tolist() == [0, 1, 1, 1, 1, 0, 1, 9, 9] and a["keep_shadow"].tolist() == [1, 0, 1, 0, 1, 0, 1, 9, 9]
    assert np.array_equal(a["throughput"][7:], thr[7:]) and np.array_equal(a["throughput"][:7, 3], thr[:7, 3])
    touched = [0, 11, 7, 5]                                                                           # rows 1, 2, 4, 6; row 0 is no surface, rows 3 and 5 name no pixel
    assert np.array_equal(np.flatnonzero((a["radiance"] != rad).any(1)), sorted(touched)) and np.array_equal(a["radiance"][:, 3], rad[:, 3])
    assert a["radiance"][11, 0] == np.float32(rad[11, 0] + np.float32(thr[2, 0] * lobes["emission"][2, 0]))
    occ = np.array([0, 1, 0, 0, 0, 0, 1, 0, 0], np.int32)
    d = PS.deposit_light(occ, light, thr, pix, rad, count=-1)                                         # -1 is 2^32 - 1: clamped to n
    assert np.array_equal(np.flatnonzero((d != rad).any(1)), [1, 3, 7, 11])                           # rows 8, 0, 4, 2
    assert PS.rows_in_use(9, None) == 9 and PS.rows_in_use(9, 14) == 9 and PS.rows_in_use(9, -1) == 9 and PS.rows_in_use(9, 0) == 0
