"""The image stages on device buffers (mrt_context_fold_guides_device / mrt_context_denoise_device / mrt_context_tonemap_device / mrt_denoise_workspace_bytes; DESIGN.md
§10n) as far as they can be checked without a GPU: the header, the ctypes mirror and the C++ one, every refusal that needs no device — each reached with a NULL context,
which is refused last — the resources of the kernels of image.hip, and the yardstick of the GPU tests (tests/image_stages_reference.py) pinned to the guide buffers built
from the oracle's dumps and to the oracle's tonemap."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as D
import image_stages_reference as IS
import stages_reference as R
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
FOLD, BYTES, DENOISE, TONEMAP = ("mrt_context_fold_guides_device", "mrt_denoise_workspace_bytes", "mrt_context_denoise_device", "mrt_context_tonemap_device")
P, SZ, I32, U32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32
WANT = {FOLD: [P, SZ, "pointer", "pointer", "pointer", "pointer", U32, "pointer"],
        BYTES: [I32, I32, "pointer"],
        DENOISE: [P, I32, I32, "pointer", "pointer", "pointer", "pointer", SZ, "pointer", "pointer", "pointer"],
        TONEMAP: [P, I32, I32, "pointer", "pointer", "pointer"]}


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
    assert _declared(FOLD)[2] == ["ctx", "npixels", "d_surfaces", "d_normal_depth", "d_albedo", "d_ids", "frame_index", "hip_stream"]
    assert _declared(BYTES)[2] == ["width", "height", "bytes"]
    assert _declared(DENOISE)[2] == ["ctx", "width", "height", "d_image", "d_normal_depth", "d_albedo", "d_workspace", "workspace_bytes", "d_out", "params", "hip_stream"]
    assert _declared(TONEMAP)[2] == ["ctx", "width", "height", "d_image", "d_rgba8", "hip_stream"]


def test_ffi_matches_the_header(mrt):
    import inspect
    from metal_raytracing_amd import _ffi
    for name in WANT:
        res, args, _ = _declared(name)
        fres, fargs = _ffi.SIGNATURES[name]
        assert fres is C.c_int and len(fargs) == len(args), name
        for k, (have, want) in enumerate(zip(fargs, args)):
            if want == "pointer": assert have is P or issubclass(have, C._Pointer), (name, k, have)          # (a typed pointer where the argument is a struct or a word of the host's)
            else: assert have is want, (name, k, have, want)
        fn = getattr(mrt.lib, name)
        assert fn.restype is fres and list(fn.argtypes) == fargs
    assert _ffi.SIGNATURES[DENOISE][1][9] is _ffi.SIGNATURES["mrt_renderer_denoise"][1][1]                  # the renderer's parameter block
    assert mrt.lib.mrt_abi_version() == 3
    sig = lambda m: list(inspect.signature(getattr(mrt.DeviceScene, m)).parameters)
    assert sig("fold_guides_device") == ["self", "surfaces", "frame_index", "out", "stream"]
    assert sig("denoise_device") == ["self", "image", "normal_depth", "albedo", "size", "iterations", "sigma_color", "sigma_normal", "sigma_depth", "demodulate", "out", "workspace", "stream"]
    assert sig("tonemap_device") == ["self", "image", "size", "out", "stream"]
    assert sig("denoise_workspace_bytes") == ["size"]


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "use_image.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*fold)(MRTContext, size_t, const void *, void *, void *, void *, uint32_t, void *) = &mrt::Scene::foldGuidesDevice;\n"
                   "size_t (*bytes)(int, int) = &mrt::Scene::denoiseWorkspaceBytes;\n"
                   "void (*denoise)(MRTContext, int, int, const void *, const void *, const void *, void *, size_t, void *, const MRTDenoiseParams *, void *) = &mrt::Scene::denoiseDevice;\n"
                   "void (*tonemap)(MRTContext, int, int, const void *, void *, void *) = &mrt::Scene::tonemapDevice;\n"
                   "void use(MRTContext ctx, void *a, void *b, void *c, void *d, void *e, void *stream) {\n"
                   "    mrt::Scene::foldGuidesDevice(ctx, 64, a, b, c, d, 0, stream);\n"
                   "    mrt::Scene::denoiseDevice(ctx, 8, 8, a, b, c, d, mrt::Scene::denoiseWorkspaceBytes(8, 8), e, nullptr, stream);\n"
                   "    mrt::Scene::tonemapDevice(ctx, 8, 8, e, a, nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "image_stages_host.cpp")])


# ---------------------------------------------------------------- refusals that need no device
def test_arguments_are_refused_before_the_context(mrt):
    """One assertion per refusal rule.  Every pointer is a plausible address that is never dereferenced: each call returns before the context is looked at, and the call
    with nothing wrong is refused for its NULL context alone."""
    from metal_raytracing_amd._ffi import DenoiseParams
    lib = mrt.lib
    A, B, D_, E, F = 0x1000000, 0x2000000, 0x3000000, 0x4000000, 0x5000000          # 16-byte aligned, 16 MiB apart

    def refused(rc, *words):
        msg = lib.mrt_last_error().decode()
        return rc == INVALID and all(w in msg for w in words)

    # ---- fold
    def fold(npix=100, surf=A, nd=B, al=D_, ids=E, frame=0):
        return lib.mrt_context_fold_guides_device(None, npix, surf, nd, al, ids, frame, None)

    assert refused(fold(), FOLD, "ctx is NULL")
    assert refused(fold(frame=2 ** 32 - 2), "ctx is NULL")
    assert refused(fold(npix=2 ** 31 - 1), "ctx is NULL")
    assert refused(fold(npix=0, surf=None, nd=None, al=None, ids=None), "ctx is NULL")
    assert refused(fold(npix=2 ** 31), "npixels", "2^31")
    assert refused(fold(frame=2 ** 32 - 1), "frame_index")
    for kw, word in (({"surf": None}, "d_surfaces"), ({"nd": None}, "d_normal_depth"), ({"al": None}, "d_albedo"), ({"ids": None}, "d_ids")):
        assert refused(fold(**kw), word, "NULL"), kw
    for kw, word in (({"surf": A + 4}, "d_surfaces"), ({"nd": B + 8}, "d_normal_depth"), ({"al": D_ + 12}, "d_albedo"), ({"ids": E + 4}, "d_ids")):
        assert refused(fold(**kw), word, "16-byte"), kw
    for kw, a, b in (({"nd": A}, "d_surfaces", "d_normal_depth"), ({"al": A}, "d_surfaces", "d_albedo"), ({"ids": A}, "d_surfaces", "d_ids"),
                     ({"al": B}, "d_normal_depth", "d_albedo"), ({"ids": B}, "d_normal_depth", "d_ids"), ({"ids": D_}, "d_albedo", "d_ids")):
        assert refused(fold(**kw), a, b, "must not be"), kw

    # ---- the workspace
    n = C.c_size_t(7)
    assert lib.mrt_denoise_workspace_bytes(1, 1, C.byref(n)) == 0 and n.value == 32
    assert lib.mrt_denoise_workspace_bytes(64, 48, C.byref(n)) == 0 and n.value == 2 * 64 * 48 * 16
    assert lib.mrt_denoise_workspace_bytes(1920, 1080, C.byref(n)) == 0 and n.value == 2 * 1920 * 1080 * 16
    assert lib.mrt_denoise_workspace_bytes(2 ** 15, 2 ** 15 - 1, C.byref(n)) == 0 and n.value == 2 * 2 ** 15 * (2 ** 15 - 1) * 16          # past 2^32 bytes
    assert refused(lib.mrt_denoise_workspace_bytes(0, 4, C.byref(n)), BYTES, "width")
    assert refused(lib.mrt_denoise_workspace_bytes(4, -1, C.byref(n)), "height")
    assert refused(lib.mrt_denoise_workspace_bytes(2 ** 15, 2 ** 15, C.byref(n)), "2^30")
    assert refused(lib.mrt_denoise_workspace_bytes(4, 4, None), "bytes", "NULL")
    assert mrt.DeviceScene.denoise_workspace_bytes((37, 23)) == 2 * 37 * 23 * 16

    # ---- denoise: 64 x 48 images of 48 KiB, a workspace of 96 KiB
    w, h = 64, 48
    img, need = w * h * 16, 2 * w * h * 16

    def denoise(width=w, height=h, image=A, nd=B, al=D_, work=E, wbytes=need, out=F, params=None):
        return lib.mrt_context_denoise_device(None, width, height, image, nd, al, work, wbytes, out, params, None)

    def par(iterations=5, sc=4.0, sn=0.25, sd=0.25, demodulate=1):
        return C.byref(DenoiseParams(iterations, sc, sn, sd, demodulate))

    assert refused(denoise(), DENOISE, "ctx is NULL")                                                   # NULL = the defaults
    assert refused(denoise(params=par()), "ctx is NULL")
    assert refused(denoise(params=par(iterations=1, demodulate=0)), "ctx is NULL") and refused(denoise(params=par(iterations=8)), "ctx is NULL")
    assert refused(denoise(wbytes=need + 16), "ctx is NULL")
    assert refused(denoise(width=0), "width") and refused(denoise(width=-3), "width")
    assert refused(denoise(height=0), "height")
    assert refused(denoise(width=2 ** 15, height=2 ** 15), "2^30")
    assert refused(denoise(params=par(iterations=0)), "iterations must be in [1,8]") and refused(denoise(params=par(iterations=9)), "iterations must be in [1,8]")
    for bad in (dict(sc=0.0), dict(sn=-1.0), dict(sd=float("nan")), dict(sc=float("inf"))):
        assert refused(denoise(params=par(**bad)), "sigma_color, sigma_normal and sigma_depth must be finite and > 0"), bad
    assert refused(denoise(params=par(demodulate=2)), "demodulate must be 0 or 1")
    for kw, word in (({"image": None}, "d_image"), ({"nd": None}, "d_normal_depth"), ({"al": None}, "d_albedo"), ({"work": None}, "d_workspace"), ({"out": None}, "d_out")):
        assert refused(denoise(**kw), word, "NULL"), kw
    for kw, word in (({"image": A + 4}, "d_image"), ({"nd": B + 8}, "d_normal_depth"), ({"al": D_ + 4}, "d_albedo"), ({"work": E + 8}, "d_workspace"), ({"out": F + 12}, "d_out")):
        assert refused(denoise(**kw), word, "16-byte"), kw
    assert refused(denoise(wbytes=need - 1), "workspace_bytes") and refused(denoise(wbytes=0), "workspace_bytes")
    # byte ranges, not pointers: the last row of one buffer on the first of another
    assert refused(denoise(out=A), "d_out overlaps d_image") and refused(denoise(out=A + img - 16), "d_out overlaps d_image") and refused(denoise(out=A - img + 16), "d_out overlaps d_image")
    assert refused(denoise(out=A + img, nd=A + 2 * img), "ctx is NULL")                                 # back to back is apart
    assert refused(denoise(out=B + 16), "d_out overlaps d_normal_depth") and refused(denoise(out=D_ - 16), "d_out overlaps d_albedo")
    assert refused(denoise(work=A - need + 16), "d_workspace overlaps d_image") and refused(denoise(work=B + img - 16), "d_workspace overlaps d_normal_depth")
    assert refused(denoise(work=D_), "d_workspace overlaps d_albedo")
    assert refused(denoise(out=E + need - 16), "d_out overlaps d_workspace") and refused(denoise(out=E - img + 16), "d_out overlaps d_workspace")
    assert refused(denoise(out=E + need), "ctx is NULL")
    assert refused(denoise(nd=A, al=A), "ctx is NULL")                                                  # inputs may share: nothing writes them

    # ---- tonemap
    def tonemap(width=w, height=h, image=A, rgba=B):
        return lib.mrt_context_tonemap_device(None, width, height, image, rgba, None)

    assert refused(tonemap(), TONEMAP, "ctx is NULL")
    assert refused(tonemap(rgba=B + 4), "ctx is NULL")                                                  # 4-byte alignment is enough for RGBA8
    assert refused(tonemap(width=0), "width") and refused(tonemap(height=-1), "height") and refused(tonemap(width=2 ** 16, height=2 ** 14), "2^30")
    assert refused(tonemap(image=None), "d_image", "NULL") and refused(tonemap(rgba=None), "d_rgba8", "NULL")
    assert refused(tonemap(image=A + 8), "d_image", "16-byte") and refused(tonemap(rgba=B + 2), "d_rgba8", "4-byte")
    assert refused(tonemap(rgba=A), "d_rgba8 overlaps d_image") and refused(tonemap(rgba=A + img - 4), "d_rgba8 overlaps d_image") and refused(tonemap(rgba=A - w * h * 4 + 4), "d_rgba8 overlaps d_image")
    assert refused(tonemap(rgba=A + img), "ctx is NULL") and refused(tonemap(rgba=A - w * h * 4), "ctx is NULL")


# ---------------------------------------------------------------- kernel resources
def _kernel_bodies(txt):
    """{symbol: its instructions} of an assembly listing"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_image_kernels_use_no_scratch_and_no_lds(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed); the figures are the ones the compiler writes into the code object's metadata.  These kernels are nothing but
    traffic — and the traffic is the contract's: at most four loads of the surface row, two 16-byte loads of the old averages except in the form for frame 0, three 16-byte
    stores; one load of the pixel and one dword store per pixel of the tonemap."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "image.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "image.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "image.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)), int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)),
                         int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block).group(1)))
    # fold x {frame 0, later frames}, tonemap: the filter's kernels stay in denoise.hip
    assert len(kernels) == 3 and sum("k_fold_guides" in k for k in kernels) == 2 and sum("k_tonemap_image" in k for k in kernels) == 1, sorted(kernels)
    for name, (scratch, lds, threads) in kernels.items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert lds == 0, f"{name}: {lds} bytes of LDS"
        assert threads == 256, f"{name}: {threads} threads per workgroup"
    bodies = _kernel_bodies(txt)
    assert set(bodies) == set(kernels), (sorted(bodies), sorted(kernels))
    count = lambda body, op: len(re.findall(r"^\s*" + op + r"\b", body, re.M))
    fold_loads = {}
    for name, body in bodies.items():
        loads16, stores16 = count(body, "global_load_dwordx4"), count(body, "global_store_dwordx4")
        other_loads = len(re.findall(r"^\s*(?:global|flat|buffer|scratch)_load_\w+", body, re.M)) - loads16
        other_stores = len(re.findall(r"^\s*(?:global|flat|buffer|scratch)_store_\w+", body, re.M)) - stores16
        assert not re.search(r"^\s*(?:ds_|global_atomic|flat_atomic|buffer_atomic)", body, re.M), f"{name}: LDS or atomics"
        if "k_tonemap_image" in name:          # one load of the pixel (the compiler may leave out the alpha it does not use: dwordx3 of the same 16 bytes), one dword store
            assert loads16 + other_loads == 1 and loads16 + count(body, "global_load_dwordx3") == 1 and (stores16, other_stores, count(body, "global_store_dword")) == (0, 1, 1), (name, body)
        else:                                  # three 16-byte stores and nothing narrower
            assert (stores16, other_stores) == (3, 0), (name, stores16, other_stores)
            fold_loads["first" if "ILb1E" in name else "later"] = (loads16, other_loads)
    # The surface row takes at most four loads (the compiler leaves out the words the fold does not use — position, slot, pad — and may cut the other 44 bytes as it likes);
    # the form for later frames adds the two 16-byte loads of the old averages, and the form for frame 0 does not contain them.
    assert set(fold_loads) == {"first", "later"} and 1 <= sum(fold_loads["first"]) <= 4, fold_loads
    assert fold_loads["later"] == (fold_loads["first"][0] + 2, fold_loads["first"][1]), fold_loads
    # no traversal, shading or builder code is compiled in this translation unit: its own header and what declares denoise_enqueue
    src = open(os.path.join(CSRC, "image.hip")).read()
    assert re.findall(r'#include "(\w+\.h)"', src) == ["image.h", "renderer.h"]
    assert re.findall(r'#include "(\w+\.h)"', open(os.path.join(CSRC, "image.h")).read()) == ["scene_device.h"]
    assert re.search(r"\bdenoise_enqueue\(", src) and "__global__" not in src[src.index("int denoise_image_device"):]


# ---------------------------------------------------------------- the reference against the oracle
def _same(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, what
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint32).reshape(a.shape[0], -1) != b.view(np.uint32).reshape(b.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {a.shape[0]} rows differ; first at {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


@pytest.mark.parametrize("name", ["cornell", "two_level"])
def test_four_folded_frames_equal_the_oracles_guides(mrt, orc, name):
    """primary rays -> the oracle's closest hit -> the surface rows -> fold, four frames: the three buffers denoise_reference.oracle_guides builds from the oracle's dumps,
    every bit.  The averages start from NaNs: frame 0 reads none of them."""
    frames = 4
    c = R.scene_case(mrt, orc, name)
    w, h, osc = c["w"], c["h"], c["osc"]
    n = w * h
    orr = orc.OracleRenderer(osc, w, h, seed=S.SEED, max_bounces=3, camera=c["scene"].camera)
    want_nd, want_al, want_ids, _ = D.oracle_guides(orr, c["scene"], frames, osc.intersect_closest)
    orr.close()
    nd = np.full((n, 4), np.nan, np.float32); al = np.full((n, 4), np.nan, np.float32); ids = None
    hit_always = np.ones(n, bool); hit_ever = np.zeros(n, bool)
    for f in range(frames):
        rays, _ = R.primary_rays(orc, c["scene"].camera, w, h, S.SEED, f)
        surf = c["ref"].resolve(rays, osc.intersect_closest(rays))
        nd, al, ids = IS.fold_guides(surf, nd, al, f)
        hit_always &= surf["type"] == 1; hit_ever |= surf["type"] == 1
    _same(nd, want_nd.reshape(-1, 4), f"{name}: normal | depth"); _same(al, want_al.reshape(-1, 4), f"{name}: albedo | coverage"); _same(ids, want_ids.reshape(-1, 4), f"{name}: ids")
    # not vacuous: pixels that never hit, pixels that always hit, and coverage strictly between
    cov = al[:, 3]
    assert (~hit_ever).any() and hit_always.any() and ((cov > 0) & (cov < 1)).any(), ((~hit_ever).sum(), hit_always.sum(), ((cov > 0) & (cov < 1)).sum())
    assert (cov[~hit_ever] == 0).all() and (cov[hit_always] == 1).all() and not nd[~hit_ever].view(np.uint32).any()
    assert (ids[ids[:, 0] == 0] == IS.MISS_IDS).all() and (ids[ids[:, 0] == 1][:, 1:] >= 0).all()


def test_rows_that_are_no_surface_contribute_zeros_whatever_they_hold():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((6, 16)).astype(np.float32)
    kinds = rows[:, 7].view(np.int32)
    kinds[:] = [1, 0, 2, 1, 0, -1]
    rows[1, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]] = np.nan; rows[4, 3] = -1.0
    rows[:, 12:16].view(np.int32)[:] = [[3, 1, 7, 0], [5, 5, 5, 5], [2, 2, 2, 2], [-4, -1, -9, 0], [-1, -1, -1, 0], [1, 1, 1, 1]]
    nd, al, ids = IS.fold_guides(rows, None, None, 0)
    off = [1, 2, 4, 5]
    assert not nd[off].view(np.uint32).any() and not al[off].view(np.uint32).any() and (ids[off] == IS.MISS_IDS).all()
    assert np.array_equal(nd[0], rows[0, [4, 5, 6, 3]]) and np.array_equal(al[3], np.append(rows[3, 8:11], np.float32(1.0))) and ids[3].tolist() == [1, -4, -1, -9]
    nd2, al2, _ = IS.fold_guides(rows, nd, al, 2 ** 24 + 1)
    fi, den = np.float32(2 ** 24 + 1), np.float32(2 ** 24 + 2)
    assert nd2[0, 3] == np.float32(np.float32(rows[0, 3] + np.float32(nd[0, 3] * fi)) / den) and np.isfinite(nd2).all() and np.isfinite(al2).all()


def test_the_tonemap_is_the_oracles(mrt, orc):
    for k, size in enumerate(IS.TONEMAP_SIZES):
        img = IS.synthetic_image(size, k)
        c = img[..., 0:3]
        assert np.isfinite(img).all() and (size == (1, 1) or c.max() == np.float32(1e6))
        assert np.array_equal(IS.tonemap_rgba8(img, size), orc.tonemap_rgba8(img)), size
        assert np.array_equal(IS.tonemap_rgba8(img.reshape(-1, 4), size), orc.tonemap_rgba8(img)), size
    assert ((c > -1) & (c < 0)).any() and (c == 0).any()
    got = IS.tonemap_rgba8(img, size)
    assert set(np.unique(got[..., 0:3]).tolist()) == set(range(256)) and (got[..., 3] == 255).all()          # every 8-bit value occurs
    # a rendered image, and the flip: the top row of the picture is the buffer's last
    c = R.scene_case(mrt, orc, "cornell")
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=3, camera=c["scene"].camera)
    orr.render(2)
    acc = orr.accumulation(); orr.close()
    got = IS.tonemap_rgba8(acc, (c["w"], c["h"]))
    assert np.array_equal(got, orc.tonemap_rgba8(acc)) and got[..., 0:3].any()
    assert np.array_equal(got[0], IS.tonemap_rgba8(acc[-1:], (c["w"], 1))[0]) and not np.array_equal(got, got[::-1])
