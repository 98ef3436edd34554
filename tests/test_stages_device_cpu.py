"""The stage entries (mrt_renderer_primary_rays_device / mrt_scene_scatter_device) as far as they can be checked without a GPU: the yardstick of the GPU
tests (tests/stages_reference.py) pinned bit for bit to the oracle's stage dumps — every record, at two frame indices — and to the oracle's image through a frame composed
from the stages, the ABI and its ctypes mirror, the refusals that need no device, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stages_reference as R
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
ENTRIES = ("mrt_renderer_primary_rays_device", "mrt_scene_scatter_device")


def _same(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint32).reshape(a.shape[0], -1) != b.view(np.uint32).reshape(b.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {a.shape[0]} rows differ; first at {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


# ---------------------------------------------------------------- the reference against the oracle's stage dump
@pytest.mark.parametrize("frame", [0, 5])
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_equals_the_oracles_stage_dump(mrt, orc, name, frame):
    """Every record the dump holds, none left out: the generated primary rays are bounce 0's org and dir; at every bounce the light's colour, whether a shadow ray was wanted,
    the light picked, the shadow ray's occlusion and — below the last bounce — the next ray are the dump's."""
    c = R.scene_case(mrt, orc, name)
    d = R.dump_case(mrt, orc, name, frame)
    n = c["w"] * c["h"]
    rays, hidx = R.primary_rays(orc, c["scene"].camera, c["w"], c["h"], S.SEED, frame)
    assert d["pixels"][0].size == n                                                   # bounce 0 holds every pixel
    _same(rays[:, 0:3], d["dump"][:, 0, 0:3], "primary origins"); _same(rays[:, 4:7], d["dump"][:, 0, 3:6], "primary directions")
    assert not rays[:, 3].any() and np.isposinf(rays[:, 7]).all()
    assert np.array_equal(hidx, [np.int32((orc.seed_hash(S.SEED, p) + frame) & 0x7FFFFFFF) for p in range(n)])
    picked = set()
    for b in range(3):
        pix, surf = d["pixels"][b], d["surfaces"][b]
        rec = d["dump"][pix, b, :]
        hit = rec[:, 7].view(np.uint32) != 0xFFFFFFFF
        assert hit.any(), f"bounce {b} holds no hit"
        assert np.array_equal(surf["type"] == 1, hit)
        st = R.scatter(orc, surf, hidx[pix], b, c["scene"].lights)
        _same(st["light"][hit, 0:3], rec[hit, 11:14], f"bounce {b}: the light's colour")
        wants = st["light"][:, 3] == np.float32(1.0)
        assert np.array_equal(wants[hit], rec[hit, 14] != -1.0) and set(np.unique(st["light"][:, 3])) <= {0.0, 1.0}, f"bounce {b}: wanted"
        assert np.array_equal(st["light_index"][hit], rec[hit, 15].astype(np.int32)), f"bounce {b}: the light picked"
        picked |= set(st["light_index"][hit].tolist())
        assert wants.any()
        occ = c["osc"].intersect_any(st["shadow_rays"][wants])
        assert np.array_equal(occ, rec[wants, 14].astype(np.int32)), f"bounce {b}: occlusion of the shadow rays"
        # rows that are no surface, and shadow rays nobody wants, are zero bytes
        for k in ("shadow_rays", "light", "next_rays"): assert not st[k][~hit].view(np.uint32).any(), k
        assert not st["shadow_rays"][~wants].view(np.uint32).any() and (st["light_index"][~hit] == -1).all()
        assert not st["shadow_rays"][wants, 3].any() and np.isposinf(st["next_rays"][hit, 7]).all() and not st["next_rays"][hit, 3].any()
        if b < 2:
            nxt = d["dump"][pix, b + 1, :]
            assert (nxt[hit, 3:6] != 0).any(-1).all()                                 # a path goes on where it hit ...
            if frame == 0: assert not nxt[~hit].any()                                 # ... and nowhere else (a later frame's dump still holds earlier frames' records there)
            assert np.array_equal(d["pixels"][b + 1], pix[hit])
            _same(st["next_rays"][hit, 0:3], nxt[hit, 0:3], f"bounce {b}: next origins"); _same(st["next_rays"][hit, 4:7], nxt[hit, 3:6], f"bounce {b}: next directions")
    if name == R.FOUR_LIGHTS:
        lights = c["scene"].lights
        assert sorted(l.type for l in lights) == [1, 2, 3, 4] and picked == {0, 1, 2, 3}, picked


def test_light_count_limits_the_pick(mrt, orc):
    c = R.scene_case(mrt, orc, R.FOUR_LIGHTS)
    d = R.dump_case(mrt, orc, R.FOUR_LIGHTS, 0)
    surf, hidx = d["surfaces"][0], R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)
    one = R.scatter(orc, surf, hidx, 0, c["scene"].lights, light_count=1)
    allof = R.scatter(orc, surf, hidx, 0, c["scene"].lights)
    hit = surf["type"] == 1
    assert (one["light_index"][hit] == 0).all() and len(set(allof["light_index"][hit].tolist())) == 4
    _same(R.scatter(orc, surf, hidx, 0, c["scene"].lights, light_count=4)["light"], allof["light"], "light_count = all")
    _same(one["next_rays"], allof["next_rays"], "the bounce ray does not depend on the light")


# ---------------------------------------------------------------- a frame composed on the CPU
@pytest.mark.parametrize("name", list(R.CASES))
def test_a_composed_frame_equals_the_oracles_image(mrt, orc, name):
    """generate -> closest -> resolve -> scatter -> any, three bounces, throughput and radiance as separate numpy products and sums: the oracle's accumulation at frame 0"""
    c = R.scene_case(mrt, orc, name)
    d = R.dump_case(mrt, orc, name, 0)
    acc = R.composed_frame(orc, c, 0)
    img = np.concatenate([acc, np.ones((acc.shape[0], 1), np.float32)], 1).reshape(c["h"], c["w"], 4)
    _same(img.reshape(-1, 4), d["accum"].reshape(-1, 4), f"{name}: the composed frame")
    assert acc.any()


def test_running_average_is_the_oracles(mrt, orc):
    c = R.scene_case(mrt, orc, "cornell")
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=3, camera=c["scene"].camera)
    orr.render(3)
    want = orr.accumulation(); orr.close()
    got = R.running_average([R.composed_frame(orc, c, f) for f in range(3)])
    _same(got, want.reshape(-1, 4)[:, 0:3], "three frames folded")


# ---------------------------------------------------------------- ABI and ffi
def test_header_declares_the_entries_and_the_version_is_still_3():
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", hdr, re.M)
    assert re.search(r"^int mrt_renderer_primary_rays_device\(MRTRenderer r, uint32_t sample_index,", hdr, re.M)
    assert re.search(r"^int mrt_scene_scatter_device\(MRTScene scene, const void \*d_surfaces", hdr, re.M)
    comment = hdr[hdr.index("int mrt_scene_vertex_offsets("):hdr.index("int mrt_renderer_primary_rays_device(")]
    assert "materials = 1" in comment and "unspecified" in comment          # the diffuse path only; what a query answers for a zero ray is no part of the contract


def test_ffi_holds_both_entries(mrt):
    from metal_raytracing_amd import _ffi
    for entry in ENTRIES:
        assert entry in _ffi.SIGNATURES and hasattr(mrt.lib, entry)
    assert len(_ffi.SIGNATURES["mrt_renderer_primary_rays_device"][1]) == 5 and len(_ffi.SIGNATURES["mrt_scene_scatter_device"][1]) == 10
    assert mrt.lib.mrt_abi_version() == 3
    assert callable(mrt.Renderer.primary_rays_device) and callable(mrt.DeviceScene.scatter_device)


def test_arguments_are_refused_before_any_gpu_work(mrt):
    """The plain arguments are checked first, so every refusal below is reached without a device, a scene or a renderer (the message names the argument); a NULL handle is
    refused last."""
    lib = mrt.lib
    P = C.c_void_p
    good = P(4096)                       # an aligned address that is never dereferenced: every call below returns before the handle is looked at

    def last():
        return lib.mrt_last_error().decode()

    def primary(rays=good, idx=good, si=0):
        return lib.mrt_renderer_primary_rays_device(None, si, rays, idx, None)

    assert primary() == INVALID and "renderer is NULL" in last()
    assert primary(rays=None) == INVALID and "NULL" in last() and "d_rays" in last()
    assert primary(idx=None) == INVALID and "NULL" in last() and "d_halton_index" in last()
    assert primary(rays=P(4104)) == INVALID and "d_rays" in last() and "16-byte" in last()
    assert primary(idx=P(4098)) == INVALID and "d_halton_index" in last() and "4-byte" in last()
    assert primary(idx=P(4100)) == INVALID and "renderer is NULL" in last()          # 4-byte alignment is enough for the index

    def scat(surf=good, idx=good, n=4, bounce=0, lc=0, sh=good, light=good, nxt=good):
        return lib.mrt_scene_scatter_device(None, surf, idx, n, bounce, lc, sh, light, nxt, None)

    assert scat() == INVALID and "scene is NULL" in last()
    assert scat(nxt=None) == INVALID and "scene is NULL" in last()                   # the bounce rays may be left out
    for kw, word in (({"surf": None}, "d_surfaces"), ({"idx": None}, "d_halton_index"), ({"sh": None}, "d_shadow_rays"), ({"light": None}, "d_light")):
        assert scat(**kw) == INVALID and "NULL" in last() and word in last(), kw
    for kw, word in (({"surf": P(4104)}, "d_surfaces"), ({"sh": P(4100)}, "d_shadow_rays"), ({"light": P(4097)}, "d_light"), ({"nxt": P(4112 + 8)}, "d_next_rays")):
        assert scat(**kw) == INVALID and "16-byte" in last() and word in last(), kw
    assert scat(idx=P(4097)) == INVALID and "4-byte" in last() and "d_halton_index" in last()
    assert scat(idx=P(4100)) == INVALID and "scene is NULL" in last()
    assert scat(n=2 ** 31) == INVALID and "2^31" in last()
    assert scat(bounce=-1) == INVALID and "bounce" in last()
    assert scat(bounce=19) == INVALID and "bounce" in last()                         # dimension 2 + 5 * 19 + 4 is past the prime table
    assert scat(lc=-1) == INVALID and "light_count" in last()
    assert scat(n=0, surf=None, idx=None, sh=None, light=None, nxt=None) == INVALID and "scene is NULL" in last()   # nothing to refuse but the handle


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_stage_kernels_use_no_scratch(tmp_path):
    """Both kernels are bound by their stores and the Halton recurrence: a spill would add traffic of its own.  Compiled as the Makefile compiles them (no GPU needed)."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "stages.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "stages.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "stages.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    seen = set()
    for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt):
        name, size = m.group(1), int(m.group(2))
        for k in ("k_primary_rays", "k_scatter"):
            if k in name:
                seen.add(name)
                assert size == 0, f"{name}: {size} bytes of scratch"
    assert len(seen) == 3, seen          # k_primary_rays, k_scatter<false>, k_scatter<true>
    for word in ("ds_read", "ds_write", "global_atomic", "ds_bpermute", "v_readlane"):          # no LDS, no atomics, no cross-lane traffic
        assert word not in txt, word
