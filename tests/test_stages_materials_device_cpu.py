"""The scatter stage with the materials extension on (mrt_scene_scatter_materials_device) as far as it can be checked without a GPU: the yardstick of the
GPU tests (tests/stages_materials_reference.py) pinned bit for bit to the oracle's stage dumps with materials on — every hit record of every bounce, at two frame indices —
and to the oracle's image through a frame composed from the stages; the ABI and its ctypes mirror, the refusals that need no device, and the kernel's resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stages_materials_reference as M
import stages_reference as R
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
ENTRY = "mrt_scene_scatter_materials_device"
FRAMES = (0, 5)
B = M.MAX_BOUNCES


def _same(a, b, what):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a.view(np.uint32).reshape(a.shape[0], -1) != b.view(np.uint32).reshape(b.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {a.shape[0]} rows differ; first at {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


def _stage(mrt, orc, name, frame, b):
    c = M.scene_case(mrt, orc, name)
    d = M.dump_case(mrt, orc, name, frame)
    hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], frame)[d["pixels"][b]]
    return M.scatter_materials(orc, c["table"], d["rays"][b], d["surfaces"][b], hidx, b, B, c["scene"].lights)


# ---------------------------------------------------------------- the reference against the oracle's stage dump, materials on
def test_size_is_the_edge_scenes():
    import test_materials
    assert M.CASES[M.EDGE][:2] == test_materials.EDGE_SIZE == M.CASES[M.EDGE_TWO_LEVEL][:2] and M.CASES[M.CORNELL][:2] == (48, 48) and B == 4


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("name", M.DEVICE_CASES)
def test_reference_equals_the_oracles_stage_dump(mrt, orc, name, frame):
    """Every hit record the dump holds for this frame, none left out: the lobe class, and on diffuse rows the light's colour, whether a shadow ray was wanted, the light
    picked and the shadow ray's occlusion, are the dump's; below the last bounce the continuation ray is the next record's org and dir.  At frame 0 the dump starts as
    zeros, so an absorbed path (lobe 5) and a miss are exactly the rows whose next record is all zero."""
    c = M.scene_case(mrt, orc, name)
    d = M.dump_case(mrt, orc, name, frame)
    n = c["w"] * c["h"]
    rays, hidx = R.primary_rays(orc, c["scene"].camera, c["w"], c["h"], S.SEED, frame)
    assert d["pixels"][0].size == n
    _same(rays[:, 0:3], d["dump"][:, 0, 0:3], "primary origins"); _same(rays[:, 4:7], d["dump"][:, 0, 3:6], "primary directions")
    for b in range(B):
        pix, surf = d["pixels"][b], d["surfaces"][b]
        rec = d["dump"][pix, b, :]
        hit = rec[:, 7].view(np.uint32) != 0xFFFFFFFF
        assert hit.any(), f"bounce {b} holds no hit"
        assert np.array_equal(surf["type"] == 1, hit)
        _same(surf["normal"][hit], rec[hit, 8:11], f"bounce {b}: the normal")
        st = _stage(mrt, orc, name, frame, b)
        lobe = st["lobes"]["lobe"]
        assert np.array_equal(lobe != 0, hit)
        assert np.array_equal((lobe == 2) | (lobe == 3), hit & (rec[:, 14] == -2.0)), f"bounce {b}: the dielectric interface"
        assert np.array_equal((lobe == 4) | (lobe == 5), hit & (rec[:, 14] == -3.0)), f"bounce {b}: the specular lobe"
        dif = lobe == 1
        assert np.array_equal(dif, hit & (rec[:, 14] >= -1.0))
        _same(st["light"][dif, 0:3], rec[dif, 11:14], f"bounce {b}: the light's colour")
        wants = st["light"][:, 3] == np.float32(1.0)
        assert not wants[~dif].any() and np.array_equal(wants[dif], rec[dif, 14] != -1.0) and set(np.unique(st["light"][:, 3])) <= {0.0, 1.0}, f"bounce {b}: wanted"
        assert np.array_equal(st["light_index"][dif], rec[dif, 15].astype(np.int32)) and (st["light_index"][~dif] == -1).all(), f"bounce {b}: the light picked"
        occ = c["osc"].intersect_any(st["shadow_rays"][wants])
        assert np.array_equal(occ, rec[wants, 14].astype(np.int32)), f"bounce {b}: occlusion of the shadow rays"
        # the lobes that make no next-event estimate, and rows that are no surface, hold zero bytes there
        for k in ("shadow_rays", "light"): assert not st[k][~dif].view(np.uint32).any(), k
        goes = (lobe >= 1) & (lobe <= 4)
        assert not st["next_rays"][~goes].view(np.uint32).any() and np.isposinf(st["next_rays"][goes, 7]).all() and not st["next_rays"][goes, 3].any()
        assert not st["lobes"][lobe == 0].view(np.uint32).any() and not st["lobes"]["weight"][lobe == 5].any() and not st["lobes"]["_pad"].any()
        assert (st["lobes"]["weight"][(lobe == 2) | (lobe == 3)] == 1.0).all()
        _same(st["lobes"]["emission"][hit], c["table"]["emission"][surf["resource_slot"][hit]], "emission")
        if b + 1 < B:
            nxt = d["dump"][pix, b + 1, :]
            assert np.array_equal(d["pixels"][b + 1], pix[goes])
            if frame == 0:          # the dump started as zeros: a path that ended left nothing behind, one that goes on left its ray — no row is left out
                assert np.array_equal(goes, (nxt[:, 3:6] != 0).any(-1)) and not nxt[~goes].any()
                assert np.array_equal(lobe == 5, hit & ~(nxt != 0).any(-1))
            # (a later frame's dump still holds earlier frames' records behind an absorbed path: there the rows the reference says continue are compared)
            _same(st["next_rays"][goes, 0:3], nxt[goes, 0:3], f"bounce {b}: next origins"); _same(st["next_rays"][goes, 4:7], nxt[goes, 3:6], f"bounce {b}: next directions")


def test_every_lobe_and_emission_occur_in_what_the_tests_compare(mrt, orc):
    """Not vacuous: over bounces 0 .. 3 of the frame indices used on the edge scene each lobe code 1 .. 5 occurs at least 3 times, and at least 3 rows emit."""
    for name in (M.EDGE, M.EDGE_TWO_LEVEL):
        counts = np.zeros(6, np.int64); emit = 0
        for frame in FRAMES:
            for b in range(B):
                st = _stage(mrt, orc, name, frame, b)
                counts += np.bincount(st["lobes"]["lobe"], minlength=6)
                emit += int(st["lobes"]["emission"].any(-1).sum())
        assert (counts[1:] >= 3).all() and emit >= 3, (name, counts, emit)
    # and frame 0 alone, what the composed frames and the GPU's stage comparison use, holds every lobe too
    counts = sum(np.bincount(_stage(mrt, orc, M.EDGE, 0, b)["lobes"]["lobe"], minlength=6) for b in range(B))
    assert (counts[1:] >= 3).all(), counts


# ---------------------------------------------------------------- a frame composed on the CPU
@pytest.mark.parametrize("name", M.DEVICE_CASES)
def test_a_composed_frame_equals_the_oracles_image(mrt, orc, name):
    """generate -> closest -> resolve -> scatter with materials -> any, four bounces; radiance += throughput * emission, throughput *= weight, radiance += light *
    throughput where lit, alive = lobe in 1 .. 4, as separate numpy products and sums: the oracle's accumulation with materials on at frame 0"""
    c = M.scene_case(mrt, orc, name)
    d = M.dump_case(mrt, orc, name, 0)
    acc = M.composed_frame(orc, c, 0)
    img = np.concatenate([acc, np.ones((acc.shape[0], 1), np.float32)], 1)
    _same(img, d["accum"].reshape(-1, 4), f"{name}: the composed frame")
    assert acc.any()


def test_three_composed_frames_fold_to_the_oracles(mrt, orc):
    c = M.scene_case(mrt, orc, M.EDGE)
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=B, camera=c["scene"].camera)
    orr.set_materials(True)
    orr.render(3)
    want = orr.accumulation(); orr.close()
    got = R.running_average([M.composed_frame(orc, c, f) for f in range(3)])
    _same(got, want.reshape(-1, 4)[:, 0:3], "three frames folded")


def test_plain_materials_are_the_diffuse_stage(mrt, orc):
    """cornell_with_materials(plain=True): no emission, no specular colour, dissolve 1 — every lobe is the diffuse one, the weight is the base colour and the three ray
    outputs are stages_reference.scatter's"""
    c = M.scene_case(mrt, orc, M.PLAIN)
    d = M.dump_case(mrt, orc, M.PLAIN, 0)
    for b in range(B):
        surf = d["surfaces"][b]
        hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)[d["pixels"][b]]
        st = M.scatter_materials(orc, c["table"], d["rays"][b], surf, hidx, b, B, c["scene"].lights)
        plain = R.scatter(orc, surf, hidx, b, c["scene"].lights)
        hit = surf["type"] == 1
        assert hit.any() and np.array_equal(st["lobes"]["lobe"], hit.astype(np.int32))
        _same(st["lobes"]["weight"], np.where(hit[:, None], surf["base_color"], np.float32(0.0)).astype(np.float32), f"bounce {b}: weight")
        assert not st["lobes"]["emission"].any()
        for k in ("shadow_rays", "light", "next_rays"): _same(st[k], plain[k], f"bounce {b}: {k}")


def test_reference_checks_the_slot_and_takes_the_rows_albedo(mrt, orc):
    c = M.scene_case(mrt, orc, M.EDGE)
    d = M.dump_case(mrt, orc, M.EDGE, 0)
    hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)
    surf = np.array(d["surfaces"][0])
    rows = np.flatnonzero(surf["type"] == 1)[:3]
    base = M.scatter_materials(orc, c["table"], d["rays"][0], surf, hidx, 0, B, c["scene"].lights)
    for k, bad in zip(rows, (-1, c["table"]["slots"], 2 ** 30)): surf["resource_slot"][k] = bad
    st = M.scatter_materials(orc, c["table"], d["rays"][0], surf, hidx, 0, B, c["scene"].lights)
    for key in ("shadow_rays", "light", "next_rays", "lobes"):
        assert not np.ascontiguousarray(st[key][rows]).view(np.uint32).any()
        keep = np.setdiff1d(np.arange(surf.shape[0]), rows)
        assert np.ascontiguousarray(st[key][keep]).tobytes() == np.ascontiguousarray(base[key][keep]).tobytes()
    surf = np.array(d["surfaces"][0])
    dif = np.flatnonzero(base["lobes"]["lobe"] == 1)[:1]
    surf["base_color"][dif] = [0.25, 0.5, 0.125]
    st = M.scatter_materials(orc, c["table"], d["rays"][0], surf, hidx, 0, B, c["scene"].lights)
    assert st["lobes"]["lobe"][dif] == 1 and np.array_equal(st["lobes"]["weight"][dif[0]], np.float32([0.25, 0.5, 0.125]))


# ---------------------------------------------------------------- ABI and ffi
def test_header_declares_the_entry_and_the_version_is_still_3():
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", hdr, re.M)
    assert re.search(r"^int mrt_scene_scatter_materials_device\(MRTScene scene, const void \*d_rays", hdr, re.M)
    assert re.search(r"\} MRTScatterLobe;", hdr)
    assert "MRT_AT(MRTScatterLobe, lobe, 12)" in open(os.path.join(CSRC, "abi_check.h")).read()
    assert "mrt_renderer_render alone" not in hdr          # the materials extension is no longer out of the stages' reach


def test_ffi_holds_the_entry(mrt):
    from metal_raytracing_amd import _ffi
    P, I32, SZ = C.c_void_p, C.c_int32, C.c_size_t
    assert _ffi.SIGNATURES[ENTRY] == (C.c_int, [P, P, P, P, SZ, I32, I32, I32, P, P, P, P, P]) and hasattr(mrt.lib, ENTRY)
    fn = getattr(mrt.lib, ENTRY)
    assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[ENTRY][1]
    assert mrt.lib.mrt_abi_version() == 3
    assert callable(mrt.DeviceScene.scatter_materials_device) and C.sizeof(mrt.ScatterLobe) == 32 and mrt.ScatterLobe.lobe.offset == 12 and mrt.ScatterLobe.emission.offset == 16
    rows = np.arange(16, dtype=np.float32).reshape(2, 8)
    u = mrt.unpack_lobes(rows)
    assert u.dtype == mrt.LOBE_DTYPE == M.LOBE_DTYPE and u.shape == (2,) and np.array_equal(u["weight"][1], [8, 9, 10]) and np.array_equal(u["emission"][0], [4, 5, 6])
    assert u["lobe"][0] == np.float32(3).view(np.int32)


def test_arguments_are_refused_before_any_gpu_work(mrt):
    """The plain arguments are checked first, so every refusal below is reached without a device or a scene (the message names the argument); a NULL handle is refused
    last."""
    lib = mrt.lib
    P = C.c_void_p
    good = P(4096)                       # an aligned address that is never dereferenced: every call below returns before the handle is looked at

    def last():
        return lib.mrt_last_error().decode()

    def scat(rays=good, surf=good, idx=good, n=4, bounce=0, mb=4, lc=0, sh=good, light=good, nxt=good, lobes=good):
        return lib.mrt_scene_scatter_materials_device(None, rays, surf, idx, n, bounce, mb, lc, sh, light, nxt, lobes, None)

    assert scat() == INVALID and "scene is NULL" in last()
    assert scat(nxt=None) == INVALID and "scene is NULL" in last()                   # the continuation rays may be left out
    for kw, word in (({"rays": None}, "d_rays"), ({"surf": None}, "d_surfaces"), ({"idx": None}, "d_halton_index"), ({"sh": None}, "d_shadow_rays"), ({"light": None}, "d_light"),
                     ({"lobes": None}, "d_lobes")):
        assert scat(**kw) == INVALID and "NULL" in last() and word in last(), kw
    for kw, word in (({"rays": P(4100)}, "d_rays"), ({"surf": P(4104)}, "d_surfaces"), ({"sh": P(4100)}, "d_shadow_rays"), ({"light": P(4097)}, "d_light"), ({"nxt": P(4112 + 8)}, "d_next_rays"),
                     ({"lobes": P(4096 + 4)}, "d_lobes")):
        assert scat(**kw) == INVALID and "16-byte" in last() and word in last(), kw
    assert scat(idx=P(4097)) == INVALID and "4-byte" in last() and "d_halton_index" in last()
    assert scat(idx=P(4100)) == INVALID and "scene is NULL" in last()               # 4-byte alignment is enough for the index
    assert scat(n=2 ** 31) == INVALID and "2^31" in last()
    assert scat(mb=0) == INVALID and "max_bounces" in last() and scat(mb=17) == INVALID and "max_bounces" in last()
    assert scat(mb=16, bounce=15) == INVALID and "scene is NULL" in last()          # dimension 2 + 5 * 16 + 15 = 97 is inside the prime table
    assert scat(bounce=-1) == INVALID and "bounce must be" in last()
    assert scat(bounce=4) == INVALID and "bounce must be" in last() and scat(mb=1, bounce=1) == INVALID and "bounce must be" in last()
    assert scat(lc=-1) == INVALID and "light_count" in last()
    assert scat(n=0, rays=None, surf=None, idx=None, sh=None, light=None, nxt=None, lobes=None) == INVALID and "scene is NULL" in last()   # nothing to refuse but the handle


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_kernel_uses_no_scratch(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed): both instantiations of k_scatter_materials hold their state in registers, and the file has no LDS, no atomics
    and no cross-lane traffic."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "stages_materials.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "stages_materials.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "stages_materials.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    seen = set()
    for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt):
        name, size = m.group(1), int(m.group(2))
        if "k_scatter_materials" in name:
            seen.add(name)
            assert size == 0, f"{name}: {size} bytes of scratch"
    assert len(seen) == 2, seen          # k_scatter_materials<false>, k_scatter_materials<true>
    for word in ("ds_read", "ds_write", "global_atomic", "ds_bpermute", "v_readlane"):
        assert word not in txt, word
