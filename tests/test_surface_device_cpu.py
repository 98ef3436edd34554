"""The surface entries (mrt_scene_resolve_hits_device / mrt_scene_interpolate_device / mrt_scene_vertex_offsets) as far as they can be checked without
a GPU: the yardstick of the GPU tests (tests/surface_reference.py) pinned bit for bit to the oracle's stage dumps, the ABI and its ctypes mirror, the refusals that need no
device, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_reference as D
import surface_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1


# ---------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("name", list(S.CASES))
def test_reference_equals_the_oracles_stage_dump(mrt, orc, name):
    """Every bounce record the dump holds, with hits from OracleScene.intersect_closest on the dumped rays: the shading normal the oracle shaded with, o + d * t of the dumped
    floats and the colour table of guides_from_dump.  Records of bounce >= 1 are the incoherent case (all three scenes hold some: asserted)."""
    c = S.case(mrt, orc, name)
    dump, ref = c["dump"], c["ref"]
    assert len(c["rays"]) == 3 and all(r.shape[0] > 0 for r in c["rays"]), "the dump holds no record of a later bounce"
    table = np.zeros((len(c["scene"].meshes), ref.max_sub, 3), np.float32)
    for i, m in enumerate(c["scene"].meshes):
        for g, sm in enumerate(m.submeshes): table[i, g] = np.asarray(sm.material.baseColor.tolist()[:3], np.float32)
    for b in range(3):
        rec = dump[:, :, b, :].reshape(-1, 16)[c["pixels"][b]]
        rays, hits = c["rays"][b], c["hits"][b]
        hit = rec[:, 7].view(np.uint32) != 0xFFFFFFFF
        assert np.array_equal(hits["type"] == 1, hit) and hit.any()
        s = ref.resolve(rays, hits)
        assert np.array_equal(s["type"], hits["type"])
        assert S.same_bits(s["normal"][hit], rec[hit, 8:11]), f"bounce {b}: {(s['normal'][hit].view(np.uint32) != rec[hit, 8:11].view(np.uint32)).any(-1).sum()} normals differ"
        assert S.same_bits(s["distance"][hit], rec[hit, 6])
        assert S.same_bits(s["position"][hit], rec[hit, 0:3] + rec[hit, 3:6] * rec[hit, 6:7])
        assert S.same_bits(s["base_color"][hit], table[hits["instance_id"][hit], hits["geometry_id"][hit]])
        for f in ("instance_id", "geometry_id", "primitive_id"): assert np.array_equal(s[f], hits[f]), f
        assert np.array_equal(s["resource_slot"][hit], hits["instance_id"][hit] * ref.max_sub + hits["geometry_id"][hit])
        assert S.differing(s[~hit], np.broadcast_to(S.miss_record(), s[~hit].shape).copy()) == 0
    # bounce 0 is what guides_from_dump builds the guide buffers from: the same normals, distances and colours
    nd, al, _ = D.guides_from_dump(dump, _full(c, 0), c["scene"])
    s0 = ref.resolve(*_full_rays(c))
    hit = (s0["type"] == 1).reshape(c["h"], c["w"])
    assert S.same_bits(nd[hit][:, :3], s0["normal"].reshape(c["h"], c["w"], 3)[hit]) and S.same_bits(al[hit][:, :3], s0["base_color"].reshape(c["h"], c["w"], 3)[hit])


def _full(c, b):
    assert c["pixels"][b].size == c["w"] * c["h"]          # bounce 0 holds every pixel
    return c["hits"][b]


def _full_rays(c):
    return c["rays"][0], _full(c, 0)


def test_reference_interpolates_the_object_space_normal_and_refuses_bad_ids(mrt, orc):
    c = S.case(mrt, orc, "two_level")
    ref, hits = c["ref"], c["hits"][1]
    assert [int(o) for o in ref.offsets[[0, 1, 2, 5]]] == [0, int(ref.offsets[1]), int(ref.offsets[1]), int(ref.offsets[1])]          # the spheres share mesh 1's rows
    a = ref.interpolate(hits, ref.attribute("normals"))
    hit = hits["type"] == 1
    u, v = hits["u"][hit][:, None], hits["v"][hit][:, None]
    n = [np.stack([ref.entries[i]["normals"][ref.entries[i]["indices"][g][p][k]] for i, g, p in zip(hits["instance_id"][hit], hits["geometry_id"][hit], hits["primitive_id"][hit])]) for k in range(3)]
    assert S.same_bits(a[hit], (u * n[1] + v * n[2]) + ((np.float32(1) - u) - v) * n[0]) and not a[~hit].any()
    bad = np.array(hits[hit][:4])
    bad["instance_id"][0] = len(ref.entries); bad["geometry_id"][1] = -1; bad["primitive_id"][2] = 2 ** 31 - 1
    r = ref.resolve(np.zeros((4, 8), np.float32), bad)
    assert list(r["type"]) == [0, 0, 0, 1] and not ref.interpolate(bad, ref.attribute("normals"))[:3].any()


# ---------------------------------------------------------------- ABI and ffi
def test_header_declares_the_entries_and_the_version_is_still_3():
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", hdr, re.M)
    for entry in ("mrt_scene_resolve_hits_device", "mrt_scene_interpolate_device", "mrt_scene_vertex_offsets"):
        assert re.search(rf"^int {entry}\(MRTScene scene,", hdr, re.M), entry
    assert re.search(r"\}\s*MRTSurface;", hdr)


def test_ffi_mirrors_the_surface_record(mrt):
    from metal_raytracing_amd import _ffi
    T = _ffi.Surface
    assert C.sizeof(T) == 64
    assert [getattr(T, f).offset for f in ("position", "distance", "normal", "type", "base_color", "resource_slot", "instance_id", "_pad")] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert mrt.SURFACE_DTYPE.itemsize == 64 and [mrt.SURFACE_DTYPE.fields[f][1] for f in ("position", "distance", "normal", "type", "base_color", "resource_slot", "instance_id", "_pad")] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert mrt.SURFACE_DTYPE == S.SURFACE_DTYPE
    for entry in ("mrt_scene_resolve_hits_device", "mrt_scene_interpolate_device", "mrt_scene_vertex_offsets"):
        assert entry in _ffi.SIGNATURES and hasattr(mrt.lib, entry)
    assert mrt.lib.mrt_abi_version() == 3
    rec = np.zeros((2, 16), np.float32); rec[1, 3] = 2.5; rec.view(np.int32)[1, 12] = 7
    u = mrt.unpack_surfaces(rec)
    assert u.shape == (2,) and u["distance"][1] == 2.5 and u["instance_id"][1] == 7


def test_arguments_are_refused_before_any_gpu_work(mrt):
    """The plain arguments are checked first, so every refusal below is reached without a device or a scene (the message names the argument); a NULL scene is refused last."""
    lib = mrt.lib
    P = C.c_void_p
    good = P(4096)                       # an aligned address that is never dereferenced: every call below returns before the scene is looked at

    def last():
        return lib.mrt_last_error().decode()

    def interp(hits=good, attr=good, stride=12, ch=3, out=good, ostride=12, n=4):
        return lib.mrt_scene_interpolate_device(None, hits, n, attr, stride, ch, out, ostride, None)

    assert interp() == INVALID and "scene is NULL" in last()
    for ch in (0, 65, -1):
        assert interp(ch=ch, stride=4 * 65, ostride=4 * 65) == INVALID and "channels" in last(), ch
    assert interp(stride=8) == INVALID and "stride" in last()                      # below 4 * channels
    assert interp(ostride=8) == INVALID and "stride" in last()
    assert interp(stride=14) == INVALID and "multiples of 4" in last()
    assert interp(ostride=18) == INVALID and "multiples of 4" in last()
    assert interp(attr=P(4097)) == INVALID and "aligned" in last()                 # an odd pointer
    assert interp(out=P(4099)) == INVALID and "aligned" in last()
    assert interp(hits=P(4104)) == INVALID and "aligned" in last()                 # records are read 16 bytes at a time
    assert interp(attr=None) == INVALID and "NULL" in last()
    assert interp(n=2 ** 31) == INVALID and "2^31" in last()

    def resolve(rays=good, hits=good, out=good, n=4):
        return lib.mrt_scene_resolve_hits_device(None, rays, hits, n, out, None)

    assert resolve() == INVALID and "scene is NULL" in last()
    for kw in ({"rays": P(4097)}, {"hits": P(4100)}, {"out": P(4104)}):
        assert resolve(**kw) == INVALID and "aligned" in last(), kw
    assert resolve(out=None) == INVALID and "NULL" in last()
    assert resolve(n=2 ** 31) == INVALID and "2^31" in last()
    assert lib.mrt_scene_vertex_offsets(None, None, 1) == INVALID


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_surface_kernels_use_no_scratch(tmp_path):
    """Both kernels are bandwidth-bound gathers: a spill would add traffic of its own.  Compiled as the Makefile compiles them (no GPU needed)."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "surface.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "surface.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "surface.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    seen = set()
    for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt):
        name, size = m.group(1), int(m.group(2))
        for k in ("k_resolve_hits", "k_interpolate"):
            if k in name:
                seen.add(name)
                assert size == 0, f"{name}: {size} bytes of scratch"
    assert len(seen) == 3, seen          # k_resolve_hits, k_interpolate<false>, k_interpolate<true>
