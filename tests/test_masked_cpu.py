"""Visibility masks (mrt_scene_set_mesh_masks, mrt_scene_intersect_*_masked_device) as far as they can be checked without a GPU: the yardstick of the
GPU tests (tests/masked_reference.py) against MultihitReference and the oracle's brute-force closest hit on the visible meshes alone, known answers that follow from the
definition, the ABI and its mirrors, the refusals that need no device, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import masked_reference as R
import multihit_reference as M
from test_gpu_parity import _rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
f32 = np.float32
QUERIES = ("mrt_scene_intersect_closest_masked_device", "mrt_scene_intersect_any_masked_device", "mrt_scene_intersect_all_masked_device")
ENTRIES = ("mrt_scene_set_mesh_masks", "mrt_scene_get_mesh_masks") + QUERIES
INTERIOR, DIAGONAL = (0.75, 0.25), (0.5, 0.5)


def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([[o[0], o[1], o[2], tmin, d[0], d[1], d[2], tmax]], f32)


def _model_rays(sc, n, seed):
    lo = np.min([(m.transform.T @ np.c_[m.positions, np.ones(len(m.positions))].T).T[:, :3].min(0) for m in sc.meshes[:-1]], axis=0)
    hi = np.max([(m.transform.T @ np.c_[m.positions, np.ones(len(m.positions))].T).T[:, :3].max(0) for m in sc.meshes[:-1]], axis=0)
    rays = _rays(np.random.default_rng(seed), n, lo, hi)
    k = np.arange(n)
    rays[k % 4 == 1, 3] = 0.5
    rays[k % 8 == 3, 7] = 4.0
    return rays


# ---------------------------------------------------------------- the reference
def test_all_ones_is_the_multihit_reference(mrt):
    sc = R.three_models(mrt)
    entries = mrt.flatten_scene(sc)
    ref = R.MaskedReference(entries)
    assert ref._subset(ref.visible(R.ALL)) is ref.full and ref._subset(ref.visible(1)) is ref.full          # every mesh has every bit: nothing is filtered
    rays = _model_rays(sc, 120, 3)
    want = M.MultihitReference(entries).intersect_all(rays, 4)
    for masks in (R.ALL, 1, np.full(len(rays), 0x80000000, np.int64)):
        got = ref.intersect_all(rays, 4, masks)
        assert M.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("visible", [(0,), (1, 3), (0, 2), (3,), (0, 1, 2), (1, 2, 3)])
def test_one_hit_equals_the_oracles_brute_force_on_the_visible_meshes(mrt, orc, visible):
    """K = 1 against OracleScene.intersect_closest(brute=True) of a scene BUILT FROM the visible meshes alone, its instance ids mapped back to the full scene's: every
    field, distances and barycentrics as bit patterns.  Mesh k carries the bit 1 << k; the ray mask is the union of the visible meshes' bits."""
    sc = R.three_models(mrt)
    entries = mrt.flatten_scene(sc)
    assert len(entries) == 4
    ref = R.MaskedReference(entries, R.quad_stack_masks(4))
    rays = _model_rays(sc, 700, 17)
    osc = orc.OracleScene([entries[k] for k in visible], sc.lights)
    try:
        o = osc.intersect_closest(rays, brute=True)
    finally:
        osc.close()
    back = np.array(visible, np.int32)
    o["instance_id"] = np.where(o["type"] == 1, back[np.clip(o["instance_id"], 0, None)], -1)
    h = ref.intersect_closest(rays, sum(1 << k for k in visible))
    assert 0.1 < (o["type"] == 1).mean()
    assert set(np.unique(h["instance_id"][h["type"] == 1])) <= set(visible)
    for f in ("type", "instance_id", "geometry_id", "primitive_id", "_pad"):
        assert np.array_equal(h[f], o[f]), f
    for f in ("distance", "u", "v"):
        bad = np.flatnonzero(h[f].view(np.uint32) != o[f].view(np.uint32))
        assert bad.size == 0, (f, bad.size, h[bad[0]], o[bad[0]])


# ---------------------------------------------------------------- known answers from the definition alone
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("L", [1, 3, 17])
def test_quad_stack_lists_exactly_the_visible_quads_in_order(mrt, L, K):
    ref = R.MaskedReference(mrt.flatten_scene(M.quad_stack(mrt, L)), R.quad_stack_masks(L))
    r = _ray((*INTERIOR, 0.0), (0, 0, 1))
    full = (1 << L) - 1
    for m in sorted({0, 1, 1 << (L - 1), full, full & 0x15555, full & 0x0AAAA, full & ~1, 0x6 & full, R.ALL}):
        want = [k for k in range(L) if m >> k & 1][:K]
        h, c = ref.intersect_all(r, K, m)
        assert c[0] == len(want), (L, K, hex(m))
        assert list(h[0, :c[0]]["instance_id"]) == want and list(h[0, :c[0]]["distance"]) == [float(k + 1) for k in want]
        assert M.differing(h[0, c[0]:], np.broadcast_to(M.miss_record(), (K - c[0],)).copy()) == 0
        assert ref.intersect_any(r, m)[0] == (1 if want else 0)
        if want: assert ref.intersect_closest(r, m)[0]["instance_id"] == want[0]
    h, c = ref.intersect_all(np.repeat(r, 3, 0), K, np.array([0, 1 << (L - 1), 1]))          # a mask per ray
    assert list(c) == [0, 1, 1] and h[1, 0]["instance_id"] == L - 1 and h[2, 0]["instance_id"] == 0 and h[0, 0]["type"] == 0


def test_mask_zero_misses(mrt):
    ref = R.MaskedReference(mrt.flatten_scene(M.quad_stack(mrt, 3)))          # default masks: all ones, and still nothing is seen
    h, c = ref.intersect_all(_ray((*INTERIOR, 0.0), (0, 0, 1)), 4, 0)
    assert c[0] == 0 and M.differing(h[0], np.broadcast_to(M.miss_record(), (4,)).copy()) == 0


def test_coincident_quads_report_the_higher_id_when_the_lower_is_invisible(mrt):
    """three coincident quads in meshes 0, 1, 2 with the masks 2, 1, 4 over a fourth quad (mask 1): the tie at distance 1 goes to the lowest id among the VISIBLE"""
    p1, i1 = M.quad(1.0); p2, i2 = M.quad(2.0)
    entries = mrt.flatten_scene(M.raw_scene(mrt, [(p1, i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p2, i2, M._plain(mrt))]))
    ref = R.MaskedReference(entries, [2, 1, 4, 1])
    for xy, prims in ((INTERIOR, [0]), (DIAGONAL, [0, 1])):
        r = _ray((*xy, 0.0), (0, 0, 1))
        for m, first in ((1, 1), (2, 0), (3, 0), (4, 2), (5, 1), (6, 0), (7, 0)):
            h = ref.intersect_closest(r, m)[0]
            assert (h["instance_id"], h["distance"], h["primitive_id"]) == (first, 1.0, 0), m
        h, c = ref.intersect_all(r, 8, 5)
        assert list(h[0, :c[0]]["instance_id"]) == [1] * len(prims) + [2] * len(prims) + [3] * len(prims) and list(h[0, :c[0]]["primitive_id"]) == prims * 3
        assert list(h[0, :c[0]]["distance"]) == [1.0] * (2 * len(prims)) + [2.0] * len(prims)


# ---------------------------------------------------------------- ABI and mirrors
def test_header_declares_the_entries_and_constants_and_the_version_is_still_3():
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", hdr, re.M)
    for name, value in (("GEOMETRY_MASK_TRIANGLE", 1), ("GEOMETRY_MASK_LIGHT", 2), ("RAY_MASK_PRIMARY", 3), ("RAY_MASK_SHADOW", 1), ("RAY_MASK_SECONDARY", 1)):
        assert re.search(rf"^#define MRT_{name} {value}u?\b", hdr, re.M), name
    assert re.search(r"^int mrt_scene_set_mesh_masks\(MRTScene scene, int32_t first_mesh_id, int32_t count, const uint32_t \*masks\);", hdr, re.M)
    assert re.search(r"^int mrt_scene_get_mesh_masks\(MRTScene scene, int32_t first_mesh_id, int32_t count, uint32_t \*masks\);", hdr, re.M)
    for q in QUERIES:
        assert re.search(rf"^int {q}\(MRTScene scene, const void \*d_rays, const void \*d_ray_masks, uint32_t ray_mask, size_t n,", hdr, re.M), q
    for cite in ("ShaderTypes.h:23-30", "Renderer.swift:196", "Raytracing.metal:243,363-365"):
        assert cite in hdr, cite


def test_library_exports_and_ffi_carries_the_entries(mrt):
    from metal_raytracing_amd import _ffi
    P, SZ, I32, U32 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32
    assert _ffi.SIGNATURES[ENTRIES[0]] == _ffi.SIGNATURES[ENTRIES[1]] == (C.c_int, [P, I32, I32, P])
    assert _ffi.SIGNATURES[QUERIES[0]] == _ffi.SIGNATURES[QUERIES[1]] == (C.c_int, [P, P, P, U32, SZ, P, P, P])
    assert _ffi.SIGNATURES[QUERIES[2]] == (C.c_int, [P, P, P, U32, SZ, I32, P, P, P, P])
    raw = C.CDLL(mrt.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        fn = getattr(mrt.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert callable(mrt.DeviceScene.set_mesh_masks) and callable(mrt.DeviceScene.mesh_masks)
    assert mrt.lib.mrt_abi_version() == 3
    assert "ignore" in mrt.Renderer.__doc__ and "mask" in mrt.Renderer.__doc__ and "IGNORE MASKS" in mrt.DeviceScene.set_mesh_masks.__doc__


def test_cpp_mirror_names_the_methods(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*set)(MRTScene, int32_t, const std::vector<uint32_t> &) = &mrt::Scene::setMeshMasks;\n"
                   "std::vector<uint32_t> (*get)(MRTScene, int32_t, int32_t) = &mrt::Scene::meshMasks;\n"
                   "void (*closest)(MRTScene, const void *, const void *, uint32_t, size_t, void *, void *, const void *) = &mrt::Scene::intersectClosestMaskedDevice;\n"
                   "void (*any)(MRTScene, const void *, const void *, uint32_t, size_t, void *, void *, const void *) = &mrt::Scene::intersectAnyMaskedDevice;\n"
                   "void (*all)(MRTScene, const void *, const void *, uint32_t, size_t, int32_t, void *, void *, void *, const void *) = &mrt::Scene::intersectAllMaskedDevice;\n"
                   "void (mrt::Renderer::*member)(const void *, const void *, uint32_t, size_t, void *, void *, const void *) = &mrt::Renderer::intersectClosestMaskedDevice;\n"
                   "void (mrt::Renderer::*setm)(int32_t, const std::vector<uint32_t> &) = &mrt::Renderer::setMeshMasks;\n"
                   "static_assert(MRT_RAY_MASK_PRIMARY == (MRT_GEOMETRY_MASK_TRIANGLE | MRT_GEOMETRY_MASK_LIGHT) && MRT_RAY_MASK_SHADOW == MRT_GEOMETRY_MASK_TRIANGLE, \"\");\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


# ---------------------------------------------------------------- refusals that need no device
def test_plain_arguments_are_refused_before_the_scene_is_looked_at(mrt):
    lib = mrt.lib
    P = C.c_void_p
    good = P(4096)                       # an aligned address that is never dereferenced: every call below returns before the scene is looked at

    def last():
        return lib.mrt_last_error().decode()

    def call(q, rays=good, masks=None, n=4, k=4, out=good, counts=good, count=None):
        if q == 2: return lib.mrt_scene_intersect_all_masked_device(None, rays, masks, 1, n, k, out, counts, None, count)
        return getattr(lib, QUERIES[q])(None, rays, masks, 1, n, out, None, count)

    for q in range(3):
        for kw in ({"rays": None}, {"out": None}):
            assert call(q, **kw) == INVALID and "NULL buffers" in last(), (q, kw)
        assert call(q, n=2 ** 31, k=1) == INVALID and "2^31" in last()
        assert call(q, rays=P(4098)) == INVALID and "aligned" in last()
        assert call(q, masks=P(4098)) == INVALID and "aligned" in last()
        assert call(q, count=P(4098)) == INVALID and "d_count" in last()
        assert call(q, out=P(4098)) == INVALID and "aligned" in last()
        assert call(q, n=0, rays=None, out=None, counts=None) == INVALID and "scene is NULL" in last()
        assert call(q, masks=good, count=good) == INVALID and "scene is NULL" in last()                # ... and the NULL scene last
    assert call(2, out=P(4104)) == INVALID and "16-byte" in last()                                     # the list's rows: two 16-byte stores per record
    assert call(0, out=P(4100)) == INVALID and "scene is NULL" in last()                               # a closest record is written in words, as the unmasked entry writes it
    assert call(1, out=P(4100)) == INVALID and "scene is NULL" in last()                               # the any-hit answers are words
    for k in (0, -1, 17):
        assert call(2, k=k) == INVALID and "max_hits" in last(), k
    assert call(2, counts=None) == INVALID and "NULL buffers" in last()
    assert call(2, counts=P(4098)) == INVALID and "aligned" in last()
    assert call(2, n=2 ** 27, k=16) == INVALID and "n * max_hits" in last()
    assert call(2, n=2 ** 27 - 1, k=16) == INVALID and "scene is NULL" in last()
    for entry in ENTRIES[:2]:
        assert getattr(lib, entry)(None, 0, 0, None) == INVALID and "scene is NULL" in last()


def test_python_arguments_raise_before_the_library_is_called(mrt):
    """a DeviceScene without a handle: any call that reached the library would fail with something other than ValueError"""
    import torch

    class Ctx:
        device = 0
    ds = object.__new__(mrt.DeviceScene)
    ds.ctx = Ctx()
    assert ds._mask_args(5, 7)[1] == 5 and ds._mask_args(0xFFFFFFFF, 7)[0].value is None
    for bad in (True, -1, 2 ** 32, 1.0, "1", [1, 2], np.zeros(7, np.uint32), torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ds._mask_args(bad, 7)
    for bad in ([[1, 2]], [1.5], [-1], [2 ** 32], 3):
        with pytest.raises(ValueError):
            ds.set_mesh_masks(bad)
    for method in (ds.intersect_closest_device, ds.intersect_any_device):
        with pytest.raises(ValueError):
            method(torch.zeros((7, 8)), mask="x")
    with pytest.raises(ValueError):
        ds.intersect_all_device(torch.zeros((7, 8)), 4, mask="x")


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_masked_kernels_use_no_scratch(tmp_path):
    """compiled as the Makefile compiles them (no GPU needed): eight kernels — three walks x three queries without the two-level all-hits —, none with scratch, none above
    128 VGPRs (four waves per SIMD stay possible)"""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "masked.o" in line.split()
    s = str(tmp_path / "masked.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "masked.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    seen = {}
    for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt):
        if "k_masked" in m.group(1): seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 8 and all(v == 0 for v in seen.values()), seen
    for name in seen:
        v = re.search(rf"\.set {re.escape(name)}\.num_vgpr, (\d+)", txt)
        assert v and int(v.group(1)) <= 128, (name, v and v.group(1))
        form, query = map(int, re.search(r"4FormE(\d)ELNS_11MaskedQueryE(\d)E", name).groups())          # Form: 8-wide, rope, two-level; MaskedQuery: closest, any, all
        ceiling = ((70, 62, 70), (51, 45, 61), (96, 71, None))[form][query]          # DESIGN.md §10p's table: a register regression fails here, not on a GPU
        assert int(v.group(1)) <= ceiling, (name, v.group(1), ceiling)
