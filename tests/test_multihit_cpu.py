"""The all-hits query (mrt_scene_intersect_all_device) as far as it can be checked without a GPU: the yardstick of the GPU tests
(tests/multihit_reference.py) pinned bit for bit to the oracle's brute-force closest hit for K = 1, known answers that follow from the definition alone, the ABI and its
ctypes mirror, the refusals that need no device, and the kernels' resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multihit_reference as M
from test_gpu_parity import _rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
f32 = np.float32
ENTRIES = ("mrt_scene_intersect_all_device", "mrt_scene_intersect_all_device_counted")


# ---------------------------------------------------------------- the fused multiply-add the reference stands on
def _exact_f32(x):
    """Fraction -> the nearest float32, ties to even, found among the neighbours of a first guess"""
    from fractions import Fraction
    g = f32(float(x))                                        # within one float32 ulp of the answer
    best = None
    for y in (g, np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(-np.inf))):
        key = (abs(Fraction(float(y)) - x), int(np.asarray(y).view(np.uint32)) & 1)
        if best is None or key < best[0]: best = (key, y)
    return best[1]


def test_fma_rounds_once():
    """against exact rational arithmetic: random operands with and without cancellation, results in the subnormal range, and the double-rounding case built by hand —
    p = 2^-24 (1 - 2^-46), c = 1 + 2^-23: the exact sum lies 2^-70 BELOW the midpoint c + 2^-24, float64 rounds it ONTO the midpoint, and ties-to-even then rounds the
    wrong way (c's significand is odd)"""
    from fractions import Fraction
    a, b, c = f32(2.0 ** -12 * (1 + 2.0 ** -23)), f32(2.0 ** -12 * (1 - 2.0 ** -23)), f32(1 + 2.0 ** -23)
    naive = f32(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive == f32(1 + 2.0 ** -22) and M.fma(a, b, c) == c and M.fma(-a, b, -c) == -c          # the naive form is wrong here; the emulation is not
    assert M.fma(a, f32(2.0 ** -12 * (1 + 2.0 ** -23)), c) == f32(1 + 2.0 ** -22)                    # above the midpoint: up
    rng = np.random.default_rng(7)
    x = rng.normal(size=3000).astype(f32); y = rng.normal(size=3000).astype(f32)
    z = (-(x.astype(np.float64) * y) * rng.choice([1.0, 1 + 2e-7, 0.5, 1e-3], 3000)).astype(f32)
    tiny = f32(2.0 ** -140)
    x = np.concatenate([x, x[:300] * tiny]); y = np.concatenate([y, y[:300]]); z = np.concatenate([z, z[:300] * tiny])
    got = M.fma(x, y, z)
    for k in range(x.size):
        want = _exact_f32(Fraction(float(x[k])) * Fraction(float(y[k])) + Fraction(float(z[k])))
        assert got[k] == want, (k, x[k], y[k], z[k], got[k], want)


# ---------------------------------------------------------------- the reference against the oracle's brute force, K = 1
@pytest.mark.parametrize("name,n", [("sphere", 3000), ("train", 3000), ("teapot", 1500)])
def test_reference_with_one_hit_equals_the_oracles_brute_force(mrt, orc, name, n):
    """the rotated and scaled models and the rays of test_gpu_parity.test_intersect_matches_brute_force, open rays and windowed ones: every field, distances and
    barycentrics as bit patterns"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name=name, position=[0.1, -0.2, 0.3], rotation=[0.2, 0.5, -0.1], scale=1.3),
                           mrt.Model(name="plane", position=[0, -3, 0], scale=50)]
    sc = S((8, 8))
    entries = mrt.flatten_scene(sc)
    osc = orc.OracleScene(entries, sc.lights)
    ref = M.MultihitReference(entries)
    assert ref.triangles == osc.triangles
    me = sc.meshes[0]
    w = (me.transform.T @ np.c_[me.positions, np.ones(len(me.positions))].T).T[:, :3]
    rays = _rays(np.random.default_rng(11), n, w.min(0), w.max(0))
    rays[:6, 4:7] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    windowed = rays.copy()
    windowed[:, 7] = np.random.default_rng(5).uniform(0.2, 6.0, len(rays)).astype(f32)
    windowed[:, 3] = 0.05
    for r in (rays, windowed):
        o = osc.intersect_closest(r, brute=True)
        h, c = ref.intersect_all(r, 1)
        assert (o["type"] == 1).mean() > (0.3 if r is rays else 0.05)          # (the windows cut most hits away; some must stay)
        assert np.array_equal(c, o["type"])
        for f in ("type", "instance_id", "geometry_id", "primitive_id", "_pad"):
            assert np.array_equal(h[:, 0][f], o[f]), f
        for f in ("distance", "u", "v"):
            bad = np.flatnonzero(h[:, 0][f].view(np.uint32) != o[f].view(np.uint32))
            assert bad.size == 0, (f, bad.size, h[bad[0], 0], o[bad[0]])
    osc.close()


# ---------------------------------------------------------------- known answers from the definition alone
def _ray(o, d, tmin=0.0, tmax=np.inf):
    return np.array([[o[0], o[1], o[2], tmin, d[0], d[1], d[2], tmax]], f32)


INTERIOR, DIAGONAL, CORNER = (0.75, 0.25), (0.5, 0.5), (1.0, 1.0)          # inside triangle 0 of every quad; on the shared diagonal; at the corner both triangles share


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_quad_stack_lists_the_layers_in_order(mrt, K):
    for L in (0, 1, K - 1, K, K + 1, 2 * K):
        ref = M.MultihitReference(mrt.flatten_scene(M.quad_stack(mrt, L)))
        assert ref.triangles == 2 * L
        h, c = ref.intersect_all(_ray((*INTERIOR, 0.0), (0, 0, 1)), K)
        m = min(L, K)
        assert c[0] == m and list(h[0, :m]["distance"]) == [float(k + 1) for k in range(m)]
        assert list(h[0, :m]["instance_id"]) == list(range(m)) and (h[0, :m]["primitive_id"] == 0).all() and (h[0, :m]["type"] == 1).all()
        assert M.differing(h[0, m:], np.broadcast_to(M.miss_record(), (K - m,)).copy()) == 0
        for xy in (DIAGONAL, CORNER):          # both triangles of every quad at one distance: the lower id first
            h, c = ref.intersect_all(_ray((*xy, 0.0), (0, 0, 1)), K)
            m = min(2 * L, K)
            assert c[0] == m, (L, K, xy)
            assert list(h[0, :m]["distance"]) == [float(k // 2 + 1) for k in range(m)]
            assert list(h[0, :m]["instance_id"]) == [k // 2 for k in range(m)] and list(h[0, :m]["primitive_id"]) == [k % 2 for k in range(m)]
            assert M.differing(h[0, m:], np.broadcast_to(M.miss_record(), (K - m,)).copy()) == 0


def test_coincident_meshes_give_pairs_ordered_by_id(mrt):
    """two meshes with identical vertices: every hit comes twice, at one distance; K = 1 keeps the lower id, an odd K cuts a pair and keeps its lower id"""
    p1, i1 = M.quad(1.0); p2, i2 = M.quad(2.0)
    ref = M.MultihitReference(mrt.flatten_scene(M.raw_scene(mrt, [(p1, i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p2, i2, M._plain(mrt)), (p2.copy(), i2, M._plain(mrt))])))
    r = _ray((*INTERIOR, 0.0), (0, 0, 1))
    h, c = ref.intersect_all(r, 16)
    assert c[0] == 4 and list(h[0, :4]["distance"]) == [1.0, 1.0, 2.0, 2.0] and list(h[0, :4]["instance_id"]) == [0, 1, 2, 3]
    h, c = ref.intersect_all(r, 1)
    assert c[0] == 1 and h[0, 0]["instance_id"] == 0
    h, c = ref.intersect_all(r, 3)
    assert c[0] == 3 and list(h[0]["instance_id"]) == [0, 1, 2] and list(h[0]["distance"]) == [1.0, 1.0, 2.0]


def test_window_ends_are_inclusive(mrt):
    ref = M.MultihitReference(mrt.flatten_scene(M.quad_stack(mrt, 3)))
    two = f32(2.0); below, above = np.nextafter(two, f32(0.0)), np.nextafter(two, f32(4.0))
    o, d = (*INTERIOR, 0.0), (0, 0, 1)
    dist = lambda **kw: [float(x) for x in (lambda hc: hc[0][0, :hc[1][0]]["distance"])(ref.intersect_all(_ray(o, d, **kw), 8))]
    assert dist(tmin=two) == [2.0, 3.0] and dist(tmin=above) == [3.0] and dist(tmin=below) == [2.0, 3.0]
    assert dist(tmax=two) == [1.0, 2.0] and dist(tmax=below) == [1.0] and dist(tmax=above) == [1.0, 2.0]
    assert dist(tmin=two, tmax=two) == [2.0]


# ---------------------------------------------------------------- ABI and ffi
def test_header_declares_the_entries_and_the_version_is_still_3():
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", hdr, re.M)
    assert re.search(r"^#define MRT_MAX_HITS 16\b", hdr, re.M)
    for entry in ENTRIES:
        assert re.search(rf"^int {entry}\(MRTScene scene, const void \*d_rays, size_t n, int32_t max_hits,", hdr, re.M), entry


def test_ffi_carries_both_signatures(mrt):
    from metal_raytracing_amd import _ffi
    P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32
    assert _ffi.SIGNATURES[ENTRIES[0]] == (C.c_int, [P, P, SZ, I32, P, P, P])
    assert _ffi.SIGNATURES[ENTRIES[1]] == (C.c_int, [P, P, SZ, I32, P, P, P, P])
    for name in ENTRIES:
        fn = getattr(mrt.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert callable(mrt.DeviceScene.intersect_all_device)
    assert mrt.lib.mrt_abi_version() == 3
    assert M.INTERSECTION_DTYPE == mrt.INTERSECTION_DTYPE


def test_cpp_mirror_names_the_methods(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*all)(MRTScene, const void *, size_t, int32_t, void *, void *, void *) = &mrt::Scene::intersectAllDevice;\n"
                   "void (*counted)(MRTScene, const void *, size_t, int32_t, void *, void *, void *, const void *) = &mrt::Scene::intersectAllDeviceCounted;\n"
                   "static_assert(MRT_MAX_HITS == 16, \"\");\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_arguments_are_refused_before_any_gpu_work(mrt):
    """The plain arguments are checked first, so every refusal below is reached without a device or a scene; a NULL scene is refused last.  (n == 0 with a committed scene is
    MRT_OK: tests/test_multihit_device.py; here, n == 0 passes every plain check, NULL buffers included, and reaches the scene.)"""
    lib = mrt.lib
    P = C.c_void_p
    good = P(4096)                       # an aligned address that is never dereferenced: every call below returns before the scene is looked at

    def last():
        return lib.mrt_last_error().decode()

    def call(rays=good, n=4, k=4, out=good, counts=good, counted=False, count=good):
        if counted: return lib.mrt_scene_intersect_all_device_counted(None, rays, n, k, out, counts, None, count)
        return lib.mrt_scene_intersect_all_device(None, rays, n, k, out, counts, None)

    for counted in (False, True):
        for k in (0, -1, 17):
            assert call(k=k, counted=counted) == INVALID and "max_hits" in last(), k
        for kw in ({"rays": None}, {"out": None}, {"counts": None}):
            assert call(counted=counted, **kw) == INVALID and "NULL" in last(), kw
        assert call(n=2 ** 31, k=1, counted=counted) == INVALID and "2^31" in last()
        assert call(n=2 ** 27, k=16, counted=counted) == INVALID and "n * max_hits" in last()          # = 2^31
        assert call(n=2 ** 27 - 1, k=16, counted=counted) == INVALID and "scene is NULL" in last()     # just below: not refused for its size
        assert call(out=P(4104), counted=counted) == INVALID and "aligned" in last()
        assert call(counts=P(4098), counted=counted) == INVALID and "aligned" in last()
        assert call(n=0, rays=None, out=None, counts=None, counted=counted) == INVALID and "scene is NULL" in last()
        assert call(counted=counted) == INVALID and "scene is NULL" in last()                          # ... and the NULL scene last
    assert call(counted=True, count=None) == INVALID and "d_count" in last()
    assert call(counted=True, count=P(4098)) == INVALID and "d_count" in last()


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_multihit_kernels_use_no_scratch(tmp_path):
    """The list lives in LDS so that nothing is indexed at run time in private memory.  Compiled as the Makefile compiles them (no GPU needed); the resource figures only."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "multihit.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "multihit.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "multihit.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    seen = set()
    for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt):
        name, size = m.group(1), int(m.group(2))
        if "k_intersect_all" in name:
            seen.add(name)
            assert size == 0, f"{name}: {size} bytes of scratch"
    assert len(seen) == 2, seen          # k_intersect_all<true> (8-wide), k_intersect_all<false> (rope)
    for name in seen:
        v = re.search(rf"\.set {re.escape(name)}\.num_vgpr, (\d+)", txt)
        assert v and int(v.group(1)) <= 128, (name, v and v.group(1))          # at most 128: four waves per SIMD stay possible (LDS bounds the kernels at three for K = 16)
        ceiling = 78 if "ILb1E" in name else 72          # what the kernels needed when they held their own copies of the walks: a register regression fails here, not on a GPU
        assert int(v.group(1)) <= ceiling, (name, v.group(1), ceiling)
