"""mrt_scene_rebuild_tlas_device without a GPU.  First the premise its kernels rest on: the host TLAS builders split at count // 2, so the links of the
rope TLAS depend on the instance count alone, and a strict order decides what goes into each half, so a re-sort of the ids from ANY start permutation — restated in numpy
float32 in tlas_resort_reference.py — gives every rope leaf the host's instance set and the 8-wide form the host's leaf order.  Then the argument checks of the C ABI, the
ctypes table, the C++ mirror and the C header, as tests/test_instances_device_cpu.py makes them for its entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tlas_resort_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mrt_scene_rebuild_tlas_device"
COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 150, 1000)
KINDS = ("random", "equal_centroids", "identical", "equal_extents")


def _boxes(kind, n, seed=0):
    rng = np.random.default_rng(100 * n + seed + 17 * KINDS.index(kind))
    c = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
    h = rng.uniform(0.05, 0.6, (n, 3)).astype(np.float32)
    if kind == "equal_centroids":          # x is the widest axis at the root, and on it the boxes share a handful of lo + hi sums: the id breaks the ties
        c[:, 0] = rng.integers(-3, 4, n).astype(np.float32) * 4.0
        h[:, 0] = 0.25
    elif kind == "identical":
        c[:] = c[0]; h[:] = h[0]
    elif kind == "equal_extents":          # every axis holds the same centre values in another order: three equal extents at the root, axis 0 is taken
        v = (np.arange(n, dtype=np.float32) - np.float32(n // 2)) * np.float32(0.5)
        c = np.stack([v[rng.permutation(n)] for _ in range(3)], axis=1)
        h[:] = 0.25
    return (c - h).astype(np.float32), (c + h).astype(np.float32)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_resort_gives_the_host_builders_sets(mrt, kind, n):
    lo, hi = _boxes(kind, n)
    host = R.host_build(mrt.lib, lo, hi)
    start = np.random.default_rng(n).permutation(n).astype(np.uint32)          # whatever tlas_index held
    ids = R.median_order(lo, hi, start)
    assert sorted(ids.tolist()) == list(range(n))
    leaves = R.rope_leaves(host["rope_links"])
    assert sum(c for _, c in leaves) == n and all(1 <= c <= 2 for _, c in leaves)
    for first, count in leaves:
        assert set(ids[first:first + count].tolist()) == set(host["rope_order"][first:first + count].tolist()), (first, count)
    assert sorted(host["wide_pos"].tolist()) == list(range(n)), "every leaf position is one entry of the 8-wide form's order"
    assert np.array_equal(ids[host["wide_pos"]], host["wide_order"])
    assert np.array_equal(R.median_order(lo, hi, ids), ids), "the order is strict: a second re-sort is a fixed point"
    assert np.array_equal(R.median_order(lo, hi, np.arange(n, dtype=np.uint32)), ids), "the result does not depend on the start"
    if kind == "equal_extents" and n >= 3:
        s = lo[:, 0] + hi[:, 0]
        half = n // 2
        assert s[ids[:half]].max() <= s[ids[half:]].min(), "three equal extents: the root splits on axis 0"
    assert int(host["rope_levels"].sum()) == len(host["rope_links"]) and int(host["wide_levels"].sum()) == host["wide_nodes"]


@pytest.mark.parametrize("n", COUNTS)
def test_the_rope_links_depend_on_the_count_alone(mrt, n):
    a = R.host_build(mrt.lib, *_boxes("random", n, seed=1))
    for kind, seed in (("random", 2), ("identical", 0), ("equal_centroids", 3)):
        b = R.host_build(mrt.lib, *_boxes(kind, n, seed=seed))
        assert np.array_equal(a["rope_links"], b["rope_links"]), kind
        assert np.array_equal(a["rope_levels"], b["rope_levels"]), kind
    # ... and they are the ranges the re-sort walks: the leaves tile [0, n) in order
    at = 0
    for first, count in R.rope_leaves(a["rope_links"]):
        assert first == at; at += count
    assert at == n


def test_host_build_checks_its_arguments(mrt):
    buf = (C.c_uint32 * 68)()
    assert mrt.lib.mrt_debug_tlas_host_build(None, None, 1, buf, buf, buf, buf, buf) == 1
    assert "mrt_debug_tlas_host_build" in mrt.lib.mrt_last_error().decode()
    f = (C.c_float * 4)()
    assert mrt.lib.mrt_debug_tlas_host_build(f, f, 0, buf, buf, buf, buf, buf) == 1


def test_the_header_declares_the_entry():
    txt = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^int mrt_scene_rebuild_tlas_device\(MRTScene scene, void \*hip_stream\);", txt, re.M)
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", txt, re.M), "an entry was added, no struct changed: the version line stays"
    dbg = open(os.path.join(ROOT, "include", "mrt_debug.h")).read()
    assert re.search(r"^int mrt_debug_tlas_host_build\(", dbg, re.M)


def test_null_scene_is_an_invalid_argument_with_a_message(mrt):
    assert mrt.lib.mrt_scene_rebuild_tlas_device(None, None) == 1          # MRT_ERR_INVALID_ARGUMENT
    assert ENTRY in mrt.lib.mrt_last_error().decode()


def test_ffi_declares_the_entry(mrt):
    from metal_raytracing_amd import _ffi
    P = C.c_void_p
    assert _ffi.SIGNATURES[ENTRY] == (C.c_int, [P, P])
    fn = getattr(mrt.lib, ENTRY)
    assert fn.restype is C.c_int and list(fn.argtypes) == [P, P]
    assert callable(mrt.DeviceScene.rebuild_tlas_device)
    assert mrt.DeviceScene._LAYOUT_PARTS["tlas_nodes"] == 6 and mrt.DeviceScene._LAYOUT_PARTS["tlas_index"] == 7


def test_abi_version_stays_3(mrt):
    assert mrt.lib.mrt_abi_version() == 3


def test_cpp_mirror_names_the_method(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*rebuild)(MRTScene, void *) = &mrt::Scene::rebuildTlasDevice;\n"
                   "void use(mrt::Renderer &r, const void *poses, size_t n) {\n"
                   "    mrt::Scene::setInstanceTransformsDevice(r.sceneHandle(), 0, n, poses, 64, r.stream());\n"
                   "    mrt::Scene::rebuildTlasDevice(r.sceneHandle(), r.stream());\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_the_header_is_still_c99_and_cpp11(tmp_path):
    body = ('#include "mrt_abi.h"\n'
            "int use(MRTScene s, const void *p, void *stream) {\n"
            "    int rc = mrt_scene_set_instance_transforms_device(s, 0, 4, p, 64, stream);\n"
            "    return rc ? rc : mrt_scene_rebuild_tlas_device(s, stream);\n"
            "}\n")
    for name, cmd in (("tu.c", ["gcc", "-std=c99"]), ("tu.cpp", ["g++", "-std=c++11"])):
        src = tmp_path / name
        src.write_text(body)
        p = subprocess.run(cmd + ["-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
