"""The stream-ordered query entries without a GPU: argument checks of the C ABI, the ctypes table, and the C++ mirror in include/mrt.hpp."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_scene_is_an_invalid_argument_with_a_message(mrt):
    buf = (C.c_int32 * 8)()
    for name in ("mrt_scene_intersect_closest_device", "mrt_scene_intersect_any_device"):
        for n in (0, 1):
            assert getattr(mrt.lib, name)(None, C.cast(buf, C.c_void_p), n, C.cast(buf, C.c_void_p), None) == 1          # MRT_ERR_INVALID_ARGUMENT
            assert name in mrt.lib.mrt_last_error().decode()
    out = C.c_void_p(1)
    assert mrt.lib.mrt_context_get_stream(None, C.byref(out)) == 1
    assert "mrt_context_get_stream" in mrt.lib.mrt_last_error().decode()


def test_abi_version_stays_3(mrt):
    assert mrt.lib.mrt_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert "#define MRT_ABI_VERSION 3 " in hdr


def test_ffi_declares_the_entries(mrt):
    from metal_raytracing_amd import _ffi
    P, SZ = C.c_void_p, C.c_size_t
    assert _ffi.SIGNATURES["mrt_scene_intersect_closest_device"] == (C.c_int, [P, P, SZ, P, P])
    assert _ffi.SIGNATURES["mrt_scene_intersect_any_device"] == (C.c_int, [P, P, SZ, P, P])
    assert _ffi.SIGNATURES["mrt_context_get_stream"] == (C.c_int, [P, C.POINTER(P)])
    for name in ("mrt_scene_intersect_closest_device", "mrt_scene_intersect_any_device", "mrt_context_get_stream"):
        fn = getattr(mrt.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert callable(mrt.DeviceScene.intersect_closest_device) and callable(mrt.DeviceScene.intersect_any_device) and callable(mrt.unpack_intersections)
    assert isinstance(mrt.Context.stream, property)


def test_cpp_mirror_names_the_methods(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*closest)(MRTScene, const void *, size_t, void *, void *) = &mrt::Scene::intersectClosestDevice;\n"
                   "void (*any)(MRTScene, const void *, size_t, void *, void *) = &mrt::Scene::intersectAnyDevice;\n"
                   "void use(mrt::Renderer &r, const void *rays, void *out, void *occluded) {\n"
                   "    r.intersectClosestDevice(rays, 16, out, r.stream());\n"
                   "    r.intersectAnyDevice(rays, 16, occluded, nullptr);\n"
                   "    mrt::Scene::intersectClosestDevice(r.sceneHandle(), rays, 16, out, nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
