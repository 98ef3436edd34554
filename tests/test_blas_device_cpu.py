"""The stream-ordered BLAS entries of two-level scenes (mrt_scene_update_blas_device / mrt_scene_refit_blas_device) without a GPU: argument checks of the C ABI, the
ctypes table, the C++ mirror in include/mrt.hpp and the C header."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mrt_scene_update_blas_device", "mrt_scene_refit_blas_device")


def test_the_header_declares_the_entries():
    txt = open(os.path.join(ROOT, "include", "mrt_abi.h")).read()
    assert re.search(r"^int mrt_scene_update_blas_device\(MRTScene scene, int32_t mesh_id, const void \*d_positions, size_t pos_stride_bytes,\s*"
                     r"const void \*d_normals, size_t nrm_stride_bytes, size_t vertex_count, void \*hip_stream\);", txt, re.M)
    assert re.search(r"^int mrt_scene_refit_blas_device\(MRTScene scene, void \*hip_stream\);", txt, re.M)
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", txt, re.M), "entries were added, no struct changed: the version line stays"


def test_null_scene_is_an_invalid_argument_with_a_message(mrt):
    buf = (C.c_float * 12)()
    p = C.cast(buf, C.c_void_p)
    calls = {"mrt_scene_update_blas_device": lambda f: f(None, 0, p, 12, p, 12, 4, None),
             "mrt_scene_refit_blas_device": lambda f: f(None, None)}
    for name, call in calls.items():
        assert call(getattr(mrt.lib, name)) == 1, name          # MRT_ERR_INVALID_ARGUMENT
        assert name in mrt.lib.mrt_last_error().decode()


def test_ffi_declares_the_entries(mrt):
    from metal_raytracing_amd import _ffi
    P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32
    assert _ffi.SIGNATURES["mrt_scene_update_blas_device"] == (C.c_int, [P, I32, P, SZ, P, SZ, SZ, P])
    assert _ffi.SIGNATURES["mrt_scene_refit_blas_device"] == (C.c_int, [P, P])
    for name in ENTRIES:
        fn = getattr(mrt.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert callable(mrt.DeviceScene.update_blas_device) and callable(mrt.DeviceScene.refit_blas_device)


def test_abi_version_stays_3(mrt):
    assert mrt.lib.mrt_abi_version() == 3


def test_cpp_mirror_names_the_methods(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*update)(MRTScene, int32_t, const void *, size_t, const void *, size_t, size_t, void *) = &mrt::Scene::updateBlasDevice;\n"
                   "void (*refit)(MRTScene, void *) = &mrt::Scene::refitBlasDevice;\n"
                   "void use(mrt::Renderer &r, const void *pos, const void *nrm, size_t n) {\n"
                   "    mrt::Scene::updateBlasDevice(r.sceneHandle(), 0, pos, 32, nrm, 32, n, r.stream());\n"
                   "    mrt::Scene::refitBlasDevice(r.sceneHandle(), nullptr);\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_the_header_is_still_c99_and_cpp11(tmp_path):
    body = ('#include "mrt_abi.h"\n'
            "int use(MRTScene s, const void *p, const void *n, void *stream) {\n"
            "    int rc = mrt_scene_update_blas_device(s, 0, p, 12, n, 16, 24, stream);\n"
            "    return rc ? rc : mrt_scene_refit_blas_device(s, stream);\n"
            "}\n")
    for name, cmd in (("tu.c", ["gcc", "-std=c99"]), ("tu.cpp", ["g++", "-std=c++11"])):
        src = tmp_path / name
        src.write_text(body)
        p = subprocess.run(cmd + ["-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
