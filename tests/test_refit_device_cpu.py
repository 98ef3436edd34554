"""The stream-ordered refit entries without a GPU: argument checks of the C ABI, the ctypes table, the C++ mirror in include/mrt.hpp and the C header."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_scene_is_an_invalid_argument_with_a_message(mrt):
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    count = C.c_uint64(7)
    calls = {"mrt_scene_update_mesh_device": lambda f: f(None, 0, p, 12, p, 12, 1, None),
             "mrt_scene_refit_device": lambda f: f(None, None),
             "mrt_scene_device_updates_rejected": lambda f: f(None, C.byref(count))}
    for name, call in calls.items():
        assert call(getattr(mrt.lib, name)) == 1, name          # MRT_ERR_INVALID_ARGUMENT
        assert name in mrt.lib.mrt_last_error().decode()


def test_ffi_declares_the_entries(mrt):
    from metal_raytracing_amd import _ffi
    P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32
    assert _ffi.SIGNATURES["mrt_scene_update_mesh_device"] == (C.c_int, [P, I32, P, SZ, P, SZ, SZ, P])
    assert _ffi.SIGNATURES["mrt_scene_refit_device"] == (C.c_int, [P, P])
    assert _ffi.SIGNATURES["mrt_scene_device_updates_rejected"] == (C.c_int, [P, C.POINTER(C.c_uint64)])
    for name in ("mrt_scene_update_mesh_device", "mrt_scene_refit_device", "mrt_scene_device_updates_rejected"):
        fn = getattr(mrt.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _ffi.SIGNATURES[name][1]
    assert callable(mrt.DeviceScene.update_mesh_device) and callable(mrt.DeviceScene.refit_device) and isinstance(mrt.DeviceScene.device_updates_rejected, property)


def test_abi_version_stays_3(mrt):
    assert mrt.lib.mrt_abi_version() == 3


def test_cpp_mirror_names_the_methods(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include "mrt.hpp"\n'
                   "void (*update)(MRTScene, int32_t, const void *, size_t, const void *, size_t, size_t, void *) = &mrt::Scene::updateMeshDevice;\n"
                   "void (*refit)(MRTScene, void *) = &mrt::Scene::refitDevice;\n"
                   "uint64_t (*rejected)(MRTScene) = &mrt::Scene::deviceUpdatesRejected;\n"
                   "uint64_t use(mrt::Renderer &r, const void *interleaved, size_t n) {\n"
                   "    r.updateMeshDevice(1, interleaved, 32, static_cast<const char *>(interleaved) + 16, 32, n, r.stream());\n"
                   "    r.refitDevice(r.stream());\n"
                   "    mrt::Scene::updateMeshDevice(r.sceneHandle(), 1, interleaved, 12, interleaved, 12, n, nullptr);\n"
                   "    mrt::Scene::refitDevice(r.sceneHandle(), nullptr);\n"
                   "    return r.deviceUpdatesRejected();\n"
                   "}\n")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]


def test_the_header_is_still_c99(tmp_path):
    src = tmp_path / "tu.c"
    src.write_text('#include "mrt_abi.h"\n'
                   "int use(MRTScene s, const void *p, void *stream, uint64_t *n) {\n"
                   "    int rc = mrt_scene_update_mesh_device(s, 0, p, 16, p, 16, 4, stream);\n"
                   "    if (!rc) rc = mrt_scene_refit_device(s, stream);\n"
                   "    return rc ? rc : mrt_scene_device_updates_rejected(s, n);\n"
                   "}\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
