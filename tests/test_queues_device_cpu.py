"""Row queues on device buffers (mrt_context_compact_rows_device and the six *_device_counted entries) as far as they can be checked without a GPU: the
header, the compile-time pin and the ctypes mirror, the workspace size, every refusal that needs no device — each reached with a NULL handle, which is refused last — and
the resources and the instruction mix of the kernels of queues.hip."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INVALID = 1
COMPACT = "mrt_context_compact_rows_device"
TWINS = ("mrt_scene_intersect_closest_device", "mrt_scene_intersect_any_device", "mrt_scene_resolve_hits_device", "mrt_scene_interpolate_device", "mrt_scene_scatter_device",
         "mrt_scene_scatter_materials_device")
P, SZ, I32 = C.c_void_p, C.c_size_t, C.c_int32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrt_abi.h")).read(), flags=re.S)


def _ctype_of(arg):
    """the ctypes type of one parameter of a declaration of include/mrt_abi.h"""
    arg = arg.strip()
    if "*" in arg: return "pointer"
    return {"size_t": SZ, "int32_t": I32, "uint32_t": C.c_uint32, "MRTScene": P, "MRTContext": P, "MRTRenderer": P}[arg.split()[0]]


def _declared(name):
    m = re.search(r"^(\w+) " + name + r"\((.*?)\);", _header(), re.M | re.S)
    assert m, f"{name} is not declared in include/mrt_abi.h"
    return m.group(1), [_ctype_of(a) for a in m.group(2).split(",")]


# ---------------------------------------------------------------- ABI and ffi
def test_header_declares_the_eight_functions_and_the_column():
    hdr = _header()
    assert re.search(r"^#define MRT_ABI_VERSION 3\b", open(os.path.join(ROOT, "include", "mrt_abi.h")).read(), re.M)
    assert re.search(r"typedef struct \{ const void \*src; void \*dst; uint32_t row_bytes; uint32_t _pad; \} MRTRowColumn;", hdr)
    assert _declared("mrt_compact_workspace_bytes") == ("size_t", [SZ])
    res, args = _declared(COMPACT)
    assert res == "int" and args == [P, "pointer", SZ, "pointer", "pointer", I32, "pointer", "pointer", SZ, "pointer"]
    for twin in TWINS:
        res, args = _declared(twin + "_counted")
        assert res == "int" and args == _declared(twin)[1] + ["pointer"], twin          # the twin's arguments and one more pointer, d_count
        assert re.search(twin + r"_counted\([^;]*const void \*d_count\);", hdr, re.S), twin


def test_abi_check_pins_the_column():
    txt = open(os.path.join(CSRC, "abi_check.h")).read()
    assert "static_assert(sizeof(MRTRowColumn) == 24" in txt
    for field, off in (("src", 0), ("dst", 8), ("row_bytes", 16), ("_pad", 20)):
        assert f"MRT_AT(MRTRowColumn, {field}, {off})" in txt, field


def test_ffi_matches_the_header(mrt):
    from metal_raytracing_amd import _ffi
    col = _ffi.RowColumn
    assert C.sizeof(col) == 24 and [getattr(col, f).offset for f in ("src", "dst", "row_bytes", "_pad")] == [0, 8, 16, 20] and mrt.RowColumn is col
    for name in ("mrt_compact_workspace_bytes", COMPACT) + tuple(t + "_counted" for t in TWINS):
        res, args = _declared(name)
        fres, fargs = _ffi.SIGNATURES[name]
        assert fres is {"int": C.c_int, "size_t": SZ}[res] and len(fargs) == len(args), name
        for have, want in zip(fargs, args):
            assert (have is P or issubclass(have, C._Pointer)) if want == "pointer" else have is want, (name, have, want)
        fn = getattr(mrt.lib, name)
        assert fn.restype is fres and list(fn.argtypes) == fargs
    assert _ffi.SIGNATURES[COMPACT][1][4] == C.POINTER(col)
    for twin in TWINS:
        assert _ffi.SIGNATURES[twin + "_counted"][1] == _ffi.SIGNATURES[twin][1] + [P]
    assert mrt.lib.mrt_abi_version() == 3
    import inspect
    for method in ("intersect_closest_device", "intersect_any_device", "resolve_hits_device", "interpolate_device", "scatter_device", "scatter_materials_device"):
        assert inspect.signature(getattr(mrt.DeviceScene, method)).parameters["count"].default is None, method
    assert list(inspect.signature(mrt.DeviceScene.compact_rows_device).parameters) == ["self", "keep", "columns", "count", "out", "workspace", "stream"]


def test_workspace_bytes_is_never_zero_and_does_not_decrease(mrt):
    sizes = [mrt.lib.mrt_compact_workspace_bytes(n) for n in (1, 2 ** 11, 2 ** 20, 2 ** 31 - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes), sizes
    assert all(s % 16 == 0 for s in sizes) and sizes[-1] >= 4 * ((2 ** 31 - 1 + 2047) // 2048)         # one dword per workgroup of 2 048 rows


# ---------------------------------------------------------------- refusals that need no device
def test_compaction_refuses_its_arguments_before_the_context(mrt):
    """One assertion per refusal rule.  Every pointer is a plausible address that is never dereferenced: each call returns before the context is looked at, and the call
    with nothing wrong is refused for its NULL context alone."""
    lib = mrt.lib
    from metal_raytracing_amd._ffi import RowColumn
    n = 1000
    keep, cin, cout, ws = 0x10000, 0x20000, 0x20010, 0x30000
    need = lib.mrt_compact_workspace_bytes(n)

    def cols(*rows):
        t = (RowColumn * max(1, len(rows)))()
        for k, (src, dst, rb) in enumerate(rows): t[k].src, t[k].dst, t[k].row_bytes = src, dst, rb
        return t, len(rows)

    good = [(0x100000, 0x200000, 32), (0x300000, 0x400000, 4)]

    def call(keep=keep, n=n, cin=cin, rows=good, ncols=None, cout=cout, ws=ws, wsb=need, table=True):
        t, k = cols(*rows)
        return lib.mrt_context_compact_rows_device(None, keep, n, cin, t if table else None, k if ncols is None else ncols, cout, ws, wsb, None)

    def last():
        return lib.mrt_last_error().decode()

    assert call() == INVALID and "ctx is NULL" in last()                                                   # nothing to refuse but the handle
    assert call(cin=None) == INVALID and "ctx is NULL" in last()                                           # the incoming count may be left out
    assert call(rows=[]) == INVALID and "ctx is NULL" in last()                                            # a count alone
    assert call(n=0, keep=None, ws=None, wsb=0) == INVALID and "ctx is NULL" in last()
    # NULL d_keep, d_count_out or d_workspace with n > 0
    assert call(keep=None) == INVALID and "d_keep" in last() and "NULL" in last()
    assert call(cout=None) == INVALID and "d_count_out" in last() and "NULL" in last()
    assert call(ws=None) == INVALID and "d_workspace" in last() and "NULL" in last()
    # the count words: 4-byte aligned, and not one another
    assert call(cin=cin + 2) == INVALID and "d_count_in" in last() and "4-byte" in last()
    assert call(cout=cout + 1) == INVALID and "d_count_out" in last() and "4-byte" in last()
    assert call(cin=cout) == INVALID and "d_count_out" in last() and "d_count_in" in last()
    # ncolumns outside 0 .. 8, NULL columns with ncolumns > 0
    assert call(ncols=-1) == INVALID and "ncolumns" in last()
    assert call(ncols=9) == INVALID and "ncolumns" in last()
    assert call(table=False) == INVALID and "columns" in last() and "NULL" in last()
    # row_bytes: 0, above 64, no multiple of 4
    for rb in (0, 68, 6):
        assert call(rows=[(0x100000, 0x200000, rb)]) == INVALID and "columns[0].row_bytes" in last(), rb
    assert call(rows=[good[0], (0x300000, 0x400000, 128)]) == INVALID and "columns[1].row_bytes" in last()
    # alignment: 16 bytes where the row is a multiple of 16, 4 bytes otherwise
    assert call(rows=[(0x100008, 0x200000, 32)]) == INVALID and "columns[0].src" in last() and "16-byte" in last()
    assert call(rows=[(0x100000, 0x200004, 64)]) == INVALID and "columns[0].dst" in last() and "16-byte" in last()
    assert call(rows=[(0x100002, 0x200000, 12)]) == INVALID and "columns[0].src" in last() and "4-byte" in last()
    assert call(rows=[(0x100000, 0x200001, 4)]) == INVALID and "columns[0].dst" in last() and "4-byte" in last()
    assert call(rows=[(0x100004, 0x200008, 12)]) == INVALID and "ctx is NULL" in last()                    # 4-byte alignment is enough for a 12-byte row
    # a dst range that overlaps its own src range, another column's dst range, d_keep or either count word
    assert call(rows=[(0x100000, 0x100000, 32)]) == INVALID and "columns[0].dst" in last() and "src" in last()                       # in place
    assert call(rows=[(0x100000, 0x100000 + 32 * (n - 1), 32)]) == INVALID and "columns[0].dst" in last() and "src" in last()        # the last source row
    assert call(rows=[(0x100000, 0x100000 + 32 * n, 32)]) == INVALID and "ctx is NULL" in last()                                     # back to back is no overlap
    assert call(rows=[good[0], (0x300000, 0x200000 + 32 * n - 4, 4)]) == INVALID and "columns[1].dst" in last() and "columns[0].dst" in last()
    assert call(rows=[(0x100000, keep + n - 4, 4)]) == INVALID and "columns[0].dst" in last() and "d_keep" in last()
    assert call(rows=[(0x100000, cin - 4 * (n - 1), 4)]) == INVALID and "columns[0].dst" in last() and "d_count_in" in last()
    assert call(rows=[(0x100000, cout, 4)]) == INVALID and "columns[0].dst" in last() and "d_count_out" in last()
    # the workspace: too small (and the contract's alignment)
    assert call(wsb=need - 1) == INVALID and "workspace_bytes" in last() and "mrt_compact_workspace_bytes" in last()
    assert call(n=2 ** 20, rows=[], wsb=lib.mrt_compact_workspace_bytes(2 ** 20) - 16) == INVALID and "workspace_bytes" in last()
    assert call(ws=ws + 8) == INVALID and "d_workspace" in last() and "16-byte" in last()
    # n >= 2^31
    assert call(n=2 ** 31, wsb=2 ** 40) == INVALID and "2^31" in last()
    assert call(n=2 ** 31 - 1, wsb=2 ** 40, rows=[]) == INVALID and "ctx is NULL" in last()


def test_counted_twins_refuse_a_bad_count_word_first(mrt):
    """Each twin: a NULL d_count and a misaligned one are refused, by name, before anything else — here with a NULL scene — and with a good one the call goes on to its
    twin's refusals in the twin's words, the NULL handle last."""
    lib = mrt.lib
    good = P(4096)

    def last():
        return lib.mrt_last_error().decode()

    calls = {
        "mrt_scene_intersect_closest_device": lambda fn, *c: fn(None, good, 4, good, None, *c),
        "mrt_scene_intersect_any_device": lambda fn, *c: fn(None, good, 4, good, None, *c),
        "mrt_scene_resolve_hits_device": lambda fn, *c: fn(None, good, good, 4, good, None, *c),
        "mrt_scene_interpolate_device": lambda fn, *c: fn(None, good, 4, good, 12, 3, good, 12, None, *c),
        "mrt_scene_scatter_device": lambda fn, *c: fn(None, good, good, 4, 0, 0, good, good, good, None, *c),
        "mrt_scene_scatter_materials_device": lambda fn, *c: fn(None, good, good, good, 4, 0, 3, 0, good, good, good, good, None, *c),
    }
    assert set(calls) == set(TWINS)
    for twin, call in calls.items():
        counted = getattr(lib, twin + "_counted")
        assert call(counted, None) == INVALID and "d_count is NULL" in last() and (twin + "_counted:") in last(), twin
        assert call(counted, P(4098)) == INVALID and "d_count" in last() and "4-byte" in last() and (twin + "_counted:") in last(), twin
        assert call(counted, P(4100)) == INVALID and "d_count" not in last() and (twin + "_counted:") in last(), twin          # the scene is NULL: the twin's refusal
        theirs = last().split(":", 1)[1]
        assert call(getattr(lib, twin)) == INVALID and last() == twin + ":" + theirs, twin
    # a plain argument of the twin's is still refused in the twin's words, after the count word
    assert lib.mrt_scene_scatter_device_counted(None, good, good, 4, 19, 0, good, good, good, None, P(4100)) == INVALID and "bounce" in last()
    assert lib.mrt_scene_scatter_device_counted(None, good, good, 4, 19, 0, good, good, good, None, None) == INVALID and "d_count is NULL" in last()
    assert lib.mrt_scene_resolve_hits_device_counted(None, P(4104), good, 4, good, None, P(4100)) == INVALID and "16-byte" in last()
    assert lib.mrt_scene_interpolate_device_counted(None, good, 4, good, 12, 65, good, 12, None, P(4100)) == INVALID and "channels" in last()
    assert lib.mrt_scene_intersect_any_device_counted(None, good, 2 ** 31, good, None, P(4100)) == INVALID and "bad argument" in last()


# ---------------------------------------------------------------- kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_queue_kernels_use_no_scratch_no_atomics_and_never_wait(tmp_path):
    """Compiled as the Makefile compiles it (no GPU needed).  A spill would add traffic to kernels that are nothing but traffic; and no workgroup may wait for another —
    a look-back or a ticket needs an atomic or a sleeping poll, so the text holds neither."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
        if line.startswith("OBJS"): assert "queues.o" in line.split()
    assert flags and "-ffp-contract=off" in flags
    s = str(tmp_path / "queues.s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, "queues.hip")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = open(s).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.set (_Z\w+)\.private_seg_size, (\d+)", txt)}
    kernels = set(re.findall(r"\.amdhsa_kernel (\S+)", txt))
    assert len(kernels) == 3 and all(any(k in name for name in kernels) for k in ("k_queue_count", "k_queue_scan", "k_queue_move")), kernels
    for name in kernels:
        assert sizes[name] == 0, f"{name}: {sizes[name]} bytes of scratch"
    for word in ("global_atomic", "flat_atomic", "ds_add", "ds_cmpst", "s_sleep", "buffer_atomic", "scratch_"):
        assert word not in txt, word
    for word in ("v_mbcnt_lo_u32_b32", "s_bcnt1_i32_b64", "ds_read", "global_load_dwordx4", "global_store_dwordx4", "global_load_ubyte"):          # ballot ranks, LDS totals, 16-byte rows
        assert word in txt, word
    # no traversal, shading or builder code is compiled in this translation unit
    src = open(os.path.join(CSRC, "queues.hip")).read()
    assert re.findall(r'#include "(\w+\.h)"', src) == ["scene_device.h"]
