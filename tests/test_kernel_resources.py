"""The stream traversal kernels read other lanes' registers — the refill takes prefetched rays by ds_bpermute, the cooperative drain reads a straggler's ray by v_readlane — so a
register's value must survive in lanes that are switched off.  Hardware keeps it; a spill store or reload inside divergent control flow covers the active lanes only.  Two variant
builds of round 6 that pushed the persistent kernel from 24 to 60 / 64 bytes of scratch (7 waves per SIMD; the fp16-plane nodes at 6) rendered wrong images in the GPU suite
(profiles/r06_wide16_ab.txt).  The cause: the drain's helpers read their owner's ray with v_readlane INSIDE `if (helping)`, where the owner's lane is off — correct only as long as
the compiler never reloads that register there.  The reads now sit where the whole wave is on (traverse_wide.h), and the 7-wave variant passes the suite; every other cross-lane read
of the library was already at wave-uniform level or names an active lane.  This test compiles the device code (no GPU needed) and keeps an early warning beside the parity suite:
the kernels built on traverse_wide_stream spill at most 32 bytes — the shipped build's 24 are loop-invariant values stored at kernel entry — and never store a spill inside their loop."""
import os, re, shutil, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metal-raytracing_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
STREAM_KERNELS = ("k_trace_mixed_wide_persist", "k_trace_mixed_wide_stream", "k_tl_top", "k_tl_blas", "k_query_stream", "k_trace_primary_wide_stream")


STREAM_UNITS = ("renderer.hip", "query.hip")          # every unit that holds a kernel built on traverse_wide_stream


@pytest.fixture(scope="module")
def stream_asm(tmp_path_factory):
    """The device code of STREAM_UNITS as the Makefile compiles it, as assembly text, one listing after the other (one compile per unit for the module)."""
    flags = None
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"): flags = [f for f in line.split("=", 1)[1].split() if not f.startswith("-W")]
    assert flags and "-ffp-contract=off" in flags
    txt = ""
    for unit in STREAM_UNITS:
        s = str(tmp_path_factory.mktemp("asm") / (unit + ".s"))
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-o", s, os.path.join(CSRC, unit)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        txt += open(s).read()
    return txt


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_stream_kernels_spill_only_at_entry(stream_asm):
    txt = stream_asm
    seen = 0
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*\.amdhsa_kernel \1", txt, re.S | re.M):
        name, body = m.group(1), m.group(2).split("\n")
        if not any(k in name for k in STREAM_KERNELS): continue
        seen += 1
        first_loop = next((i for i, l in enumerate(body) if "in Loop:" in l), len(body))
        stores = [i for i, l in enumerate(body) if re.search(r"\b(scratch_store|buffer_store)\w*\b.*Spill", l)]
        assert all(i < first_loop for i in stores), f"{name}: a register is spilled inside the traversal loop (line {stores[-1]} of the kernel, loop from {first_loop})"
        size = re.search(rf"\.set {re.escape(name)}\.private_seg_size, (\d+)", txt)
        assert size and int(size.group(1)) <= 32, f"{name}: {size.group(1) if size else '?'} bytes of scratch"
    assert seen == 22, seen          # every instantiation of STREAM_KERNELS in STREAM_UNITS: a kernel that drops out of view fails here


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_shade_kernels_keep_their_scratch(stream_asm):
    """The shade kernels are compiled for six (k_shade_primary on the 8-wide layout: five) waves per SIMD and fit with a few registers to spare: shade.h records that 16-48 bytes of
    spills made the frame 4 % slower.  What they share with the device-buffer stages (scatter_math.h) is inlined into them, so the shape of a helper there decides their registers:
    k_shade_primary and k_shade hold everything in registers, k_shade_pack spills what it always has (12, 20, 20, 24 and 20 bytes over its five instantiations)."""
    seen = {"k_shade_primary": 0, "k_shade_pack": 0, "k_shade": 0}
    for m in re.finditer(r"\.set _ZN3mrt\d+_GLOBAL__N_1\d+(k_shade_primary|k_shade_pack|k_shade)I(\w+)\.private_seg_size, (\d+)", stream_asm):
        kernel, size = m.group(1), int(m.group(3))
        seen[kernel] += 1
        assert size <= (24 if kernel == "k_shade_pack" else 0), f"{kernel}<{m.group(2)[:24]}>: {size} bytes of scratch"
    assert seen["k_shade_primary"] >= 3 and seen["k_shade_pack"] >= 5 and seen["k_shade"] >= 5, seen
