"""Per-kernel comparison of two `hipcc --cuda-device-only -S` listings of one translation unit (or of the units it was split into, concatenated): is the instruction sequence identical, and the
instruction count, VGPR, AGPR, scratch bytes, LDS bytes and occupancy of both sides (A | B).  Comments and the __hip_cuid_* lines are dropped first.
Usage: hipcc $(CXXFLAGS) --offload-arch=gfx950 --cuda-device-only -S -o a.s x.hip   (at both commits);  python tools/isa_diff.py a.s b.s [--only-different]
Exit status 1 when a kernel exists on one side only or its resources differ; a different sequence with equal resources is reported, not an error."""
import re, subprocess, sys

def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        if "__hip_cuid_" in ln: continue
        m = re.match(r"\s+\.type\s+(\S+),@function", ln)
        if m: name, body = m.group(1), []; out[name] = {"body": body}; continue
        if name is None: continue
        m = re.match(r"; (NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", ln)
        if m: out[name][m.group(1)] = m.group(2); continue
        if ln.startswith(".Lfunc_end"): out[name]["done"] = True
        code = re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", ln.split(";")[0].strip())       # labels carry the function's index in its translation unit: a kernel that moved to another file keeps its code, not that index
        if code and not out[name].get("done"): body.append(code)
    return out

def demangle(names):
    dem = names
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try: dem = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]; break
        except Exception: pass
    return {n: re.sub(r"^void ", "", d.replace("mrt::(anonymous namespace)::", "")) for n, d in zip(names, dem)}

def count(body): return sum(1 for c in body if not c.startswith(".") and not c.endswith(":"))       # instructions: neither directives nor labels

a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
only_diff, bad = "--only-different" in sys.argv, 0
names = sorted(set(a) | set(b)); dem = demangle(names)
keys = ["NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy"]
print(f"{'kernel':100s} {'same':>5s} {'instr':>11s} {'vgpr':>9s} {'agpr':>7s} {'scratch':>9s} {'lds':>11s} {'occ':>5s}")
for n in names:
    ka, kb = a.get(n), b.get(n)
    if ka is None or kb is None: print(f"{dem[n][:100]:100s} only in {'B' if ka is None else 'A'}"); bad = 1; continue
    same = ka["body"] == kb["body"]
    if any(ka.get(k) != kb.get(k) for k in keys): bad = 1
    if same and only_diff: continue
    cols = [f"{count(ka['body'])}|{count(kb['body'])}"] + [f"{ka.get(k, '?')}|{kb.get(k, '?')}" for k in keys]
    print(f"{dem[n][:100]:100s} {'yes' if same else 'NO':>5s} {cols[0]:>11s} {cols[1]:>9s} {cols[2]:>7s} {cols[3]:>9s} {cols[4]:>11s} {cols[5]:>5s}")
sys.exit(bad)
