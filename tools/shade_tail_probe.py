"""Times of the shade launches of serialised 8-frame passes (DragonScene 1920x1080, one stream, tile_groups = 1: the regime of bench.py's
kernel_ms_serialised_pass), per launch.  Needs the probe build (tools/build_variant.sh tails "-DMRT_PROBE_SHADE_TAILS", selected with MRT_LIB_PATH) for the per-launch
lines: MRT_PROBE_LOG=1 makes the library print every timed launch in enqueue order, MRT_PROBE_TAILS=<mask of bounces> makes those bounces' shade launches reserve on
eight words instead of one (images are garbage then, and the stages behind a probed launch see empty queues: read only the probed launch's time).
With the release library only the per-class sums of Renderer.kernel_times are printed."""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = """
import sys; sys.path.insert(0, %r)
import metal_raytracing_amd as mrt
w, h = 1920, 1080
r = mrt.Renderer((w, h), mrt.DragonScene((w, h)), seed=1)
r.set_option("frames_in_flight", 1); r.set_option("frame_batch", 8); r.set_option("tile_groups", 1)
r.draw(16, wait=True)
print("probe_begin", file=sys.stderr, flush=True)
tot = {}
for _ in range(5):
    r.draw(16, wait=True)
    for k, (ms, n) in r.kernel_times.items():
        if n: t = tot.setdefault(k, [0.0, 0]); t[0] += ms; t[1] += n
print("classes", {k: (round(ms / n, 4), n) for k, (ms, n) in tot.items()}, flush=True)
r.close()
""" % ROOT
p = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=240)
sys.stdout.write(p.stdout)
if p.returncode: sys.stdout.write(p.stderr[-2000:]); sys.exit(p.returncode)
err = p.stderr.split("probe_begin", 1)[-1]
rows = [(int(m.group(1)), int(m.group(2)), float(m.group(3))) for m in re.finditer(r"probe_launch (\d+) kind (\d+) ms ([0-9.]+)", err)]
# a pass enqueues shade(0), trace(0), shade(1), trace(1), shade(2), trace(2), accumulate: the n-th shade launch of a draw is bounce n % 3
per = {0: [], 1: [], 2: []}
draw_shades = 0; last_k = -1
for k, kind, ms in rows:
    if k < last_k: draw_shades = 0
    last_k = k
    if kind == 1: per[draw_shades % 3].append(ms); draw_shades += 1
for b, v in per.items():
    if v: v.sort(); print(f"shade({b}): launches {len(v)} mean {sum(v) / len(v):.4f} median {v[len(v) // 2]:.4f} min {v[0]:.4f} max {v[-1]:.4f} ms", flush=True)
