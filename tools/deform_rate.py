"""One step of "new vertices -> refit -> 2^20 closest-hit queries" on DragonScene, two ways:
  (a) on ONE stream, nothing of the host in between: a torch expression displaces the dragon along its normals on the device, DeviceScene.update_mesh_device +
      refit_device + intersect_closest_device follow it on the same stream; HIP events around the step, on that stream;
  (b) the path there was before: the same torch expression, .cpu(), DeviceScene.update_mesh + commit, then the same device query; wall time, the stream drained at both ends.
Both in this process on this device, alternating; 3 warm + 20 timed steps each, median.  (b) on the same box is the yardstick: there is no bar.
With --parent-lib it also runs bench.py --gpus 1 --steps 20 --warmup 5 on this tree's library and on that one (a build of the parent commit, e.g. from
tools/build_variant.sh in a checkout of it), alternating, to show that the render path has not moved.
Usage: python tools/deform_rate.py [--rays 1048576] [--reps 20] [--parent-lib PATH] [--bench-rounds 3]      (prints one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_ab(parent_lib, rounds):
    """bench.py on this tree's library and on the parent's, alternating; the 'value' of each JSON line"""
    out = {"this": [], "parent": []}
    for _ in range(rounds):
        for which in ("this", "parent"):
            env = dict(os.environ)
            if which == "parent":
                env["MRT_LIB_PATH"] = parent_lib
            else:
                env.pop("MRT_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"bench.py ({which}) failed: {p.stderr[-1000:]}")
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            r = json.loads(line)
            out[which].append(r.get("value", r.get("primary")))
            print(f"bench.py {which}: {out[which][-1]}", file=sys.stderr, flush=True)
    res = {k: {"runs": v, "median": statistics.median(v)} for k, v in out.items()}
    res["this_over_parent"] = res["this"]["median"] / res["parent"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--amplitude", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    result = {"tool": "deform_rate", "rays": a.rays, "reps": a.reps}
    if a.parent_lib:          # first, in child processes of a parent that has not opened the GPU yet
        result["bench"] = bench_ab(os.path.abspath(a.parent_lib), a.bench_rounds)

    import numpy as np
    import torch
    import metal_raytracing_amd as m
    from test_fuzz_geometry import _rays

    size = (1920, 1080)
    sc = m.DragonScene(size)
    meshes = m.flatten_scene(sc, share=True)
    big = [k for k, e in enumerate(meshes) if len(e[0]) > 100000]
    assert len(big) == 1
    dragon = big[0]
    ctx = m.Context(0)
    dev = torch.device("cuda", ctx.device)
    dsa, dsb = m.DeviceScene(ctx, sc), m.DeviceScene(ctx, sc)          # (a) and (b) each deform a scene of their own
    base_p = torch.from_numpy(np.ascontiguousarray(meshes[dragon][0], np.float32)).to(dev)
    base_n = torch.from_numpy(np.ascontiguousarray(meshes[dragon][1], np.float32)).to(dev)
    rays = _rays(np.random.default_rng(11), a.rays)
    rays[:, 0:3] = rays[:, 0:3] * 0.5 + np.array([0.3, 0.2, 2.0], np.float32)          # towards the dragon
    d_rays = torch.from_numpy(rays).to(dev)
    out = torch.empty((a.rays, 8), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    result.update(device=ctx.device_name, triangles=int(dsa.stats.triangles), dragon_vertices=int(base_p.shape[0]), build_ms=dsa.stats.build_ms)

    def displaced(step):
        """the dragon pushed along its normals by a wave that moves with the step: a torch expression, on the current stream"""
        w = a.amplitude * torch.sin(9.0 * base_p[:, 1:2] + 0.37 * step) * torch.cos(7.0 * base_p[:, 0:1] - 0.21 * step)
        return base_p + base_n * w

    ta, tb, parts = [], [], []
    e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
    for step in range(a.warm + a.reps):
        with torch.cuda.stream(stream):
            # (a): everything on the stream
            e0.record(stream)
            p = displaced(step)
            e1.record(stream)
            dsa.update_mesh_device(dragon, p, base_n)
            dsa.refit_device()
            e2.record(stream)
            dsa.intersect_closest_device(d_rays, out=out)
            e3.record(stream)
            stream.synchronize()
            hits_a = int((out[:, 0] == 1).sum())
            if step >= a.warm:
                ta.append(e0.elapsed_time(e3)); parts.append((e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
            # (b): through the host
            stream.synchronize()
            t0 = time.perf_counter()
            p = displaced(step)
            hp = p.cpu().numpy()
            dsb.update_mesh(dragon, hp, meshes[dragon][1])
            dsb.commit()
            dsb.intersect_closest_device(d_rays, out=out)
            stream.synchronize()
            if step >= a.warm:
                tb.append((time.perf_counter() - t0) * 1e3)
            hits_b = int((out[:, 0] == 1).sum())
            assert hits_a == hits_b, (hits_a, hits_b)
    med = statistics.median
    result.update(a_stream_ms=med(ta), b_host_ms=med(tb), b_over_a=med(tb) / med(ta), a_min_ms=min(ta), b_min_ms=min(tb),
                  a_parts_ms={"displace": med([x[0] for x in parts]), "update_and_refit": med([x[1] for x in parts]), "query": med([x[2] for x in parts])},
                  hits=hits_a, refits=(dsa.refits, dsb.refits), rejected=dsa.device_updates_rejected,
                  stats_a={"refit_ms": dsa.stats.build_ms, "wide_cost": dsa.stats.wide_cost, "leaf_growth": dsa.stats.leaf_growth},
                  stats_b={"refit_ms": dsb.stats.build_ms, "wide_cost": dsb.stats.wide_cost, "leaf_growth": dsb.stats.leaf_growth})
    dsa.close(); dsb.close(); ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
