"""One step of "new poses -> TLAS refit -> 2^20 closest-hit queries" on two-level scenes (scene option instancing = 1), two ways:
  (a) on ONE stream, nothing of the host in between: a torch expression makes the poses on the device, DeviceScene.set_instance_transforms_device +
      refit_instances_device + intersect_closest_device follow it on the same stream; HIP events around the step, on that stream;
  (b) the path there was before: the same torch expression, .cpu(), DeviceScene.set_instance_transform per instance + commit, then the same device query; wall time,
      the stream drained at both ends.
Both in this process on this device, alternating; 3 warm + 20 timed steps each, median.  (b) on the same box is the yardstick: there is no bar.
  (c) as (a) with DeviceScene.rebuild_tlas_device in place of the refit: the topology of both TLAS forms rebuilt on the stream at every step.
Then the price of the kept topology: the movers trade places end for end (the first with the last, ...), (a) refits the tree it has, (b) commits, (c) rebuilds on the
device, and the same queries are timed on the three trees.
Scenes: dragon4 (DragonScene with the dragon four times: 1 BLAS x 4 instances beside the scene's other meshes) and a plane under 64 and under 1 024 small spheres.
Usage: python tools/instance_rate.py [--rays 1048576] [--reps 20] [--scenes dragon4,64,1024]      (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def swarm(m, size, n):
    import numpy as np
    rng = np.random.default_rng(n)

    class S(m.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [m.Model(name="plane", position=[0, 0, 0], scale=10)]
            for _ in range(n):
                self.models.append(m.Model(name="sphere", position=[float(rng.uniform(-2.5, 2.5)), float(rng.uniform(0.1, 2.0)), float(rng.uniform(-2.0, 2.0))],
                                           rotation=[float(x) for x in rng.uniform(-3, 3, 3)], scale=float(rng.uniform(0.4, 1.2)) * (8.0 / n) ** (1.0 / 3.0)))
    return S(size)


def run(m, ctx, name, a):
    import numpy as np
    import torch
    from test_fuzz_geometry import _rays

    size = (1920, 1080)
    sc = m.InstancedDragonScene(size, copies=4) if name == "dragon4" else swarm(m, size, int(name))
    meshes = m.flatten_scene(sc, share=True)
    I = len(meshes)
    if name == "dragon4":
        movers = [k for k, e in enumerate(meshes) if len(e[0]) > 100000 or (e[4] >= 0 and len(meshes[e[4]][0]) > 100000)]
        assert len(movers) == 4
    else:
        movers = list(range(1, I))
    dev = torch.device("cuda", ctx.device)
    dsa, dsb, dsc = (m.DeviceScene(ctx, sc, {"instancing": 1}) for _ in range(3))          # (a), (b) and (c) each move a scene of their own
    base = torch.from_numpy(np.stack([np.asarray(e[2], np.float32).reshape(16) for e in meshes])).to(dev)
    mask = torch.zeros((I, 1), device=dev); mask[movers] = 1.0
    phase = torch.arange(I, device=dev, dtype=torch.float32).reshape(I, 1)
    rays = _rays(np.random.default_rng(11), a.rays)
    d_rays = torch.from_numpy(rays).to(dev)
    out = torch.empty((a.rays, 8), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)

    def poses(step):
        """the movers on small orbits about their places: a torch expression, on the current stream"""
        x = base.clone()
        x[:, 12:15] += a.amplitude * mask * torch.cat([torch.sin(0.37 * step + phase), 0.3 * (1.0 + torch.sin(0.21 * step + 2.0 * phase)), torch.cos(0.37 * step + phase)], 1)
        return x

    def host_move(ds, x):
        h = x.cpu().numpy()
        for k in movers: ds.set_instance_transform(k, h[k])
        ds.commit()

    ta, tb, parts, tc, tcommit = [], [], [], [], []
    e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
    hits = 0
    with torch.cuda.stream(stream):
        for step in range(a.warm + a.reps):
            # (a): everything on the stream
            e0.record(stream)
            x = poses(step)
            e1.record(stream)
            dsa.set_instance_transforms_device(0, x)
            dsa.refit_instances_device()
            e2.record(stream)
            dsa.intersect_closest_device(d_rays, out=out)
            e3.record(stream)
            stream.synchronize()
            hits_a = int((out[:, 0] == 1).sum())
            if step >= a.warm:
                ta.append(e0.elapsed_time(e3)); parts.append((e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
            # (c): as (a), the TLAS rebuilt instead of refitted
            e0.record(stream)
            x = poses(step)
            e1.record(stream)
            dsc.set_instance_transforms_device(0, x)
            dsc.rebuild_tlas_device()
            e2.record(stream)
            dsc.intersect_closest_device(d_rays, out=out)
            e3.record(stream)
            stream.synchronize()
            hits_c = int((out[:, 0] == 1).sum())
            if step >= a.warm: tc.append((e1.elapsed_time(e2), e2.elapsed_time(e3)))
            # (b): through the host
            stream.synchronize()
            t0 = time.perf_counter()
            host_move(dsb, poses(step))
            stream.synchronize()
            t1 = time.perf_counter()
            dsb.intersect_closest_device(d_rays, out=out)
            stream.synchronize()
            if step >= a.warm:
                tb.append((time.perf_counter() - t0) * 1e3); tcommit.append((t1 - t0) * 1e3)
            hits = int((out[:, 0] == 1).sum())
            assert hits_a == hits and hits_c == hits, (hits_a, hits_c, hits)
        # the kept topology at its worst: the movers trade places end for end; (a) refits the tree it has, (b) builds one for the new places
        x = poses(0)
        idx = torch.tensor(movers, device=dev)
        x[idx, 12:15] = x[idx.flip(0), 12:15]
        dsa.set_instance_transforms_device(0, x); dsa.refit_instances_device()
        dsc.set_instance_transforms_device(0, x); dsc.rebuild_tlas_device()
        host_move(dsb, x)
        q = {"refit": [], "rebuild": [], "rebuild_device": []}
        for rep in range(a.warm + a.reps):
            for which, ds in (("refit", dsa), ("rebuild", dsb), ("rebuild_device", dsc)):
                e0.record(stream)
                ds.intersect_closest_device(d_rays, out=out)
                e1.record(stream)
                stream.synchronize()
                if rep >= a.warm: q[which].append(e0.elapsed_time(e1))
    med = statistics.median
    res = {"instances": I, "movers": len(movers), "triangles": int(dsa.stats.triangles), "tlas_nodes": int(dsa.stats.bvh_nodes),
           "a_stream_ms": med(ta), "b_host_ms": med(tb), "b_over_a": med(tb) / med(ta), "a_min_ms": min(ta), "b_min_ms": min(tb),
           "a_parts_ms": {"poses": med([p[0] for p in parts]), "set_and_refit": med([p[1] for p in parts]), "query": med([p[2] for p in parts])},
           "hits": hits, "rejected": dsa.device_updates_rejected,
           "c_set_and_rebuild_ms": med([p[0] for p in tc]), "c_query_ms": med([p[1] for p in tc]), "b_commit_step_ms": med(tcommit),
           "swapped_query_ms": {k: med(v) for k, v in q.items()}, "refit_over_rebuild_rate": med(q["rebuild"]) / med(q["refit"]),
           "device_rebuild_over_rebuild_rate": med(q["rebuild"]) / med(q["rebuild_device"])}
    dsa.close(); dsb.close(); dsc.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--amplitude", type=float, default=0.2)
    ap.add_argument("--scenes", default="dragon4,64,1024")
    a = ap.parse_args()
    import metal_raytracing_amd as m
    ctx = m.Context(0)
    result = {"tool": "instance_rate", "rays": a.rays, "reps": a.reps, "device": ctx.device_name, "scenes": {}}
    for name in a.scenes.split(","):
        result["scenes"][name] = run(m, ctx, name, a)
        print(f"{name}: {result['scenes'][name]}", file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
