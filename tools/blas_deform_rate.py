"""One step of "new vertices -> BLAS refit -> 2^20 closest-hit queries" on InstancedDragonScene as a TWO-LEVEL scene (instancing = 1: one dragon BLAS shared by four
instances), two ways:
  (a) on ONE stream, nothing of the host in between: a torch expression displaces the dragon along its normals on the device, DeviceScene.update_blas_device +
      refit_blas_device + intersect_closest_device follow it on the same stream; HIP events around the step, on that stream;
  (b) the path there was before: the same torch expression, .cpu(), DeviceScene.update_mesh + commit (refit_two_level), then the same device query; wall time, the stream
      drained at both ends.
Both in this process on this device, alternating; 3 warm + 20 timed steps each, median and fastest.  (b) on the same box is the yardstick: there is no bar.
It also prints how many kernels one refit_blas_device launches for this scene (counted from the resident layout: the levels of the BLAS and of both TLAS forms).
With --parent-lib it also runs bench.py --gpus 1 --steps 20 --warmup 5 on this tree's library and on that one (a build of the parent commit), alternating, to show that the
render path has not moved.
Usage: python tools/blas_deform_rate.py [--rays 1048576] [--reps 20] [--parent-lib PATH] [--bench-rounds 3]      (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deform_rate import bench_ab  # noqa: E402


def refit_launches(ds, mesh_id):
    """kernels of one refit_blas_device after one update of mesh_id: k_flatten, the 8-wide packets, one launch per level of the BLAS, the rope packets, the rope nodes'
    prepare and refit, the fold, the instances' boxes (7 + the BLAS's levels: enqueue_refit and device_refit_blas of bvh_refit.hip, restated here and to be kept in step with
    them); then one launch per depth of the rope TLAS and per level of the 8-wide TLAS (device_refit_instances).  Kernels only: the two hipMemsetAsync per BLAS are not counted."""
    import numpy as np
    wn, inst, hdr = ds.read_layout("wnodes"), ds.read_layout("instances"), ds.read_layout("header")
    root = int(inst[mesh_id, 19])          # InstanceDev::wroot
    pop = np.array([bin(i).count("1") for i in range(256)], np.int64)
    levels, frontier = 0, np.array([root], np.int64)
    while len(frontier):          # breadth first: the internal children of node i are child_base .. child_base + popcount(imask) - 1
        levels += 1
        cnt = pop[wn[frontier, 3] >> 24]
        base = wn[frontier, 4].astype(np.int64)
        frontier = np.repeat(base, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    tlas_wide = int(hdr[3]) - 1 - int(hdr[5])
    tlas_rope = int(ds.stats.max_depth)
    return {"blas_levels": levels, "tlas_rope_depths": tlas_rope, "tlas_wide_levels": tlas_wide, "update": 2, "refit": 7 + levels + tlas_rope + tlas_wide}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--amplitude", type=float, default=0.01)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    a = ap.parse_args()
    result = {"tool": "blas_deform_rate", "rays": a.rays, "reps": a.reps}
    if a.parent_lib:          # first, in child processes of a parent that has not opened the GPU yet
        result["bench"] = bench_ab(os.path.abspath(a.parent_lib), a.bench_rounds)

    import numpy as np
    import torch
    import metal_raytracing_amd as m
    from test_fuzz_geometry import _rays

    size = (1920, 1080)
    sc = m.InstancedDragonScene(size)
    meshes = m.flatten_scene(sc, share=True)
    big = [k for k, e in enumerate(meshes) if e[4] < 0 and len(e[0]) > 100000]
    assert len(big) == 1
    dragon = big[0]
    copies = 1 + sum(1 for e in meshes if e[4] == dragon)
    ctx = m.Context(0)
    dev = torch.device("cuda", ctx.device)
    two = {"instancing": 1}
    dsa, dsb = m.DeviceScene(ctx, sc, two), m.DeviceScene(ctx, sc, two)          # (a) and (b) each deform a scene of their own
    base_p = torch.from_numpy(np.ascontiguousarray(meshes[dragon][0], np.float32)).to(dev)
    base_n = torch.from_numpy(np.ascontiguousarray(meshes[dragon][1], np.float32)).to(dev)
    rays = _rays(np.random.default_rng(11), a.rays)
    rays[:, 0:3] = rays[:, 0:3] * 0.5 + np.array([0.3, 0.2, 2.0], np.float32)          # towards the dragons
    d_rays = torch.from_numpy(rays).to(dev)
    out = torch.empty((a.rays, 8), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    result.update(device=ctx.device_name, triangles=int(dsa.stats.triangles), instances=int(dsa.stats.instances), dragon_instances=copies, dragon_vertices=int(base_p.shape[0]),
                  build_ms=dsa.stats.build_ms, launches=refit_launches(dsa, dragon))

    def displaced(step):
        """the dragon pushed along its normals by a wave that moves with the step: a torch expression, on the current stream"""
        w = a.amplitude * torch.sin(9.0 * base_p[:, 1:2] + 0.37 * step) * torch.cos(7.0 * base_p[:, 0:1] - 0.21 * step)
        return base_p + base_n * w

    ta, tb, parts, hits = [], [], [], []
    e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
    for step in range(a.warm + a.reps):
        with torch.cuda.stream(stream):
            # (a): everything on the stream
            e0.record(stream)
            p = displaced(step)
            e1.record(stream)
            dsa.update_blas_device(dragon, p, base_n)
            dsa.refit_blas_device()
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
            hits.append(hits_a)
    med = statistics.median
    sa, sb = dsa.stats, dsb.stats
    result.update(a_stream_ms=med(ta), b_host_ms=med(tb), b_over_a=med(tb) / med(ta), a_min_ms=min(ta), b_min_ms=min(tb),
                  a_parts_ms={"displace": med([x[0] for x in parts]), "update_and_refit": med([x[1] for x in parts]), "query": med([x[2] for x in parts])},
                  hits_per_step=hits, refits=(dsa.refits, dsb.refits), rejected=dsa.device_updates_rejected,
                  stats_a={"refit_ms": sa.build_ms, "wide_cost": sa.wide_cost, "sah_cost": sa.sah_cost, "leaf_growth": sa.leaf_growth},
                  stats_b={"refit_ms": sb.build_ms, "wide_cost": sb.wide_cost, "sah_cost": sb.sah_cost, "leaf_growth": sb.leaf_growth})
    dsa.close(); dsb.close(); ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
