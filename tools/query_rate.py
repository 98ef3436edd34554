"""Rate of the stream-ordered ray queries on device buffers (DeviceScene.intersect_closest_device / intersect_any_device) — DESIGN.md §10c.
Per scene (DragonScene flattened; dragon4 two-level) and ray distribution (incoherent: tests/test_fuzz_geometry.py::_rays scaled to the scene's box; coherent: the camera's
primary rays through pixel centres), 2^22 rays built on the device with torch from a fixed seed:
  (a) the entry on rays with min_distance = 0: the 8-wide stream walk;
  (b) the entry on a copy whose rays all have min_distance = 1e-30: the whole batch takes the one-ray-per-lane walk of the host entries;
  (c) the wall time of the host entry (host arrays in and out) for the same rays.
(a) and (b) alternate in one process; device time from HIP events on the stream, 3 warm + 20 timed repetitions, median.
All-hits leg (DeviceScene.intersect_all_device; flattened scenes), the forms alternating in one process the same way:
  (1) all-hits with K = 1 against (b) on the min_distance = 1e-30 rays: the same walk with one candidate in registers — what the list costs when it is not needed;
  (2) all-hits with K = 4 and K = 8 against K successive intersect_closest_device calls, each with min_distance one float past the previous distance (torch ops on
      the same stream in between, no compaction: a ray that has missed walks and misses again) — what a caller does without the entry, and it loses ties;
  (3) all-hits with K = 1 against (a) on the min_distance = 0 rays: what the missing lane refill costs.
Masked leg (mask= of the three methods), the forms alternating in one process the same way; the unmasked entry in the same job is the yardstick:
  (i)  flattened scenes: closest and any with every mask all-ones against (b) on the min_distance = 1e-30 rays — the like-for-like one-ray-per-lane walk: what the filter
       costs — and against (a) on the min_distance = 0 rays: what the missing lane refill costs; all-hits K = 4 masked against unmasked;
  (ii) two-level scenes (dragon x 4): dragon j carries the bit 1 << j, every other mesh the bit 0x10; a ray mask that sees ONE dragon of the four (0x11) against one that
       sees all four (0x1F) against the unmasked entry in both of its forms — are skipped instances nearly free?
Usage: python tools/query_rate.py [--rays 4194304] [--scenes dragon,dragon4] [--legs queries,all_hits,masked]      (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene_box(m, sc):
    """the box that holds the bulk of the scene: 2nd .. 98th percentile of the world-space vertices per axis (the ground planes' four corners do not set it)"""
    import numpy as np
    pts = []
    for pos, _, xf, _ in m.flatten_scene(sc):
        M = np.asarray(xf, np.float64).reshape(4, 4)          # [col][row]
        pts.append(np.asarray(pos, np.float64) @ M[:3, :3] + M[3, :3])
    p = np.concatenate(pts)
    return np.percentile(p, 2, axis=0), np.percentile(p, 98, axis=0)


def incoherent_rays(torch, dev, n, lo, hi, eye, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32, device=dev), torch.tensor(hi, dtype=torch.float32, device=dev)
    o = torch.tensor(eye, dtype=torch.float32, device=dev) + torch.randn((n, 3), generator=g, device=dev) * (0.14 * float((hi - lo).max()))
    t = lo_t + torch.rand((n, 3), generator=g, device=dev) * (hi_t - lo_t)
    d = t - o; d = d / d.norm(dim=1, keepdim=True)
    r = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    r[:, 0:3] = o; r[:, 4:7] = d; r[:, 7] = float("inf")
    return r


def coherent_rays(torch, dev, n, cam):
    side = int(round(n ** 0.5))
    assert side * side == n, "--rays must be a square number for the camera grid"
    v = lambda f: torch.tensor([f.x, f.y, f.z], dtype=torch.float32, device=dev)
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 2.0 - 1.0
    uy, ux = torch.meshgrid(u, u, indexing="ij")
    d = ux.reshape(-1, 1) * v(cam.right) + uy.reshape(-1, 1) * v(cam.up) + v(cam.forward)
    d = d / d.norm(dim=1, keepdim=True)
    r = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    r[:, 0:3] = v(cam.position); r[:, 4:7] = d; r[:, 7] = float("inf")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--scenes", default="dragon,dragon4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--legs", default="queries,all_hits,masked")
    a = ap.parse_args()
    import torch
    import metal_raytracing_amd as m
    ctx = m.Context(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(dev)
    res = {"device": ctx.device_name, "rays": a.rays, "reps": a.reps, "scenes": {}}

    def timed(fns):
        """the callables in turn, reps times over; median device ms of each"""
        ms = [[] for _ in fns]
        with torch.cuda.stream(ts):
            for rep in range(3 + a.reps):
                for k, fn in enumerate(fns):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ts); fn(); e1.record(ts); ts.synchronize()
                    if rep >= 3: ms[k].append(e0.elapsed_time(e1))
        return [statistics.median(x) for x in ms]

    legs = set(a.legs.split(","))
    for name in a.scenes.split(","):
        two_level = name == "dragon4"
        sc = m.SCENES[name]((1920, 1080))
        ds = m.DeviceScene(ctx, sc, {"instancing": 1} if two_level else None)
        lo, hi = scene_box(m, sc)
        eye = [sc.camera.position.x, sc.camera.position.y, sc.camera.position.z]
        row = {"triangles": int(ds.stats.triangles), "instancing": int(two_level), "box": [lo.tolist(), hi.tolist()]}
        for dist, rays in (("incoherent", incoherent_rays(torch, dev, a.rays, lo, hi, eye, 1234)), ("coherent", coherent_rays(torch, dev, a.rays, sc.camera))):
            lane = rays.clone(); lane[:, 3] = 1e-30
            oc = torch.empty((a.rays, 8), dtype=torch.int32, device=dev); oa = torch.empty((a.rays,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            s = ts.cuda_stream
            mr = lambda ms: a.rays / ms / 1e3
            row[dist] = {}
            if "masked" in legs:
                ALL = 0xFFFFFFFF
                if two_level:
                    names = [mo.name for mo in sc.models for _ in mo.meshes]
                    dragons = [i for i, nm in enumerate(names) if nm == "dragon"]
                    masks = [0x10] * len(names)
                    for j, i in enumerate(dragons): masks[i] = 1 << j
                    ds.set_mesh_masks(masks)
                    one, four = 0x11, 0x10 | ((1 << len(dragons)) - 1)
                    v = timed([lambda: ds.intersect_closest_device(rays, out=oc, stream=s), lambda: ds.intersect_closest_device(lane, out=oc, stream=s),
                               lambda: ds.intersect_closest_device(rays, out=oc, stream=s, mask=four), lambda: ds.intersect_closest_device(rays, out=oc, stream=s, mask=one),
                               lambda: ds.intersect_any_device(lane, out=oa, stream=s), lambda: ds.intersect_any_device(rays, out=oa, stream=s, mask=four),
                               lambda: ds.intersect_any_device(rays, out=oa, stream=s, mask=one)])
                    row[dist]["masked"] = {"dragons": len(dragons), "closest_a_stream_ms": v[0], "closest_b_lane_ms": v[1], "closest_sees_four_ms": v[2], "closest_sees_one_ms": v[3],
                                           "four_over_b": v[2] / v[1], "one_over_four": v[3] / v[2], "any_b_lane_ms": v[4], "any_sees_four_ms": v[5], "any_sees_one_ms": v[6],
                                           "any_one_over_four": v[6] / v[5], "sees_four_Mrays": mr(v[2]), "sees_one_Mrays": mr(v[3])}
                    ds.set_mesh_masks([ALL] * len(names))
                else:
                    cnt = torch.empty((a.rays,), dtype=torch.int32, device=dev); o4 = torch.empty((a.rays, 4, 8), dtype=torch.int32, device=dev)
                    v = timed([lambda: ds.intersect_closest_device(lane, out=oc, stream=s), lambda: ds.intersect_closest_device(lane, out=oc, stream=s, mask=ALL),
                               lambda: ds.intersect_closest_device(rays, out=oc, stream=s), lambda: ds.intersect_closest_device(rays, out=oc, stream=s, mask=ALL),
                               lambda: ds.intersect_any_device(lane, out=oa, stream=s), lambda: ds.intersect_any_device(lane, out=oa, stream=s, mask=ALL),
                               lambda: ds.intersect_all_device(rays, 4, out=o4, counts_out=cnt, stream=s), lambda: ds.intersect_all_device(rays, 4, out=o4, counts_out=cnt, stream=s, mask=ALL)])
                    row[dist]["masked"] = {"closest_b_lane_ms": v[0], "closest_masked_lane_ms": v[1], "masked_over_b": v[1] / v[0], "closest_a_stream_ms": v[2], "closest_masked_ms": v[3],
                                           "masked_over_a": v[3] / v[2], "any_b_lane_ms": v[4], "any_masked_lane_ms": v[5], "any_masked_over_b": v[5] / v[4],
                                           "all4_ms": v[6], "all4_masked_ms": v[7], "all4_masked_over_all4": v[7] / v[6], "closest_masked_Mrays": mr(v[3])}
                    del o4, cnt
            if not legs & {"queries", "all_hits"}: continue
            t = timed([lambda: ds.intersect_closest_device(rays, out=oc, stream=s), lambda: ds.intersect_closest_device(lane, out=oc, stream=s),
                       lambda: ds.intersect_any_device(rays, out=oa, stream=s), lambda: ds.intersect_any_device(lane, out=oa, stream=s)])
            hit_share = float((oc[:, 0] == 1).float().mean())
            h = rays.cpu().numpy()
            wall = []
            for fn in (ds.intersect_closest, ds.intersect_any):
                fn(h[:4096])
                t0 = time.perf_counter(); fn(h); wall.append((time.perf_counter() - t0) * 1e3)
            if not two_level and "all_hits" in legs:
                cnt = torch.empty((a.rays,), dtype=torch.int32, device=dev)
                outs = {K: torch.empty((a.rays, K, 8), dtype=torch.int32, device=dev) for K in (1, 4, 8)}
                work = rays.clone()

                def successive(K):
                    work.copy_(rays)
                    for k in range(K):
                        ds.intersect_closest_device(work, out=oc, stream=s)
                        if k + 1 < K:          # one float past the hit; a ray that missed keeps its window
                            work[:, 3] = torch.where(oc[:, 0] == 1, (oc[:, 1] + 1).view(torch.float32), work[:, 3])
                torch.cuda.synchronize()
                u = timed([lambda: ds.intersect_closest_device(lane, out=oc, stream=s), lambda: ds.intersect_all_device(lane, 1, out=outs[1], counts_out=cnt, stream=s),
                           lambda: ds.intersect_closest_device(rays, out=oc, stream=s), lambda: ds.intersect_all_device(rays, 1, out=outs[1], counts_out=cnt, stream=s),
                           lambda: ds.intersect_all_device(rays, 4, out=outs[4], counts_out=cnt, stream=s), lambda: successive(4),
                           lambda: ds.intersect_all_device(rays, 8, out=outs[8], counts_out=cnt, stream=s), lambda: successive(8)])
                mean_hits = float(cnt.float().mean())          # of the K = 8 call
                all_hits = {"b_lane_ms": u[0], "all1_lane_ms": u[1], "all1_over_b": u[1] / u[0], "a_stream_ms": u[2], "all1_ms": u[3], "all1_over_a": u[3] / u[2],
                            "all4_ms": u[4], "closest_x4_ms": u[5], "x4_over_all4": u[5] / u[4], "all8_ms": u[6], "closest_x8_ms": u[7], "x8_over_all8": u[7] / u[6],
                            "all1_Mrays": mr(u[3]), "all4_Mrays": mr(u[4]), "all8_Mrays": mr(u[6]), "mean_hits_at_8": mean_hits}
                del outs, work
            row[dist].update({"hit_share": hit_share,
                         "closest": {"a_stream_ms": t[0], "b_lane_ms": t[1], "c_host_wall_ms": wall[0], "a_Mrays": mr(t[0]), "b_Mrays": mr(t[1]), "c_Mrays": mr(wall[0]), "a_over_b": t[1] / t[0], "a_over_c": wall[0] / t[0]},
                         **({} if two_level or "all_hits" not in legs else {"all_hits": all_hits}),
                         "any": {"a_stream_ms": t[2], "b_lane_ms": t[3], "c_host_wall_ms": wall[1], "a_Mrays": mr(t[2]), "b_Mrays": mr(t[3]), "c_Mrays": mr(wall[1]), "a_over_b": t[3] / t[2], "a_over_c": wall[1] / t[2]}})
        res["scenes"][name] = row
        ds.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
