"""Rate of the surface entries on device buffers (DeviceScene.resolve_hits_device / interpolate_device) beside the query that feeds them — DESIGN.md §10h.
Per scene (DragonScene flattened; dragon4 two-level) and ray distribution (the coherent and incoherent rays of tools/query_rate.py: 2^22 built on the device, seed 1234):
  (a) the closest-hit query (intersect_closest_device);
  (b) resolve_hits_device on its result;
  (c) interpolate_device on its result at 3 and at 16 channels (random attributes, contiguous rows);
  (d) the byte floor of (b): 128 B per hit in and out (32 B ray + 32 B record + 64 B surface) at this box's device copy bandwidth — a 256 MiB torch copy, read + write counted,
      timed the same way (as tools/denoise_demo.py --time does).  The gathers of (b) — table row, shading record, three normals, three columns, a colour: 144 B per hit when
      nothing is shared — come on top of the floor.
Device time from HIP events on the stream, 3 warm + 20 timed repetitions, the calls alternating, median.
Usage: python tools/surface_rate.py [--rays 4194304] [--scenes dragon,dragon4]      (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--scenes", default="dragon,dragon4")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import metal_raytracing_amd as m
    from query_rate import coherent_rays, incoherent_rays, scene_box
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

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    copy_ms = timed([lambda: dst.copy_(src)])[0]
    copy_gbs = 2 * src.numel() / copy_ms / 1e6                     # read + write
    res["copy_256MiB_ms"] = copy_ms; res["copy_GBps"] = copy_gbs
    del src, dst
    for name in a.scenes.split(","):
        two_level = name == "dragon4"
        sc = m.SCENES[name]((1920, 1080))
        ds = m.DeviceScene(ctx, sc, {"instancing": 1} if two_level else None)
        lo, hi = scene_box(m, sc)
        eye = [sc.camera.position.x, sc.camera.position.y, sc.camera.position.z]
        V = int(ds.vertex_offsets()[-1])
        g = torch.Generator(device=dev); g.manual_seed(1234)
        attr3 = torch.randn((V, 3), generator=g, device=dev); attr16 = torch.randn((V, 16), generator=g, device=dev)
        row = {"triangles": int(ds.stats.triangles), "vertices": V, "instancing": int(two_level)}
        for dist, rays in (("coherent", coherent_rays(torch, dev, a.rays, sc.camera)), ("incoherent", incoherent_rays(torch, dev, a.rays, lo, hi, eye, 1234))):
            hits = torch.empty((a.rays, 8), dtype=torch.int32, device=dev); surf = torch.empty((a.rays, 16), dtype=torch.float32, device=dev)
            o3 = torch.empty((a.rays, 3), dtype=torch.float32, device=dev); o16 = torch.empty((a.rays, 16), dtype=torch.float32, device=dev)
            s = ts.cuda_stream
            ds.intersect_closest_device(rays, out=hits, stream=0); ds.resolve_hits_device(rays, hits, out=surf, stream=0)          # (the first call makes the table)
            torch.cuda.synchronize()
            t = timed([lambda: ds.intersect_closest_device(rays, out=hits, stream=s), lambda: ds.resolve_hits_device(rays, hits, out=surf, stream=s),
                       lambda: ds.interpolate_device(hits, attr3, out=o3, stream=s), lambda: ds.interpolate_device(hits, attr16, out=o16, stream=s)])
            floor_ms = 128.0 * a.rays / copy_gbs / 1e6
            mr = lambda ms: a.rays / ms / 1e3
            row[dist] = {"hit_share": float((hits[:, 0] == 1).float().mean()),
                         "a_query_ms": t[0], "b_resolve_ms": t[1], "c_interpolate3_ms": t[2], "c_interpolate16_ms": t[3], "d_floor_ms": floor_ms,
                         "a_Mrays": mr(t[0]), "b_Mhits": mr(t[1]), "c3_Mhits": mr(t[2]), "c16_Mhits": mr(t[3]), "b_over_floor": t[1] / floor_ms, "b_over_a": t[1] / t[0]}
        res["scenes"][name] = row
        ds.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
