"""Rate of the variance-guided a-trous filter and of the moments beside it (DeviceScene.moments_sample_device / reproject_device / denoise_variance_device) — DESIGN.md §10t.
One scene (DragonScene flattened by default) at 1920 x 1080, HIP events on a side stream, the legs of a group alternating in one loop, 3 warm + 20 timed, medians (and the
spread min .. max of each leg):
  (a) a 256 MiB device-to-device torch copy, read + write counted: the byte rate every floor below is taken at, as tools/integrator_rate.py defines it;
  (b) moments_sample_device against its byte floor: 48 B per pixel (two 16-byte loads, one 16-byte store);
  (c) reproject_device of a still world on the colour, the same call on the moments (moments_sample_device's image as the sample, the moments as the history) — the price
      of not fusing the two —, and both one after the other;
  (d) denoise_device and denoise_variance_device on the same image and guides, five iterations, with a history of 32 frames everywhere (every pixel takes its variance from
      its own moments) and of 1 frame everywhere (every pixel gathers the 7 x 7 window of moments), and the ratios.
The image is four frames of the renderer's accumulation, the guides this frame's own entries (fold_guides_device at frame index 0) and the moments one sample's.
Usage: python tools/variance_rate.py [--scene dragon] [--reps 20]          (prints one JSON line)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="dragon")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import metal_raytracing_amd as m
    ctx = m.Context(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(dev)
    w, h = 1920, 1080
    n = w * h
    res = {"device": ctx.device_name, "size": [w, h], "reps": a.reps, "scene": a.scene}

    def timed(fns):
        """name -> callable, in turn on the side stream, reps times over -> name -> {median, min, max} of device ms"""
        ms = {k: [] for k in fns}
        with torch.cuda.stream(ts):
            for rep in range(3 + a.reps):
                for k, fn in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ts); fn(); e1.record(ts); ts.synchronize()
                    if rep >= 3: ms[k].append(e0.elapsed_time(e1))
        return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    copy = timed({"copy": lambda: dst.copy_(src)})["copy"]
    copy_gbs = 2 * src.numel() / copy["ms"] / 1e6                     # read + write
    res["copy_256MiB"] = copy; res["copy_GBps"] = copy_gbs
    del src, dst

    two_level = a.scene == "dragon4"
    r = m.Renderer((w, h), m.SCENES[a.scene]((w, h)), ctx=ctx, scene_options={"instancing": 1} if two_level else None)
    ds = r.device_scene
    s = ts.cuda_stream
    r.draw(4, wait=True)
    image = torch.from_numpy(r.accumulation()).to(dev).reshape(n, 4).contiguous()
    cam = m.Camera.from_buffer_copy(r.scene.camera)
    rays, _ = r.primary_rays_device(sample_index=0, stream=0)
    rows = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays, stream=0), stream=0)
    nd, albedo, ids = ds.fold_guides_device(rows, 0, stream=0)
    torch.cuda.synchronize()
    res["surface_share"] = float((albedo[:, 3] != 0).float().mean())

    # (b)
    ms_image = torch.empty((n, 4), device=dev)
    row = timed({"moments_sample": lambda: ds.moments_sample_device(image, albedo, (w, h), out=ms_image, stream=s)})["moments_sample"]
    floor = 48.0 * n / copy_gbs / 1e6
    row.update(floor_ms=floor, over_floor=row["ms"] / floor)
    res["b"] = row

    # (c)
    hist = image.clone(); hist[:, 3] = 5.0
    moments = ms_image.clone(); moments[:, 3] = 5.0
    out_c = torch.empty((n, 4), device=dev); out_m = torch.empty((n, 4), device=dev)
    colour = lambda: ds.reproject_device(rows, image, nd, ids, hist, (w, h), cam, cam, out=out_c, stream=s)
    second = lambda: ds.reproject_device(rows, ms_image, nd, ids, moments, (w, h), cam, cam, out=out_m, stream=s)
    res["c"] = timed({"colour": colour, "moments": second, "both": lambda: (colour(), second())})
    torch.cuda.synchronize()
    res["c"]["kept_share"] = float((out_m[:, 3] > 1.0).float().mean())

    # (d)
    work = torch.empty(ds.denoise_workspace_bytes((w, h)), dtype=torch.uint8, device=dev)
    out_d = torch.empty((n, 4), device=dev); out_v = torch.empty((n, 4), device=dev)
    long_history = out_m.clone(); long_history[:, 3] = 32.0
    short_history = out_m.clone(); short_history[:, 3] = 1.0
    d = timed({"denoise": lambda: ds.denoise_device(image, nd, albedo, (w, h), out=out_d, workspace=work, stream=s),
               "variance_history_32": lambda: ds.denoise_variance_device(image, long_history, nd, albedo, (w, h), out=out_v, workspace=work, stream=s),
               "variance_history_1": lambda: ds.denoise_variance_device(image, short_history, nd, albedo, (w, h), out=out_v, workspace=work, stream=s)})
    d["ratio_history_32"] = d["variance_history_32"]["ms"] / d["denoise"]["ms"]
    d["ratio_history_1"] = d["variance_history_1"]["ms"] / d["denoise"]["ms"]
    d["prepass_gather_ms"] = d["variance_history_1"]["ms"] - d["variance_history_32"]["ms"]
    res["d"] = d
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
