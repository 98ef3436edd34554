"""Render N frames of a named scene with the guide buffers on and write the noisy and the denoised image as PNGs; --time measures the denoiser and
the cost of the guide buffers instead (HIP events, 20 warm repetitions, median).
Usage: python tools/denoise_demo.py [--scene cornell] [--size 640x360] [--frames 4] [--iterations 5] [--out-prefix demo] [--time]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell")
    ap.add_argument("--size", default="640x360")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--out-prefix", default="denoise_demo")
    ap.add_argument("--time", action="store_true", help="time the denoiser (per iteration count) and a draw with guides on / off at this size")
    ap.add_argument("--time-frames", default="20,240", help="--time: frames per draw for the guides on / off comparison")
    a = ap.parse_args()
    import torch
    import metal_raytracing_amd as m
    w, h = (int(x) for x in a.size.split("x"))
    sc = m.SCENES[a.scene]((w, h))
    with m.Renderer((w, h), sc) as r:
        r.set_option("guides", 1)
        r.draw(a.frames, wait=True)
        if not a.time:
            m.save_png(a.out_prefix + "_noisy.png", r.tonemapped())
            r.denoise(iterations=a.iterations, read=False)
            m.save_png(a.out_prefix + "_denoised.png", r.denoised_tonemapped())
            print(f"wrote {a.out_prefix}_noisy.png and {a.out_prefix}_denoised.png ({w}x{h}, {a.frames} frames, {a.iterations} iterations)")
            return
        res = {"scene": a.scene, "size": [w, h], "device": r.ctx.device_name}
        # the renderer's main stream becomes a torch stream, so that torch's HIP events bracket what the library enqueues
        ts = torch.cuda.Stream()
        r.wait(); r.ctx.set_stream(ts.cuda_stream)

        def timed(fn, reps=20, warm=3):
            with torch.cuda.stream(ts):
                for _ in range(warm): fn()
                ts.synchronize()
                ms = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ts); fn(); e1.record(ts); ts.synchronize()
                    ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)
        den = {it: timed(lambda: r.denoise(iterations=it, read=False)) for it in (1, 2, 3, 4, 5)}
        res["denoise_ms_by_iterations"] = den
        res["denoise_ms_per_iteration_at_5"] = den[5] / 5
        # yardstick: the byte floor of one iteration (two 16-byte reads and one 16-byte write per pixel) at the device-to-device copy bandwidth of this box
        # (calibrate.hip reports VALU and gather rates, no copy bandwidth: a 256 MiB copy is timed here)
        src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0"); dst = torch.empty_like(src)
        copy_ms = timed(lambda: dst.copy_(src))
        res["copy_GBps"] = 2 * src.numel() / copy_ms / 1e6
        res["iteration_byte_floor_MB"] = w * h * 48 / 1e6
        res["iteration_floor_ms"] = w * h * 48 / (res["copy_GBps"] * 1e9) * 1e3
        res["iteration_over_floor"] = res["denoise_ms_per_iteration_at_5"] / res["iteration_floor_ms"]
        ts.synchronize(); r.ctx.set_stream(None)
        draws = {}
        for n in (int(x) for x in a.time_frames.split(",")):
            row = {}
            for on in (0, 1, 0, 1):
                r.set_option("guides", on)
                r.draw(n, wait=True)
                ms = []
                for _ in range(5):
                    r.draw(n, wait=True); ms.append(r.stats.ms_gpu_last)
                row.setdefault(f"guides_{on}_ms", []).append(statistics.median(ms))
            row["ratio"] = statistics.mean(row["guides_1_ms"]) / statistics.mean(row["guides_0_ms"])
            draws[n] = row
        res["draw_ms"] = draws
        r.set_option("guides", 0)
        r.draw(20, wait=True)
        res["kernel_times_20_frames_guides_0"] = r.kernel_times
        print(json.dumps(res))


if __name__ == "__main__":
    main()
