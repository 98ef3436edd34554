"""Rate of the path-tracing stages on device buffers (Renderer.primary_rays_device / DeviceScene.scatter_device) and of a frame composed from the five public stages beside
Renderer drawing the same frame — DESIGN.md §10i.  Per scene (DragonScene flattened; dragon4 two-level):
  (a) each new stage alone at 2^22 rows — primary_rays_device of a 2048 x 2048 image; scatter_device at bounce 0 on the surfaces its rays hit and at bounce 1 on the surfaces
      the bounce rays hit (dense rows, the misses among them) — against its byte floor at this box's device copy bandwidth (a 256 MiB torch copy, read + write counted, timed
      the same way, as tools/surface_rate.py defines it): 36 B per pixel written; 68 B read + 80 B written per row;
  (b) one composed frame at 1920 x 1080 — generate, closest, resolve, scatter, any; three bounces; throughput and radiance as torch mul / add / where — against Renderer
      drawing one frame alone (frame index 0 both).  Host wall time from the first enqueue to the end of a device synchronize for both legs; the composed leg's HIP-event time
      and the renderer's own device time (stats.ms_gpu_last) beside them.  No bar: the composed frame has dense rows, no compaction, more launches and torch ops in between.
and, once (the materials leg; the Cornell box with a glass sphere, a glossy sphere and an emitting quad of the materials tests, max_bounces 4):
  (c) scatter_materials_device alone at 2^22 rows at bounce 0 against its byte floor — per row the contract reads 48 B of surface, 16 B of ray and 4 B of index and writes
      32 + 16 + 32 + 32 B: 180 B (with whole 64-byte surface rows and 32-byte ray rows, as the lines are fetched: 212 B, reported beside it; the material and light rows are
      gathers from tables of a few lines and are not counted) — and one composed materials frame at 1920 x 1080, four bounces, beside Renderer with materials = 1 drawing one
      frame, timed as (b).
and, per scene and for the materials leg (the queue legs):
  (d) compact_rows_device alone at 2^22 rows on the columns of a path's state — rays 32 B, Halton index 4 B, pixel 4 B, throughput 16 B — keeping the surfaces of bounce 1's
      dense rows and keeping a random 50 %, against its byte floor at the same copy bandwidth: 2 B of keep per row (it is read twice) plus 56 B read and 56 B written per
      kept row;
  (e) the composed 1080p frame ON QUEUES (tests/queues_compose.py: the wanted shadow rays and the surviving paths compacted at every bounce), in two forms — the counts read
      by the host once per bounce and every tensor sliced to them; no host read at all, the counts handed on as count= and torch's ops over the capacity with the tail
      masked — beside the dense composed frame and Renderer of (b) / (c), timed the same way in the same loop.  Both must report same_bits true.
and, per scene and for the materials leg (the path-state legs):
  (f) each path-state stage alone at 2^22 rows against its byte floor at the same copy bandwidth — advance_paths_device, diffuse form: 32 B of surface, 16 B of light and
      16 B of throughput read, 16 B + 2 B of masks written per row (the materials form, in the materials leg: 32 B of lobe and the 2 x 16 B of the radiance row in place of
      the surface); deposit_light_device: 4 + 16 + 16 + 4 B read per row and 2 x 16 B of radiance per lit row; fold_sample_device: 2 x 16 B read and 16 B written per
      pixel, 16 B more with clear_sample;
  (g) the frame on queues composed with the path-state stages (tests/paths_compose.py: no torch op between the stages, count= throughout, fold_sample_device at the end) in
      the loop of (e), beside its legs; same_bits against Renderer, and its medians over those of (e)'s no-host-read form.
and, per scene (the image legs), at 1920 x 1080:
  (h) each image stage alone, HIP events — fold_guides_device at frame 0 and at a later frame against its byte floors at the same copy bandwidth (112 and 144 B per pixel:
      the 64-byte surface row, the two old averages except at frame 0, three 16-byte entries written), tonemap_device against 20 B per pixel, and denoise_device beside
      Renderer.denoise on the same image and guides (the same kernels: the expectation is equality);
  (i) the fused frame of (g) with and without the guide fold of its bounce-0 rows, beside Renderer drawing the frame with guides = 0 and with guides = 1 (which walks the
      primary rays a second time), the four alternating in one loop: what guides cost a composed frame and what they cost the renderer.
and, per scene (the temporal legs), at 1920 x 1080:
  (j) reproject_device alone, HIP events, in three cases — a still world (equal cameras, no previous positions), a camera turned by a third of a pixel and by three pixels
      (previous positions given) — against its byte floor at the same copy bandwidth: per pixel the 64-byte surface row, 16 B of sample and 16 B written, and per
      surface pixel 48 B of the previous frame's ids, normal | depth and history (a moved frame's four taps are its neighbours' too: the lines are the same), 16 B more
      with previous positions;
  (k) the fused frame of (g) ending in reproject_device and the fold of the frame's own guide entries (fold_guides_device at frame index 0, the next frame's previous
      entries) beside the same frame ending in fold_sample_device, alternating in one loop.
3 warm + 20 timed repetitions, the legs alternating, medians.
Usage: python tools/integrator_rate.py [--scenes dragon,dragon4] [--materials 1] [--reps 20] [--legs all|image|temporal]
(prints one JSON line; --legs image: (h) and (i) alone; --legs temporal: (j) and (k) alone)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compose(torch, r, ds, sample_index, dev, miss, bounces=3):
    """one frame of the reference's integrator from the public stages on torch's current stream -> (n, 3) radiance sample"""
    rays, hidx = r.primary_rays_device(sample_index=sample_index)
    n = rays.shape[0]
    thr = torch.ones((n, 3), device=dev); acc = torch.zeros((n, 3), device=dev); alive = torch.ones(n, dtype=torch.bool, device=dev)
    for b in range(bounces):
        hits = ds.intersect_closest_device(rays)
        surf = ds.resolve_hits_device(rays, hits)
        alive = alive & (surf[:, 7].view(torch.int32) == 1)
        surf = torch.where(alive[:, None], surf, miss)
        shadow, light, nxt = ds.scatter_device(surf, hidx, b, next_rays=b + 1 < bounces)
        occluded = ds.intersect_any_device(shadow)
        thr = torch.mul(thr, surf[:, 8:11])
        lit = alive & (light[:, 3] == 1.0) & (occluded == 0)
        acc = torch.where(lit[:, None], torch.add(acc, torch.mul(light[:, 0:3], thr)), acc)
        rays = nxt
    return acc


def compose_materials(torch, r, ds, sample_index, dev, miss, bounces):
    """one frame of the renderer's integrator with materials = 1 from the public stages on torch's current stream -> (n, 3) radiance sample"""
    rays, hidx = r.primary_rays_device(sample_index=sample_index)
    n = rays.shape[0]
    thr = torch.ones((n, 3), device=dev); acc = torch.zeros((n, 3), device=dev); alive = torch.ones(n, dtype=torch.bool, device=dev)
    for b in range(bounces):
        hits = ds.intersect_closest_device(rays)
        surf = ds.resolve_hits_device(rays, hits)
        surf = torch.where(alive[:, None], surf, miss)
        shadow, light, nxt, lobes = ds.scatter_materials_device(rays, surf, hidx, b, bounces, next_rays=b + 1 < bounces)
        occluded = ds.intersect_any_device(shadow)
        lobe = lobes[:, 3].view(torch.int32)
        acc = torch.add(acc, torch.mul(thr, lobes[:, 4:7]))
        thr = torch.mul(thr, lobes[:, 0:3])
        lit = (light[:, 3] == 1.0) & (occluded == 0)
        acc = torch.where(lit[:, None], torch.add(acc, torch.mul(light[:, 0:3], thr)), acc)
        alive = (lobe >= 1) & (lobe <= 4)
        rays = nxt
    return acc


def queue_legs(torch, m, ds, dev, rows, keeps, copy_gbs, timed, stream):
    """(d): compact_rows_device alone on a path's state, one entry per keep mask of `keeps` (name -> (rows,) bool)"""
    cols = [torch.empty((rows, 8), device=dev).normal_(), torch.zeros(rows, dtype=torch.int32, device=dev), torch.arange(rows, dtype=torch.int32, device=dev), torch.ones((rows, 4), device=dev)]
    out = [torch.empty_like(c) for c in cols]
    ws = torch.empty(ds.compact_workspace_bytes(rows), dtype=torch.uint8, device=dev)
    res = {}
    for name, keep in keeps.items():
        ds.compact_rows_device(keep, cols, out=out, workspace=ws, stream=0)
        torch.cuda.synchronize()
        ms = timed([lambda: ds.compact_rows_device(keep, cols, out=out, workspace=ws, stream=stream)])[0]
        share = float(keep.float().mean())
        floor = (2.0 + 112.0 * share) * rows / copy_gbs / 1e6
        res[name] = {"keep_share": share, "ms": ms, "floor_ms": floor, "over_floor": ms / floor}
    return res


def path_legs(torch, ds, dev, rows, surfaces, lobes, light, copy_gbs, timed, stream):
    """(f): the path-state stages alone on `rows` rows — advance in the form the rows given allow (surfaces or lobes), deposit on the light rows with a random half of the
    shadow rays occluded, fold with and without clear_sample"""
    thr, pix, rad = ds.reset_paths_device(rows, stream=0)
    masks = (torch.empty(rows, dtype=torch.uint8, device=dev), torch.empty(rows, dtype=torch.uint8, device=dev))
    gen = torch.Generator(device=dev); gen.manual_seed(2)
    occluded = (torch.rand(rows, device=dev, generator=gen) < 0.5).to(torch.int32)
    accum = torch.zeros((rows, 4), device=dev)
    form = {"surfaces": surfaces} if lobes is None else {"lobes": lobes, "pixel": pix, "radiance": rad}
    fns = [lambda: ds.advance_paths_device(light, thr, out=masks, stream=stream, **form), lambda: ds.advance_paths_device(light, thr, keep_path=False, out=masks[:1], stream=stream, **form),
           lambda: ds.deposit_light_device(occluded, light, thr, pix, rad, stream=stream), lambda: ds.fold_sample_device(rad, accum, 1, stream=stream),
           lambda: ds.fold_sample_device(rad, accum, 1, clear_sample=True, stream=stream)]
    for fn in fns: fn()
    torch.cuda.synchronize()
    t = timed(fns)
    lit = float((occluded == 0).float().mean())
    per_row = {"advance": (114.0 if lobes is not None else 82.0), "advance_last_bounce": (113.0 if lobes is not None else 81.0), "deposit": 40.0 + 32.0 * lit, "fold": 48.0, "fold_clear": 64.0}
    res = {"form": "materials" if lobes is not None else "diffuse", "lit_share": lit}
    for (k, b), ms in zip(per_row.items(), t):
        floor = b * rows / copy_gbs / 1e6
        res[k] = {"ms": ms, "bytes_per_row": b, "floor_ms": floor, "over_floor": ms / floor}
    return res


def fused_over_queued(e):
    """(g) out of the loop of (e): the fused leg and its medians over the no-host-read form's"""
    g = e.pop("fused_path_state")
    q = e["queued_no_host_read"]
    g["wall_over_queued_no_host_read"] = g["wall_ms"] / q["wall_ms"]; g["event_over_queued_no_host_read"] = g["event_ms"] / q["event_ms"]
    return g


class FoldAtBounceZero:
    """a DeviceScene whose resolve_hits_device also folds the rows into the guide buffers where they are a frame's bounce-0 rows (the dense call, without count=): the
    fused frame of paths_compose.compose_fused with the guide fold in it, call for call"""

    def __init__(self, ds, frame_index, guides):
        self._ds, self._frame, self.guides = ds, frame_index, guides

    def __getattr__(self, name):
        return getattr(self._ds, name)

    def resolve_hits_device(self, rays, hits, **kw):
        surf = self._ds.resolve_hits_device(rays, hits, **kw)
        if "count" not in kw: self.guides = self._ds.fold_guides_device(surf, self._frame, out=self.guides)
        return surf


def image_legs(torch, m, ctx, r, ds, dev, ts, reps, copy_gbs, timed, compose_fused):
    """(h) and (i) on a 1920 x 1080 renderer"""
    w, h = r.size
    n = w * h
    s = ts.cuda_stream
    r.set_option("guides", 1)
    r.frameIndex = 0
    r.draw(4, wait=True)
    g = r.guides()
    image = torch.from_numpy(r.accumulation()).to(dev); nd = torch.from_numpy(g["normal_depth"]).to(dev); al = torch.from_numpy(g["albedo"]).to(dev)
    rays, _ = r.primary_rays_device(sample_index=4, stream=0)
    surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays, stream=0), stream=0)
    guides = (nd.reshape(-1, 4).clone(), al.reshape(-1, 4).clone(), torch.empty((n, 4), dtype=torch.int32, device=dev))
    den = torch.empty_like(image); rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(ds.denoise_workspace_bytes((w, h)), dtype=torch.uint8, device=dev)
    theirs = torch.cuda.ExternalStream(ctx.stream, device=dev)                     # the renderer's stream: its filter is enqueued there
    torch.cuda.synchronize()
    t = timed([lambda: ds.fold_guides_device(surf, 0, out=guides, stream=s), lambda: ds.fold_guides_device(surf, 4, out=guides, stream=s),
               lambda: ds.tonemap_device(image, (w, h), out=rgba, stream=s)])
    mine, own = [], []
    for rep in range(3 + reps):                                                    # the two filters alternating with nothing between them: each finds what the other left in the caches
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts); ds.denoise_device(image, nd, al, (w, h), out=den, workspace=work, stream=s); e1.record(ts); ts.synchronize()
        if rep >= 3: mine.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(theirs); r.denoise(read=False); e1.record(theirs); theirs.synchronize()
        if rep >= 3: own.append(e0.elapsed_time(e1))
    t.append(statistics.median(mine))
    same = bool(torch.equal(den.view(torch.int32), torch.from_numpy(r.denoised()).to(dev).view(torch.int32)))
    res = {"surface_share": float((surf[:, 7].view(torch.int32) == 1).float().mean())}
    for k, ms, b in (("fold_frame_0", t[0], 112.0), ("fold_later_frame", t[1], 144.0), ("tonemap", t[2], 20.0)):
        floor = b * n / copy_gbs / 1e6
        res[k] = {"ms": ms, "bytes_per_pixel": b, "floor_ms": floor, "over_floor": ms / floor}
    res["denoise"] = {"device_ms": t[3], "renderer_ms": statistics.median(own), "device_over_renderer": t[3] / statistics.median(own), "same_bits": same}
    # (i)
    accum = torch.empty((n, 4), device=dev)
    folded = FoldAtBounceZero(ds, 0, (torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev)))

    def fused(scene):
        rad = compose_fused(torch, r, scene, 0, dev, bounces=3)
        ds.fold_sample_device(rad, accum, 0)
        return accum

    legs = {"fused": lambda: fused(ds), "fused_with_guide_fold": lambda: fused(folded)}
    wall = {k: [] for k in legs}; ev = {k: [] for k in legs}; rw = {0: [], 1: []}; rd = {0: [], 1: []}
    for rep in range(3 + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts); fn(); e1.record(ts); ts.synchronize()
                t1 = time.perf_counter()
            if rep >= 3: wall[k].append((t1 - t0) * 1e3); ev[k].append(e0.elapsed_time(e1))
        for on in (0, 1):
            r.set_option("guides", on)
            r.frameIndex = 0
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            r.draw(1, wait=True)
            t3 = time.perf_counter()
            if rep >= 3: rw[on].append((t3 - t2) * 1e3); rd[on].append(float(r.stats.ms_gpu_last))
    gr = r.guides()                                                                # (the last draw had guides = 1, frame 0)
    med = statistics.median
    frame = {k: {"wall_ms": med(wall[k]), "event_ms": med(ev[k])} for k in legs}
    frame["guide_fold_cost_event_ms"] = med(ev["fused_with_guide_fold"]) - med(ev["fused"]); frame["guide_fold_cost_wall_ms"] = med(wall["fused_with_guide_fold"]) - med(wall["fused"])
    frame["renderer"] = {"wall_ms": med(rw[0]), "device_ms": med(rd[0])}; frame["renderer_guides"] = {"wall_ms": med(rw[1]), "device_ms": med(rd[1])}
    frame["renderer_guides_cost_wall_ms"] = med(rw[1]) - med(rw[0]); frame["renderer_guides_cost_device_ms"] = med(rd[1]) - med(rd[0])
    frame["same_bits"] = bool(torch.equal(accum.view(torch.int32), torch.from_numpy(r.accumulation()).to(dev).reshape(-1, 4).view(torch.int32))
                              and all(torch.equal(a.view(torch.int32), torch.from_numpy(gr[k]).to(dev).reshape(-1, 4).view(torch.int32))
                                      for a, k in zip(folded.guides, ("normal_depth", "albedo", "ids"))))
    r.set_option("guides", 0)
    return {"h": res, "i": frame}


class KeepBounceZero:
    """a DeviceScene that keeps the rows of the dense resolve_hits_device call — a frame's bounce-0 rows — for the stage after the frame"""

    def __init__(self, ds):
        self._ds, self.rows = ds, None

    def __getattr__(self, name):
        return getattr(self._ds, name)

    def resolve_hits_device(self, rays, hits, **kw):
        surf = self._ds.resolve_hits_device(rays, hits, **kw)
        if "count" not in kw: self.rows = surf
        return surf


def temporal_legs(torch, m, r, ds, dev, ts, reps, copy_gbs, timed, compose_fused):
    """(j) and (k) on a 1920 x 1080 renderer"""
    w, h = r.size
    n = w * h
    s = ts.cuda_stream
    base = m.Camera.from_buffer_copy(r.scene.camera)

    def turned(pixels):
        c = m.Camera.from_buffer_copy(base)
        for k in "xyz": setattr(c.forward, k, getattr(base.forward, k) + 2.0 * pixels / w * getattr(base.right, k))          # every pixel moves by about `pixels` columns
        return c

    def rows_of(camera, sample_index):
        r.set_camera(camera)
        rays, _ = r.primary_rays_device(sample_index=sample_index, stream=0)
        return ds.resolve_hits_device(rays, ds.intersect_closest_device(rays, stream=0), stream=0)

    prev_rows = rows_of(base, 0)
    nd, _, ids = ds.fold_guides_device(prev_rows, 0, stream=0)
    hist = torch.rand((n, 4), device=dev); hist[:, 3] = 5.0
    sample = torch.rand((n, 4), device=dev)
    out = torch.empty((n, 4), device=dev)
    cases = {"still": (base, rows_of(base, 1), False), "third_of_a_pixel": (turned(1.0 / 3.0), None, True), "three_pixels": (turned(3.0), None, True)}
    res = {}
    fns = []
    for name, (cam, rows, moved) in cases.items():
        rows = rows_of(cam, 1) if rows is None else rows
        pos = rows[:, 0:4].contiguous() if moved else None                              # (the scene stands still: a point's previous position is its own)
        share = float((rows[:, 7].view(torch.int32) == 1).float().mean())
        res[name] = {"surface_share": share, "bytes_per_pixel": 96.0 + (48.0 + (16.0 if moved else 0.0)) * share}
        fns.append(lambda cam=cam, rows=rows, pos=pos: ds.reproject_device(rows, sample, nd, ids, hist, (w, h), cam, base, prev_position=pos, out=out, stream=s))
    r.set_camera(base)
    torch.cuda.synchronize()
    for (name, row), ms, fn in zip(res.items(), timed(fns), fns):
        fn(); torch.cuda.synchronize()
        floor = row["bytes_per_pixel"] * n / copy_gbs / 1e6
        row.update(ms=ms, floor_ms=floor, over_floor=ms / floor, kept_share=float((out[:, 3] > 1.0).float().mean()))
    # (k)
    accum = torch.empty((n, 4), device=dev)
    keeper = KeepBounceZero(ds)
    guides = (torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev))

    def folded():
        ds.fold_sample_device(compose_fused(torch, r, ds, 1, dev, bounces=3), accum, 1)

    def reprojected():
        rad = compose_fused(torch, r, keeper, 1, dev, bounces=3)
        ds.reproject_device(keeper.rows, rad, nd, ids, hist, (w, h), base, base, out=out)
        ds.fold_guides_device(keeper.rows, 0, out=guides)

    legs = {"fused_fold_sample": folded, "fused_reproject": reprojected}
    wall = {k: [] for k in legs}; ev = {k: [] for k in legs}
    for rep in range(3 + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts); fn(); e1.record(ts); ts.synchronize()
                t1 = time.perf_counter()
            if rep >= 3: wall[k].append((t1 - t0) * 1e3); ev[k].append(e0.elapsed_time(e1))
    med = statistics.median
    frame = {k: {"wall_ms": med(wall[k]), "event_ms": med(ev[k])} for k in legs}
    frame["reproject_cost_event_ms"] = med(ev["fused_reproject"]) - med(ev["fused_fold_sample"]); frame["reproject_cost_wall_ms"] = med(wall["fused_reproject"]) - med(wall["fused_fold_sample"])
    return {"j": res, "k": frame}


def frame_legs(torch, r, dev, ts, reps, legs):
    """(b) / (c) / (e) in one loop: each callable of `legs` (name -> fn() -> (n, 3) sample) composed on the side stream, then Renderer drawing frame 0; medians of host wall
    and HIP-event time per leg, and whether each leg's sample has the renderer's bits"""
    wall = {k: [] for k in legs}; ev = {k: [] for k in legs}; rw = []; own = []; acc = {}
    for rep in range(3 + reps):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts); acc[k] = fn(); e1.record(ts); ts.synchronize()
                t1 = time.perf_counter()
            if rep >= 3: wall[k].append((t1 - t0) * 1e3); ev[k].append(e0.elapsed_time(e1))
        r.frameIndex = 0
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r.draw(1, wait=True)
        t3 = time.perf_counter()
        if rep >= 3: rw.append((t3 - t2) * 1e3); own.append(float(r.stats.ms_gpu_last))
    img = torch.from_numpy(r.accumulation()).to(dev).reshape(-1, 4)[:, 0:3].contiguous().view(torch.int32)
    out = {"renderer_wall_ms": statistics.median(rw), "renderer_device_ms": statistics.median(own)}
    for k in legs:
        out[k] = {"wall_ms": statistics.median(wall[k]), "event_ms": statistics.median(ev[k]), "over_renderer_wall": statistics.median(wall[k]) / statistics.median(rw),
                  "same_bits": bool(torch.equal(acc[k][:, 0:3].contiguous().view(torch.int32), img))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="dragon,dragon4")
    ap.add_argument("--materials", type=int, default=1, help="(c): the materials leg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=2048, help="(a): the image is side x side pixels")
    ap.add_argument("--legs", choices=("all", "image", "temporal"), default="all", help="image: (h) and (i) alone, per scene (no materials leg); temporal: (j) and (k) alone")
    a = ap.parse_args()
    if a.legs != "all": a.materials = 0
    import torch
    import metal_raytracing_amd as m
    ctx = m.Context(0)
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(dev)
    rows = a.side * a.side
    res = {"device": ctx.device_name, "rows": rows, "reps": a.reps, "scenes": {}}

    def timed(fns):
        """the callables in turn on the side stream, reps times over; median device ms of each"""
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
    miss = torch.tensor([[0.0, 0.0, 0.0, -1.0] + [0.0] * 12], device=dev)
    miss.view(torch.int32)[0, 11] = -1; miss.view(torch.int32)[0, 12:15] = -1          # the miss record of resolve_hits_device
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from queues_compose import compose_queued                       # the queued frame of the GPU tests (test infrastructure: the tool runs from the repository)
    from paths_compose import compose_fused                         # and the same frame with the path state kept by the library

    def fused(r, ds, bounces, materials, accum):
        rad = compose_fused(torch, r, ds, 0, dev, bounces=bounces, materials=materials)
        ds.fold_sample_device(rad, accum, 0)
        return accum
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    half = torch.rand(rows, device=dev, generator=gen) < 0.5
    for name in [x for x in a.scenes.split(",") if x]:
        two_level = name == "dragon4"
        opts = {"instancing": 1} if two_level else None
        row = {"instancing": int(two_level)}
        if a.legs != "all":
            r = m.Renderer((1920, 1080), m.SCENES[name]((1920, 1080)), ctx=ctx, scene_options=opts)
            row["triangles"] = int(r.device_scene.stats.triangles)
            if a.legs == "image": row.update(image_legs(torch, m, ctx, r, r.device_scene, dev, ts, a.reps, copy_gbs, timed, compose_fused))
            else: row.update(temporal_legs(torch, m, r, r.device_scene, dev, ts, a.reps, copy_gbs, timed, compose_fused))
            r.close()
            res["scenes"][name] = row
            continue
        # (a) the stages alone
        sc = m.SCENES[name]((a.side, a.side))
        r = m.Renderer((a.side, a.side), sc, ctx=ctx, scene_options=opts)
        ds = r.device_scene
        row["triangles"] = int(ds.stats.triangles)
        prim = (torch.empty((rows, 8), device=dev), torch.empty((rows,), dtype=torch.int32, device=dev))
        outs = (torch.empty((rows, 8), device=dev), torch.empty((rows, 4), device=dev), torch.empty((rows, 8), device=dev))
        s = ts.cuda_stream
        r.primary_rays_device(sample_index=0, out=prim, stream=0)
        surf0 = ds.resolve_hits_device(prim[0], ds.intersect_closest_device(prim[0], stream=0), stream=0)
        ds.scatter_device(surf0, prim[1], 0, out=outs, stream=0)
        surf1 = ds.resolve_hits_device(outs[2], ds.intersect_closest_device(outs[2], stream=0), stream=0)
        torch.cuda.synchronize()
        t = timed([lambda: r.primary_rays_device(sample_index=0, out=prim, stream=s), lambda: ds.scatter_device(surf0, prim[1], 0, out=outs, stream=s),
                   lambda: ds.scatter_device(surf1, prim[1], 1, out=outs, stream=s)])
        floor_p = 36.0 * rows / copy_gbs / 1e6; floor_s = 148.0 * rows / copy_gbs / 1e6
        row["a"] = {"primary_ms": t[0], "primary_floor_ms": floor_p, "primary_over_floor": t[0] / floor_p,
                    "scatter_b0_ms": t[1], "scatter_b1_ms": t[2], "scatter_floor_ms": floor_s, "scatter_b0_over_floor": t[1] / floor_s, "scatter_b1_over_floor": t[2] / floor_s,
                    "surface_share_b0": float((surf0[:, 7].view(torch.int32) == 1).float().mean()), "surface_share_b1": float((surf1[:, 7].view(torch.int32) == 1).float().mean())}
        row["d"] = queue_legs(torch, m, ds, dev, rows, {"bounce_1_surfaces": (surf1[:, 7].view(torch.int32) == 1).contiguous(), "random_half": half}, copy_gbs, timed, s)
        row["f"] = path_legs(torch, ds, dev, rows, surf0, None, outs[1], copy_gbs, timed, s)
        del prim, outs, surf0, surf1
        r.close()
        # (b) the composed frame beside the renderer's
        sc = m.SCENES[name]((1920, 1080))
        r = m.Renderer((1920, 1080), sc, ctx=ctx, scene_options=opts)
        ds = r.device_scene
        wall = {"composed": [], "renderer": []}; ev = []; own = []
        for rep in range(3 + a.reps):
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts); acc = compose(torch, r, ds, 0, dev, miss); e1.record(ts); ts.synchronize()
                t1 = time.perf_counter()
            r.frameIndex = 0
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            r.draw(1, wait=True)
            t3 = time.perf_counter()
            if rep >= 3:
                wall["composed"].append((t1 - t0) * 1e3); wall["renderer"].append((t3 - t2) * 1e3); ev.append(e0.elapsed_time(e1)); own.append(float(r.stats.ms_gpu_last))
        img = torch.from_numpy(r.accumulation()).to(dev).reshape(-1, 4)[:, 0:3]
        row["b"] = {"composed_wall_ms": statistics.median(wall["composed"]), "renderer_wall_ms": statistics.median(wall["renderer"]), "composed_event_ms": statistics.median(ev),
                    "renderer_device_ms": statistics.median(own), "composed_over_renderer_wall": statistics.median(wall["composed"]) / statistics.median(wall["renderer"]),
                    "same_bits": bool(torch.equal(acc.view(torch.int32), img.contiguous().view(torch.int32)))}
        # (e) the same frame on queues, both forms, beside the dense one and the renderer in one loop; (g) the fused form in the same loop
        accum = torch.empty((1920 * 1080, 4), device=dev)
        row["e"] = frame_legs(torch, r, dev, ts, a.reps, {"dense": lambda: compose(torch, r, ds, 0, dev, miss),
                                                          "queued_host_counts": lambda: compose_queued(torch, r, ds, 0, dev, bounces=3, host_counts=True),
                                                          "queued_no_host_read": lambda: compose_queued(torch, r, ds, 0, dev, bounces=3, host_counts=False),
                                                          "fused_path_state": lambda: fused(r, ds, 3, False, accum)})
        row["g"] = fused_over_queued(row["e"])
        row.update(image_legs(torch, m, ctx, r, ds, dev, ts, a.reps, copy_gbs, timed, compose_fused))
        row.update(temporal_legs(torch, m, r, ds, dev, ts, a.reps, copy_gbs, timed, compose_fused))
        r.close()
        res["scenes"][name] = row
    if a.materials:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from material_scenes import cornell_with_materials          # the scene of the materials tests (test infrastructure: the tool runs from the repository)
        bounces = 4
        row = {"max_bounces": bounces}
        r = m.Renderer((a.side, a.side), cornell_with_materials(m, (a.side, a.side)), ctx=ctx, max_bounces=bounces)
        ds = r.device_scene
        prim = r.primary_rays_device(sample_index=0, stream=0)
        surf0 = ds.resolve_hits_device(prim[0], ds.intersect_closest_device(prim[0], stream=0), stream=0)
        outs = (torch.empty((rows, 8), device=dev), torch.empty((rows, 4), device=dev), torch.empty((rows, 8), device=dev), torch.empty((rows, 8), device=dev))
        ds.scatter_materials_device(prim[0], surf0, prim[1], 0, bounces, out=outs, stream=0)
        torch.cuda.synchronize()
        s = ts.cuda_stream
        t = timed([lambda: ds.scatter_materials_device(prim[0], surf0, prim[1], 0, bounces, out=outs, stream=s), lambda: ds.scatter_materials_device(prim[0], surf0, prim[1], 0, bounces, next_rays=False, out=(outs[0], outs[1], outs[3]), stream=s)])
        floor_c = 180.0 * rows / copy_gbs / 1e6; floor_l = 212.0 * rows / copy_gbs / 1e6
        lobes = outs[3][:, 3].view(torch.int32)
        row["c"] = {"scatter_materials_b0_ms": t[0], "no_next_rays_ms": t[1], "floor_180B_ms": floor_c, "over_floor_180B": t[0] / floor_c, "floor_212B_ms": floor_l, "over_floor_212B": t[0] / floor_l,
                    "lobe_share": [float((lobes == k).float().mean()) for k in range(6)]}
        row["d"] = queue_legs(torch, m, ds, dev, rows, {"bounce_0_paths_that_go_on": ((lobes >= 1) & (lobes <= 4)).contiguous(), "random_half": half}, copy_gbs, timed, s)
        row["f"] = path_legs(torch, ds, dev, rows, None, outs[3], outs[1], copy_gbs, timed, s)
        del prim, outs, surf0, lobes
        r.close()
        r = m.Renderer((1920, 1080), cornell_with_materials(m, (1920, 1080)), ctx=ctx, max_bounces=bounces)
        r.set_option("materials", 1)
        ds = r.device_scene
        wall = {"composed": [], "renderer": []}; ev = []; own = []
        for rep in range(3 + a.reps):
            torch.cuda.synchronize()
            with torch.cuda.stream(ts):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(ts); acc = compose_materials(torch, r, ds, 0, dev, miss, bounces); e1.record(ts); ts.synchronize()
                t1 = time.perf_counter()
            r.frameIndex = 0
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            r.draw(1, wait=True)
            t3 = time.perf_counter()
            if rep >= 3:
                wall["composed"].append((t1 - t0) * 1e3); wall["renderer"].append((t3 - t2) * 1e3); ev.append(e0.elapsed_time(e1)); own.append(float(r.stats.ms_gpu_last))
        img = torch.from_numpy(r.accumulation()).to(dev).reshape(-1, 4)[:, 0:3]
        row["frame"] = {"composed_wall_ms": statistics.median(wall["composed"]), "renderer_wall_ms": statistics.median(wall["renderer"]), "composed_event_ms": statistics.median(ev),
                        "renderer_device_ms": statistics.median(own), "composed_over_renderer_wall": statistics.median(wall["composed"]) / statistics.median(wall["renderer"]),
                        "same_bits": bool(torch.equal(acc.view(torch.int32), img.contiguous().view(torch.int32)))}
        accum = torch.empty((1920 * 1080, 4), device=dev)
        row["e"] = frame_legs(torch, r, dev, ts, a.reps, {"dense": lambda: compose_materials(torch, r, ds, 0, dev, miss, bounces),
                                                          "queued_host_counts": lambda: compose_queued(torch, r, ds, 0, dev, bounces=bounces, materials=True, host_counts=True),
                                                          "queued_no_host_read": lambda: compose_queued(torch, r, ds, 0, dev, bounces=bounces, materials=True, host_counts=False),
                                                          "fused_path_state": lambda: fused(r, ds, bounces, True, accum)})
        row["g"] = fused_over_queued(row["e"])
        r.close()
        res["materials"] = row
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
