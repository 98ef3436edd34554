"""Temporal reprojection of the accumulated image on device buffers, on a stream (DeviceScene.reproject_device).  Every comparison is on bits, as int32
views, against tests/temporal_reference.py fed the same inputs: the known-answer and rejection cases of tests/temporal_cases.py, random images with every feature present
at sizes around a wave and a workgroup and on non-square images, both streams, every refusal with the outputs left alone, and one sequence composed from the stage
entries — camera and one instance moving — whose every frame equals the reference fed the downloaded inputs."""
import gc
import os
import subprocess

import numpy as np
import pytest

import temporal_cases as TC
import temporal_reference as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7B7B7B7B
f32 = np.float32


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _camera(mrt, rows):
    c = mrt.Camera()
    for name, row in zip(("position", "right", "up", "forward"), np.asarray(rows, f32)):
        setattr(c, name, mrt.Float3(float(row[0]), float(row[1]), float(row[2])))
    return c


def _same(got, want, what):
    g = np.ascontiguousarray(got).view(np.int32).reshape(-1, 4); w = np.ascontiguousarray(want).view(np.int32).reshape(-1, 4)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at {bad[0]}: {np.asarray(got).reshape(-1, 4)[bad[0]]} != {np.asarray(want).reshape(-1, 4)[bad[0]]}")


@pytest.fixture(scope="module")
def ds(mrt, gpu_ctx):
    """any committed scene of the context: the stage reads none"""
    r = mrt.Renderer((16, 16), mrt.CornellScene((16, 16)), ctx=gpu_ctx, seed=1)
    yield r.device_scene
    r.close()


def _upload(c, dev):
    """the case's buffers on the device, in reproject_device's order: surfaces, sample, prev_normal_depth, prev_ids, prev_history, prev_position (or None)"""
    rows = np.ascontiguousarray(c["surfaces"]).view(f32).reshape(-1, 16)
    return [_t(rows, dev), _t(c["sample"], dev), _t(c["prev_normal_depth"], dev), _t(c["prev_ids"], dev), _t(c["prev_history"], dev),
            None if c["prev_position"] is None else _t(c["prev_position"], dev)]


def _call(mrt, ds, c, t, out=None, stream=None):
    return ds.reproject_device(t[0], t[1], t[2], t[3], t[4], c["size"], _camera(mrt, c["camera"]), _camera(mrt, c["prev_camera"]), prev_position=t[5], out=out, stream=stream, **c["params"])


def _check(mrt, gpu_ctx, ds, c):
    import torch
    dev = _dev(gpu_ctx)
    t = _upload(c, dev)
    before = [None if x is None else x.clone() for x in t]
    out = torch.full((c["size"][0] * c["size"][1], 4), float("nan"), device=dev)
    assert _call(mrt, ds, c, t, out=out) is out
    want = TC.run_reference(c)
    _same(out.cpu().numpy(), want, c["name"])
    for x, b in zip(t, before):
        if x is not None: assert torch.equal(x.view(torch.int32), b.view(torch.int32)), f"{c['name']}: an input was modified"
    return want


# ---------------------------------------------------------------- 1. the cases whose answers are known, and each rejection alone
@pytest.mark.parametrize("c", TC.known_answer_cases() + TC.rejection_cases(), ids=lambda c: c["name"])
def test_known_answers_and_rejections_equal_the_reference(mrt, gpu_ctx, ds, c):
    want = _check(mrt, gpu_ctx, ds, c)
    for pixel, taps in c["checks"].items():                                                             # (what tests/test_temporal_cpu.py holds the reference to)
        assert np.array_equal(want[pixel].view(np.uint32), TC.blend(c, pixel, taps).view(np.uint32)), (c["name"], pixel)


# ---------------------------------------------------------------- 2. random images: non-square ones, a row of pixels around a wave and a workgroup
@pytest.mark.parametrize("size", [(16, 8), (33, 17), (64, 64), (1, 1), (63, 1), (64, 1), (65, 1), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_images_equal_the_reference(mrt, gpu_ctx, ds, size):
    c = TC.random_case(size, 100 + size[0])                                                             # (tests/test_temporal_cpu.py: every feature is in the 33 x 17 one)
    want = _check(mrt, gpu_ctx, ds, c)
    assert np.isfinite(want).all()
    if size[0] * size[1] >= 128: assert (want[:, 3] > 1).any() and (want[:, 3] == 1).any()
    # fresh output; other parameters
    c2 = dict(c); c2["params"] = dict(max_history=5.0, min_cos_normal=0.99, depth_tolerance=0.01); c2["name"] += " tight"
    t = _upload(c2, _dev(gpu_ctx))
    _same(_call(mrt, ds, c2, t).cpu().numpy(), TC.run_reference(c2), c2["name"])


def test_no_previous_position_is_the_surfaces_own(mrt, gpu_ctx, ds):
    c = TC.random_case((33, 17), 7)
    still = dict(c); still["prev_position"] = None; still["name"] = "no previous position"
    own = dict(c); own["name"] = "own positions"
    own["prev_position"] = np.zeros((33 * 17, 4), f32); own["prev_position"][:, 0:3] = c["surfaces"]["position"]; own["prev_position"][:, 3] = np.nan          # (w is not used)
    a = _check(mrt, gpu_ctx, ds, still); b = _check(mrt, gpu_ctx, ds, own)
    _same(a, b, "NULL against the rows' own positions")
    assert not np.array_equal(a, TC.run_reference(c)) and (a[:, 3] > 1).sum() > 50


# ---------------------------------------------------------------- 3. streams and memory
def test_a_side_stream_and_the_null_stream(mrt, gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    c = TC.random_case((33, 17), 11)
    want = TC.run_reference(c)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        t = _upload(c, dev)
        warm = torch.zeros(16, device=dev) + 1.0                                                      # the torch op the calls queue behind
        got_a = _call(mrt, ds, c, t)                                                                  # stream=None: torch's current stream, the side stream
        got_b = _call(mrt, ds, c, t, stream=side)
    side.synchronize()
    assert float(warm.sum()) == 16.0
    _same(got_a.cpu().numpy(), want, "current stream"); _same(got_b.cpu().numpy(), want, "side stream")
    torch.cuda.synchronize()
    got_c = _call(mrt, ds, c, t, stream=0)
    torch.cuda.synchronize()
    _same(got_c.cpu().numpy(), want, "null stream")


def test_the_call_allocates_nothing(mrt, gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    c = TC.random_case((64, 64), 3)
    t = _upload(c, dev)
    out = torch.empty((64 * 64, 4), device=dev)
    cams = _camera(mrt, c["camera"]), _camera(mrt, c["prev_camera"])

    def call():
        ds.reproject_device(t[0], t[1], t[2], t[3], t[4], c["size"], cams[0], cams[1], prev_position=t[5], out=out)

    call()                                                                                            # the warm one
    torch.cuda.synchronize()
    first = out.clone()
    gc.collect()
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20): call()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert torch.equal(out.view(torch.int32), first.view(torch.int32)) and (out[:, 3] > 1).any()


# ---------------------------------------------------------------- 4. refusals: status, message, and nothing written
def test_refusals_leave_every_buffer_alone(mrt, gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    w, h = 16, 8
    n = w * h
    c = TC.random_case((w, h), 5)
    cam, prev = _camera(mrt, c["camera"]), _camera(mrt, c["prev_camera"])
    # one arena of float32 rows of 16 bytes, n rows of slack around every buffer: surfaces (4 n rows), position, normal | depth, ids, history, sample, out (n rows each)
    at = {"surf": n, "pos": 6 * n, "nd": 8 * n, "ids": 10 * n, "hist": 12 * n, "sample": 14 * n, "out": 16 * n}
    arena = torch.empty((18 * n + 1, 4), dtype=torch.float32, device=dev)
    arena.view(torch.int32)[:] = SENTINEL
    rows = lambda name, shift=0, count=n: arena[at[name] + shift:at[name] + shift + count]
    up = _upload(c, dev)
    rows("surf", count=4 * n).view(-1)[:] = up[0].view(-1); rows("sample")[:] = up[1]; rows("nd")[:] = up[2]; rows("ids").view(torch.int32)[:] = up[3]; rows("hist")[:] = up[4]; rows("pos")[:] = up[5]
    snapshot = arena.view(torch.int32).clone()

    def call(size=(w, h), camera=cam, prev_camera=prev, **kw):
        a = dict(surf=rows("surf", count=4 * n).view(n, 16), sample=rows("sample"), nd=rows("nd"), ids=rows("ids").view(torch.int32), hist=rows("hist"), pos=rows("pos"), out=rows("out"))
        par = {k: kw.pop(k) for k in ("max_history", "min_cos_normal", "depth_tolerance") if k in kw}
        a.update(kw)
        return ds.reproject_device(a["surf"], a["sample"], a["nd"], a["ids"], a["hist"], size, camera, prev_camera, prev_position=a["pos"], out=a["out"], **par)

    def refused(words, **kw):
        with pytest.raises(mrt.MRTError) as e: call(**kw)
        assert e.value.code == 1 and all(x in str(e.value) for x in words), (kw.keys(), str(e.value))
        torch.cuda.synchronize()
        assert torch.equal(arena.view(torch.int32), snapshot), f"{words}: a refused call wrote"

    # d_out on each input, byte ranges: its last row on the input's first, its first row on the input's last
    for name, word, count in (("surf", "d_surfaces", 4 * n), ("pos", "d_prev_position", n), ("nd", "d_prev_normal_depth", n), ("ids", "d_prev_ids", n), ("hist", "d_prev_history", n),
                              ("sample", "d_sample", n)):
        for shift in (0, 1 - n, count - 1):
            refused(("d_out overlaps " + word,), out=rows(name, shift))
    # misalignment: every buffer 4, 8 and 12 bytes off
    flat = arena.view(-1)
    off = lambda name, words, count=n: flat[at[name] * 4 + words:at[name] * 4 + words + count * 4].view(count, 4)
    for words in (1, 2, 3):
        refused(("d_surfaces", "16-byte"), surf=flat[at["surf"] * 4 + words:at["surf"] * 4 + words + 16 * n].view(n, 16))
        refused(("d_prev_position", "16-byte"), pos=off("pos", words)); refused(("d_prev_normal_depth", "16-byte"), nd=off("nd", words))
        refused(("d_prev_ids", "16-byte"), ids=off("ids", words).view(torch.int32)); refused(("d_prev_history", "16-byte"), hist=off("hist", words))
        refused(("d_sample", "16-byte"), sample=off("sample", words)); refused(("d_out", "16-byte"), out=off("out", words))
    # parameters
    for bad in (0.5, 0.0, -3.0, float("nan"), float("inf")): refused(("max_history",), max_history=bad)
    refused(("min_cos_normal",), min_cos_normal=float("nan"))
    refused(("depth_tolerance",), depth_tolerance=float("nan")); refused(("depth_tolerance",), depth_tolerance=-0.5)
    # sizes: the library's refusals, then the Python argument checks
    for size in ((0, 8), (16, 0), (-1, 8)):
        with pytest.raises(mrt.MRTError) as e: call(size=size)
        assert e.value.code == 1
    for kw in (dict(size=(8, 8)), dict(size=(16, 9)), dict(surf=rows("surf", count=4 * n).view(2 * n, 8)), dict(ids=rows("ids")), dict(hist=rows("hist")[:-1]), dict(sample=rows("sample").double()),
               dict(pos=rows("pos")[:, 0:3]), dict(out=rows("out").view(-1)), dict(camera=None), dict(prev_camera=c["prev_camera"]), dict(nd=rows("nd").cpu())):
        with pytest.raises(ValueError): call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(arena.view(torch.int32), snapshot)
    # and the call with nothing wrong writes d_out alone
    got = call()
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), TC.run_reference(c), "the arena's call")
    arena.view(torch.int32)[at["out"]:at["out"] + n] = SENTINEL
    assert torch.equal(arena.view(torch.int32), snapshot), "something but d_out was written"


# ---------------------------------------------------------------- 5. the C++ mirror
def test_cpp_mirror_temporal_host_matches_python(mrt, gpu_ctx, tmp_path):
    import torch
    dev = _dev(gpu_ctx)
    exe, out = str(tmp_path / "temporal_host"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "temporal_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    w, h = 40, 24
    p = subprocess.run([exe, str(w), str(h), out], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    raw = open(out, "rb").read()
    n = w * h
    assert len(raw) == 2 * n * 16
    sc = mrt.CornellScene((w, h))
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=1)
    try:
        dsr = r.device_scene
        hist = torch.zeros((n, 4), device=dev); nd = torch.zeros((n, 4), device=dev); ids = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        prev = sc.camera
        for f in range(2):
            cam = mrt.Camera.from_buffer_copy(sc.camera)
            cam.position.x = float(f32(cam.position.x) + f32(0.05) * f32(f)); cam.forward.x = float(f32(cam.forward.x) - f32(0.02) * f32(f))
            r.set_camera(cam); r.frameIndex = 0
            r.draw(1, wait=True)
            sample = _t(r.accumulation().reshape(-1, 4), dev)
            rays, _ = r.primary_rays_device(sample_index=0)
            surf = dsr.resolve_hits_device(rays, dsr.intersect_closest_device(rays))
            hist = dsr.reproject_device(surf, sample, nd, ids, hist, (w, h), cam, prev)
            nd, _, ids = dsr.fold_guides_device(surf, 0)
            torch.cuda.synchronize()
            assert raw[f * n * 16:(f + 1) * n * 16] == hist.cpu().numpy().tobytes(), f"frame {f}"
            prev = cam
        lens = hist[:, 3].cpu().numpy()
        on = (surf[:, 7].view(torch.int32) == 1).cpu().numpy()
        assert on.sum() > 100 and (lens[on] == 2).sum() * 2 > on.sum() and (lens[on] == 1).any() and (lens[~on] == 1).all()          # most surface pixels kept frame 0's sample
    finally:
        r.close()


# ---------------------------------------------------------------- 6. one sequence composed from the stage entries: the camera and one instance move
def test_a_composed_sequence_equals_the_reference_frame_by_frame(mrt, gpu_ctx):
    """primary_rays_device -> intersect_closest_device -> resolve_hits_device -> fold_guides_device(frame 0) -> bounce-0 direct light as the sample (scatter_device +
    intersect_any_device) -> reproject_device, six frames at 48 x 32; the camera by set_camera, the instance by set_instance_transforms_device + refit_instances_device,
    the previous positions with torch from the two poses.  Each frame's output is the reference's on the downloaded inputs, bit for bit; what
    tests/test_temporal_cpu.py shows for the CPU form of the sequence is shown here for the device's."""
    import torch
    dev = _dev(gpu_ctx)
    w, h = TC.SEQUENCE["size"]
    n = w * h
    mover = TC.SEQUENCE["mover"]
    sc = TC.sequence_scene(mrt)
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=TC.SEQUENCE["seed"], scene_options={"instancing": 1})
    try:
        dsr = r.device_scene
        hist = torch.zeros((n, 4), device=dev); nd = torch.zeros((n, 4), device=dev); ids = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        cam_prev = pose_prev = None
        for k in range(TC.SEQUENCE["frames"]):
            cam = TC.sequence_camera(mrt, sc.camera, k); pose = TC.sequence_pose(mrt, k)
            r.set_camera(cam)
            dsr.set_instance_transforms_device(mover, _t(pose.reshape(1, 16), dev)); dsr.refit_instances_device()
            rays, hidx = r.primary_rays_device(sample_index=k)
            surf = dsr.resolve_hits_device(rays, dsr.intersect_closest_device(rays))
            shadow, light, _ = dsr.scatter_device(surf, hidx, 0, next_rays=False)
            occluded = dsr.intersect_any_device(shadow)
            lit = (light[:, 3] == 1.0) & (occluded == 0)
            sample = torch.zeros((n, 4), device=dev)
            sample[:, 0:3] = torch.where(lit[:, None], light[:, 0:3] * surf[:, 8:11], torch.zeros((), device=dev))
            pp = torch.zeros((n, 4), device=dev); pp[:, 0:3] = surf[:, 0:3]
            if k:
                M = _t(TC.pose_step(pose_prev, pose), dev)
                words = surf.view(torch.int32)
                moved = (words[:, 7] == 1) & (words[:, 12] == mover)
                pp[:, 0:3] = torch.where(moved[:, None], surf[:, 0:3] @ M[0:3, 0:3].T + M[0:3, 3], surf[:, 0:3])
            prev = cam_prev if k else cam
            out = dsr.reproject_device(surf, sample, nd, ids, hist, (w, h), cam, prev, prev_position=pp)
            torch.cuda.synchronize()
            c = dict(name=f"sequence_{k}", size=(w, h), camera=T.camera_rows(cam), prev_camera=T.camera_rows(prev), surfaces=surf.cpu().numpy().view(TC.S.SURFACE_DTYPE).reshape(-1),
                     sample=sample.cpu().numpy(), prev_normal_depth=nd.cpu().numpy(), prev_ids=ids.cpu().numpy(), prev_history=hist.cpu().numpy(), prev_position=pp.cpu().numpy(),
                     params={}, checks={}, info={})
            want = TC.run_reference(c, info=c["info"])
            _same(out.cpu().numpy(), want, c["name"])
            if k:
                L = TC.sequence_losses(c)
                on = c["surfaces"]["type"] == 1
                assert (want[on, 3] > 1).sum() * 2 >= on.sum() and ((c["surfaces"]["instance_id"] == mover) & on).sum() >= 10, k
                for why in ("outside", "ids", "depth"): assert L[why].any(), (k, why)
                assert want[:, 3].max() > k and sample[:, 0:3].any()
            else:
                assert (want[:, 3] == 1).all()
            hist = out
            nd, _, ids = dsr.fold_guides_device(surf, 0)
            cam_prev, pose_prev = cam, pose
    finally:
        r.close()
