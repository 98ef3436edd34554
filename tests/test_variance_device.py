"""The variance-guided a-trous filter and the sample image of its moments on device buffers, on a stream (DeviceScene.moments_sample_device,
DeviceScene.denoise_variance_device).  Every comparison is on bits, as int32 views, against tests/variance_reference.py fed the same inputs: the
known-answer cases of tests/variance_cases.py, random images with every feature present at sizes around a tile and a workgroup, on non-square images and on single rows,
at 1, 2, 3 and 5 iterations (both tile steps, the first direct step, halos wider than the image), both streams, every refusal with the outputs left alone, and one
sequence composed from the stage entries whose moments equal the reference's fed the downloaded inputs and whose filtered image is nearer the converged one."""
import gc

import numpy as np
import pytest

import temporal_cases as TC
import temporal_reference as T
import variance_cases as VC
import variance_reference as V

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B7B7B
f32 = np.float32
ITERATIONS = (1, 2, 3, 5)
SIZES = [(16, 8), (17, 17), (33, 17), (64, 64), (15, 33), (1, 1), (63, 1), (64, 1), (65, 1), (257, 1)]


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _same(got, want, what, where=None):
    g = np.ascontiguousarray(got).view(np.int32).reshape(-1, 4); w = np.ascontiguousarray(want, f32).view(np.int32).reshape(-1, 4)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    differ = (g != w).any(-1) if where is None else (g != w).any(-1) & where.reshape(-1)
    if differ.any():
        bad = np.flatnonzero(differ)
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at {bad[0]}: {np.asarray(got).reshape(-1, 4)[bad[0]]} != {np.asarray(want).reshape(-1, 4)[bad[0]]}")


@pytest.fixture(scope="module")
def ds(mrt, gpu_ctx):
    """any committed scene of the context: the stages read none"""
    r = mrt.Renderer((16, 16), mrt.CornellScene((16, 16)), ctx=gpu_ctx, seed=1)
    yield r.device_scene
    r.close()


def _upload(c, dev):
    return [_t(c[k], dev) for k in ("image", "moments", "normal_depth", "albedo")]


def _size(c):
    return c["image"].shape[1], c["image"].shape[0]


def _check(gpu_ctx, ds, c, name, iterations=ITERATIONS, **kw):
    """the filter of a case at each iteration count against the reference, every word; the inputs come back unmodified"""
    import torch
    dev = _dev(gpu_ctx)
    t = _upload(c, dev)
    before = [x.clone() for x in t]
    out = torch.full(c["image"].shape, float("nan"), device=dev)
    work = torch.empty(ds.denoise_workspace_bytes(_size(c)), dtype=torch.uint8, device=dev)
    for it in iterations:
        assert ds.denoise_variance_device(*t, _size(c), iterations=it, out=out, workspace=work, **kw) is out
        _same(out.cpu().numpy(), VC.run(c, iterations=it, **kw), f"{name}, {it} iterations")
    for x, b in zip(t, before): assert torch.equal(x.view(torch.int32), b.view(torch.int32)), f"{name}: an input was modified"


# ---------------------------------------------------------------- 1. the cases whose answers are known
@pytest.mark.parametrize("name,c", VC.known_answer_cases(), ids=[n for n, _ in VC.known_answer_cases()])
def test_known_answers_equal_the_reference(gpu_ctx, ds, name, c):
    if name == "nan_behind_uncovered":
        # the pixels that are not covered hold NaN and pass through as NaN; every covered word is the reference's
        import torch
        t = _upload(c, _dev(gpu_ctx))
        un = c["albedo"][..., 3] == 0
        for it in ITERATIONS:
            got = ds.denoise_variance_device(*t, _size(c), iterations=it).cpu().numpy()
            _same(got, VC.run(c, iterations=it), f"{name}, {it} iterations", where=~un)
            assert np.isnan(got[un][:, 0:3]).all() and (got[..., 3] == 1).all() and np.isfinite(got[~un]).all()
        return
    _check(gpu_ctx, ds, c, name)
    if name == "flat_v1":          # (what tests/test_variance_cpu.py holds the reference to)
        assert np.array_equal(VC.run(c, iterations=1)[..., 0:3], c["image"][..., 0:3])


# ---------------------------------------------------------------- 2. random images: around a tile and a workgroup, non-square ones, single rows
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_images_equal_the_reference(gpu_ctx, ds, size):
    c = VC.random_case(size, 100 + size[0])                                                             # (tests/test_variance_cpu.py: every feature is in them)
    _check(gpu_ctx, ds, c, f"random {size}")
    if size in ((33, 17), (15, 33)):
        _check(gpu_ctx, ds, c, f"random {size}, other parameters", iterations=(2, 4), sigma_color=1.5, sigma_normal=0.5, sigma_depth=0.1)
        _check(gpu_ctx, ds, c, f"random {size}, demodulate = 0", iterations=(1, 3), demodulate=0)


def test_flat_rows_as_images(gpu_ctx, ds):
    """(h * w, 4) tensors are the same images"""
    c = VC.random_case((33, 17), 9)
    t = [x.reshape(-1, 4) for x in _upload(c, _dev(gpu_ctx))]
    out = ds.denoise_variance_device(*t, (33, 17), iterations=3)
    assert tuple(out.shape) == (33 * 17, 4)
    _same(out.cpu().numpy(), VC.run(c, iterations=3), "rows")


# ---------------------------------------------------------------- 3. the moments' sample image
@pytest.mark.parametrize("size", [(33, 17), (1, 1), (255, 1), (256, 1), (257, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_sample_equals_the_reference(gpu_ctx, ds, size):
    import torch
    dev = _dev(gpu_ctx)
    c = VC.random_case(size, 7)
    sample, alb = _t(c["image"], dev), _t(c["albedo"], dev)
    out = torch.full(c["image"].shape, float("nan"), device=dev)
    assert ds.moments_sample_device(sample, alb, size, out=out) is out
    _same(out.cpu().numpy(), V.moments_sample(c["image"], c["albedo"]), "moments sample")
    _same(ds.moments_sample_device(sample, alb, size, demodulate=0).cpu().numpy(), V.moments_sample(c["image"], c["albedo"], 0), "moments sample, demodulate = 0")
    assert torch.equal(sample.view(torch.int32), _t(c["image"], dev).view(torch.int32)) and torch.equal(alb.view(torch.int32), _t(c["albedo"], dev).view(torch.int32))


# ---------------------------------------------------------------- 4. streams and memory
def test_a_side_stream_and_the_null_stream(gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    c = VC.random_case((33, 17), 11)
    want = VC.run(c); want_ms = V.moments_sample(c["image"], c["albedo"])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        t = _upload(c, dev)
        warm = torch.zeros(16, device=dev) + 1.0                                                      # the torch op the calls queue behind
        got_a = ds.denoise_variance_device(*t, (33, 17))                                              # stream=None: torch's current stream, the side stream
        got_b = ds.denoise_variance_device(*t, (33, 17), stream=side)
        ms_a = ds.moments_sample_device(t[0], t[3], (33, 17), stream=side)
    side.synchronize()
    assert float(warm.sum()) == 16.0
    _same(got_a.cpu().numpy(), want, "current stream"); _same(got_b.cpu().numpy(), want, "side stream"); _same(ms_a.cpu().numpy(), want_ms, "sample, side stream")
    torch.cuda.synchronize()
    got_c = ds.denoise_variance_device(*t, (33, 17), stream=0); ms_c = ds.moments_sample_device(t[0], t[3], (33, 17), stream=0)
    torch.cuda.synchronize()
    _same(got_c.cpu().numpy(), want, "null stream"); _same(ms_c.cpu().numpy(), want_ms, "sample, null stream")


def test_the_calls_allocate_nothing(gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    c = VC.random_case((64, 64), 3)
    t = _upload(c, dev)
    out = torch.empty((64, 64, 4), device=dev); ms = torch.empty((64, 64, 4), device=dev)
    work = torch.empty(ds.denoise_workspace_bytes((64, 64)), dtype=torch.uint8, device=dev)

    def call():
        ds.moments_sample_device(t[0], t[3], (64, 64), out=ms)
        ds.denoise_variance_device(*t, (64, 64), out=out, workspace=work)

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
    assert torch.equal(out.view(torch.int32), first.view(torch.int32))
    _same(out.cpu().numpy(), VC.run(c), "after 20 calls")


# ---------------------------------------------------------------- 5. refusals: status, message, and nothing written
def test_refusals_leave_every_buffer_alone(mrt, gpu_ctx, ds):
    import torch
    dev = _dev(gpu_ctx)
    w, h = 16, 8
    n = w * h
    c = VC.random_case((w, h), 5)
    # one arena of float32 rows of 16 bytes, 2 n rows of slack before every input and n around the others: image, moments, normal | depth, albedo, out (n rows each), the workspace (2 n rows)
    at = {"image": 2 * n, "moments": 5 * n, "nd": 8 * n, "albedo": 11 * n, "out": 14 * n, "work": 16 * n}
    arena = torch.empty((19 * n + 1, 4), dtype=torch.float32, device=dev)
    arena.view(torch.int32)[:] = SENTINEL
    rows = lambda name, shift=0, count=n: arena[at[name] + shift:at[name] + shift + count]
    for name, x in zip(("image", "moments", "nd", "albedo"), _upload(c, dev)): rows(name)[:] = x.reshape(-1, 4)
    snapshot = arena.view(torch.int32).clone()
    bytes_of = lambda t: t.reshape(-1).view(torch.uint8)

    def call(size=(w, h), **kw):
        a = dict(image=rows("image"), moments=rows("moments"), nd=rows("nd"), albedo=rows("albedo"), out=rows("out"), work=bytes_of(rows("work", count=2 * n)))
        par = {k: kw.pop(k) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_depth", "demodulate") if k in kw}
        a.update(kw)
        return ds.denoise_variance_device(a["image"], a["moments"], a["nd"], a["albedo"], size, out=a["out"], workspace=a["work"], **par)

    def sample(size=(w, h), **kw):
        a = dict(image=rows("image"), albedo=rows("albedo"), out=rows("out")); a.update(kw)
        return ds.moments_sample_device(a["image"], a["albedo"], size, out=a["out"])

    def refused(fn, words, **kw):
        with pytest.raises(mrt.MRTError) as e: fn(**kw)
        assert e.value.code == 1 and all(x in str(e.value) for x in words), (kw.keys(), str(e.value))
        torch.cuda.synchronize()
        assert torch.equal(arena.view(torch.int32), snapshot), f"{words}: a refused call wrote"

    # d_out and the workspace on each input, byte ranges: the last row on the input's first, the first row on the input's last
    for name, word in (("image", "d_image"), ("moments", "d_moments"), ("nd", "d_normal_depth"), ("albedo", "d_albedo")):
        for shift in (0, 1 - n, n - 1): refused(call, ("d_out overlaps " + word,), out=rows(name, shift))
        for shift in (0, 1 - 2 * n, n - 1): refused(call, ("d_workspace overlaps " + word,), work=bytes_of(rows(name, shift, 2 * n)))
    for shift in (0, 1 - n, 2 * n - 1): refused(call, ("d_out overlaps d_workspace",), out=rows("work", shift))
    for name, word in (("image", "d_sample"), ("albedo", "d_albedo")):
        for shift in (0, 1 - n, n - 1): refused(sample, ("d_out overlaps " + word,), out=rows(name, shift))
    # misalignment: every buffer 4, 8 and 12 bytes off
    flat = arena.view(-1)
    off = lambda name, words, count=n: flat[at[name] * 4 + words:at[name] * 4 + words + count * 4].view(count, 4)
    for words in (1, 2, 3):
        for key, word in (("image", "d_image"), ("moments", "d_moments"), ("nd", "d_normal_depth"), ("albedo", "d_albedo"), ("out", "d_out")):
            refused(call, (word, "16-byte"), **{key: off(key, words)})
        refused(call, ("d_workspace", "16-byte"), work=bytes_of(off("work", words, 2 * n)))
        refused(sample, ("d_sample", "16-byte"), image=off("image", words)); refused(sample, ("d_albedo", "16-byte"), albedo=off("albedo", words)); refused(sample, ("d_out", "16-byte"), out=off("out", words))
    # the workspace too small; parameters
    refused(call, ("workspace_bytes",), work=bytes_of(rows("work", count=2 * n))[:-1])
    for bad in (0, 9, -1): refused(call, ("iterations",), iterations=bad)
    for key in ("sigma_color", "sigma_normal", "sigma_depth"):
        for bad in (0.0, -2.0, float("nan"), float("inf")): refused(call, (key,), **{key: bad})
    refused(call, ("demodulate",), demodulate=2)
    # sizes: the library's refusals, then the Python argument checks
    for fn in (call, sample):
        for size in ((0, 8), (16, 0), (-1, 8)):
            with pytest.raises(mrt.MRTError) as e: fn(size=size)
            assert e.value.code == 1
        for kw in (dict(size=(8, 8)), dict(size=(16, 9)), dict(image=rows("image")[:-1]), dict(albedo=rows("albedo").double()), dict(out=rows("out").view(-1)), dict(image=rows("image").cpu()),
                   dict(out=rows("out").view(h, w, 4))):
            with pytest.raises(ValueError): fn(**kw)
    with pytest.raises(ValueError): call(work=rows("work", count=2 * n))
    with pytest.raises(ValueError): call(moments=rows("moments")[:, 0:3])
    torch.cuda.synchronize()
    assert torch.equal(arena.view(torch.int32), snapshot)
    # and the calls with nothing wrong write d_out (and the workspace) alone
    got = sample().clone()
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), V.moments_sample(c["image"], c["albedo"]), "the arena's sample")
    got = call()
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), VC.run(c), "the arena's call")
    arena.view(torch.int32)[at["out"]:at["out"] + n] = SENTINEL; arena.view(torch.int32)[at["work"]:at["work"] + 2 * n] = SENTINEL
    assert torch.equal(arena.view(torch.int32), snapshot), "something but d_out and the workspace was written"


# ---------------------------------------------------------------- 6. one sequence composed from the stage entries: colour and moments, then the filter
def _direct_light(dsr, r, k, n, dev):
    """frame k's bounce-0 rows and its sample: direct light through one shadow ray per pixel, as tests/test_temporal_device.py composes it"""
    import torch
    rays, hidx = r.primary_rays_device(sample_index=k)
    surf = dsr.resolve_hits_device(rays, dsr.intersect_closest_device(rays))
    shadow, light, _ = dsr.scatter_device(surf, hidx, 0, next_rays=False)
    lit = (light[:, 3] == 1.0) & (dsr.intersect_any_device(shadow) == 0)
    sample = torch.zeros((n, 4), device=dev)
    sample[:, 0:3] = torch.where(lit[:, None], light[:, 0:3] * surf[:, 8:11], torch.zeros((), device=dev))
    return surf, sample


def test_a_composed_sequence_its_moments_and_the_filtered_image(mrt, gpu_ctx):
    """tests/test_temporal_device.py's six frames at 48 x 32 — the camera and one instance move — with the moments beside the colour: moments_sample_device, then a
    second reproject_device call with the same arguments.  Each frame's sample image and moments equal the references fed the downloaded inputs, bit for bit, and carry
    the colour's history length.  Then the last frame through denoise_variance_device: the reference's bits, and nearer the converged image (128 more samples at the
    last camera and pose, averaged) than the unfiltered accumulation."""
    import torch
    dev = _dev(gpu_ctx)
    w, h = TC.SEQUENCE["size"]
    n = w * h
    mover = TC.SEQUENCE["mover"]
    sc = TC.sequence_scene(mrt)
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=TC.SEQUENCE["seed"], scene_options={"instancing": 1})
    try:
        dsr = r.device_scene
        hist = torch.zeros((n, 4), device=dev); mom = torch.zeros((n, 4), device=dev); nd = torch.zeros((n, 4), device=dev); ids = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        cam_prev = pose_prev = None
        for k in range(TC.SEQUENCE["frames"]):
            cam = TC.sequence_camera(mrt, sc.camera, k); pose = TC.sequence_pose(mrt, k)
            r.set_camera(cam)
            dsr.set_instance_transforms_device(mover, _t(pose.reshape(1, 16), dev)); dsr.refit_instances_device()
            surf, sample = _direct_light(dsr, r, k, n, dev)
            pp = torch.zeros((n, 4), device=dev); pp[:, 0:3] = surf[:, 0:3]
            if k:
                M = _t(TC.pose_step(pose_prev, pose), dev)
                words = surf.view(torch.int32)
                moved = (words[:, 7] == 1) & (words[:, 12] == mover)
                pp[:, 0:3] = torch.where(moved[:, None], surf[:, 0:3] @ M[0:3, 0:3].T + M[0:3, 3], surf[:, 0:3])
            prev = cam_prev if k else cam
            nd_k, al_k, ids_k = dsr.fold_guides_device(surf, 0)
            ms = dsr.moments_sample_device(sample, al_k, (w, h))
            out = dsr.reproject_device(surf, sample, nd, ids, hist, (w, h), cam, prev, prev_position=pp)
            out_m = dsr.reproject_device(surf, ms, nd, ids, mom, (w, h), cam, prev, prev_position=pp)
            torch.cuda.synchronize()
            want_ms = V.moments_sample(sample.cpu().numpy(), al_k.cpu().numpy())
            _same(ms.cpu().numpy(), want_ms, f"sample image {k}")
            want_m = T.reproject((w, h), T.camera_rows(cam), T.camera_rows(prev), surf.cpu().numpy().view(TC.S.SURFACE_DTYPE).reshape(-1), want_ms, nd.cpu().numpy(), ids.cpu().numpy(),
                                 mom.cpu().numpy(), prev_position=pp.cpu().numpy())
            _same(out_m.cpu().numpy(), want_m, f"moments {k}")
            assert torch.equal(out_m[:, 3], out[:, 3]) and not out_m[:, 2].any()
            hist, mom, nd, ids = out, out_m, nd_k, ids_k
            cam_prev, pose_prev = cam, pose
        lens = hist[:, 3].cpu().numpy(); covered = al_k[:, 3].cpu().numpy() != 0
        assert (lens[covered] >= 4).sum() > 300 and (lens[covered] < 4).sum() > 50 and (~covered).sum() > 300          # both variance estimates are in the frame
        filtered = dsr.denoise_variance_device(hist, mom, nd_k, al_k, (w, h))
        torch.cuda.synchronize()
        img = lambda t: VC.as_image(t.cpu().numpy(), (w, h))
        _same(filtered.cpu().numpy(), V.denoise_variance(img(hist), img(mom), img(nd_k), img(al_k)), "the filtered frame")
        converged = torch.zeros((n, 4), device=dev)
        for j in range(128):
            converged += _direct_light(dsr, r, 1000 + j, n, dev)[1]
        converged /= 128.0
        e_new, e_hist = TC.rmse(filtered.cpu().numpy(), converged.cpu().numpy()), TC.rmse(hist.cpu().numpy(), converged.cpu().numpy())
        print(f"RMSE against 128 samples at the last camera: reprojected {e_hist:.4f}, variance-guided {e_new:.4f}")
        assert e_new < e_hist, (e_new, e_hist)
    finally:
        r.close()
