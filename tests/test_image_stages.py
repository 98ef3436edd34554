"""Guide buffers, denoiser and tonemap as stages on device buffers, on a stream (DeviceScene.fold_guides_device / denoise_device / tonemap_device).
Every comparison is on bits, as int32 views: the fold against tests/image_stages_reference.py on rows resolved on the device mixed with rows no scene would write, and
against the guide buffers Renderer(guides = 1) keeps by walking the primary rays a second time; the filter against that renderer's own and against
tests/denoise_reference.py; the tonemap against the renderer's and the reference; and a frame composed OUTSIDE the library from the stages alone (tests/paths_compose.py),
folded, filtered and tonemapped, against the RGBA8 image the renderer hands a host."""
import os
import subprocess

import numpy as np
import pytest

import denoise_reference as D
import image_stages_reference as IS
import stages_materials_reference as M
import surface_reference as S
from paths_compose import compose_fused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097)          # around a wave, around a workgroup of 256, more than one workgroup
FRAMES = (0, 1, 2, 2 ** 24 + 1)
SENTINEL = 0x7B7B7B7B


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the pool is read-only)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.size == want.size and got.shape[-1] == want.shape[-1] and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)          # (an image or its rows)
    g = got.view(np.int32 if got.dtype.itemsize == 4 else np.uint8).reshape(-1, 4); w = want.view(g.dtype).reshape(-1, 4)
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {g.shape[0]} pixels differ; first at {bad[0]}: {got.reshape(-1, 4)[bad[0]]} != {want.reshape(-1, 4)[bad[0]]}")


def _scene(mrt, name, size=None):
    if name == "cornell" and size is not None: return mrt.CornellScene(size), size, False
    w, h, instancing = (M.CASES if name == M.CORNELL else S.CASES)[name]
    return (M if name == M.CORNELL else S).make_scene(mrt, name), (w, h), instancing


@pytest.fixture(scope="module")
def renderers(mrt, gpu_ctx):
    """a Renderer with guides = 1 (and through it a committed DeviceScene) per case, made once and closed at the end of the module; the materials case draws with
    materials = 1 and four bounces"""
    made = {}

    def get(name, extra=None, size=None):
        key = (name, tuple(sorted((extra or {}).items())), size)
        if key not in made:
            sc, sz, instancing = _scene(mrt, name, size)
            o = {"instancing": 1} if instancing else {}
            o.update(extra or {})
            materials = name == M.CORNELL
            r = mrt.Renderer(sz, sc, ctx=gpu_ctx, seed=S.SEED, max_bounces=M.MAX_BOUNCES if materials else 3, scene_options=o)
            if materials: r.set_option("materials", 1)
            r.set_option("guides", 1)
            made[key] = r
        return made[key]

    yield get
    for r in made.values(): r.close()


@pytest.fixture(scope="module")
def pool(mrt, gpu_ctx, renderers):
    """(N, 16) float32 surface rows, never changed: the bounce-0 rows of three frames of CornellScene 64 x 64 resolved ON THE DEVICE, and among them rows no scene writes —
    type 0 with NaN or -1 in every other word, type 2 (not a hit) over a real hit's words, type 1 with negative ids"""
    import torch
    r = renderers("cornell")
    ds = r.device_scene
    rows = []
    for f in range(3):
        rays, _ = r.primary_rays_device(sample_index=f)
        rows.append(ds.resolve_hits_device(rays, ds.intersect_closest_device(rays)).cpu().numpy())
    torch.cuda.synchronize()
    real = np.concatenate(rows)
    kinds = real[:, 7].view(np.int32)
    assert real.shape[0] >= 3 * 4096 and 0 < (kinds == 1).sum() < kinds.size and set(np.unique(kinds).tolist()) == {0, 1}
    hits = real[kinds == 1]
    rng = np.random.default_rng(7)
    odd = hits[rng.permutation(hits.shape[0])[:1200]].copy()
    ok = odd[:, 7].view(np.int32)
    odd[0:300] = np.nan; ok[0:300] = 0                                                                  # no surface, NaN everywhere else
    odd[300:600] = -1.0; ok[300:600] = 0                                                                # no surface, -1.0f everywhere else (the miss record's distance among them)
    ok[600:900] = 2                                                                                     # not a hit, over a hit's words
    odd[900:1200, 12:15].view(np.int32)[:] = rng.integers(-2 ** 31, 0, (300, 3))                        # a hit whose ids are negative: they are carried, not interpreted
    out = np.concatenate([real, odd])
    out = out[np.random.default_rng(8).permutation(out.shape[0])]
    out.setflags(write=False)
    return out


def _fold_case(pool, n, frame, rng):
    rows = pool[rng.permutation(pool.shape[0])[:n]].copy()
    if frame == 0:
        nd = np.full((n, 4), np.nan, np.float32); al = np.full((n, 4), np.nan, np.float32)              # frame 0 reads no average
    else:
        nd = rng.standard_normal((n, 4)).astype(np.float32) * np.float32(3.0); al = rng.random((n, 4)).astype(np.float32)
    ids = np.full((n, 4), SENTINEL, np.int32)
    return rows, nd, al, ids


# ---------------------------------------------------------------- 1. the fold against the reference
@pytest.mark.parametrize("n", SIZES)
def test_fold_guides_equals_the_reference(mrt, gpu_ctx, renderers, pool, n):
    """every frame index, every kind of row: the three buffers against the reference over all their rows, and the surface rows left as they were"""
    dev = _dev(gpu_ctx)
    ds = renderers("cornell").device_scene
    rng = np.random.default_rng(100 + n)
    for frame in FRAMES:
        rows, nd, al, ids = _fold_case(pool, n, frame, rng)
        t = [_t(a, dev) for a in (rows, nd, al, ids)]
        got = ds.fold_guides_device(t[0], frame, out=t[1:])
        assert all(a is b for a, b in zip(got, t[1:]))
        want = IS.fold_guides(rows, nd, al, frame)
        for g, w, what in zip(got, want, ("normal | depth", "albedo | coverage", "ids")): _same(g.cpu().numpy(), w, f"n={n} frame={frame}: {what}")
        _same(t[0].cpu().numpy(), rows, f"n={n} frame={frame}: the surface rows")
        if n >= 255:
            kinds = rows[:, 7].view(np.int32)
            assert {0, 1, 2} <= set(kinds.tolist()) and np.isnan(rows[kinds == 0]).any() and (rows[kinds == 1][:, 12:15].view(np.int32) < 0).any()
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all(), "a row that is no surface leaked"
    fresh = ds.fold_guides_device(t[0], 0)                                                              # out=None: allocated, frame 0
    for g, w in zip(fresh, IS.fold_guides(rows, None, None, 0)): _same(g.cpu().numpy(), w, f"n={n}: fresh outputs")


def test_fold_guides_refusals(mrt, gpu_ctx, renderers, pool):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell").device_scene
    rows = _t(pool[:64], dev)
    nd, al, ids = ds.fold_guides_device(rows, 0)
    with pytest.raises(mrt.MRTError) as e: ds.fold_guides_device(rows, 1, out=(nd, nd, ids))
    assert e.value.code == 1 and "d_normal_depth" in str(e.value) and "d_albedo" in str(e.value)
    with pytest.raises(ValueError): ds.fold_guides_device(rows, 2 ** 32 - 1, out=(nd, al, ids))
    with pytest.raises(ValueError): ds.fold_guides_device(rows, 0, out=(nd, al))
    with pytest.raises(ValueError): ds.fold_guides_device(rows, 0, out=(nd, al, ids.float()))
    with pytest.raises(ValueError): ds.fold_guides_device(rows[:-1], 0, out=(nd, al, ids))
    with pytest.raises(ValueError): ds.fold_guides_device(rows[:, :8], 0)
    img = torch.zeros((4, 4, 4), device=dev)
    with pytest.raises(mrt.MRTError) as e: ds.denoise_device(img, img, img, (4, 4), out=img)
    assert e.value.code == 1 and "d_out overlaps d_image" in str(e.value)
    with pytest.raises(mrt.MRTError) as e: ds.denoise_device(img, img, img, (4, 4), iterations=9)
    assert e.value.code == 1 and "iterations must be in [1,8]" in str(e.value)
    with pytest.raises(mrt.MRTError) as e: ds.denoise_device(img, img, img, (4, 4), workspace=torch.empty(2 * 16 * 16 - 1, dtype=torch.uint8, device=dev))
    assert e.value.code == 1 and "workspace_bytes" in str(e.value)
    with pytest.raises(ValueError): ds.denoise_device(img, img, img, (4, 5))
    with pytest.raises(mrt.MRTError): ds.tonemap_device(img, (0, 4))
    with pytest.raises(ValueError): ds.tonemap_device(img, (4, 4), out=torch.empty((4, 4, 4), device=dev))


# ---------------------------------------------------------------- 2. streams and memory
def _one_of_each(torch, ds, dev, pool, rng, stream):
    """the three calls on `stream`, with every output given -> (device tensors, what the references make of the same inputs)"""
    n = 1000
    rows, nd, al, ids = _fold_case(pool, n, 3, rng)
    t = [_t(a, dev) for a in (rows, nd, al, ids)]
    ds.fold_guides_device(t[0], 3, out=t[1:], stream=stream)
    w, h = 40, 25                                                                                       # the same 1000 pixels as an image: the folded buffers guide the filter
    image = (rng.random((h, w, 4)) * 2.0).astype(np.float32)
    want_fold = IS.fold_guides(rows, nd, al, 3)
    ti = _t(image, dev)
    den = torch.empty((h, w, 4), device=dev); rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(ds.denoise_workspace_bytes((w, h)), dtype=torch.uint8, device=dev)
    ds.denoise_device(ti, t[1], t[2], (w, h), iterations=3, out=den, workspace=work, stream=stream)
    ds.tonemap_device(den, (w, h), out=rgba, stream=stream)
    want_den = D.denoise_reference(image, want_fold[0].reshape(h, w, 4), want_fold[1].reshape(h, w, 4), iterations=3)
    return t[1:] + [den, rgba], list(want_fold) + [want_den, IS.tonemap_rgba8(want_den, (w, h))]


def test_every_call_on_a_side_stream_and_on_the_null_stream(mrt, gpu_ctx, renderers, pool):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell").device_scene
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        warm = torch.zeros(16, device=dev) + 1.0                                                      # the torch op the calls queue behind
        got_a, want_a = _one_of_each(torch, ds, dev, pool, rng, None)                                 # stream=None: torch's current stream, the side stream
        got_b, want_b = _one_of_each(torch, ds, dev, pool, rng, side)
    side.synchronize()
    assert float(warm.sum()) == 16.0
    for k, (g, w) in enumerate(zip(got_a + got_b, want_a + want_b)): _same(g.cpu().numpy(), w, f"side stream, output {k}")
    torch.cuda.synchronize()
    got_c, want_c = _one_of_each(torch, ds, dev, pool, rng, 0)
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got_c, want_c)): _same(g.cpu().numpy(), w, f"null stream, output {k}")


def test_the_calls_allocate_nothing(mrt, gpu_ctx, renderers, pool):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell").device_scene
    w, h = 64, 64
    n = w * h
    rows = _t(pool[:n], dev)
    guides = (torch.empty((n, 4), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev))
    image = torch.rand((n, 4), device=dev)
    den = torch.empty((n, 4), device=dev); rgba = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
    work = torch.empty(ds.denoise_workspace_bytes((w, h)), dtype=torch.uint8, device=dev)

    def calls():
        for f in range(2): ds.fold_guides_device(rows, f, out=guides)
        ds.denoise_device(image, guides[0], guides[1], (w, h), out=den, workspace=work)
        ds.tonemap_device(den, (w, h), out=rgba)

    calls()                                                                                           # the warm ones
    torch.cuda.synchronize()
    first = rgba.clone()
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20): calls()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert torch.equal(rgba, first) and rgba[..., 0:3].any()


# ---------------------------------------------------------------- 3. the fold against the renderer: the bounce-0 rows hold what its second walk finds
RENDERER_CASES = [("cornell", None, None), ("two_level", None, None), ("cornell", {"wide": 0}, None), ("cornell", None, (37, 21))]


def _folded_guides(r, ds, frames):
    out = None
    for f in range(frames):
        rays, _ = r.primary_rays_device(sample_index=f)
        surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
        out = ds.fold_guides_device(surf, f, out=out)
    return out


@pytest.mark.parametrize("name,extra,size", RENDERER_CASES, ids=["cornell", "two_level", "rope_walk", "ragged_37x21"])
def test_four_folded_frames_equal_the_renderers_guides(mrt, gpu_ctx, renderers, name, extra, size):
    r = renderers(name, extra, size)
    ds = r.device_scene
    assert ds.stats.wide_layout == (0 if extra else 1)
    nd, al, ids = _folded_guides(r, ds, 4)
    r.frameIndex = 0
    r.draw(4, wait=True)
    g = r.guides()
    tag = f"{name} {extra} {size}"
    _same(nd.cpu().numpy(), g["normal_depth"], tag + ": normal | depth"); _same(al.cpu().numpy(), g["albedo"], tag + ": albedo | coverage"); _same(ids.cpu().numpy(), g["ids"], tag + ": ids")
    cov = g["albedo"][..., 3]
    assert (cov == 0).any() and (cov == 1).any() and ((cov > 0) & (cov < 1)).any(), tag + ": the case is vacuous"
    if name == "two_level": assert len(np.unique(g["ids"][..., 1])) >= 4


# ---------------------------------------------------------------- 4. the filter
def _drawn(mrt, gpu_ctx, scene, size, frames=3, seed=4):
    """(accumulation, guides, the renderer) of a fresh Renderer(guides = 1) after `frames` frames"""
    r = mrt.Renderer(size, scene, ctx=gpu_ctx, seed=seed)
    r.set_option("guides", 1)
    r.draw(frames, wait=True)
    return r.accumulation(), r.guides(), r


def _denoise_scenes(mrt):
    from test_denoise import _sky
    return [("cornell", (64, 64)), ("cornell", (37, 23)), ("no_dragon", (96, 54)), ("sky", (64, 48)), ("cornell", (1, 1)), ("cornell", (15, 17)), ("cornell", (17, 15)), ("cornell", (33, 9))], _sky


@pytest.mark.parametrize("k", range(8), ids=["64x64", "37x23", "96x54", "sky_64x48", "1x1", "15x17", "17x15", "33x9"])
def test_denoise_device_equals_the_renderers_filter_and_the_reference(mrt, gpu_ctx, renderers, k):
    """iterations 1, 2, 3 and 5 — the tile kernel of step 1, that of step 2 and the gather kernel, each as the last and as an inner iteration — with and without
    demodulation, on the accumulation and the guides copied out of a Renderer: that renderer's denoised(), and the numpy restatement.  One workspace and one output serve
    every call; the inputs are left as they were."""
    import torch
    dev = _dev(gpu_ctx)
    cases, sky = _denoise_scenes(mrt)
    name, size = cases[k]
    scene = sky(mrt, size) if name == "sky" else S.make_scene(mrt, name) if name == "no_dragon" else mrt.CornellScene(size)
    acc, g, r = _drawn(mrt, gpu_ctx, scene, size)
    try:
        ds = renderers("cornell").device_scene                                                          # any scene of the context: the stage reads none
        w, h = size
        if k < 4: assert (g["albedo"][..., 3] > 0).any() and acc[..., 0:3].any()
        inputs = [_t(acc, dev), _t(g["normal_depth"], dev), _t(g["albedo"], dev)]
        before = [t.clone() for t in inputs]
        work = torch.full((ds.denoise_workspace_bytes(size) + 64,), 0x7B, dtype=torch.uint8, device=dev)
        out = torch.full((h, w, 4), float("nan"), device=dev)
        for demodulate in (1, 0):
            for iterations in (1, 2, 3, 5):
                p = dict(iterations=iterations, demodulate=demodulate)
                got = ds.denoise_device(*inputs, size, out=out, workspace=work, **p)
                assert got is out
                got = got.cpu().numpy()
                _same(got, r.denoise(**p), f"{name} {size} {p}: the renderer's filter")
                q = dict(D.DEFAULTS); q.update(p)
                _same(got, D.denoise_reference(acc, g["normal_depth"], g["albedo"], **q), f"{name} {size} {p}: the restatement")
                assert (got[..., 3] == 1.0).all()
        for t, b in zip(inputs, before): assert torch.equal(t.view(torch.int32), b.view(torch.int32)), "an input was modified"
        assert (work[-64:] == 0x7B).all(), "the workspace was written past denoise_workspace_bytes"
        # defaults, a fresh workspace and output, rows instead of an image; the alpha of the image is ignored
        flat = [t.reshape(-1, 4).clone() for t in inputs]
        flat[0][:, 3] = float("nan")
        got = ds.denoise_device(*flat, size)
        assert tuple(got.shape) == (w * h, 4)
        _same(got.cpu().numpy().reshape(h, w, 4), r.denoise(), f"{name} {size}: defaults")
        p = dict(sigma_color=0.7, sigma_normal=0.1, sigma_depth=0.05, iterations=4)
        _same(ds.denoise_device(*inputs, size, **p).cpu().numpy(), r.denoise(**p), f"{name} {size} {p}")
    finally:
        r.close()


# ---------------------------------------------------------------- 5. the tonemap
@pytest.mark.parametrize("size", IS.TONEMAP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tonemap_device_equals_the_renderers_and_the_reference(mrt, gpu_ctx, renderers, size):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell").device_scene
    w, h = size
    acc, _, r = _drawn(mrt, gpu_ctx, mrt.CornellScene(size), size, frames=2)
    try:
        want = r.tonemapped()
    finally:
        r.close()
    got = ds.tonemap_device(_t(acc, dev), size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 4)
    _same(got.cpu().numpy(), want, f"{size}: the renderer's tonemap")
    _same(got.cpu().numpy(), IS.tonemap_rgba8(acc, size), f"{size}: the reference on the rendered image")
    img = IS.synthetic_image(size, IS.TONEMAP_SIZES.index(size))
    out = torch.full((h, w, 4), 0x7B, dtype=torch.uint8, device=dev)
    t = _t(img.reshape(-1, 4), dev)
    assert ds.tonemap_device(t, size, out=out) is out
    _same(out.cpu().numpy(), IS.tonemap_rgba8(img, size), f"{size}: the reference on the synthetic image")
    _same(t.cpu().numpy(), img.reshape(-1, 4), f"{size}: the image")
    if size != (1, 1): assert ((img[..., 0:3] > -1) & (img[..., 0:3] < 0)).any() and img[..., 0:3].max() == np.float32(1e6)


# ---------------------------------------------------------------- 6. end to end: camera rays to RGBA8 with no Renderer in the loop after primary_rays_device
@pytest.mark.parametrize("name", ["cornell", M.CORNELL])
def test_a_composed_frame_folded_filtered_and_tonemapped_is_the_renderers_picture(mrt, gpu_ctx, renderers, name):
    import torch
    dev = _dev(gpu_ctx)
    materials = name == M.CORNELL
    r = renderers(name)
    ds = r.device_scene
    w, h = r.size
    n = w * h
    bounces = M.MAX_BOUNCES if materials else 3
    sample = torch.zeros((n, 4), device=dev)
    accum = torch.full((n, 4), float("nan"), device=dev)
    guides = None
    for f in range(4):
        assert compose_fused(torch, r, ds, f, dev, bounces=bounces, materials=materials, radiance=sample) is sample
        ds.fold_sample_device(sample, accum, f, clear_sample=True)
        rays, _ = r.primary_rays_device(sample_index=f)                                               # the frame's bounce-0 rows once more: compose_fused keeps its own to itself
        guides = ds.fold_guides_device(ds.resolve_hits_device(rays, ds.intersect_closest_device(rays)), f, out=guides)
    den = ds.denoise_device(accum, guides[0], guides[1], (w, h))
    rgba = ds.tonemap_device(den, (w, h))
    r.frameIndex = 0
    r.draw(4, wait=True)
    want_den = r.denoise()
    _same(accum.cpu().numpy(), r.accumulation(), f"{name}: four composed frames")
    _same(den.cpu().numpy(), want_den, f"{name}: denoised")
    _same(rgba.cpu().numpy(), r.denoised_tonemapped(), f"{name}: RGBA8")
    assert rgba[..., 0:3].any() and not np.array_equal(want_den, r.accumulation())


# ---------------------------------------------------------------- 7. the C++ mirror
def test_cpp_mirror_image_stages_match_python(mrt, gpu_ctx, tmp_path):
    import torch
    dev = _dev(gpu_ctx)
    exe, out = str(tmp_path / "image_stages_host"), str(tmp_path / "out.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "image_stages_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    w, h, frames = 40, 24, 3
    p = subprocess.run([exe, str(w), str(h), str(frames), out], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    raw = open(out, "rb").read()
    n = w * h * 16
    assert len(raw) == 4 * n + w * h * 4
    r = mrt.Renderer((w, h), mrt.CornellScene((w, h)), ctx=gpu_ctx, seed=1)
    try:
        ds = r.device_scene
        nd, al, ids = _folded_guides(r, ds, frames)
        r.draw(frames, wait=True)
        den = ds.denoise_device(_t(r.accumulation(), dev), nd, al, (w, h))
        img = ds.tonemap_device(den, (w, h))
        torch.cuda.synchronize()
        assert raw[0:n] == nd.cpu().numpy().tobytes() and raw[n:2 * n] == al.cpu().numpy().tobytes() and raw[2 * n:3 * n] == ids.cpu().numpy().tobytes()
        assert raw[3 * n:4 * n] == den.cpu().numpy().tobytes() and raw[4 * n:] == img.cpu().numpy().tobytes()
        assert any(raw[4 * n:])
    finally:
        r.close()
