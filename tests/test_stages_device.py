"""The path-tracing stages on device buffers, on a stream (Renderer.primary_rays_device / DeviceScene.scatter_device).  Every comparison is on bits: each
stage against tests/stages_reference.py (pinned to the oracle's stage dumps and image by tests/test_stages_device_cpu.py), and a path tracer composed OUTSIDE the library
from its five public stages and torch element-wise ops against the image Renderer draws of the same scene, seed and camera."""
import os
import re
import subprocess

import numpy as np
import pytest

import stages_reference as R
import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 5
TWO = {"instancing": 1}
SIZES = {"cornell": (64, 64), "two_level": (64, 48), R.FOUR_LIGHTS: R.CASES[R.FOUR_LIGHTS][:2]}


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_dev(ctx))


def _surf_t(surf, ctx):
    return _t(np.ascontiguousarray(surf).view(np.float32).reshape(-1, 16), ctx)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(got.shape[0], -1) != want.view(np.uint32).reshape(want.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ; first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _options(c, extra=None):
    o = dict(TWO) if c["instancing"] else {}
    o.update(extra or {})
    return o


@pytest.fixture(scope="module")
def renderers(mrt, orc, gpu_ctx):
    """a Renderer (and through it a committed DeviceScene) per (case, scene options), made once and closed at the end of the module"""
    made = {}

    def get(name, extra=None):
        key = (name, tuple(sorted((extra or {}).items())))
        if key not in made:
            c = R.scene_case(mrt, orc, name)
            assert (c["w"], c["h"]) == SIZES[name]
            made[key] = mrt.Renderer((c["w"], c["h"]), c["scene"], ctx=gpu_ctx, seed=S.SEED, scene_options=_options(c, extra))
        return made[key]

    yield get
    for r in made.values(): r.close()


# ---------------------------------------------------------------- 1. each stage against the reference
def test_primary_rays_equal_the_reference(mrt, orc, gpu_ctx):
    """sample index 0, 5 and 2^32 - 3 (the wrap), a large and a negative index; then another camera; then 9 x 1 and 1 x 1 images"""
    w, h = SIZES["cornell"]
    scene = R.make_scene(mrt, "cornell")                                              # (its own: drawableSizeWillChange moves the scene's camera)
    r = mrt.Renderer((w, h), scene, ctx=gpu_ctx, seed=S.SEED)
    try:
        base = R.halton_index(orc, S.SEED, w * h, 0)
        assert base.min() >= 3 and base.max() < 2 ** 20
        # 2^32 - 3: the sum wraps to the seed - 3; 2^22 + 1: beyond the fast digit extraction of halton_dev; 2^31 + 7: every index negative, Halton value 0
        for si in (0, 5, 2 ** 32 - 3, 2 ** 22 + 1, 2 ** 31 + 7):
            rays, idx = r.primary_rays_device(sample_index=si)
            want_r, want_i = R.primary_rays(orc, scene.camera, w, h, S.SEED, si)
            assert tuple(rays.shape) == (w * h, 8) and tuple(idx.shape) == (w * h,)
            _same(idx.cpu().numpy(), want_i, f"halton index at sample {si}"); _same(rays.cpu().numpy(), want_r, f"rays at sample {si}")
            if si == 2 ** 32 - 3: assert np.array_equal(want_i, base - 3)
            if si == 2 ** 31 + 7: assert (want_i < 0).all()
        r.frameIndex = 5
        _same(r.primary_rays_device()[0].cpu().numpy(), R.primary_rays(orc, scene.camera, w, h, S.SEED, 5)[0], "sample_index=None is the frame index")
        assert r.frameIndex == 5
        cam = mrt.Camera(); cam.position = mrt.Float3(0.3, 1.2, 4.0); cam.right = mrt.Float3(0.5, 0.0, 0.1); cam.up = mrt.Float3(0.0, 0.4, 0.05); cam.forward = mrt.Float3(-0.1, -0.05, -1.0)
        r.set_camera(cam)
        _same(r.primary_rays_device(sample_index=1)[0].cpu().numpy(), R.primary_rays(orc, cam, w, h, S.SEED, 1)[0], "after set_camera")
        for size in ((9, 1), (1, 1)):
            r.drawableSizeWillChange(size)
            rays, idx = r.primary_rays_device(sample_index=2)
            want_r, want_i = R.primary_rays(orc, r.scene.camera, size[0], size[1], S.SEED, 2)
            _same(idx.cpu().numpy(), want_i, f"halton index at {size}"); _same(rays.cpu().numpy(), want_r, f"rays at {size}")
    finally:
        r.close()


@pytest.mark.parametrize("name,extra", [("cornell", None), ("two_level", None), (R.FOUR_LIGHTS, None)])
def test_scatter_equals_the_reference_on_every_bounce(mrt, orc, gpu_ctx, renderers, name, extra):
    """surfaces resolved ON THE DEVICE from the oracle-dumped rays of each bounce; the Halton index of each ray's pixel"""
    c = R.scene_case(mrt, orc, name)
    d = R.dump_case(mrt, orc, name, 0)
    ds = renderers(name, extra).device_scene
    hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)
    picked = set()
    for b in range(3):
        rays = _t(d["rays"][b], gpu_ctx)
        surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
        h = _t(hidx[d["pixels"][b]], gpu_ctx)
        sh, light, nxt = ds.scatter_device(surf, h, b)
        want = R.scatter(orc, mrt.unpack_surfaces(surf), hidx[d["pixels"][b]], b, c["scene"].lights)
        assert (want["light"][:, 3] == 1).any() and (mrt.unpack_surfaces(surf)["type"] == 1).any()
        _same(light.cpu().numpy(), want["light"], f"{name} bounce {b}: light"); _same(sh.cpu().numpy(), want["shadow_rays"], f"{name} bounce {b}: shadow rays")
        _same(nxt.cpu().numpy(), want["next_rays"], f"{name} bounce {b}: next rays")
        picked |= set(want["light_index"][want["light_index"] >= 0].tolist())
    if name == R.FOUR_LIGHTS: assert picked == {0, 1, 2, 3}


def test_light_count_and_no_next_rays(mrt, orc, gpu_ctx, renderers):
    import torch
    c = R.scene_case(mrt, orc, R.FOUR_LIGHTS)
    d = R.dump_case(mrt, orc, R.FOUR_LIGHTS, 0)
    ds = renderers(R.FOUR_LIGHTS).device_scene
    hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)[d["pixels"][1]]
    rays = _t(d["rays"][1], gpu_ctx)
    surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
    h = _t(hidx, gpu_ctx)
    full = ds.scatter_device(surf, h, 1)
    for lc in (1, 2, 4):
        sh, light, nxt = ds.scatter_device(surf, h, 1, light_count=lc)
        want = R.scatter(orc, mrt.unpack_surfaces(surf), hidx, 1, c["scene"].lights, light_count=lc)
        _same(light.cpu().numpy(), want["light"], f"light_count {lc}: light"); _same(sh.cpu().numpy(), want["shadow_rays"], f"light_count {lc}: shadow rays")
        assert torch.equal(nxt.view(torch.int32), full[2].view(torch.int32))
        assert want["light_index"].max() == min(lc - 1, 3) if lc < 4 else True
    assert torch.equal(ds.scatter_device(surf, h, 1, light_count=4)[1].view(torch.int32), full[1].view(torch.int32))
    assert not torch.equal(ds.scatter_device(surf, h, 1, light_count=1)[1].view(torch.int32), full[1].view(torch.int32))
    # next_rays=False: two outputs, the same bits, and a third buffer given all the same is refused rather than half used
    sh, light, none = ds.scatter_device(surf, h, 1, next_rays=False)
    assert none is None and torch.equal(sh.view(torch.int32), full[0].view(torch.int32)) and torch.equal(light.view(torch.int32), full[1].view(torch.int32))
    with pytest.raises(ValueError): ds.scatter_device(surf, h, 1, next_rays=False, out=(sh, light, full[2]))
    with pytest.raises(mrt.MRTError) as e: ds.scatter_device(surf, h, 1, light_count=5)
    assert e.value.code == INVALID and "light_count" in str(e.value)


# ---------------------------------------------------------------- 2. the composed integrator
def _compose(mrt, r, ds, sample_index, gpu_ctx, stream=None):
    """One frame of the reference's integrator from the five public stages, three bounces, dense rows; throughput and radiance are separate torch mul / add / where ops (no
    fused multiply-add anywhere).  -> the frame's radiance sample, torch (n, 3) float32"""
    import torch
    dev = _dev(gpu_ctx)
    rays, hidx = r.primary_rays_device(sample_index=sample_index, stream=stream)
    n = rays.shape[0]
    thr = torch.ones((n, 3), device=dev); acc = torch.zeros((n, 3), device=dev); alive = torch.ones(n, dtype=torch.bool, device=dev)
    miss = _surf_t(np.array([S.miss_record()]), gpu_ctx)
    for b in range(3):
        hits = ds.intersect_closest_device(rays, stream=stream)
        surf = ds.resolve_hits_device(rays, hits, stream=stream)
        alive = alive & (surf[:, 7].view(torch.int32) == 1)                           # a miss ends the path: its rows stay the miss record from here on
        surf = torch.where(alive[:, None], surf, miss).contiguous()
        shadow, light, nxt = ds.scatter_device(surf, hidx, b, next_rays=b < 2, stream=stream)
        occluded = ds.intersect_any_device(shadow, stream=stream)
        thr = torch.mul(thr, surf[:, 8:11])                                           # :339
        lit = alive & (light[:, 3] == 1.0) & (occluded == 0)                          # by light.w and the surface's type, never by the answer for a zero ray alone
        acc = torch.where(lit[:, None], torch.add(acc, torch.mul(light[:, 0:3], thr)), acc)   # :371-373
        rays = nxt
    return acc


def _image(acc, w, h):
    a = acc.cpu().numpy() if not isinstance(acc, np.ndarray) else acc
    return np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], 1).reshape(h, w, 4)


@pytest.mark.parametrize("name,extra", [("cornell", None), ("two_level", None), ("cornell", {"wide": 0})])
def test_composed_integrator_draws_the_renderers_image(mrt, orc, gpu_ctx, renderers, name, extra):
    """On a side stream behind a torch op, no host wait between the stages.  Frame 0: the bits of Renderer.accumulation().  Four frames: the per-frame samples folded with
    the reference's running average in numpy float32 (torch's divide stays out of the claim)."""
    import torch
    c = R.scene_case(mrt, orc, name)
    w, h = c["w"], c["h"]
    r = renderers(name, extra)
    ds = r.device_scene
    assert ds.stats.wide_layout == (0 if extra else 1)
    side = torch.cuda.Stream(device=_dev(gpu_ctx))
    side.wait_stream(torch.cuda.current_stream(_dev(gpu_ctx)))
    with torch.cuda.stream(side):
        warm = torch.zeros(16, device=_dev(gpu_ctx)) + 1.0                            # the torch op the stages queue behind
        samples = [_compose(mrt, r, ds, f, gpu_ctx) for f in range(4)]                # stream=None: torch's current stream, the side stream
    side.synchronize()
    assert float(warm.sum()) == 16.0
    r.frameIndex = 0
    r.draw(1, wait=True)
    _same(_image(samples[0], w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: frame 0")
    assert samples[0].any()
    r.draw(3, wait=True)
    assert r.frameIndex == 4
    folded = R.running_average([s.cpu().numpy() for s in samples])
    _same(_image(folded, w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: four frames")


# ---------------------------------------------------------------- 3. launch edges
def test_launch_edges(mrt, orc, gpu_ctx, renderers):
    import torch
    c = R.scene_case(mrt, orc, "cornell")
    d = R.dump_case(mrt, orc, "cornell", 0)
    ds = renderers("cornell").device_scene
    m = 300
    surf_np = np.array(d["surfaces"][1][:m])
    assert (surf_np["type"][1::2] == 1).sum() > 50
    surf_np[::2] = S.miss_record()                                                    # every second surface is the miss record
    hidx_np = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)[d["pixels"][1][:m]]
    surf, hidx = _surf_t(surf_np, gpu_ctx), _t(hidx_np, gpu_ctx)
    full = ds.scatter_device(surf, hidx, 1)
    want = R.scatter(orc, surf_np, hidx_np, 1, c["scene"].lights)
    for got, k in zip(full, ("shadow_rays", "light", "next_rays")):
        _same(got.cpu().numpy(), want[k], k)
        assert not got.cpu().numpy()[::2].view(np.uint32).any(), k                    # zero rows between untouched valid neighbours
    assert want["light"][1::2, 3].any() and want["next_rays"][1::2].any()
    for n in (0, 1, 63, 64, 65, 257):
        got = ds.scatter_device(surf[:n], hidx[:n], 1)                                # out not given
        assert [tuple(g.shape) for g in got] == [(n, 8), (n, 4), (n, 8)]
        out = tuple(torch.full(sh, 7.0, device=_dev(gpu_ctx)) for sh in ((n, 8), (n, 4), (n, 8)))
        ret = ds.scatter_device(surf[:n], hidx[:n], 1, out=out)
        for g, o, rt, f in zip(got, out, ret, full):
            assert rt is o and torch.equal(g.view(torch.int32), f[:n].view(torch.int32)) and torch.equal(o.view(torch.int32), f[:n].view(torch.int32)), n
        two = tuple(torch.full(sh, 7.0, device=_dev(gpu_ctx)) for sh in ((n, 8), (n, 4)))
        assert ds.scatter_device(surf[:n], hidx[:n], 1, next_rays=False, out=two)[2] is None and torch.equal(two[1].view(torch.int32), full[1][:n].view(torch.int32))
    # the rows past n are left alone
    big = tuple(torch.full(sh, 7.0, device=_dev(gpu_ctx)) for sh in ((66, 8), (66, 4), (66, 8)))
    ds.scatter_device(surf[:65], hidx[:65], 1, out=tuple(b[:65] for b in big))
    assert all(bool((b[65] == 7.0).all()) for b in big)
    # the null stream, and the renderer's entry with out= given
    torch.cuda.synchronize()
    s0 = ds.scatter_device(surf, hidx, 1, stream=0)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), f.view(torch.int32)) for a, f in zip(s0, full))
    r = renderers("cornell")
    n = c["w"] * c["h"]
    a = r.primary_rays_device(sample_index=3)
    out = (torch.full((n, 8), 7.0, device=_dev(gpu_ctx)), torch.full((n,), 7, dtype=torch.int32, device=_dev(gpu_ctx)))
    b = r.primary_rays_device(sample_index=3, out=out, stream=0)
    torch.cuda.synchronize()
    assert b[0] is out[0] and b[1] is out[1] and torch.equal(a[0].view(torch.int32), out[0].view(torch.int32)) and torch.equal(a[1], out[1])
    with pytest.raises(ValueError): r.primary_rays_device(out=(out[0][:-1], out[1]))
    with pytest.raises(ValueError): ds.scatter_device(surf, hidx[:-1], 1)
    with pytest.raises(ValueError): ds.scatter_device(surf.to(torch.int32), hidx, 1)


def test_refusals_on_a_live_scene(mrt, orc, gpu_ctx, renderers):
    import ctypes as C
    import torch
    ds = renderers("cornell").device_scene
    lib, P = mrt.lib, C.c_void_p
    dev = _dev(gpu_ctx)
    surf = torch.zeros((4, 16), device=dev); hidx = torch.zeros(4, dtype=torch.int32, device=dev); sh = torch.zeros((4, 8), device=dev); li = torch.zeros((4, 4), device=dev)

    def call(scene=ds.handle, n=4, bounce=0, lc=0, s=surf.data_ptr(), l=li.data_ptr()):
        return lib.mrt_scene_scatter_device(scene, P(s), P(hidx.data_ptr()), n, bounce, lc, P(sh.data_ptr()), P(l), None, None)

    assert call() == 0 and call(n=0) == 0
    assert lib.mrt_scene_scatter_device(ds.handle, None, None, 0, 0, 0, None, None, None, None) == 0
    assert call(lc=2) == INVALID and "light_count" in lib.mrt_last_error().decode()   # the Cornell box has one light
    assert call(lc=1) == 0
    assert call(s=surf.data_ptr() + 8) == INVALID and call(l=li.data_ptr() + 4) == INVALID and call(bounce=19) == INVALID and call(bounce=-1) == INVALID
    torch.cuda.synchronize()
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    try:
        assert call(scene=h) == STATE                                                 # not committed
    finally:
        lib.mrt_scene_destroy(h)
    dark = mrt.CornellScene((8, 8)); dark.lights = []
    nol = mrt.DeviceScene(gpu_ctx, dark)
    try:
        assert call(scene=nol.handle) == STATE and "no lights" in lib.mrt_last_error().decode()
    finally:
        nol.close()


# ---------------------------------------------------------------- 4. it follows the device's state
def _rotated(xf16, angle, shift):
    m = np.asarray(xf16, np.float32).reshape(4, 4).T.astype(np.float64)
    r = np.eye(4); r[0, 0] = r[2, 2] = np.cos(angle); r[0, 2] = np.sin(angle); r[2, 0] = -np.sin(angle); r[0, 3] = shift
    return np.ascontiguousarray((r @ m).T.reshape(16).astype(np.float32))


def test_composed_frame_follows_instance_moves_on_the_device(mrt, orc, gpu_ctx, renderers):
    import torch
    c = R.scene_case(mrt, orc, "two_level")
    xfs = np.stack([_rotated(e[2], 0.4 + 0.1 * i, 0.05 * i) for i, e in enumerate(c["entries"])])
    r = renderers("two_level")                                                        # the rays' source only: primary rays read no scene
    a = mrt.DeviceScene(gpu_ctx, c["scene"], TWO); b = mrt.DeviceScene(gpu_ctx, c["scene"], TWO)
    try:
        before = _compose(mrt, r, a, 0, gpu_ctx)
        a.set_instance_transforms_device(0, _t(xfs, gpu_ctx)); a.refit_instances_device()
        got = _compose(mrt, r, a, 0, gpu_ctx)                                         # stream order, no host wait since the update
        for i in range(len(xfs)): b.set_instance_transform(i, xfs[i])
        b.commit()
        want = _compose(mrt, r, b, 0, gpu_ctx)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(got.any())
        assert int((got.view(torch.int32) != before.view(torch.int32)).any(-1).sum()) > 100
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 5. nothing is allocated
def test_nothing_is_allocated(mrt, orc, gpu_ctx, renderers):
    import torch
    c = R.scene_case(mrt, orc, "cornell")
    r = renderers("cornell")
    ds = r.device_scene
    dev = _dev(gpu_ctx)
    n = c["w"] * c["h"]
    prim = (torch.empty((n, 8), device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
    outs = (torch.empty((n, 8), device=dev), torch.empty((n, 4), device=dev), torch.empty((n, 8), device=dev))
    r.primary_rays_device(sample_index=0, out=prim)
    surf = ds.resolve_hits_device(prim[0], ds.intersect_closest_device(prim[0]))
    ds.scatter_device(surf, prim[1], 0, out=outs)                                     # the warm calls
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20):
        r.primary_rays_device(sample_index=0, out=prim); ds.scatter_device(surf, prim[1], 0, out=outs)
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert all(torch.equal(o.view(torch.int32), f.view(torch.int32)) for o, f in zip(outs, first))


# ---------------------------------------------------------------- 6. C++
def test_cpp_host_runs_the_composed_loop(mrt, orc, gpu_ctx, tmp_path):
    exe = str(tmp_path / "integrator_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "integrator_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    w, h = 40, 24
    p = subprocess.run([exe, str(w), str(h)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    m = re.search(r"pixels=(\d+) surfaces=(\d+) wanted=(\d+) lit=(\d+) checksum=(\S+)", p.stdout)
    assert m, p.stdout
    sc = mrt.CornellScene((w, h))
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=1)
    try:
        ds = r.device_scene
        rays, hidx = r.primary_rays_device(sample_index=0)
        surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
        shadow, light, nxt = ds.scatter_device(surf, hidx, 0)
        occ = ds.intersect_any_device(shadow).cpu().numpy()
        light, nxt, types = light.cpu().numpy(), nxt.cpu().numpy(), mrt.unpack_surfaces(surf)["type"]
    finally:
        r.close()
    checksum = 0.0
    for v in np.concatenate([light, nxt[:, 0:7]], axis=1).astype(np.float64).ravel(): checksum += float(v)          # the C++ side's order, in double (max_distance, +inf, left out)
    wanted = light[:, 3] == 1.0
    assert int(m.group(1)) == w * h and int(m.group(2)) == int((types == 1).sum()) > 0 and int(m.group(3)) == int(wanted.sum()) > 0
    assert int(m.group(4)) == int((wanted & (occ == 0)).sum()) > 0
    assert float(m.group(5)) == checksum                                              # %.17g prints the double exactly
