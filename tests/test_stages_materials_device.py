"""The scatter stage with the materials extension on, on device buffers and a stream (DeviceScene.scatter_materials_device).  Every comparison is on bits:
the stage against tests/stages_materials_reference.py (pinned to the oracle's stage dumps and image by tests/test_stages_materials_device_cpu.py), and a path tracer
composed OUTSIDE the library from its five public stages and torch element-wise ops against the image Renderer draws with materials = 1 of the same scene, seed and camera."""
import os
import re
import subprocess

import numpy as np
import pytest

import stages_materials_reference as M
import stages_reference as R
import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 5
B = M.MAX_BOUNCES
KEYS = ("shadow_rays", "light", "next_rays", "lobes")


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_dev(ctx))


def _surf_t(surf, ctx):
    return _t(np.ascontiguousarray(surf).view(np.float32).reshape(-1, 16), ctx)


def _rows(a):
    """a reference output as the float32 rows the entry writes"""
    a = np.ascontiguousarray(a)
    return a.view(np.float32).reshape(a.shape[0], -1) if a.dtype == M.LOBE_DTYPE else a


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = _rows(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(got.shape[0], -1) != want.view(np.uint32).reshape(want.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ; first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _eq(a, b):
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def renderers(mrt, orc, gpu_ctx):
    """a Renderer with materials = 1 and four bounces (and through it a committed DeviceScene) per (case, scene options), made once and closed at the end of the module"""
    made = {}

    def get(name, extra=None):
        key = (name, tuple(sorted((extra or {}).items())))
        if key not in made:
            c = M.scene_case(mrt, orc, name)
            o = {"instancing": 1} if c["instancing"] else {}
            o.update(extra or {})
            r = mrt.Renderer((c["w"], c["h"]), c["scene"], ctx=gpu_ctx, seed=S.SEED, max_bounces=B, scene_options=o)
            r.set_option("materials", 1)
            made[key] = r
        return made[key]

    yield get
    for r in made.values(): r.close()


# ---------------------------------------------------------------- 1. the stage against the reference
@pytest.mark.parametrize("name", M.DEVICE_CASES)
def test_scatter_materials_equals_the_reference_on_every_bounce(mrt, orc, gpu_ctx, renderers, name):
    """surfaces resolved ON THE DEVICE from the oracle-dumped rays of each bounce; the Halton index of each ray's pixel; light_count 1 and all; with and without the
    continuation rays"""
    c = M.scene_case(mrt, orc, name)
    d = M.dump_case(mrt, orc, name, 0)
    ds = renderers(name).device_scene
    assert ds.stats.instances * ds.stats.max_submeshes == c["table"]["slots"]
    hidx = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)
    counts = np.zeros(6, np.int64)
    for b in range(B):
        rays = _t(d["rays"][b], gpu_ctx)
        surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
        h = _t(hidx[d["pixels"][b]], gpu_ctx)
        got = ds.scatter_materials_device(rays, surf, h, b, B)
        want = M.scatter_materials(orc, c["table"], d["rays"][b], mrt.unpack_surfaces(surf), hidx[d["pixels"][b]], b, B, c["scene"].lights)
        for g, k in zip(got, KEYS): _same(g.cpu().numpy(), want[k], f"{name} bounce {b}: {k}")
        counts += np.bincount(want["lobes"]["lobe"], minlength=6)
        assert np.array_equal(mrt.unpack_lobes(got[3])["lobe"], want["lobes"]["lobe"])
        for lc in (1, len(c["scene"].lights)):
            again = ds.scatter_materials_device(rays, surf, h, b, B, light_count=lc)
            wl = M.scatter_materials(orc, c["table"], d["rays"][b], mrt.unpack_surfaces(surf), hidx[d["pixels"][b]], b, B, c["scene"].lights, light_count=lc)
            for g, k in zip(again, KEYS): _same(g.cpu().numpy(), wl[k], f"{name} bounce {b} light_count {lc}: {k}")
        sh, light, none, lobes = ds.scatter_materials_device(rays, surf, h, b, B, next_rays=False)
        assert none is None and _eq(sh, got[0]) and _eq(light, got[1]) and _eq(lobes, got[3])
    assert (counts[1:] >= 3).all(), counts                                            # every lobe was compared
    with pytest.raises(ValueError): ds.scatter_materials_device(rays, surf, h, 0, B, next_rays=False, out=got)
    with pytest.raises(mrt.MRTError) as e: ds.scatter_materials_device(rays, surf, h, 0, B, light_count=len(c["scene"].lights) + 1)
    assert e.value.code == INVALID and "light_count" in str(e.value)


# ---------------------------------------------------------------- 2. the composed integrator
def _compose(mrt, r, ds, sample_index, gpu_ctx, stream=None):
    """One frame of the renderer's integrator with materials on from the five public stages, four bounces, dense rows; throughput and radiance are separate torch mul / add /
    where ops (no fused multiply-add anywhere).  -> the frame's radiance sample, torch (n, 3) float32"""
    import torch
    dev = _dev(gpu_ctx)
    rays, hidx = r.primary_rays_device(sample_index=sample_index, stream=stream)
    n = rays.shape[0]
    thr = torch.ones((n, 3), device=dev); acc = torch.zeros((n, 3), device=dev); alive = torch.ones(n, dtype=torch.bool, device=dev)
    miss = _surf_t(np.array([S.miss_record()]), gpu_ctx)
    for b in range(B):
        hits = ds.intersect_closest_device(rays, stream=stream)
        surf = ds.resolve_hits_device(rays, hits, stream=stream)
        surf = torch.where(alive[:, None], surf, miss).contiguous()                   # a path that ended stays ended: its rows are the miss record from here on
        shadow, light, nxt, lobes = ds.scatter_materials_device(rays, surf, hidx, b, B, next_rays=b + 1 < B, stream=stream)
        occluded = ds.intersect_any_device(shadow, stream=stream)
        lobe = lobes[:, 3].view(torch.int32)
        acc = torch.add(acc, torch.mul(thr, lobes[:, 4:7]))                           # emission along the path
        thr = torch.mul(thr, lobes[:, 0:3])
        lit = (light[:, 3] == 1.0) & (occluded == 0)                                  # by light.w, never by the answer for a zero ray alone
        acc = torch.where(lit[:, None], torch.add(acc, torch.mul(light[:, 0:3], thr)), acc)
        alive = (lobe >= 1) & (lobe <= 4)
        rays = nxt
    return acc


def _image(acc, w, h):
    a = acc.cpu().numpy() if not isinstance(acc, np.ndarray) else acc
    return np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], 1).reshape(h, w, 4)


@pytest.mark.parametrize("name,extra", [(M.EDGE, None), (M.EDGE_TWO_LEVEL, None), (M.EDGE, {"wide": 0})])
def test_composed_integrator_draws_the_renderers_image(mrt, orc, gpu_ctx, renderers, name, extra):
    """On a side stream behind a torch op, no host wait between the stages.  Frame 0: the bits of Renderer.accumulation() with materials = 1.  Three frames: the per-frame
    samples folded with the reference's running average in numpy float32 (torch's divide stays out of the claim)."""
    import torch
    c = M.scene_case(mrt, orc, name)
    w, h = c["w"], c["h"]
    r = renderers(name, extra)
    ds = r.device_scene
    assert ds.stats.wide_layout == (0 if extra else 1) and int(r.get_option("materials")) == 1
    side = torch.cuda.Stream(device=_dev(gpu_ctx))
    side.wait_stream(torch.cuda.current_stream(_dev(gpu_ctx)))
    with torch.cuda.stream(side):
        warm = torch.zeros(16, device=_dev(gpu_ctx)) + 1.0                            # the torch op the stages queue behind
        samples = [_compose(mrt, r, ds, f, gpu_ctx) for f in range(3)]                # stream=None: torch's current stream, the side stream
    side.synchronize()
    assert float(warm.sum()) == 16.0
    r.frameIndex = 0
    r.draw(1, wait=True)
    _same(_image(samples[0], w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: frame 0")
    assert samples[0].any()
    r.draw(2, wait=True)
    assert r.frameIndex == 3
    folded = R.running_average([s.cpu().numpy() for s in samples])
    _same(_image(folded, w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: three frames")


# ---------------------------------------------------------------- 3. launch edges
def test_launch_edges(mrt, orc, gpu_ctx, renderers):
    import torch
    c = M.scene_case(mrt, orc, M.EDGE)
    d = M.dump_case(mrt, orc, M.EDGE, 0)
    ds = renderers(M.EDGE).device_scene
    dev = _dev(gpu_ctx)
    m = 300
    surf_np = np.array(d["surfaces"][1][:m]); rays_np = np.array(d["rays"][1][:m])
    assert (surf_np["type"][1::2] == 1).sum() > 50
    surf_np[::2] = S.miss_record()                                                    # every second surface is the miss record
    hidx_np = R.halton_index(orc, S.SEED, c["w"] * c["h"], 0)[d["pixels"][1][:m]]
    pre = M.scatter_materials(orc, c["table"], rays_np, surf_np, hidx_np, 1, B, c["scene"].lights)["lobes"]["lobe"]
    slots = c["table"]["slots"]
    bad = np.array([k for k in range(3, m - 2, 6) if pre[k] != 0 and pre[k - 2] != 0 and pre[k + 2] != 0][:3])          # valid rows between valid rows, apart from one another
    for k, s in zip(bad, (-1, slots, 2 ** 30)): surf_np["resource_slot"][k] = s       # slots outside the table: no surface, and nothing is indexed
    swapped = np.array([[k for k in range(1, m, 2) if pre[k] == lobe and k not in bad][0] for lobe in (1, 4)])
    surf_np["base_color"][swapped] = [0.25, 0.5, 0.125]                               # a substituted albedo, on a diffuse row (the weight) and on a specular one (kd: the lobe's probability)
    rays, surf, hidx = _t(rays_np, gpu_ctx), _surf_t(surf_np, gpu_ctx), _t(hidx_np, gpu_ctx)
    full = ds.scatter_materials_device(rays, surf, hidx, 1, B)
    want = M.scatter_materials(orc, c["table"], rays_np, surf_np, hidx_np, 1, B, c["scene"].lights)
    assert bad.size == 3 and (want["lobes"]["lobe"][swapped] != 0).all() and (want["lobes"]["lobe"][bad] == 0).all() and (want["lobes"]["lobe"][bad + 2] != 0).all() and (want["lobes"]["lobe"][bad - 2] != 0).all()
    assert np.array_equal(want["lobes"]["weight"][swapped[0]], np.float32([0.25, 0.5, 0.125]))
    for got, k in zip(full, KEYS):
        _same(got.cpu().numpy(), want[k], k)
        assert not got.cpu().numpy()[::2].view(np.uint32).any() and not got.cpu().numpy()[bad].view(np.uint32).any(), k   # zero rows between untouched valid neighbours
    assert want["light"][1::2, 3].any() and want["next_rays"][1::2].any() and len(set(want["lobes"]["lobe"].tolist())) >= 4
    shapes = lambda n: ((n, 8), (n, 4), (n, 8), (n, 8))
    for n in (0, 1, 63, 64, 65, 257):
        got = ds.scatter_materials_device(rays[:n], surf[:n], hidx[:n], 1, B)         # out not given
        assert [tuple(g.shape) for g in got] == list(shapes(n))
        out = tuple(torch.full(sh, 7.0, device=dev) for sh in shapes(n))
        ret = ds.scatter_materials_device(rays[:n], surf[:n], hidx[:n], 1, B, out=out)
        for g, o, rt, f in zip(got, out, ret, full):
            assert rt is o and _eq(g, f[:n]) and _eq(o, f[:n]), n
        three = tuple(torch.full(sh, 7.0, device=dev) for sh in ((n, 8), (n, 4), (n, 8)))
        ret = ds.scatter_materials_device(rays[:n], surf[:n], hidx[:n], 1, B, next_rays=False, out=three)
        assert ret[2] is None and ret[3] is three[2] and _eq(three[0], full[0][:n]) and _eq(three[1], full[1][:n]) and _eq(three[2], full[3][:n])
    # the rows past n are left alone
    big = tuple(torch.full(sh, 7.0, device=dev) for sh in shapes(66))
    ds.scatter_materials_device(rays[:65], surf[:65], hidx[:65], 1, B, out=tuple(b[:65] for b in big))
    torch.cuda.synchronize()
    assert all(bool((b[65] == 7.0).all()) for b in big) and all(_eq(b[:65], f[:65]) for b, f in zip(big, full))
    # the null stream
    s0 = ds.scatter_materials_device(rays, surf, hidx, 1, B, stream=0)
    torch.cuda.synchronize()
    assert all(_eq(a, f) for a, f in zip(s0, full))
    with pytest.raises(ValueError): ds.scatter_materials_device(rays, surf, hidx[:-1], 1, B)
    with pytest.raises(ValueError): ds.scatter_materials_device(rays[:-1], surf, hidx, 1, B)
    with pytest.raises(ValueError): ds.scatter_materials_device(rays, surf.to(torch.int32), hidx, 1, B)
    with pytest.raises(mrt.MRTError): ds.scatter_materials_device(rays, surf, hidx, 4, B)
    with pytest.raises(mrt.MRTError): ds.scatter_materials_device(rays, surf, hidx, 0, 17)


def test_refusals_on_a_live_scene(mrt, orc, gpu_ctx, renderers):
    import ctypes as C
    import torch
    ds = renderers(M.EDGE).device_scene
    lib, P = mrt.lib, C.c_void_p
    dev = _dev(gpu_ctx)
    rays = torch.zeros((4, 8), device=dev); surf = torch.zeros((4, 16), device=dev); hidx = torch.zeros(4, dtype=torch.int32, device=dev)
    sh = torch.zeros((4, 8), device=dev); li = torch.zeros((4, 4), device=dev); lo = torch.zeros((4, 8), device=dev)

    def call(scene=ds.handle, n=4, bounce=0, mb=B, lc=0, s=surf.data_ptr(), l=lo.data_ptr()):
        return lib.mrt_scene_scatter_materials_device(scene, P(rays.data_ptr()), P(s), P(hidx.data_ptr()), n, bounce, mb, lc, P(sh.data_ptr()), P(li.data_ptr()), None, P(l), None)

    assert call() == 0 and call(n=0) == 0
    assert lib.mrt_scene_scatter_materials_device(ds.handle, None, None, None, 0, 0, B, 0, None, None, None, None, None) == 0
    assert call(lc=2) == INVALID and "light_count" in lib.mrt_last_error().decode()   # the box has one light
    assert call(lc=1) == 0
    assert call(s=surf.data_ptr() + 8) == INVALID and call(l=lo.data_ptr() + 4) == INVALID and call(bounce=B) == INVALID and call(bounce=-1) == INVALID and call(mb=17) == INVALID
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


# ---------------------------------------------------------------- 4. nothing is allocated
def test_nothing_is_allocated(mrt, orc, gpu_ctx, renderers):
    import torch
    c = M.scene_case(mrt, orc, M.EDGE)
    r = renderers(M.EDGE)
    ds = r.device_scene
    dev = _dev(gpu_ctx)
    n = c["w"] * c["h"]
    rays, hidx = r.primary_rays_device(sample_index=0)
    surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
    outs = tuple(torch.empty(sh, device=dev) for sh in ((n, 8), (n, 4), (n, 8), (n, 8)))
    ds.scatter_materials_device(rays, surf, hidx, 0, B, out=outs)                     # the warm call
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20):
        ds.scatter_materials_device(rays, surf, hidx, 0, B, out=outs)
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert all(_eq(o, f) for o, f in zip(outs, first))


# ---------------------------------------------------------------- 5. C++
def test_cpp_host_runs_one_bounce_with_materials(mrt, orc, gpu_ctx, tmp_path):
    import material_scenes
    exe = str(tmp_path / "materials_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "materials_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    w, h = 40, 24
    p = subprocess.run([exe, str(w), str(h)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    m = re.search(r"pixels=(\d+) lobes=(\d+),(\d+),(\d+),(\d+),(\d+),(\d+) wanted=(\d+) lit=(\d+) checksum=(\S+)", p.stdout)
    assert m, p.stdout
    sc = material_scenes.cornell_with_materials(mrt, (w, h))
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=1, max_bounces=B)
    try:
        ds = r.device_scene
        rays, hidx = r.primary_rays_device(sample_index=0)
        surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
        shadow, light, nxt, lobes = ds.scatter_materials_device(rays, surf, hidx, 0, B)
        occ = ds.intersect_any_device(shadow).cpu().numpy()
        light, nxt, lobes = light.cpu().numpy(), nxt.cpu().numpy(), lobes.cpu().numpy()
    finally:
        r.close()
    checksum = 0.0
    for v in np.concatenate([light, nxt[:, 0:7], lobes[:, 0:3], lobes[:, 4:7]], axis=1).astype(np.float64).ravel(): checksum += float(v)          # the C++ side's order, in double
    counts = np.bincount(mrt.unpack_lobes(lobes)["lobe"], minlength=6)
    wanted = light[:, 3] == 1.0
    assert int(m.group(1)) == w * h and [int(m.group(k)) for k in range(2, 8)] == counts.tolist() and counts[1] > 0 and counts[2] + counts[3] > 0 and counts[4] > 0
    assert int(m.group(8)) == int(wanted.sum()) > 0 and int(m.group(9)) == int((wanted & (occ == 0)).sum()) > 0
    assert float(m.group(10)) == checksum                                             # %.17g prints the double exactly
