"""The path-state stages on device buffers, on a stream (DeviceScene.reset_paths_device / advance_paths_device / deposit_light_device / fold_sample_device; DESIGN.md
§10m).  Every comparison is on bits, as int32 views: each stage against tests/path_state_reference.py on rows resolved and scattered on the device, what lies past the
count and outside the named pixels against what it held before, and a path tracer composed OUTSIDE the library from the stages alone (tests/paths_compose.py) against the
image Renderer draws of the same scene, seed and camera and against the torch form of the same frame (tests/queues_compose.py)."""
import numpy as np
import pytest

import path_state_reference as PS
import stages_materials_reference as M
import stages_reference as R
import surface_reference as S
from paths_compose import compose_fused
from queues_compose import compose_queued

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097)          # around a wave, around a workgroup of 256, more than one workgroup
SENTINEL = 0x7B7B7B7B
MASK_SENTINEL = 0x7B
FAR = 2 ** 30


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _counts(n):
    return (None, 0, 1, n // 2, n, n + 5, -1)          # n + 5 and -1 (2^32 - 1 as the kernel reads it) are clamped to n


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        u = {1: np.uint8, 4: np.uint32}[k]
        bad = np.flatnonzero((got.view(u).reshape(got.shape[0], -1) != want.view(u).reshape(want.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ; first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _scene_cases():
    return [("cornell", None, False), ("two_level", None, False), ("cornell", {"wide": 0}, False), (M.CORNELL, None, True)]


@pytest.fixture(scope="module")
def renderers(mrt, orc, gpu_ctx):
    """a Renderer (and through it a committed DeviceScene) per case, made once and closed at the end of the module; the materials case draws with materials = 1 and four bounces"""
    made = {}

    def get(name, extra, materials):
        key = (name, tuple(sorted((extra or {}).items())))
        if key not in made:
            c = (M if materials else R).scene_case(mrt, orc, name)
            o = {"instancing": 1} if c["instancing"] else {}
            o.update(extra or {})
            r = mrt.Renderer((c["w"], c["h"]), c["scene"], ctx=gpu_ctx, seed=S.SEED, max_bounces=M.MAX_BOUNCES if materials else 3, scene_options=o)
            if materials: r.set_option("materials", 1)
            made[key] = r
        return made[key]

    yield get
    for r in made.values(): r.close()


@pytest.fixture(scope="module")
def pools(mrt, orc, gpu_ctx, renderers):
    """rows resolved and scattered ON THE DEVICE, bounce 0 and (dense) bounce 1 one after the other, as numpy arrays made once and never changed: 'diffuse' from
    CornellScene 64 x 64 — surfaces (N, 16), light (N, 4) — and 'materials' from cornell_with_materials — lobes (N, 8), light (N, 4)"""
    import torch
    out = {}
    for key, (name, materials) in (("diffuse", ("cornell", False)), ("materials", (M.CORNELL, True))):
        r = renderers(name, None, materials)
        ds = r.device_scene
        rays, hidx = r.primary_rays_device(sample_index=0)
        rows = {"surfaces": [], "light": [], "lobes": []}
        for b in range(2):
            surf = ds.resolve_hits_device(rays, ds.intersect_closest_device(rays))
            if materials:
                _, light, rays, lobes = ds.scatter_materials_device(rays, surf, hidx, b, M.MAX_BOUNCES)
                rows["lobes"].append(lobes.cpu().numpy())
            else:
                _, light, rays = ds.scatter_device(surf, hidx, b)
            rows["surfaces"].append(surf.cpu().numpy()); rows["light"].append(light.cpu().numpy())
        pool = {k: np.concatenate(v) for k, v in rows.items() if v}
        for a in pool.values(): a.setflags(write=False)
        out[key] = pool
    torch.cuda.synchronize()
    # the pools are no pretence: hits and misses, wanted and unwanted shadow rays, every lobe code and a material that emits
    d, m = out["diffuse"], out["materials"]
    kinds = d["surfaces"][:, 7].view(np.int32)
    assert d["surfaces"].shape[0] >= 4097 and 0 < (kinds == 1).sum() < kinds.size and 0 < (d["light"][:, 3] == 1.0).sum() < kinds.size
    assert m["lobes"].shape[0] >= 4097 and set(range(0, 5)) <= set(m["lobes"][:, 3].view(np.int32).tolist()) and m["lobes"][:, 4:7].any()
    assert 0 < (m["light"][:, 3] == 1.0).sum() < m["light"].shape[0]
    return out


def _case(pool, n, count, rng, materials):
    """the inputs of one advance / deposit call as numpy arrays: rows drawn from the pool, a random throughput whose fourth component holds a bit pattern, pixels as a
    random permutation of an image of n + 7 pixels with two rows < m sent outside it, an image holding a pattern; and from m on what no kernel may depend on"""
    m = PS.rows_in_use(n, count)
    pick = rng.permutation(pool["light"].shape[0])[:n]
    npix = n + 7
    c = dict(n=n, m=m, npix=npix, light=pool["light"][pick].copy(), thr=(rng.random((n, 4)) + 0.25).astype(np.float32), pixel=rng.permutation(npix)[:n].astype(np.int32),
             radiance=rng.standard_normal((npix, 4)).astype(np.float32), occluded=rng.choice(np.array([0, 0, 1, 7, -1], np.int32), n))
    c["radiance"][:, 3].view(np.uint32)[:] = rng.integers(0, 2 ** 32, npix, dtype=np.uint64).astype(np.uint32)          # any bits, NaNs among them: the kernels keep them
    c["thr"][:, 3].view(np.uint32)[:] = 0xFFC0FFEE
    rows = pool["lobes" if materials else "surfaces"][pick].copy()
    if m >= 2:                                                                                          # two depositing rows (where there are any) name no pixel
        live = np.flatnonzero(rows[:m, 3].view(np.int32) != 0) if materials else np.flatnonzero(c["occluded"][:m] == 0)
        a, b = (live[0], live[-1]) if live.size >= 2 else (0, m - 1)
        c["pixel"][a] = npix; c["pixel"][b] = -1
    c["light"][m:] = np.nan; c["pixel"][m:] = FAR; c["occluded"][m:] = 0
    c["thr"].view(np.uint32)[m:] = SENTINEL
    if materials: rows[m:] = np.nan; rows[m:, 3].view(np.int32)[:] = FAR
    else: rows[m:] = np.nan; rows[m:, 7].view(np.int32)[:] = 1
    c["rows"] = rows
    return c


def _count_word(torch, dev, count, unsigned=False):
    if count is None: return None
    t = torch.tensor([count], dtype=torch.int32, device=dev)
    return t.view(torch.uint32) if unsigned and hasattr(torch, "uint32") else t


# ---------------------------------------------------------------- 1. each stage against the reference
@pytest.mark.parametrize("n", SIZES)
def test_advance_paths_equals_the_reference(mrt, gpu_ctx, renderers, pools, n):
    """both forms, with and without the second mask, every count: throughput, masks and image against the reference over ALL their rows — so the rows from m on still hold
    the sentinel, a pixel no row names keeps its bits, and every .w keeps its bits — and the inputs are left as they were"""
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    rng = np.random.default_rng(100 + n)
    for materials in (False, True):
        pool = pools["materials" if materials else "diffuse"]
        for turn, count in enumerate(_counts(n)):
            for keep_path in (True, False):
                c = _case(pool, n, count, rng, materials)
                t = {k: torch.from_numpy(c[k]).to(dev) for k in ("light", "thr", "pixel", "radiance", "rows")}
                masks = tuple(torch.full((n,), MASK_SENTINEL, dtype=torch.uint8, device=dev) for _ in range(2 if keep_path else 1))
                kw = dict(lobes=t["rows"], pixel=t["pixel"], radiance=t["radiance"]) if materials else dict(surfaces=t["rows"])
                if not materials and turn % 2: kw.update(pixel=t["pixel"], radiance=t["radiance"])          # the diffuse form may be handed an image: it does not touch it
                got = ds.advance_paths_device(t["light"], t["thr"], count=_count_word(torch, dev, count, unsigned=turn % 2 == 1), keep_path=keep_path, out=masks, **kw)
                assert got[0] is masks[0] and (got[1] is masks[1] if keep_path else got[1] is None)
                pre = np.full(n, MASK_SENTINEL, np.uint8)
                want = PS.advance_paths(c["thr"], c["light"], pixel=c["pixel"], radiance=c["radiance"], count=count, keep_shadow=pre, keep_path=pre,
                                        **({"lobes": c["rows"]} if materials else {"surfaces": c["rows"]}))
                tag = f"{'materials' if materials else 'diffuse'} n={n} count={count} keep_path={keep_path}"
                _same(t["thr"].cpu().numpy(), want["throughput"], tag + ": throughput")
                _same(masks[0].cpu().numpy(), want["keep_shadow"], tag + ": keep_shadow")
                if keep_path: _same(masks[1].cpu().numpy(), want["keep_path"], tag + ": keep_path")
                _same(t["radiance"].cpu().numpy(), want["radiance"] if materials else c["radiance"], tag + ": radiance")
                for k in ("light", "pixel", "rows"): _same(t[k].cpu().numpy(), c[k], tag + ": input " + k)
                if materials and c["m"] >= 4000: assert (want["radiance"] != c["radiance"]).any(), tag + ": no row emits"


@pytest.mark.parametrize("n", SIZES)
def test_deposit_light_equals_the_reference(mrt, gpu_ctx, renderers, pools, n):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    rng = np.random.default_rng(200 + n)
    for turn, count in enumerate(_counts(n)):
        c = _case(pools["diffuse"], n, count, rng, False)
        dark = np.flatnonzero(~c["light"][:c["m"], 0:3].any(1))[::2]                                   # most rows of the pool are unlit: every second of them gets a colour
        c["light"][dark, 0:3] = rng.random((dark.size, 3)).astype(np.float32) * np.float32(4.0)
        t = {k: torch.from_numpy(c[k]).to(dev) for k in ("occluded", "light", "thr", "pixel", "radiance")}
        assert ds.deposit_light_device(t["occluded"], t["light"], t["thr"], t["pixel"], t["radiance"], count=_count_word(torch, dev, count, unsigned=turn % 2 == 1)) is None
        want = PS.deposit_light(c["occluded"], c["light"], c["thr"], c["pixel"], c["radiance"], count=count)
        tag = f"n={n} count={count}"
        _same(t["radiance"].cpu().numpy(), want, tag + ": radiance")
        for k in ("occluded", "light", "thr", "pixel"): _same(t[k].cpu().numpy(), c[k], tag + ": input " + k)
        if c["m"] >= 32: assert (want != c["radiance"]).any(), tag + ": no row deposits"


@pytest.mark.parametrize("n", SIZES)
def test_reset_paths_with_and_without_the_image(mrt, gpu_ctx, renderers, n):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    thr, pix, rad = ds.reset_paths_device(n)
    assert thr.dtype == torch.float32 and pix.dtype == torch.int32 and tuple(rad.shape) == (n, 4)
    want = PS.reset_paths(n, n)
    for g, w, what in zip((thr, pix, rad), want, ("throughput", "pixel", "radiance")): _same(g.cpu().numpy(), w, f"n={n}: {what}")
    thr2, pix2, none = ds.reset_paths_device(n, radiance=False)
    assert none is None
    _same(thr2.cpu().numpy(), want[0], "throughput, no image"); _same(pix2.cpu().numpy(), want[1], "pixel, no image")
    for npix in (n + 300, max(n - 3, 0)):                                                             # an image with more pixels than rows, and with fewer
        out = (torch.full((n, 4), float("nan"), device=dev), torch.full((n,), FAR, dtype=torch.int32, device=dev), torch.full((npix, 4), float("nan"), device=dev))
        got = ds.reset_paths_device(n, out=out)
        assert all(a is b for a, b in zip(got, out))
        want = PS.reset_paths(n, npix)
        if n == 0: want = (want[0], want[1], np.full((npix, 4), np.nan, np.float32))                  # no rows: nothing is launched
        for g, w, what in zip(out, want, ("throughput", "pixel", "radiance")): _same(g.cpu().numpy().view(np.uint32), w.view(np.uint32), f"n={n} npix={npix}: {what}")


@pytest.mark.parametrize("clear", [False, True], ids=["keep_sample", "clear_sample"])
def test_fold_sample_equals_the_reference(mrt, gpu_ctx, renderers, clear):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    rng = np.random.default_rng(300)
    for npix in (0, 1, 255, 257, 4097):
        for frame in (0, 1, 2, 2 ** 24 + 1):
            sample = rng.random((npix, 4)).astype(np.float32) * np.float32(3.0)
            accum = rng.random((npix, 4)).astype(np.float32)
            if frame == 0: accum[:] = np.nan                                                          # frame 0 reads no accumulation
            s, a = torch.from_numpy(sample).to(dev), torch.from_numpy(accum).to(dev)
            ds.fold_sample_device(s, a, frame, clear_sample=clear)
            want_s, want_a = PS.fold_sample(sample, accum, frame, clear_sample=clear)
            _same(a.cpu().numpy(), want_a, f"npix={npix} frame={frame}: accum"); _same(s.cpu().numpy(), want_s, f"npix={npix} frame={frame}: sample")
            if npix: assert (want_a[:, 3] == 1.0).all() and np.isfinite(want_a).all()
    with pytest.raises(mrt.MRTError) as e: ds.fold_sample_device(s, s, 0)
    assert e.value.code == 1 and "d_sample" in str(e.value)
    with pytest.raises(ValueError): ds.fold_sample_device(s, a, 2 ** 32 - 1)
    with pytest.raises(ValueError): ds.fold_sample_device(s, a[:-1], 0)
    with pytest.raises(ValueError): ds.advance_paths_device(a, a)                                      # neither form
    with pytest.raises(ValueError): ds.advance_paths_device(a, a, lobes=torch.zeros((4097, 8), device=dev))   # the materials form without pixel and radiance
    with pytest.raises(ValueError): ds.deposit_light_device(torch.zeros(4097, device=dev), a, a, torch.zeros(4097, dtype=torch.int32, device=dev), a)   # occluded is int32


# ---------------------------------------------------------------- 2. streams and memory
def _one_of_each(torch, ds, dev, pools, rng, n, stream):
    """the four calls on `stream`, with every output given -> (device tensors, what the reference makes of the same inputs)"""
    got, want = [], []
    out = (torch.empty((n, 4), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n + 7, 4), device=dev))
    ds.reset_paths_device(n, out=out, stream=stream)
    got += list(out); want += list(PS.reset_paths(n, n + 7))
    for materials in (False, True):
        c = _case(pools["materials" if materials else "diffuse"], n, n - 9, rng, materials)
        t = {k: torch.from_numpy(c[k]).to(dev) for k in ("light", "thr", "pixel", "radiance", "rows", "occluded")}
        masks = tuple(torch.full((n,), MASK_SENTINEL, dtype=torch.uint8, device=dev) for _ in range(2))
        cw = torch.tensor([n - 9], dtype=torch.int32, device=dev)
        ds.advance_paths_device(t["light"], t["thr"], pixel=t["pixel"], radiance=t["radiance"], count=cw, out=masks, stream=stream, **({"lobes": t["rows"]} if materials else {"surfaces": t["rows"]}))
        pre = np.full(n, MASK_SENTINEL, np.uint8)
        w = PS.advance_paths(c["thr"], c["light"], pixel=c["pixel"], radiance=c["radiance"], count=n - 9, keep_shadow=pre, keep_path=pre, **({"lobes": c["rows"]} if materials else {"surfaces": c["rows"]}))
        ds.deposit_light_device(t["occluded"], t["light"], t["thr"], t["pixel"], t["radiance"], count=cw, stream=stream)
        rad = PS.deposit_light(c["occluded"], c["light"], w["throughput"], c["pixel"], w["radiance"] if materials else c["radiance"], count=n - 9)
        got += [t["thr"], masks[0], masks[1], t["radiance"]]; want += [w["throughput"], w["keep_shadow"], w["keep_path"], rad]
    sample = (rng.random((n, 4)) * 2.0).astype(np.float32); accum = rng.random((n, 4)).astype(np.float32)
    s, a = torch.from_numpy(sample).to(dev), torch.from_numpy(accum).to(dev)
    ds.fold_sample_device(s, a, 5, clear_sample=True, stream=stream)
    got += [s, a]; want += list(PS.fold_sample(sample, accum, 5, clear_sample=True))
    return got, want


def test_every_call_on_a_side_stream_and_on_the_null_stream(mrt, gpu_ctx, renderers, pools):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    rng = np.random.default_rng(11)
    n = 1000
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        warm = torch.zeros(16, device=dev) + 1.0                                                      # the torch op the calls queue behind
        got_a, want_a = _one_of_each(torch, ds, dev, pools, rng, n, None)                             # stream=None: torch's current stream, the side stream
        got_b, want_b = _one_of_each(torch, ds, dev, pools, rng, n, side)
    side.synchronize()
    assert float(warm.sum()) == 16.0
    for k, (g, w) in enumerate(zip(got_a + got_b, want_a + want_b)): _same(g.cpu().numpy(), w, f"side stream, output {k}")
    torch.cuda.synchronize()
    got_c, want_c = _one_of_each(torch, ds, dev, pools, rng, n, 0)
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got_c, want_c)): _same(g.cpu().numpy(), w, f"null stream, output {k}")


def test_the_calls_allocate_nothing(mrt, gpu_ctx, renderers, pools):
    import torch
    dev = _dev(gpu_ctx)
    ds = renderers("cornell", None, False).device_scene
    rng = np.random.default_rng(3)
    n = 4097
    c = _case(pools["materials"], n, n - 7, rng, True)
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ("light", "thr", "pixel", "radiance", "rows", "occluded")}
    surf = torch.from_numpy(pools["diffuse"]["surfaces"][:n].copy()).to(dev)
    masks = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev))
    state = (torch.empty((n, 4), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n + 7, 4), device=dev))
    accum = torch.zeros((n + 7, 4), device=dev)
    cw = torch.tensor([n - 7], dtype=torch.int32, device=dev)

    def calls():
        ds.reset_paths_device(n, out=state)
        ds.advance_paths_device(t["light"], state[0], surfaces=surf, count=cw, out=masks)
        ds.advance_paths_device(t["light"], state[0], pixel=t["pixel"], radiance=state[2], lobes=t["rows"], count=cw, out=masks)
        ds.deposit_light_device(t["occluded"], t["light"], state[0], t["pixel"], state[2], count=cw)
        ds.fold_sample_device(state[2], accum, 0, clear_sample=True)

    calls()                                                                                           # the warm ones
    torch.cuda.synchronize()
    first = accum.clone()
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20): calls()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert torch.equal(accum.view(torch.int32), first.view(torch.int32)) and not state[2].view(torch.int32).any()


# ---------------------------------------------------------------- 3. the composed integrator: library calls only
@pytest.mark.parametrize("name,extra,materials", _scene_cases())
def test_composed_integrator_on_path_state_stages_draws_the_renderers_image(mrt, orc, gpu_ctx, renderers, name, extra, materials):
    """Frame 0: the bits of Renderer.accumulation(), and of the torch form of the same frame.  Four frames deposited into ONE sample buffer that the fold clears: four
    rendered frames.  And the queues are no pretence: after bounce 0 the path queue is shorter than the image and not empty, and the materials scene deposits emission and
    holds every lobe that goes on."""
    import torch
    dev = _dev(gpu_ctx)
    c = (M if materials else R).scene_case(mrt, orc, name)
    w, h = c["w"], c["h"]
    n = w * h
    r = renderers(name, extra, materials)
    ds = r.device_scene
    assert ds.stats.wide_layout == (0 if extra else 1)
    bounces = M.MAX_BOUNCES if materials else 3
    info = {}
    rad = compose_fused(torch, r, ds, 0, dev, bounces=bounces, materials=materials, info=info)
    queued = compose_queued(torch, r, ds, 0, dev, bounces=bounces, materials=materials, host_counts=False)
    accum = torch.full((n, 4), float("nan"), device=dev)
    ds.fold_sample_device(rad, accum, 0)
    counts = [int(k) for k in info["counts"]]
    assert len(counts) == bounces - 1 and 0 < counts[0] < n and all(a >= b for a, b in zip(counts, counts[1:])), counts
    if materials:
        seen = set()
        for lobe, cnt in info["lobes"]:
            seen |= set(lobe[:lobe.shape[0] if cnt is None else int(cnt)].cpu().numpy().tolist())
        assert {1, 2, 3, 4} <= seen, seen
        first = info["lobe_rows"][0].cpu().numpy()                                                    # bounce 0: the throughput is 1, the term is the emission itself
        assert first[first[:, 3].view(np.int32) != 0][:, 4:7].any()
    r.frameIndex = 0
    r.draw(1, wait=True)
    _same(accum.cpu().numpy(), r.accumulation().reshape(-1, 4), f"{name} {extra}: frame 0")
    _same(rad.cpu().numpy()[:, 0:3], queued.cpu().numpy(), f"{name} {extra}: the torch form of frame 0")
    assert rad[:, 0:3].any() and not rad[:, 3].any()
    sample = torch.zeros((n, 4), device=dev)
    accum = torch.full((n, 4), float("nan"), device=dev)
    for f in range(4):
        assert compose_fused(torch, r, ds, f, dev, bounces=bounces, materials=materials, radiance=sample) is sample
        ds.fold_sample_device(sample, accum, f, clear_sample=True)
    r.frameIndex = 0
    r.draw(4, wait=True)
    assert r.frameIndex == 4
    _same(accum.cpu().numpy(), r.accumulation().reshape(-1, 4), f"{name} {extra}: four frames")
    assert not sample.view(torch.int32).any()
