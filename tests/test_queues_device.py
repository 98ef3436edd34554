"""Row queues on device buffers, on a stream (DeviceScene.compact_rows_device and count= of the six stage methods).  Every comparison is on bits, as int32
views: the compaction against x[:m][mask[:m]] in torch, each counted entry against its uncounted twin on the same rows, and a path tracer composed OUTSIDE the library on
compacted queues — in both forms of tests/queues_compose.py — against the image Renderer draws of the same scene, seed and camera."""
import numpy as np
import pytest

import stages_materials_reference as M
import stages_reference as R
import surface_reference as S
from queues_compose import compose_queued

pytestmark = pytest.mark.gpu

# the implementation's constants (queues.hip / scene_device.h): rows per workgroup of the count and move kernels, totals the scan workgroup takes at a step
COMPACT_ROWS, COMPACT_SCAN_THREADS = 2048, 1024
BIG = 2 ** 21 + 3                                   # 1 025 workgroups: the scan of their totals takes two steps
assert (BIG + COMPACT_ROWS - 1) // COMPACT_ROWS > COMPACT_SCAN_THREADS
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 8191, 8193)
COLUMN_SETS = ((4,), (12,), (32,), (64,), (4, 12, 32, 64, 16, 8, 48, 4))
SENTINEL = 0x7B7B7B7B


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _patterns(n, m, rng):
    """name -> keep mask over n rows (numpy bool); m = the rows in use"""
    p = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0}
    first = np.zeros(n, bool); first[:1] = True; p["only row 0"] = first
    lastrow = np.zeros(n, bool)
    if m: lastrow[m - 1] = True
    p["only row m - 1"] = lastrow
    edges = np.zeros(n, bool)
    for k in range(COMPACT_ROWS, n + 2, COMPACT_ROWS):
        for i in (k - 1, k + 1):
            if i < n: edges[i] = True
    p["around the multiples of 2048"] = edges
    p["random 50 %"] = rng.random(n) < 0.5
    p["random 3 %"] = rng.random(n) < 0.03
    return p


def _columns(torch, dev, n, row_bytes, rng):
    return [torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=(n, rb // 4) if rb > 4 or k % 2 else (n,), dtype=np.int64).astype(np.int32)).to(dev) for k, rb in enumerate(row_bytes)]


def _check_compaction(torch, ds, dev, n, keep_np, cols, count_in, as_bytes, stream=None):
    """one call against torch's boolean indexing -> a device-side bool: everything held (no host wait here)"""
    m = n if count_in is None else min(n, count_in)
    keep = torch.from_numpy(keep_np.astype(np.uint8) * 7 if as_bytes else keep_np).to(dev)          # non-zero keeps, whatever the byte
    cin = None if count_in is None else torch.tensor([count_in], dtype=torch.int32, device=dev)
    out = [torch.full_like(c, SENTINEL) for c in cols]
    src_before, keep_before = [c.clone() for c in cols], keep.clone()
    ws = torch.empty(ds.compact_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ret, cnt = ds.compact_rows_device(keep, cols, count=cin, out=out, workspace=ws, stream=stream)
    assert all(a is b for a, b in zip(ret, out)) and cnt.dtype == torch.int32 and tuple(cnt.shape) == (1,)
    mask = torch.from_numpy(keep_np[:m]).to(dev)
    k = int(keep_np[:m].sum())
    ok = cnt[0] == k
    for c, o, before in zip(cols, out, src_before):
        want = torch.full_like(c, SENTINEL)
        want[:k] = c[:m][mask]                                                                     # the order is kept; the rows from count_out on still hold the sentinel
        ok = ok & (_bits(o) == _bits(want)).all() & (_bits(c) == _bits(before)).all()
    return ok & (keep.view(torch.uint8) == keep_before.view(torch.uint8)).all()


def _assert_all(torch, oks, what):
    flags = torch.stack([o.reshape(()) for o in oks]).cpu().numpy()
    assert flags.all(), f"{int((~flags).sum())} of {flags.size} checks failed; the first: {[what[i] for i in np.flatnonzero(~flags)[:5]]}"


@pytest.fixture(scope="module")
def any_scene(mrt, gpu_ctx):
    """compaction reads no scene: the smallest one carries the method"""
    ds = mrt.DeviceScene(gpu_ctx, mrt.CornellScene((8, 8)))
    yield ds
    ds.close()


# ---------------------------------------------------------------- 1. compaction against torch
@pytest.mark.parametrize("n", SIZES)
def test_compaction_equals_torch_boolean_indexing(mrt, gpu_ctx, any_scene, n):
    """every keep pattern x every incoming count (none, 0, n // 2, n, n + 5: clamped), the column sets in turn; then every column set at the random pattern"""
    import torch
    dev = _dev(gpu_ctx)
    rng = np.random.default_rng(1000 + n)
    oks, what = [], []
    turn = 0
    for count_in in (None, 0, n // 2, n, n + 5):
        m = n if count_in is None else min(n, count_in)
        for name, keep in _patterns(n, m, rng).items():
            rbs = COLUMN_SETS[turn % len(COLUMN_SETS)]; turn += 1
            oks.append(_check_compaction(torch, any_scene, dev, n, keep, _columns(torch, dev, n, rbs, rng), count_in, as_bytes=turn % 2 == 0))
            what.append((name, count_in, rbs))
    for rbs in COLUMN_SETS:
        for count_in in (None, n // 2, n + 5):
            oks.append(_check_compaction(torch, any_scene, dev, n, rng.random(n) < 0.5, _columns(torch, dev, n, rbs, rng), count_in, as_bytes=False))
            what.append(("random 50 %", count_in, rbs))
    _assert_all(torch, oks, what)


def test_compaction_where_the_scan_takes_two_steps(mrt, gpu_ctx, any_scene):
    import torch
    dev = _dev(gpu_ctx)
    rng = np.random.default_rng(7)
    cols = _columns(torch, dev, BIG, (32, 4), rng)
    pats = _patterns(BIG, BIG, rng)
    oks, what = [], []
    for name, count_in in (("random 50 %", None), ("around the multiples of 2048", None), ("random 3 %", BIG // 2), ("all", BIG + 5), ("only row m - 1", BIG)):
        oks.append(_check_compaction(torch, any_scene, dev, BIG, pats[name], cols, count_in, as_bytes=False)); what.append((name, count_in))
    _assert_all(torch, oks, what)


def test_compaction_a_count_alone_and_refusals_on_a_live_context(mrt, gpu_ctx, any_scene):
    import torch
    dev = _dev(gpu_ctx)
    keep = torch.arange(5000, device=dev) % 3 == 0
    outs, cnt = any_scene.compact_rows_device(keep, [])                                               # ncolumns == 0; out, workspace and count not given
    assert outs == [] and int(cnt) == 1667
    x = torch.arange(5000, dtype=torch.int32, device=dev)
    (y,), cnt = any_scene.compact_rows_device(keep.to(torch.uint8), [x], count=torch.tensor([3001], dtype=torch.int32, device=dev))
    assert int(cnt) == 1001 and torch.equal(y[:1001], x[:3001][keep[:3001]])
    with pytest.raises(mrt.MRTError) as e: any_scene.compact_rows_device(keep, [x], out=[x])          # in place
    assert e.value.code == 1 and "overlaps" in str(e.value)
    with pytest.raises(mrt.MRTError) as e: any_scene.compact_rows_device(keep, [torch.zeros((5000, 17), dtype=torch.int32, device=dev)])
    assert "row_bytes" in str(e.value)
    with pytest.raises(mrt.MRTError) as e: any_scene.compact_rows_device(keep, [x], workspace=torch.empty(0, dtype=torch.uint8, device=dev))
    assert "workspace" in str(e.value)
    with pytest.raises(ValueError): any_scene.compact_rows_device(keep, [x[:-1]])
    with pytest.raises(ValueError): any_scene.compact_rows_device(keep.to(torch.int32), [x])
    with pytest.raises(ValueError): any_scene.compact_rows_device(keep, [x], count=torch.tensor([1, 2], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError): any_scene.compact_rows_device(keep, [x], count=torch.tensor([1], dtype=torch.int32))       # on the host
    torch.cuda.synchronize()


def test_compaction_on_a_side_stream_and_on_the_null_stream(mrt, gpu_ctx, any_scene):
    import torch
    dev = _dev(gpu_ctx)
    rng = np.random.default_rng(11)
    n = 2049
    keep = rng.random(n) < 0.5
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        warm = torch.zeros(16, device=dev) + 1.0                                                      # the torch op the call queues behind
        cols = _columns(torch, dev, n, (32, 4, 16), rng)
        a = _check_compaction(torch, any_scene, dev, n, keep, cols, n // 2, as_bytes=False)           # stream=None: torch's current stream, the side stream
        b = _check_compaction(torch, any_scene, dev, n, keep, cols, None, as_bytes=True, stream=side)
    side.synchronize()
    assert float(warm.sum()) == 16.0 and bool(a) and bool(b)
    torch.cuda.synchronize()
    c = _check_compaction(torch, any_scene, dev, n, keep, cols, n + 5, as_bytes=False, stream=0)
    torch.cuda.synchronize()
    assert bool(c)


def test_compaction_allocates_nothing(mrt, gpu_ctx, any_scene):
    import torch
    dev = _dev(gpu_ctx)
    n = 8193
    rng = np.random.default_rng(3)
    cols = _columns(torch, dev, n, (32, 4, 4, 16), rng)
    keep = torch.from_numpy(rng.random(n) < 0.5).to(dev)
    out = [torch.empty_like(c) for c in cols]
    ws = torch.empty(any_scene.compact_workspace_bytes(n), dtype=torch.uint8, device=dev)
    cin = torch.tensor([n - 7], dtype=torch.int32, device=dev)
    _, cnt = any_scene.compact_rows_device(keep, cols, count=cin, out=out, workspace=ws)              # the warm call
    torch.cuda.synchronize()
    first = [o.clone() for o in out]; k = int(cnt)
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(dev)[0]]
    for _ in range(20):
        _, cnt = any_scene.compact_rows_device(keep, cols, count=cin, out=out, workspace=ws)
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(dev)[0])
    assert free[0] == free[1], free
    assert int(cnt) == k and all(torch.equal(_bits(o)[:k], _bits(f)[:k]) for o, f in zip(out, first))


# ---------------------------------------------------------------- 2. the counted entries against their twins
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


def _poisoned(torch, t, live, fill):
    """t with the rows from `live` on replaced: what a counted entry must never look at"""
    p = t.clone()
    if p.dtype == torch.float32: p[live:] = float("nan")
    else: p[live:] = fill
    return p


@pytest.mark.parametrize("name,extra,materials", _scene_cases())
def test_counted_entries_equal_their_twins_below_the_count_and_touch_nothing_else(mrt, orc, gpu_ctx, renderers, name, extra, materials):
    """Rays with min_distance == 0 and a second set with min_distance = 1e-3 (the lane kernel on a scene with the 8-wide layout).  For every twin and every count: the rows
    below min(n, count) are the twin's on the same inputs, the later rows keep the sentinel, and the tail of every input holds NaN rays, hit records with ids of 2^30 and
    surfaces with slot 2^30, on which nothing depends."""
    import torch
    dev = _dev(gpu_ctx)
    r = renderers(name, extra, materials)
    ds = r.device_scene
    assert ds.stats.wide_layout == (0 if extra else 1)
    rays0, hidx = r.primary_rays_device(sample_index=0)
    n = rays0.shape[0]
    rays1 = rays0.clone(); rays1[:, 3] = 1e-3
    attrs = [torch.from_numpy(np.random.default_rng(5).standard_normal((int(ds.vertex_offsets()[-1]), ch)).astype(np.float32)).to(dev) for ch in (3, 8)]
    bounces = M.MAX_BOUNCES
    oks, what = [], []

    def sentinel_like(w):
        t = torch.full(tuple(w.shape), SENTINEL, dtype=torch.int32, device=dev)
        return t if w.dtype == torch.int32 else t.view(torch.float32)

    def blank(ref):
        return tuple(None if w is None else sentinel_like(w) for w in ref)

    def check(tag, count, got, ref):
        live = min(n, count)
        for g, w in zip(got, ref):
            if w is None: continue
            want = sentinel_like(w)
            want[:live] = w[:live]
            oks.append((_bits(g) == _bits(want)).all()); what.append((tag, count))

    for rays in (rays0, rays1):
        hits = ds.intersect_closest_device(rays)
        occ = ds.intersect_any_device(rays)
        surf = ds.resolve_hits_device(rays, hits)
        assert 0 < int((surf[:, 7].view(torch.int32) == 1).sum()) < n                                  # hits and misses among the rows
        interp = [ds.interpolate_device(hits, a) for a in attrs]
        scat = ds.scatter_device(surf, hidx, 0)
        scat_last = ds.scatter_device(surf, hidx, 2, next_rays=False)
        mats = ds.scatter_materials_device(rays, surf, hidx, 0, bounces) if materials else None
        assert torch.equal(_bits(ds.intersect_closest_device(rays, count=None)), _bits(hits))          # count=None is the old entry
        for count in (0, 1, 63, 64, 65, 257, n, n + 5):
            live = min(n, count)
            cw = torch.tensor([count], dtype=torch.int32, device=dev)
            p_rays = _poisoned(torch, rays, live, 0)
            p_hits = _poisoned(torch, hits, live, 2 ** 30); p_hits[live:, 0] = 1                       # type 1, every id 2^30
            p_surf = _poisoned(torch, surf, live, 0); p_surf.view(torch.int32)[live:, 7] = 1; p_surf.view(torch.int32)[live:, 11] = 2 ** 30
            p_hidx = _poisoned(torch, hidx, live, 2 ** 30)
            o = blank((hits,)); ds.intersect_closest_device(p_rays, out=o[0], count=cw); check("closest", count, o, (hits,))
            o = blank((occ,)); ds.intersect_any_device(p_rays, out=o[0], count=cw); check("any", count, o, (occ,))
            o = blank((surf,)); ds.resolve_hits_device(p_rays, p_hits, out=o[0], count=cw); check("resolve", count, o, (surf,))
            for a, ref in zip(attrs, interp):
                o = blank((ref,)); ds.interpolate_device(p_hits, a, out=o[0], count=cw); check(f"interpolate {a.shape[1]}", count, o, (ref,))
            o = blank(scat); ds.scatter_device(p_surf, p_hidx, 0, out=o, count=cw); check("scatter", count, o, scat)
            o = blank(scat_last[:2]); ds.scatter_device(p_surf, p_hidx, 2, next_rays=False, out=o, count=cw); check("scatter, no next rays", count, o, scat_last[:2])
            if materials:
                o = blank(mats); ds.scatter_materials_device(p_rays, p_surf, p_hidx, 0, bounces, out=o, count=cw); check("scatter_materials", count, o, mats)
        cu = getattr(torch, "uint32", None)
        if cu is not None:                                                                             # the word is unsigned: uint32 is taken as it is, and -1 is clamped to n
            o = blank((occ,)); ds.intersect_any_device(rays, out=o[0], count=torch.tensor([65], dtype=torch.int32, device=dev).view(cu)); check("any, uint32", 65, o, (occ,))
        o = blank((occ,)); ds.intersect_any_device(rays, out=o[0], count=torch.tensor([-1], dtype=torch.int32, device=dev)); check("any, count -1", n, o, (occ,))
    _assert_all(torch, oks, what)


# ---------------------------------------------------------------- 3. the composed integrator on queues
def _image(acc, w, h):
    a = acc.cpu().numpy() if not isinstance(acc, np.ndarray) else acc
    return np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], 1).reshape(h, w, 4)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(got.shape[0], -1) != want.view(np.uint32).reshape(want.shape[0], -1)).any(-1))
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ; first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


@pytest.mark.parametrize("host_counts", [True, False], ids=["host_counts", "no_host_read"])
@pytest.mark.parametrize("name,extra,materials", _scene_cases())
def test_composed_integrator_on_queues_draws_the_renderers_image(mrt, orc, gpu_ctx, renderers, name, extra, materials, host_counts):
    """Frame 0: the bits of Renderer.accumulation().  Three frames: the per-frame samples folded with the reference's running average in numpy float32.  And the queues are
    no pretence: after bounce 0 the path queue is shorter than the image and not empty, and the materials scene's queues hold every lobe that goes on."""
    import torch
    dev = _dev(gpu_ctx)
    c = (M if materials else R).scene_case(mrt, orc, name)
    w, h = c["w"], c["h"]
    r = renderers(name, extra, materials)
    ds = r.device_scene
    bounces = M.MAX_BOUNCES if materials else 3
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    infos = [{} for _ in range(3)]
    with torch.cuda.stream(side):
        samples = [compose_queued(torch, r, ds, f, dev, bounces=bounces, materials=materials, host_counts=host_counts, info=infos[f]) for f in range(3)]
    side.synchronize()
    counts = [int(k) for k in infos[0]["counts"]]
    assert len(counts) == bounces - 1 and 0 < counts[0] < w * h and all(a >= b for a, b in zip(counts, counts[1:])), counts
    if materials:
        seen = set()
        for lobe, cnt in infos[0]["lobes"]:
            seen |= set(lobe[:lobe.shape[0] if cnt is None else int(cnt)].cpu().numpy().tolist())
        assert {1, 2, 3, 4} <= seen, seen
    r.frameIndex = 0
    r.draw(1, wait=True)
    _same(_image(samples[0], w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: frame 0")
    assert samples[0].any()
    r.draw(2, wait=True)
    assert r.frameIndex == 3
    folded = R.running_average([s.cpu().numpy() for s in samples])
    _same(_image(folded, w, h).reshape(-1, 4), r.accumulation().reshape(-1, 4), f"{name} {extra}: three frames")
