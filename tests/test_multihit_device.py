"""All-hits ray queries on device buffers (DeviceScene.intersect_all_device): per ray the K smallest hits under (distance, triangle id), in order.  Every
record and every count must have the bits of tests/multihit_reference.py — every triangle against every ray, pinned to the oracle without a GPU by
tests/test_multihit_cpu.py — in every layout and for every builder, before and after a refit; record 0 must be intersect_closest_device's record and count > 0
intersect_any_device's answer.  The reference of a scene is computed once for K = 16: the answer for a smaller K is its first K entries, by the definition."""
import functools
import gc

import numpy as np
import pytest

import multihit_reference as M
from test_gpu_parity import _rays

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0x7F7F7F7F
KS = (1, 3, 8, 16)
LAYOUTS = {"wide_b1": {"builder": 1}, "wide_b2": {"builder": 2}, "wide_rope": {"rope": 1}, "rope_b0": {"wide": 0, "builder": 0}, "rope_b1": {"wide": 0, "builder": 1}}
INTERIOR, DIAGONAL, CORNER = (0.75, 0.25), (0.5, 0.5), (1.0, 1.0)


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_dev(ctx))


def _query(mrt, ds, ctx, rays, K, **kw):
    """-> (hits (n, K) records, counts (n,)) as numpy"""
    import torch
    h, c = ds.intersect_all_device(_t(rays, ctx), K, **kw)
    torch.cuda.synchronize()
    assert h.dtype == torch.int32 and tuple(h.shape) == (len(rays), K, 8) and c.dtype == torch.int32 and tuple(c.shape) == (len(rays),)
    return h.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(len(rays), K), c.cpu().numpy()


def _first(ref16, K):
    """the reference for K from the reference for 16: the first K entries"""
    h, c = ref16
    return np.ascontiguousarray(h[:, :K]), np.minimum(c, K).astype(np.int32)


def _assert_same(got, want, what):
    (gh, gc), (wh, wc) = got, want
    assert gh.shape == wh.shape and gh.dtype == wh.dtype, what
    bad = np.flatnonzero(gc != wc)
    assert bad.size == 0, f"{what}: {bad.size} counts differ; first at ray {bad[0]}: {gc[bad[0]]} != {wc[bad[0]]}"
    x = np.ascontiguousarray(gh).view(np.uint32).reshape(*gh.shape, 8); y = np.ascontiguousarray(wh).view(np.uint32).reshape(*wh.shape, 8)
    bad = np.argwhere((x != y).any(-1))
    assert bad.size == 0, f"{what}: {len(bad)} records differ; first at ray {bad[0][0]} slot {bad[0][1]}: {gh[tuple(bad[0])]} != {wh[tuple(bad[0])]}"


def _stack_rays(layers):
    """+z through a quad's interior, the shared diagonal and the shared corner, open and with windows that end exactly on a layer"""
    rows = []
    for xy in (INTERIOR, DIAGONAL, CORNER):
        rows.append([*xy, 0.0, 0.0, 0, 0, 1, np.inf])
        rows.append([*xy, 0.0, 2.0, 0, 0, 1, float(max(layers - 1, 2))])
        rows.append([*xy, float(layers + 1), 0.0, 0, 0, -1, np.inf])          # from above: the layers in reverse, ids still ascending inside a tie
    rows.append([2.0, 2.0, 0.0, 0.0, 0, 0, 1, np.inf])                          # beside the stack: nothing
    return np.array(rows, f32)


@functools.lru_cache(maxsize=None)
def _model_case(mrt, name):
    """scene, its flatten_scene tuples, 500 rays (six axis directions among them, a quarter with windows) and the reference for K = 16; made once, never modified"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name=name, position=[0.1, -0.2, 0.3], rotation=[0.2, 0.5, -0.1], scale=1.3),
                           mrt.Model(name="plane", position=[0, -3, 0], scale=50)]
    sc = S((8, 8))
    entries = mrt.flatten_scene(sc)
    me = sc.meshes[0]
    w = (me.transform.T @ np.c_[me.positions, np.ones(len(me.positions))].T).T[:, :3]
    rays = _rays(np.random.default_rng(11), 500, w.min(0), w.max(0))
    rays[:6, 4:7] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    k = np.arange(len(rays))
    rays[k % 4 == 1, 3] = 1.5
    rays[k % 8 == 3, 7] = 3.0
    ref = M.MultihitReference(entries)
    ref16 = ref.intersect_all(rays, 16)
    for a in (rays, *ref16): a.setflags(write=False)
    return sc, entries, rays, ref16


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_quad_stack_and_coincident_meshes(mrt, gpu_ctx, layout):
    for L in (1, 3, 9, 17):
        sc = M.quad_stack(mrt, L)
        ref = M.MultihitReference(mrt.flatten_scene(sc))
        rays = _stack_rays(L)
        ref16 = ref.intersect_all(rays, 16)
        assert ref16[1][0] == min(L, 16) and ref16[1][3] == min(2 * L, 16)          # the interior ray meets every layer once, the diagonal ray twice
        ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
        try:
            for K in (1, 2, 3, 16):
                _assert_same(_query(mrt, ds, gpu_ctx, rays, K), _first(ref16, K), f"{layout} stack of {L}, K = {K}")
        finally:
            ds.close()
    p1, i1 = M.quad(1.0); p2, i2 = M.quad(2.0)
    sc = M.raw_scene(mrt, [(p1, i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p2, i2, M._plain(mrt)), (p2.copy(), i2, M._plain(mrt))])
    ref16 = M.MultihitReference(mrt.flatten_scene(sc)).intersect_all(_stack_rays(2), 16)
    assert list(ref16[0][0, :4]["instance_id"]) == [0, 1, 2, 3] and list(ref16[0][0, :4]["distance"]) == [1.0, 1.0, 2.0, 2.0]
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    try:
        for K in (1, 2, 3, 16):
            _assert_same(_query(mrt, ds, gpu_ctx, _stack_rays(2), K), _first(ref16, K), f"{layout} coincident meshes, K = {K}")
    finally:
        ds.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", ["sphere", "train", "teapot"])
def test_models_equal_the_reference(mrt, gpu_ctx, name, layout):
    sc, _, rays, ref16 = _model_case(mrt, name)
    assert (ref16[1] >= 3).mean() > 0.2 and (ref16[1] == 0).any(), "the rays must hold lists longer than one hit, and misses"
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    try:
        assert ds.stats.wide_layout == (0 if layout.startswith("rope") else 1)
        for K in KS:
            _assert_same(_query(mrt, ds, gpu_ctx, rays, K), _first(ref16, K), f"{name} {layout} K = {K}")
    finally:
        ds.close()


# ---------------------------------------------------------------- 2. pre-split references
def _needles():
    """six slivers 60 long and at most 0.4 wide, rising across the sphere-over-plane scene: what the build's pre-splitting cuts into references (it leaves fat triangles —
    the plane's two — whole: k_split_count)"""
    pos, idx = [], []
    for k in range(6):
        z0 = -10.0 + 4.0 * k
        pos += [[-30.0, -2.5, z0], [30.0, 0.5 + 0.1 * k, z0], [30.0, 0.5 + 0.1 * k, z0 + 0.4]]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    return np.array(pos, f32), np.array(idx, np.uint32)


def test_a_presplit_triangle_is_listed_once(mrt, gpu_ctx):
    """The sphere over the plane with six long slivers between them.  The scene must hold more packets than triangles (asserted from the layout read-back: without that
    the test could pass because nothing was split).  A sliver's references are slabs across its long axis, x: rays aimed at the slab boundaries of a 32-way split (and
    of every coarser power of two) pass through the boxes of two references of one triangle; random rays through slivers and plane join them."""
    base = _model_case(mrt, "sphere")[0]
    npos, nidx = _needles()

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = list(base.models) + [M._Raw(mrt, "needles", npos, np.tile(np.array([0, 1, 0], f32), (len(npos), 1)), nidx, M._plain(mrt))]
    sc = S((8, 8))
    ref = M.MultihitReference(mrt.flatten_scene(sc))
    rng = np.random.default_rng(3)
    rows = []
    for k in range(6):
        z0 = -10.0 + 4.0 * k
        for p in range(1, 32):
            x = -30.0 + 60.0 * p / 32.0
            rows.append([x, 5.0, z0 + 0.2 * (x + 30.0) / 60.0, 0.0, 0.0, -1.0, 0.0, np.inf])
    for _ in range(200):          # slanted rays that run along a sliver
        k = rng.integers(0, 6); x = rng.uniform(-25, 25); d = np.array([rng.uniform(-1, 1), -1.0, rng.uniform(-0.02, 0.02)]); d /= np.linalg.norm(d)
        hit = np.array([x, -2.5 + (3.0 + 0.1 * k) * (x + 30.0) / 60.0, -10.0 + 4.0 * k + 0.2 * (x + 30.0) / 60.0])
        rows.append([*(hit - 4.0 * d), 0.0, *d, np.inf])
    rays = np.array(rows, f32)
    want = ref.intersect_all(rays, 16)
    needle = want[0]["instance_id"] == 2
    assert (needle.sum(1) >= 1).mean() > 0.9 and (want[1] >= 2).mean() > 0.9, "the rays must cross a sliver, and the plane behind it"
    split = mrt.DeviceScene(gpu_ctx, sc); whole = mrt.DeviceScene(gpu_ctx, sc, {"presplit": 0})
    try:
        assert int(split.read_layout("header")[4]) >= split.stats.triangles + 6 * 8, "nothing was split: the test would pass for no reason"
        assert int(whole.read_layout("header")[4]) == whole.stats.triangles
        got = _query(mrt, split, gpu_ctx, rays, 16)
        for r in range(len(rays)):
            ids = [(int(h["instance_id"]), int(h["geometry_id"]), int(h["primitive_id"])) for h in got[0][r, :got[1][r]]]
            assert len(set(ids)) == len(ids), f"ray {r} lists a triangle twice: {ids}"
        for K in (1, 2, 16):
            _assert_same(_query(mrt, split, gpu_ctx, rays, K), _first(want, K), f"pre-split, K = {K}")
            _assert_same(_query(mrt, whole, gpu_ctx, rays, K), _first(want, K), f"presplit = 0, K = {K}")
    finally:
        split.close(); whole.close()


# ---------------------------------------------------------------- 3. agreement with the other entries
@pytest.mark.parametrize("layout", ["wide_b1", "rope_b1"])
def test_first_record_is_the_closest_hit_and_count_is_any_hit(mrt, gpu_ctx, layout):
    import torch
    sc, _, _, _ = _model_case(mrt, "train")
    me = sc.meshes[0]
    w = (me.transform.T @ np.c_[me.positions, np.ones(len(me.positions))].T).T[:, :3]
    rays = _rays(np.random.default_rng(21), 3006, w.min(0), w.max(0))
    rays[:6, 4:7] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    k = np.arange(len(rays))
    rays[k % 4 == 1, 3] = np.asarray([1e-3, 1.5, 3.0], f32)[(k[k % 4 == 1] // 4) % 3]
    rays[k % 4 == 2, 7] = 2.5
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    try:
        d = _t(rays, gpu_ctx)
        closest = ds.intersect_closest_device(d); occluded = ds.intersect_any_device(d)
        for K in (1, 4, 16):
            h, c = ds.intersect_all_device(d, K)
            torch.cuda.synchronize()
            assert torch.equal(h[:, 0, :], closest), f"K = {K}: {(h[:, 0, :] != closest).any(1).sum().item()} first records differ from intersect_closest_device"
            assert torch.equal((c > 0).to(torch.int32), occluded), f"K = {K}"
        assert 0.3 < float(occluded.float().mean()) < 1.0
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. launch shapes, the device-side count
@pytest.mark.parametrize("layout", ["wide_b1", "rope_b1"])
def test_launch_shapes_and_the_device_side_count(mrt, gpu_ctx, layout):
    import torch
    sc, _, rays, ref16 = _model_case(mrt, "sphere")
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    dev = _dev(gpu_ctx)
    K = 3
    try:
        for n in (1, 63, 64, 65, 257):
            want = _first((ref16[0][:n], ref16[1][:n]), K)
            d = _t(rays[:n], gpu_ctx)
            for count in (None, n, n // 2, 0):
                out = torch.full((n, K, 8), SENTINEL, dtype=torch.int32, device=dev); cnt = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
                word = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
                h, c = ds.intersect_all_device(d, K, out=out, counts_out=cnt, count=word)
                torch.cuda.synchronize()
                assert h is out and c is cnt
                m = n if count is None else count
                assert (out[m:] == SENTINEL).all().item() and (cnt[m:] == SENTINEL).all().item(), (n, count, "a row at or past the count was written")
                assert not (out[:m] == SENTINEL).any().item() and not (cnt[:m] == SENTINEL).any().item(), (n, count, "a record below the count was not written")
                got = (out[:m].cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(m, K), cnt[:m].cpu().numpy())
                _assert_same(got, (want[0][:m], want[1][:m]), f"{layout} n = {n} count = {count}")
        e = torch.empty((0, 8), dtype=torch.float32, device=dev)
        h, c = ds.intersect_all_device(e, K)                                            # n == 0: MRT_OK, nothing launched
        assert tuple(h.shape) == (0, K, 8) and tuple(c.shape) == (0,)
        for bad_k in (0, 17, -1, 2.0):
            with pytest.raises((ValueError, TypeError)):
                ds.intersect_all_device(d, bad_k)
        with pytest.raises((ValueError, TypeError)):
            ds.intersect_all_device(d, K, out=torch.empty((len(d), K, 8), dtype=torch.float32, device=dev))
        with pytest.raises((ValueError, TypeError)):
            ds.intersect_all_device(d, K, counts_out=torch.empty((len(d) + 1,), dtype=torch.int32, device=dev))
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. streams
def test_a_side_stream_and_the_null_stream_agree(mrt, gpu_ctx):
    import torch
    sc, _, rays, ref16 = _model_case(mrt, "teapot")
    ds = mrt.DeviceScene(gpu_ctx, sc)
    dev = _dev(gpu_ctx)
    try:
        src = _t(rays, gpu_ctx); torch.cuda.synchronize()
        side = torch.cuda.Stream(dev)
        assert side.cuda_stream not in (0, gpu_ctx.stream)
        got = []
        for stream, handle in ((side, None), (torch.cuda.default_stream(dev), 0)):
            with torch.cuda.stream(stream):
                big = torch.randn(1024, 1024, device=dev) @ torch.randn(1024, 1024, device=dev)          # the stream is busy when the rays are made
                d = torch.where(torch.isnan(big[0, 0]), src, (src * 2.0) * 0.5).contiguous()              # exact; exists only once this stream reaches it
                h, c = ds.intersect_all_device(d, 8, stream=handle)          # None: torch's current stream = the side stream; 0: the null stream
                folded = torch.stack([h.to(torch.int64).sum(), c.to(torch.int64).sum()])
            stream.synchronize()
            got.append((h.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(len(rays), 8), c.cpu().numpy(), folded.cpu().numpy()))
        _assert_same(got[0][:2], _first(ref16, 8), "side stream"); _assert_same(got[1][:2], _first(ref16, 8), "null stream")
        assert np.array_equal(got[0][2], got[1][2])
    finally:
        ds.close()


# ---------------------------------------------------------------- 6. a deformed scene
@pytest.mark.parametrize("layout", ["wide_b1", "wide_rope", "rope_b1"])
def test_after_update_mesh_device_and_refit_device(mrt, gpu_ctx, layout):
    sc, entries, rays, ref16 = _model_case(mrt, "sphere")
    pos, nrm = np.asarray(entries[0][0], f32), np.asarray(entries[0][1], f32)
    moved = (pos + f32(0.08) * np.sin(f32(5.0) * pos[:, [2, 0, 1]])).astype(f32)
    ref = M.MultihitReference(entries); ref.set_mesh(0, moved)
    want = ref.intersect_all(rays, 16)
    assert M.differing(want[0], ref16[0]) > 100, "the displacement must change the answers"
    a = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout]); b = mrt.DeviceScene(gpu_ctx, sc, {**LAYOUTS[layout], "refit": 0})
    try:
        _assert_same(_query(mrt, a, gpu_ctx, rays, 8), _first(ref16, 8), "before the update")
        a.update_mesh_device(0, _t(moved, gpu_ctx), _t(nrm, gpu_ctx)); a.refit_device()
        b.update_mesh(0, moved, nrm); b.commit()          # refit = 0: this commit BUILDS the deformed scene
        assert b.refits == 0
        for K in (1, 8, 16):
            got = _query(mrt, a, gpu_ctx, rays, K)
            _assert_same(got, _first(want, K), f"{layout} refitted, K = {K}")
            _assert_same(got, _query(mrt, b, gpu_ctx, rays, K), f"{layout} refitted against freshly built, K = {K}")
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 7. scenes at the edges
def test_empty_scene(mrt, gpu_ctx):
    class Empty(mrt.Scene):
        pass
    rays = _rays(np.random.default_rng(0), 100, np.zeros(3), np.ones(3))
    for options in (None, {"wide": 0}):
        ds = mrt.DeviceScene(gpu_ctx, Empty((8, 8)), options)
        try:
            assert ds.stats.triangles == 0
            h, c = _query(mrt, ds, gpu_ctx, rays, 4)
            assert (c == 0).all() and M.differing(h, np.broadcast_to(M.miss_record(), h.shape).copy()) == 0
        finally:
            ds.close()


def test_two_level_scene_is_refused(mrt, gpu_ctx):
    import torch
    sc, _, rays, _ = _model_case(mrt, "sphere")
    dev = _dev(gpu_ctx)
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    try:
        d = _t(rays[:64], gpu_ctx)
        out = torch.full((64, 4, 8), SENTINEL, dtype=torch.int32, device=dev); cnt = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
        for count in (None, torch.tensor([64], dtype=torch.int32, device=dev)):
            with pytest.raises(mrt.MRTError) as e:
                ds.intersect_all_device(d, 4, out=out, counts_out=cnt, count=count)
            assert e.value.code == 7 and "two-level" in str(e.value)          # MRT_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (out == SENTINEL).all().item() and (cnt == SENTINEL).all().item()
    finally:
        ds.close()
    flat = mrt.DeviceScene(gpu_ctx, sc)
    try:
        flat.set_instance_transform(0, np.eye(4, dtype=f32).reshape(16))          # not committed any more
        with pytest.raises(mrt.MRTError) as e:
            flat.intersect_all_device(d, 4)
        assert e.value.code == 5          # MRT_ERR_STATE
    finally:
        flat.close()


# ---------------------------------------------------------------- 8. composition: what a shadow ray lets through
def test_transmittance_from_hits_resolve_and_the_slot_column(mrt, gpu_ctx):
    import torch
    L, K = 6, 8
    dissolve = [0.5 if k % 2 == 0 else 1.0 for k in range(L)]
    sc = M.quad_stack(mrt, L, dissolve=dissolve)
    table = np.array([m.submeshes[0].material.dissolve for m in sc.meshes], f32)          # per resource slot (one submesh per mesh): from the scene's materials, on the host
    assert list(table) == dissolve
    rays = np.array([[*INTERIOR, 0.0, 0.0, 0, 0, 1, np.inf], [*INTERIOR, 0.0, 0.0, 0, 0, 1, 3.5], [*INTERIOR, 0.0, 1.5, 0, 0, 1, np.inf], [2.0, 2.0, 0.0, 0.0, 0, 0, 1, np.inf],
                     [*INTERIOR, 7.0, 0.0, 0, 0, -1, 2.5]], f32)
    layers = [[0, 1, 2, 3, 4, 5], [0, 1, 2], [1, 2, 3, 4, 5], [], [5, 4]]          # the quads each ray crosses, in its order (the last ray comes from above)
    want = np.array([np.prod([f32(dissolve[k]) for k in ls], dtype=f32) if len(ls) else f32(1.0) for ls in layers], f32)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    try:
        d = _t(rays, gpu_ctx)
        hits, counts = ds.intersect_all_device(d, K)
        surf = ds.resolve_hits_device(d.repeat_interleave(K, 0).contiguous(), hits.view(-1, 8))
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [len(ls) for ls in layers]
        s = mrt.unpack_surfaces(surf).reshape(len(rays), K)
        valid = np.arange(K)[None, :] < counts.cpu().numpy()[:, None]
        assert (s["type"][valid] == 1).all() and (s["resource_slot"][valid] >= 0).all()
        import surface_reference as S
        assert S.differing(s[~valid], np.broadcast_to(S.miss_record(), s[~valid].shape).copy()) == 0, "padding rows are the surface miss record"
        slot = torch.from_numpy(s["resource_slot"].copy()).to(_dev(gpu_ctx)).to(torch.int64)
        through = torch.where(slot >= 0, _t(table, gpu_ctx)[slot.clamp(min=0)], torch.ones((), device=_dev(gpu_ctx))).prod(1)
        assert np.array_equal(through.cpu().numpy(), want), (through.cpu().numpy(), want)
        assert [[int(x) for x in s["instance_id"][r][valid[r]]] for r in range(len(rays))] == layers
    finally:
        ds.close()


# ---------------------------------------------------------------- 9. nothing is allocated
@pytest.mark.parametrize("layout", ["wide_b1", "rope_b1"])
def test_nothing_is_allocated(mrt, gpu_ctx, layout):
    import torch
    sc, _, rays, ref16 = _model_case(mrt, "sphere")
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    dev = _dev(gpu_ctx)
    try:
        d = _t(rays, gpu_ctx)
        out = torch.empty((len(rays), 16, 8), dtype=torch.int32, device=dev); cnt = torch.empty((len(rays),), dtype=torch.int32, device=dev)
        word = torch.tensor([len(rays)], dtype=torch.int32, device=dev)
        ds.intersect_all_device(d, 16, out=out, counts_out=cnt); ds.intersect_all_device(d, 16, out=out, counts_out=cnt, count=word)          # the warm calls
        torch.cuda.synchronize()
        gc.collect()          # tensors that earlier tests left in reference cycles are freed now, not by a collection in the middle of the loop (as tests/test_masked_device.py does)
        before = (torch.cuda.memory_allocated(dev), torch.cuda.mem_get_info(dev)[0])
        for k in range(20):
            ds.intersect_all_device(d, 16, out=out, counts_out=cnt, count=word if k % 2 else None)
        torch.cuda.synchronize()
        assert (torch.cuda.memory_allocated(dev), torch.cuda.mem_get_info(dev)[0]) == before
        _assert_same((out.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(len(rays), 16), cnt.cpu().numpy()), _first(ref16, 16), "after 20 calls")
    finally:
        ds.close()
