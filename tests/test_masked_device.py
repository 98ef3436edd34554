"""Visibility masks on device buffers (DeviceScene.set_mesh_masks, mask= of intersect_closest_device / _any_device / _all_device).  Every record and every
count must have the bits of tests/masked_reference.py — MultihitReference on the visible triangles alone, pinned to the oracle without a GPU by tests/test_masked_cpu.py —
in every flattened layout; two-level scenes are compared with the unmasked entries of a two-level scene built from the visible entries only, and with the oracle.  Wherever
the three queries run on the same rays, record 0 of the list must be the closest record and count > 0 the any-hit answer."""
import ctypes as C
import functools
import gc
import os
import re
import subprocess

import numpy as np
import pytest

import masked_reference as R
import multihit_reference as M
from test_gpu_parity import _rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SENTINEL = 0x7F7F7F7F
LAYOUTS = {"wide_b1": {"builder": 1}, "wide_b2": {"builder": 2}, "wide_rope": {"rope": 1}, "rope_b0": {"wide": 0, "builder": 0}, "rope_b1": {"wide": 0, "builder": 1}}
TWO_LEVEL = {"tl_wide": {"instancing": 1}, "tl_rope": {"instancing": 1, "wide": 0}}
INTERIOR, DIAGONAL, CORNER = (0.75, 0.25), (0.5, 0.5), (1.0, 1.0)


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_dev(ctx))


def _mask_arg(masks, ctx):
    """an int stays an int (one mask for every ray); an array becomes the per-ray tensor"""
    if isinstance(masks, (int, np.integer)): return int(masks)
    return _t(np.asarray(masks, np.int64).astype(np.uint32).view(np.int32), ctx)


def _records(mrt, t):
    return t.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(t.shape[:-1])


def _closest_any(mrt, ds, ctx, rays, masks):
    import torch
    d = _t(rays, ctx); m = _mask_arg(masks, ctx)
    c = ds.intersect_closest_device(d, mask=m); a = ds.intersect_any_device(d, mask=m)
    torch.cuda.synchronize()
    return _records(mrt, c), a.cpu().numpy()


def _all(mrt, ds, ctx, rays, masks, K):
    import torch
    h, c = ds.intersect_all_device(_t(rays, ctx), K, mask=_mask_arg(masks, ctx))
    torch.cuda.synchronize()
    return _records(mrt, h), c.cpu().numpy()


def _assert_records(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    x = np.ascontiguousarray(got).view(np.uint32).reshape(*got.shape, 8); y = np.ascontiguousarray(want).view(np.uint32).reshape(*want.shape, 8)
    bad = np.argwhere((x != y).any(-1))
    assert bad.size == 0, f"{what}: {len(bad)} records differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _check_three(mrt, ds, ctx, rays, masks, ref16, what, Ks=(1, 3, 16)):
    """closest, any and all-hits against the reference for K = 16 (a smaller K is its first K entries), and against each other"""
    wh, wc = ref16
    closest, occluded = _closest_any(mrt, ds, ctx, rays, masks)
    _assert_records(closest, wh[:, 0], f"{what}: closest")
    assert np.array_equal(occluded, (wc > 0).astype(np.int32)), f"{what}: any, {(occluded != (wc > 0)).sum()} differ"
    for K in Ks:
        h, c = _all(mrt, ds, ctx, rays, masks, K)
        assert np.array_equal(c, np.minimum(wc, K)), f"{what}: K = {K}: {(c != np.minimum(wc, K)).sum()} counts differ"
        _assert_records(h, np.ascontiguousarray(wh[:, :K]), f"{what}: K = {K}")
        _assert_records(h[:, 0], closest, f"{what}: K = {K}: record 0 against masked closest")
        assert np.array_equal((c > 0).astype(np.int32), occluded), f"{what}: K = {K}: count > 0 against masked any"


def _two_level_expected(mrt, ctx, scene_of, options, mesh_masks, rays, rm, orc=None):
    """What a two-level scene must answer: per distinct ray mask, the EXISTING intersect_closest_device / _any_device of a two-level scene built from the visible entries
    only (scene_of(visible ids)), its instance ids mapped back; orc: the oracle's two-level restatement on the same entries must agree -> (closest records, any)"""
    closest = np.empty(len(rays), mrt.INTERSECTION_DTYPE); closest[:] = M.miss_record()
    occluded = np.zeros(len(rays), np.int32)
    for m in np.unique(rm):
        visible = tuple(i for i, mm in enumerate(mesh_masks) if int(mm) & int(m))
        if not visible: continue
        sel = rm == m
        part = scene_of(visible)
        back = np.array(visible, np.int32)
        sub = mrt.DeviceScene(ctx, part, options)
        try:
            d = _t(rays[sel], ctx)
            want = _records(mrt, sub.intersect_closest_device(d)).copy(); occluded[sel] = sub.intersect_any_device(d).cpu().numpy()
        finally:
            sub.close()
        want["instance_id"] = np.where(want["type"] == 1, back[np.clip(want["instance_id"], 0, None)], -1)
        closest[sel] = want
        if orc is not None:
            osc = orc.OracleScene(mrt.flatten_scene(part, share=True), part.lights, instancing=True)
            try:
                o = osc.intersect_closest(rays[sel]); oa = osc.intersect_any(rays[sel])
            finally:
                osc.close()
            o["instance_id"] = np.where(o["type"] == 1, back[np.clip(o["instance_id"], 0, None)], -1)
            _assert_records(want, o, f"instances {visible}: the sub-scene against the oracle")
            assert np.array_equal(occluded[sel], oa), visible
    return closest, occluded


def _stack_rays(layers):
    """+z through a quad's interior, the shared diagonal and the shared corner, open and with windows that end exactly on a layer; from above; beside the stack"""
    rows = []
    for xy in (INTERIOR, DIAGONAL, CORNER):
        rows.append([*xy, 0.0, 0.0, 0, 0, 1, np.inf])
        rows.append([*xy, 0.0, 2.0, 0, 0, 1, float(max(layers - 1, 2))])
        rows.append([*xy, float(layers + 1), 0.0, 0, 0, -1, np.inf])
    rows.append([2.0, 2.0, 0.0, 0.0, 0, 0, 1, np.inf])
    return np.array(rows, f32)


def _stack_case(L):
    """every ray of _stack_rays under every mask of a list that holds 0, single quads, alternating quads, everything but the first, everything"""
    full = (1 << L) - 1
    masks = sorted({0, 1, 1 << (L - 1), full & 0x15555, full & 0x0AAAA, full & ~1, full & 0x6, full, R.ALL})
    base = _stack_rays(L)
    rays = np.repeat(base, len(masks), 0)
    rm = np.tile(np.array(masks, np.int64), len(base))
    return rays, rm, masks


def _coincident_case(mrt):
    p1, i1 = M.quad(1.0); p2, i2 = M.quad(2.0)
    sc = M.raw_scene(mrt, [(p1, i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p1.copy(), i1, M._plain(mrt)), (p2, i2, M._plain(mrt))])
    mm = [2, 1, 4, 1]
    masks = np.array([1, 2, 3, 4, 5, 6, 7], np.int64)
    base = _stack_rays(2)
    rays = np.repeat(base, len(masks), 0); rm = np.tile(masks, len(base))
    ref16 = R.MaskedReference(mrt.flatten_scene(sc), mm).intersect_all(rays, 16, rm)
    first = {int(m): int(ref16[0][k, 0]["instance_id"]) for k, m in enumerate(masks)}          # the interior ray, open: its closest hit under each mask
    assert first == {1: 1, 2: 0, 3: 0, 4: 2, 5: 1, 6: 0, 7: 0} and (ref16[0][:7, 0]["distance"] == 1.0).all()
    k = 3 * len(masks) + 4          # the diagonal ray under mask 5: both triangles of meshes 1 and 2 at one distance, then mesh 3
    assert rm[k] == 5 and list(ref16[0][k, :6]["instance_id"]) == [1, 1, 2, 2, 3, 3] and list(ref16[0][k, :4]["distance"]) == [1.0] * 4
    return sc, mm, rays, rm, ref16


def _many_coincident_case(mrt):
    """eight coincident quads in eight meshes (quad k: 1 << k) over a ninth (0x100), every ray of _stack_rays under EVERY subset of the nine bits.  Sixteen triangles at one
    distance do not fit one leaf, so a walk meets them in an order that is not the id order, and some subset has a visible triangle, then a lower invisible one, then a
    visible one between the two: a tie decided before the filter reports the first of them"""
    p1, i1 = M.quad(1.0); p2, i2 = M.quad(2.0)
    sc = M.raw_scene(mrt, [(p1.copy(), i1, M._plain(mrt)) for _ in range(8)] + [(p2, i2, M._plain(mrt))])
    mm = [1 << k for k in range(8)] + [0x100]
    base = _stack_rays(2)
    rays = np.repeat(base, 512, 0); rm = np.tile(np.arange(512, dtype=np.int64), len(base))
    ref16 = R.MaskedReference(mrt.flatten_scene(sc), mm).intersect_all(rays, 16, rm)
    lowest = np.array([-1 if m == 0 else (int(m) & -int(m)).bit_length() - 1 for m in range(512)])          # the interior ray, open: the lowest visible mesh
    assert np.array_equal(ref16[0][:512, 0]["instance_id"], lowest) and (ref16[0][1:256, 0]["distance"] == 1.0).all() and ref16[0][256, 0]["distance"] == 2.0
    return sc, mm, rays, rm, ref16


# ---------------------------------------------------------------- 1. against the reference: known answers
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_quad_stacks_and_coincident_quads(mrt, gpu_ctx, layout):
    for L in (1, 3, 17):
        sc = M.quad_stack(mrt, L)
        ref = R.MaskedReference(mrt.flatten_scene(sc), R.quad_stack_masks(L))
        rays, rm, masks = _stack_case(L)
        ref16 = ref.intersect_all(rays, 16, rm)
        first = np.flatnonzero(rm == masks[-2])[0]          # the interior ray with every quad's bit: every layer once
        assert ref16[1][first] == min(L, 16) and (ref16[1][rm == 0] == 0).all()
        ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
        try:
            ds.set_mesh_masks(R.quad_stack_masks(L))
            _check_three(mrt, ds, gpu_ctx, rays, rm, ref16, f"{layout} stack of {L}, a mask per ray")
            for m in masks:          # the same mask for a whole call
                sel = rm == m
                _check_three(mrt, ds, gpu_ctx, rays[sel], int(m), (ref16[0][sel], ref16[1][sel]), f"{layout} stack of {L}, mask {m:#x}", Ks=(3,))
        finally:
            ds.close()
    # three coincident quads in different meshes over a fourth quad: with the lower ids invisible a higher id is reported, at the same distance — whatever the order in
    # which the walk meets the three, the tie is decided among the visible ones
    for case, what in ((_coincident_case, "three coincident quads"), (_many_coincident_case, "eight coincident quads under every subset")):
        sc, mm, rays, rm, ref16 = case(mrt)
        ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
        try:
            ds.set_mesh_masks(mm)
            _check_three(mrt, ds, gpu_ctx, rays, rm, ref16, f"{layout} {what}")
        finally:
            ds.close()


# ---------------------------------------------------------------- 2. against the reference: models
MODEL_MESH_MASKS = ([1, 2, 4, 8], [1, 1, 2, 2], [3, 6, 12, 0x80000001], [R.ALL, 0, 5, 0x10])
MODEL_RAY_MASKS = (1, 2, 4, 8, 3, 6, 10, 0x80000000, 0, R.ALL, 0x10)


@functools.lru_cache(maxsize=None)
def _model_case(mrt):
    """the scene, its entries, 1500 rays — 500 aimed at each model's box, a quarter with windows — a mask per ray that changes from lane to lane, and per list of mesh
    masks the reference for K = 16; made once, never modified"""
    sc = R.three_models(mrt)
    entries = mrt.flatten_scene(sc)
    parts = []
    for k, me in enumerate(sc.meshes[:3]):
        w = (me.transform.T @ np.c_[me.positions, np.ones(len(me.positions))].T).T[:, :3]
        parts.append(_rays(np.random.default_rng(40 + k), 500, w.min(0), w.max(0)))
    rays = np.concatenate(parts)
    rays[:6, 4:7] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    k = np.arange(len(rays))
    rays[k % 4 == 1, 3] = 0.75
    rays[k % 8 == 3, 7] = 3.0
    rm = np.array(MODEL_RAY_MASKS, np.int64)[(k * 7 + k // 64) % len(MODEL_RAY_MASKS)]
    assert len(set(rm[:64])) == len(MODEL_RAY_MASKS)          # the masks vary inside one wave
    refs = []
    for mm in MODEL_MESH_MASKS:
        ref16 = R.MaskedReference(entries, mm).intersect_all(rays, 16, rm)
        for a in ref16: a.setflags(write=False)
        refs.append(ref16)
    rays.setflags(write=False); rm.setflags(write=False)
    return sc, entries, rays, rm, refs


@functools.lru_cache(maxsize=None)
def _one_mask_case(mrt):
    """every third ray of _model_case under ONE mask for the whole call, per mask of a short list: the reference under the last list of mesh masks"""
    sc, entries, rays, rm, refs = _model_case(mrt)
    sel = np.arange(0, len(rays), 3)
    ref = R.MaskedReference(entries, MODEL_MESH_MASKS[-1])
    return sel, {m: ref.intersect_all(rays[sel], 16, m) for m in (2, 6, 0x80000000)}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_models_equal_the_reference(mrt, gpu_ctx, layout):
    sc, entries, rays, rm, refs = _model_case(mrt)
    assert (refs[0][1] >= 2).mean() > 0.1 and (refs[0][1] == 0).mean() > 0.1, "the rays must hold lists longer than one hit, and misses"
    assert M.differing(refs[0][0], refs[1][0]) > 100, "the mesh masks must change the answers"
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    try:
        assert ds.stats.wide_layout == (0 if layout.startswith("rope") else 1)
        for mm, ref16 in zip(MODEL_MESH_MASKS, refs):
            ds.set_mesh_masks(mm)          # a committed scene: at once, no commit
            assert list(ds.mesh_masks()) == list(mm)
            _check_three(mrt, ds, gpu_ctx, rays, rm, ref16, f"{layout} mesh masks {mm}, a mask per ray", Ks=(1, 4, 16))
        sel, wants = _one_mask_case(mrt)          # one mask for a whole call, under the last list of mesh masks
        for m, want in wants.items():
            _check_three(mrt, ds, gpu_ctx, rays[sel], m, want, f"{layout} one mask {m:#x}", Ks=(4,))
    finally:
        ds.close()


# ---------------------------------------------------------------- 3. a triangle the build pre-splits
def _needles():
    """six slivers 60 long and at most 0.4 wide (tests/test_multihit_device.py's): what the build's pre-splitting cuts into references"""
    pos, idx = [], []
    for k in range(6):
        z0 = -10.0 + 4.0 * k
        pos += [[-30.0, -2.5, z0], [30.0, 0.5 + 0.1 * k, z0], [30.0, 0.5 + 0.1 * k, z0 + 0.4]]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    return np.array(pos, f32), np.array(idx, np.uint32)


def test_a_presplit_sliver_is_gone_when_invisible_and_listed_once_when_visible(mrt, gpu_ctx):
    npos, nidx = _needles()

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="sphere", position=[0.1, -0.2, 0.3], rotation=[0.2, 0.5, -0.1], scale=1.3), mrt.Model(name="plane", position=[0, -3, 0], scale=50),
                           M._Raw(mrt, "needles", npos, np.tile(np.array([0, 1, 0], f32), (len(npos), 1)), nidx, M._plain(mrt))]
    sc = S((8, 8))
    ref = R.MaskedReference(mrt.flatten_scene(sc), [1, 1, 2])
    rows = []
    for k in range(6):          # rays aimed at the slab boundaries of a 32-way split: through the boxes of two references of one triangle
        z0 = -10.0 + 4.0 * k
        for p in range(1, 32):
            x = -30.0 + 60.0 * p / 32.0
            rows.append([x, 5.0, z0 + 0.2 * (x + 30.0) / 60.0, 0.0, 0.0, -1.0, 0.0, np.inf])
    rays = np.array(rows, f32)
    rm = np.array([1, 3, 2], np.int64)[np.arange(len(rays)) % 3]
    want = ref.intersect_all(rays, 16, rm)
    sliver = (want[0]["instance_id"] == 2).sum(1)
    assert (sliver[rm == 1] == 0).all() and (sliver[rm != 1] == 1).mean() > 0.9 and (want[1][rm == 3] >= 2).mean() > 0.9
    ds = mrt.DeviceScene(gpu_ctx, sc)
    try:
        assert int(ds.read_layout("header")[4]) >= ds.stats.triangles + 6 * 8, "nothing was split: the test would pass for no reason"
        ds.set_mesh_masks([1, 1, 2])
        _check_three(mrt, ds, gpu_ctx, rays, rm, want, "pre-split slivers", Ks=(1, 2, 16))
    finally:
        ds.close()


# ---------------------------------------------------------------- 4. launch shapes, the device-side count, sentinel-filled outputs
@pytest.mark.parametrize("layout", ["wide_b1", "rope_b1", "tl_wide"])
def test_launch_shapes_and_the_device_side_count(mrt, gpu_ctx, layout):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    two_level = layout.startswith("tl")
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO_LEVEL[layout] if two_level else LAYOUTS[layout])
    dev = _dev(gpu_ctx)
    K = 3
    try:
        ds.set_mesh_masks(MODEL_MESH_MASKS[0])
        wh, wc = refs[0]
        if two_level:          # (a two-level scene intersects in object space: its bits are those of two-level scenes of the visible meshes, not the flattened reference's)
            c257, a257 = _two_level_expected(mrt, gpu_ctx, lambda visible: R.three_models(mrt, visible), TWO_LEVEL[layout], MODEL_MESH_MASKS[0], rays[:257], rm[:257])
            wh, wc = c257[:, None], a257
        for n in (1, 63, 64, 65, 257):
            d = _t(rays[:n], gpu_ctx); m = _mask_arg(rm[:n], gpu_ctx)
            for count in (None, n, n // 2, 0):
                word = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
                live = n if count is None else count
                oc = torch.full((n, 8), SENTINEL, dtype=torch.int32, device=dev); oa = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
                assert ds.intersect_closest_device(d, out=oc, count=word, mask=m) is oc and ds.intersect_any_device(d, out=oa, count=word, mask=m) is oa
                outs = [oc, oa]
                if not two_level:
                    oh = torch.full((n, K, 8), SENTINEL, dtype=torch.int32, device=dev); cnt = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
                    ds.intersect_all_device(d, K, out=oh, counts_out=cnt, count=word, mask=m)
                    outs += [oh, cnt]
                torch.cuda.synchronize()
                for o in outs:
                    assert (o[live:] == SENTINEL).all().item(), (layout, n, count, "a row at or past the count was written")
                    assert not (o[:live] == SENTINEL).any().item(), (layout, n, count, "a row below the count was not written")
                _assert_records(_records(mrt, oc[:live]), wh[:live, 0], f"{layout} n = {n} count = {count}: closest")
                assert np.array_equal(oa[:live].cpu().numpy(), (wc[:live] > 0).astype(np.int32))
                if not two_level:
                    _assert_records(_records(mrt, oh[:live]), np.ascontiguousarray(wh[:live, :K]), f"{layout} n = {n} count = {count}: all")
                    assert np.array_equal(cnt[:live].cpu().numpy(), np.minimum(wc[:live], K))
        n = 257          # closest records one word off every 16-byte boundary, as the unmasked entry takes them
        d = _t(rays[:n], gpu_ctx); m = _mask_arg(rm[:n], gpu_ctx)
        buf = torch.full((n * 8 + 2,), SENTINEL, dtype=torch.int32, device=dev)
        off = buf[1:1 + n * 8].view(n, 8)
        assert off.data_ptr() % 16 == 4 and ds.intersect_closest_device(d, out=off, mask=m) is off
        torch.cuda.synchronize()
        _assert_records(_records(mrt, off.contiguous()), wh[:n, 0], f"{layout}: closest records at 4-byte alignment")
        assert buf[0].item() == SENTINEL and buf[-1].item() == SENTINEL
        e = torch.empty((0, 8), dtype=torch.float32, device=dev)          # n == 0: MRT_OK, nothing launched
        assert tuple(ds.intersect_closest_device(e, mask=1).shape) == (0, 8) and tuple(ds.intersect_any_device(e, mask=torch.empty((0,), dtype=torch.int32, device=dev)).shape) == (0,)
    finally:
        ds.close()


# ---------------------------------------------------------------- 5. streams
def test_a_side_stream_and_the_null_stream_agree(mrt, gpu_ctx):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    dev = _dev(gpu_ctx)
    try:
        ds.set_mesh_masks(MODEL_MESH_MASKS[2])
        src = _t(rays, gpu_ctx); m = _mask_arg(rm, gpu_ctx); torch.cuda.synchronize()
        side = torch.cuda.Stream(dev)
        assert side.cuda_stream not in (0, gpu_ctx.stream)
        got = []
        for stream, handle in ((side, None), (torch.cuda.default_stream(dev), 0)):
            with torch.cuda.stream(stream):
                big = torch.randn(1024, 1024, device=dev) @ torch.randn(1024, 1024, device=dev)          # the stream is busy when the rays are made
                d = torch.where(torch.isnan(big[0, 0]), src, (src * 2.0) * 0.5).contiguous()              # exact; exists only once this stream reaches it
                c = ds.intersect_closest_device(d, stream=handle, mask=m); a = ds.intersect_any_device(d, stream=handle, mask=m)
                h, n = ds.intersect_all_device(d, 8, stream=handle, mask=m)
            stream.synchronize()
            got.append((_records(mrt, c), a.cpu().numpy(), _records(mrt, h), n.cpu().numpy()))
        for g, what in zip(got, ("side stream", "null stream")):
            _assert_records(g[0], refs[2][0][:, 0], what); assert np.array_equal(g[1], (refs[2][1] > 0).astype(np.int32))
            _assert_records(g[2], np.ascontiguousarray(refs[2][0][:, :8]), what); assert np.array_equal(g[3], np.minimum(refs[2][1], 8))
    finally:
        ds.close()


# ---------------------------------------------------------------- 6. every mask all-ones: the unmasked entries' bits
@pytest.mark.parametrize("layout", list(LAYOUTS) + list(TWO_LEVEL))
def test_all_ones_equals_the_unmasked_entries(mrt, gpu_ctx, layout):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    two_level = layout.startswith("tl")
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO_LEVEL[layout] if two_level else LAYOUTS[layout])
    try:
        d = _t(rays, gpu_ctx)
        ones = torch.full((len(rays),), -1, dtype=torch.int32, device=_dev(gpu_ctx))
        closest = ds.intersect_closest_device(d); occluded = ds.intersect_any_device(d)
        assert 0.2 < float(occluded.float().mean()) < 1.0
        for m in (R.ALL, ones, 1):          # (1: every mesh mask is still all-ones)
            assert torch.equal(ds.intersect_closest_device(d, mask=m), closest) and torch.equal(ds.intersect_any_device(d, mask=m), occluded), layout
        if not two_level:
            for K in (1, 5, 16):
                h, c = ds.intersect_all_device(d, K)
                for m in (R.ALL, ones):
                    hm, cm = ds.intersect_all_device(d, K, mask=m)
                    assert torch.equal(hm, h) and torch.equal(cm, c), (layout, K)
        torch.cuda.synchronize()
    finally:
        ds.close()


# ---------------------------------------------------------------- 7. two-level scenes
def _ring(mrt, visible=None, count=9):
    """`count` spheres of one mesh, placed so that the order along x — what a median split sorts a TLAS leaf range by — is not the id order; visible: the ids kept (all)"""
    order = [4, 0, 7, 2, 8, 5, 1, 6, 3][:count]

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="sphere", position=[1.5 * order[k] - 6.0, 0.3 * (k % 3), 0.4 * (k % 2)], rotation=[0.1 * k, 0.2, 0.0], scale=0.9 + 0.05 * k)
                           for k in (range(count) if visible is None else visible)]
    return S((8, 8))


@pytest.mark.parametrize("layout", list(TWO_LEVEL))
def test_two_level_instances_are_selected_by_their_own_masks(mrt, orc, gpu_ctx, layout):
    import torch
    sc = _ring(mrt)
    shared = mrt.flatten_scene(sc, share=True)
    assert [e[4] for e in shared] == [-1] + [0] * 8          # one mesh, eight instances of it
    rays = _rays(np.random.default_rng(9), 1024, np.array([-7.0, -1.0, -1.0]), np.array([7.0, 1.5, 1.5]))
    k = np.arange(len(rays))
    rays[k % 4 == 1, 3] = 0.5
    rays[k % 8 == 3, 7] = 6.0
    subsets = [(3,), (0,), (8,), (1, 2), (0, 4, 7), (1, 2, 3, 4, 5, 6, 7, 8), tuple(range(9)), ()]          # (3,): an instance visible, its source mesh (id 0) not
    rm = np.array([sum(1 << i for i in s) for s in subsets], np.int64)[(k * 5 + k // 64) % len(subsets)]
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO_LEVEL[layout])
    try:
        assert ds.stats.wide_layout == (1 if layout == "tl_wide" else 0)
        leaf_order = [int(i) for i in ds.read_layout("tlas_index")]
        assert sorted(leaf_order) == list(range(9)) and leaf_order != list(range(9)), "the TLAS leaf order must differ from the id order"
        ds.set_mesh_masks(R.quad_stack_masks(9))
        closest, occluded = _closest_any(mrt, ds, gpu_ctx, rays, rm)
        want, want_any = _two_level_expected(mrt, gpu_ctx, lambda visible: _ring(mrt, visible=visible), TWO_LEVEL[layout], R.quad_stack_masks(9), rays, rm, orc)
        for s_ in subsets:
            sel = rm == sum(1 << i for i in s_)
            assert sel.sum() >= 64 and ((want[sel]["type"] == 1).any() or not s_), s_
            _assert_records(closest[sel], want[sel], f"{layout} instances {s_}: closest")
            assert np.array_equal(occluded[sel], want_any[sel]), f"{layout} instances {s_}: any"
        # one mask for the whole call; and the all-hits entry refuses the scene and writes nothing
        c3, a3 = _closest_any(mrt, ds, gpu_ctx, rays, 1 << 3)
        assert set(np.unique(c3["instance_id"])) == {-1, 3} and np.array_equal(a3, (c3["type"] == 1).astype(np.int32))
        dev = _dev(gpu_ctx)
        out = torch.full((64, 4, 8), SENTINEL, dtype=torch.int32, device=dev); cnt = torch.full((64,), SENTINEL, dtype=torch.int32, device=dev)
        with pytest.raises(mrt.MRTError) as e:
            ds.intersect_all_device(_t(rays[:64], gpu_ctx), 4, out=out, counts_out=cnt, mask=1)
        assert e.value.code == 7 and "two-level" in str(e.value)          # MRT_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (out == SENTINEL).all().item() and (cnt == SENTINEL).all().item()
    finally:
        ds.close()


# ---------------------------------------------------------------- 7b. the empty scene, and the first mesh added to it
@pytest.mark.parametrize("options", [None, {"wide": 0}])
def test_empty_scene_and_the_first_mesh_added_to_it(mrt, gpu_ctx, options):
    """A committed scene without a mesh answers misses (its mask table is an allocation of one word that nobody wrote); the mesh added to it afterwards has the default mask
    on the DEVICE too — the commit uploads the table although its allocation keeps its size."""
    import torch

    class Empty(mrt.Scene):
        pass
    rays = np.repeat(_stack_rays(2), 7, 0)          # 70 rays: more than one wave
    rm = np.array([1, 0x80000000, R.ALL, 0, 5, 2, 0x40], np.int64)[np.arange(len(rays)) % 7]
    ds = mrt.DeviceScene(gpu_ctx, Empty((8, 8)), options)
    try:
        assert ds.stats.triangles == 0 and len(ds.mesh_masks()) == 0
        for m in (rm, R.ALL, 1):
            closest, occluded = _closest_any(mrt, ds, gpu_ctx, rays, m)
            assert (occluded == 0).all() and M.differing(closest, np.broadcast_to(M.miss_record(), closest.shape).copy()) == 0
            h, c = _all(mrt, ds, gpu_ctx, rays, m, 4)
            assert (c == 0).all() and M.differing(h, np.broadcast_to(M.miss_record(), h.shape).copy()) == 0
        mid, p, i, mat = _add_quad_mesh(mrt, ds, 1.0)
        ds.commit()
        assert mid == 0 and list(ds.mesh_masks()) == [R.ALL]
        entry = [(p, np.tile(np.array([0, 0, -1], f32), (4, 1)), np.eye(4, dtype=f32).reshape(16), [(i, mat)])]
        hit_rays = np.array([[1.0, -1.0, 0.0, 0.0, 0, 0, 1, np.inf], [0.5, -0.5, -3.0, 0.0, 0, 0, 1, np.inf], [9.0, 9.0, 0.0, 0.0, 0, 0, 1, np.inf]] * 24, f32)
        hm = np.array([1, 0x80000000, R.ALL, 0, 5, 2, 0x40, 3], np.int64)[np.arange(len(hit_rays)) % 8]
        want = R.MaskedReference(entry).intersect_all(hit_rays, 16, hm)
        at_quad = np.arange(len(hit_rays)) % 3 != 2
        assert (want[1][at_quad & (hm != 0)] == 1).all() and (want[1][~at_quad | (hm == 0)] == 0).all()          # every non-zero mask sees the new mesh
        _check_three(mrt, ds, gpu_ctx, hit_rays, hm, want, "the first mesh", Ks=(4,))
        ds.set_mesh_masks([2])
        closest, occluded = _closest_any(mrt, ds, gpu_ctx, hit_rays, hm)
        assert np.array_equal(occluded, ((want[1] > 0) & ((hm & 2) != 0)).astype(np.int32))
        torch.cuda.synchronize()
    finally:
        ds.close()


# ---------------------------------------------------------------- 8. persistence
def _add_quad_mesh(mrt, ds, z):
    """one more mesh through the C ABI, as DeviceScene's constructor adds them -> its mesh id"""
    p, i = M.quad(z)
    p = np.ascontiguousarray(p * f32(4.0) - f32([2.0, 2.0, 3.0 * z]), f32); nrm = np.tile(np.array([0, 0, -1], f32), (4, 1)); xf = np.eye(4, dtype=f32).reshape(16)
    mid = C.c_int32()
    from metal_raytracing_amd._ffi import check, ptr
    check(mrt.lib.mrt_scene_add_mesh(ds.handle, ptr(p), 12, ptr(nrm), 12, 4, ptr(xf), C.byref(mid)))
    mat = M._plain(mrt)
    check(mrt.lib.mrt_mesh_add_submesh(ds.handle, mid.value, ptr(np.ascontiguousarray(i, np.uint32)), 2, C.byref(mat), None))
    return mid.value, p, i, mat


def test_masks_persist_in_a_flattened_scene(mrt, gpu_ctx):
    sc, entries, rays, rm, refs = _model_case(mrt)
    rays, rm = rays[:600], rm[:600]
    ds = mrt.DeviceScene(gpu_ctx, sc, {"refit_max_cost_ratio": 1.5})
    try:
        assert list(ds.mesh_masks()) == [R.ALL] * 4
        ds.set_instance_transform(0, entries[0][2])          # the scene is not committed any more: masks set now reach the device with the commit
        ds.set_mesh_masks(MODEL_MESH_MASKS[0])
        ds.commit()
        check = lambda k, what: _check_three(mrt, ds, gpu_ctx, rays, rm, (refs[k][0][:600], refs[k][1][:600]), what, Ks=(4,))
        check(0, "masks set before the commit")
        before = (ds.stats.build_ms, ds.refits, ds.stats.triangles)
        ds.set_mesh_masks(MODEL_MESH_MASKS[2][1:], first_mesh_id=1); ds.set_mesh_masks(MODEL_MESH_MASKS[2][:1])          # after it: no commit, no build, no refit
        assert (ds.stats.build_ms, ds.refits, ds.stats.triangles) == before and list(ds.mesh_masks()) == list(MODEL_MESH_MASKS[2])
        check(2, "masks changed after the commit")
        pos, nrm = _t(np.asarray(entries[0][0], f32), gpu_ctx), _t(np.asarray(entries[0][1], f32), gpu_ctx)
        ds.update_mesh_device(0, pos, nrm); ds.refit_device()          # the same vertices: the answers stay, the refit runs
        check(2, "after update_mesh_device + refit_device")
        ds.update_mesh(0, np.asarray(entries[0][0], f32), np.asarray(entries[0][1], f32)); ds.commit()          # the same vertices again: a refitting commit
        st = ds.stats
        assert ds.refits >= 1 and max(st.wide_cost / st.wide_cost_built, st.leaf_growth) <= 1.5, (ds.refits, st.wide_cost, st.wide_cost_built, st.leaf_growth)
        check(2, "after a refitting commit")
        # the sphere's vertices shuffled: every triangle a chord of the sphere, the refitted tree far beyond refit_max_cost_ratio — that commit builds again by itself
        pos0, nrm0 = np.asarray(entries[0][0], f32), np.asarray(entries[0][1], f32)
        moved = np.ascontiguousarray(pos0[np.random.default_rng(5).permutation(len(pos0))])
        ds.update_mesh(0, moved, nrm0); ds.commit()
        st = ds.stats
        assert ds.refits == 0 and st.wide_cost == st.wide_cost_built and st.leaf_growth == 1.0, "the build forced by refit_max_cost_ratio did not run"
        assert list(ds.mesh_masks()) == list(MODEL_MESH_MASKS[2])
        shuffled = R.MaskedReference(entries, MODEL_MESH_MASKS[2]); shuffled.full.set_mesh(0, moved)
        _check_three(mrt, ds, gpu_ctx, rays, rm, shuffled.intersect_all(rays, 16, rm), "after a build forced by refit_max_cost_ratio", Ks=(4,))
        ds.update_mesh(0, pos0, nrm0); ds.commit()          # and back
        check(2, "after the vertices came back")
        ds.set_instance_transform(1, entries[1][2]); ds.commit()          # a full build
        assert ds.refits == 0 and list(ds.mesh_masks()) == list(MODEL_MESH_MASKS[2])
        check(2, "after a full re-commit")
        mid, p, i, mat = _add_quad_mesh(mrt, ds, 1.0)
        ds.commit()
        assert mid == 4 and list(ds.mesh_masks()) == list(MODEL_MESH_MASKS[2]) + [R.ALL]
        grown = R.MaskedReference(entries + [(p, np.tile(np.array([0, 0, -1], f32), (4, 1)), np.eye(4, dtype=f32).reshape(16), [(i, mat)])], list(MODEL_MESH_MASKS[2]) + [R.ALL])
        for m in (0x40, 2, rm):          # 0x40: no older mesh has the bit, the new mesh has every bit
            want = grown.intersect_all(rays, 16, m)
            if isinstance(m, int) and m == 0x40: assert set(np.unique(want[0]["instance_id"])) == {-1, 4}
            _check_three(mrt, ds, gpu_ctx, rays, m, want, "a mesh added afterwards", Ks=(4,))
    finally:
        ds.close()


@pytest.mark.parametrize("layout", list(TWO_LEVEL))
def test_masks_persist_in_a_two_level_scene(mrt, gpu_ctx, layout):
    import torch
    sc = _ring(mrt)
    rays = _rays(np.random.default_rng(10), 512, np.array([-7.0, -1.0, -1.0]), np.array([7.0, 1.5, 1.5]))
    rm = np.array([1 << 3, 0x111, 0x0F0, 0x1FF, 1], np.int64)[np.arange(len(rays)) % 5]
    xf = np.stack([np.ascontiguousarray(m.transform.reshape(16)) for m in sc.meshes]).astype(f32)
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO_LEVEL[layout])
    try:
        before = (ds.stats.build_ms, ds.refits, ds.stats.triangles)
        ds.set_mesh_masks(R.quad_stack_masks(9))
        assert (ds.stats.build_ms, ds.refits, ds.stats.triangles) == before, "setting masks built or refitted something"
        want = _closest_any(mrt, ds, gpu_ctx, rays, rm)
        assert {int(i) for i in np.unique(want[0]["instance_id"][rm == (1 << 3)])} == {-1, 3}

        def same(what):
            got = _closest_any(mrt, ds, gpu_ctx, rays, rm)
            _assert_records(got[0], want[0], f"{layout} {what}"); assert np.array_equal(got[1], want[1]), what
            assert list(ds.mesh_masks()) == list(R.quad_stack_masks(9))
        ds.set_instance_transforms_device(0, _t(xf, gpu_ctx)); ds.refit_instances_device()          # the same poses: the answers stay
        same("after set_instance_transforms_device + refit_instances_device")
        ds.rebuild_tlas_device()
        same("after rebuild_tlas_device")
        me = sc.meshes[0]
        if layout == "tl_wide":          # (the BLAS refit takes scenes whose BLASes have the 8-wide layout)
            ds.update_blas_device(0, _t(np.asarray(me.positions, f32), gpu_ctx), _t(np.asarray(me.normals, f32), gpu_ctx)); ds.refit_blas_device()
            same("after update_blas_device + refit_blas_device")
        torch.cuda.synchronize()
        ds.set_instance_transform(2, xf[2]); ds.commit()          # a TLAS-only commit
        same("after a transforms-only commit")
        ds.update_mesh(0, np.asarray(me.positions, f32), np.asarray(me.normals, f32)); ds.commit()          # a BLAS-refitting commit (a build where the scene cannot be refitted)
        same("after a vertices-only commit")
    finally:
        ds.close()


# ---------------------------------------------------------------- 9. composition: hits -> surfaces
def test_masked_hits_resolve_to_the_surfaces_of_visible_meshes(mrt, gpu_ctx):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    try:
        ds.set_mesh_masks(MODEL_MESH_MASKS[0])
        d = _t(rays, gpu_ctx)
        hits = ds.intersect_closest_device(d, mask=_mask_arg(rm, gpu_ctx))
        surf = ds.resolve_hits_device(d, hits)
        torch.cuda.synchronize()
        s = mrt.unpack_surfaces(surf); h = _records(mrt, hits)
        assert np.array_equal(s["type"], h["type"]) and np.array_equal(s["instance_id"], h["instance_id"]) and np.array_equal(s["primitive_id"], h["primitive_id"])
        hit = s["type"] == 1
        assert hit.mean() > 0.2 and np.array_equal(s["distance"][hit].view(np.uint32), h["distance"][hit].view(np.uint32))
        assert ((np.uint32(1) << s["instance_id"][hit].astype(np.uint32)) & rm[hit].astype(np.uint32) != 0).all(), "a surface of a mesh its ray may not see"
        other = mrt.DeviceScene(gpu_ctx, sc)          # the same records resolved on a scene without masks: resolving does not depend on them
        try:
            assert torch.equal(other.resolve_hits_device(d, hits).view(torch.int32), surf.view(torch.int32))          # (bit patterns: a miss row holds -1 ids, NaN as floats)
        finally:
            other.close()
    finally:
        ds.close()


# ---------------------------------------------------------------- 10. nothing is allocated
@pytest.mark.parametrize("layout", ["wide_b1", "rope_b1", "tl_wide"])
def test_nothing_is_allocated(mrt, gpu_ctx, layout):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    two_level = layout.startswith("tl")
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO_LEVEL[layout] if two_level else LAYOUTS[layout])
    dev = _dev(gpu_ctx)
    try:
        ds.set_mesh_masks(MODEL_MESH_MASKS[0])
        d = _t(rays, gpu_ctx); m = _mask_arg(rm, gpu_ctx)
        oc = torch.empty((len(rays), 8), dtype=torch.int32, device=dev); oa = torch.empty((len(rays),), dtype=torch.int32, device=dev)
        oh = torch.empty((len(rays), 16, 8), dtype=torch.int32, device=dev); cnt = torch.empty((len(rays),), dtype=torch.int32, device=dev)
        word = torch.tensor([len(rays)], dtype=torch.int32, device=dev)

        def calls(k):
            w = word if k % 2 else None; mk = 5 if k % 3 == 2 else m          # (the warm call 1 and the last call, 21, carry a mask per ray)
            ds.intersect_closest_device(d, out=oc, count=w, mask=mk); ds.intersect_any_device(d, out=oa, count=w, mask=mk)
            if not two_level: ds.intersect_all_device(d, 16, out=oh, counts_out=cnt, count=w, mask=mk)
        calls(0); calls(1)          # the warm calls
        torch.cuda.synchronize()
        first = oc.clone()
        gc.collect()          # tensors that earlier tests left in reference cycles are freed now, not by a collection in the middle of the loop
        before = (torch.cuda.memory_allocated(dev), torch.cuda.mem_get_info(dev)[0])
        for k in range(2, 22): calls(k)
        torch.cuda.synchronize()
        assert (torch.cuda.memory_allocated(dev), torch.cuda.mem_get_info(dev)[0]) == before
        assert torch.equal(oc, first)
        if not two_level: _assert_records(_records(mrt, oc), refs[0][0][:, 0], "after 20 calls")
    finally:
        ds.close()


# ---------------------------------------------------------------- 11. refusals
def test_refusals_leave_the_outputs_untouched(mrt, gpu_ctx):
    import torch
    sc, entries, rays, rm, refs = _model_case(mrt)
    dev = _dev(gpu_ctx)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    lib = mrt.lib
    P = C.c_void_p
    try:
        n, K = 64, 4
        d = _t(rays[:n], gpu_ctx); m = _mask_arg(rm[:n], gpu_ctx)
        oc = torch.full((n + 1, 8), SENTINEL, dtype=torch.int32, device=dev); oa = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev)
        oh = torch.full((n, K, 8), SENTINEL, dtype=torch.int32, device=dev); cnt = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev)
        word = torch.tensor([n], dtype=torch.int32, device=dev)
        r, mp, c, a, h, ct, w = (P(t.data_ptr()) for t in (d, m, oc, oa, oh, cnt, word))

        def refused(rc, code, text):
            assert rc == code and text in lib.mrt_last_error().decode(), (rc, lib.mrt_last_error().decode())
        closest = lambda rays=r, masks=mp, n=n, out=c, count=None, scene=ds.handle: lib.mrt_scene_intersect_closest_masked_device(scene, rays, masks, 1, n, out, None, count)
        occluded = lambda rays=r, masks=mp, n=n, out=a, count=None, scene=ds.handle: lib.mrt_scene_intersect_any_masked_device(scene, rays, masks, 1, n, out, None, count)
        every = lambda rays=r, masks=mp, n=n, k=K, out=h, counts=ct, count=None, scene=ds.handle: lib.mrt_scene_intersect_all_masked_device(scene, rays, masks, 1, n, k, out, counts, None, count)
        for fn in (closest, occluded, every):
            refused(fn(rays=None), 1, "NULL buffers"); refused(fn(out=None), 1, "NULL buffers")
            refused(fn(rays=P(d.data_ptr() + 2)), 1, "4-byte aligned"); refused(fn(masks=P(m.data_ptr() + 1)), 1, "4-byte aligned")
            refused(fn(count=P(word.data_ptr() + 2)), 1, "d_count must be 4-byte aligned")
            refused(fn(n=2 ** 31), 1, "n must be below 2^31")
            refused(fn(scene=None), 1, "scene is NULL")
        refused(closest(out=P(oc.data_ptr() + 2)), 1, "d_out must be 4-byte aligned"); refused(every(out=P(oh.data_ptr() + 8)), 1, "records must be 16-byte aligned")
        refused(occluded(out=P(oa.data_ptr() + 2)), 1, "d_occluded must be 4-byte aligned")
        for k in (0, -1, 17):
            refused(every(k=k), 1, "max_hits must be 1 .. 16")
        refused(every(counts=None), 1, "NULL buffers"); refused(every(counts=P(cnt.data_ptr() + 2)), 1, "4-byte aligned")
        refused(every(n=2 ** 27, k=16), 1, "n * max_hits must be below 2^31")
        ds.set_instance_transform(0, entries[0][2])          # not committed any more
        for fn in (closest, occluded, every):
            refused(fn(), 5, "scene not committed")          # MRT_ERR_STATE
        for bad in ("x", 1.5, -1, 2 ** 32, torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32)):
            with pytest.raises(ValueError):
                ds.intersect_closest_device(d, out=oc[:n], mask=bad)
            with pytest.raises(ValueError):
                ds.intersect_all_device(d, K, out=oh, counts_out=cnt[:n], mask=bad)
        for bad_range in ((0, 5), (4, 1), (-1, 1)):
            masks = (C.c_uint32 * 8)()
            refused(lib.mrt_scene_set_mesh_masks(ds.handle, bad_range[0], bad_range[1], masks), 1, "mesh ids out of range")
            refused(lib.mrt_scene_get_mesh_masks(ds.handle, bad_range[0], bad_range[1], masks), 1, "mesh ids out of range")
        refused(lib.mrt_scene_set_mesh_masks(ds.handle, 0, 2, None), 1, "masks is NULL")
        torch.cuda.synchronize()
        for o in (oc, oa, oh, cnt):
            assert (o == SENTINEL).all().item(), "a refused call wrote to an output"
    finally:
        ds.close()


# ---------------------------------------------------------------- 12. the C++ mirror
def test_cpp_example_prints_the_visible_quads(mrt, gpu_ctx, tmp_path):
    exe = str(tmp_path / "masks_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "masks_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    L = 7
    p = subprocess.run([exe, str(L)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    m = re.search(r"ids=((?:-?\d+ )+)distances=((?:\S+ )+)", p.stdout)
    assert m, p.stdout
    ids = [int(x) for x in m.group(1).split()]; dist = [float(x) for x in m.group(2).split()]
    assert ids == list(range(L)) + [-1] and dist == [float(k + 1) for k in range(L)] + [-1.0]
    ds = mrt.DeviceScene(gpu_ctx, M.quad_stack(mrt, L))          # the same call from Python
    try:
        ds.set_mesh_masks(R.quad_stack_masks(L))
        rays = np.repeat(np.array([[*INTERIOR, 0.0, 0.0, 0, 0, 1, np.inf]], f32), L + 1, 0)
        rm = np.array([~((1 << j) - 1) & 0xFFFFFFFF for j in range(L + 1)], np.int64)
        c, _ = _closest_any(mrt, ds, gpu_ctx, rays, rm)
        assert list(c["instance_id"]) == ids and [float(x) for x in c["distance"]] == dist
    finally:
        ds.close()
