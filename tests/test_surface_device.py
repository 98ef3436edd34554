"""Hit records resolved to surface data on device buffers, on a stream (DeviceScene.resolve_hits_device / interpolate_device / vertex_offsets).  Every
comparison is on bits, against tests/surface_reference.py (pinned to the oracle's stage dumps by tests/test_surface_device_cpu.py), against the guide buffers of a drawn
frame — a second, independent route to the same normals, distances and colours — and against a twin scene that got the same arrays through the host path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = 1, 5
TWO = {"instancing": 1}


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _t(a, ctx):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(_dev(ctx))          # (a copy: the shared cases are read-only arrays)


def _records(mrt, t):
    return t.cpu().numpy().view(mrt.INTERSECTION_DTYPE).reshape(-1)


def _options(c, extra=None):
    o = dict(TWO) if c["instancing"] else {}
    o.update(extra or {})
    return o


def _query_resolve(mrt, ds, ctx, rays):
    """query -> resolve on the current stream with no wait in between -> (hit records, surface records) as numpy"""
    r = _t(rays, ctx)
    hits = ds.intersect_closest_device(r)
    surf = ds.resolve_hits_device(r, hits)
    return _records(mrt, hits), mrt.unpack_surfaces(surf)


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = S.differing(got, want)
    if bad:
        k = int(np.flatnonzero((np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1) != np.ascontiguousarray(want).view(np.uint32).reshape(want.shape[0], -1)).any(-1))[0])
        raise AssertionError(f"{what}: {bad} of {got.shape[0]} records differ; first at {k}: {got[k]} != {want[k]}")


@pytest.fixture(scope="module")
def scenes(mrt, orc, gpu_ctx):
    """committed device scenes, made once per (case, options) and closed at the end of the module"""
    made = {}

    def get(name, extra=None):
        key = (name, tuple(sorted((extra or {}).items())))
        if key not in made:
            c = S.case(mrt, orc, name)
            made[key] = mrt.DeviceScene(gpu_ctx, c["scene"], _options(c, extra))
        return made[key]

    yield get
    for ds in made.values(): ds.close()


# ---------------------------------------------------------------- 1. against the reference, and against the guide buffers
@pytest.mark.parametrize("name", list(S.CASES))
def test_resolve_equals_the_reference_on_every_bounce(mrt, orc, gpu_ctx, scenes, name):
    c = S.case(mrt, orc, name)
    ds = scenes(name)
    for b in range(3):                       # bounce 0: coherent camera rays; bounces 1 and 2: the incoherent case
        hits, surf = _query_resolve(mrt, ds, gpu_ctx, c["rays"][b])
        assert (hits["type"] == 1).any()
        _assert_same(surf, c["ref"].resolve(c["rays"][b], hits), f"{name} bounce {b}")
        for f in ("type", "instance_id", "geometry_id", "primitive_id"): assert np.array_equal(surf[f], hits[f]), f
        assert S.same_bits(surf["distance"], hits["distance"])


@pytest.mark.parametrize("name", list(S.CASES))
def test_resolve_equals_the_guide_buffers_of_a_drawn_frame(mrt, orc, gpu_ctx, name):
    c = S.case(mrt, orc, name)
    w, h = c["w"], c["h"]
    r = mrt.Renderer((w, h), c["scene"], ctx=gpu_ctx, seed=S.SEED, scene_options=_options(c))
    try:
        r.set_option("guides", 1)
        r.draw(1, wait=True)
        g = r.guides()
        hits, surf = _query_resolve(mrt, r.device_scene, gpu_ctx, c["rays"][0])          # the dumped primary rays of that frame (same seed, same camera)
    finally:
        r.close()
    hit = (surf["type"] == 1).reshape(h, w)
    nd, al, ids = g["normal_depth"], g["albedo"], g["ids"]
    assert hit.any()
    assert S.same_bits(nd[..., :3], surf["normal"].reshape(h, w, 3)), "normals"          # (a miss is zeros on both sides)
    assert S.same_bits(nd[..., 3][hit], surf["distance"].reshape(h, w)[hit]) and not nd[..., 3][~hit].any(), "distances"
    assert S.same_bits(al[..., :3], surf["base_color"].reshape(h, w, 3)), "colours"
    assert np.array_equal(al[..., 3], hit.astype(np.float32)), "coverage"
    assert np.array_equal(ids, np.stack([surf[f].reshape(h, w) for f in ("type", "instance_id", "geometry_id", "primitive_id")], -1)), "ids"


# ---------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("name,extra", [("cornell", {"wide": 0}), ("cornell", {"rope": 1}), ("two_level", {"wide": 0})])
def test_the_layout_does_not_matter(mrt, orc, gpu_ctx, scenes, name, extra):
    c = S.case(mrt, orc, name)
    base, other = scenes(name), scenes(name, extra)
    assert other.stats.wide_layout == (0 if "wide" in extra else 1)
    for b in (0, 1):
        rays = _t(c["rays"][b], gpu_ctx)
        hits = base.intersect_closest_device(rays)
        want = mrt.unpack_surfaces(base.resolve_hits_device(rays, hits))
        _assert_same(mrt.unpack_surfaces(other.resolve_hits_device(rays, hits)), want, f"{name} {extra}: the default layout's hit records")
        own, surf = _query_resolve(mrt, other, gpu_ctx, c["rays"][b])                  # and its own walk's records
        _assert_same(surf, c["ref"].resolve(c["rays"][b], own), f"{name} {extra}: its own hit records")
        attr = _t(c["ref"].attribute("normals"), gpu_ctx)
        assert S.same_bits(other.interpolate_device(hits, attr).cpu().numpy(), base.interpolate_device(hits, attr).cpu().numpy())


# ---------------------------------------------------------------- 3. launch edges
def _half_missing(rays):
    r = np.array(rays)
    r[::2, 0:3] = (0.0, 50.0, 0.0); r[::2, 4:7] = (0.0, 1.0, 0.0)          # every second ray starts above the scene and points away from it
    return r


def test_launch_edges(mrt, orc, gpu_ctx, scenes):
    import torch
    c = S.case(mrt, orc, "cornell")
    ds = scenes("cornell")
    rays_np = _half_missing(c["rays"][1][:300])
    rays = _t(rays_np, gpu_ctx)
    hits = ds.intersect_closest_device(rays)
    full = ds.resolve_hits_device(rays, hits)
    rec, surf = _records(mrt, hits), mrt.unpack_surfaces(full)
    assert not rec["type"][::2].any() and rec["type"][1::2].any()
    _assert_same(surf, c["ref"].resolve(rays_np, rec), "every second ray misses")
    _assert_same(surf[::2], np.broadcast_to(S.miss_record(), surf[::2].shape).copy(), "the miss record")
    attr = _t(np.random.default_rng(1).standard_normal((int(ds.vertex_offsets()[-1]), 3)).astype(np.float32), gpu_ctx)
    full_i = ds.interpolate_device(hits, attr)
    assert not full_i.cpu().numpy()[::2].any()
    for n in (0, 1, 63, 64, 65, 257):
        got = ds.resolve_hits_device(rays[:n], hits[:n])                                 # out not given
        assert tuple(got.shape) == (n, 16) and torch.equal(got.view(torch.int32), full[:n].view(torch.int32)), n
        out = torch.full((n, 16), 7.0, device=_dev(gpu_ctx))
        assert ds.resolve_hits_device(rays[:n], hits[:n], out=out) is out and torch.equal(out.view(torch.int32), full[:n].view(torch.int32)), n
        gi = ds.interpolate_device(hits[:n], attr)
        assert tuple(gi.shape) == (n, 3) and torch.equal(gi.view(torch.int32), full_i[:n].view(torch.int32)), n
    # a side stream, the rays produced on it by a torch op immediately before; then the null stream
    side = torch.cuda.Stream(device=_dev(gpu_ctx))
    side.wait_stream(torch.cuda.current_stream(_dev(gpu_ctx)))
    with torch.cuda.stream(side):
        r2 = rays * 1.0
        h2 = ds.intersect_closest_device(r2, stream=side)
        s2 = ds.resolve_hits_device(r2, h2, stream=side)
        i2 = ds.interpolate_device(h2, attr, stream=side)
    side.synchronize()
    assert torch.equal(s2.view(torch.int32), full.view(torch.int32)) and torch.equal(i2.view(torch.int32), full_i.view(torch.int32))
    torch.cuda.synchronize()
    s0 = ds.resolve_hits_device(rays, hits, stream=0); i0 = ds.interpolate_device(hits, attr, stream=0)
    torch.cuda.synchronize()
    assert torch.equal(s0.view(torch.int32), full.view(torch.int32)) and torch.equal(i0.view(torch.int32), full_i.view(torch.int32))


def test_refusals_on_a_live_scene(mrt, orc, gpu_ctx, scenes):
    import torch
    ds = scenes("cornell")
    lib = mrt.lib
    rays = torch.zeros((4, 8), device=_dev(gpu_ctx)); hits = torch.zeros((4, 8), dtype=torch.int32, device=_dev(gpu_ctx)); out = torch.zeros((4, 16), device=_dev(gpu_ctx))
    attr = torch.zeros((int(ds.vertex_offsets()[-1]), 4), device=_dev(gpu_ctx))
    P = C.c_void_p
    assert lib.mrt_scene_resolve_hits_device(ds.handle, P(rays.data_ptr() + 4), P(hits.data_ptr()), 4, P(out.data_ptr()), None) == INVALID
    assert lib.mrt_scene_resolve_hits_device(ds.handle, None, P(hits.data_ptr()), 4, P(out.data_ptr()), None) == INVALID
    assert lib.mrt_scene_resolve_hits_device(ds.handle, None, None, 0, None, None) == 0
    assert lib.mrt_scene_resolve_hits_device(ds.handle, P(rays.data_ptr()), P(hits.data_ptr()), 2 ** 31, P(out.data_ptr()), None) == INVALID
    for ch, st in ((0, 16), (65, 260), (4, 12), (3, 14)):
        assert lib.mrt_scene_interpolate_device(ds.handle, P(hits.data_ptr()), 4, P(attr.data_ptr()), st, ch, P(out.data_ptr()), 64, None) == INVALID, (ch, st)
    assert lib.mrt_scene_interpolate_device(ds.handle, P(hits.data_ptr()), 4, P(attr.data_ptr() + 1), 16, 4, P(out.data_ptr()), 64, None) == INVALID
    assert lib.mrt_scene_interpolate_device(ds.handle, None, 0, None, 16, 4, None, 64, None) == 0
    with pytest.raises(mrt.MRTError) as e: ds.interpolate_device(hits, attr[:-1])          # a row per vertex of the scene, or the device would read past the end
    assert e.value.code == INVALID
    with pytest.raises(ValueError): ds.resolve_hits_device(rays[:3], hits)
    with pytest.raises(ValueError): ds.interpolate_device(hits.to(torch.float32), attr)
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    try:
        assert lib.mrt_scene_resolve_hits_device(h, P(rays.data_ptr()), P(hits.data_ptr()), 4, P(out.data_ptr()), None) == STATE          # not committed
        assert lib.mrt_scene_interpolate_device(h, P(hits.data_ptr()), 4, P(attr.data_ptr()), 16, 4, P(out.data_ptr()), 64, None) == STATE
        o = (C.c_uint64 * 1)()
        assert lib.mrt_scene_vertex_offsets(h, o, 1) == 0 and o[0] == 0 and lib.mrt_scene_vertex_offsets(h, o, 2) == INVALID
    finally:
        lib.mrt_scene_destroy(h)


# ---------------------------------------------------------------- 4. hostile ids
@pytest.mark.parametrize("name", ["cornell", "two_level", "no_dragon"])
def test_hostile_ids_give_the_miss_record(mrt, orc, gpu_ctx, scenes, name):
    """The bounds check reads the table sizes: ids one before the start, one past the end and 2^31 - 1 in each field, between untouched valid neighbours."""
    c = S.case(mrt, orc, name)
    ds, ref = scenes(name), c["ref"]
    hits0, _ = _query_resolve(mrt, ds, gpu_ctx, c["rays"][0])
    k = int(np.flatnonzero(hits0["type"] == 1)[hits0["type"].sum() // 2])
    good = hits0[k]
    i, g = int(good["instance_id"]), int(good["geometry_id"])
    ends = {"instance_id": [len(ref.entries)], "geometry_id": [len(ref.entries[i]["indices"]), ref.max_sub], "primitive_id": [ref.entries[i]["indices"][g].shape[0]]}
    rec, bad = [], []
    for f, past in ends.items():
        for v in [-1, 2 ** 31 - 1, -2 ** 31] + past:
            h = good.copy(); h[f] = v
            bad.append(len(rec) + 1); rec += [good, h]
    rec.append(good)
    rec = np.array(rec, dtype=mrt.INTERSECTION_DTYPE)
    other = np.array([good]); other["type"] = 2                                            # a record that is neither a miss nor a triangle
    rec = np.concatenate([rec, other, np.array([good])])
    bad.append(len(rec) - 2)
    rays = np.repeat(c["rays"][0][k:k + 1], len(rec), 0)
    ht = _t(rec.view(np.int32).reshape(-1, 8), gpu_ctx)
    surf = mrt.unpack_surfaces(ds.resolve_hits_device(_t(rays, gpu_ctx), ht))
    attr = ref.attribute("normals")
    ip = ds.interpolate_device(ht, _t(attr, gpu_ctx)).cpu().numpy()
    want = ref.resolve(rays[:1], rec[:1])[0]
    assert want["type"] == 1
    for j in range(len(rec)):
        if j in bad:
            assert S.differing(surf[j:j + 1], np.array([S.miss_record()])) == 0, (j, rec[j], surf[j])
            assert not ip[j].view(np.uint32).any(), (j, rec[j])
        else:
            assert S.differing(surf[j:j + 1], np.array([want])) == 0, (j, surf[j])
            assert S.same_bits(ip[j], ref.interpolate(rec[:1], attr)[0]) and ip[j].any()


# ---------------------------------------------------------------- 5. it follows the device's state
def _deformed(pos, nrm, amount):
    p = np.array(pos, np.float32); n = np.array(nrm, np.float32)
    p[:, 1] += np.float32(amount) * np.sin(p[:, 0] * np.float32(3.0) + p[:, 2]).astype(np.float32)
    n = n + np.array([0.3, 0.0, 0.2], np.float32) * np.float32(amount * 10)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n.astype(np.float32))


def test_resolve_follows_update_mesh_device(mrt, orc, gpu_ctx):
    c = S.case(mrt, orc, "cornell")
    mesh = 0                                               # the plane the five walls are instances of
    pos, nrm = _deformed(c["entries"][mesh][0], c["entries"][mesh][1], 0.05)
    a = mrt.DeviceScene(gpu_ctx, c["scene"]); b = mrt.DeviceScene(gpu_ctx, c["scene"])
    try:
        rays = c["rays"][0]
        _, before = _query_resolve(mrt, a, gpu_ctx, rays)                              # (the table exists before the update: it must not go stale)
        a.update_mesh_device(mesh, _t(pos, gpu_ctx), _t(nrm, gpu_ctx)); a.refit_device()
        hits_a, surf_a = _query_resolve(mrt, a, gpu_ctx, rays)                         # stream order, no host wait since the update
        b.update_mesh(mesh, pos, nrm); b.commit()
        hits_b, surf_b = _query_resolve(mrt, b, gpu_ctx, rays)
        _assert_same(hits_a, hits_b, "hit records"); _assert_same(surf_a, surf_b, "surfaces")
        assert S.differing(surf_a, before) > 100
        ref = S.SurfaceReference(c["entries"]); ref.set_mesh(mesh, pos, nrm)
        _assert_same(surf_a, ref.resolve(rays, hits_a), "the reference with the new normals")
        attr = _t(ref.attribute("normals"), gpu_ctx)
        assert S.same_bits(a.interpolate_device(_t(hits_a.view(np.int32).reshape(-1, 8), gpu_ctx), attr).cpu().numpy(), ref.interpolate(hits_a, ref.attribute("normals")))
    finally:
        a.close(); b.close()


def _rotated(xf16, angle, shift):
    m = np.asarray(xf16, np.float32).reshape(4, 4).T.astype(np.float64)
    r = np.eye(4); r[0, 0] = r[2, 2] = np.cos(angle); r[0, 2] = np.sin(angle); r[2, 0] = -np.sin(angle); r[0, 3] = shift
    return np.ascontiguousarray((r @ m).T.reshape(16).astype(np.float32))


def test_resolve_follows_set_instance_transforms_device(mrt, orc, gpu_ctx):
    c = S.case(mrt, orc, "two_level")
    xfs = np.stack([_rotated(e[2], 0.4 + 0.1 * i, 0.05 * i) for i, e in enumerate(c["entries"])])
    a = mrt.DeviceScene(gpu_ctx, c["scene"], TWO); b = mrt.DeviceScene(gpu_ctx, c["scene"], TWO)
    try:
        rays = c["rays"][0]
        _, before = _query_resolve(mrt, a, gpu_ctx, rays)
        a.set_instance_transforms_device(0, _t(xfs, gpu_ctx)); a.refit_instances_device()
        hits_a, surf_a = _query_resolve(mrt, a, gpu_ctx, rays)
        for i in range(len(xfs)): b.set_instance_transform(i, xfs[i])
        b.commit()
        hits_b, surf_b = _query_resolve(mrt, b, gpu_ctx, rays)
        _assert_same(hits_a, hits_b, "hit records"); _assert_same(surf_a, surf_b, "surfaces")
        assert S.differing(surf_a, before) > 100
        ref = S.SurfaceReference(c["entries"])
        for i in range(len(xfs)): ref.set_transform(i, xfs[i])
        want = ref.resolve(rays, hits_a)                                               # normals through the rotated columns, positions from the rays
        _assert_same(surf_a, want, "the reference with the rotated columns")
    finally:
        a.close(); b.close()


def test_resolve_follows_update_blas_device(mrt, orc, gpu_ctx):
    c = S.case(mrt, orc, "two_level")
    mesh = 1                                               # the sphere three instances share
    pos, nrm = _deformed(c["entries"][mesh][0], c["entries"][mesh][1], 0.03)
    a = mrt.DeviceScene(gpu_ctx, c["scene"], TWO); b = mrt.DeviceScene(gpu_ctx, c["scene"], TWO)
    try:
        rays = c["rays"][0]
        _, before = _query_resolve(mrt, a, gpu_ctx, rays)
        a.update_blas_device(mesh, _t(pos, gpu_ctx), _t(nrm, gpu_ctx)); a.refit_blas_device()
        hits_a, surf_a = _query_resolve(mrt, a, gpu_ctx, rays)
        b.update_mesh(mesh, pos, nrm); b.commit()
        hits_b, surf_b = _query_resolve(mrt, b, gpu_ctx, rays)
        _assert_same(hits_a, hits_b, "hit records"); _assert_same(surf_a, surf_b, "surfaces")
        assert S.differing(surf_a, before) > 50
        ref = S.SurfaceReference(c["entries"]); ref.set_mesh(mesh, pos, nrm)
        _assert_same(surf_a, ref.resolve(rays, hits_a), "the reference with the new normals")
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------- 6. interpolate
@pytest.mark.parametrize("name,extra", [("cornell", None), ("two_level", None), ("no_dragon", None), ("two_level", {"instancing": 0})])
def test_interpolate_gives_the_object_space_normal(mrt, orc, gpu_ctx, scenes, name, extra):
    """The scene's own normals as a 3-channel attribute in the caller's numbering; the last case is the instanced scene FLATTENED: every flattened instance has a vertex
    range of its own inside the library and still reads its source's rows."""
    c = S.case(mrt, orc, name)
    ds, ref = scenes(name, extra), c["ref"]
    assert np.array_equal(ds.vertex_offsets(), ref.offsets)
    attr = ref.attribute("normals")
    assert attr.shape[0] == int(ref.offsets[-1])
    for b in (0, 2):
        rays = _t(c["rays"][b], gpu_ctx)
        hits = ds.intersect_closest_device(rays)
        got = ds.interpolate_device(hits, _t(attr, gpu_ctx)).cpu().numpy()
        rec = _records(mrt, hits)
        assert S.same_bits(got, ref.interpolate(rec, attr)), f"{name} bounce {b}: {(got.view(np.uint32) != ref.interpolate(rec, attr).view(np.uint32)).any(-1).sum()} rows differ"
        _assert_same(mrt.unpack_surfaces(ds.resolve_hits_device(rays, hits)), ref.resolve(c["rays"][b], rec), f"{name} {extra} bounce {b}")


def test_interpolated_positions_are_near_the_resolved_ones(mrt, orc, gpu_ctx):
    """A sanity check and the only inexact comparison: the bound, 1e-4 x the scene's extent, is no claim about the kernel.  One mesh under the identity (CornellScene's
    transforms are not identities)."""
    class One(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="sphere", position=[0, 0, 0], scale=1)]
    sc = One((32, 32))
    assert np.array_equal(sc.meshes[0].transform, np.eye(4, dtype=np.float32))
    rng = np.random.default_rng(4)
    o = rng.normal(size=(500, 3)); o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.normal(size=(500, 3)) * 0.3 - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((500, 8), np.float32); rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = np.inf
    ds = mrt.DeviceScene(gpu_ctx, sc)
    try:
        r = _t(rays, gpu_ctx)
        hits = ds.intersect_closest_device(r)
        surf = mrt.unpack_surfaces(ds.resolve_hits_device(r, hits))
        pos = ds.interpolate_device(hits, _t(sc.meshes[0].positions, gpu_ctx)).cpu().numpy()
        hit = surf["type"] == 1
        extent = float(np.ptp(sc.meshes[0].positions, axis=0).max())
        assert hit.sum() > 100 and np.abs(pos[hit] - surf["position"][hit]).max() <= 1e-4 * extent
    finally:
        ds.close()


@pytest.mark.parametrize("channels,pad_in,pad_out", [(1, 1, 2), (3, 1, 1), (3, 0, 0), (4, 1, 3), (4, 4, 4), (5, 3, 1), (16, 0, 0), (16, 1, 2), (16, 4, 8), (64, 4, 4), (64, 3, 1)])
def test_interpolate_channels_and_strides(mrt, orc, gpu_ctx, scenes, channels, pad_in, pad_out):
    """Random data at 1 .. 64 channels, rows padded on input and output (a multiple of 16 bytes takes the 16-byte form, anything else the 4-byte form); the padding of
    `out` is left as it was."""
    import torch
    c = S.case(mrt, orc, "two_level")
    ds, ref = scenes("two_level"), c["ref"]
    V = int(ref.offsets[-1])
    data = np.random.default_rng(channels * 100 + pad_in).standard_normal((V, channels + pad_in)).astype(np.float32)
    rays = _half_missing(c["rays"][1][:777])
    hits = ds.intersect_closest_device(_t(rays, gpu_ctx))
    wide = _t(data, gpu_ctx)
    out_wide = torch.full((hits.shape[0], channels + pad_out), -7.0, device=_dev(gpu_ctx))
    got = ds.interpolate_device(hits, wide[:, :channels], out=out_wide[:, :channels])
    assert got.data_ptr() == out_wide.data_ptr()
    res = out_wide.cpu().numpy()
    want = ref.interpolate(_records(mrt, hits), data[:, :channels])
    assert S.same_bits(np.ascontiguousarray(res[:, :channels]), want) and want.any()
    assert (res[:, channels:] == -7.0).all()


def test_an_instance_and_its_source_give_equal_rows(mrt, orc, gpu_ctx, scenes):
    c = S.case(mrt, orc, "two_level")
    ref = c["ref"]
    src, inst = 1, 5                                      # the sphere and its last instance
    assert ref.entries[inst]["source"] == src
    rng = np.random.default_rng(9)
    n = 200
    rec = np.zeros(2 * n, mrt.INTERSECTION_DTYPE)
    rec["type"] = 1; rec["distance"] = 1.0; rec["geometry_id"] = 0
    rec["primitive_id"][:n] = rec["primitive_id"][n:] = rng.integers(0, ref.entries[src]["indices"][0].shape[0], n)
    u = rng.uniform(0, 1, n).astype(np.float32); v = (rng.uniform(0, 1, n) * (1 - u)).astype(np.float32)
    rec["u"][:n] = rec["u"][n:] = u; rec["v"][:n] = rec["v"][n:] = v
    rec["instance_id"][:n] = src; rec["instance_id"][n:] = inst
    attr = np.random.default_rng(10).standard_normal((int(ref.offsets[-1]), 5)).astype(np.float32)
    for extra in (None, {"instancing": 0}):
        got = scenes("two_level", extra).interpolate_device(_t(rec.view(np.int32).reshape(-1, 8), gpu_ctx), _t(attr, gpu_ctx)).cpu().numpy()
        assert S.same_bits(got[:n], got[n:]) and S.same_bits(got, ref.interpolate(rec, attr)) and got.any()


# ---------------------------------------------------------------- 7. nothing is allocated after the first call
@pytest.mark.parametrize("name", ["cornell", "two_level"])
def test_nothing_is_allocated_after_the_first_call(mrt, orc, gpu_ctx, name):
    import torch
    c = S.case(mrt, orc, name)
    ds = mrt.DeviceScene(gpu_ctx, c["scene"], _options(c))
    try:
        rays = _t(c["rays"][1], gpu_ctx)
        hits = ds.intersect_closest_device(rays)
        attr = _t(c["ref"].attribute("normals"), gpu_ctx)
        surf = torch.empty((rays.shape[0], 16), device=_dev(gpu_ctx)); ip = torch.empty((rays.shape[0], 3), device=_dev(gpu_ctx))
        ds.resolve_hits_device(rays, hits, out=surf); ds.interpolate_device(hits, attr, out=ip)          # the warm call: the table exists
        torch.cuda.synchronize()
        first = surf.clone(); first_i = ip.clone()
        torch.cuda.synchronize()
        free = [torch.cuda.mem_get_info(_dev(gpu_ctx))[0]]
        for _ in range(20):
            ds.resolve_hits_device(rays, hits, out=surf); ds.interpolate_device(hits, attr, out=ip)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(_dev(gpu_ctx))[0])
        assert free[0] == free[1], free
        ds.commit()                                                                       # the table goes with the commit; the next call makes it again
        surf.zero_(); ip.zero_()
        ds.resolve_hits_device(rays, hits, out=surf); ds.interpolate_device(hits, attr, out=ip)
        torch.cuda.synchronize()
        assert torch.equal(surf.view(torch.int32), first.view(torch.int32)) and torch.equal(ip.view(torch.int32), first_i.view(torch.int32))
        _assert_same(mrt.unpack_surfaces(surf), c["ref"].resolve(c["rays"][1], _records(mrt, hits)), "after the commit")
    finally:
        ds.close()


# ---------------------------------------------------------------- 8. C++
def test_cpp_host_resolves_hits(mrt, orc, gpu_ctx, scenes, tmp_path):
    exe = str(tmp_path / "surface_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                           os.path.join(ROOT, "examples", "surface_host.cpp"), "-L" + os.path.join(ROOT, "metal-raytracing_amd"), "-lmrt_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "metal-raytracing_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    side = 24
    p = subprocess.run([exe, str(side)], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr
    m = re.search(r"rays=(\d+) hits=(\d+) ids=(-?\d+) vertices=(\d+) checksum=(\S+)", p.stdout)
    assert m, p.stdout
    f = np.float32
    x = ((2 * np.arange(side) + 1).astype(f) / f(side) - f(1)) * f(1.25)
    rays = np.zeros((side * side, 8), f)
    rays[:, 1] = 1.0; rays[:, 2] = 3.0; rays[:, 4] = np.tile(x, side); rays[:, 5] = np.repeat(x, side); rays[:, 6] = -2.0; rays[:, 7] = np.inf
    _, surf = _query_resolve(mrt, scenes("cornell"), gpu_ctx, rays)
    checksum = 0.0
    flat = np.concatenate([surf["position"], surf["distance"][:, None], surf["normal"], surf["base_color"]], axis=1).astype(np.float64)
    for v in flat.ravel(): checksum += float(v)                                            # the C++ side's order, in double
    ids = int(sum(int(surf[k].astype(np.int64).sum()) for k in ("type", "resource_slot", "instance_id", "geometry_id", "primitive_id")))
    c = S.case(mrt, orc, "cornell")
    assert int(m.group(1)) == side * side and int(m.group(2)) == int((surf["type"] == 1).sum()) > 0 and int(m.group(3)) == ids
    assert int(m.group(4)) == sum(mesh.positions.shape[0] for mesh in c["scene"].meshes)                # the C++ mirror adds every model as a mesh of its own
    assert float(m.group(5)) == checksum                                                                # %.17g prints the double exactly
