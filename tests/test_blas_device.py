"""Meshes that deform INSIDE a two-level scene, from device buffers and on the caller's stream (DeviceScene.update_blas_device / refit_blas_device): scene A takes new
object-space vertices of a source mesh from a torch tensor, refits that mesh's BLAS in place, hands the BLAS's new root box to its instances and refits both TLAS forms with
the topology kept; scene B gets the same vertices through update_mesh + commit (refit_two_level: the same BLAS kernels, then a TLAS built again on the host).  Everything
compared is bit-exact: the instance rows and boxes, the BLAS part of the 8-wide nodes, all packets, every field of every query record, the image, the statistics — and the
records equal the two-level oracle's brute force on the deformed meshes.  The scenes are test_instances_device's: instances of a 12-triangle box (its BLAS has real 8-wide
nodes and several rope nodes) and of a 2-triangle quad (its packets are inlined in the instance's TLAS slot: the BLAS root is all there is)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_audit as A
from test_instances_device import (INVALID, SIZE, STATE, UNSUPPORTED, _bits, _case, _dev, _device_records, _host_move, _poses, _same_records, _same_snapshot, _snapshot, _start, _t)

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 9, 65)          # 1: no quad; 3: a BLAS shared by two instances; 9: two 8-wide TLAS levels, the tree-less TLAS pass; 65: the TLAS walk
BOX, QUAD = 0, 1
TWO = {"instancing": 1}
UPDATE, REFIT = "mrt_scene_update_blas_device", "mrt_scene_refit_blas_device"


@functools.lru_cache(maxsize=None)
def _deformed(mrt, k, s):
    """mesh k (0 box, 1 quad) as step s deforms it: every vertex scaled about the origin and jittered; normals perturbed and renormalised"""
    pos = np.asarray(_case(mrt, 2)[1][k][0], np.float32); nrm = np.asarray(_case(mrt, 2)[1][k][1], np.float32)
    rng = np.random.default_rng(5000 + 10 * s + k)
    p = (pos * rng.uniform(0.6, 1.6, (len(pos), 1)) + rng.normal(size=pos.shape) * 0.1).astype(np.float32)
    q = nrm + rng.normal(size=nrm.shape) * 0.2
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    p.setflags(write=False); q.setflags(write=False)
    return p, q


@functools.lru_cache(maxsize=None)
def _oracle(mrt, orc, n, pose_key, dkey):
    """the two-level oracle's brute force on the scene with the poses pose_key = ((step, first), ...) and the meshes dkey = (box step or None, quad step or None)"""
    sc, meshes, rays = _case(mrt, n)
    xf = _start(n)
    for step, first in pose_key: xf[first:] = _poses(n, step)[first:]
    geo = {k: _deformed(mrt, k, s) for k, s in enumerate(dkey) if s is not None}
    moved = [(*geo.get(k % 2, (p, nr)), np.ascontiguousarray(xf[k]), subs, src) for k, (p, nr, _, subs, src) in enumerate(meshes)]
    out = orc.OracleScene(moved, sc.lights, instancing=True).intersect_closest(np.array(rays), brute=True)
    out.setflags(write=False)
    return out


def _links(ds):
    wn = ds.read_layout("wnodes")
    return np.column_stack([wn[:, 4], wn[:, 5], wn[:, 3] >> 24, wn[:, 6], wn[:, 7]])


def _layout(ds):
    return {p: ds.read_layout(p) for p in ("instances", "inst_box", "wnodes", "wpackets", "rope_nodes", "rope_packets")}          # (the rope arrays hold the BLASes only: compared in full)


def _same_layout(a, b, n, what, tlas_too=False):
    """what a device refit and a refitting commit must both leave: the TLAS slots in front of the BLASes differ only where B's TLAS was built again"""
    la, lb = _layout(a), _layout(b)
    for part in la:
        first = 0 if tlas_too or part != "wnodes" else max(n, 1)
        assert la[part].shape == lb[part].shape and np.array_equal(_bits(la[part])[first:], _bits(lb[part])[first:]), what + part


def _stats(ds):
    s = ds.stats
    return (s.refits, s.wide_cost, s.wide_cost_built, s.sah_cost, s.leaf_growth)


def _rays_of(mrt, gpu_ctx, n):
    r = np.array(_case(mrt, n)[2])
    finite = r.copy(); finite[:, 7] = 3.0
    return r, finite, _t(r, gpu_ctx), _t(finite, gpu_ctx)


def _check(mrt, orc, gpu_ctx, a, b, n, pose_key, dkey, rr, what, layout=True):
    """scene A (deformed on the device) against scene B (deformed on the host) and the oracle; returns the oracle's records"""
    import torch
    r, finite, d_rays, d_finite = rr
    torch.cuda.synchronize()
    if layout: _same_layout(a, b, n, what)
    A.audit(A.layout_of(a)).check()
    ref = _oracle(mrt, orc, n, pose_key, dkey)
    share = float((ref["distance"] >= 0).mean())
    print(f"{what}hit share {share:.3f}")
    assert share >= 0.08, what + "too few rays hit for the comparison to mean much"
    hb = b.intersect_closest(r)
    _same_records(hb, ref, what + "host path against the oracle: ")
    _same_records(a.intersect_closest(r), ref, what + "rope walk ")
    _same_records(_device_records(a.intersect_closest_device(d_rays)), ref, what + "device entry ")
    _same_records(a.intersect_stream(r), ref, what + "stream walk ")
    occ = b.intersect_any(finite)
    assert np.array_equal(a.intersect_any(finite), occ), what + "any-hit"
    assert np.array_equal(a.intersect_any_device(d_finite).cpu().numpy(), occ), what + "any-hit device entry"
    return ref


def _changed(x, y, what):
    k = int((_bits(x["distance"]) != _bits(y["distance"])).sum())
    print(f"{what}{k} distances changed")
    assert k >= 200, what + "the step must change the answers"


def _td(a, gpu_ctx):
    return _t(np.array(a), gpu_ctx)          # (a copy: the cached arrays are read-only)


def _dev_update(mrt, ds, gpu_ctx, k, s):
    """step s of mesh k through the device entry; returns the tensors, which must outlive the stream's use of them"""
    tp, tq = (_td(x, gpu_ctx) for x in _deformed(mrt, k, s))
    ds.update_blas_device(k, tp, tq)
    return tp, tq


def _host_update(mrt, ds, k, s, commit=True):
    ds.update_mesh(k, *_deformed(mrt, k, s))
    if commit: ds.commit()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", ["wide", "wide+rope"])
def test_parity_with_the_host_path(mrt, orc, gpu_ctx, layout, n):
    import torch
    sc, meshes, rays = _case(mrt, n)
    rr = _rays_of(mrt, gpu_ctx, n)
    opts = dict({"wide": {}, "wide+rope": {"rope": 1}}[layout], instancing=1)
    a, b = mrt.DeviceScene(gpu_ctx, sc, opts), mrt.DeviceScene(gpu_ctx, sc, opts)
    assert a.stats.wide_layout == 1 and a.stats.instances == n
    links, nodes, depth = _links(a), a.stats.bvh_nodes, a.stats.max_depth
    start = _oracle(mrt, orc, n, (), (None, None))
    # step 0: the box alone, packed rows
    keep = _dev_update(mrt, a, gpu_ctx, BOX, 0); a.refit_blas_device()
    _host_update(mrt, b, BOX, 0)
    h0 = _check(mrt, orc, gpu_ctx, a, b, n, (), (0, None), rr, f"{layout} n={n} step 0: ")
    _changed(h0, start, f"{layout} n={n} step 0: ")
    # step 1: both meshes before one refit; the quad's rows 32 bytes apart, the padding never read
    keep1 = _dev_update(mrt, a, gpu_ctx, BOX, 1)
    if n >= 2:
        p, q = _deformed(mrt, QUAD, 1)
        wide = torch.full((len(p), 8), float("nan"), device=_dev(gpu_ctx))
        wide[:, 0:3] = _td(p, gpu_ctx); wide[:, 4:7] = _td(q, gpu_ctx)
        assert wide[:, 0:3].stride(0) * 4 == 32
        a.update_blas_device(QUAD, wide[:, 0:3], wide[:, 4:7])
    a.refit_blas_device()
    _host_update(mrt, b, BOX, 1, commit=n < 2)
    if n >= 2: _host_update(mrt, b, QUAD, 1)
    dkey = (1, 1 if n >= 2 else None)
    h1 = _check(mrt, orc, gpu_ctx, a, b, n, (), dkey, rr, f"{layout} n={n} step 1: ")
    _changed(h1, h0, f"{layout} n={n} step 1: ")
    sa, sb = _stats(a), _stats(b)
    assert sa == sb and sa[0] == 2 and not any(np.isnan(x) for x in sa), (sa, sb)
    assert a.stats.build_ms > 0
    assert np.array_equal(_links(a), links), "a refit moves boxes, never the links between the nodes, to the packets and to the instances"
    assert (a.stats.bvh_nodes, a.stats.max_depth) == (nodes, depth)
    assert a.device_updates_rejected == 0
    del keep, keep1
    a.close(); b.close()


def test_refused_without_the_wide_layout_and_on_flattened_scenes(mrt, orc, gpu_ctx):
    n = 3
    sc, meshes, rays = _case(mrt, n)
    lib = mrt.lib
    p, q = _deformed(mrt, BOX, 0)
    d_p, d_q = _td(p, gpu_ctx), _td(q, gpu_ctx)

    def last():
        return lib.mrt_last_error().decode()

    def raw(ds, fn=lib.mrt_scene_update_blas_device):
        return fn(ds.handle, BOX, C.c_void_p(d_p.data_ptr()), 12, C.c_void_p(d_q.data_ptr()), 12, len(p), None)

    for opts in ({"instancing": 1, "wide": 0}, {}, {"instancing": 1, "refit": 0}):
        ds = mrt.DeviceScene(gpu_ctx, sc, opts)
        before = ds.intersect_closest(np.array(rays[:512]))
        assert raw(ds) == UNSUPPORTED and UPDATE in last(), opts
        assert lib.mrt_scene_refit_blas_device(ds.handle, None) == UNSUPPORTED and REFIT in last(), opts
        _same_records(ds.intersect_closest(np.array(rays[:512])), before)
        assert ds.refits == 0 and ds.device_updates_rejected == 0
        ds.close()
    two = mrt.DeviceScene(gpu_ctx, sc, TWO)          # the flat-scene entries go on refusing two-level scenes
    assert raw(two, lib.mrt_scene_update_mesh_device) == UNSUPPORTED and "mrt_scene_update_mesh_device" in last()
    assert lib.mrt_scene_refit_device(two.handle, None) == UNSUPPORTED and "mrt_scene_refit_device" in last()
    two.close()


@pytest.mark.parametrize("n,guides", [(9, 1), (65, 0)])
def test_a_renderer_made_before_the_deformation_draws_it(mrt, orc, gpu_ctx, n, guides):
    import torch
    sc, meshes, rays = _case(mrt, n)
    ra = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options=TWO); rb = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options=TWO)
    if guides:
        for rr in (ra, rb): rr.set_option("guides", 1)
    ra.draw(2, wait=True)
    still = ra.accumulation().copy()
    keep = [_dev_update(mrt, ra.device_scene, gpu_ctx, BOX, 0), _dev_update(mrt, ra.device_scene, gpu_ctx, QUAD, 0)]
    ra.device_scene.refit_blas_device()
    torch.cuda.synchronize()          # (the renderer draws on the context's streams)
    _host_update(mrt, rb.device_scene, BOX, 0, commit=False); _host_update(mrt, rb.device_scene, QUAD, 0)
    for rr in (ra, rb):
        rr.frameIndex = 0; rr.reset_stats(); rr.draw(2, wait=True)
    assert np.array_equal(_bits(ra.accumulation()), _bits(rb.accumulation())), "the two paths must render the same image"
    assert (ra.stats.closest_rays, ra.stats.shadow_rays) == (rb.stats.closest_rays, rb.stats.shadow_rays)
    assert not np.array_equal(_bits(ra.accumulation()), _bits(still))
    del keep
    ra.close(); rb.close()


@pytest.mark.parametrize("n", [3, 9])
def test_poses_and_vertices_together(mrt, orc, gpu_ctx, n):
    import torch
    sc, meshes, rays = _case(mrt, n)
    rr = _rays_of(mrt, gpu_ctx, n)
    x = _poses(n, 0)
    d_x = _t(x, gpu_ctx)
    # poses first, then vertices, ONE refit: refit_blas_device recomputes the world boxes under the poses the device holds and refits the TLAS
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    a.set_instance_transforms_device(0, d_x)
    keep = [_dev_update(mrt, a, gpu_ctx, BOX, 0), _dev_update(mrt, a, gpu_ctx, QUAD, 0)]
    a.refit_blas_device()
    for k in range(n): b.set_instance_transform(k, x[k])
    _host_update(mrt, b, BOX, 0, commit=False); _host_update(mrt, b, QUAD, 0)          # vertices and transforms: a full build, so only the answers compare
    h = _check(mrt, orc, gpu_ctx, a, b, n, ((0, 0),), (0, 0), rr, f"n={n} poses then vertices: ", layout=False)
    _changed(h, _oracle(mrt, orc, n, (), (None, None)), f"n={n} poses then vertices: ")
    a.close(); b.close()
    # the other order: the set call must see the object box the BLAS refit left
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    keep = [_dev_update(mrt, a, gpu_ctx, BOX, 0), _dev_update(mrt, a, gpu_ctx, QUAD, 0)]
    a.refit_blas_device()
    a.set_instance_transforms_device(0, d_x); a.refit_instances_device()
    _host_update(mrt, b, BOX, 0, commit=False); _host_update(mrt, b, QUAD, 0)
    _host_move(b, 0, x)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), "instance boxes"
    _check(mrt, orc, gpu_ctx, a, b, n, ((0, 0),), (0, 0), rr, f"n={n} vertices then poses: ", layout=False)
    del keep
    a.close(); b.close()


def test_stream_order(mrt, orc, gpu_ctx):
    """a torch expression that makes the vertices, the update, the refit and a query on ONE stream, nothing of the host in between, one synchronise at the end — on a
    side stream and on the null stream"""
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    dev = _dev(gpu_ctx)
    d_rays = _t(r, gpu_ctx)
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream not in (0, gpu_ctx.stream)
    for step, (stream, handle) in enumerate(((side, None), (torch.cuda.default_stream(dev), 0))):
        p, q = _deformed(mrt, BOX, step)
        a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
        _host_update(mrt, b, BOX, step)
        src, d_q = _td(p, gpu_ctx), _td(q, gpu_ctx)
        d_p = torch.zeros_like(src)
        a.refit_blas_device()          # (the first call after a commit makes the workspaces and may block: not part of what is ordered below)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            big = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)          # the stream is busy when the vertices are made
            z = torch.nan_to_num(big[0, 0] * 0.0)
            d_p.copy_(src * 2.0 * 0.5 + z)          # exact; the vertices exist only once this stream reaches them
            a.update_blas_device(BOX, d_p, d_q, stream=handle)
            a.refit_blas_device(stream=handle)
            gc = a.intersect_closest_device(d_rays, stream=handle)
        stream.synchronize()
        ref = _oracle(mrt, orc, n, (), (step, None))
        assert float((ref["distance"] >= 0).mean()) >= 0.08
        _same_records(b.intersect_closest(r), ref, f"stream {handle} host path ")
        _same_records(_device_records(gc), ref, f"stream {handle} ")
        a.close(); b.close()


def _snap(ds, r):
    """test_instances_device's snapshot and the packets, which a vertex update rewrites"""
    snap = _snapshot(ds, r)
    snap["wpackets"] = ds.read_layout("wpackets")
    return snap


def test_a_bad_update_writes_nothing(mrt, orc, gpu_ctx):
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    rr = _rays_of(mrt, gpu_ctx, n)
    r, finite = rr[0], rr[1]
    a = mrt.DeviceScene(gpu_ctx, sc, TWO)
    keep = _dev_update(mrt, a, gpu_ctx, BOX, 0); a.refit_blas_device()          # a scene that already deformed once
    torch.cuda.synchronize()
    before = _snap(a, r)
    count = a.device_updates_rejected
    assert count == 0
    p, q = _deformed(mrt, BOX, 1)
    assert len(p) == 24
    nan = p.copy(); nan[-1, 2] = np.nan
    inf = p.copy(); inf[-1, 0] = -np.inf
    qn = q.copy(); qn[7, 1] = np.nan
    qi = q.copy(); qi[-1, 2] = np.inf
    for what, bp, bq in (("NaN position", nan, q), ("infinite position", inf, q), ("NaN normal", p, qn), ("infinite normal", p, qi)):
        tp, tq = _td(bp, gpu_ctx), _td(bq, gpu_ctx)
        a.update_blas_device(BOX, tp, tq); a.refit_blas_device()
        torch.cuda.synchronize()
        count += 1
        assert a.device_updates_rejected == count, what
        _same_snapshot(_snap(a, r), before, f"after a refused call ({what})")
    # a refused pose set of the same scene is counted by another workspace: the two counts add up
    x = _poses(n, 0); x[-1, 13] = np.nan
    d_x = _t(x, gpu_ctx)
    a.set_instance_transforms_device(0, d_x); a.refit_instances_device()
    torch.cuda.synchronize()
    count += 1
    assert a.device_updates_rejected == count, "rejected pose sets and rejected vertex updates add up"
    _same_snapshot(_snap(a, r), before, "after a refused pose set")
    keep1 = _dev_update(mrt, a, gpu_ctx, BOX, 1); a.refit_blas_device()
    b = mrt.DeviceScene(gpu_ctx, sc, TWO)
    _host_update(mrt, b, BOX, 0); _host_update(mrt, b, BOX, 1)
    h = _check(mrt, orc, gpu_ctx, a, b, n, (), (1, None), rr, "a good call after the refused ones: ")
    _changed(h, before["closest"], "a good call after the refused ones: ")
    assert a.device_updates_rejected == count
    del keep, keep1
    a.close(); b.close()


def test_nothing_is_allocated_after_the_first_call(mrt, orc, gpu_ctx):
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    a = mrt.DeviceScene(gpu_ctx, sc, TWO)
    steps = [[_td(x, gpu_ctx) for x in _deformed(mrt, k, s)] for s in range(4) for k in (BOX, QUAD)]
    free = []
    for s in range(4):
        for k in (BOX, QUAD): a.update_blas_device(k, *steps[2 * s + k])
        a.refit_blas_device()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(_dev(gpu_ctx))[0])
    assert len(set(free)) == 1, free          # (the first call made the workspaces before it was measured)
    a.close()


def test_the_host_stays_truthful(mrt, orc, gpu_ctx):
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    rr = _rays_of(mrt, gpu_ctx, n)
    r = rr[0]
    x0 = _poses(n, 0)
    start = _oracle(mrt, orc, n, (), (None, None))
    # an update that no refit followed, then a commit with nothing else changed: a vertex change, so the commit refits
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    links = _links(a)
    keep = _dev_update(mrt, a, gpu_ctx, BOX, 0)          # no refit, no synchronise
    a.commit()
    _host_update(mrt, b, BOX, 0)
    assert a.refits == 1 and b.refits == 1
    _same_layout(a, b, n, "update, no refit, commit: ", tlas_too=True)
    assert _stats(a) == _stats(b), (_stats(a), _stats(b))
    assert np.array_equal(_links(a)[n:], links[n:]), "the commit refits the BLASes (and builds the TLAS in the slots in front of them again)"
    h = _check(mrt, orc, gpu_ctx, a, b, n, (), (0, None), rr, "update, no refit, commit: ")
    _changed(h, start, "update, no refit, commit: ")
    # mrt_scene_stats resolves a device refit with no other call behind it (no synchronise: it has to wait itself)
    keep1 = [_dev_update(mrt, a, gpu_ctx, BOX, 1), _dev_update(mrt, a, gpu_ctx, QUAD, 1)]; a.refit_blas_device()
    sa = _stats(a)
    _host_update(mrt, b, BOX, 1, commit=False); _host_update(mrt, b, QUAD, 1)
    assert sa == _stats(b) and sa[0] == 2, (sa, _stats(b))
    # ... then a transform of ANOTHER instance + commit: a transforms-only commit, whose update_tlas must build from the BLAS roots the device left
    a.set_instance_transform(8, x0[8]); a.commit()
    b.set_instance_transform(8, x0[8]); b.commit()
    _same_layout(a, b, n, "device refit, then a transforms-only commit: ", tlas_too=True)
    h = _check(mrt, orc, gpu_ctx, a, b, n, ((0, 8),), (1, 1), rr, "device refit, then a transforms-only commit: ")
    # the workspace outlives that commit: another device refit on top of it
    keep2 = _dev_update(mrt, a, gpu_ctx, BOX, 0); a.refit_blas_device()
    _host_update(mrt, b, BOX, 0)
    _check(mrt, orc, gpu_ctx, a, b, n, ((0, 8),), (0, 1), rr, "a device refit after the transforms-only commit: ")
    assert _stats(a) == _stats(b), (_stats(a), _stats(b))
    # update_mesh of the same mesh after a device refit: the host copy is the newer one
    a.update_mesh(BOX, *_deformed(mrt, BOX, 1)); a.commit()
    _host_update(mrt, b, BOX, 1)
    _check(mrt, orc, gpu_ctx, a, b, n, ((0, 8),), (1, 1), rr, "update_mesh over a device refit: ")
    # a host change is pending: the device entries refuse
    p, q = _deformed(mrt, BOX, 0)
    d_p, d_q = _td(p, gpu_ctx), _td(q, gpu_ctx)
    a.set_instance_transform(3, x0[3])
    assert mrt.lib.mrt_scene_update_blas_device(a.handle, BOX, C.c_void_p(d_p.data_ptr()), 12, C.c_void_p(d_q.data_ptr()), 12, len(p), None) == STATE and UPDATE in mrt.lib.mrt_last_error().decode()
    assert mrt.lib.mrt_scene_refit_blas_device(a.handle, None) == STATE and REFIT in mrt.lib.mrt_last_error().decode()
    a.commit(); b.set_instance_transform(3, x0[3]); b.commit()
    # add_instance after a device refit: the build starts from the vertices the device holds
    a.update_blas_device(BOX, d_p, d_q); a.refit_blas_device()
    _host_update(mrt, b, BOX, 0)
    before = b.intersect_closest(r)
    xf = np.ascontiguousarray(x0[0], np.float32); xf[12:15] = [0.0, 0.9, 0.2]
    for ds in (a, b):
        mid = C.c_int32()
        assert mrt.lib.mrt_scene_add_instance(ds.handle, BOX, xf.ctypes.data_as(C.c_void_p), C.byref(mid)) == 0 and mid.value == n
        ds.commit()
    assert a.stats.instances == n + 1 and a.refits == 0
    hb = b.intersect_closest(r)
    _same_records(a.intersect_closest(r), hb, "add_instance after a device refit ")
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), "add_instance after a device refit: instance boxes"
    assert (_bits(hb["distance"]) != _bits(before["distance"])).sum() > 20
    del keep, keep1, keep2
    a.close(); b.close()


@pytest.mark.parametrize("route", ["device poses", "device poses, refitted", "host transform"])
def test_an_unrefitted_update_beside_a_transform_change_is_not_lost(mrt, orc, gpu_ctx, route):
    """update_blas_device with no refit behind it, and a transform change pending as well — poses set on the device before it, or set_instance_transform after it: the
    commit must not take the transforms-only branch, which would keep the old BLAS under the new vertices"""
    n = 9
    sc, meshes, rays = _case(mrt, n)
    rr = _rays_of(mrt, gpu_ctx, n)
    x = _poses(n, 0)
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    if route == "host transform":
        keep = [_dev_update(mrt, a, gpu_ctx, BOX, 0), _dev_update(mrt, a, gpu_ctx, QUAD, 0)]          # no refit
        a.set_instance_transform(8, x[8])
        pose_key = ((0, 8),)
        b.set_instance_transform(8, x[8])
    else:
        d_x = _t(x, gpu_ctx)
        a.set_instance_transforms_device(0, d_x)
        if route == "device poses, refitted": a.refit_instances_device()
        keep = [_dev_update(mrt, a, gpu_ctx, BOX, 0), _dev_update(mrt, a, gpu_ctx, QUAD, 0)]          # no refit
        pose_key = ((0, 0),)
        for k in range(n): b.set_instance_transform(k, x[k])
    a.commit()
    _host_update(mrt, b, BOX, 0, commit=False); _host_update(mrt, b, QUAD, 0)          # vertices and transforms on the host: a full build
    assert a.refits == 0 and b.refits == 0
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), route + ": instance boxes"
    assert np.array_equal(_bits(a.read_layout("wpackets")), _bits(b.read_layout("wpackets"))), route + ": packets"
    h = _check(mrt, orc, gpu_ctx, a, b, n, pose_key, (0, 0), rr, route + ": ", layout=False)
    _changed(h, _oracle(mrt, orc, n, pose_key, (None, None)), route + ": against the undeformed meshes under the same poses: ")
    # nothing of it lingers: the next device refit is the host path's again
    keep1 = _dev_update(mrt, a, gpu_ctx, BOX, 1); a.refit_blas_device()
    _host_update(mrt, b, BOX, 1)
    _check(mrt, orc, gpu_ctx, a, b, n, pose_key, (1, 0), rr, route + ", then a device refit: ")
    assert _stats(a) == _stats(b), (_stats(a), _stats(b))
    del keep, keep1
    a.close(); b.close()


def test_refusals(mrt, orc, gpu_ctx):
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays[:512])
    lib = mrt.lib
    p, q = _deformed(mrt, BOX, 0)
    d_p, d_q = _td(p, gpu_ctx), _td(q, gpu_ctx)
    nv = len(p)

    def last():
        return lib.mrt_last_error().decode()

    def raw(h, mesh=BOX, ps=12, ns=12, count=nv, pp=d_p.data_ptr(), qq=d_q.data_ptr()):
        return lib.mrt_scene_update_blas_device(h, mesh, C.c_void_p(pp), ps, C.c_void_p(qq), ns, count, None)

    ds = mrt.DeviceScene(gpu_ctx, sc, TWO)
    before = ds.intersect_closest(r)
    for args in (dict(count=nv - 1), dict(count=nv + 1), dict(ps=10), dict(ns=14), dict(ps=8), dict(ns=0), dict(mesh=2), dict(mesh=n - 1), dict(mesh=n), dict(mesh=99), dict(mesh=-1),
                 dict(pp=None), dict(qq=None), dict(pp=d_p.data_ptr() + 2), dict(qq=d_q.data_ptr() + 1)):
        assert raw(ds.handle, **args) == INVALID, args
        assert UPDATE in last(), last()
    assert raw(ds.handle, mesh=2) == INVALID and "instance" in last()
    for bad in (d_p.cpu(), d_p.double(), d_p.t().contiguous().t(), d_p[:, :2], p):
        with pytest.raises((ValueError, TypeError)):
            ds.update_blas_device(BOX, bad, d_q)
        with pytest.raises((ValueError, TypeError)):
            ds.update_blas_device(BOX, d_p, bad)
    with pytest.raises(mrt.MRTError) as e:
        ds.update_blas_device(BOX, d_p, d_q[:-1])
    assert e.value.code == INVALID
    torch.cuda.synchronize()
    _same_records(ds.intersect_closest(r), before, "after the refused calls ")
    assert ds.refits == 0 and ds.device_updates_rejected == 0
    ds.close()
    # never committed
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    assert lib.mrt_scene_refit_blas_device(h, None) == STATE and REFIT in last()
    assert raw(h) == STATE and UPDATE in last()
    # a mesh without triangles beside the box: its BLAS has nothing to refit, and the call names the mesh
    ident = np.eye(4, dtype=np.float32).reshape(16)
    bp, bn, bi = (np.ascontiguousarray(x) for x in (meshes[BOX][0], meshes[BOX][1], meshes[BOX][3][0][0]))
    mid = C.c_int32()
    assert lib.mrt_scene_set_option(h, b"instancing", 1.0) == 0
    assert lib.mrt_scene_add_mesh(h, bp.ctypes.data_as(C.c_void_p), 12, bn.ctypes.data_as(C.c_void_p), 12, len(bp), ident.ctypes.data_as(C.c_void_p), C.byref(mid)) == 0 and mid.value == 0
    bi = np.ascontiguousarray(bi, np.uint32)
    assert lib.mrt_mesh_add_submesh(h, 0, bi.ctypes.data_as(C.c_void_p), bi.shape[0], C.byref(meshes[BOX][3][0][1]), None) == 0
    assert lib.mrt_scene_add_mesh(h, bp.ctypes.data_as(C.c_void_p), 12, bn.ctypes.data_as(C.c_void_p), 12, len(bp), ident.ctypes.data_as(C.c_void_p), C.byref(mid)) == 0 and mid.value == 1
    assert lib.mrt_scene_commit(h) == 0, last()
    assert raw(h, mesh=1) == UNSUPPORTED and UPDATE in last() and "mesh 1" in last()
    assert raw(h, mesh=0) == 0 and lib.mrt_scene_refit_blas_device(h, None) == 0, last()          # the mesh beside it deforms
    torch.cuda.synchronize()
    assert lib.mrt_scene_destroy(h) == 0


# ------------------------------------------------------------------------------------------------ what a commit makes of changes of several kinds (csrc/scene_changes.h)
# The sequences in which the three booleans that came before the one value ended in a TLAS-only commit over stale BLASes (tests/test_scene_changes_cpu.py lists them), on
# the scene of 9 instances.  Each needs the host to learn of a device-side change between two changes without a commit: mrt_group_renderer_create does that to its template.
N_SEQ = 9
FROM = 5          # the instances FROM .. 8 take their poses of step 1, the others keep those of step 0


def _found_by_a_sync(mrt, ds):
    """what mrt_group_renderer_create does to its template scene: the host copies brought up to date (mrt_scene_sync_host_meshes); the group and its renderer go again"""
    lib = mrt.lib
    ids = (C.c_int32 * 1)(0)
    g, r = C.c_void_p(), C.c_void_p()
    assert lib.mrt_group_create(ids, 1, C.byref(g)) == 0, lib.mrt_last_error()
    assert lib.mrt_group_renderer_create(g, ds.handle, 16, 16, 1, 3, C.byref(r)) == 0, lib.mrt_last_error()
    assert lib.mrt_group_renderer_destroy(r) == 0 and lib.mrt_group_destroy(g) == 0, lib.mrt_last_error()


def _dev_move(ds, gpu_ctx, step, first=0):
    t = _t(_poses(N_SEQ, step)[first:], gpu_ctx)
    ds.set_instance_transforms_device(first, t)
    return t


def _from_scratch(mrt, gpu_ctx, opts, pose_key, box_step):
    """a scene with the final vertices and poses that is built, not updated: an option set before the commit makes it build everything"""
    ds = mrt.DeviceScene(gpu_ctx, _case(mrt, N_SEQ)[0], opts)
    xf = _start(N_SEQ)
    for step, first in pose_key: xf[first:] = _poses(N_SEQ, step)[first:]
    for k in range(N_SEQ): ds.set_instance_transform(k, xf[k])
    ds.update_mesh(BOX, *_deformed(mrt, BOX, box_step))
    assert mrt.lib.mrt_scene_set_option(ds.handle, b"validate", 1.0) == 0
    ds.commit()
    assert ds.stats.refits == 0
    return ds


def _row_1(mrt, ds, gpu_ctx, keep):
    keep.append(_dev_move(ds, gpu_ctx, 0)); _found_by_a_sync(mrt, ds)
    ds.update_mesh(BOX, *_deformed(mrt, BOX, 0))
    return ((0, 0),)


def _row_2(mrt, ds, gpu_ctx, keep):
    keep.append(_dev_move(ds, gpu_ctx, 0)); _found_by_a_sync(mrt, ds)
    keep.append(_dev_update(mrt, ds, gpu_ctx, BOX, 0)); _found_by_a_sync(mrt, ds)
    return ((0, 0),)


def _row_3(mrt, ds, gpu_ctx, keep):
    keep.append(_dev_update(mrt, ds, gpu_ctx, BOX, 0)); keep.append(_dev_move(ds, gpu_ctx, 0)); _found_by_a_sync(mrt, ds)
    for k in range(FROM, N_SEQ): ds.set_instance_transform(k, _poses(N_SEQ, 1)[k])
    return ((0, 0), (1, FROM))


def _row_4(mrt, ds, gpu_ctx, keep):
    keep.append(_dev_update(mrt, ds, gpu_ctx, BOX, 0)); keep.append(_dev_move(ds, gpu_ctx, 0)); _found_by_a_sync(mrt, ds)
    keep.append(_dev_move(ds, gpu_ctx, 1, FROM)); _found_by_a_sync(mrt, ds)
    return ((0, 0), (1, FROM))


@pytest.mark.parametrize("row", [_row_1, _row_2, _row_3, _row_4], ids=["moves found, then update_mesh", "moves found, then an unrefitted update found", "both found, then set_instance_transform", "both found, then moves found again"])
def test_a_commit_after_changes_of_both_kinds_builds_the_blases_too(mrt, orc, gpu_ctx, row):
    import torch
    r = np.array(_case(mrt, N_SEQ)[2])
    ds = mrt.DeviceScene(gpu_ctx, _case(mrt, N_SEQ)[0], TWO)
    keep = []
    pose_key = row(mrt, ds, gpu_ctx, keep)
    ds.commit()
    torch.cuda.synchronize()
    assert ds.stats.refits == 0 and ds.refits == 0          # vertices and transforms: the recipe is a build, and a build counts no refit
    ref = _oracle(mrt, orc, N_SEQ, pose_key, (0, None))
    assert float((ref["distance"] >= 0).mean()) >= 0.08
    _changed(ref, _oracle(mrt, orc, N_SEQ, pose_key, (None, None)), "the deformed box against the box as it was: ")          # (what a TLAS-only commit would answer)
    scratch = _from_scratch(mrt, gpu_ctx, TWO, pose_key, 0)
    hits = ds.intersect_closest(r)
    _same_records(hits, scratch.intersect_closest(r), "against the scene built from scratch: ")
    _same_records(hits, ref, "against the oracle: ")
    A.audit(A.layout_of(ds)).check()
    assert ds.device_updates_rejected == 0
    del keep
    ds.close(); scratch.close()


def test_a_flattened_scene_waiting_with_transforms_keeps_the_vertices_the_device_wrote(mrt, orc, gpu_ctx):
    """the one exception to the join: update_mesh_device without a refit, then set_instance_transform, then commit — built from the geometry on the device, where the update wrote"""
    import torch
    sc, meshes, rays = _case(mrt, N_SEQ)
    r = np.array(rays)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    tp, tq = (_td(x, gpu_ctx) for x in _deformed(mrt, BOX, 0))
    ds.update_mesh_device(BOX, tp, tq)
    for k in range(FROM, N_SEQ): ds.set_instance_transform(k, _poses(N_SEQ, 1)[k])
    ds.commit()
    torch.cuda.synchronize()
    assert ds.stats.refits == 0 and ds.refits == 0          # build_keep_geometry is a build
    xf = _start(N_SEQ); xf[FROM:] = _poses(N_SEQ, 1)[FROM:]
    geo = _deformed(mrt, BOX, 0)
    moved = [(*(geo if k % 2 == BOX else (p, nr)), np.ascontiguousarray(xf[k]), subs, src) for k, (p, nr, _, subs, src) in enumerate(meshes)]
    ref = orc.OracleScene(moved, sc.lights).intersect_closest(r, brute=True)
    assert float((ref["distance"] >= 0).mean()) >= 0.08
    scratch = _from_scratch(mrt, gpu_ctx, {}, ((1, FROM),), 0)
    hits = ds.intersect_closest(r)
    _same_records(hits, scratch.intersect_closest(r), "against the scene built from scratch: ")
    _same_records(hits, ref, "against the oracle: ")
    assert ds.device_updates_rejected == 0
    del tp, tq
    ds.close(); scratch.close()
