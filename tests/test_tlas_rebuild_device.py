"""The TLAS of a two-level scene rebuilt on the device, on the caller's stream (DeviceScene.rebuild_tlas_device).  Scene A gets poses from a torch tensor
and rebuilds; scene B gets the same matrices through set_instance_transform + commit, which builds both TLAS forms on the host.  The host builders split every range of
instances at half its count, so the rope TLAS of A must be B's bit for bit (`tlas_nodes`), every rope leaf must hold B's instance set, and every query must return B's
record; the 8-wide form keeps the last commit's collapse and gets fresh sets under it.  Scene C only refits (refit_instances_device): the yardstick for the direction of
quality.  The scene, pose and comparison helpers are those of tests/test_instances_device.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_audit as A
import tlas_resort_reference as R
import test_instances_device as T
from test_blas_device import BOX, QUAD, _dev_update, _host_update
from test_fuzz_geometry import _material, _rays
from test_instances_device import (FIELDS, OPTIONS, SIZE, STATE, UNSUPPORTED, _bits, _case, _dev, _device_records, _host_move, _oracle_hits, _poses, _same_records, _same_snapshot,
                                   _snapshot, _start, _t)

pytestmark = pytest.mark.gpu

LIMIT = 1024                    # instances one workgroup re-sorts in LDS (TLAS_RESORT_LDS_LIMIT)
BIG = 2 * LIMIT + 3             # the smallest count at which the one-level-per-step path runs twice (2051 -> 1025 + 1026 -> four ranges in LDS) and a range is odd
COUNTS = T.COUNTS + (BIG,)      # 1, 2, 3, 9, 65, 150 as tests/test_instances_device.py explains them
TWO = {"instancing": 1}
ENTRY = "mrt_scene_rebuild_tlas_device"


@functools.lru_cache(maxsize=None)
def _quad_case(mrt, n):
    """n instances of the quad alone at their start poses, and the rays: the scene of the large count"""
    qp, qn, qi = T._quad_mesh()
    subs = [mrt.Submesh("quad", qi, _material(mrt, (0.2, 0.4, 0.8)))]
    start = _start(n)

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            first = T._Hand(mrt, "quad", qp, qn, subs)
            src = first.meshes[0]
            self.models = [first] + [T._Hand(mrt, src.modelName, src.positions, src.normals, src.submeshes) for _ in range(1, n)]
            for k in range(n): self.models[k].meshes[0].transform = start[k].reshape(4, 4).copy()

    sc = S(SIZE)
    rays = _rays(np.random.default_rng(300 + n), 4000)
    rays.setflags(write=False)
    return sc, None, rays


def _scene_of(mrt, n):
    return _quad_case(mrt, n) if n > 150 else _case(mrt, n)


def _leaf_sets(ds):
    """the instance set of every leaf of the rope TLAS, in node order"""
    nodes, index = ds.read_layout("tlas_nodes"), ds.read_layout("tlas_index")
    return [frozenset(index[first:first + count].tolist()) for first, count in R.rope_leaves(nodes[:, [3, 7, 8, 8]])]


def _live(ds):
    box = ds.read_layout("inst_box")
    return np.flatnonzero(box[:, 8] <= box[:, 12])          # (an instance outside the TLAS has an empty world box)


def _check(mrt, orc, gpu_ctx, a, b, n, key, rays, what, header=None):
    """scene A (moved and rebuilt on the device) against scene B (moved on the host, TLAS built by the commit) and, up to 150 instances, the oracle's brute force"""
    import torch
    torch.cuda.synchronize()
    r = np.array(rays)
    finite = r.copy(); finite[:, 7] = 3.0
    d_rays, d_finite = _t(r, gpu_ctx), _t(finite, gpu_ctx)
    assert np.array_equal(a.read_layout("instances"), b.read_layout("instances")), what + "instance rows"
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), what + "instance boxes"
    ta, tb = a.read_layout("tlas_nodes"), b.read_layout("tlas_nodes")
    assert ta.shape == tb.shape and len(ta) == a.stats.bvh_nodes
    bad = np.flatnonzero((ta != tb).any(axis=1))
    assert len(bad) == 0, f"{what}tlas_nodes: {len(bad)} of {len(ta)} rope nodes differ from the commit's, first {bad[0]}: {ta[bad[0]]} against {tb[bad[0]]}"
    assert _leaf_sets(a) == _leaf_sets(b), what + "rope leaf sets"
    live = _live(b)
    assert np.array_equal(np.sort(a.read_layout("tlas_index")), live), what + "tlas_index is a permutation of the live ids"
    assert a.stats.wide_layout == b.stats.wide_layout
    if a.stats.wide_layout:
        assert np.array_equal(np.sort(a.read_layout("wtlas_index")), live), what + "wtlas_index is a permutation of the live ids"
        A.audit(A.layout_of(a)).check()
    if header is not None: assert np.array_equal(a.read_layout("header"), header), what + "header"
    hb = b.intersect_closest(r)
    _same_records(a.intersect_closest(r), hb, what + "host entry ")
    _same_records(_device_records(a.intersect_closest_device(d_rays)), hb, what + "device entry ")
    if a.stats.wide_layout:
        _same_records(a.intersect_stream(r), b.intersect_stream(r), what + "stream walk ")
        assert np.array_equal(a.intersect_stream(finite, any_hit=True)["type"], b.intersect_stream(finite, any_hit=True)["type"]), what + "stream any"
    if n <= 150: _same_records(hb, _oracle_hits(mrt, orc, n, key), what + "oracle ")
    occ = b.intersect_any(finite)
    assert np.array_equal(a.intersect_any(finite), occ), what + "any-hit"
    assert np.array_equal(a.intersect_any_device(d_finite).cpu().numpy(), occ), what + "any-hit device entry"
    return hb


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", list(OPTIONS))
def test_parity_with_the_host_path(mrt, orc, gpu_ctx, layout, n):
    sc, _, rays = _scene_of(mrt, n)
    opts = dict(OPTIONS[layout], instancing=1)
    a, b = mrt.DeviceScene(gpu_ctx, sc, opts), mrt.DeviceScene(gpu_ctx, sc, opts)
    assert a.stats.wide_layout == (0 if layout == "rope" else 1) and a.stats.instances == n
    header = a.read_layout("header")
    nodes, depth = a.stats.bvh_nodes, a.stats.max_depth
    before = a.intersect_closest(np.array(rays))
    x0 = _poses(n, 0)          # every instance moves; the far-left and the far-right one trade places
    d0 = _t(x0, gpu_ctx)
    a.set_instance_transforms_device(0, d0); a.rebuild_tlas_device()
    _host_move(b, 0, x0)
    h0 = _check(mrt, orc, gpu_ctx, a, b, n, ((0, 0),), rays, f"{layout} n={n} step 0: ", header)
    assert (_bits(h0["distance"]) != _bits(before["distance"])).sum() > 50, "the move must change some answers"
    # a second step from the order the first rebuild left: a sub-range of the instances
    first = 1 if n >= 2 else 0
    x1 = _poses(n, 1)
    d1 = _t(x1[first:], gpu_ctx)
    a.set_instance_transforms_device(first, d1); a.rebuild_tlas_device()
    _host_move(b, first, x1[first:])
    _check(mrt, orc, gpu_ctx, a, b, n, ((0, 0), (1, first)), rays, f"{layout} n={n} step 1: ", header)
    assert (a.stats.bvh_nodes, a.stats.max_depth) == (nodes, depth)
    assert a.device_updates_rejected == 0
    a.close(); b.close()


def _wide_tlas_area(ds):
    """the summed surface area of the child boxes of the 8-wide TLAS, decoded as bvh_audit decodes them"""
    cap = int(ds.read_layout("header")[1])
    D = A.decode_nodes(ds.read_layout("wnodes")[:cap])
    occupied = (((D["imask"][:, None] >> np.arange(8)[None, :]) & 1) != 0) | ((D["meta"] >> 5) > 0)
    e = D["hi"] - D["lo"]
    area = 2.0 * (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0])
    return float(area[occupied].sum())


@pytest.mark.parametrize("n", COUNTS)
def test_a_rebuild_tightens_what_a_refit_leaves_loose(mrt, orc, gpu_ctx, n):
    """all instances reversed end for end: instance k takes the start pose of instance n - 1 - k"""
    import torch
    sc, _, rays = _scene_of(mrt, n)
    x = _start(n)[::-1].copy()
    d = _t(x, gpu_ctx)
    a, b, c = (mrt.DeviceScene(gpu_ctx, sc, TWO) for _ in range(3))
    a.set_instance_transforms_device(0, d); a.rebuild_tlas_device()
    c.set_instance_transforms_device(0, d); c.refit_instances_device()
    _host_move(b, 0, x)
    torch.cuda.synchronize()
    sa, sb, sc_ = _wide_tlas_area(a), _wide_tlas_area(b), _wide_tlas_area(c)
    print(f"n={n}: 8-wide TLAS child area rebuilt on the device {sa:.6g}, refitted {sc_:.6g}, committed {sb:.6g}; rebuilt / committed {sa / sb:.4f}, refitted / committed {sc_ / sb:.4f}")
    assert sa <= sc_, (sa, sc_)
    if n in (65, 150): assert sa < sc_, (sa, sc_)
    r = np.array(rays)
    _same_records(a.intersect_closest(r), b.intersect_closest(r), f"n={n} reversed: ")
    for ds in (a, b, c): ds.close()


@pytest.mark.parametrize("n,guides", [(9, 0), (9, 1), (65, 0)])
def test_a_renderer_made_before_the_rebuild_draws_the_moved_scene(mrt, orc, gpu_ctx, n, guides):
    """9 instances: the two-level primary walk, and bounce and shadow rays through the tree-less TLAS pass over inst_box; 65: they walk the rebuilt TLAS"""
    import torch
    sc, meshes, rays = _case(mrt, n)
    ra = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options=TWO); rb = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options=TWO)
    if guides:
        for rr in (ra, rb): rr.set_option("guides", 1)
    ra.draw(2, wait=True)
    still = ra.accumulation().copy()
    for step in range(2):
        x = _poses(n, step)
        d = _t(x, gpu_ctx)
        ra.device_scene.set_instance_transforms_device(0, d); ra.device_scene.rebuild_tlas_device()
        torch.cuda.synchronize()          # (the renderer draws on the context's streams)
        _host_move(rb.device_scene, 0, x)
        for rr in (ra, rb):
            rr.frameIndex = 0; rr.reset_stats(); rr.draw(2, wait=True)
        assert np.array_equal(_bits(ra.accumulation()), _bits(rb.accumulation())), f"step {step}: the two paths must render the same image"
        assert (ra.stats.closest_rays, ra.stats.shadow_rays) == (rb.stats.closest_rays, rb.stats.shadow_rays)
    assert not np.array_equal(_bits(ra.accumulation()), _bits(still))
    ra.close(); rb.close()


def test_stream_order(mrt, orc, gpu_ctx):
    """a torch expression that makes the poses, the set call, the rebuild and a query on ONE side stream, nothing of the host in between, one synchronise at the end"""
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    dev = _dev(gpu_ctx)
    d_rays = _t(r, gpu_ctx)
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream not in (0, gpu_ctx.stream)
    x = _poses(n, 0)
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    _host_move(b, 0, x)
    src = _t(x, gpu_ctx)
    d_x = torch.zeros_like(src)
    a.rebuild_tlas_device()          # (the first call after a commit makes the workspace and may block: not part of what is ordered below)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)          # the stream is busy when the poses are made
        z = torch.nan_to_num(big[0, 0] * 0.0)
        d_x.copy_(src * 2.0 * 0.5 + z)          # exact; the poses exist only once this stream reaches them
        a.set_instance_transforms_device(0, d_x)
        a.rebuild_tlas_device()
        gc = a.intersect_closest_device(d_rays)
    side.synchronize()
    _same_records(_device_records(gc), b.intersect_closest(r), "side stream ")
    torch.cuda.synchronize()
    assert np.array_equal(a.read_layout("tlas_nodes"), b.read_layout("tlas_nodes"))
    a.close(); b.close()


def _forms(ds):
    """parts 0 (the TLAS slots), 4, 6 and 7: every word of both TLAS forms"""
    cap = int(ds.read_layout("header")[1])
    out = {"tlas_nodes": ds.read_layout("tlas_nodes"), "tlas_index": ds.read_layout("tlas_index")}
    if ds.stats.wide_layout: out.update(wnodes=ds.read_layout("wnodes")[:cap], wtlas_index=ds.read_layout("wtlas_index"))
    return out


@pytest.mark.parametrize("n", (2, 9, 150, BIG))
@pytest.mark.parametrize("layout", ("wide", "rope"))
def test_a_second_rebuild_is_a_fixed_point(mrt, orc, gpu_ctx, layout, n):
    import torch
    sc, _, rays = _scene_of(mrt, n)
    r = np.array(rays)
    a = mrt.DeviceScene(gpu_ctx, sc, dict(OPTIONS[layout], instancing=1))
    # at the start poses: the rope nodes are the commit's, and no answer changes
    committed = a.read_layout("tlas_nodes")
    before = a.intersect_closest(r), a.intersect_any(r)
    a.rebuild_tlas_device()
    torch.cuda.synchronize()
    assert np.array_equal(a.read_layout("tlas_nodes"), committed), "a rebuild at the start poses leaves tlas_nodes as the commit wrote it"
    _same_records(a.intersect_closest(r), before[0], "a rebuild with nothing moved ")
    assert np.array_equal(a.intersect_any(r), before[1])
    # after a move: the second rebuild finds the order the first left
    d = _t(_poses(n, 0), gpu_ctx)
    a.set_instance_transforms_device(0, d); a.rebuild_tlas_device()
    torch.cuda.synchronize()
    first = _forms(a)
    assert not np.array_equal(first["tlas_nodes"], committed)
    a.rebuild_tlas_device()
    torch.cuda.synchronize()
    second = _forms(a)
    for part in first: assert np.array_equal(first[part], second[part]), part
    a.close()


def test_mixed_with_the_refits(mrt, orc, gpu_ctx):
    """set -> refit_instances -> set -> rebuild -> update_blas_device + refit_blas_device -> rebuild: the host path's tree and answers"""
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    x0, x1 = _poses(n, 0), _poses(n, 1)
    d0, d1 = _t(x0, gpu_ctx), _t(x1[1:], gpu_ctx)
    a.set_instance_transforms_device(0, d0); a.refit_instances_device()
    a.set_instance_transforms_device(1, d1); a.rebuild_tlas_device()
    keep = [_dev_update(mrt, a, gpu_ctx, BOX, 0), _dev_update(mrt, a, gpu_ctx, QUAD, 0)]
    a.refit_blas_device()
    a.rebuild_tlas_device()
    torch.cuda.synchronize()
    _host_move(b, 0, x0); _host_move(b, 1, x1[1:])
    _host_update(mrt, b, BOX, 0, commit=False); _host_update(mrt, b, QUAD, 0)
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), "instance boxes"
    assert np.array_equal(a.read_layout("tlas_nodes"), b.read_layout("tlas_nodes")), "the rope TLAS over the deformed meshes' boxes"
    assert _leaf_sets(a) == _leaf_sets(b)
    A.audit(A.layout_of(a)).check()
    _same_records(a.intersect_closest(r), b.intersect_closest(r), "mixed ")
    _same_records(a.intersect_stream(r), b.intersect_stream(r), "mixed, stream walk ")
    assert np.array_equal(a.intersect_any(r), b.intersect_any(r))
    del keep
    a.close(); b.close()


def test_a_refused_set_call_before_a_rebuild(mrt, orc, gpu_ctx):
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a = mrt.DeviceScene(gpu_ctx, sc, TWO)
    good = _t(_poses(n, 0), gpu_ctx)
    a.set_instance_transforms_device(0, good); a.rebuild_tlas_device()
    torch.cuda.synchronize()
    before = _snapshot(a, r); forms = _forms(a)
    bad = _poses(n, 1); bad[-1, 13] = np.nan
    d = _t(bad, gpu_ctx)
    a.set_instance_transforms_device(0, d); a.rebuild_tlas_device()
    torch.cuda.synchronize()
    assert a.device_updates_rejected == 1
    _same_snapshot(_snapshot(a, r), before, "after a refused set call and a rebuild")
    now = _forms(a)
    for part in forms: assert np.array_equal(forms[part], now[part]), part
    a.close()


@pytest.mark.parametrize("n", (65, BIG))
def test_nothing_is_allocated_after_the_first_call(mrt, orc, gpu_ctx, n):
    import torch
    sc, _, rays = _scene_of(mrt, n)
    a = mrt.DeviceScene(gpu_ctx, sc, TWO)
    steps = [_t(_poses(n, s), gpu_ctx) for s in range(4)]
    a.set_instance_transforms_device(0, steps[0]); a.rebuild_tlas_device()          # each entry once: the workspace exists
    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(_dev(gpu_ctx))[0]]
    for s in range(20):
        a.set_instance_transforms_device(0, steps[s % 4]); a.rebuild_tlas_device()
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info(_dev(gpu_ctx))[0])
    assert free[0] == free[1], free
    a.close()


def test_refusals(mrt, orc, gpu_ctx):
    n = 9
    sc, meshes, rays = _case(mrt, n)
    lib = mrt.lib

    def last():
        return lib.mrt_last_error().decode()

    flat = mrt.DeviceScene(gpu_ctx, sc)
    assert lib.mrt_scene_rebuild_tlas_device(flat.handle, None) == UNSUPPORTED and ENTRY in last()
    with pytest.raises(mrt.MRTError) as e: flat.rebuild_tlas_device()
    assert e.value.code == UNSUPPORTED
    flat.close()
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    assert lib.mrt_scene_rebuild_tlas_device(h, None) == STATE and ENTRY in last()          # never committed
    assert lib.mrt_scene_destroy(h) == 0
    ds = mrt.DeviceScene(gpu_ctx, sc, TWO)
    x = _poses(n, 0)
    ds.set_instance_transform(3, x[3])
    assert lib.mrt_scene_rebuild_tlas_device(ds.handle, None) == STATE and ENTRY in last() and "commit" in last()          # a host change is pending
    ds.commit()
    assert lib.mrt_scene_rebuild_tlas_device(ds.handle, None) == 0
    ds.close()
    # a scene whose only instance is singular: nothing is in the TLAS
    one = mrt.DeviceScene(gpu_ctx, _case(mrt, 1)[0], TWO)
    assert lib.mrt_scene_rebuild_tlas_device(one.handle, None) == 0
    m = _poses(1, 0)[0].copy(); m[0:4] = 0.0
    one.set_instance_transform(0, m); one.commit()
    assert lib.mrt_scene_rebuild_tlas_device(one.handle, None) == UNSUPPORTED and ENTRY in last()
    one.close()


def test_the_host_stays_truthful(mrt, orc, gpu_ctx):
    """after a rebuild, set_instance_transform on one instance + commit gives the layout and the answers of a scene built from scratch with those matrices"""
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a, b = mrt.DeviceScene(gpu_ctx, sc, TWO), mrt.DeviceScene(gpu_ctx, sc, TWO)
    x0, x1 = _poses(n, 0), _poses(n, 1)
    d = _t(x0, gpu_ctx)
    a.set_instance_transforms_device(0, d); a.rebuild_tlas_device()          # no synchronise: the commit below has to wait for the stream's poses itself
    st = a.stats
    assert st.instances == n and st.bvh_nodes > 0
    a.set_instance_transform(8, x1[8]); a.commit()
    x = x0.copy(); x[8] = x1[8]
    _host_move(b, 0, x)
    tlas = int(a.read_layout("header")[1])
    for part in ("instances", "inst_box", "wnodes", "wtlas_index", "tlas_nodes", "tlas_index", "header"):
        pa, pb = a.read_layout(part), b.read_layout(part)
        if part == "wnodes": pa, pb = pa[:tlas], pb[:tlas]
        assert np.array_equal(_bits(pa), _bits(pb)), part          # the same build from the same matrices
    _same_records(a.intersect_closest(r), b.intersect_closest(r))
    assert np.array_equal(a.intersect_any(r), b.intersect_any(r))
    A.audit(A.layout_of(a)).check()
    a.close(); b.close()
