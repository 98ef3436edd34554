"""Stream-ordered instance moves of two-level scenes (DeviceScene.set_instance_transforms_device / refit_instances_device): poses that live in a torch tensor on the GPU
replace the instances' matrices, and both TLAS forms are refitted with the topology of the last commit, on the caller's stream.  Scene A moves through the new entries,
scene B gets the same matrices through set_instance_transform + commit.  The instance rows and boxes are restated on the device in the host's arithmetic, so they must have
the host's bits; the trees differ in shape (B's is rebuilt), but the closest hit does not depend on the tree: every field of every record, and the image, must be equal,
and equal to the two-level oracle's brute force on the moved scene.  The scenes are instances of two tiny meshes: a 12-triangle box (more than 8 triangles: its BLAS has
an 8-wide root) and a 2-triangle quad (its packets are inlined in the instance's slot)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bvh_audit as A
from test_fuzz_geometry import _material, _rays

pytestmark = pytest.mark.gpu

SIZE = (96, 64)
FIELDS = ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v")
OPTIONS = {"wide": {}, "wide+rope": {"rope": 1}, "rope": {"wide": 0}}
# 1: a root with one leaf child; 2: one rope leaf of two instances; 3: the first median split; 9: the 8-wide TLAS gets a second level; 65: past the 64-instance limit of
# the tree-less TLAS pass (bounce and shadow rays take the TLAS walk), and three 8-wide TLAS levels (asserted from the header below); 150: three full blocks of the set kernels
COUNTS = (1, 2, 3, 9, 65, 150)
UNSUPPORTED, STATE, INVALID = 7, 5, 1


def _box_mesh():
    c = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    pos, nrm, idx = [], [], []
    for q in quads:
        p = c[list(q)]
        n = np.cross(p[1] - p[0], p[2] - p[0]); n /= np.linalg.norm(n)
        b = len(pos)
        pos.extend(p); nrm.extend([n] * 4); idx.extend([[b, b + 1, b + 2], [b, b + 2, b + 3]])
    return np.array(pos, np.float32), np.array(nrm, np.float32), np.array(idx, np.uint32)


def _quad_mesh():
    pos = np.array([[-1, 0, -1], [1, 0, -1], [1, 0.2, 1], [-1, 0, 1]], np.float32)
    return pos, np.array([[0, 1, 0]] * 4, np.float32), np.array([[0, 2, 1], [0, 3, 2]], np.uint32)


class _Hand:
    """stands in for Model: one hand-made mesh, or an earlier one's arrays again (flatten_scene(share=True) makes it an instance)"""
    def __init__(self, mrt, name, pos, nrm, subs):
        self.name = name
        self.meshes = [mrt.Mesh(name, pos, nrm, subs, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)]


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _home(n):
    """where instance k starts: a jittered lattice inside the volume the rays aim at; instance 0 at the far left, instance n - 1 at the far right"""
    rng = np.random.default_rng(7 + n)
    p = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(0.2, 1.6, n), rng.uniform(-1.3, 1.5, n)]
    p[0] = [-1.7, 0.6, 0.3]
    p[-1] = [1.7, 1.0, -0.2]
    return p


def _poses(n, step):
    """(n, 16) float32 column-major matrices: every instance a rotation with non-uniform scale about its (jittered) home; instance 1 mirrored (negative determinant);
    instance 2 translated 1e4 away (where instance_box's delta growth matters); the far-left instance 0 and the far-right instance n - 1 swap places in step 0 and stay
    swapped (the kept topology at its worst)."""
    rng = np.random.default_rng(1000 * n + step)
    home = _home(n)
    out = np.zeros((n, 4, 4))          # [col][row]
    for k in range(n):
        s = rng.uniform(0.05, 0.22, 3) * (1.0 if n > 20 else 1.6 if n > 3 else 4.0)
        M = _rot(rng) * s[None, :]
        if k == 1: M = M * np.array([1.0, -1.0, 1.0])[None, :]
        t = home[k] + rng.normal(size=3) * 0.08
        if k == 2: t = t + np.array([1.0e4, 0.0, -1.0e4]) * (1 + step)
        out[k, :3, :3] = M.T; out[k, 3, :3] = t; out[k, 3, 3] = 1.0
    if n >= 2:
        out[0, 3, :3], out[n - 1, 3, :3] = out[n - 1, 3, :3].copy(), out[0, 3, :3].copy()
    return out.reshape(n, 16).astype(np.float32)


def _start(n):
    out = np.zeros((n, 4, 4))
    home = _home(n)
    for k in range(n):
        out[k, :3, :3] = np.eye(3) * (0.12 if n > 20 else 0.2 if n > 3 else 0.5); out[k, 3, :3] = home[k]; out[k, 3, 3] = 1.0
    return out.reshape(n, 16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(mrt, n):
    """the scene of n instances (even ids: the box, odd ids: the quad) at their start poses, and the rays"""
    bp, bn, bi = _box_mesh(); qp, qn, qi = _quad_mesh()
    box_subs = [mrt.Submesh("box", bi, _material(mrt, (0.8, 0.3, 0.2)))]; quad_subs = [mrt.Submesh("quad", qi, _material(mrt, (0.2, 0.4, 0.8)))]
    start = _start(n)

    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            first = [_Hand(mrt, "box", bp, bn, box_subs), _Hand(mrt, "quad", qp, qn, quad_subs)]
            self.models = []
            for k in range(n):
                src = first[k % 2].meshes[0]
                self.models.append(first[k % 2] if k < 2 else _Hand(mrt, src.modelName, src.positions, src.normals, src.submeshes))
                self.models[-1].meshes[0].transform = start[k].reshape(4, 4).copy()

    sc = S(SIZE)
    meshes = mrt.flatten_scene(sc, share=True)
    assert [m[4] for m in meshes] == [-1, -1][:n] + [k % 2 for k in range(2, n)]
    rays = _rays(np.random.default_rng(300 + n), 4000)
    rays.setflags(write=False)
    return sc, meshes, rays


@functools.lru_cache(maxsize=None)
def _oracle_hits(mrt, orc, n, key):
    """the two-level oracle's brute force on the scene with the poses `key` = ((step, first), ...) applied in that order; computed once per scene and pose set"""
    sc, meshes, rays = _case(mrt, n)
    xf = _start(n)
    for step, first in key: xf[first:] = _poses(n, step)[first:]
    moved = [(p, nr, np.ascontiguousarray(xf[k]), subs, src) for k, (p, nr, _, subs, src) in enumerate(meshes)]
    out = orc.OracleScene(moved, sc.lights, instancing=True).intersect_closest(np.array(rays), brute=True)
    out.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_records(a, b, what=""):
    for f in FIELDS:
        bad = np.flatnonzero(_bits(a[f]) != _bits(b[f]))
        assert len(bad) == 0, f"{what}{f}: {len(bad)} records differ, first {bad[0]}: {a[bad[0]]} against {b[bad[0]]}"


def _device_records(t):
    g = t.cpu().numpy()
    out = np.zeros(len(g), dtype=[("type", np.int32), ("distance", np.float32), ("instance_id", np.int32), ("geometry_id", np.int32), ("primitive_id", np.int32), ("u", np.float32), ("v", np.float32)])
    for c, f in enumerate(FIELDS): out[f] = g[:, c].view(out.dtype[f])
    return out


def _dev(gpu_ctx):
    import torch
    return torch.device("cuda", gpu_ctx.device)


def _t(a, gpu_ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(_dev(gpu_ctx))


def _host_move(ds, first, xf):
    for k in range(len(xf)): ds.set_instance_transform(first + k, xf[k])
    ds.commit()


def _snapshot(ds, rays):
    """every layout part the entries write and every query record: what a refused call must leave as it was"""
    snap = {p: ds.read_layout(p) for p in ("instances", "inst_box")}
    if ds.stats.wide_layout: snap["wnodes"] = ds.read_layout("wnodes"); snap["wtlas_index"] = ds.read_layout("wtlas_index")
    snap["closest"] = ds.intersect_closest(rays); snap["any"] = ds.intersect_any(rays)
    return snap


def _same_snapshot(a, b, what):
    for k in a:
        if k == "closest": _same_records(a[k], b[k], what + " ")
        else: assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k}"


def _tlas_levels(ds):
    hdr = ds.read_layout("header")
    return int(hdr[3]) - 1 - int(hdr[5])          # wide_depth = TLAS levels + the parked TLAS group + the deepest BLAS


def _check_against_host(mrt, orc, gpu_ctx, a, b, n, key, rays, d_rays, finite, d_finite, what):
    """assertions 1 - 6 of scene A (moved on the device) against scene B (moved on the host) and the oracle"""
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(a.read_layout("instances"), b.read_layout("instances")), what + "instance rows"
    assert np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box"))), what + "instance boxes"
    assert a.stats.wide_layout == b.stats.wide_layout
    if a.stats.wide_layout:
        A.audit(A.layout_of(a)).check()
    hb = b.intersect_closest(rays)
    _same_records(a.intersect_closest(rays), hb, what + "host entry ")
    _same_records(_device_records(a.intersect_closest_device(d_rays)), hb, what + "device entry ")
    if a.stats.wide_layout:
        _same_records(a.intersect_stream(rays), b.intersect_stream(rays), what + "stream walk ")
        assert np.array_equal(a.intersect_stream(finite, any_hit=True)["type"], b.intersect_stream(finite, any_hit=True)["type"]), what + "stream any"
    else:
        for ds in (a, b):
            with pytest.raises(mrt.MRTError) as e: ds.intersect_stream(rays)
            assert e.value.code == UNSUPPORTED
    _same_records(hb, _oracle_hits(mrt, orc, n, key), what + "oracle ")
    occ = b.intersect_any(finite)
    assert np.array_equal(a.intersect_any(finite), occ), what + "any-hit"
    assert np.array_equal(a.intersect_any_device(d_finite).cpu().numpy(), occ), what + "any-hit device entry"
    return hb


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", list(OPTIONS))
def test_parity_with_the_host_path(mrt, orc, gpu_ctx, layout, n):
    import torch
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    finite = r.copy(); finite[:, 7] = 3.0
    d_rays, d_finite = _t(r, gpu_ctx), _t(finite, gpu_ctx)
    opts = dict(OPTIONS[layout], instancing=1)
    a, b = mrt.DeviceScene(gpu_ctx, sc, opts), mrt.DeviceScene(gpu_ctx, sc, opts)
    assert a.stats.wide_layout == (0 if layout == "rope" else 1) and a.stats.instances == n
    if a.stats.wide_layout:
        levels = _tlas_levels(a)
        assert levels == {1: 1, 2: 1, 3: 1, 9: 2, 65: 3, 150: 3}[n], levels
        links = a.read_layout("wnodes")[:, [3, 4, 5, 6, 7]].copy(); links[:, 0] >>= 24
    nodes, depth = a.stats.bvh_nodes, a.stats.max_depth
    before = a.intersect_closest(r)
    # step 0: the whole scene, packed rows
    x0 = _poses(n, 0)
    d0 = _t(x0, gpu_ctx)
    a.set_instance_transforms_device(0, d0); a.refit_instances_device()
    _host_move(b, 0, x0)
    h0 = _check_against_host(mrt, orc, gpu_ctx, a, b, n, ((0, 0),), r, d_rays, finite, d_finite, f"{layout} n={n} step 0: ")
    assert (_bits(h0["distance"]) != _bits(before["distance"])).sum() > 50, "the move must change some answers"
    # step 1: a sub-range that is not the whole scene (instance 0 keeps its pose), rows 80 bytes apart
    first = 1 if n >= 2 else 0
    x1 = _poses(n, 1)
    wide = torch.full((n - first, 20), float("nan"), device=_dev(gpu_ctx))          # the padding columns are never read
    wide[:, :16] = _t(x1[first:], gpu_ctx)
    d1 = wide[:, :16]
    assert n - first < 2 or d1.stride(0) * 4 == 80
    a.set_instance_transforms_device(first, d1); a.refit_instances_device()
    _host_move(b, first, x1[first:])
    h1 = _check_against_host(mrt, orc, gpu_ctx, a, b, n, ((0, 0), (1, first)), r, d_rays, finite, d_finite, f"{layout} n={n} step 1: ")
    assert (_bits(h1["distance"]) != _bits(h0["distance"])).sum() > 50
    # the topology is the commit's; the statistics keep working
    if a.stats.wide_layout:
        now = a.read_layout("wnodes")[:, [3, 4, 5, 6, 7]].copy(); now[:, 0] >>= 24
        assert np.array_equal(now, links), "a refit moves boxes, never the links between the nodes and to the instances"
    assert (a.stats.bvh_nodes, a.stats.max_depth) == (nodes, depth)
    assert a.device_updates_rejected == 0
    a.close(); b.close()


@pytest.mark.parametrize("n,guides", [(9, 0), (9, 1), (65, 0)])
def test_a_renderer_made_before_the_move_draws_the_moved_scene(mrt, orc, gpu_ctx, n, guides):
    """9 instances: bounce and shadow rays take the tree-less TLAS pass over inst_box; 65: they walk the refitted TLAS"""
    import torch
    sc, meshes, rays = _case(mrt, n)
    ra = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options={"instancing": 1}); rb = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, max_bounces=3, scene_options={"instancing": 1})
    if guides:
        for rr in (ra, rb): rr.set_option("guides", 1)
    ra.draw(2, wait=True)
    still = ra.accumulation().copy()
    for step in range(2):
        x = _poses(n, step)
        d = _t(x, gpu_ctx)
        ra.device_scene.set_instance_transforms_device(0, d); ra.device_scene.refit_instances_device()
        torch.cuda.synchronize()          # (the renderer draws on the context's streams)
        _host_move(rb.device_scene, 0, x)
        for rr in (ra, rb):
            rr.frameIndex = 0; rr.reset_stats(); rr.draw(2, wait=True)
        assert np.array_equal(_bits(ra.accumulation()), _bits(rb.accumulation())), f"step {step}: the two paths must render the same image"
        assert (ra.stats.closest_rays, ra.stats.shadow_rays) == (rb.stats.closest_rays, rb.stats.shadow_rays)
    assert not np.array_equal(_bits(ra.accumulation()), _bits(still))
    ra.close(); rb.close()


def test_stream_order(mrt, orc, gpu_ctx):
    """a torch kernel that makes the poses, the set call, the refit and a query on ONE stream, nothing of the host in between, one synchronise at the end — on a side
    stream and on the null stream"""
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    dev = _dev(gpu_ctx)
    d_rays = _t(r, gpu_ctx)
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream not in (0, gpu_ctx.stream)
    for step, (stream, handle) in enumerate(((side, None), (torch.cuda.default_stream(dev), 0))):
        x = _poses(n, step)
        a, b = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1}), mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
        _host_move(b, 0, x)
        src = _t(x, gpu_ctx)
        d_x = torch.zeros_like(src)
        a.refit_instances_device()          # (the first call after a commit makes the workspace and may block: not part of what is ordered below)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            big = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)          # the stream is busy when the poses are made
            z = torch.nan_to_num(big[0, 0] * 0.0)
            d_x.copy_(src * 2.0 * 0.5 + z)          # exact; the poses exist only once this stream reaches them
            a.set_instance_transforms_device(0, d_x, stream=handle)
            a.refit_instances_device(stream=handle)
            gc = a.intersect_closest_device(d_rays, stream=handle)
        stream.synchronize()
        _same_records(_device_records(gc), b.intersect_closest(r), f"stream {handle} ")
        a.close(); b.close()


def test_several_set_calls_before_one_refit_and_a_refit_with_nothing_moved(mrt, orc, gpu_ctx):
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a, b = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1}), mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    before = _snapshot(a, r)
    a.refit_instances_device()
    torch.cuda.synchronize()
    after = _snapshot(a, r)
    _same_records(after["closest"], before["closest"], "a refit with nothing moved ")
    assert np.array_equal(after["any"], before["any"])
    x = _poses(n, 0)
    lo, hi = _t(x[:4], gpu_ctx), _t(x[4:], gpu_ctx)
    a.set_instance_transforms_device(4, hi); a.set_instance_transforms_device(0, lo); a.refit_instances_device()
    torch.cuda.synchronize()
    _host_move(b, 0, x)
    assert np.array_equal(a.read_layout("instances"), b.read_layout("instances")) and np.array_equal(_bits(a.read_layout("inst_box")), _bits(b.read_layout("inst_box")))
    A.audit(A.layout_of(a)).check()
    _same_records(a.intersect_closest(r), b.intersect_closest(r))
    a.close(); b.close()


def test_a_bad_matrix_refuses_the_whole_call(mrt, orc, gpu_ctx):
    import torch
    n = 65          # more than one wave of matrices: the bad one sits in the last
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    x = _poses(n, 0)
    good = _t(x, gpu_ctx)
    a.set_instance_transforms_device(0, good); a.refit_instances_device()          # a scene that already moved once
    torch.cuda.synchronize()
    before = _snapshot(a, r)
    count = a.device_updates_rejected
    assert count == 0
    x1 = _poses(n, 1)
    nan = x1.copy(); nan[-1, 13] = np.nan
    inf = x1.copy(); inf[-1, 5] = np.inf
    pad = x1.copy(); pad[-1, 7] = np.inf          # the last row is forced to 0 0 0 1, but mrt_scene_set_instance_transform refuses a matrix that is not finite there too
    singular = x1.copy(); singular[-1, 4:8] = 0.0          # a zero column
    for what, bad in (("NaN", nan), ("infinity", inf), ("infinity in the last row", pad), ("singular", singular)):
        d = _t(bad, gpu_ctx)
        a.set_instance_transforms_device(0, d); a.refit_instances_device()
        torch.cuda.synchronize()
        count += 1
        assert a.device_updates_rejected == count, what
        _same_snapshot(_snapshot(a, r), before, f"after a refused call ({what})")
    d = _t(x1, gpu_ctx)
    a.set_instance_transforms_device(0, d); a.refit_instances_device()
    torch.cuda.synchronize()
    assert a.device_updates_rejected == count
    b = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    _host_move(b, 0, x1)
    hb = b.intersect_closest(r)
    assert (_bits(hb["distance"]) != _bits(before["closest"]["distance"])).sum() > 50
    _same_records(a.intersect_closest(r), hb, "a good call after the refused ones ")
    assert np.array_equal(a.read_layout("instances"), b.read_layout("instances"))
    a.close(); b.close()


def test_nothing_is_allocated_after_the_first_call(mrt, orc, gpu_ctx):
    import torch
    n = 65
    sc, meshes, rays = _case(mrt, n)
    a = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    steps = [_t(_poses(n, s), gpu_ctx) for s in range(4)]
    free = []
    for d in steps:
        a.set_instance_transforms_device(0, d); a.refit_instances_device()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(_dev(gpu_ctx))[0])
    assert len(set(free)) == 1, free          # (the first call made the workspace before it was measured)
    a.close()


def test_refusals(mrt, orc, gpu_ctx):
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays[:512])
    lib = mrt.lib
    x = _poses(n, 0)
    d = _t(x, gpu_ctx)
    SET, REFIT = "mrt_scene_set_instance_transforms_device", "mrt_scene_refit_instances_device"

    def last():
        return lib.mrt_last_error().decode()

    def raw(ds, first=0, count=n, ptr=d.data_ptr(), stride=64):
        return lib.mrt_scene_set_instance_transforms_device(ds.handle, first, count, C.c_void_p(ptr), stride, None)

    # a flattened scene: both entries
    flat = mrt.DeviceScene(gpu_ctx, sc)
    assert raw(flat) == UNSUPPORTED and SET in last()
    assert lib.mrt_scene_refit_instances_device(flat.handle, None) == UNSUPPORTED and REFIT in last()
    flat.close()
    # a two-level scene without an instance
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    assert lib.mrt_scene_refit_instances_device(h, None) == STATE and REFIT in last()          # never committed
    assert lib.mrt_scene_set_instance_transforms_device(h, 0, 1, C.c_void_p(d.data_ptr()), 64, None) == STATE and SET in last()
    assert lib.mrt_scene_set_option(h, b"instancing", 1.0) == 0 and lib.mrt_scene_commit(h) == 0
    assert lib.mrt_scene_refit_instances_device(h, None) == UNSUPPORTED and REFIT in last()
    assert lib.mrt_scene_set_instance_transforms_device(h, 0, 0, None, 64, None) == UNSUPPORTED and SET in last()
    assert lib.mrt_scene_destroy(h) == 0
    # argument checks
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    before = ds.intersect_closest(r)
    for args in (dict(first=-1), dict(first=n), dict(first=1), dict(count=n + 1), dict(first=99, count=1), dict(stride=60), dict(stride=66), dict(stride=0), dict(ptr=None), dict(ptr=d.data_ptr() + 2)):
        assert raw(ds, **args) == INVALID, args
        assert SET in last(), last()
    assert raw(ds, count=0, ptr=None) == 0          # nothing to do, nothing launched
    dev = _dev(gpu_ctx)
    for bad in (d.cpu(), d.double(), d.t().contiguous().t(), d[:, :12], d.reshape(n, 4, 4), x):
        with pytest.raises((ValueError, TypeError)):
            ds.set_instance_transforms_device(0, bad)
    assert ds.device_updates_rejected == 0
    # host-side changes pending
    ds.set_instance_transform(3, x[3])
    assert raw(ds) == STATE and SET in last()
    assert lib.mrt_scene_refit_instances_device(ds.handle, None) == STATE and REFIT in last()
    ds.commit()
    # an instance that is not in the TLAS of the last commit: a singular matrix at that commit
    flatm = x[5].copy(); flatm[0:4] = 0.0
    ds.set_instance_transform(5, flatm); ds.commit()
    with_5_out = ds.intersect_closest(r)
    assert raw(ds) == UNSUPPORTED and SET in last() and "instance 5" in last() and "commit" in last()
    assert raw(ds, first=5, count=1) == UNSUPPORTED
    assert raw(ds, first=0, count=5) == 0 and raw(ds, first=6, count=n - 6, ptr=d.data_ptr() + 6 * 64) == 0          # the ranges around it are fine
    ds.refit_instances_device()
    torch.cuda.synchronize()
    moved = ds.intersect_closest(r)
    # ... and a commit brings it in: the poses the device holds plus the new one
    ds.set_instance_transform(5, x[5]); ds.commit()
    b = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    _host_move(b, 0, x)          # (0 .. 4 and 6 .. 8 moved on the device, 3 and 5 on the host: every instance has its pose of x)
    _same_records(ds.intersect_closest(r), b.intersect_closest(r), "after the commit that brings the instance in ")
    assert (_bits(moved["distance"]) != _bits(with_5_out["distance"])).sum() > 20 and (_bits(before["distance"]) != _bits(moved["distance"])).sum() > 20
    ds.close(); b.close()


def test_the_host_stays_truthful(mrt, orc, gpu_ctx):
    """after a device move, set_instance_transform on ANOTHER instance + commit builds the TLAS from the poses the device holds plus the new one"""
    import torch
    n = 9
    sc, meshes, rays = _case(mrt, n)
    r = np.array(rays)
    a, b = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1}), mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    x0, x1 = _poses(n, 0), _poses(n, 1)
    d = _t(x0[2:7], gpu_ctx)
    a.set_instance_transforms_device(2, d); a.refit_instances_device()          # no synchronise: the commit below has to wait for the stream's poses itself
    st = a.stats
    assert st.instances == n and st.bvh_nodes > 0
    a.set_instance_transform(8, x1[8]); a.commit()
    for k in range(2, 7): b.set_instance_transform(k, x0[k])
    b.set_instance_transform(8, x1[8]); b.commit()
    tlas = int(a.read_layout("header")[1])          # (the slots of the 8-wide TLAS in front of the BLASes, whose nodes two builds may number differently)
    for part in ("instances", "inst_box", "wnodes", "wtlas_index"):
        assert np.array_equal(_bits(a.read_layout(part))[:tlas if part == "wnodes" else None], _bits(b.read_layout(part))[:tlas if part == "wnodes" else None]), part          # the same build from the same matrices
    _same_records(a.intersect_closest(r), b.intersect_closest(r))
    assert np.array_equal(a.intersect_any(r), b.intersect_any(r))
    # a host transform of an instance the device moved before is the newer one; and a commit with nothing else changed keeps the device's poses
    d2 = _t(x1[0:3], gpu_ctx)
    a.set_instance_transforms_device(0, d2)          # never refitted on the device
    a.set_instance_transform(1, x0[1]); a.commit()
    b.set_instance_transform(0, x1[0]); b.set_instance_transform(1, x0[1]); b.set_instance_transform(2, x1[2]); b.commit()
    for part in ("instances", "inst_box", "wnodes"):
        assert np.array_equal(_bits(a.read_layout(part))[:tlas if part == "wnodes" else None], _bits(b.read_layout(part))[:tlas if part == "wnodes" else None]), part
    _same_records(a.intersect_closest(r), b.intersect_closest(r), "host transform over a device move ")
    out = (C.c_float * 12)()
    assert mrt.lib.mrt_scene_instance_transform(a.handle, 2, out) == 0
    assert np.array_equal(np.array(out, np.float32).reshape(4, 3), x1[2].reshape(4, 4)[:, :3])
    a.close(); b.close()
