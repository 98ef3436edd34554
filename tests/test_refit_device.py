"""Stream-ordered deformation (DeviceScene.update_mesh_device / refit_device): vertices that live in torch tensors on the GPU replace a mesh's, and the resident tree is
refitted, on the caller's stream.  The device path runs the kernels of the host path (update_mesh + commit), so everything it leaves behind — the 8-wide nodes and packets,
every field of every query record, the image, the statistics — must have the bits the host path leaves; the closest hits must be the oracle's brute force on the deformed
meshes; and the host side must stay truthful afterwards.  The scene is test_fuzz_geometry's hostile one: a plane, a 300-sliver pole fan with two flattened instances, a
triangle soup and stacked sheets."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import bvh_audit as A
import tree_stats_reference as T
from test_fuzz_geometry import _material, _rays, _scene

pytestmark = pytest.mark.gpu

SIZE = (96, 64)
SEED = 1
F32 = np.float32
FIELDS = ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v")
LAYOUTS = {"wide": None, "wide+rope": {"rope": 1}, "rope": {"wide": 0}}
FAN, FAN_COPIES, SOUP = 1, (1, 2, 3), 4          # mesh ids in _scene: the pole fan is not the first mesh (its vertices do not start at 0) and is flattened three times


@functools.lru_cache(maxsize=None)
def _case(mrt):
    sc = _scene(mrt, SIZE, SEED)
    rays = _rays(np.random.default_rng(100 + SEED), 4000)
    rays.setflags(write=False)
    meshes = mrt.flatten_scene(sc, share=True)
    assert [m[4] for m in meshes] == [-1, -1, 1, 1, -1, -1]
    nv = [len(meshes[k][0]) for k in (FAN, SOUP)]
    assert all(n % 64 != 0 and n % 256 != 0 for n in nv), nv          # the ingest kernel's last wave and last workgroup are partial
    return sc, rays, meshes


def _moved(pos, step):
    pos = np.asarray(pos, np.float32)
    return (pos + np.float32(0.05) * np.sin(7.0 * pos[:, [2, 0, 1]] + step)).astype(np.float32)


def _tilted(nrm, step):
    t = np.asarray(nrm, np.float32) + np.float32(0.2 * (step + 1)) * np.array([1, 0, 0], np.float32)
    return (t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), 1e-6)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_records(a, b, what=""):
    for f in FIELDS:
        bad = np.flatnonzero(_bits(a[f]) != _bits(b[f]))
        assert len(bad) == 0, f"{what}{f}: {len(bad)} records differ, first {bad[0]}: {a[bad[0]]} against {b[bad[0]]}"


def _device_records_equal(t, host, what=""):
    g = t.cpu().numpy().view(np.uint32)
    for c, f in enumerate(FIELDS):
        assert np.array_equal(g[:, c], _bits(host[f])), what + f


def _canonical(ds):
    """The 8-wide layout read in the order a walk finds it: the 18 words of every node that do not depend on where the builder put its children and packets (all but
    child_base and tri_base), depth first in slot order, and the packets of every leaf slot behind each other.  Two builds of one scene number the nodes of a level in
    the order their parents' waves reserved them (tests/test_build_sizes.py), so the arrays of two scenes are compared in this form: every bit of every node and packet,
    and the links between them, up to that relabelling."""
    wn, wp = ds.read_layout("wnodes"), ds.read_layout("wpackets")
    keep = [0, 1, 2, 3] + list(range(6, 20))
    nodes, packets, stack, seen = [], [], [0], 0
    while stack:
        i = stack.pop()
        seen += 1
        assert seen <= len(wn), "a cycle in the tree"
        row = wn[i]
        nodes.append(row[keep])
        imask, cbase, tbase = int(row[3]) >> 24, int(row[4]), int(row[5])
        meta = row[6:8].view(np.uint8)
        kids = []
        for sl in range(8):
            if (imask >> sl) & 1:
                kids.append(cbase + bin(imask & ((1 << sl) - 1)).count("1"))
            else:
                cnt, off = int(meta[sl]) >> 5, int(meta[sl]) & 31
                packets.extend(wp[tbase + off + k] for k in range(cnt))
        stack.extend(reversed(kids))
    assert seen == len(wn)
    return np.array(nodes), np.array(packets)


def _same_layout(a, b, rope=False):
    assert a.stats.wide_layout == b.stats.wide_layout
    if rope:          # the rope layout beside the 8-wide one or alone: every word of every node (boxes, links, escapes) and packet
        for part in ("rope_nodes", "rope_packets"):
            pa, pb = a.read_layout(part), b.read_layout(part)
            assert pa.shape == pb.shape and len(pa) > 0 and np.array_equal(_bits(pa), _bits(pb)), part
    if a.stats.wide_layout:
        (na, pa), (nb, pb) = _canonical(a), _canonical(b)
        assert na.shape == nb.shape and len(na) > 0 and np.array_equal(na, nb), "wnodes"
        assert pa.shape == pb.shape and len(pa) > 0 and np.array_equal(pa, pb), "wpackets"


def _links(ds):
    """what a refit must not touch in the 8-wide nodes: child_base and tri_base, the internal mask and the per-slot packet counts and offsets (None without the layout)"""
    if not ds.stats.wide_layout:
        return None
    wn = ds.read_layout("wnodes")
    return np.column_stack([wn[:, 4], wn[:, 5], wn[:, 3] >> 24, wn[:, 6], wn[:, 7]])


def _same_stats(a, b):
    sa, sb = a.stats, b.stats
    va, vb = (sa.refits, sa.leaf_growth, sa.wide_cost, sa.sah_cost), (sb.refits, sb.leaf_growth, sb.wide_cost, sb.sah_cost)          # (ctypes floats: exact float32 values)
    assert va == vb and not any(math.isnan(x) for x in vb), (va, vb)
    assert sb.build_ms > 0


def _oracle(mrt, orc, sc, meshes, new):
    """the oracle's scene with `new` = {mesh id: (positions, normals)} in place of those meshes' arrays (an instance takes its source's)"""
    out = []
    for k, (pos, nrm, xf, subs, source) in enumerate(meshes):
        g = source if source >= 0 else k
        p, n = new.get(g, (pos, nrm))
        out.append((p, n, xf, subs))
    return orc.OracleScene(out, sc.lights)


def _dev(gpu_ctx):
    import torch
    return torch.device("cuda", gpu_ctx.device)


def _t(a, gpu_ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(_dev(gpu_ctx))


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_parity_with_the_host_path(mrt, orc, gpu_ctx, layout):
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    ra = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, scene_options=LAYOUTS[layout]); rb = mrt.Renderer(SIZE, sc, ctx=gpu_ctx, scene_options=LAYOUTS[layout])
    a, b = ra.device_scene, rb.device_scene
    assert a.stats.wide_layout == (0 if layout == "rope" else 1)
    d_rays = _t(r, gpu_ctx)
    before = a.intersect_closest(r)
    sah_built = b.stats.sah_cost
    links = _links(b)
    assert (links is None) == (layout == "rope")
    for step in range(2):          # the second step chains leaf_growth on the first
        pos, nrm = _moved(meshes[FAN][0], step), _tilted(meshes[FAN][1], step)
        a.update_mesh(FAN, pos, nrm); a.commit()
        d_pos, d_nrm = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
        b.update_mesh_device(FAN, d_pos, d_nrm); b.refit_device()
        gc = b.intersect_closest_device(d_rays); ga = b.intersect_any_device(d_rays)          # torch's current stream: behind the refit
        torch.cuda.synchronize()
        assert a.refits == step + 1 and b.refits == step + 1
        _same_layout(a, b, rope=layout != "wide")
        assert links is None or np.array_equal(_links(b), links), "a refit moves boxes, never the links between the nodes and to the packets"
        hc, ha = a.intersect_closest(r), a.intersect_any(r)
        _same_records(b.intersect_closest(r), hc, f"step {step} host entry ")
        assert np.array_equal(b.intersect_any(r), ha)
        _device_records_equal(gc, hc, f"step {step} device entry ")
        assert np.array_equal(ga.cpu().numpy(), ha)
        assert (_bits(hc["distance"]) != _bits(before["distance"])).sum() > 50, "the deformation must change some answers"
        oc = _oracle(mrt, orc, sc, meshes, {FAN: (pos, nrm)}).intersect_closest(r, brute=True)
        _same_records(hc, oc, f"step {step} oracle ")
        for rr in (ra, rb):
            rr.frameIndex = 0; rr.reset_stats(); rr.draw(3, wait=True)
        assert np.array_equal(_bits(ra.accumulation()), _bits(rb.accumulation())), "the two paths must render the same image"
        assert (ra.stats.closest_rays, ra.stats.shadow_rays) == (rb.stats.closest_rays, rb.stats.shadow_rays)
        _same_stats(a, b)
        assert b.stats.refits == step + 1
        if layout != "rope":          # ... and equal to the recount from the layout the scene dumps (tests/tree_stats_reference.py; test_tree_stats.py has the other figures)
            cost, _ = T.scene_wide_cost(A.layout_of(b))
            assert T.ulps32(b.stats.wide_cost, cost.emu) <= 2 and abs(float(b.stats.wide_cost) - cost.exact) <= cost.bound, (b.stats.wide_cost, cost)
            assert F32(b.stats.sah_cost) == F32(sah_built) * (F32(b.stats.wide_cost) / F32(b.stats.wide_cost_built))
    assert b.device_updates_rejected == 0
    ra.close(); rb.close()


class _Hand:
    """stands in for Model: one hand-made mesh (or an earlier one's arrays again: a flattened instance of it)"""
    def __init__(self, mrt, name, pos, nrm, subs, position, scale):
        self.name = name
        self.meshes = [mrt.Mesh(name, pos, nrm, subs, position, (0.0, 0.0, 0.0), scale)]


def _sphere_scene(mrt):
    """plane.obj under sphere.obj twice; the sphere's triangles cut into three submeshes"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            pos, nrm, subs = mrt.load_obj(mrt.scene.find_resource("sphere"))
            idx = np.vstack([s.indices for s in subs])
            cut = [0, len(idx) // 3 + 1, 2 * len(idx) // 3 + 2, len(idx)]
            parts = [mrt.Submesh(f"part{k}", idx[cut[k]:cut[k + 1]], _material(mrt, c)) for k, c in enumerate([(0.8, 0.2, 0.2), (0.2, 0.8, 0.2), (0.2, 0.2, 0.8)])]
            first = _Hand(mrt, "sphere", pos, nrm, parts, [-0.6, 0.5, 0.3], 0.5)
            m = first.meshes[0]
            self.models = [mrt.Model(name="plane", position=[0, 0, 0], scale=10), first, _Hand(mrt, "sphere", m.positions, m.normals, m.submeshes, [0.7, 0.8, -0.2], 0.8)]
    return S(SIZE)


@pytest.mark.parametrize("stride", [12, 16, 32])
def test_strided_rows_submeshes_and_a_flattened_instance(mrt, orc, gpu_ctx, stride):
    import torch
    sc = _sphere_scene(mrt)
    meshes = mrt.flatten_scene(sc, share=True)
    assert [m[4] for m in meshes] == [-1, -1, 1] and len(meshes[1][3]) == 3
    n = len(meshes[1][0])
    assert n % 64 != 0
    pos, nrm = _moved(meshes[1][0], 0.5), _tilted(meshes[1][1], 0)
    a, b = mrt.DeviceScene(gpu_ctx, sc), mrt.DeviceScene(gpu_ctx, sc)
    a.update_mesh(1, pos, nrm); a.commit()
    dev = _dev(gpu_ctx)
    if stride == 12:
        d_pos, d_nrm = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    elif stride == 16:
        wp = torch.full((n, 4), float("nan"), device=dev); wn = torch.full((n, 4), float("inf"), device=dev)          # the padding column is never read
        wp[:, :3] = _t(pos, gpu_ctx); wn[:, :3] = _t(nrm, gpu_ctx)
        d_pos, d_nrm = wp[:, :3], wn[:, :3]
    else:
        w = torch.full((n, 8), float("nan"), device=dev)          # positions and normals interleaved in one tensor
        w[:, 0:3] = _t(pos, gpu_ctx); w[:, 4:7] = _t(nrm, gpu_ctx)
        d_pos, d_nrm = w[:, 0:3], w[:, 4:7]
    assert d_pos.stride(0) * 4 == stride and d_nrm.stride(0) * 4 == stride
    b.update_mesh_device(1, d_pos, d_nrm); b.refit_device()
    torch.cuda.synchronize()
    assert b.device_updates_rejected == 0 and b.refits == 1
    _same_layout(a, b)
    rng = np.random.default_rng(5)
    r = _rays(rng, 3000)
    hc = a.intersect_closest(r)
    assert len(set(hc["instance_id"][hc["type"] == 1].tolist())) == 3 and len(set(hc["geometry_id"][hc["instance_id"] == 2].tolist())) == 3          # both spheres, every submesh
    _same_records(b.intersect_closest(r), hc)
    assert np.array_equal(b.intersect_any(r), a.intersect_any(r))
    _same_records(hc, _oracle(mrt, orc, sc, meshes, {1: (pos, nrm)}).intersect_closest(r, brute=True), "oracle ")
    _same_stats(a, b)
    a.close(); b.close()


def test_two_meshes_before_one_refit(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    a, b = mrt.DeviceScene(gpu_ctx, sc), mrt.DeviceScene(gpu_ctx, sc)
    new = {FAN: (_moved(meshes[FAN][0], 0), _tilted(meshes[FAN][1], 0)), SOUP: (_moved(meshes[SOUP][0], 2), _tilted(meshes[SOUP][1], 1))}
    for k, (p, n) in new.items(): a.update_mesh(k, p, n)
    a.commit()
    keep = [(_t(p, gpu_ctx), _t(n, gpu_ctx)) for p, n in new.values()]
    for k, (p, n) in zip(new, keep): b.update_mesh_device(k, p, n)
    b.refit_device()
    torch.cuda.synchronize()
    assert a.refits == 1 and b.refits == 1
    _same_layout(a, b)
    hc = a.intersect_closest(r)
    _same_records(b.intersect_closest(r), hc)
    _same_records(hc, _oracle(mrt, orc, sc, meshes, new).intersect_closest(r, brute=True), "oracle ")
    _same_stats(a, b)
    a.close(); b.close()


def test_stream_order(mrt, orc, gpu_ctx):
    """a torch kernel that makes the vertices, the update, the refit and a query on ONE stream with a single synchronise at the end — on a side stream and on the null stream"""
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    dev = _dev(gpu_ctx)
    d_rays = _t(r, gpu_ctx)
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream not in (0, gpu_ctx.stream)
    for step, (stream, handle) in enumerate(((side, None), (torch.cuda.default_stream(dev), 0))):
        pos, nrm = _moved(meshes[FAN][0], step), _tilted(meshes[FAN][1], step)
        a, b = mrt.DeviceScene(gpu_ctx, sc), mrt.DeviceScene(gpu_ctx, sc)
        a.update_mesh(FAN, pos, nrm); a.commit()
        src_p, src_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
        d_pos = torch.zeros_like(src_p); d_nrm = torch.zeros_like(src_n)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            big = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)          # the stream is busy when the vertices are made
            z = torch.nan_to_num(big[0, 0] * 0.0)
            d_pos.copy_(src_p * 2.0 * 0.5 + z); d_nrm.copy_(src_n * 2.0 * 0.5 + z)          # exact; the vertices exist only once this stream reaches them
            b.update_mesh_device(FAN, d_pos, d_nrm, stream=handle)
            b.refit_device(stream=handle)
            gc = b.intersect_closest_device(d_rays, stream=handle)
        stream.synchronize()
        _device_records_equal(gc, a.intersect_closest(r), f"stream {handle} ")
        a.close(); b.close()


def test_a_nan_or_an_infinity_leaves_the_scene_as_it_was(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    b = mrt.DeviceScene(gpu_ctx, sc)
    before_c, before_a = b.intersect_closest(r), b.intersect_any(r)
    pos, nrm = _moved(meshes[SOUP][0], 0), _tilted(meshes[SOUP][1], 0)
    assert len(pos) > 256          # the bad value sits in the last vertex, many waves behind the first
    bad_pos = pos.copy(); bad_pos[-1, 1] = np.nan
    bad_nrm = nrm.copy(); bad_nrm[-1, 2] = np.inf
    count = b.device_updates_rejected
    for p, n in ((bad_pos, nrm), (pos, bad_nrm)):
        d_p, d_n = _t(p, gpu_ctx), _t(n, gpu_ctx)
        b.update_mesh_device(SOUP, d_p, d_n); b.refit_device()
        torch.cuda.synchronize()
        _same_records(b.intersect_closest(r), before_c, "after a refused update ")
        assert np.array_equal(b.intersect_any(r), before_a)
        count += 1
        assert b.device_updates_rejected == count
    d_p, d_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    b.update_mesh_device(SOUP, d_p, d_n); b.refit_device()
    torch.cuda.synchronize()
    assert b.device_updates_rejected == count
    a = mrt.DeviceScene(gpu_ctx, sc)
    a.update_mesh(SOUP, pos, nrm); a.commit()
    hc = a.intersect_closest(r)
    assert (_bits(hc["distance"]) != _bits(before_c["distance"])).sum() > 50
    _same_records(b.intersect_closest(r), hc, "a good update after the refused ones ")
    a.close(); b.close()


def test_nothing_is_allocated_after_the_first_call(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    b = mrt.DeviceScene(gpu_ctx, sc)
    steps = [(_t(_moved(meshes[FAN][0], s), gpu_ctx), _t(_tilted(meshes[FAN][1], s), gpu_ctx)) for s in range(5)]
    free = []
    for p, n in steps:
        b.update_mesh_device(FAN, p, n); b.refit_device()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(_dev(gpu_ctx))[0])
    assert len(set(free[1:])) == 1 and free[1] == free[0], free          # (the first call made the workspace before it was measured)
    assert b.refits == 5 and b.stats.refits == 5
    b.close()


def test_a_later_build_takes_the_vertices_the_device_holds(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    pos, nrm = _moved(meshes[FAN][0], 1), _tilted(meshes[FAN][1], 1)
    xf = mrt.make_transform([0.3, 0.2, 0.1], [0.0, 0.4, 0.0], 0.9)
    b = mrt.DeviceScene(gpu_ctx, sc)
    d_p, d_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    b.update_mesh_device(FAN, d_p, d_n); b.refit_device()
    torch.cuda.synchronize()
    b.set_instance_transform(SOUP, xf.reshape(16)); b.commit()
    assert b.refits == 0, "a transform change builds"
    fresh_sc = _scene(mrt, SIZE, SEED)
    ms = fresh_sc.meshes
    for k in FAN_COPIES: ms[k].positions, ms[k].normals = pos, nrm          # (the same arrays: still one geometry, flattened three times)
    ms[SOUP].transform = xf
    fresh = mrt.DeviceScene(gpu_ctx, fresh_sc)
    hc = fresh.intersect_closest(r)
    _same_records(b.intersect_closest(r), hc)
    assert np.array_equal(b.intersect_any(r), fresh.intersect_any(r))
    _same_layout(fresh, b)
    # and an update that was never refitted on the device is not lost either: the commit of another mesh's host update refits both
    pos2 = _moved(meshes[FAN][0], 3)
    d_p2 = _t(pos2, gpu_ctx)
    b.update_mesh_device(FAN, d_p2, d_n)
    torch.cuda.synchronize()
    soup = _moved(meshes[SOUP][0], 1)
    b.update_mesh(SOUP, soup, meshes[SOUP][1]); b.commit()
    assert b.refits == 1
    fresh.update_mesh(FAN, pos2, nrm); fresh.update_mesh(SOUP, soup, meshes[SOUP][1]); fresh.commit()
    assert fresh.refits == 1
    _same_records(b.intersect_closest(r), fresh.intersect_closest(r), "host refit after a device update ")
    _same_layout(fresh, b)
    fresh.close(); b.close()


@pytest.mark.parametrize("added", ["instance", "mesh"])
def test_a_mesh_added_after_a_device_update_does_not_lose_it(mrt, orc, gpu_ctx, added):
    """the scene grows between the device update and the commit (meshes are only appended): the build that follows still starts from the vertices the device holds —
    for the deformed mesh, for its flattened instances and for an instance of it added just now"""
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    lib = mrt.lib
    pos, nrm = _moved(meshes[FAN][0], 2), _tilted(meshes[FAN][1], 1)
    xf = np.ascontiguousarray(mrt.make_transform([-0.4, 0.6, 0.5], [0.3, 0.0, 0.2], 0.7), np.float32).reshape(16)
    tri = (np.array([[-1.0, 0.2, 0.0], [1.0, 0.2, 0.0], [0.0, 1.8, 0.5]], np.float32), np.array([[0, 0, 1]] * 3, np.float32), np.array([0, 1, 2], np.uint32))

    def grow(ds):
        mid = C.c_int32(-1)
        if added == "instance":
            assert lib.mrt_scene_add_instance(ds.handle, FAN, xf.ctypes.data_as(C.c_void_p), C.byref(mid)) == 0
        else:
            assert lib.mrt_scene_add_mesh(ds.handle, tri[0].ctypes.data_as(C.c_void_p), 12, tri[1].ctypes.data_as(C.c_void_p), 12, 3, xf.ctypes.data_as(C.c_void_p), C.byref(mid)) == 0
            assert lib.mrt_mesh_add_submesh(ds.handle, mid.value, tri[2].ctypes.data_as(C.c_void_p), 1, C.byref(_material(mrt, (0.5, 0.5, 0.5))), None) == 0
        assert mid.value == len(meshes)
        ds.commit()

    b = mrt.DeviceScene(gpu_ctx, sc)
    before = b.intersect_closest(r)
    d_p, d_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    b.update_mesh_device(FAN, d_p, d_n); b.refit_device()          # no synchronise: the commit below has to wait for the stream's vertices itself
    grow(b)
    assert b.refits == 0 and b.stats.instances == len(meshes) + 1, "an added mesh builds"
    fresh_sc = _scene(mrt, SIZE, SEED)
    for k in FAN_COPIES: fresh_sc.meshes[k].positions, fresh_sc.meshes[k].normals = pos, nrm
    fresh = mrt.DeviceScene(gpu_ctx, fresh_sc)
    grow(fresh)
    hc = fresh.intersect_closest(r)
    assert (_bits(hc["distance"]) != _bits(before["distance"])).sum() > 50
    assert (hc["instance_id"][hc["type"] == 1] == len(meshes)).sum() > 0, "some rays must meet what was added"
    _same_records(b.intersect_closest(r), hc)
    assert np.array_equal(b.intersect_any(r), fresh.intersect_any(r))
    _same_layout(fresh, b)
    # the workspace went with the build; the next device update makes one for the grown scene
    pos2 = _moved(meshes[FAN][0], 4)
    d_p2 = _t(pos2, gpu_ctx)
    b.update_mesh_device(FAN, d_p2, d_n); b.refit_device()
    torch.cuda.synchronize()
    fresh.update_mesh(FAN, pos2, nrm); fresh.commit()
    assert b.refits == 1 and fresh.refits == 1
    _same_records(b.intersect_closest(r), fresh.intersect_closest(r), "a device refit of the grown scene ")
    fresh.close(); b.close()


def test_a_commit_after_an_update_that_was_never_refitted_refits(mrt, orc, gpu_ctx):
    """update_mesh_device with no refit_device behind it, then a commit with nothing else changed: a vertex change like update_mesh's, so the commit keeps the tree"""
    sc, rays, meshes = _case(mrt)
    r = np.array(rays)
    pos, nrm = _moved(meshes[SOUP][0], 3), _tilted(meshes[SOUP][1], 0)
    a, b = mrt.DeviceScene(gpu_ctx, sc), mrt.DeviceScene(gpu_ctx, sc)
    links = _links(b)
    a.update_mesh(SOUP, pos, nrm); a.commit()
    d_p, d_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    b.update_mesh_device(SOUP, d_p, d_n)          # no refit, no synchronise
    b.commit()
    assert a.refits == 1 and b.refits == 1
    assert np.array_equal(_links(b), links)
    _same_layout(a, b)
    _same_records(b.intersect_closest(r), a.intersect_closest(r))
    _same_stats(a, b)
    a.close(); b.close()


def test_refusals(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    r = np.array(rays[:512])
    pos, nrm = _moved(meshes[FAN][0], 0), np.asarray(meshes[FAN][1], np.float32)
    d_p, d_n = _t(pos, gpu_ctx), _t(nrm, gpu_ctx)
    n = len(pos)
    lib = mrt.lib

    def last():
        return lib.mrt_last_error().decode()

    def raw(ds, mesh, ps=12, ns=12, count=n, p=d_p, q=d_n):
        return lib.mrt_scene_update_mesh_device(ds.handle, mesh, C.c_void_p(p.data_ptr()), ps, C.c_void_p(q.data_ptr()), ns, count, None)

    two = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    assert raw(two, FAN) == 7 and "mrt_scene_update_mesh_device" in last()          # MRT_ERR_UNSUPPORTED
    assert lib.mrt_scene_refit_device(two.handle, None) == 7 and "mrt_scene_refit_device" in last()
    two.close()
    norefit = mrt.DeviceScene(gpu_ctx, sc, {"refit": 0})
    assert raw(norefit, FAN) == 7 and "mrt_scene_update_mesh_device" in last()
    norefit.close()
    ds = mrt.DeviceScene(gpu_ctx, sc)
    before = ds.intersect_closest(r)
    for rc, args in ((1, dict(count=n - 1)), (1, dict(ps=10)), (1, dict(ns=14)), (1, dict(ps=8)), (1, dict(mesh=2)), (1, dict(mesh=99)), (1, dict(mesh=-1))):
        kw = dict(mesh=FAN); kw.update(args)
        assert raw(ds, **kw) == rc, args          # MRT_ERR_INVALID_ARGUMENT
        assert "mrt_scene_update_mesh_device" in last(), last()
    assert lib.mrt_scene_update_mesh_device(ds.handle, FAN, None, 12, C.c_void_p(d_n.data_ptr()), 12, n, None) == 1 and "mrt_scene_update_mesh_device" in last()
    for bad in (d_p.cpu(), d_p.double(), d_p.t().contiguous().t(), d_p[:, :2], pos):
        with pytest.raises((ValueError, TypeError)):
            ds.update_mesh_device(FAN, bad, d_n)
        with pytest.raises((ValueError, TypeError)):
            ds.update_mesh_device(FAN, d_p, bad)
    with pytest.raises(mrt.MRTError) as e:
        ds.update_mesh_device(FAN, d_p, d_n[:-1])
    assert e.value.code == 1
    torch.cuda.synchronize()
    _same_records(ds.intersect_closest(r), before, "after the refused calls ")
    assert ds.refits == 0 and ds.device_updates_rejected == 0
    ds.update_mesh(FAN, pos, nrm)          # host-side changes pending
    assert raw(ds, FAN) == 5 and "mrt_scene_update_mesh_device" in last()          # MRT_ERR_STATE
    assert lib.mrt_scene_refit_device(ds.handle, None) == 5 and "mrt_scene_refit_device" in last()
    ds.commit()
    ds.update_mesh_device(FAN, d_p, d_n); ds.refit_device()
    torch.cuda.synchronize()
    assert ds.refits == 2
    ds.close()
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0          # never committed
    assert lib.mrt_scene_refit_device(h, None) == 5 and "mrt_scene_refit_device" in last()
    assert lib.mrt_scene_update_mesh_device(h, 0, C.c_void_p(d_p.data_ptr()), 12, C.c_void_p(d_n.data_ptr()), 12, n, None) == 5 and "mrt_scene_update_mesh_device" in last()
    assert lib.mrt_scene_destroy(h) == 0


def test_the_refitted_tree_encloses_the_deformed_triangles(mrt, orc, gpu_ctx):
    import torch
    sc, rays, meshes = _case(mrt)
    b = mrt.DeviceScene(gpu_ctx, sc)
    new = {FAN: (_moved(meshes[FAN][0], 2), _tilted(meshes[FAN][1], 0)), SOUP: (_moved(meshes[SOUP][0], 1), _tilted(meshes[SOUP][1], 0))}
    keep = [(_t(p, gpu_ctx), _t(n, gpu_ctx)) for p, n in new.values()]
    for k, (p, n) in zip(new, keep): b.update_mesh_device(k, p, n)
    b.refit_device()
    torch.cuda.synchronize()
    lay = A.layout_of(b)
    rep = A.audit(lay, presplit=True, num_tris=sc.triangleCount)
    rep.check()
    # the packets hold the DEFORMED triangles: world-space vertices of every instance, float64 from the new float32 positions, within float32 rounding of the packets'
    V, gid = A.decode_packets(lay["wpackets"])
    world, base = {}, 0
    for k, (pos, nrm, xf, subs, source) in enumerate(meshes):
        g = source if source >= 0 else k
        p = np.asarray(new.get(g, (pos, nrm))[0], np.float64)
        M = np.asarray(xf, np.float64).reshape(4, 4)          # [col][row]
        w = p @ M[:3, :3] + M[3, :3]
        for idx, _ in subs:
            idx = np.asarray(idx, np.int64).reshape(-1, 3)
            for t in range(len(idx)): world[base + t] = w[idx[t]]
            base += len(idx)
    assert base == sc.triangleCount
    want = np.stack([world[int(g)] for g in gid])
    assert np.abs(V - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    b.close()
