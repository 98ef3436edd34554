"""Stream-ordered ray queries on device buffers (DeviceScene.intersect_closest_device / intersect_any_device): rays that live in a torch tensor on the GPU, results in
a torch tensor, both launches on the caller's stream.  Every field of every record must have the bits the host entries (intersect_closest / intersect_any) return for the
same rays and scene — on the flattened 8-wide layout, on a two-level scene and on a scene without the 8-wide layout, for any min_distance — and on the min_distance == 0
subset also the oracle's.  The scene is test_fuzz_geometry's hostile one (pole fans, coincident triangles, slivers)."""
import functools

import numpy as np
import pytest

from test_fuzz_geometry import _rays, _scene

pytestmark = pytest.mark.gpu

SIZE = (96, 64)
SEED = 1
FIELDS = ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v")
# min_distance values of the quarter of the rays that get one.  The rays start about 4 units in front of the scene and hit it 2 .. 6 units away: 1e-3 changes nothing
# (the walk must still carry it), 3.0 and 4.0 cut the nearest surfaces away for a good part of the rays (the precondition below counts them).
TMINS = (1e-3, 3.0, 4.0)
LAYOUTS = {"flat": None, "two_level": {"instancing": 1}, "rope": {"wide": 0}}


@functools.lru_cache(maxsize=None)
def _case(mrt, orc, two_level):
    """scene, oracle scene, the 20 000 rays and the oracle's answers (computed once per level form, never modified)"""
    sc = _scene(mrt, SIZE, SEED)
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=two_level), sc.lights, instancing=two_level)
    base = _rays(np.random.default_rng(100 + SEED), 20000)
    o0 = osc.intersect_closest(base)
    rays = base.copy()
    k = np.arange(len(rays))
    q_min = k % 4 == 1
    rays[q_min, 3] = np.asarray(TMINS, np.float32)[(k[q_min] // 4) % 3]
    q_max = k % 4 == 2
    near = np.nextafter(o0["distance"], np.float32(np.inf)).astype(np.float32)          # one float beyond the hit: the hit is still inside the ray
    at_hit = q_max & ((k // 4) % 2 == 1) & (o0["type"] == 1)
    rays[q_max, 7] = 2.5
    rays[at_hit, 7] = near[at_hit]
    for a in (rays, base): a.setflags(write=False)
    return sc, osc, rays, o0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_records_equal(t, host, what=""):
    """t: torch.int32 (n, 8) from the device entry; host: the structured array of the host entry — every field as uint32 bit patterns"""
    g = t.cpu().numpy().view(np.uint32)
    for c, f in enumerate(FIELDS):
        bad = np.flatnonzero(g[:, c] != _bits(host[f]))
        assert len(bad) == 0, f"{what}{f}: {len(bad)} records differ, first {bad[0]}: device {g[bad[0]].tolist()} host {host[bad[0]]}"
    assert (g[:, 7] == 0).all(), "_pad must be written as 0"


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_parity_with_host_entry_and_oracle(mrt, orc, gpu_ctx, layout):
    import torch
    two_level = layout == "two_level"
    sc, osc, rays, o0 = _case(mrt, orc, two_level)
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    assert ds.stats.wide_layout == (0 if layout == "rope" else 1)
    hc = ds.intersect_closest(rays); ha = ds.intersect_any(rays)
    # preconditions: the test cannot pass on misses, or on min_distance values that change nothing
    assert (o0["type"] == 1).mean() > 0.6
    with_min = rays[:, 3] > 0
    zero_min = np.array(rays); zero_min[:, 3] = 0
    h0 = ds.intersect_closest(zero_min)
    changed = (_bits(hc["distance"]) != _bits(h0["distance"])) | (hc["primitive_id"] != h0["primitive_id"])
    assert (changed & with_min).sum() >= 1000, (changed & with_min).sum()
    d_rays = torch.from_numpy(np.array(rays)).to(f"cuda:{gpu_ctx.device}")
    gc = ds.intersect_closest_device(d_rays)
    ga = ds.intersect_any_device(d_rays)
    torch.cuda.synchronize()
    assert gc.dtype == torch.int32 and tuple(gc.shape) == (len(rays), 8) and ga.dtype == torch.int32 and tuple(ga.shape) == (len(rays),)
    _assert_records_equal(gc, hc, layout + " ")
    assert np.array_equal(ga.cpu().numpy(), ha)
    # the min_distance == 0 subset against the oracle, as the existing tests compare
    z = np.flatnonzero(~with_min)
    oc = osc.intersect_closest(np.array(rays[z])); oa = osc.intersect_any(np.array(rays[z]))
    g = gc.cpu().numpy()
    u = mrt.unpack_intersections(gc)
    for c, f in enumerate(FIELDS):
        assert np.array_equal(g[z, c].view(np.uint32), _bits(oc[f])), f
        assert np.array_equal(_bits(u[f].cpu().numpy()), g[:, c].view(np.uint32)), f          # unpack_intersections: views of the same words
    assert u["distance"].dtype == torch.float32 and u["u"].dtype == torch.float32 and u["type"].dtype == torch.int32
    assert np.array_equal(ga.cpu().numpy()[z], oa)
    ds.close()


@pytest.mark.parametrize("layout", ["flat", "two_level"])
def test_edges_of_the_launch_shape(mrt, orc, gpu_ctx, layout):
    """one lane, a wave's 64-ray batch +- 1, a wave's 256-ray range +- 1, two ranges + 1; all rays on the stream kernel, all on the lane kernel, and alternating
    (inert and live rays in one refill batch); every record must be written"""
    import torch
    sc, _, rays, _ = _case(mrt, orc, layout == "two_level")
    ds = mrt.DeviceScene(gpu_ctx, sc, LAYOUTS[layout])
    dev = f"cuda:{gpu_ctx.device}"
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        for mode in ("zero", "positive", "alternating"):
            r = np.array(rays[:n]); r[:, 7] = np.inf
            r[:, 3] = {"zero": 0.0, "positive": 3.0, "alternating": np.where(np.arange(n) % 2 == 0, 0.0, 3.0)}[mode]
            d_rays = torch.from_numpy(r).to(dev)
            oc = torch.full((n, 8), 0x7F7F7F7F, dtype=torch.int32, device=dev); oa = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
            assert ds.intersect_closest_device(d_rays, out=oc) is oc and ds.intersect_any_device(d_rays, out=oa) is oa
            torch.cuda.synchronize()
            assert not (oc == 0x7F7F7F7F).any().item() and not (oa == 0x7F7F7F7F).any().item(), (n, mode, "a record was not written")
            _assert_records_equal(oc, ds.intersect_closest(r), f"n={n} {mode} ")
            assert np.array_equal(oa.cpu().numpy(), ds.intersect_any(r)), (n, mode)
    e = ds.intersect_closest_device(torch.empty((0, 8), dtype=torch.float32, device=dev))
    assert tuple(e.shape) == (0, 8) and tuple(ds.intersect_any_device(torch.empty((0, 8), dtype=torch.float32, device=dev)).shape) == (0,)
    ds.close()


def test_stream_order(mrt, orc, gpu_ctx):
    """rays built by torch ops, the query, and a torch reduction of its result on ONE stream with a single synchronise at the end — on a side stream that is neither the
    null stream nor the context's, and on the null stream (handle 0, taken literally)"""
    import torch
    sc, _, rays, _ = _case(mrt, orc, False)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    dev = torch.device("cuda", gpu_ctx.device)
    r = np.array(rays[:8192])
    hc = ds.intersect_closest(r); ha = ds.intersect_any(r)
    want = (int((hc["type"] == 1).sum()), int(hc["primitive_id"].astype(np.int64).sum()), int(ha.sum()))
    src = torch.from_numpy(r).to(dev); torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream not in (0, gpu_ctx.stream) and gpu_ctx.stream != 0
    for stream, handle in ((side, None), (torch.cuda.default_stream(dev), 0)):
        with torch.cuda.stream(stream):
            big = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)          # the stream is busy when the rays are made
            d_rays = (src * 2.0 + big[0, 0] * 0.0) * 0.5          # exact: x * 2 * 0.5 (+ 0 or NaN-free 0): the rays exist only once this stream reaches them
            d_rays = torch.where(torch.isnan(d_rays), src, d_rays).contiguous()
            gc = ds.intersect_closest_device(d_rays, stream=handle)          # None: torch's current stream = the side stream; 0: the null stream
            ga = ds.intersect_any_device(d_rays, stream=handle)
            got = torch.stack([(gc[:, 0] == 1).sum(), gc[:, 4].to(torch.int64).sum(), ga.to(torch.int64).sum()])
        stream.synchronize()
        assert tuple(int(x) for x in got.cpu()) == want
    ds.close()


def test_refusals(mrt, orc, gpu_ctx):
    import torch
    sc, _, rays, _ = _case(mrt, orc, False)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    dev = f"cuda:{gpu_ctx.device}"
    good = torch.from_numpy(np.array(rays[:128])).to(dev)
    for f in (ds.intersect_closest_device, ds.intersect_any_device):
        for bad in (good.cpu(), good.double(), good[::2], good.t().contiguous().t(), good[:, :7].contiguous(), np.array(rays[:128])):
            with pytest.raises((ValueError, TypeError)):
                f(bad)
        with pytest.raises((ValueError, TypeError)):
            f(good, out=torch.empty((128, 8), dtype=torch.float32, device=dev))
    xf = np.eye(4, dtype=np.float32).T.reshape(16)
    ds.set_instance_transform(0, xf)          # not committed any more
    for f in (ds.intersect_closest_device, ds.intersect_any_device):
        with pytest.raises(mrt.MRTError) as e:
            f(good)
        assert e.value.code == 5          # MRT_ERR_STATE
    ds.close()


def test_after_a_refit(mrt, orc, gpu_ctx):
    import torch
    sc, _, rays, _ = _case(mrt, orc, False)
    ds = mrt.DeviceScene(gpu_ctx, sc)
    meshes = mrt.flatten_scene(sc, share=True)
    pos, nrm = np.asarray(meshes[1][0], np.float32), np.asarray(meshes[1][1], np.float32)          # the first pole fan (its flattened copies follow it)
    moved = (pos + np.float32(0.05) * np.sin(7.0 * pos[:, [2, 0, 1]])).astype(np.float32)
    ds.update_mesh(1, moved, nrm); ds.commit()
    assert ds.refits == 1
    r = np.array(rays[:5000])
    d_rays = torch.from_numpy(r).to(f"cuda:{gpu_ctx.device}")
    gc = ds.intersect_closest_device(d_rays); ga = ds.intersect_any_device(d_rays)
    torch.cuda.synchronize()
    _assert_records_equal(gc, ds.intersect_closest(r))
    assert np.array_equal(ga.cpu().numpy(), ds.intersect_any(r))
    ds.close()


def test_after_a_transform_change(mrt, orc, gpu_ctx):
    import torch
    sc, _, rays, _ = _case(mrt, orc, True)
    ds = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    r = np.array(rays[:5000])
    before = ds.intersect_closest(r)
    ds.set_instance_transform(2, mrt.make_transform([-0.4, 1.1, 0.6], [0.3, 1.0, -0.2], 0.8).reshape(16)); ds.commit()          # the second pole fan, an instance of the first
    host = ds.intersect_closest(r)
    assert (_bits(host["distance"]) != _bits(before["distance"])).sum() > 50, "the moved instance must change some answers"
    d_rays = torch.from_numpy(r).to(f"cuda:{gpu_ctx.device}")
    gc = ds.intersect_closest_device(d_rays); ga = ds.intersect_any_device(d_rays)
    torch.cuda.synchronize()
    _assert_records_equal(gc, host)
    assert np.array_equal(ga.cpu().numpy(), ds.intersect_any(r))
    ds.close()


def test_image_unchanged_by_queries(mrt, orc, gpu_ctx):
    import torch
    sc = _scene(mrt, (32, 32), SEED)
    rays = _case(mrt, orc, False)[2]
    d_rays = torch.from_numpy(np.array(rays[:4096])).to(f"cuda:{gpu_ctx.device}")
    with mrt.Renderer((32, 32), sc, ctx=gpu_ctx) as r:
        r.draw(2, wait=True)
        img = r.accumulation().copy()
        for _ in range(3):
            r.device_scene.intersect_closest_device(d_rays); r.device_scene.intersect_any_device(d_rays)
        torch.cuda.synchronize()
        r.frameIndex = 0; r.reset_stats()
        r.draw(2, wait=True)
        assert np.array_equal(img.view(np.uint32), r.accumulation().view(np.uint32))
