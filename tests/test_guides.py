"""First-hit guide buffers (renderer option guides = 1; include/mrt_abi.h MRT_GUIDE_*, csrc/guides.h): shading normal | distance, base colour |
coverage and the ids of the PRIMARY hit, the first two averaged over the frames by the accumulation buffer's rule.  The oracle's stage dump holds
all of it for bounce 0 (origin, direction, t, id, shading normal), so the buffers are compared bit for bit; and switching them on moves nothing
that existed before."""
import numpy as np
import pytest

import denoise_reference as D

ERR_STATE = 5


def _owned_mask(w, h, rank, world):
    y, x = np.mgrid[0:h, 0:w]
    return ((y // 8) * ((w + 7) // 8) + (x // 8)) % world == rank


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _run(mrt, orc, gpu_ctx, sc, w, h, draws, options=None, scene_options=None, instancing=False, materials=False, shard=None, seed=3):
    """draw `draws` (a list of frame counts, one render call each) with guides on and compare with the buffers built from the oracle's dumps"""
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=True) if instancing else mrt.flatten_scene(sc), sc.lights, instancing=instancing)
    orr = orc.OracleRenderer(osc, w, h, seed=seed, max_bounces=3, camera=sc.camera)
    if materials: orr.set_materials(True)
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=seed, scene_options=scene_options)
    try:
        r.set_option("guides", 1)
        for k, v in (options or {}).items(): r.set_option(k, v)
        owned = None
        if shard:
            r.set_shard(*shard); orr.set_shard(*shard); owned = _owned_mask(w, h, *shard)
        for n in draws: r.draw(n)
        r.wait()
        g = r.guides()
        nd, al, ids, rays = D.oracle_guides(orr, sc, sum(draws), r.device_scene.intersect_closest, owned=owned)
        assert _same_bits(g["normal_depth"], nd), f"normal | depth: {(g['normal_depth'].view(np.uint32) != nd.view(np.uint32)).any(-1).sum()} pixels differ"
        assert _same_bits(g["albedo"], al), f"albedo | coverage: {(g['albedo'].view(np.uint32) != al.view(np.uint32)).any(-1).sum()} pixels differ"
        assert np.array_equal(g["ids"], ids), f"ids: {(g['ids'] != ids).any(-1).sum()} pixels differ"
        # the ids once more, against the scene query on the last frame's rays
        q = r.device_scene.intersect_closest(rays).reshape(h, w)
        m = np.ones((h, w), bool) if owned is None else owned
        for k, f in enumerate(("type", "instance_id", "geometry_id", "primitive_id")):
            assert np.array_equal(g["ids"][..., k][m], q[f][m]), f
        if owned is not None:
            for name in ("normal_depth", "albedo", "ids"): assert not g[name][~owned].any(), name
        # the colour path is the oracle's as ever
        assert (r.stats.closest_rays, r.stats.shadow_rays) == orr.counters()
        return g
    finally:
        r.close(); orr.close(); osc.close()


def _no_dragon(mrt, size):
    sc = mrt.DragonScene(size)
    sc.models = [m for m in sc.models if m.name != "dragon"]
    return sc


def _sky(mrt, size):
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="plane", position=[0, 0, 0], scale=10)]
    return S(size)


@pytest.mark.gpu
@pytest.mark.parametrize("draws,options", [([1], {}), ([5], {}), ([2, 3], {}), ([5], {"frame_batch": 1}), ([5], {"frame_batch": 4}), ([2, 3], {"frame_batch": 4, "frames_in_flight": 1}),
                                           ([5], {"megakernel": 1})])
def test_cornell_guides_equal_the_oracle(mrt, orc, gpu_ctx, draws, options):
    g = _run(mrt, orc, gpu_ctx, mrt.CornellScene((64, 64)), 64, 64, draws, options)
    assert (g["albedo"][..., 3] == 1).any() and (g["normal_depth"][..., 3] > 0).any()


@pytest.mark.gpu
def test_train_submeshes_give_geometry_ids(mrt, orc, gpu_ctx):
    g = _run(mrt, orc, gpu_ctx, _no_dragon(mrt, (96, 54)), 96, 54, [3])
    assert (g["ids"][..., 2] > 0).any(), "no pixel shows a submesh beyond the first: the case does not cover geometry_id"


@pytest.mark.gpu
def test_two_level_scene(mrt, orc, gpu_ctx):
    from test_instancing import _scene
    g = _run(mrt, orc, gpu_ctx, _scene(mrt, (64, 48)), 64, 48, [3], scene_options={"instancing": 1}, instancing=True)
    assert len(np.unique(g["ids"][..., 1])) >= 4


@pytest.mark.gpu
def test_two_level_scene_without_the_wide_layout(mrt, orc, gpu_ctx):
    from test_instancing import _scene
    _run(mrt, orc, gpu_ctx, _scene(mrt, (64, 48)), 64, 48, [3], scene_options={"instancing": 1, "wide": 0}, instancing=True)


@pytest.mark.gpu
def test_rope_walk(mrt, orc, gpu_ctx):
    _run(mrt, orc, gpu_ctx, mrt.CornellScene((64, 64)), 64, 64, [3], scene_options={"wide": 0})


@pytest.mark.gpu
def test_ragged_size(mrt, orc, gpu_ctx):
    _run(mrt, orc, gpu_ctx, mrt.CornellScene((37, 23)), 37, 23, [3])


@pytest.mark.gpu
def test_sky_pixels_are_misses(mrt, orc, gpu_ctx):
    g = _run(mrt, orc, gpu_ctx, _sky(mrt, (64, 48)), 64, 48, [4])
    hit = g["ids"][..., 0] == 1
    assert hit.any() and (~hit).any()
    never = g["albedo"][..., 3] == 0
    assert never.any() and np.array_equal(g["ids"][never], np.broadcast_to(np.array([0, -1, -1, -1], np.int32), g["ids"][never].shape))
    assert not g["normal_depth"][never].any() and not g["albedo"][never].any()


@pytest.mark.gpu
def test_shard_owns_its_pixels_only(mrt, orc, gpu_ctx):
    _run(mrt, orc, gpu_ctx, mrt.CornellScene((64, 64)), 64, 64, [2, 2], shard=(1, 3))


@pytest.mark.gpu
def test_materials_extension(mrt, orc, gpu_ctx):
    _run(mrt, orc, gpu_ctx, mrt.CornellScene((64, 64)), 64, 64, [3], options={"materials": 1}, materials=True)


@pytest.mark.gpu
def test_guides_restart_after_a_resize_and_follow_the_frame_index(mrt, orc, gpu_ctx):
    sc = mrt.CornellScene((64, 64))
    r = mrt.Renderer((64, 64), sc, ctx=gpu_ctx, seed=5)
    try:
        r.set_option("guides", 1)
        r.draw(3, wait=True)
        r.drawableSizeWillChange((48, 40))
        with pytest.raises(mrt.MRTError) as e: r.guides()           # nothing rendered since
        assert e.value.code == ERR_STATE
        r.draw(2, wait=True)
        osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
        orr = orc.OracleRenderer(osc, 48, 40, seed=5, max_bounces=3, camera=sc.camera)
        nd, al, ids, _ = D.oracle_guides(orr, sc, 2, r.device_scene.intersect_closest)
        g = r.guides()
        assert _same_bits(g["normal_depth"], nd) and _same_bits(g["albedo"], al) and np.array_equal(g["ids"], ids)
        # frameIndex = 0 restarts the average, as it restarts the accumulation
        r.frameIndex = 0; orr.set_frame_index(0)
        r.draw(1, wait=True)
        nd, al, ids, _ = D.oracle_guides(orr, sc, 1, r.device_scene.intersect_closest)
        g = r.guides()
        assert _same_bits(g["normal_depth"], nd) and _same_bits(g["albedo"], al) and np.array_equal(g["ids"], ids)
        orr.close(); osc.close()
    finally:
        r.close()


# ---------------------------------------------------------------- nothing existing moves
@pytest.mark.gpu
def test_guides_leave_image_counters_and_queue_memory_alone(mrt, gpu_ctx):
    sc = mrt.CornellScene((64, 64))
    a = mrt.Renderer((64, 64), sc, ctx=gpu_ctx, seed=2)
    b = mrt.Renderer((64, 64), sc, ctx=gpu_ctx, seed=2)
    try:
        lane0 = b.get_option("lane_bytes")
        b.set_option("guides", 1)
        assert b.get_option("guides") == 1 and b.get_option("lane_bytes") == lane0
        a.draw(5, wait=True); b.draw(5, wait=True)
        assert _same_bits(a.accumulation(), b.accumulation())
        assert (a.stats.closest_rays, a.stats.shadow_rays, a.stats.primary_rays) == (b.stats.closest_rays, b.stats.shadow_rays, b.stats.primary_rays)
        assert a.get_option("guides") == 0
        for call in (a.guides, a.denoise, a.denoised, a.denoised_tonemapped):
            with pytest.raises(mrt.MRTError) as e: call()
            assert e.value.code == ERR_STATE, call
        b.set_option("guides", 0)
        assert b.get_option("lane_bytes") == lane0
        with pytest.raises(mrt.MRTError) as e: b.guides()
        assert e.value.code == ERR_STATE
        b.draw(2, wait=True); a.draw(2, wait=True)
        assert _same_bits(a.accumulation(), b.accumulation())
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_guide_arguments_are_checked(mrt, gpu_ctx):
    import ctypes as C
    r = mrt.Renderer((32, 32), mrt.CornellScene((32, 32)), ctx=gpu_ctx)
    try:
        r.set_option("guides", 1)
        with pytest.raises(mrt.MRTError) as e: r.guides()           # before any frame
        assert e.value.code == ERR_STATE
        r.draw(1, wait=True)
        buf = np.zeros((32, 32, 4), np.float32)
        assert mrt.lib.mrt_renderer_read_guide(r.handle, 3, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert mrt.lib.mrt_renderer_read_guide(r.handle, -1, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 1
        assert mrt.lib.mrt_renderer_read_guide(r.handle, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 16) == 1
        assert mrt.lib.mrt_renderer_read_guide(r.handle, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
        with pytest.raises(mrt.MRTError): r.set_option("guides", 2)
    finally:
        r.close()


@pytest.mark.gpu
def test_copy_guide_to_a_torch_tensor(mrt, gpu_ctx):
    import torch
    r = mrt.Renderer((40, 24), mrt.CornellScene((40, 24)), ctx=gpu_ctx)
    try:
        r.set_option("guides", 1)
        r.draw(2)
        t = torch.zeros((24, 40, 4), dtype=torch.float32, device="cuda:0")
        r.copy_guide_to(0, t.data_ptr(), t.numel() * 4)
        r.wait(); torch.cuda.synchronize()
        assert _same_bits(t.cpu().numpy(), r.guides()["normal_depth"])
    finally:
        r.close()
