"""The materials extension (renderer option materials = 1): emission, a specular lobe and dielectric refraction from the
Material fields the reference already carries (ShaderTypes.h:99-107) but never reads (README.md:8 lists them as open work).  The
semantics are docs/HISTORY.md §10; the oracle (trace_pixel `if (materials)`) implements them and is pinned against float64 physics and known answers
(test_independent_f64.py, test_oracle_kat.py); the HIP kernel k_shade<true> must restate the oracle bit for bit — here at the boundaries of every
material predicate and queue shape — and with plain diffuse materials the extension must reduce to the reference path exactly."""
import numpy as np
import pytest

from material_scenes import with_material as _with_material, cornell_with_materials as _scene
from test_gpu_parity import assert_parity


def test_extension_reduces_to_the_reference_path_for_plain_materials(mrt, orc):
    w, h = 64, 48
    sc = _scene(mrt, (w, h), plain=True)
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    a = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); a.render(2)
    b = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); b.set_materials(True); b.render(2)
    assert np.array_equal(a.accumulation(), b.accumulation()) and a.counters() == b.counters()


def test_oracle_materials_change_the_image_where_expected(mrt, orc):
    w, h = 96, 72
    plain, fancy = _scene(mrt, (w, h), plain=True), _scene(mrt, (w, h))
    op = orc.OracleScene(mrt.flatten_scene(plain), plain.lights); of = orc.OracleScene(mrt.flatten_scene(fancy), fancy.lights)
    a = orc.OracleRenderer(op, w, h, max_bounces=4, camera=plain.camera); a.render(8)
    b = orc.OracleRenderer(of, w, h, max_bounces=4, camera=fancy.camera); b.set_materials(True); b.render(8)
    ia, ib = a.accumulation()[..., :3], b.accumulation()[..., :3]
    assert np.isfinite(ib).all() and (ib >= 0).all()
    assert np.abs(ia - ib).max() > 0.2                                  # the lamp is visible, the spheres look different
    # fewer shadow rays: specular and refracted bounces cast none
    assert b.counters()[1] < a.counters()[1]
    # without the option the fields are ignored, as in the reference kernel
    c = orc.OracleRenderer(of, w, h, max_bounces=4, camera=fancy.camera); c.render(8)
    d = orc.OracleRenderer(op, w, h, max_bounces=4, camera=plain.camera); d.render(8)
    assert not np.array_equal(c.accumulation(), b.accumulation())
    lit = np.abs(c.accumulation()[..., :3] - d.accumulation()[..., :3]).max()
    assert lit > 0                                                      # base colours differ, so the diffuse-only images differ too


@pytest.mark.gpu
def test_gpu_materials_match_the_oracle_bit_for_bit(mrt, orc, gpu_ctx):
    w, h = 160, 120
    sc = _scene(mrt, (w, h))
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, max_bounces=4)
    r.set_option("materials", 1)
    r.draw(6, wait=True)
    ref = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); ref.set_materials(True); ref.render(6)
    assert_parity(r.accumulation(), ref.accumulation())
    assert (r.stats.closest_rays, r.stats.shadow_rays) == ref.counters()
    # option off again: the reference kernel, same renderer
    r.set_option("materials", 0); r.frameIndex = 0; r.reset_stats()
    r.draw(2, wait=True)
    ref0 = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); ref0.render(2)
    assert_parity(r.accumulation(), ref0.accumulation())
    with pytest.raises(mrt.MRTError):
        r.set_option("max_bounces", 17); r.set_option("materials", 1)
    r.close()


@pytest.mark.gpu
def test_gpu_materials_on_the_benchmark_scene(mrt, orc, gpu_ctx):
    """DragonScene's own MTL values (Ks 0.2 / 0.8, Ns 37 ... 155 on the train, the dragon and the spheres) through the extension."""
    w, h = 192, 108
    sc = mrt.DragonScene((w, h))
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx)
    r.set_option("materials", 1)
    r.draw(3, wait=True)
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    ref = orc.OracleRenderer(osc, w, h, camera=sc.camera); ref.set_materials(True); ref.render(3)
    assert_parity(r.accumulation(), ref.accumulation())
    assert (r.stats.closest_rays, r.stats.shadow_rays) == ref.counters()
    r.close()


# ---------------------------------------------------------------- the extension's edges: material predicates at their boundaries, queue shapes, layouts, shards
import collections

import f64_reference as F
from material_scenes import EDGE_MATERIALS, edge_material_scene, look_at, quad_scene

EDGE_SIZE = (67, 45)            # ragged against the 8 x 8 tiles and against the 256-thread shade block (3015 pixels = 11 blocks + 199)


def _oracle_branches(orc, mrt, sc, w, h, max_bounces, frames):
    """What the oracle's paths did, from its per-bounce dump (origin, direction, t, triangle, normal, lobe code): Counter over F.BRANCHES, and one per object of the scene.
    reflect / refract: whether the next ray left on the side it came from; tir: sin theta_t >= 1 for the dumped direction and normal; absorbed: a specular sample with no next ray."""
    flat = mrt.flatten_scene(sc)
    tris = F.Triangles(flat)
    osc = orc.OracleScene(flat, sc.lights)
    r = orc.OracleRenderer(osc, w, h, max_bounces=max_bounces, camera=sc.camera); r.set_materials(True)
    total, per = collections.Counter(), collections.defaultdict(collections.Counter)
    names = getattr(sc, "object_names", None)
    for _ in range(frames):
        dump = r.render(1, dump=True).reshape(-1, max_bounces, 16)
        for b in range(max_bounces):
            rec = np.ascontiguousarray(dump[:, b])
            gid = np.ascontiguousarray(rec[:, 7]).view(np.uint32)
            hit = (rec[:, 3:6] != 0).any(1) & (gid != 0xFFFFFFFF)
            went_on = (dump[:, b + 1, 3:6] != 0).any(1) if b + 1 < max_bounces else None
            rec, gid = rec[hit].astype(np.float64), gid[hit].astype(np.int64)
            d, n, code = rec[:, 3:6], rec[:, 8:11], rec[:, 14]
            ev = {"emitter": (tris.emission[gid] > 0).any(1), "diffuse": code > -1.5}
            if went_on is not None:
                d2 = dump[:, b + 1, 3:6][hit].astype(np.float64)
                same_side = (d2 * n).sum(1) * (d * n).sum(1) < 0
                ev["reflect"] = (code == -2) & same_side; ev["refract"] = (code == -2) & ~same_side
                ev["specular"] = (code == -3) & went_on[hit]; ev["absorbed"] = (code == -3) & ~went_on[hit]
                die = code == -2
                tir = np.zeros(len(d), bool)
                if die.any(): tir[die] = F.dielectric(d[die], n[die], tris.Ni[gid[die]])["tir"]
                ev["tir"] = tir & ev["reflect"]
            for k, m in ev.items():
                total[k] += int(m.sum())
                if names:
                    for inst in np.unique(tris.ids[gid[m], 0]): per[names[inst]][k] += int((tris.ids[gid[m], 0] == inst).sum())
    r.close(); osc.close()
    return total, per


def _assert_every_branch_is_taken(orc, mrt, sc, w, h, max_bounces=4, frames=2):
    total, per = _oracle_branches(orc, mrt, sc, w, h, max_bounces, frames)
    assert all(total[k] >= 5 for k in F.BRANCHES), total
    assert set(per) == {"wall"} | set(EDGE_MATERIALS), sorted(per)                                          # every object is met by some path
    die = lambda c: c["reflect"] + c["refract"]
    assert die(per["glass_thin"]) > 100 and per["glass_thin"]["reflect"] > 0 and per["glass_thin"]["refract"] > 0
    assert per["glass_tir"]["tir"] > 0 and per["glass_tir"]["refract"] > 0 and per["glass_tir"]["diffuse"] > 0
    assert per["glass_index_1"]["refract"] > 0 and per["glass_index_1"]["specular"] > 0 and per["glass_index_1"]["diffuse"] > 0
    assert die(per["index_0"]) == 0 and per["index_0"]["specular"] > 0 and per["index_0"]["absorbed"] > 0 and per["index_0"]["diffuse"] > 0
    assert die(per["dissolve_0"]) == 0 and per["dissolve_0"]["specular"] + per["dissolve_0"]["absorbed"] == 0 and per["dissolve_0"]["diffuse"] > 0
    assert die(per["mirror"]) == 0 and per["mirror"]["diffuse"] == 0 and per["mirror"]["specular"] > 0      # ps = 1
    assert per["black_emitter"]["emitter"] > 0 and per["black_emitter"]["diffuse"] > 0
    assert per["emissive_glass"]["emitter"] > 0 and die(per["emissive_glass"]) > 0 and per["emissive_glass"]["specular"] > 0
    assert die(per["wall"]) + per["wall"]["specular"] + per["wall"]["absorbed"] == 0


def test_edge_material_scene_takes_every_branch_of_the_definition(mrt, orc):
    """The precondition of the GPU comparisons below: in the oracle's image of the edge-material scene every branch of docs/HISTORY.md §10 is taken, and each material does what its
    boundary values say (Ni 0 or dissolve 0 / 1: never the interface; Ns 0: never the lobe; Kd 0: always the lobe)."""
    w, h = EDGE_SIZE
    sc = edge_material_scene(mrt, (w, h))
    _assert_every_branch_is_taken(orc, mrt, sc, w, h)
    img = orc.OracleRenderer(orc.OracleScene(mrt.flatten_scene(sc), sc.lights), w, h, max_bounces=4, camera=sc.camera)
    img.set_materials(True); img.render(2)
    a = img.accumulation()
    assert np.isfinite(a).all() and (a[..., :3] >= 0).all() and (a[..., :3].sum(-1) > 0).mean() > 0.6          # most of the frame is lit


def _bits_equal(gpu, ref, what=""):
    assert_parity(gpu, ref)
    bad = (gpu.view(np.uint32) != ref.view(np.uint32)).any(-1)
    assert not bad.any(), f"{what}: {bad.sum()} pixels differ in their bits, first at {np.argwhere(bad)[:4].tolist()}"


def _gpu_against_oracle(mrt, orc, gpu_ctx, sc, w, h, draws, max_bounces=4, options=None, scene_options=None, instancing=False, shard=None):
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=True) if instancing else mrt.flatten_scene(sc), sc.lights, instancing=instancing)
    ref = orc.OracleRenderer(osc, w, h, max_bounces=max_bounces, camera=sc.camera); ref.set_materials(True)
    r = mrt.Renderer((w, h), sc, ctx=gpu_ctx, max_bounces=max_bounces, scene_options=scene_options)
    try:
        r.set_option("materials", 1)
        for k, v in (options or {}).items(): r.set_option(k, v)
        if shard: r.set_shard(*shard); ref.set_shard(*shard)
        for n in draws: r.draw(n)
        r.wait()
        ref.render(sum(draws))
        _bits_equal(r.accumulation(), ref.accumulation(), f"{options} {scene_options} {shard}")
        assert (r.stats.closest_rays, r.stats.shadow_rays) == ref.counters()
        return r.accumulation(), ref.counters(), r.device_scene.stats
    finally:
        r.close(); ref.close(); osc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "frame_batch_1", "frame_batch_4", "one_in_flight", "one_bounce", "sixteen_bounces", "rope_layout", "two_level", "two_level_rope"])
def test_gpu_edge_materials_match_the_oracle_bit_for_bit(mrt, orc, gpu_ctx, case):
    """k_shade<MATERIALS> at the boundaries of its predicates (EDGE_MATERIALS) on an image that is ragged against the tiles and the shade block, across pass sizes, bounce
    counts, the rope-only layout and two-level scenes: accumulation bits and both ray counts equal the oracle's."""
    w, h = EDGE_SIZE
    sc = edge_material_scene(mrt, (w, h))
    kw = {"default": dict(draws=[3]),
          "frame_batch_1": dict(draws=[3], options={"frame_batch": 1}),
          "frame_batch_4": dict(draws=[4], options={"frame_batch": 4}),
          "one_in_flight": dict(draws=[2, 2], options={"frame_batch": 2, "frames_in_flight": 1}),
          "one_bounce": dict(draws=[3], max_bounces=1),
          "sixteen_bounces": dict(draws=[2], max_bounces=16),
          "rope_layout": dict(draws=[3], scene_options={"wide": 0}),
          "two_level": dict(draws=[3], scene_options={"instancing": 1}, instancing=True),
          "two_level_rope": dict(draws=[2], scene_options={"instancing": 1, "wide": 0}, instancing=True)}[case]
    if case == "default":
        _assert_every_branch_is_taken(orc, mrt, sc, w, h)
    _, counters, st = _gpu_against_oracle(mrt, orc, gpu_ctx, sc, w, h, **kw)
    if case == "one_bounce": assert counters[0] == 3 * w * h
    if case == "sixteen_bounces":                                                    # the last bounce (and with it Halton dimension 2 + 5 * 16 + 15 = 97) is reached
        deep = orc.OracleRenderer(orc.OracleScene(mrt.flatten_scene(sc), sc.lights), w, h, max_bounces=16, camera=sc.camera); deep.set_materials(True)
        assert (deep.render(2, dump=True)[:, :, 15, 3:6] != 0).any(-1).sum() >= 20
    if case in ("rope_layout", "two_level_rope"): assert st.wide_layout == 0
    if case.startswith("two_level"): assert st.instances == 14 and mrt.flatten_scene(sc, share=True)[-1][4] == 5 and [e[4] for e in mrt.flatten_scene(sc, share=True)[:5]] == [-1, 0, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_edge_materials_shards_sum_to_the_full_frame(mrt, orc, gpu_ctx):
    w, h = EDGE_SIZE
    sc = edge_material_scene(mrt, (w, h))
    total, rays = np.zeros((h, w, 4), np.float32), np.zeros(2, np.int64)
    for rank in range(3):
        a, c, _ = _gpu_against_oracle(mrt, orc, gpu_ctx, sc, w, h, [3], shard=(rank, 3))          # each shard == the oracle's shard
        total += a; rays += c
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    full = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); full.set_materials(True); full.render(3)
    assert np.array_equal(total.view(np.uint32), full.accumulation().view(np.uint32)) and tuple(rays) == full.counters()


@pytest.mark.gpu
def test_gpu_materials_toggled_between_draws_of_one_renderer(mrt, orc, gpu_ctx):
    w, h = EDGE_SIZE
    sc = edge_material_scene(mrt, (w, h))
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    with mrt.Renderer((w, h), sc, ctx=gpu_ctx, max_bounces=4) as r:
        for on in (0, 1, 0, 1):
            r.set_option("materials", on); r.frameIndex = 0; r.reset_stats()
            r.draw(2, wait=True)
            ref = orc.OracleRenderer(osc, w, h, max_bounces=4, camera=sc.camera); ref.set_materials(bool(on)); ref.render(2)
            _bits_equal(r.accumulation(), ref.accumulation(), f"materials = {on}")
            assert (r.stats.closest_rays, r.stats.shadow_rays) == ref.counters()
            ref.close()


def _glass_wall_scene(mrt, size):
    """the camera close to a quad of dissolve 2^-20 that fills the frame, a lit floor and back wall behind it: every primary hit takes the interface"""
    glass = dict(EDGE_MATERIALS["glass_thin"], refractionIndex=1.5)
    quads = [dict(position=[0, 1, 1.5], rotation=[np.pi / 2, 0, 0], scale=2.0, **glass), dict(position=[0, 0, 0], scale=4.0), dict(position=[0, 1, -1], rotation=[np.pi / 2, 0, 0], scale=4.0)]
    return quad_scene(mrt, size, quads, [mrt.Scene.setupLight()], look_at(mrt, [0.0, 1.0, 2.5], [0.1, 0.8, 0.0], 0.5, 0.375))


@pytest.mark.gpu
def test_gpu_queue_with_an_empty_diffuse_class(mrt, orc, gpu_ctx):
    """Every primary hit is glass: in the first shade no lane queues a diffuse ray or a shadow ray (m_nx = m_sh = 0), all of them queue a special one."""
    w, h = 32, 24
    sc = _glass_wall_scene(mrt, (w, h))
    one = orc.OracleRenderer(orc.OracleScene(mrt.flatten_scene(sc), sc.lights), w, h, max_bounces=1, camera=sc.camera); one.set_materials(True); one.render(2)
    assert one.counters() == (2 * w * h, 0) and not one.accumulation()[..., :3].any()                       # the precondition: no primary sample cast a shadow ray, all hit
    _, counters, _ = _gpu_against_oracle(mrt, orc, gpu_ctx, sc, w, h, [2], max_bounces=4)
    assert counters[0] > 2 * 2 * w * h and counters[1] > 0                                                    # ... and the special rays went on to lit surfaces


@pytest.mark.gpu
def test_gpu_queue_with_an_empty_special_class(mrt, orc, gpu_ctx):
    """Plain materials with the option on: no lane is ever special (m_sp = 0), and the GPU's own image with the option off has the same bits."""
    w, h = 32, 24
    sc = _scene(mrt, (w, h), plain=True)
    on, counters, _ = _gpu_against_oracle(mrt, orc, gpu_ctx, sc, w, h, [3])
    with mrt.Renderer((w, h), sc, ctx=gpu_ctx, max_bounces=4) as r:
        r.draw(3, wait=True)
        assert np.array_equal(r.accumulation().view(np.uint32), on.view(np.uint32)) and (r.stats.closest_rays, r.stats.shadow_rays) == counters


@pytest.mark.gpu
def test_gpu_materials_on_a_one_pixel_image(mrt, orc, gpu_ctx):
    sc = edge_material_scene(mrt, (1, 1))
    sc.camera = look_at(mrt, [0.0, 1.0, 3.4], [-0.6, 0.25, 0.3], 0.02, 0.02)         # the one pixel looks at the glass_thin sphere
    a, counters, _ = _gpu_against_oracle(mrt, orc, gpu_ctx, sc, 1, 1, [4])
    assert counters[0] >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("x0,y0", [(16, 8), (28, 8)])
def test_gpu_materials_match_float64_physics_directly(mrt, orc, gpu_ctx, x0, y0):
    """The hardware path against tests/f64_reference.py without the oracle in between: the crops, rule and bound of
    test_independent_f64.test_oracle_materials_match_float64_physics_on_a_cornell_crop."""
    from test_independent_f64 import MATERIAL_CROPS, _crop_against_f64, materials_crop_is_not_vacuous
    assert (x0, y0) in MATERIAL_CROPS
    w, h = 64, 48
    sc = _scene(mrt, (w, h))
    with mrt.Renderer((w, h), sc, ctx=gpu_ctx, seed=1, max_bounces=4) as r:
        r.set_option("materials", 1)
        def image(f):
            r.draw(1, wait=True)
            assert r.frameIndex == f + 1
            return r.accumulation()
        _, _, _, _, tally = _crop_against_f64(orc, mrt, sc, w, h, x0, y0, materials=True, max_bounces=4, image=image)
    materials_crop_is_not_vacuous(tally)
