"""Every rope layout the library emits or refits, read back (mrt_debug_read_layout parts 8 and 9) and audited exactly by tests/rope_audit.py: structure,
all eight escape links of every node, every parent box the bitwise union of its children's, every triangle inside its leaf box with half a pad to spare, and
— across a refit — links and ids untouched.  Flattened scenes of every builder, leaf size and pre-split setting; degenerate shapes; three refits of a
20 K-triangle mesh (about 40 K rope nodes over a few hundred workgroups: the refit's hand-off between compute units, checked node by node) through the commit
and through the stream-ordered entries; a partial refit beside unmoved geometry; the BLASes of two-level scenes through builds, refits and TLAS updates.
The tests build, update, read back and audit: none launches a traversal.  Every test prints what it audited (nodes, leaves, packets, packets excused from
the pad check as pre-split references)."""
import numpy as np
import pytest

import rope_audit as R
from test_blas_device import BOX, QUAD, _deformed, _dev_update, _host_update
from test_bvh_bounds import BUILDS, SCENES, _Scene, _cube, _opts, _quad
from test_deep_tree import _scene as _chain_scene
from test_fuzz_geometry import _fan, _scene as _hostile_scene
from test_instances_device import _case as _instances_case, _host_move, _poses, _t
from test_refit_device import FAN, _moved

pytestmark = pytest.mark.gpu

ROPE_LAYOUTS = {"rope_only": {"wide": 0}, "wide+rope": {"rope": 1}}


def _audit(ds, what, presplit, num_tris=None, before=None):
    """the full audit of the scene's rope layout (and links_kept against an earlier read-back); prints the counts; returns the layout"""
    lay = R.layout_of(ds)
    rep = R.audit(lay, presplit=presplit, num_tris=num_tris)
    print(f"rope audit [{what}]: trees {rep.counts['trees']} nodes {rep.counts['nodes']} leaves {rep.counts['leaves']} packets {rep.counts['packets']} "
          f"excused from the pad check {rep.counts['pad_excused']}; thinnest margin {rep.summary().get('pad')}")
    try:
        rep.check()
        if before is not None:
            R.links_kept(before, lay).check()
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    assert rep.counts["nodes"] == 2 * rep.counts["leaves"] - rep.counts["trees"], (what, rep.counts)          # binary trees
    return lay, rep


def _no_rope(ds):
    return len(ds.read_layout("rope_nodes")) == 0 and len(ds.read_layout("rope_packets")) == 0


# ------------------------------------------------------------------------------------------------ builds, flattened
@pytest.mark.parametrize("layout", list(ROPE_LAYOUTS))
@pytest.mark.parametrize("scene", ["axis", "axis_far", "axis_tiny", "stadium", "hostile"])
def test_every_flattened_build(mrt, gpu_ctx, scene, layout):
    """builders 0, 1, 2 x max_leaf 1, 4 x pre-split off and default, alone (wide = 0) and beside the 8-wide layout (rope = 1).  Only slivers much longer than
    the scene's mean triangle are pre-split (k_split_count): none in test_bvh_bounds' scenes, a few of the soup's in test_fuzz_geometry's hostile scene"""
    sc = SCENES[scene](mrt) if scene in SCENES else _hostile_scene(mrt, (96, 64), 1)
    T = sc.triangleCount
    for b in BUILDS:
        ds = mrt.DeviceScene(gpu_ctx, sc, {**_opts(b), **ROPE_LAYOUTS[layout]})
        assert ds.stats.wide_layout == (0 if layout == "rope_only" else 1)
        lay, rep = _audit(ds, f"{scene} {layout} {b}", presplit=b["presplit"] is None, num_tris=T)
        assert rep.counts["packets"] >= T and (b["presplit"] is None or rep.counts["packets"] == T)
        if b["max_leaf"] == 1:
            assert rep.counts["leaves"] == rep.counts["packets"]
        if scene == "hostile" and b["presplit"] is None:
            assert rep.counts["pad_excused"] > 0 and rep.counts["packets"] > T, "the hostile scene's slivers enter the build as several references"
        ds.close()


def test_a_scene_that_keeps_no_rope_layout_reports_none(mrt, gpu_ctx):
    sc = SCENES["axis"](mrt)
    for opts in ({}, {"rope": 0}):
        ds = mrt.DeviceScene(gpu_ctx, sc, opts)
        assert ds.stats.wide_layout == 1 and _no_rope(ds)
        assert R.audit(R.layout_of(ds)).failures == ["structure: no rope layout"]
        with pytest.raises(mrt.MRTError):          # parts are 0 .. 9
            ds.read_layout(10)
        ds.close()


# ------------------------------------------------------------------------------------------------ degenerate shapes
def _soup_scene(mrt, tris):
    pos = np.asarray(tris, np.float32).reshape(-1, 3)
    return _Scene(mrt, (64, 48), [("tris", pos, np.arange(len(pos), dtype=np.uint32).reshape(-1, 3), (0, 0, 0), 1.0)])


def _shapes(mrt):
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32) + [-0.5, 0.3, -0.2]
    rng = np.random.default_rng(29)
    return {
        "one": _soup_scene(mrt, [tri]),
        "two": _soup_scene(mrt, [tri, tri + [2, 0, 1]]),
        "three": _soup_scene(mrt, [tri, tri + [2, 0, 1], tri * 0.01 + [0, 5, 0]]),
        "coincident": _soup_scene(mrt, np.tile(tri, (67, 1, 1))),          # one Morton key: the radix tree splits by index
        "fan": _Scene(mrt, (64, 48), [("fan", *_fan(rng, 300), (0, 0, 0), 1.0)]),
    }


@pytest.mark.parametrize("shape", ["one", "two", "three", "coincident", "fan"])
def test_degenerate_shapes(mrt, gpu_ctx, shape):
    sc = _shapes(mrt)[shape]
    T = sc.triangleCount
    for layout, lopt in ROPE_LAYOUTS.items():
        for b in BUILDS:
            ds = mrt.DeviceScene(gpu_ctx, sc, {**_opts(b), **lopt})
            lay, rep = _audit(ds, f"{shape} {layout} {b}", presplit=b["presplit"] is None, num_tris=T)
            if T == 1:
                assert rep.counts["nodes"] == 1 and (lay["rope_nodes"][0, 8:16] == R.NODE_TERM).all()
            ds.close()


def test_the_empty_scene_has_no_rope_layout(mrt, gpu_ctx):
    sc = mrt.Scene((64, 48))
    sc.models = []
    for opts in ({"wide": 0}, {"rope": 1}, {}):
        ds = mrt.DeviceScene(gpu_ctx, sc, opts)
        assert _no_rope(ds), opts
        ds.close()


@pytest.mark.parametrize("n,growth", [(150, 1.055), (520, 1.0155)])
def test_nested_chains(mrt, gpu_ctx, n, growth):
    """the agglomerative builder's chain, as deep as it has triangles, as the rope layout keeps it (wide = 0)"""
    sc = _chain_scene(mrt, n, growth)
    ds = mrt.DeviceScene(gpu_ctx, sc, {"wide": 0, "max_leaf": 1})
    lay, rep = _audit(ds, f"chain {n}", presplit=True, num_tris=sc.triangleCount)
    print(f"chain {n}: rope depth {ds.stats.max_depth}")
    assert ds.stats.max_depth > n // 2
    ds.close()


# ------------------------------------------------------------------------------------------------ refits, flattened
def _sheet_scene(mrt):
    """test_bvh_bounds.test_three_refits_keep_every_box's scene: a 19 602-triangle sheet and a cube"""
    X, Z = np.eye(3)[0], np.eye(3)[2]
    pos, idx = _quad((0, 0, 0), X, Z, 99)
    return _Scene(mrt, (96, 64), [("sheet", pos, idx, (0, 0.5, 0), 1.0), ("cube", *_cube((0, 0, 0), 0.2), (1.5, 0.3, 0), 1.0)]), pos


def _sheet_steps(pos):
    """three deformations by up to 20 % of the extent, some vertices pushed past the old root box"""
    rng = np.random.default_rng(3)
    p = pos.astype(np.float64)
    for k in range(3):
        q = p + rng.uniform(-0.2, 0.2, p.shape) * 2.0 * rng.random((len(p), 1))
        q[rng.random(len(p)) < 0.01] *= 1.25
        yield k, q.astype(np.float32), np.tile(np.float32([0, 1, 0]), (len(q), 1))


@pytest.mark.parametrize("path", ["commit", "device"])
@pytest.mark.parametrize("max_leaf", [4, 1])
@pytest.mark.parametrize("layout", list(ROPE_LAYOUTS))
def test_three_refits_of_a_large_mesh(mrt, gpu_ctx, layout, max_leaf, path):
    """after each refit: the full audit — every parent the union of its children, whichever workgroup arrived second — and the build's links kept.  The default
    leaf size (about 10 K nodes, leaves of several triangles) and max_leaf = 1 (about 39 K nodes, one climbing thread per triangle)"""
    import torch
    sc, pos = _sheet_scene(mrt)
    T = sc.triangleCount
    ds = mrt.DeviceScene(gpu_ctx, sc, {**ROPE_LAYOUTS[layout], "max_leaf": max_leaf})
    built, rep = _audit(ds, f"sheet {layout} max_leaf {max_leaf} built", presplit=True, num_tris=T)
    assert rep.counts["nodes"] > (9000 if max_leaf == 4 else 39000), "large enough for the hand-off to happen between compute units"
    last = built
    for k, q, nrm in _sheet_steps(pos):
        if path == "commit":
            ds.update_mesh(0, q, nrm); ds.commit()
        else:
            tq, tn = _t(q, gpu_ctx), _t(nrm, gpu_ctx)
            ds.update_mesh_device(0, tq, tn); ds.refit_device()
            torch.cuda.synchronize()
        assert ds.refits == k + 1
        lay, rep = _audit(ds, f"sheet {layout} max_leaf {max_leaf} {path} refit {k}", presplit=True, num_tris=T, before=built)
        assert not np.array_equal(lay["rope_nodes"][:, :8], last["rope_nodes"][:, :8]), "the refit must have moved boxes"
        last = lay
    assert ds.device_updates_rejected == 0
    ds.close()


def _partial_case(mrt, scene):
    """(scene, mesh to deform, its new vertices): Cornell's tessellated box beside its ten wall triangles; test_fuzz_geometry's hostile scene with its pole
    fan (three flattened copies) moving beside the triangle soup, whose slivers the build pre-splits"""
    if scene == "cornell":
        sc = mrt.CornellScene((64, 64))
        meshes = mrt.flatten_scene(sc, share=True)
        k = max(range(len(meshes)), key=lambda i: len(meshes[i][0]) if meshes[i][4] < 0 else -1)
        pos = np.asarray(meshes[k][0], np.float32)
        return sc, meshes, k, (pos * np.float32(1.07) + np.float32(0.02) * np.sin(9.0 * pos[:, [2, 0, 1]])).astype(np.float32)
    sc = _hostile_scene(mrt, (96, 64), 1)
    meshes = mrt.flatten_scene(sc, share=True)
    return sc, meshes, FAN, _moved(meshes[FAN][0], 0)


@pytest.mark.parametrize("layout", list(ROPE_LAYOUTS))
@pytest.mark.parametrize("scene", ["cornell", "hostile"])
def test_a_partial_refit_keeps_the_unmoved_leaves(mrt, gpu_ctx, scene, layout):
    """one mesh deformed beside geometry that stays: the leaves none of whose triangles moved (pre-split references with their clipped boxes among them in
    the hostile scene) keep their boxes bit for bit, the others get new ones, the whole tree passes the audit"""
    sc, meshes, k, new_pos = _partial_case(mrt, scene)
    T = sc.triangleCount
    ntri = [sum(len(idx) for idx, _ in m[3]) for m in meshes]
    first = np.cumsum([0] + ntri)
    assert first[-1] == T
    moved_gid = np.zeros(T, bool)
    for i, m in enumerate(meshes):
        if i == k or m[4] == k:
            moved_gid[first[i]:first[i + 1]] = True
    ds = mrt.DeviceScene(gpu_ctx, sc, ROPE_LAYOUTS[layout])
    built, rep0 = _audit(ds, f"{scene} {layout} built", presplit=True, num_tris=T)
    ds.update_mesh(k, new_pos, np.asarray(meshes[k][1], np.float32)); ds.commit()
    assert ds.refits == 1
    lay, rep = _audit(ds, f"{scene} {layout} refitted", presplit=True, num_tris=T, before=built)
    wn0, wn1 = built["rope_nodes"], lay["rope_nodes"]
    leaves = np.nonzero(wn0[:, 3] & R.NODE_LEAF)[0]
    gid = lay["rope_packets"][:, 3]
    touched = np.array([moved_gid[gid[(wn0[nd, 3] & 0x7FFFFFFF):(wn0[nd, 3] & 0x7FFFFFFF) + wn0[nd, 7]]].any() for nd in leaves])
    print(f"{scene} {layout}: {touched.sum()} of {len(leaves)} leaves hold a moved triangle; pre-split packets {rep.counts['pad_excused']}")
    assert touched.any() and not touched.all()
    still = leaves[~touched]
    assert np.array_equal(wn0[still], wn1[still]), "a leaf none of whose triangles moved keeps its box bit for bit"
    assert not np.array_equal(wn0[leaves[touched]], wn1[leaves[touched]])
    assert rep.counts["pad_excused"] == rep0.counts["pad_excused"]
    if scene == "hostile":
        assert rep.counts["pad_excused"] > 0, "the soup's slivers are long against the scene's mean triangle: the build pre-splits them (k_split_count)"
    ds.close()


# ------------------------------------------------------------------------------------------------ two-level scenes: every BLAS
def _same_rope(a, b, what):
    assert np.array_equal(a["rope_nodes"], b["rope_nodes"]) and np.array_equal(a["rope_packets"], b["rope_packets"]), what + ": the BLASes' rope nodes and packets must be untouched bit for bit"


@pytest.mark.parametrize("rope", [0, 1])
@pytest.mark.parametrize("n", [2, 5])
def test_the_blases_of_a_two_level_scene(mrt, gpu_ctx, n, rope):
    """test_instances_device's scenes: the 12-triangle box (a BLAS of several rope nodes, shared by its instances) and the two-triangle quad (its BLAS root is a
    leaf when max_leaf allows).  Scene A: build, a BLAS refit by update_mesh + commit, a transform-only commit.  Scene B: build, the same refit through the device
    entries, a device TLAS rebuild.  The TLAS-only steps leave parts 8 and 9 as they were."""
    import torch
    sc, meshes, rays = _instances_case(mrt, n)
    opts = dict({"rope": 1} if rope else {}, instancing=1)
    tag = f"two-level n={n} rope={rope}"
    a, b = mrt.DeviceScene(gpu_ctx, sc, opts), mrt.DeviceScene(gpu_ctx, sc, opts)
    built_a, rep = _audit(a, tag + " A built", presplit=False)
    built_b, _ = _audit(b, tag + " B built", presplit=False)
    assert rep.counts["trees"] == 2 and rep.counts["packets"] == 14
    inst = R.decode_instances(built_a["instances"])
    assert len(set(inst["node_base"][0::2])) == 1 and len(set(inst["node_base"][1::2])) == 1, "instances that share a BLAS name one root"
    quad_root = built_a["rope_nodes"][inst["node_base"][1]]
    print(f"{tag}: the quad's BLAS root is {'a leaf' if quad_root[3] & R.NODE_LEAF else 'internal'}; box BLAS nodes {int(inst['node_base'][1]) - int(inst['node_base'][0])}")
    # scene A: the commit path
    _host_update(mrt, a, BOX, 0, commit=False); _host_update(mrt, a, QUAD, 0)
    assert a.refits == 1
    refit_a, _ = _audit(a, tag + " A refitted by the commit", presplit=False, before=built_a)
    assert not np.array_equal(refit_a["rope_nodes"][:, :8], built_a["rope_nodes"][:, :8])
    _host_move(a, 0, _poses(n, 0))
    moved_a, _ = _audit(a, tag + " A after a transform-only commit", presplit=False, before=built_a)
    _same_rope(refit_a, moved_a, tag + " transform-only commit")
    # scene B: the device entries
    keep = [_dev_update(mrt, b, gpu_ctx, BOX, 0), _dev_update(mrt, b, gpu_ctx, QUAD, 0)]
    b.refit_blas_device()
    torch.cuda.synchronize()
    refit_b, _ = _audit(b, tag + " B refitted through the device entry", presplit=False, before=built_b)
    poses = _t(_poses(n, 0), gpu_ctx)
    b.set_instance_transforms_device(0, poses); b.rebuild_tlas_device()
    torch.cuda.synchronize()
    moved_b, _ = _audit(b, tag + " B after a device TLAS rebuild", presplit=False, before=built_b)
    _same_rope(refit_b, moved_b, tag + " device TLAS rebuild")
    assert b.device_updates_rejected == 0
    del keep, poses
    a.close(); b.close()
