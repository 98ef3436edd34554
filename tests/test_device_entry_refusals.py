"""What the eleven stream-ordered entries (and update_mesh, whose argument checks they share) answer when they refuse: the status AND the text of mrt_last_error, compared
with tests/golden/device_entry_refusals.json.  The parity tests pin what an accepted call computes; this pins which refusal a call gets and, where two apply at once,
which of them wins: in the three device-update families the scene is looked at before the buffers, in the surface and scatter entries the plain arguments come first.

Everything goes through `lib`, so that arguments the Python layer would stop (a misaligned pointer, an odd stride) reach the library.  Every call here is refused
before anything is launched; the buffers are nevertheless large enough for every count a call names.  The scenes are test_instances_device._case(mrt, 2) — the
12-triangle box and the 2-triangle quad — flattened and two-level, one of them never committed and one with a host change pending, and a quad with one instance of it
(a mesh id that names an instance).

MRT_RECORD_REFUSALS=1 in the environment rewrites the golden file from what the library answers (run so on the commit BEFORE a change to the entry layer); without
it the file is only read."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_fuzz_geometry import _material
from test_instances_device import _case, _quad_mesh

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_entry_refusals.json")
BOX, QUAD, NV = 0, 1, 24          # mesh ids of the case; the box's vertex count
N = 4                             # rows of the surface and scatter calls


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_scene(mrt, gpu_ctx, options, instance, commit=True):
    """a scene made through `lib` alone: the quad, `instance` more meshes that are instances of it, the options; returns its handle"""
    lib = mrt.lib
    h = C.c_void_p()
    assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
    for k, v in options.items(): assert lib.mrt_scene_set_option(h, k.encode(), float(v)) == 0
    qp, qn, qi = _quad_mesh()
    xf = np.eye(4, dtype=np.float32).reshape(16)
    mat = _material(mrt, (0.2, 0.4, 0.8))
    assert lib.mrt_scene_add_mesh(h, _ptr(qp), 12, _ptr(qn), 12, len(qp), _ptr(xf), None) == 0
    assert lib.mrt_mesh_add_submesh(h, 0, _ptr(qi), len(qi), C.byref(mat), None) == 0
    for k in range(instance):
        xf2 = xf.copy(); xf2[12:15] = (3.0 * (k + 1), 0.0, 0.0)
        assert lib.mrt_scene_add_instance(h, 0, _ptr(xf2), None) == 0
    if commit: assert lib.mrt_scene_commit(h) == 0
    return h


def _answers(mrt, gpu_ctx):
    """{case name: [status, message]} of every refusal, in a fixed order"""
    import torch
    lib = mrt.lib
    sc, meshes, _ = _case(mrt, 2)
    dev = torch.device("cuda", gpu_ctx.device)
    pos = torch.from_numpy(np.ascontiguousarray(meshes[BOX][0], np.float32)).to(dev); nrm = torch.from_numpy(np.ascontiguousarray(meshes[BOX][1], np.float32)).to(dev)
    assert tuple(pos.shape) == (NV, 3)
    P, Q = pos.data_ptr(), nrm.data_ptr()
    xf = torch.eye(4, device=dev).reshape(1, 16).repeat(2, 1).contiguous()
    X = xf.data_ptr()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)          # ten 1-KiB pieces: N rows of the widest record (64 bytes) fit four times over
    RAYS, HITS, SURF, HALTON, SHADOW, LIGHT, NEXT, LOBES, ATTR, OUT = (buf.data_ptr() + 1024 * k for k in range(10))
    assert buf.data_ptr() % 256 == 0
    h_pos, h_nrm = np.ascontiguousarray(meshes[BOX][0], np.float32), np.ascontiguousarray(meshes[BOX][1], np.float32)
    bad_pos = h_pos.copy(); bad_pos[5, 1] = np.nan

    flat = mrt.DeviceScene(gpu_ctx, sc)
    two = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    flat_norefit = mrt.DeviceScene(gpu_ctx, sc, {"refit": 0})
    two_norefit = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1, "refit": 0})
    two_nowide = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1, "wide": 0})
    pending = mrt.DeviceScene(gpu_ctx, sc)
    pending.update_mesh(BOX, h_pos, h_nrm)          # a host change no commit followed
    pending_two = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    pending_two.set_instance_transform(QUAD, np.eye(4, dtype=np.float32).reshape(16) * np.float32(0.5))
    singular = mrt.DeviceScene(gpu_ctx, sc, {"instancing": 1})
    singular.set_instance_transform(QUAD, np.zeros(16, np.float32)); singular.commit()          # the quad is not in the TLAS of this commit
    dark = mrt.DeviceScene(gpu_ctx, sc)
    dark.set_lights([])
    assert flat.stats.triangles == 14 and two.stats.triangles == 14
    raw = {k: _raw_scene(mrt, gpu_ctx, o, i, c) for k, (o, i, c) in {
        "uncommitted": ({}, 0, False), "flat_inst": ({}, 1, True), "two_inst": ({"instancing": 1}, 1, True)}.items()}
    empty, empty_two = C.c_void_p(), C.c_void_p()
    for h, o in ((empty, {}), (empty_two, {"instancing": 1})):          # committed, and nothing in them
        assert lib.mrt_scene_create(gpu_ctx.handle, C.byref(h)) == 0
        for k, v in o.items(): assert lib.mrt_scene_set_option(h, k.encode(), float(v)) == 0
        assert lib.mrt_scene_commit(h) == 0
    UNC, FI, TI = raw["uncommitted"], raw["flat_inst"], raw["two_inst"]

    out = {}

    def note(name, rc):
        assert name not in out, name
        assert rc != 0, f"{name}: the call was accepted"
        out[name] = [int(rc), lib.mrt_last_error().decode()]

    def um(h, mesh=BOX, p=P, ps=12, q=Q, qs=12, nv=NV): return lib.mrt_scene_update_mesh_device(h, mesh, p, ps, q, qs, nv, None)
    def ub(h, mesh=BOX, p=P, ps=12, q=Q, qs=12, nv=NV): return lib.mrt_scene_update_blas_device(h, mesh, p, ps, q, qs, nv, None)
    def hm(h, mesh=BOX, p=_ptr(h_pos), ps=12, q=_ptr(h_nrm), qs=12, nv=NV): return lib.mrt_scene_update_mesh(h, mesh, p, ps, q, qs, nv)
    def si(h, first=0, count=2, p=X, stride=64): return lib.mrt_scene_set_instance_transforms_device(h, first, count, p, stride, None)
    def rh(h, rays=RAYS, hits=HITS, n=N, surf=SURF): return lib.mrt_scene_resolve_hits_device(h, rays, hits, n, surf, None)
    def ip(h, hits=HITS, n=N, attr=ATTR, astride=4, ch=1, o=OUT, ostride=4): return lib.mrt_scene_interpolate_device(h, hits, n, attr, astride, ch, o, ostride, None)
    def sd(h, surf=SURF, hal=HALTON, n=N, bounce=0, lc=0, sh=SHADOW, li=LIGHT, nx=NEXT): return lib.mrt_scene_scatter_device(h, surf, hal, n, bounce, lc, sh, li, nx, None)
    def sm(h, rays=RAYS, surf=SURF, hal=HALTON, n=N, bounce=0, mb=4, lc=0, sh=SHADOW, li=LIGHT, nx=NEXT, lo=LOBES):
        return lib.mrt_scene_scatter_materials_device(h, rays, surf, hal, n, bounce, mb, lc, sh, li, nx, lo, None)

    # ---- the three device-update families: the scene first (NULL, not committed, changes pending, the wrong form, refit = 0, nothing to refit), then the arguments
    scene_cases = {"null": None, "uncommitted": UNC, "pending": pending.handle, "pending_two": pending_two.handle}
    families = {
        "update_mesh_device": (um, {"two_level": two.handle, "refit_0": flat_norefit.handle, "empty": empty}),
        "refit_device": (lambda h: lib.mrt_scene_refit_device(h, None), {"two_level": two.handle, "refit_0": flat_norefit.handle, "empty": empty}),
        "set_instance_transforms_device": (si, {"flat": flat.handle, "empty": empty_two}),
        "refit_instances_device": (lambda h: lib.mrt_scene_refit_instances_device(h, None), {"flat": flat.handle, "empty": empty_two}),
        "rebuild_tlas_device": (lambda h: lib.mrt_scene_rebuild_tlas_device(h, None), {"flat": flat.handle, "empty": empty_two}),
        "update_blas_device": (ub, {"flat": flat.handle, "refit_0": two_norefit.handle, "wide_0": two_nowide.handle}),
        "refit_blas_device": (lambda h: lib.mrt_scene_refit_blas_device(h, None), {"flat": flat.handle, "refit_0": two_norefit.handle, "wide_0": two_nowide.handle}),
    }
    for entry, (fn, forms) in families.items():
        for name, h in {**scene_cases, **forms}.items(): note(f"{entry}/{name}", fn(h))
    vertex_args = {"null_positions": dict(p=None), "null_normals": dict(q=None), "mesh_-1": dict(mesh=-1), "mesh_2": dict(mesh=2), "pos_stride_8": dict(ps=8), "nrm_stride_14": dict(qs=14),
                   "pos_stride_0": dict(ps=0), "positions_misaligned": dict(p=P + 2), "normals_misaligned": dict(q=Q + 1), "count_23": dict(nv=NV - 1), "count_0": dict(nv=0),
                   # two at once: the earlier check wins
                   "mesh_2+stride_8": dict(mesh=2, ps=8), "stride_14+misaligned": dict(ps=14, p=P + 2), "misaligned+count_23": dict(p=P + 2, nv=NV - 1), "null+mesh_9": dict(p=None, mesh=9)}
    for entry, fn, good, inst, other in (("update_mesh_device", um, flat.handle, FI, two.handle), ("update_blas_device", ub, two.handle, TI, flat.handle)):
        for name, kw in vertex_args.items(): note(f"{entry}/{name}", fn(good, **kw))
        note(f"{entry}/instance_target", fn(inst, mesh=1, nv=4))
        note(f"{entry}/instance_target+count", fn(inst, mesh=1, nv=5))
        note(f"{entry}/wrong_form+mesh_9", fn(other, mesh=9))          # the scene before the arguments
        note(f"{entry}/uncommitted+null_buffers", fn(UNC, p=None, q=None))
    for name, kw in vertex_args.items():
        if "misaligned" not in name: note(f"update_mesh/{name}", hm(flat.handle, **kw))          # (host arrays may lie anywhere)
    note("update_mesh/null_scene", hm(None))
    note("update_mesh/instance_target", hm(FI, mesh=1, nv=4))
    note("update_mesh/not_finite", hm(flat.handle, p=_ptr(bad_pos)))
    note("update_mesh/count_23+not_finite", hm(flat.handle, p=_ptr(bad_pos), nv=NV - 1))
    for name, kw in {"first_-1": dict(first=-1), "first_2_count_1": dict(first=2, count=1), "count_3": dict(count=3), "null_buffer": dict(p=None), "stride_60": dict(stride=60),
                     "stride_66": dict(stride=66), "misaligned": dict(p=X + 2), "count_3+stride_60": dict(count=3, stride=60), "null_buffer+stride_60": dict(p=None, stride=60),
                     "stride_66+misaligned": dict(stride=66, p=X + 2)}.items():
        note(f"set_instance_transforms_device/{name}", si(two.handle, **kw))
    note("set_instance_transforms_device/not_in_tlas", si(singular.handle))
    note("set_instance_transforms_device/not_in_tlas_alone", si(singular.handle, first=QUAD, count=1))
    note("set_instance_transforms_device/misaligned+not_in_tlas", si(singular.handle, p=X + 2))
    note("set_instance_transforms_device/flat+null_buffer", si(flat.handle, p=None))

    # ---- the surface entries: the plain arguments first, then the scene
    for name, kw in {"null_rays": dict(rays=None), "null_surfaces": dict(surf=None), "rays_misaligned": dict(rays=RAYS + 8), "hits_misaligned": dict(hits=HITS + 4), "surfaces_misaligned": dict(surf=SURF + 4),
                     "too_many": dict(n=1 << 31), "null_rays+hits_misaligned": dict(rays=None, hits=HITS + 4)}.items():
        note(f"resolve_hits_device/{name}", rh(UNC if name == "too_many" else flat.handle, **kw))
    note("resolve_hits_device/null_scene", rh(None))
    note("resolve_hits_device/uncommitted", rh(UNC))
    note("resolve_hits_device/misaligned+uncommitted", rh(UNC, rays=RAYS + 8))
    for name, kw in {"channels_0": dict(ch=0), "channels_65": dict(ch=65, astride=260, ostride=260), "attr_stride_below": dict(ch=2, astride=4, ostride=8), "out_stride_below": dict(ch=2, astride=8, ostride=4),
                     "attr_stride_odd": dict(astride=6), "out_stride_odd": dict(ostride=7), "null_hits": dict(hits=None), "null_out": dict(o=None), "hits_misaligned": dict(hits=HITS + 4),
                     "attr_misaligned": dict(attr=ATTR + 2), "out_misaligned": dict(o=OUT + 1), "too_many": dict(n=1 << 31), "channels_0+null_hits": dict(ch=0, hits=None),
                     "stride_odd+hits_misaligned": dict(astride=6, hits=HITS + 4)}.items():
        note(f"interpolate_device/{name}", ip(UNC if name == "too_many" else flat.handle, **kw))
    note("interpolate_device/null_scene", ip(None))
    note("interpolate_device/uncommitted", ip(UNC))
    note("interpolate_device/channels_65+uncommitted", ip(UNC, ch=65, astride=260, ostride=260))

    # ---- the scatter entries: as the surface entries, then the lights
    shared = {"null_surfaces": dict(surf=None), "null_light": dict(li=None), "surfaces_misaligned": dict(surf=SURF + 4), "next_rays_misaligned": dict(nx=NEXT + 8), "halton_misaligned": dict(hal=HALTON + 2),
              "bounce_-1": dict(bounce=-1), "light_count_-1": dict(lc=-1), "too_many": dict(n=1 << 31), "light_count_3": dict(lc=3), "null_light+bounce_-1": dict(li=None, bounce=-1),
              "halton_misaligned+light_count_-1": dict(hal=HALTON + 2, lc=-1), "bounce_-1+light_count_3": dict(bounce=-1, lc=3)}
    for entry, fn, more in (("scatter_device", sd, {"bounce_19": dict(bounce=19)}),
                            ("scatter_materials_device", sm, {"null_rays": dict(rays=None), "null_lobes": dict(lo=None), "rays_misaligned": dict(rays=RAYS + 4), "lobes_misaligned": dict(lo=LOBES + 4),
                                                              "max_bounces_0": dict(mb=0), "max_bounces_17": dict(mb=17, bounce=16), "bounce_4_of_4": dict(bounce=4), "max_bounces_0+light_count_-1": dict(mb=0, lc=-1)})):
        for name, kw in {**shared, **more}.items(): note(f"{entry}/{name}", fn(UNC if name == "too_many" else flat.handle, **kw))
        note(f"{entry}/null_scene", fn(None))
        note(f"{entry}/uncommitted", fn(UNC))
        note(f"{entry}/bounce_-1+uncommitted", fn(UNC, bounce=-1))
        note(f"{entry}/uncommitted+light_count_3", fn(UNC, lc=3))
        note(f"{entry}/no_lights", fn(dark.handle))
        note(f"{entry}/no_lights_n_0", fn(dark.handle, n=0))
        note(f"{entry}/no_lights+light_count_1", fn(dark.handle, lc=1))

    torch.cuda.synchronize()
    for ds in (flat, two, flat_norefit, two_norefit, two_nowide, pending, pending_two, singular, dark):
        assert ds.device_updates_rejected == 0          # nothing reached the device
        ds.close()
    for h in (*raw.values(), empty, empty_two): assert lib.mrt_scene_destroy(h) == 0
    return out


def test_every_refusal_keeps_its_status_and_text(mrt, gpu_ctx):
    got = _answers(mrt, gpu_ctx)
    if os.environ.get("MRT_RECORD_REFUSALS") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True); f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    for k, (g, w) in wrong.items(): print(f"{k}:\n  now  {g}\n  then {w}")
    assert not wrong, f"{len(wrong)} of {len(want)} refusals changed: {sorted(wrong)}"
    # the three families look at the scene before the buffers; the surface and scatter entries at the plain arguments before the scene
    for entry in ("update_mesh_device", "update_blas_device"):
        assert want[f"{entry}/uncommitted+null_buffers"] == want[f"{entry}/uncommitted"] and want[f"{entry}/wrong_form+mesh_9"][0] == 7
    assert want["set_instance_transforms_device/flat+null_buffer"] == want["set_instance_transforms_device/flat"]
    assert want["resolve_hits_device/misaligned+uncommitted"] == want["resolve_hits_device/rays_misaligned"]
    assert want["interpolate_device/channels_65+uncommitted"] == want["interpolate_device/channels_65"]
    for entry in ("scatter_device", "scatter_materials_device"):
        assert want[f"{entry}/bounce_-1+uncommitted"] == want[f"{entry}/bounce_-1"] and want[f"{entry}/uncommitted+light_count_3"] == want[f"{entry}/uncommitted"]
