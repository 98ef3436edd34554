"""numpy restatement of the scatter stage with the materials extension on (include/mrt_abi.h mrt_scene_scatter_materials_device; csrc/stages_materials.hip): what follows a
surface when renderer option materials = 1 — the oracle's `if (materials)` block of trace_pixel (emission, the lobe choice, the dielectric interface, the GGX specular
lobe) followed by the diffuse path of stages_reference.scatter.

TEST INFRASTRUCTURE.  float32 throughout, one operation per numpy call in the order written here (numpy rounds each one: no contraction).  halton, sincos_2pi, hemisphere
and align are the oracle's own (tests/oracle.py exposes sincos_2pi itself, so no detour through hemisphere(hx, 0) is needed); the surface rows are surface_reference.py's and
the diffuse rows go through stages_reference.scatter unchanged.  tests/test_stages_materials_device_cpu.py pins all of it to the oracle's stage dumps and to its image with
no GPU; tests/test_stages_materials_device.py compares the kernel with it bit for bit."""
import functools

import numpy as np

import stages_reference as R
import surface_reference as S

f32 = np.float32
INF = f32(np.inf)
LOBE_DTYPE = np.dtype([("weight", np.float32, 3), ("lobe", np.int32), ("emission", np.float32, 3), ("_pad", np.int32)])
MAX_BOUNCES = 4


def material_table(entries):
    """entries: flatten_scene(scene, share=True) 5-tuples -> dict of per-slot arrays (slot = instance * max_sub + geometry): specular (S, 3), emission (S, 3), ns, ni,
    dissolve (S,) float32; `slots` = instances * max_sub.  An instance carries its source's materials; slots no submesh fills stay zero (as the library's table)."""
    subs = [(e[3] if len(e) < 5 or e[4] < 0 else entries[e[4]][3]) for e in entries]
    max_sub = max([len(s) for s in subs] + [1])
    n = len(entries) * max_sub
    t = dict(specular=np.zeros((n, 3), f32), emission=np.zeros((n, 3), f32), ns=np.zeros(n, f32), ni=np.zeros(n, f32), dissolve=np.zeros(n, f32), slots=n, max_sub=max_sub)
    for i, s in enumerate(subs):
        for g, (_, m) in enumerate(s):
            k = i * max_sub + g
            t["specular"][k] = [m.specular.x, m.specular.y, m.specular.z]; t["emission"][k] = [m.emission.x, m.emission.y, m.emission.z]
            t["ns"][k] = m.specularExponent; t["ni"][k] = m.refractionIndex; t["dissolve"][k] = m.dissolve
    return t


def _max3(a):
    return np.maximum(a[:, 0], np.maximum(a[:, 1], a[:, 2]))


def scatter_materials(orc, table, rays, surfaces, hidx, bounce, max_bounces, lights, light_count=0):
    """rays (n, 8) float32, surfaces (n,) SURFACE_DTYPE, hidx (n,) int32 -> dict: shadow_rays (n, 8), light (n, 4), next_rays (n, 8) float32 and lobes (n,) LOBE_DTYPE as
    the entry writes them, and light_index (n,) int32 (-1 where the row is not diffuse)"""
    n = surfaces.shape[0]
    rays = np.asarray(rays, f32).reshape(-1, 8)
    assert rays.shape[0] == n and 1 <= max_bounces <= 16 and 0 <= bounce < max_bounces
    lobes = np.zeros(n, LOBE_DTYPE)
    nxt = np.zeros((n, 8), f32)
    slot = surfaces["resource_slot"].astype(np.int64)
    rows = np.flatnonzero((surfaces["type"] == 1) & (slot >= 0) & (slot < table["slots"]))
    diffuse_surf = R.miss_rows(n)
    if rows.size:
        k = slot[rows]
        P = surfaces["position"][rows].astype(f32); N = surfaces["normal"][rows].astype(f32); surf = surfaces["base_color"][rows].astype(f32)
        D = rays[rows, 4:7]
        idx = np.asarray(hidx, np.int32)[rows]
        spec = table["specular"][k]; ns = table["ns"][k]; ni = table["ni"][k]; dis = table["dissolve"][k]
        m = rows.size
        lobe = np.ones(m, np.int32); weight = np.zeros((m, 3), f32); norg = np.zeros((m, 3), f32); ndir = np.zeros((m, 3), f32)
        dim0 = 2 + 5 * bounce
        with np.errstate(all="ignore"):
            ul = R._halton(orc, idx, 2 + 5 * max_bounces + bounce)
            kd = _max3(surf); ks = _max3(spec)
            trn = np.where((dis > f32(0.0)) & (dis < f32(1.0)) & (ni > f32(0.0)), f32(1.0) - dis, f32(0.0)).astype(f32)
            die = ul < trn
            # ---- the dielectric interface
            u2 = ul / trn
            cd = R._dot(D, N)
            entering = cd < f32(0.0)
            nn = np.where(entering[:, None], N, -N).astype(f32)
            eta = np.where(entering, f32(1.0) / ni, ni).astype(f32)
            cosi = np.where(entering, -cd, cd).astype(f32)
            sin2t = (eta * eta) * (f32(1.0) - cosi * cosi)
            r0 = (f32(1.0) - ni) / (f32(1.0) + ni); r0 = r0 * r0
            ok = sin2t < f32(1.0)
            cost = np.where(ok, np.sqrt(f32(1.0) - sin2t), f32(0.0)).astype(f32)
            c = np.where(entering, cosi, cost).astype(f32)
            x = f32(1.0) - c; x2 = x * x
            F = np.where(ok, r0 + (f32(1.0) - r0) * ((x2 * x2) * x), f32(1.0)).astype(f32)
            refl = u2 < F
            nd_refl = D + nn * (f32(2.0) * cosi)[:, None]; org_refl = P + nn * f32(1e-3)
            nd_refr = D * eta[:, None] + nn * (eta * cosi - cost)[:, None]; org_refr = P + nn * f32(-1e-3)
            nd = np.where(refl[:, None], nd_refl, nd_refr).astype(f32)
            s = np.flatnonzero(die)
            lobe[s] = np.where(refl[s], 2, 3); weight[s] = f32(1.0)
            norg[s] = np.where(refl[s, None], org_refl[s], org_refr[s]); ndir[s] = R._normalize(nd[s])
            # ---- the specular lobe
            ud = np.where(trn > f32(0.0), (ul - trn) / (f32(1.0) - trn), ul).astype(f32)
            ps = np.where((ks > f32(0.0)) & (ns > f32(0.0)), ks / (ks + kd), f32(0.0)).astype(f32)
            s = np.flatnonzero(~die & (ud < ps))
            if s.size:
                hx = R._halton(orc, idx[s], dim0 + 3); hy = R._halton(orc, idx[s], dim0 + 4)
                a2 = f32(2.0) / (ns[s] + f32(2.0))
                ct2 = (f32(1.0) - hy) / (f32(1.0) + (a2 - f32(1.0)) * hy)
                ct = np.sqrt(ct2); st = np.sqrt(f32(1.0) - ct2)
                sc = np.array([orc.sincos_2pi(v) for v in hx], f32).reshape(-1, 2)
                sp_, cp_ = sc[:, 0], sc[:, 1]
                local = np.stack([st * cp_, ct, st * sp_], 1).astype(f32)
                hw = np.stack([orc.align(local[j], N[s[j]]) for j in range(s.size)]).astype(f32)
                dh = R._dot(D[s], hw)
                wi = D[s] - hw * (f32(2.0) * dh)[:, None]
                above = R._dot(wi, N[s]) > f32(0.0)
                lobe[s] = np.where(above, 4, 5)
                w = spec[s] * (f32(1.0) / ps[s])[:, None]
                weight[s] = np.where(above[:, None], w, f32(0.0))
                norg[s] = P[s] + N[s] * f32(1e-3); ndir[s] = R._normalize(wi)
            # ---- the diffuse path
            s = np.flatnonzero(~die & ~(ud < ps))
            scaled = surf * (f32(1.0) / (f32(1.0) - ps))[:, None]
            weight[s] = np.where((ps[s] > f32(0.0))[:, None], scaled[s], surf[s])
        diffuse_surf[rows[s]] = surfaces[rows[s]]
        go = np.flatnonzero((lobe >= 2) & (lobe <= 4))
        nxt[rows[go], 0:3] = norg[go]; nxt[rows[go], 4:7] = ndir[go]; nxt[rows[go], 7] = INF
        lobes["weight"][rows] = weight; lobes["lobe"][rows] = lobe; lobes["emission"][rows] = table["emission"][k]
    st = R.scatter(orc, diffuse_surf, hidx, bounce, lights, light_count)
    d = np.flatnonzero(lobes["lobe"] == 1)
    nxt[d] = st["next_rays"][d]
    return dict(shadow_rays=st["shadow_rays"], light=st["light"], next_rays=nxt, lobes=lobes, light_index=st["light_index"])


# ---------------------------------------------------------------- the scenes of the tests and the oracle's stage dump of each at a frame index, made once
EDGE, EDGE_TWO_LEVEL, CORNELL, PLAIN = "edge", "edge_two_level", "cornell_materials", "cornell_plain"
CASES = {EDGE: (67, 45, False), EDGE_TWO_LEVEL: (67, 45, True), CORNELL: (48, 48, False), PLAIN: (48, 48, False)}          # 67 x 45 = test_materials.EDGE_SIZE
DEVICE_CASES = (EDGE, EDGE_TWO_LEVEL, CORNELL)


def make_scene(mrt, name):
    import material_scenes as M
    w, h, _ = CASES[name]
    if name in (EDGE, EDGE_TWO_LEVEL): return M.edge_material_scene(mrt, (w, h))
    return M.cornell_with_materials(mrt, (w, h), plain=name == PLAIN)


@functools.lru_cache(maxsize=None)
def scene_case(mrt, orc, name):
    """-> dict: scene, entries (share=True), ref (SurfaceReference), table (material_table), osc (the OracleScene, left open for its queries), w, h, instancing"""
    w, h, instancing = CASES[name]
    sc = make_scene(mrt, name)
    shared = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(shared if instancing else mrt.flatten_scene(sc), sc.lights, instancing=instancing)
    return dict(scene=sc, entries=shared, ref=S.SurfaceReference(shared), table=material_table(shared), osc=osc, w=w, h=h, instancing=instancing)


@functools.lru_cache(maxsize=None)
def dump_case(mrt, orc, name, frame):
    """the oracle's stage dump, materials on, of frame index `frame` (the last of frame + 1 rendered frames) -> dict: dump (h * w, MAX_BOUNCES, 16), accum (h, w, 4) and
    per bounce b: pixels[b] (the pixels whose record at b is this frame's: every pixel at frame 0 whose path reached b), rays[b], hits[b] (the oracle's records for them),
    surfaces[b] (SurfaceReference.resolve of both)"""
    c = scene_case(mrt, orc, name)
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=MAX_BOUNCES, camera=c["scene"].camera)
    orr.set_materials(True)
    dump = orr.render(frame + 1, dump=True).reshape(c["w"] * c["h"], MAX_BOUNCES, 16)
    out = dict(dump=dump, accum=orr.accumulation(), pixels=[], rays=[], hits=[], surfaces=[])
    orr.close()
    hidx = R.halton_index(orc, S.SEED, dump.shape[0], frame)
    held = np.arange(dump.shape[0])
    for b in range(MAX_BOUNCES):
        rec = dump[:, b, :]
        rays = np.zeros((held.size, 8), f32)
        rays[:, 0:3] = rec[held, 0:3]; rays[:, 4:7] = rec[held, 3:6]; rays[:, 7] = np.inf
        hits = c["osc"].intersect_closest(rays)
        surf = c["ref"].resolve(rays, hits)
        for a in (rays, hits, surf): a.setflags(write=False)
        out["pixels"].append(held); out["rays"].append(rays); out["hits"].append(hits); out["surfaces"].append(surf)
        # a path reaches bounce b + 1 where the reference says it goes on: it hit at b and was not absorbed (the test pins both to the dump's own records)
        st = scatter_materials(orc, c["table"], rays, surf, hidx[held], b, MAX_BOUNCES, c["scene"].lights)
        held = held[(st["lobes"]["lobe"] >= 1) & (st["lobes"]["lobe"] <= 4)]
    dump.setflags(write=False)
    return out


def composed_frame(orc, c, sample_index, bounces=MAX_BOUNCES):
    """One frame of the materials integrator composed from the reference stages and the oracle's queries, dense rows: -> the frame's radiance sample (h * w, 3) float32"""
    w, h, osc, ref, lights = c["w"], c["h"], c["osc"], c["ref"], c["scene"].lights
    rays, hidx = R.primary_rays(orc, c["scene"].camera, w, h, S.SEED, sample_index)
    n = w * h
    thr = np.ones((n, 3), f32); acc = np.zeros((n, 3), f32); alive = np.ones(n, bool)
    for b in range(bounces):
        surf = R.miss_rows(n)
        rows = np.flatnonzero(alive)
        surf[rows] = ref.resolve(rays[rows], osc.intersect_closest(rays[rows]))
        st = scatter_materials(orc, c["table"], rays, surf, hidx, b, bounces, lights)
        lobe = st["lobes"]["lobe"]
        acc = acc + thr * st["lobes"]["emission"]
        thr = thr * st["lobes"]["weight"]
        want = np.flatnonzero(st["light"][:, 3] == f32(1.0))
        lit = np.zeros(n, bool)
        lit[want] = osc.intersect_any(st["shadow_rays"][want]) == 0
        acc = np.where(lit[:, None], acc + st["light"][:, 0:3] * thr, acc)
        alive = (lobe >= 1) & (lobe <= 4)
        rays = st["next_rays"]
    return acc
