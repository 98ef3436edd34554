"""numpy restatement of the two path-tracing stages on device buffers (include/mrt_abi.h mrt_renderer_primary_rays_device / mrt_scene_scatter_device; csrc/stages.hip):
where the rays come from (Raytracing.metal:171-221) and what follows a surface in the reference's diffuse path (:272-391) — light pick and evaluation, next-event shadow
ray, cosine-hemisphere bounce.

TEST INFRASTRUCTURE.  float32 throughout, one operation per numpy call in the order written here (numpy rounds each one: no contraction).  halton, seed_hash, hemisphere
(sincos_2pi inside it) and align are the oracle's own (tests/oracle.py); the surface rows are surface_reference.py's.  cos(coneAngle) is libm's cosf, the function both the
oracle and the library call on the host.  tests/test_stages_device_cpu.py pins all of it to the oracle's stage dumps and to its image with no GPU;
tests/test_stages_device.py compares the kernels with it bit for bit."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

import surface_reference as S

f32 = np.float32
INF = f32(np.inf)
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = C.c_float; _libm.cosf.argtypes = [C.c_float]


def _v(p):
    return np.array([p.x, p.y, p.z], f32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _length(a):
    return np.sqrt(_dot(a, a))


def _normalize(a):
    inv = f32(1.0) / np.sqrt(_dot(a, a))
    return a * inv[..., None]


def _saturate(x):
    return np.where(x < f32(0.0), f32(0.0), np.where(x > f32(1.0), f32(1.0), x)).astype(f32)


def _halton(orc, idx, d):
    return np.array([orc.halton(int(i), d) for i in idx], f32)


def halton_index(orc, seed, npix, sample_index):
    """(npix,) int32: the renderer's per-pixel seed plus the sample index, with wrap-around"""
    off = np.array([orc.seed_hash(seed, p) for p in range(npix)], np.uint64)
    return ((off + np.uint64(sample_index & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)


def primary_rays(orc, camera, w, h, seed, sample_index):
    """-> rays (w * h, 8) float32 {camera position | 0, direction | +inf}, halton_index (w * h,) int32; pixel p = y * w + x"""
    n = w * h
    idx = halton_index(orc, seed, n, sample_index)
    r0, r1 = _halton(orc, idx, 0), _halton(orc, idx, 1)                              # :202-203
    p = np.arange(n)
    px = (p % w).astype(f32) + r0; py = (p // w).astype(f32) + r1                     # :204
    uvx = px / f32(w); uvy = py / f32(h)                                              # :207
    uvx = uvx * f32(2.0) - f32(1.0); uvy = uvy * f32(2.0) - f32(1.0)                  # :208
    d = (uvx[:, None] * _v(camera.right) + uvy[:, None] * _v(camera.up)) + _v(camera.forward)   # :216-218
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3] = _v(camera.position); rays[:, 4:7] = _normalize(d); rays[:, 7] = INF
    return rays, idx


def scatter(orc, surfaces, hidx, bounce, lights, light_count=0):
    """surfaces (n,) SURFACE_DTYPE, hidx (n,) int32 -> dict: shadow_rays (n, 8), light (n, 4), next_rays (n, 8) float32 as the entry writes them, and light_index (n,)
    int32 (-1 where the row is no surface)"""
    n = surfaces.shape[0]
    out = dict(shadow_rays=np.zeros((n, 8), f32), light=np.zeros((n, 4), f32), next_rays=np.zeros((n, 8), f32), light_index=np.full(n, -1, np.int32))
    rows = np.flatnonzero(surfaces["type"] == 1)
    if rows.size == 0: return out
    lc = int(light_count) or len(lights)
    assert 1 <= lc <= len(lights) and 0 <= bounce <= 18
    P = surfaces["position"][rows].astype(f32); N = surfaces["normal"][rows].astype(f32); idx = np.asarray(hidx, np.int32)[rows]
    dim0 = 2 + 5 * bounce
    ls = _halton(orc, idx, dim0)                                                      # :272
    li = np.minimum((ls * f32(lc)).astype(np.int32), np.int32(lc - 1))                # :273
    m = rows.size
    ldir = np.zeros((m, 3), f32); lcol = np.zeros((m, 3), f32); ldist = np.zeros(m, f32)
    with np.errstate(all="ignore"):
        for k in range(lc):
            s = np.flatnonzero(li == k)
            if s.size == 0: continue
            L = lights[k]
            col = _v(L.color)
            if L.type == 4:                                                           # area light, :281-290, :94-128
                ax = _halton(orc, idx[s], dim0 + 1) * f32(2.0) - f32(1.0)
                ay = _halton(orc, idx[s], dim0 + 2) * f32(2.0) - f32(1.0)
                sp = (_v(L.position) + _v(L.right) * ax[:, None]) + _v(L.up) * ay[:, None]
                d = sp - P[s]
                dist = _length(d)
                inv = f32(1.0) / np.where(dist > f32(1e-3), dist, f32(1e-3)).astype(f32)
                d = d * inv[:, None]
                c = col * (inv * inv)[:, None]
                c = c * _saturate(_dot(-d, _v(L.forward)))[:, None]
            elif L.type in (2, 3):                                                    # spot :292-316, point :317-322
                d = _v(L.position) - P[s]
                dist = _length(d)
                inv = f32(1.0) / np.where(dist > f32(1e-3), dist, f32(1e-3)).astype(f32)
                d = d * inv[:, None]
                c = (col * inv[:, None]) * inv[:, None]
                if L.type == 2:
                    spot = _dot(-d, _normalize(_v(L.direction)))
                    c = np.where((spot > f32(_libm.cosf(L.coneAngle)))[:, None], c, f32(0.0)).astype(f32)
            else:                                                                     # sun, :323-327
                d = np.broadcast_to(-_normalize(_v(L.direction)), (s.size, 3)).astype(f32)
                dist = np.full(s.size, INF, f32)
                c = np.broadcast_to(col, (s.size, 3)).astype(f32)
            ldir[s] = d; lcol[s] = c; ldist[s] = dist
        lcol = lcol * _saturate(_dot(N, ldir))[:, None]                               # :331
        lcol = lcol * f32(lc)                                                         # :335
        wants = _length(lcol) > f32(0.0001)                                           # :341
        org = P + N * f32(1e-3)                                                       # :350, :390
        smax = ldist - f32(1e-3)                                                      # :356
    hx = _halton(orc, idx, dim0 + 3); hy = _halton(orc, idx, dim0 + 4)                # :384-385
    nd = np.stack([orc.align(orc.hemisphere(hx[j], hy[j]), N[j]) for j in range(m)]).astype(f32)   # :387-388
    sh = np.zeros((m, 8), f32)
    sh[:, 0:3] = org; sh[:, 4:7] = ldir; sh[:, 7] = smax
    sh[~wants] = 0
    out["shadow_rays"][rows] = sh
    out["light"][rows, 0:3] = lcol; out["light"][rows, 3] = wants.astype(f32)
    out["next_rays"][rows, 0:3] = org; out["next_rays"][rows, 4:7] = nd; out["next_rays"][rows, 7] = INF
    out["light_index"][rows] = li
    return out


# ---------------------------------------------------------------- the scenes of the stage tests and the oracle's stage dump of each at a frame index, made once
FOUR_LIGHTS = "four_lights"
CASES = dict(S.CASES)
CASES[FOUR_LIGHTS] = (48, 32, False)          # the scene of test_all_light_types_parity: spot + sun + point + area


def make_scene(mrt, name):
    if name != FOUR_LIGHTS: return S.make_scene(mrt, name)
    w, h, _ = CASES[name]
    sc = mrt.GardenScene((w, h))
    sc.lights = sc.lights + [mrt.Light.pointLight([0, 2.5, 1], [3, 2, 1]), mrt.Scene.setupLight()]
    return sc


@functools.lru_cache(maxsize=None)
def scene_case(mrt, orc, name):
    """-> dict: scene, entries (share=True), ref (SurfaceReference), osc (the OracleScene, left open for its queries), w, h, instancing"""
    w, h, instancing = CASES[name]
    sc = make_scene(mrt, name)
    shared = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(shared if instancing else mrt.flatten_scene(sc), sc.lights, instancing=instancing)
    return dict(scene=sc, entries=shared, ref=S.SurfaceReference(shared), osc=osc, w=w, h=h, instancing=instancing)


@functools.lru_cache(maxsize=None)
def dump_case(mrt, orc, name, frame):
    """the oracle's stage dump of frame index `frame` (the last of frame + 1 rendered frames) -> dict: dump (h * w, 3, 16), accum (h, w, 4) and per bounce b: pixels[b] (the
    pixels whose path reached it), rays[b] (the dumped rays there), hits[b] (the oracle's records for them), surfaces[b] (SurfaceReference.resolve of both)"""
    c = scene_case(mrt, orc, name)
    orr = orc.OracleRenderer(c["osc"], c["w"], c["h"], seed=S.SEED, max_bounces=3, camera=c["scene"].camera)
    dump = orr.render(frame + 1, dump=True).reshape(c["w"] * c["h"], 3, 16)
    out = dict(dump=dump, accum=orr.accumulation(), pixels=[], rays=[], hits=[], surfaces=[])
    orr.close()
    held = np.arange(dump.shape[0])
    for b in range(3):
        if b: held = held[dump[held, b - 1, 7].view(np.uint32) != 0xFFFFFFFF]          # a path reaches bounce b where it hit at b - 1; a record beyond its end is an earlier frame's, or zero
        rec = dump[:, b, :]
        rays = np.zeros((held.size, 8), f32)
        rays[:, 0:3] = rec[held, 0:3]; rays[:, 4:7] = rec[held, 3:6]; rays[:, 7] = np.inf
        hits = c["osc"].intersect_closest(rays)
        surf = c["ref"].resolve(rays, hits)
        for a in (rays, hits, surf): a.setflags(write=False)
        out["pixels"].append(held); out["rays"].append(rays); out["hits"].append(hits); out["surfaces"].append(surf)
    dump.setflags(write=False)
    return out


def miss_rows(n):
    m = np.empty(n, S.SURFACE_DTYPE); m[:] = S.miss_record()
    return m


def composed_frame(orc, c, sample_index, bounces=3):
    """One frame of the integrator composed from the reference stages and the oracle's queries, dense rows: -> the frame's radiance sample (h * w, 3) float32"""
    w, h, osc, ref, lights = c["w"], c["h"], c["osc"], c["ref"], c["scene"].lights
    rays, hidx = primary_rays(orc, c["scene"].camera, w, h, S.SEED, sample_index)
    n = w * h
    thr = np.ones((n, 3), f32); acc = np.zeros((n, 3), f32); alive = np.ones(n, bool)
    for b in range(bounces):
        surf = miss_rows(n)
        rows = np.flatnonzero(alive)
        surf[rows] = ref.resolve(rays[rows], osc.intersect_closest(rays[rows]))
        alive = surf["type"] == 1                                                     # :246-247: a miss ends the path
        st = scatter(orc, surf, hidx, b, lights)
        thr = thr * surf["base_color"]                                                # :339
        want = np.flatnonzero(st["light"][:, 3] == f32(1.0))
        lit = np.zeros(n, bool)
        lit[want] = osc.intersect_any(st["shadow_rays"][want]) == 0                   # :367
        acc = np.where(lit[:, None], acc + st["light"][:, 0:3] * thr, acc)            # :371-373
        rays = st["next_rays"]
    return acc


def running_average(samples):
    """the reference's accumulation (:395-401) of per-frame samples (frames, n, 3) from frame index 0 on -> (n, 3) float32"""
    a = np.asarray(samples[0], f32)
    for f in range(1, len(samples)):
        c = np.asarray(samples[f], f32) + a * f32(f)
        a = c / f32(f + 1)
    return a
