"""numpy restatement of the edge-avoiding a-trous filter (include/mrt_abi.h mrt_renderer_denoise; Dammertz et al. 2010) and of the first-hit
guide buffers it reads (MRT_GUIDE_*), the latter built from the CPU oracle's stage dumps.

TEST INFRASTRUCTURE.  `denoise_reference` is the specification the kernels of csrc/denoise.hip follow: float32 throughout, every operation in
the order written here, vectorised over the pixels with a Python loop over the 25 taps.  With dtype=np.float64 the same expressions are evaluated
in double precision (the quality test compares both)."""
import numpy as np

B5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
DEFAULTS = dict(iterations=5, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.25, demodulate=1)      # == MRT_DENOISE_DEFAULT_* (include/mrt_abi.h)


def _lum(c, dt):
    return (dt(0.2126) * c[..., 0] + dt(0.7152) * c[..., 1]) + dt(0.0722) * c[..., 2]


def denoise_reference(accum, normal_depth, albedo, iterations=5, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=1, dtype=np.float32):
    """accum, normal_depth, albedo: (h, w, 4) float32 as Renderer.accumulation() / Renderer.guides() return them -> (h, w, 4) denoised image."""
    dt = dtype
    f32 = np.float32
    # the parameters are float32 numbers (MRTDenoiseParams) whatever the precision of the evaluation
    sigma_color = dt(f32(DEFAULTS["sigma_color"] if sigma_color is None else sigma_color))
    sigma_normal = dt(f32(DEFAULTS["sigma_normal"] if sigma_normal is None else sigma_normal))
    sigma_depth = dt(f32(DEFAULTS["sigma_depth"] if sigma_depth is None else sigma_depth))
    assert 1 <= iterations <= 8
    acc = np.asarray(accum, np.float32).astype(dt)
    nd = np.asarray(normal_depth, np.float32).astype(dt)
    alb = np.asarray(albedo, np.float32).astype(dt)
    h, w = acc.shape[:2]
    cov = alb[..., 3] != 0
    A = np.where(cov[..., None], np.maximum(alb[..., :3], dt(f32(1e-3))), dt(1)) if demodulate else np.ones((h, w, 3), dt)          # coverage 0: A = 1, the pixel is copied through to the bit
    one, zero = dt(1), dt(0)
    with np.errstate(all="ignore"):
        I = acc[..., :3] / A
        for it in range(iterations):
            step = 1 << it
            fstep = dt(step)
            sc = sigma_color / fstep
            P = 2 * step
            Ipad = np.zeros((h + 2 * P, w + 2 * P, 3), dt); Ipad[P:P + h, P:P + w] = I
            ndpad = np.zeros((h + 2 * P, w + 2 * P, 4), dt); ndpad[P:P + h, P:P + w] = nd
            cpad = np.zeros((h + 2 * P, w + 2 * P), bool); cpad[P:P + h, P:P + w] = cov
            lum_p = _lum(I, dt)
            zden = (sigma_depth * nd[..., 3]) * fstep
            s = np.zeros((h, w, 3), dt)
            ws = np.zeros((h, w), dt)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, x0 = P + dy * step, P + dx * step
                    Iq = Ipad[y0:y0 + h, x0:x0 + w]
                    hk = dt(f32(B5[dy + 2]) * f32(B5[dx + 2]))
                    if dy == 0 and dx == 0:
                        wgt = np.full((h, w), hk, dt)
                        valid = np.ones((h, w), bool)
                    else:
                        nq = ndpad[y0:y0 + h, x0:x0 + w]
                        valid = cpad[y0:y0 + h, x0:x0 + w]
                        dot = (nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2]
                        xn = (one - np.maximum(zero, dot)) / sigma_normal
                        xz = np.abs(nd[..., 3] - nq[..., 3]) / zden
                        xc = np.abs(lum_p - _lum(Iq, dt)) / sc
                        kn = np.maximum(zero, one - xn); kz = np.maximum(zero, one - xz); kc = np.maximum(zero, one - xc)
                        wgt = ((hk * (kn * kn)) * (kz * kz)) * (kc * kc)
                    s = np.where(valid[..., None], s + wgt[..., None] * Iq, s)
                    ws = np.where(valid, ws + wgt, ws)
            I = np.where(cov[..., None], s / ws[..., None], I)
        out = np.empty((h, w, 4), dt)
        out[..., :3] = I * A
        out[..., 3] = one
    return out


def guides_from_dump(dump, ids, scene):
    """One frame's guide contribution from the oracle's stage dump (OracleRenderer.render(dump=True): record 0 = the primary ray) and the
    intersection records of the dumped rays: -> normal_depth (h, w, 4) f32, albedo (h, w, 4) f32, ids (h, w, 4) i32."""
    h, w = dump.shape[:2]
    rec = dump[:, :, 0, :]
    hit = rec[..., 7].view(np.uint32) != 0xFFFFFFFF
    nd = np.zeros((h, w, 4), np.float32); al = np.zeros((h, w, 4), np.float32); idb = np.zeros((h, w, 4), np.int32)
    nd[..., :3] = np.where(hit[..., None], rec[..., 8:11], 0.0)
    nd[..., 3] = np.where(hit, rec[..., 6], 0.0)
    ids = ids.reshape(h, w)
    assert np.array_equal(ids["type"] != 0, hit)
    table = np.zeros((len(scene.meshes), max(len(m.submeshes) for m in scene.meshes), 3), np.float32)
    for i, m in enumerate(scene.meshes):
        for g, sm in enumerate(m.submeshes):
            table[i, g] = np.asarray(sm.material.baseColor.tolist()[:3], np.float32)
    al[..., :3] = np.where(hit[..., None], table[np.maximum(ids["instance_id"], 0), np.maximum(ids["geometry_id"], 0)], 0.0)
    al[..., 3] = hit.astype(np.float32)
    idb[..., 0] = ids["type"]; idb[..., 1] = ids["instance_id"]; idb[..., 2] = ids["geometry_id"]; idb[..., 3] = ids["primitive_id"]
    return nd, al, idb


def dump_rays(dump):
    """(h * w, 8) float32 query rays [origin, tmin = 0, direction, tmax = inf] of the dumped primary rays."""
    h, w = dump.shape[:2]
    rays = np.zeros((h * w, 8), np.float32)
    rays[:, 0:3] = dump[:, :, 0, 0:3].reshape(-1, 3); rays[:, 4:7] = dump[:, :, 0, 3:6].reshape(-1, 3); rays[:, 7] = np.inf
    return rays


def running_average(old, new, frame_index):
    """The accumulation buffer's rule (Raytracing.metal:395-401) in float32, per component."""
    if frame_index == 0:
        return new.copy()
    fi, den = np.float32(frame_index), np.float32(frame_index + 1)
    return ((new + old * fi) / den).astype(np.float32)


def oracle_guides(orr, scene, frames, intersect, owned=None, first_frame=0):
    """Drive an OracleRenderer `frames` frames one at a time and build the three guide buffers from its dumps.  intersect: rays -> intersection
    records (DeviceScene.intersect_closest or OracleScene.intersect_closest); owned: (h, w) bool mask of a shard's pixels (the oracle leaves the
    dump of the others untouched — they stay zero here).  -> (normal_depth, albedo, ids, rays of the last frame)."""
    nd = al = idb = rays = None
    for f in range(frames):
        dump = orr.render(1, dump=True)
        rays = dump_rays(dump)
        if owned is not None:          # the oracle leaves the records of the other shards' pixels empty: a ray that hits nothing in their place
            rays[~owned.ravel()] = np.array([0.0, 1e6, 0.0, 0.0, 0.0, 1.0, 0.0, np.inf], np.float32)
        rec_ids = intersect(rays)
        if owned is not None:
            dump = np.ascontiguousarray(dump).copy()
            dump.view(np.uint32)[~owned, 0, 7] = 0xFFFFFFFF
            rec_ids = rec_ids.copy().reshape(owned.shape); rec_ids["type"][~owned] = 0; rec_ids["instance_id"][~owned] = -1; rec_ids["geometry_id"][~owned] = -1; rec_ids["primitive_id"][~owned] = -1
        n1, a1, i1 = guides_from_dump(dump, rec_ids, scene)
        if owned is not None:
            i1[~owned] = 0
        fi = first_frame + f
        nd = n1 if nd is None and fi == 0 else running_average(np.zeros_like(n1) if nd is None else nd, n1, fi)
        al = a1 if al is None and fi == 0 else running_average(np.zeros_like(a1) if al is None else al, a1, fi)
        idb = i1
    return nd, al, idb, rays
