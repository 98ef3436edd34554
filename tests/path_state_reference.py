"""numpy restatement of the four path-state stages on device buffers (include/mrt_abi.h mrt_context_reset_paths_device / _advance_paths_device / _deposit_light_device /
_fold_sample_device; csrc/paths.hip): the bookkeeping between the stage entries — throughput x colour (Raytracing.metal:339), emission along the path,
the keep masks of a bounce's two compactions, radiance += light x throughput where the shadow ray got through (:371-373) and the running average (:395-401).

TEST INFRASTRUCTURE.  float32 throughout, one operation per numpy call in the order written here (numpy rounds each one: no contraction).  Rows are those of
surface_reference.py (SURFACE_DTYPE, or the same 64 bytes as (n, 16) float32) and stages_materials_reference.py (LOBE_DTYPE, or (n, 8) float32); throughput, light and
radiance rows are (., 4) float32; pixel and count words are read as unsigned.  No function changes an argument: each returns new arrays, and rows from
m = min(n, count) on — and every image row no row names — come back as they went in.  tests/test_paths_device_cpu.py pins all of it to the oracle's image with no GPU
(composed_frame below); tests/test_paths_device.py compares the kernels with it bit for bit."""
import numpy as np

f32 = np.float32


def _f(rows, width):
    """structured rows or a float32 array -> (n, width) float32 over the same bytes"""
    a = np.ascontiguousarray(rows)
    if a.dtype != np.float32: a = a.view(np.float32)
    return a.reshape(-1, width)


def _i(col):
    return _f(col, 1).reshape(-1).view(np.int32)


def rows_in_use(n, count):
    """m: the count word is unsigned, so one that is too large — or negative — is clamped to n"""
    return n if count is None else min(n, int(count) & 0xFFFFFFFF)


def _deposit(radiance, pixel, rows, term):
    """radiance[pixel[rows]].rgb + term[rows], for the rows whose pixel lies in the image; a pixel may occur once"""
    out = radiance.copy()
    p = pixel.view(np.uint32)[rows].astype(np.int64)
    inside = p < radiance.shape[0]
    p, rows = p[inside], rows[inside]
    assert np.unique(p).size == p.size, "a pixel occurs twice among the rows of one call: the sum is unspecified"
    out[p, 0:3] = radiance[p, 0:3] + term[rows]
    return out


def reset_paths(n, npixels=None):
    """-> throughput (n, 4) of ones, pixel (n,) int32 = 0 .. n - 1, radiance (npixels, 4) of zeros (None when npixels is None)"""
    return np.ones((n, 4), f32), np.arange(n, dtype=np.int32), None if npixels is None else np.zeros((npixels, 4), f32)


def advance_paths(throughput, light, surfaces=None, lobes=None, pixel=None, radiance=None, count=None, keep_shadow=None, keep_path=None):
    """-> dict: throughput, radiance (None in the diffuse form without one), keep_shadow, keep_path — (n,) uint8 each, the arrays given (what the buffers held before the
    call; zeros when None) with the rows < m written as 0 or 1"""
    assert (surfaces is None) != (lobes is None), "exactly one of surfaces / lobes"
    thr = _f(throughput, 4).copy(); light = _f(light, 4)
    n = thr.shape[0]
    m = rows_in_use(n, count)
    ks = np.zeros(n, np.uint8) if keep_shadow is None else np.array(keep_shadow, np.uint8)
    kp = np.zeros(n, np.uint8) if keep_path is None else np.array(keep_path, np.uint8)
    rad = None if radiance is None else _f(radiance, 4).copy()
    wanted = light[:m, 3] == f32(1.0)
    if surfaces is not None:
        s = _f(surfaces, 16)
        on = s[:m, 7].view(np.int32) == 1
        thr[:m, 0:3] = thr[:m, 0:3] * s[:m, 8:11]
        kp[:m] = on
        ks[:m] = on & wanted
    else:
        l = _f(lobes, 8)
        lobe = l[:m, 3].view(np.int32)
        e = thr[:m, 0:3] * l[:m, 4:7]                                  # the throughput before its update
        rad = _deposit(rad, _i(pixel), np.flatnonzero(lobe != 0), e)
        thr[:m, 0:3] = thr[:m, 0:3] * l[:m, 0:3]
        kp[:m] = (lobe >= 1) & (lobe <= 4)
        ks[:m] = wanted
    return dict(throughput=thr, radiance=rad, keep_shadow=ks, keep_path=kp)


def deposit_light(occluded, light, throughput, pixel, radiance, count=None):
    """-> radiance with light.rgb * throughput.rgb added at the pixels of the rows < m whose shadow ray got through"""
    occ = _i(occluded); light = _f(light, 4); thr = _f(throughput, 4)
    m = rows_in_use(occ.shape[0], count)
    term = light[:m, 0:3] * thr[:m, 0:3]
    return _deposit(_f(radiance, 4), _i(pixel), np.flatnonzero(occ[:m] == 0), term)


def fold_sample(sample, accum, frame_index, clear_sample=False):
    """-> (sample, accum) after the call: the running average as stages_reference.running_average takes a step, accum.w = 1, the sample zeroed on request"""
    s = _f(sample, 4); a = _f(accum, 4).copy()
    f = int(frame_index)
    assert 0 <= f < 2 ** 32 - 1
    if f == 0:
        a[:, 0:3] = s[:, 0:3]
    else:
        c = s[:, 0:3] + a[:, 0:3] * f32(f)
        a[:, 0:3] = c / f32(f + 1)
    a[:, 3] = f32(1.0)
    return (np.zeros_like(s) if clear_sample else s.copy()), a


def composed_frame(orc, c, sample_index, bounces, materials=False, info=None):
    """One frame of the integrator ON QUEUES, composed from the reference stages (stages_reference / stages_materials_reference), the oracle's two queries and the
    functions above; numpy's boolean indexing stands in for the compaction.  c: a scene_case of either module.  -> the frame's radiance sample (h * w, 4) float32.
    info: a dict that receives 'counts' (the path queue's length after each bounce but the last), 'lobes' (the set of lobe codes met) and 'emitted' (whether a non-zero
    emission term was deposited)"""
    import stages_materials_reference as M
    import stages_reference as R
    import surface_reference as S
    w, h, osc, ref, lights = c["w"], c["h"], c["osc"], c["ref"], c["scene"].lights
    rays, hidx = R.primary_rays(orc, c["scene"].camera, w, h, S.SEED, sample_index)
    n = w * h
    thr, pix, rad = reset_paths(n, n)
    if info is not None: info.update(counts=[], lobes=set(), emitted=False)
    for b in range(bounces):
        k = rays.shape[0]
        surf = ref.resolve(rays, osc.intersect_closest(rays)) if k else R.miss_rows(0)
        if materials:
            st = M.scatter_materials(orc, c["table"], rays, surf, hidx, b, bounces, lights)
            a = advance_paths(thr, st["light"], lobes=st["lobes"], pixel=pix, radiance=rad)
            if info is not None:
                info["lobes"] |= set(st["lobes"]["lobe"].tolist())
                info["emitted"] |= bool((thr[:, 0:3] * st["lobes"]["emission"])[st["lobes"]["lobe"] != 0].any())
            rad = a["radiance"]
        else:
            st = R.scatter(orc, surf, hidx, b, lights)
            a = advance_paths(thr, st["light"], surfaces=surf)
        thr = a["throughput"]
        ks, kp = a["keep_shadow"] != 0, a["keep_path"] != 0
        if ks.any():
            occ = osc.intersect_any(st["shadow_rays"][ks])
            rad = deposit_light(occ, st["light"][ks], thr[ks], pix[ks], rad)
        if b + 1 < bounces:
            rays, hidx, pix, thr = st["next_rays"][kp], hidx[kp], pix[kp], thr[kp]
            if info is not None: info["counts"].append(int(kp.sum()))
    return rad
