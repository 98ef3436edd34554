"""Cases of the variance-guided a-trous filter (tests/variance_reference.py) shared by tests/test_variance_cpu.py and tests/test_variance_device.py: images
whose answers are known by hand, a one-pixel scalar evaluation of a level that shares no code with the vectorised reference, random images that hold every feature, and
the moved sequences of §10r with their moments.

TEST INFRASTRUCTURE."""
import numpy as np

import temporal_cases as TC
import temporal_reference as T
import variance_reference as V

f32 = np.float32
B5 = [f32(b) for b in V.B5]


# ---------------------------------------------------------------- hand-made images
def flat(w, h, colour=(0.5, 0.25, 0.125), variance=1.0, length=32.0):
    """a constant image on one plane seen head-on: unit axis normals, equal depth, equal luminance — every k is 1 —, m1 = 0 and m2 = variance
    -> dict(image, moments, normal_depth, albedo), each (h, w, 4) float32"""
    img = np.zeros((h, w, 4), f32); img[..., 0:3] = np.asarray(colour, f32); img[..., 3] = f32(7.0)          # (alpha is ignored)
    mom = np.zeros((h, w, 4), f32); mom[..., 1] = f32(variance); mom[..., 2] = f32(-3.0); mom[..., 3] = f32(length)
    nd = np.zeros((h, w, 4), f32); nd[..., 2] = f32(1.0); nd[..., 3] = f32(2.0)
    alb = np.ones((h, w, 4), f32)
    return dict(image=img, moments=mom, normal_depth=nd, albedo=alb)


def halves(w, h, left=0.5, right=0.25, variance=0.0, length=32.0):
    """flat(), the columns from w // 2 on of another grey"""
    c = flat(w, h, (left,) * 3, variance, length)
    c["image"][:, w // 2:, 0:3] = f32(right)
    return c


def run(c, **kw):
    return V.denoise_variance(c["image"], c["moments"], c["normal_depth"], c["albedo"], **kw)


def lum(c):
    return (f32(0.2126) * f32(c[0]) + f32(0.7152) * f32(c[1])) + f32(0.0722) * f32(c[2])


def scalar_level(I, v, nd, x, y, step, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.25):
    """ONE covered pixel of one iteration, written out tap by tap on np.float32 scalars from the header's text -> (I' (3,), v', g).  Shares no code with
    variance_reference.level."""
    h, w = v.shape
    sc, sn, sd = f32(sigma_color), f32(sigma_normal), f32(sigma_depth)
    k = lambda t: max(f32(0.0), f32(1.0) - t)
    gs = gw = f32(0.0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qx, qy = x + dx, y + dy
            if not (0 <= qx < w and 0 <= qy < h) or v[qy, qx] < 0: continue
            wk = f32(0.25) if dx == 0 and dy == 0 else f32(0.125) if dx == 0 or dy == 0 else f32(0.0625)
            gs = gs + wk * v[qy, qx]; gw = gw + wk
    g = gs / gw
    den = sc * np.sqrt(g) + f32(1e-6)
    n_p, t_p = nd[y, x, 0:3], nd[y, x, 3]
    zden = (sd * t_p) * f32(step)
    s = np.zeros(3, f32); vs = ws = f32(0.0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            hk = B5[dy + 2] * B5[dx + 2]
            qx, qy = x + dx * step, y + dy * step
            if dx == 0 and dy == 0: wq = hk
            else:
                if not (0 <= qx < w and 0 <= qy < h) or v[qy, qx] < 0: continue
                n_q, t_q = nd[qy, qx, 0:3], nd[qy, qx, 3]
                dot = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
                kn = k((f32(1.0) - max(f32(0.0), dot)) / sn); kz = k(abs(t_p - t_q) / zden); kc = k(abs(lum(I[y, x]) - lum(I[qy, qx])) / den)
                wq = ((hk * (kn * kn)) * (kz * kz)) * (kc * kc)
            for ch in range(3): s[ch] = s[ch] + wq * I[qy, qx, ch]
            vs = vs + (wq * wq) * v[qy, qx]; ws = ws + wq
    for a in (g, den, vs, ws): assert isinstance(a, np.float32), type(a)
    return s / ws, vs / (ws * ws), g


def scalar_spatial(c, x, y, sigma_normal=0.25, sigma_depth=0.25):
    """the prepass's spatial estimate of ONE covered pixel, tap by tap on np.float32 scalars -> v"""
    mom, nd, alb = c["moments"], c["normal_depth"], c["albedo"]
    h, w = mom.shape[:2]
    sn, sd = f32(sigma_normal), f32(sigma_depth)
    k = lambda t: max(f32(0.0), f32(1.0) - t)
    s1 = s2 = sw = f32(0.0)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            qx, qy = x + dx, y + dy
            if dx == 0 and dy == 0: wq = f32(1.0)
            else:
                if not (0 <= qx < w and 0 <= qy < h) or alb[qy, qx, 3] == 0: continue
                n_p, n_q = nd[y, x], nd[qy, qx]
                dot = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2]
                kn = k((f32(1.0) - max(f32(0.0), dot)) / sn); kz = k(abs(n_p[3] - n_q[3]) / (sd * n_p[3]))
                wq = (kn * kn) * (kz * kz)
            s1 = s1 + wq * mom[qy, qx, 0]; s2 = s2 + wq * mom[qy, qx, 1]; sw = sw + wq
    M1 = s1 / sw; M2 = s2 / sw
    ln = mom[y, x, 3]
    return max(f32(0.0), M2 - M1 * M1) * (f32(4.0) / (ln if ln > 1 else f32(1.0)))


def known_answer_cases():
    """the images whose answers tests/test_variance_cpu.py derives by hand; the GPU test holds the kernels to the reference's bits on them"""
    out = [("flat_v1", flat(12, 11)), ("flat_v0", flat(12, 11, variance=0.0)), ("halves_v0", halves(12, 9)), ("halves_v100", halves(12, 9, variance=100.0)),
           ("flat_len1", flat(9, 9, length=1.0)), ("flat_len2", flat(9, 9, length=2.0)), ("flat_len3999", flat(9, 9, length=3.999)), ("flat_len4", flat(9, 9, length=4.0))]
    c = halves(12, 9, variance=1.0); c["moments"][4, 5, 1] = f32(0.0); out.append(("one_pixel_of_variance_0", c))
    c = flat(11, 11, variance=0.0, length=2.0); c["moments"][..., 0] = f32(0.5) * ((np.arange(11)[None, :] + np.arange(11)[:, None]) % 2).astype(f32)
    c["moments"][..., 1] = c["moments"][..., 0]; out.append(("two_valued_moments", c))          # m1 in {0, 1/2}, m2 = m1: M1 and M2 are exact
    c = nan_behind_uncovered(); out.append(("nan_behind_uncovered", c))
    return out


def nan_behind_uncovered():
    """a flat image with a few pixels that are not covered and hold NaN in image, moments and guide: they pass through, and no covered pixel sees them"""
    c = flat(13, 10, variance=1.0, length=2.0)
    for (y, x) in ((0, 0), (4, 5), (4, 6), (9, 12), (7, 1)):
        c["albedo"][y, x] = (0.3, 0.3, 0.3, 0.0)
        c["image"][y, x, 0:3] = np.nan; c["moments"][y, x] = np.nan; c["normal_depth"][y, x] = np.nan
    return c


# ---------------------------------------------------------------- random images that hold every feature
def random_case(size, seed):
    """covered and uncovered pixels (NaN moments and guides behind the uncovered ones), history lengths on both sides of 4 and a few NaN, zero and large variance, depth
    and normal edges, blocks of colour -> dict(image, moments, normal_depth, albedo), each (h, w, 4) float32"""
    w, h = size
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    block = ((xx // 5) + (yy // 3)) % 3
    img = np.zeros((h, w, 4), f32)
    img[..., 0:3] = (f32(0.2) + f32(0.6) * block[..., None].astype(f32) + rng.random((h, w, 3)).astype(f32) * f32(0.5))
    img[..., 3] = rng.standard_normal((h, w)).astype(f32)
    alb = np.zeros((h, w, 4), f32)
    alb[..., 0:3] = rng.choice(np.array([0.0, 5e-4, 0.2, 0.7, 1.0], f32), (h, w, 3))
    alb[..., 3] = rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 1.0, 1.0], f32), (h, w))
    axes = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8]], f32)
    nrm = axes[((xx // 7) + (yy // 6)) % 3] + rng.standard_normal((h, w, 3)).astype(f32) * f32(0.05)
    nrm = (nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True))).astype(f32)
    nd = np.zeros((h, w, 4), f32); nd[..., 0:3] = nrm
    nd[..., 3] = np.where((xx + yy) % 11 < 8, f32(2.0), f32(3.5)) + (xx * f32(0.02) + rng.random((h, w)).astype(f32) * f32(0.05))
    m1 = V._lum(img[..., 0:3], f32) * (f32(0.8) + rng.random((h, w)).astype(f32) * f32(0.4))
    var = rng.choice(np.array([0.0, 0.0, 1e-4, 0.02, 0.5, 10.0], f32), (h, w)) * rng.random((h, w)).astype(f32)
    mom = np.zeros((h, w, 4), f32)
    mom[..., 0] = m1; mom[..., 1] = m1 * m1 + var; mom[..., 2] = rng.standard_normal((h, w)).astype(f32)
    mom[..., 3] = rng.choice(np.array([1.0, 1.5, 2.0, 3.0, 3.999, 4.0, 4.0, 5.0, 17.25, 32.0, 32.0, np.nan], f32), (h, w))
    un = alb[..., 3] == 0
    mom[un] = np.nan; nd[un & (rng.random((h, w)) < 0.7)] = np.nan
    return dict(image=img, moments=mom, normal_depth=nd, albedo=alb)


# ---------------------------------------------------------------- the moved sequences of §10r, with moments
QUALITY_TWO_LEVEL = dict(size=(64, 48), frames=8, seed=1)          # the two-level scene of test_instancing, the camera a step every frame


def two_level_frames(mrt, orc):
    """tests/temporal_cases.py quality_frames for the two-level scene at 64 x 48 with sequence_camera's step before every frame"""
    import image_stages_reference as IS
    import stages_reference as R
    from test_instancing import _scene
    w, h = QUALITY_TWO_LEVEL["size"]
    sc = _scene(mrt, (w, h))
    entries = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(entries, sc.lights, instancing=True)
    ref = TC.S.SurfaceReference(entries)
    out = []
    try:
        for k in range(QUALITY_TWO_LEVEL["frames"]):
            cam = TC.sequence_camera(mrt, sc.camera, k)
            orr = orc.OracleRenderer(osc, w, h, seed=QUALITY_TWO_LEVEL["seed"], max_bounces=3, camera=cam)
            orr.set_sample_offset(k)
            orr.render(1)
            sample = orr.accumulation().reshape(-1, 4); orr.close()
            rays, _ = R.primary_rays(orc, cam, w, h, QUALITY_TWO_LEVEL["seed"], k)
            surf = ref.resolve(rays, osc.intersect_closest(rays))
            nd, _, ids = IS.fold_guides(surf, None, None, 0)
            out.append((T.camera_rows(cam), surf, sample, (nd, ids)))
        orr = orc.OracleRenderer(osc, w, h, seed=QUALITY_TWO_LEVEL["seed"] + 1, max_bounces=3, camera=cam)
        orr.render(512, threads=4)
        converged = orr.accumulation().reshape(-1, 4); orr.close()
    finally:
        osc.close()
    return out, converged


def accumulate(frames, size, demodulate=1):
    """the colour and the moments of a sequence of quality frames, both through temporal_reference.reproject (the second call's sample is moments_sample's image)
    -> (history (n, 4), moments (n, 4), normal_depth (n, 4), albedo (n, 4)) at the last frame, the guides being the last frame's own entries"""
    import image_stages_reference as IS
    n = frames[0][2].shape[0]
    hist = np.zeros((n, 4), f32); mom = np.zeros((n, 4), f32)
    for k, (cam, surf, sample, guides) in enumerate(frames):
        prev_cam, prev_guides = (frames[k - 1][0], frames[k - 1][3]) if k else (cam, guides)
        nd, alb, _ = IS.fold_guides(surf, None, None, 0)
        hist = T.reproject(size, cam, prev_cam, surf, sample, prev_guides[0], prev_guides[1], hist)
        mom = T.reproject(size, cam, prev_cam, surf, V.moments_sample(sample, alb, demodulate), prev_guides[0], prev_guides[1], mom)
    return hist, mom, nd, alb


def as_image(a, size):
    return np.ascontiguousarray(a, f32).reshape(size[1], size[0], 4)
