"""numpy restatement of the variance-guided a-trous filter on device buffers and of the sample image of its moments (include/mrt_abi.h mrt_context_moments_sample_device,
mrt_context_denoise_variance_device; csrc/variance.hip; Schied et al. 2017).

TEST INFRASTRUCTURE.  `moments_sample` and `denoise_variance` are the specification the kernels of csrc/variance.hip follow: float32 throughout, one operation per numpy
call in the order the header's definition writes them, vectorised over the pixels with Python loops over the taps.  A skipped tap is selected away with np.where after being
computed on whatever its words hold, under errstate(all="ignore"): a selected-away NaN changes no bit of the output.  max(a, b) is fmaxf (np.fmax).  With dtype=np.float64 the
same expressions are evaluated in double precision.  `mistake` makes ONE named deviation from the definition (MISTAKES): tests/test_variance_cpu.py shows that each one
changes an answer known by hand."""
import numpy as np

from denoise_reference import B5, DEFAULTS, _lum

f32 = np.float32
MIN_HISTORY = 4.0          # MRT_VARIANCE_MIN_HISTORY
EPSILON = 1e-6             # MRT_VARIANCE_EPSILON
G3 = (1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0, 1.0 / 8.0, 1.0 / 4.0, 1.0 / 8.0, 1.0 / 16.0, 1.0 / 8.0, 1.0 / 16.0)          # row-major from (-1, -1)
MISTAKES = ("w_not_squared", "wsum_not_squared", "g_is_v_p", "g_at_step", "no_boost", "history_gt", "sentinel_eq_0", "sigma_over_step", "g_not_renormalised")


def _albedo(alb, demodulate, dt):
    cov = alb[..., 3] != 0
    A = np.where(cov[..., None], np.fmax(alb[..., :3], dt(f32(1e-3))), dt(1)) if demodulate else np.ones(alb.shape[:-1] + (3,), dt)
    return cov, A


def moments_sample(sample, albedo, demodulate=1):
    """sample, albedo: (..., 4) float32 -> (..., 4) float32 {l, l * l, 0, 0}, l the luminance of sample.rgb / A"""
    smp = np.asarray(sample, f32); alb = np.asarray(albedo, f32)
    with np.errstate(all="ignore"):
        _, A = _albedo(alb, demodulate, f32)
        c = smp[..., :3] / A
        l = _lum(c, f32)
        out = np.zeros(smp.shape, f32)
        out[..., 0] = l
        out[..., 1] = l * l
    assert c.dtype == np.float32 and l.dtype == np.float32
    return out


def _pad(a, P, fill):
    out = np.full((a.shape[0] + 2 * P, a.shape[1] + 2 * P) + a.shape[2:], fill, a.dtype)
    out[P:P + a.shape[0], P:P + a.shape[1]] = a
    return out


def _guide_terms(nd, nq, sigma_normal, zden, dt):
    one, zero = dt(1), dt(0)
    dot = (nd[..., 0] * nq[..., 0] + nd[..., 1] * nq[..., 1]) + nd[..., 2] * nq[..., 2]
    xn = (one - np.fmax(zero, dot)) / sigma_normal
    xz = np.abs(nd[..., 3] - nq[..., 3]) / zden
    kn = np.fmax(zero, one - xn); kz = np.fmax(zero, one - xz)
    return kn, kz


def prepass(image, moments, normal_depth, albedo, sigma_normal=None, sigma_depth=None, demodulate=1, dtype=np.float32, mistake=None, info=None):
    """-> (I (h, w, 3), v (h, w), A (h, w, 3), cov (h, w)): the working entries of the first level; v = -1 where the pixel is not covered"""
    dt = dtype
    sigma_normal = dt(f32(DEFAULTS["sigma_normal"] if sigma_normal is None else sigma_normal))
    sigma_depth = dt(f32(DEFAULTS["sigma_depth"] if sigma_depth is None else sigma_depth))
    img = np.asarray(image, f32).astype(dt); mom = np.asarray(moments, f32).astype(dt); nd = np.asarray(normal_depth, f32).astype(dt); alb = np.asarray(albedo, f32).astype(dt)
    h, w = img.shape[:2]
    one, zero = dt(1), dt(0)
    with np.errstate(all="ignore"):
        cov, A = _albedo(alb, demodulate, dt)
        I = img[..., :3] / A
        m1, m2, ln = mom[..., 0], mom[..., 1], mom[..., 3]
        long_history = (ln > dt(f32(MIN_HISTORY))) if mistake == "history_gt" else (ln >= dt(f32(MIN_HISTORY)))          # a NaN length is a short one
        v_time = np.fmax(zero, m2 - m1 * m1)
        # the spatial estimate: 7 x 7 at distance 1, row-major from (-3, -3)
        P = 3
        mpad = _pad(mom, P, dt(0)); ndpad = _pad(nd, P, dt(0)); cpad = _pad(cov, P, False)
        zden = (sigma_depth * nd[..., 3]) * one
        s1 = np.zeros((h, w), dt); s2 = np.zeros((h, w), dt); sw = np.zeros((h, w), dt)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                y0, x0 = P + dy, P + dx
                mq = mpad[y0:y0 + h, x0:x0 + w]
                if dy == 0 and dx == 0:
                    wgt = np.ones((h, w), dt); valid = np.ones((h, w), bool)
                else:
                    kn, kz = _guide_terms(nd, ndpad[y0:y0 + h, x0:x0 + w], sigma_normal, zden, dt)
                    wgt = (kn * kn) * (kz * kz)
                    valid = cpad[y0:y0 + h, x0:x0 + w]
                s1 = np.where(valid, s1 + wgt * mq[..., 0], s1)
                s2 = np.where(valid, s2 + wgt * mq[..., 1], s2)
                sw = np.where(valid, sw + wgt, sw)
        M1 = s1 / sw; M2 = s2 / sw
        v_space = np.fmax(zero, M2 - M1 * M1)
        if mistake != "no_boost":
            v_space = v_space * (dt(4) / np.fmax(ln, one))
        v = np.where(cov, np.where(long_history, v_time, v_space), dt(-1))
    if info is not None: info.update(long_history=long_history & cov, short_history=~long_history & cov, v=v)
    for a in (I, v): assert a.dtype == dt
    return I, v, A, cov


def level(I, v, nd, step, sigma_color, sigma_normal, sigma_depth, dt=np.float32, mistake=None):
    """one iteration on the working entries {I, v} (v < 0: not covered) -> (I', v')"""
    h, w = v.shape
    one, zero = dt(1), dt(0)
    fstep = dt(step)
    skip = (lambda a: a == zero) if mistake == "sentinel_eq_0" else (lambda a: a < zero)
    with np.errstate(all="ignore"):
        cov = ~skip(v)
        # 1. g: the 3 x 3 Gaussian of v over the adjacent pixels
        gd = step if mistake == "g_at_step" else 1
        vpad = _pad(v, gd, dt(-1))
        ipad = _pad(np.ones((h, w), bool), gd, False)
        gs = np.zeros((h, w), dt); gw = np.zeros((h, w), dt)
        k = 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y0, x0 = gd + dy * gd, gd + dx * gd
                vq = vpad[y0:y0 + h, x0:x0 + w]
                valid = ipad[y0:y0 + h, x0:x0 + w] & ~skip(vq)
                wk = dt(f32(G3[k])); k += 1
                gs = np.where(valid, gs + wk * vq, gs)
                gw = np.where(valid, gw + wk, gw)
        g = gs if mistake == "g_not_renormalised" else gs / gw
        if mistake == "g_is_v_p": g = v
        # 2.
        sc = sigma_color / fstep if mistake == "sigma_over_step" else sigma_color
        den = sc * np.sqrt(g) + dt(f32(EPSILON))
        # 3. the 25 taps
        P = 2 * step
        Ipad = _pad(I, P, dt(0)); vpad = _pad(v, P, dt(-1)); ndpad = _pad(nd, P, dt(0)); ipad = _pad(np.ones((h, w), bool), P, False)
        lum_p = _lum(I, dt)
        zden = (sigma_depth * nd[..., 3]) * fstep
        s = np.zeros((h, w, 3), dt); vs = np.zeros((h, w), dt); ws = np.zeros((h, w), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, x0 = P + dy * step, P + dx * step
                Iq = Ipad[y0:y0 + h, x0:x0 + w]; vq = vpad[y0:y0 + h, x0:x0 + w]
                hk = dt(f32(B5[dy + 2]) * f32(B5[dx + 2]))
                if dy == 0 and dx == 0:
                    wgt = np.full((h, w), hk, dt); valid = np.ones((h, w), bool)
                else:
                    kn, kz = _guide_terms(nd, ndpad[y0:y0 + h, x0:x0 + w], sigma_normal, zden, dt)
                    xc = np.abs(lum_p - _lum(Iq, dt)) / den
                    kc = np.fmax(zero, one - xc)
                    wgt = ((hk * (kn * kn)) * (kz * kz)) * (kc * kc)
                    valid = ipad[y0:y0 + h, x0:x0 + w] & ~skip(vq)
                s = np.where(valid[..., None], s + wgt[..., None] * Iq, s)
                vs = np.where(valid, vs + (wgt if mistake == "w_not_squared" else wgt * wgt) * vq, vs)
                ws = np.where(valid, ws + wgt, ws)
        # 4.
        I2 = np.where(cov[..., None], s / ws[..., None], I)
        v2 = np.where(cov, vs / (ws if mistake == "wsum_not_squared" else ws * ws), v)
    for a in (I2, v2, g, den): assert a.dtype == dt
    return I2, v2


def denoise_variance(image, moments, normal_depth, albedo, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, dtype=np.float32, mistake=None,
                     info=None):
    """image, moments, normal_depth, albedo: (h, w, 4) float32 — image.rgb the accumulated colour, moments {m1, m2, ., len} -> (h, w, 4) the filtered image, alpha 1.
    info: a dict that receives the prepass masks 'long_history', 'short_history', the first level's 'v' and the last level's 'v_last'."""
    assert mistake is None or mistake in MISTAKES, mistake
    dt = dtype
    iterations = DEFAULTS["iterations"] if iterations is None else int(iterations)
    demodulate = DEFAULTS["demodulate"] if demodulate is None else int(demodulate)
    sc = dt(f32(DEFAULTS["sigma_color"] if sigma_color is None else sigma_color))          # in standard deviations
    sn = dt(f32(DEFAULTS["sigma_normal"] if sigma_normal is None else sigma_normal))
    sd = dt(f32(DEFAULTS["sigma_depth"] if sigma_depth is None else sigma_depth))
    assert 1 <= iterations <= 8
    nd = np.asarray(normal_depth, f32).astype(dt)
    I, v, A, cov = prepass(image, moments, normal_depth, albedo, sn, sd, demodulate, dt, mistake, info)
    for it in range(iterations):
        I, v = level(I, v, nd, 1 << it, sc, sn, sd, dt, mistake)
    if info is not None: info["v_last"] = v
    out = np.empty(I.shape[:2] + (4,), dt)
    with np.errstate(all="ignore"):
        out[..., :3] = I * A
    out[..., 3] = dt(1)
    return out
