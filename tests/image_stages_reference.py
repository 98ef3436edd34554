"""numpy restatement of the image stages on device buffers (include/mrt_abi.h mrt_context_fold_guides_device / mrt_context_tonemap_device; csrc/image.hip; DESIGN.md
§10n): one frame folded into the first-hit guide buffers from its bounce-0 surface rows, and Reinhard + flip into RGBA8.  The filter between them has its restatement
already: denoise_reference.denoise_reference.

TEST INFRASTRUCTURE.  float32 throughout, one operation per numpy call in the order written here (numpy rounds each one: no contraction).  The fold is built on
denoise_reference.running_average, the rule the oracle's guide buffers are built with; tests/test_image_stages_cpu.py pins it to denoise_reference.oracle_guides and the
tonemap to the oracle's with no GPU; tests/test_image_stages.py compares the kernels with both bit for bit."""
import numpy as np

import denoise_reference as D
import surface_reference as S

f32 = np.float32
MISS_IDS = np.array([0, -1, -1, -1], np.int32)


def surface_rows(surfaces):
    """(n,) SURFACE_DTYPE records or (n, 16) float32 rows -> (n,) SURFACE_DTYPE (a view: no value is touched, NaNs and all)"""
    a = np.ascontiguousarray(surfaces)
    if a.dtype == S.SURFACE_DTYPE: return a.reshape(-1)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 16, (a.dtype, a.shape)
    return a.view(S.SURFACE_DTYPE).reshape(-1)


def frame_guides(surfaces):
    """What one frame contributes: -> n_new (n, 4) float32, a_new (n, 4) float32, ids (n, 4) int32.  A row that is no surface (type != 1) gives zeros and the miss ids
    whatever its other words hold: they are selected away, never computed with."""
    s = surface_rows(surfaces)
    n = s.shape[0]
    on = s["type"] == 1
    n_new = np.zeros((n, 4), f32); a_new = np.zeros((n, 4), f32); ids = np.empty((n, 4), np.int32); ids[:] = MISS_IDS
    n_new[on, 0:3] = s["normal"][on]; n_new[on, 3] = s["distance"][on]
    a_new[on, 0:3] = s["base_color"][on]; a_new[on, 3] = f32(1.0)
    ids[on, 0] = 1; ids[on, 1] = s["instance_id"][on]; ids[on, 2] = s["geometry_id"][on]; ids[on, 3] = s["primitive_id"][on]
    return n_new, a_new, ids


def fold_guides(surfaces, normal_depth, albedo, frame_index):
    """-> (normal_depth, albedo, ids) after the frame: frame_index 0 replaces the averages (the old ones are not read — None will do), otherwise
    (new + old * frame_index) / (frame_index + 1) per component; the ids are the frame's"""
    assert 0 <= frame_index < 2 ** 32 - 1
    n_new, a_new, ids = frame_guides(surfaces)
    with np.errstate(all="ignore"):
        return D.running_average(normal_depth, n_new, frame_index), D.running_average(albedo, a_new, frame_index), ids


TONEMAP_SIZES = ((1, 1), (16, 16), (17, 15), (64, 48))


def synthetic_image(size, seed=0):
    """an (h, w, 4) float32 image for the tonemap: finite values over [0, 1e6] on a log scale, exact 0 and 1e6, values whose 8-bit result lies next to a rounding
    boundary, a few in (-1, 0), any finite alpha"""
    w, h = size
    rng = np.random.default_rng(1000 + seed)
    img = (10.0 ** rng.uniform(-4.0, 6.0, (h, w, 4))).astype(f32)
    flat = img.reshape(-1, 4)
    t = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    edges = (t / (1.0 - t)).astype(f32)                                                    # c with c / (1 + c) * 255 = k + 0.5, k = 0 .. 254
    special = np.concatenate([np.array([0.0, 1e6, 1.0, -0.0], f32), edges, np.nextafter(edges, f32(0)), (-rng.uniform(0.0, 0.999, 8)).astype(f32)])
    m = min(special.size, flat.shape[0] * 3)                                               # (a 1 x 1 image holds three of them)
    idx = rng.permutation(flat.shape[0] * 3)[:m]
    flat[idx // 3, idx % 3] = rng.permutation(special)[:m]
    flat[:, 3] = rng.standard_normal(flat.shape[0]).astype(f32)
    return img


def tonemap_rgba8(image, size):
    """image (h, w, 4) or (h * w, 4) float32, row 0 = bottom; size (w, h) -> (h, w, 4) uint8, top row first: c / (1 + c), saturate, (unsigned char)(v * 255 + 0.5), alpha 255.
    For finite c > -1 (what the kernel's conversion is pinned for)."""
    w, h = size
    a = np.ascontiguousarray(image, f32).reshape(h, w, 4)
    c = a[::-1, :, 0:3]
    with np.errstate(all="ignore"):
        v = c / (f32(1.0) + c)
        v = np.where(v < f32(0.0), f32(0.0), np.where(v > f32(1.0), f32(1.0), v)).astype(f32)
        q = v * f32(255.0) + f32(0.5)
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0:3] = q.astype(np.int32).astype(np.uint8)           # truncation toward zero, as the conversion in C; the values are in [0.5, 255.5]
    out[..., 3] = 255
    return out
