"""numpy restatement of the temporal reprojection stage on device buffers (include/mrt_abi.h mrt_context_reproject_device; csrc/temporal.hip): where
each visible surface point was in the previous frame, the history fetched there if it is the same surface, the running average carried on.

TEST INFRASTRUCTURE.  float32 throughout — np.float32 scalars and arrays, no float64 intermediate — one operation per numpy call in the order the header's definition
writes them (numpy rounds each one: no contraction).  What the definition selects away is selected away here with np.where after being computed on whatever the words
hold, under errstate(all="ignore"): a selected-away NaN changes no bit of the output.  tests/test_temporal_cpu.py pins it to known answers, to
path_state_reference.fold_sample and to the oracle with no GPU; tests/test_temporal_device.py compares the kernel with it bit for bit."""
import numpy as np

import surface_reference as S

f32 = np.float32
DEFAULTS = dict(max_history=32.0, min_cos_normal=0.9, depth_tolerance=0.1)          # MRT_REPROJECT_DEFAULT_*
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def camera_rows(camera):
    """a Camera structure, or four 3-vectors (position, right, up, forward) -> (4, 3) float32"""
    if hasattr(camera, "position"):
        return np.array([[v.x, v.y, v.z] for v in (camera.position, camera.right, camera.up, camera.forward)], f32)
    a = np.asarray(camera, f32)
    assert a.shape == (4, 3), a.shape
    return a


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(f32)


def project(camera, q, width, height):
    """q (n, 3) float32 -> px, py, d2 (n,) float32 and ok (n,) bool: c > 0 and both coordinates finite"""
    pos, right, up, fwd = camera_rows(camera)
    nx = _cross(up, fwd); ny = _cross(fwd, right); nz = _cross(right, up)
    det = _dot(right, nx)
    v = np.asarray(q, f32) - pos
    a = _dot(v, nx) / det; b = _dot(v, ny) / det; c = _dot(v, nz) / det
    px = ((a / c + f32(1.0)) * f32(0.5)) * f32(width)
    py = ((b / c + f32(1.0)) * f32(0.5)) * f32(height)
    d2 = _dot(v, v)
    ok = (c > f32(0.0)) & np.isfinite(px) & np.isfinite(py)
    for r in (px, py, d2): assert r.dtype == np.float32
    return px, py, d2, ok


def reproject(size, camera, prev_camera, surfaces, sample, prev_normal_depth, prev_ids, prev_history, prev_position=None, max_history=None, min_cos_normal=None,
              depth_tolerance=None, info=None):
    """-> out (n, 4) float32 {rgb = the new accumulated colour, w = the new history length}, n = width * height, pixel p = y * width + x.  surfaces: (n,) SURFACE_DTYPE or
    (n, 16) float32 rows.  info: a dict that receives, per pixel, 'on', 'projected', 'fx', 'fy', 'kept' (sw > 0) and, per tap (4, n), 'read' (weight not 0), 'inside',
    'ids', 'normal', 'depth', 'length' — each test on its own, whatever the tests before it said — and 'valid'."""
    w, h = int(size[0]), int(size[1])
    n = w * h
    s = np.ascontiguousarray(surfaces)
    s = (s if s.dtype == S.SURFACE_DTYPE else s.view(S.SURFACE_DTYPE)).reshape(-1)
    smp = np.asarray(sample, f32).reshape(n, 4); nd = np.asarray(prev_normal_depth, f32).reshape(n, 4); hist = np.asarray(prev_history, f32).reshape(n, 4)
    ids = np.asarray(prev_ids).reshape(n, 4)
    assert s.shape[0] == n and ids.dtype == np.int32
    M = f32(DEFAULTS["max_history"] if max_history is None else max_history)
    cosn = f32(DEFAULTS["min_cos_normal"] if min_cos_normal is None else min_cos_normal)
    tol = f32(DEFAULTS["depth_tolerance"] if depth_tolerance is None else depth_tolerance)
    with np.errstate(all="ignore"):
        on = s["type"] == 1                                                                              # 1.
        cur = s["position"].astype(f32)
        was = cur if prev_position is None else np.asarray(prev_position, f32).reshape(n, 4)[:, 0:3]
        px1, py1, _, ok1 = project(camera, cur, w, h)                                                    # 2.
        px0, py0, d2, ok0 = project(prev_camera, was, w, h)
        projected = ok1 & ok0
        p = np.arange(n)
        x = (p % w).astype(f32); y = (p // w).astype(f32)
        fx = x + (px0 - px1); fy = y + (py0 - py1)                                                       # 3.
        x0 = np.floor(fx); y0 = np.floor(fy)
        ax = fx - x0; ay = fy - y0
        sw = np.zeros(n, f32); sl = np.zeros(n, f32); sc = np.zeros((n, 3), f32)
        tests = {k: [] for k in ("read", "inside", "ids", "normal", "depth", "length", "valid")}
        for i, j in TAPS:                                                                                # 4.
            wt = (ax if i else f32(1.0) - ax) * (ay if j else f32(1.0) - ay)
            cx = x0 + f32(i); cy = y0 + f32(j)
            read = ~(wt == f32(0.0))
            inside = (cx >= f32(0.0)) & (cx <= f32(w - 1)) & (cy >= f32(0.0)) & (cy <= f32(h - 1))         # decided in float
            q = np.where(inside, cy, f32(0.0)).astype(np.int64) * w + np.where(inside, cx, f32(0.0)).astype(np.int64)
            tid = ids[q]; tnd = nd[q]; th = hist[q]
            same = (tid[:, 0] == 1) & (tid[:, 1] == s["instance_id"]) & (tid[:, 2] == s["geometry_id"])
            normal = _dot(tnd[:, 0:3], s["normal"].astype(f32)) >= cosn
            depth = np.abs(tnd[:, 3] * tnd[:, 3] - d2) <= tol * d2
            length = th[:, 3] >= f32(1.0)
            valid = on & projected & read & inside & same & normal & depth & length
            sw = np.where(valid, sw + wt, sw)
            sc = np.where(valid[:, None], sc + wt[:, None] * th[:, 0:3], sc)
            sl = np.where(valid, sl + wt * th[:, 3], sl)
            for k, v in zip(tests, (read, inside, same, normal, depth, length, valid)): tests[k].append(v)
        kept = sw > f32(0.0)                                                                             # 5.
        hst = sc / sw[:, None]
        grown = sl / sw + f32(1.0)
        ln = np.where(grown < M, grown, M)
        rgb = (smp[:, 0:3] + hst * (ln - f32(1.0))[:, None]) / ln[:, None]
        out = np.empty((n, 4), f32)
        out[:, 0:3] = np.where(kept[:, None], rgb, smp[:, 0:3])
        out[:, 3] = np.where(kept, ln, f32(1.0))
    for a in (fx, ax, sw, sc, sl, hst, ln, rgb): assert a.dtype == np.float32
    if info is not None:
        info.update(on=on, projected=projected, fx=fx, fy=fy, kept=kept, **{k: np.array(v) for k, v in tests.items()})
    return out


def surfaces_of(position, normal, instance=0, geometry=0, primitive=0, kind=1, distance=None):
    """(n,) SURFACE_DTYPE rows for hand-made cases: positions and normals (n, 3); ids scalars or (n,)"""
    position = np.asarray(position, f32)
    n = position.shape[0]
    s = np.zeros(n, S.SURFACE_DTYPE)
    s["position"] = position; s["normal"] = np.asarray(normal, f32); s["type"] = kind
    s["distance"] = f32(1.0) if distance is None else distance
    s["base_color"] = f32(0.5); s["instance_id"] = instance; s["geometry_id"] = geometry; s["primitive_id"] = primitive
    s["resource_slot"] = 0
    return s


def guides_of(surfaces):
    """the previous frame's own guide entries of its rows, as fold_guides(rows, frame 0) writes them: (normal | depth (n, 4) float32, ids (n, 4) int32)"""
    import image_stages_reference as IS
    nd, _, ids = IS.fold_guides(surfaces, None, None, 0)
    return nd, ids
