"""Inputs for the temporal reprojection tests (tests/test_temporal_cpu.py checks tests/temporal_reference.py on them with no GPU; tests/test_temporal_device.py runs the
kernel on the same ones): hand-made images under an exact camera whose answers are known, one case per rejection rule, and random images with every feature present.

TEST INFRASTRUCTURE.  A case is a dict: name, size (w, h), camera and prev_camera (4, 3) float32, surfaces (n,) SURFACE_DTYPE, sample, prev_normal_depth, prev_history
(n, 4) float32, prev_ids (n, 4) int32, prev_position (n, 4) float32 or None, params (keywords of temporal_reference.reproject) and checks: {pixel: [(weight, tap pixel),
...]} — the taps that pixel must blend, in order, with their exact weights; an empty list: the pixel restarts at its sample."""
import numpy as np

import surface_reference as S
import temporal_reference as T

f32 = np.float32
EXACT_CAMERA = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], f32)          # position, right, up, forward: px = x + 0.5 for the points below, exactly
W = H = 8
K = 3 * W + 2                                                                       # the pixel (2, 3) the rejection cases change


def grid_points(dx=0.0, dy=0.0, z=1.0, w=W, h=H):
    """(w * h, 3) float32: ((x + 0.5 + dx) / w * 2 - 1, (y + 0.5 + dy) / h * 2 - 1, 1) * z — all representable for w = h = 8, shifts that are multiples of 1/4, z 1 or 2"""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    p = np.stack([(xs.ravel() + 0.5 + dx) / w * 2 - 1, (ys.ravel() + 0.5 + dy) / h * 2 - 1, np.ones(w * h)], -1) * z
    assert np.array_equal(p.astype(f32).astype(np.float64), p)
    return p.astype(f32)


def _positions4(p):
    out = np.zeros((p.shape[0], 4), f32)
    out[:, 0:3] = p
    return out


def exact_case(name, z=1.0, shift=None, params=None, checks=None):
    """the 8 x 8 image under the exact camera: every pixel a surface at its centre, instance y // 4, geometry x // 4, primitive p; the previous frame saw the same points;
    histories of lengths 1 .. 8 with distinct colours; shift = (dx, dy): where the points were a frame ago, in pixels"""
    n = W * H
    q = grid_points(z=z)
    rng = np.random.default_rng(17)
    s = T.surfaces_of(q, np.tile(np.array([0, 0, -1], f32), (n, 1)), instance=np.arange(n) // W // 4, geometry=np.arange(n) % W // 4, primitive=np.arange(n),
                      distance=np.sqrt(T._dot(q, q)))
    nd, ids = T.guides_of(s)
    hist = rng.random((n, 4)).astype(f32) * f32(4.0)
    hist[:, 3] = (np.arange(n) % 8 + 1).astype(f32)
    sample = rng.random((n, 4)).astype(f32)
    sample[:, 3] = np.nan                                                          # ignored
    pp = None if shift is None else _positions4(grid_points(shift[0], shift[1], z))
    return dict(name=name, size=(W, H), camera=EXACT_CAMERA, prev_camera=EXACT_CAMERA, surfaces=s, sample=sample, prev_normal_depth=nd, prev_ids=ids, prev_history=hist,
                prev_position=pp, params=dict(params or {}), checks=dict(checks or {}))


def jittered(c, z):
    """the case's points seen a quarter of a pixel off their pixels' centres, now and a frame ago: the primary ray's jitter cancels and every pixel fetches itself"""
    c["surfaces"]["position"] = grid_points(0.25, -0.25, z)
    return c


def known_answer_cases():
    """shifts whose taps and weights are known exactly.  The depth test is opened wide (depth_tolerance 1: neighbouring pixels of a plane seen at an angle differ by up to
    16 % in squared distance); ids are constant over the 4 x 4 blocks the checked pixels' taps stay in."""
    p = K
    wide = dict(depth_tolerance=1.0)
    out = []
    for z in (1.0, 2.0):
        tag = f"z{int(z)}"
        out += [exact_case(f"still_{tag}", z, None, None, {p: [(1.0, p)], 0: [(1.0, 0)], W * H - 1: [(1.0, W * H - 1)]}),
                exact_case(f"one_pixel_x_{tag}", z, (1, 0), wide, {p - 2: [(1.0, p - 1)], p - 1 + W: [(1.0, p + W)], 7: []}),          # column 7 fetches column 8: outside
                exact_case(f"one_pixel_y_{tag}", z, (0, 1), wide, {p - W: [(1.0, p)], p - 3 * W: [(1.0, p - 2 * W)], W * (H - 1) + 1: []}),
                exact_case(f"half_pixel_x_{tag}", z, (0.5, 0), wide, {p: [(0.5, p), (0.5, p + 1)], 3 * W + 7: [(0.5, 3 * W + 7)]}),          # some taps outside
                exact_case(f"half_pixel_y_{tag}", z, (0, 0.5), wide, {p - W: [(0.5, p - W), (0.5, p)], W * (H - 1) + 1: [(0.5, W * (H - 1) + 1)]}),
                exact_case(f"quarter_pixel_xy_{tag}", z, (0.25, 0.25), wide, {p - W: [(9 / 16, p - W), (3 / 16, p - W + 1), (3 / 16, p), (1 / 16, p + 1)]}),
                exact_case(f"quarter_back_x_{tag}", z, (-0.25, 0), wide, {p: [(0.25, p - 1), (0.75, p)], 3 * W: [(0.75, 3 * W)]}),
                jittered(exact_case(f"still_off_centre_{tag}", z, None, None, {p: [(1.0, p)], p + 1: [(1.0, p + 1)], 0: [(1.0, 0)]}), z),
                exact_case(f"all_outside_{tag}", z, (8, 0), wide, {k: [] for k in range(W * H)}),
                exact_case(f"all_below_{tag}", z, (0, -8), wide, {k: [] for k in range(W * H)})]
    return out


def rejection_cases():
    """each rule alone: the still image (every pixel fetches itself with weight 1) with one thing changed at pixel K — and the cases that change nothing for K"""
    p = K
    keep, lose = {p: [(1.0, p)]}, {p: []}
    out = []

    def case(name, checks, shift=None, params=None):
        c = exact_case(name, 1.0, shift, params, checks)
        if shift is None:
            for k in (p - 1, p + 1, p + W, p - W): c["checks"].setdefault(k, [(1.0, k)])          # the neighbours go on as before
        out.append(c)
        return c

    c = case("behind_the_previous_camera", lose, (0, 0)); c["prev_position"][p, 2] = -1.0                # c <= 0
    c = case("in_the_previous_cameras_plane", lose, (0, 0)); c["prev_position"][p, 2] = 0.0
    c = case("behind_this_camera", lose); c["surfaces"]["position"][p, 2] = -1.0
    c = case("wrong_instance", lose); c["prev_ids"][p, 1] += 1
    c = case("wrong_geometry", lose); c["prev_ids"][p, 2] += 1
    c = case("another_primitive_is_accepted", keep); c["prev_ids"][p, 3] += 5
    c = case("previous_pixel_not_on", lose); c["prev_ids"][p, 0] = 0
    c = case("previous_on_is_2", lose); c["prev_ids"][p, 0] = 2
    c = case("normal_just_under", lose, params=dict(min_cos_normal=0.9)); c["prev_normal_depth"][p, 0:3] = [0, 0, -np.nextafter(f32(0.9), f32(0))]
    c = case("normal_just_at", keep, params=dict(min_cos_normal=0.9)); c["prev_normal_depth"][p, 0:3] = [0, 0, -f32(0.9)]
    c = case("normal_is_nan", lose); c["prev_normal_depth"][p, 1] = np.nan
    # d2 = 4 and tolerance 1.25: |t * t - 4| <= 5 holds up to t = 3 exactly
    c = case("depth_just_at", keep, params=dict(depth_tolerance=1.25)); c["surfaces"]["position"][p] = [0, 0, 2]; c["prev_normal_depth"][p, 3] = 3.0
    c = case("depth_just_outside", lose, params=dict(depth_tolerance=1.25)); c["surfaces"]["position"][p] = [0, 0, 2]; c["prev_normal_depth"][p, 3] = np.nextafter(f32(3.0), f32(4))
    c = case("depth_is_not_compared_unsquared", lose, params=dict(depth_tolerance=0.25)); c["surfaces"]["position"][p] = [0, 0, 2]; c["prev_normal_depth"][p, 3] = 2.25          # |t - d| = 0.125 d, |t^2 - d2| = 0.27 d2
    c = case("depth_zero_tolerance_exact", keep, params=dict(depth_tolerance=0.0)); c["surfaces"]["position"][p] = [0, 0, 2]; c["prev_normal_depth"][p, 3] = 2.0
    for k in list(c["checks"]):
        if k != p: del c["checks"][k]                                                                  # (the other pixels' distances are rounded square roots)
    c = case("history_length_0", lose); c["prev_history"][p, 3] = 0.0
    c = case("history_length_under_1", lose); c["prev_history"][p, 3] = np.nextafter(f32(1.0), f32(0))
    c = case("history_length_1", keep); c["prev_history"][p, 3] = 1.0
    c = case("history_length_nan", lose); c["prev_history"][p, 3] = np.nan
    c = case("history_clamped_to_4", {p: [(1.0, p)], p + 2: [(1.0, p + 2)], p + 5: [(1.0, p + 5)]}, params=dict(max_history=4.0))          # lengths 3, 4, 5 and 8: clamped BEFORE the blend
    assert [c["prev_history"][k, 3] for k in (p, p + 1, p + 2, p + 5)] == [3, 4, 5, 8]
    c = case("history_clamped_to_1", keep, params=dict(max_history=1.0))
    c = case("zero_history_everywhere", {k: [] for k in range(W * H)}); c["prev_history"][:] = 0.0
    c = case("nan_in_prev_position", lose, (0, 0)); c["prev_position"][p, 0] = np.nan
    c = case("inf_in_prev_position", lose, (0, 0)); c["prev_position"][p, 1] = np.inf
    c = case("current_miss_row_full_of_nans", lose)
    c["surfaces"].view(f32).reshape(-1, 16)[p] = np.nan; c["surfaces"]["type"][p] = 0
    c = case("current_row_of_type_2", lose); c["surfaces"]["type"][p] = 2
    # a NaN in a rejected tap: the half-pixel shift blends p and p + 1; p + 1 is rejected (each way once) and holds NaNs where it is not looked at
    wide = dict(depth_tolerance=1.0)
    half = {p - 1: [(0.5, p - 1), (0.5, p)], p: [(0.5, p)], p + 1: []}                                  # (p + 1's other tap lies in the next geometry block)
    c = case("nan_behind_a_wrong_id", half, (0.5, 0), wide); c["prev_ids"][p + 1, 1] += 1; c["prev_normal_depth"][p + 1] = np.nan; c["prev_history"][p + 1] = np.nan
    c = case("nan_behind_a_wrong_normal", half, (0.5, 0), wide); c["prev_normal_depth"][p + 1, 0:3] = [0, 0, 1]; c["prev_history"][p + 1] = np.nan
    c = case("nan_behind_a_wrong_depth", half, (0.5, 0), wide); c["prev_normal_depth"][p + 1, 3] = 100.0; c["prev_history"][p + 1] = np.nan
    c = case("nan_colour_behind_length_0", half, (0.5, 0), wide); c["prev_history"][p + 1] = [np.nan, np.nan, np.nan, 0.0]
    c = case("nan_outside_weight_0", {p: [(1.0, p)]}); c["prev_history"][p + 1] = np.nan; c["prev_history"][p + W] = np.nan; c["prev_history"][p + W + 1] = np.nan
    del c["checks"][p + 1], c["checks"][p + W]                                                         # (their own history is the NaN: a valid tap's NaN is the caller's)
    return out


# ---------------------------------------------------------------- random images
def tilted_camera(k=0):
    """a camera whose basis is neither axis-aligned nor orthogonal, and its k-th small move"""
    t = f32(0.013) * f32(k)
    return np.array([[0.1 + 0.5 * t, 1.0 - 0.3 * t, 3.4 + 0.2 * t], [0.52 + t, 0.03, -0.08], [0.02, 0.39, 0.05 - t], [-0.07 + t, -0.04, -1.0]], f32)


def unproject(camera, px, py, depth, size):
    pos, right, up, fwd = T.camera_rows(camera)
    u = (px / f32(size[0])) * f32(2.0) - f32(1.0); v = (py / f32(size[1])) * f32(2.0) - f32(1.0)
    return (pos + depth[:, None] * ((u[:, None] * right + v[:, None] * up) + fwd)).astype(f32)


def random_case(size, seed):
    """every feature in some pixels: motion up to +- 3 pixels under two different cameras, a quarter of the previous ids scrambled, history lengths 0, 1, 7.5 and 32 among
    random ones, previous pixels that are off, current rows that miss, normals and distances off by more than the tolerances — and NaNs in every word a rejection leaves
    unread for every fetcher: the guide and history entries of previous pixels that are off, the colour of a history of length 0, the rows of current misses"""
    w, h = size
    n = w * h
    rng = np.random.default_rng(seed)
    cam, prev_cam = tilted_camera(1), tilted_camera(0)
    p = np.arange(n)
    x, y = (p % w).astype(f32), (p // w).astype(f32)
    jit = rng.random((2, n)).astype(f32)
    depth = (f32(2.0) + f32(0.02) * x + f32(0.03) * y + rng.random(n).astype(f32) * f32(0.01)).astype(f32)
    cur = unproject(cam, x + jit[0], y + jit[1], depth, size)
    motion = (rng.random((2, n)).astype(f32) * f32(6.0) - f32(3.0)) * (rng.random(n) < 0.7)          # (a third does not move at all)
    was = unproject(prev_cam, x + jit[0] + motion[0], y + jit[1] + motion[1], depth * (f32(1.0) + (rng.random(n).astype(f32) - f32(0.5)) * f32(0.02)), size)
    normal = np.tile(np.array([0.05, 0.1, 0.99], f32), (n, 1)) + rng.standard_normal((n, 3)).astype(f32) * f32(0.05)
    block = lambda xx, yy: (np.clip(xx, 0, w - 1) // 8 + 5 * (np.clip(yy, 0, h - 1) // 8)).astype(np.int32)
    s = T.surfaces_of(cur, normal, instance=block(x + motion[0], y + motion[1]), geometry=0, primitive=rng.integers(0, 1000, n), distance=depth)
    miss = rng.random(n) < 0.06
    s.view(f32).reshape(-1, 16)[miss] = np.nan; s["type"][miss] = 0
    # the previous frame's own guides: blocks of one instance, normals near the current ones, distances near the previous points'
    prev_rows = T.surfaces_of(np.zeros((n, 3), f32), normal + rng.standard_normal((n, 3)).astype(f32) * f32(0.02), instance=block(x, y), geometry=0, primitive=rng.integers(0, 1000, n))
    d_prev = np.sqrt(T._dot(was - prev_cam[0], was - prev_cam[0]))
    prev_rows["distance"] = np.where(rng.random(n) < 0.1, d_prev * f32(1.2), d_prev * (f32(1.0) + (rng.random(n).astype(f32) - f32(0.5)) * f32(0.04)))
    turned = rng.random(n) < 0.08
    prev_rows["normal"][turned] = -prev_rows["normal"][turned]
    nd, ids = T.guides_of(prev_rows)
    scrambled = rng.random(n) < 0.25
    ids[scrambled, 1] = rng.integers(0, 40, int(scrambled.sum())); ids[scrambled & (rng.random(n) < 0.3), 2] = 1
    hist = rng.random((n, 4)).astype(f32) * f32(3.0)
    hist[:, 3] = rng.choice(np.array([0.0, 1.0, 7.5, 32.0, 2.0, 31.5, 100.0], f32), n)
    off = rng.random(n) < 0.08
    ids[off] = [0, -1, -1, -1]; nd[off] = np.nan; hist[off] = np.nan
    hist[hist[:, 3] == 0, 0:3] = np.nan
    sample = rng.random((n, 4)).astype(f32)
    return dict(name=f"random_{w}x{h}", size=size, camera=cam, prev_camera=prev_cam, surfaces=s, sample=sample, prev_normal_depth=nd, prev_ids=ids, prev_history=hist,
                prev_position=_positions4(was), params={}, checks={})


def run_reference(c, info=None, **over):
    kw = dict(c["params"]); kw.update(over)
    return T.reproject(c["size"], c["camera"], c["prev_camera"], c["surfaces"], c["sample"], c["prev_normal_depth"], c["prev_ids"], c["prev_history"], c["prev_position"], info=info, **kw)


def blend(c, pixel, taps):
    """what the definition gives pixel `pixel` for these (weight, tap pixel) pairs under the case's max_history, written out: -> (4,) float32"""
    smp, hist = c["sample"][pixel], c["prev_history"]
    max_history = c["params"].get("max_history", T.DEFAULTS["max_history"])
    if not taps: return np.append(smp[0:3], f32(1.0))
    sw = f32(0.0); sl = f32(0.0); sc = np.zeros(3, f32)
    for wt, q in taps:
        wt = f32(wt)
        sw = sw + wt; sc = sc + wt * hist[q, 0:3]; sl = sl + wt * hist[q, 3]
    grown = sl / sw + f32(1.0)
    ln = grown if grown < f32(max_history) else f32(max_history)
    return np.append((smp[0:3] + (sc / sw) * (ln - f32(1.0))) / ln, ln).astype(f32)


# ---------------------------------------------------------------- the composed sequence: a camera that moves a little each frame and one instance that moves
SEQUENCE = dict(size=(48, 32), frames=6, mover=5, seed=S.SEED)          # mesh 5: the small sphere above the ground of test_instancing's scene


def sequence_scene(mrt):
    from test_instancing import _scene
    return _scene(mrt, SEQUENCE["size"])


def sequence_camera(mrt, base, k):
    """frame k's camera: a step to the right and up each frame, turning a little to the left"""
    c = mrt.Camera.from_buffer_copy(base)
    c.position.x += 0.06 * k; c.position.y += 0.045 * k; c.forward.x -= 0.012 * k
    return c


def sequence_pose(mrt, k):
    """frame k's pose of the moving instance: (16,) float32, column-major"""
    return mrt.make_transform([0.2 - 0.11 * k, 1.1 + 0.03 * k, 0.8], [0, 0, 0], 0.4).reshape(16).astype(f32)


def pose_step(pose_prev, pose_now):
    """the (4, 4) float32 matrix M with previous position = M . (position, 1): the previous pose after the inverse of this frame's (column vectors)"""
    a = np.asarray(pose_prev, np.float64).reshape(4, 4).T; b = np.asarray(pose_now, np.float64).reshape(4, 4).T          # (column-major storage)
    return (a @ np.linalg.inv(b)).astype(f32)


def cpu_sequence(mrt, orc):
    """the sequence on the CPU: the oracle's queries, surface_reference's rows, stages_reference's light rows (bounce-0 direct light as the sample), image_stages_reference's
    guide entries -> per frame a dict of reproject's inputs, its output `out` and `info`"""
    import image_stages_reference as IS
    import stages_reference as R
    w, h = SEQUENCE["size"]
    n = w * h
    sc = sequence_scene(mrt)
    entries = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(entries, sc.lights, instancing=True)
    ref = S.SurfaceReference(entries)
    frames = []
    hist = np.zeros((n, 4), f32); nd = np.zeros((n, 4), f32); ids = np.zeros((n, 4), np.int32)
    cam_prev = pose_prev = None
    try:
        for k in range(SEQUENCE["frames"]):
            cam = sequence_camera(mrt, sc.camera, k); pose = sequence_pose(mrt, k)
            osc.set_transform(SEQUENCE["mover"], pose); ref.set_transform(SEQUENCE["mover"], pose)
            rays, hidx = R.primary_rays(orc, cam, w, h, SEQUENCE["seed"], k)
            surf = ref.resolve(rays, osc.intersect_closest(rays))
            st = R.scatter(orc, surf, hidx, 0, sc.lights)
            lit = (st["light"][:, 3] == f32(1.0)) & (osc.intersect_any(st["shadow_rays"]) == 0)
            sample = np.zeros((n, 4), f32)
            sample[:, 0:3] = np.where(lit[:, None], st["light"][:, 0:3] * surf["base_color"], f32(0.0))
            pp = np.zeros((n, 4), f32); pp[:, 0:3] = surf["position"]
            if k:
                M = pose_step(pose_prev, pose)
                moved = (surf["type"] == 1) & (surf["instance_id"] == SEQUENCE["mover"])
                q = surf["position"]
                was = ((q[:, 0:1] * M[:, 0] + q[:, 1:2] * M[:, 1]) + q[:, 2:3] * M[:, 2]) + M[:, 3]
                pp[moved, 0:3] = was[moved, 0:3]
            c = dict(name=f"sequence_{k}", size=(w, h), camera=T.camera_rows(cam), prev_camera=T.camera_rows(cam_prev if k else cam), surfaces=surf, sample=sample, prev_normal_depth=nd,
                     prev_ids=ids, prev_history=hist, prev_position=pp, params={}, checks={})
            c["info"] = {}
            c["out"] = run_reference(c, info=c["info"])
            frames.append(c)
            hist = c["out"]
            nd, _, ids = IS.fold_guides(surf, None, None, 0)
            cam_prev, pose_prev = cam, pose
    finally:
        osc.close()
    return frames


def sequence_losses(c):
    """of a frame of the sequence -> dict of pixel masks: 'surface' (on and projected), 'kept', and the pixels that lost their history to 'outside' (a tap they wanted
    lies outside the image), 'ids' (a tap inside is another surface, and this pixel or that tap is the moving instance) and 'depth' (a tap of the same surface and a
    like normal is too near or too far)"""
    i = c["info"]
    s = c["surfaces"]
    surface = i["on"] & i["projected"]
    lost = surface & ~i["kept"]
    live = i["read"] & surface[None]
    mover = SEQUENCE["mover"]
    w, h = c["size"]
    x0 = np.floor(i["fx"]); y0 = np.floor(i["fy"])
    about = np.zeros_like(live)
    for t, (a, b) in enumerate(T.TAPS):
        q = (np.clip(y0 + b, 0, h - 1) * w + np.clip(x0 + a, 0, w - 1)).astype(np.int64)
        q = np.where(surface, q, 0)
        about[t] = (s["instance_id"] == mover) | (c["prev_ids"][q, 1] == mover)
    return dict(surface=surface, kept=i["kept"], outside=lost & (live & ~i["inside"]).any(0), ids=lost & (live & i["inside"] & ~i["ids"] & about).any(0),
                depth=lost & (live & i["inside"] & i["ids"] & i["normal"] & ~i["depth"]).any(0))


# ---------------------------------------------------------------- the quality direction: a short camera move over the Cornell box
QUALITY = dict(size=(64, 64), frames=8, seed=1, moves=(2, 4, 6))          # the camera steps before frames 2, 4 and 6


def quality_camera(mrt, base, k):
    step = sum(k >= m for m in QUALITY["moves"])
    c = mrt.Camera.from_buffer_copy(base)
    c.position.x += 0.05 * step; c.forward.x -= 0.015 * step
    return c


def quality_frames(mrt, orc):
    """-> per frame (camera rows, surfaces, the oracle's one-frame sample (n, 4), this frame's guide entries (nd, ids)), and the converged image at the last camera"""
    import image_stages_reference as IS
    import stages_reference as R
    w, h = QUALITY["size"]
    sc = mrt.CornellScene((w, h))
    entries = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(mrt.flatten_scene(sc), sc.lights)
    ref = S.SurfaceReference(entries)
    out = []
    try:
        for k in range(QUALITY["frames"]):
            cam = quality_camera(mrt, sc.camera, k)
            orr = orc.OracleRenderer(osc, w, h, seed=QUALITY["seed"], max_bounces=3, camera=cam)
            orr.set_sample_offset(k)
            orr.render(1)
            sample = orr.accumulation().reshape(-1, 4); orr.close()
            rays, _ = R.primary_rays(orc, cam, w, h, QUALITY["seed"], k)
            surf = ref.resolve(rays, osc.intersect_closest(rays))
            nd, _, ids = IS.fold_guides(surf, None, None, 0)
            out.append((T.camera_rows(cam), surf, sample, (nd, ids)))
        orr = orc.OracleRenderer(osc, w, h, seed=QUALITY["seed"] + 1, max_bounces=3, camera=cam)
        orr.render(512, threads=4)
        converged = orr.accumulation().reshape(-1, 4); orr.close()
    finally:
        osc.close()
    return out, converged


def quality_run(frames, **params):
    """-> (the reprojected accumulation, the running average restarted at every move, the last sample) at the last frame"""
    n = frames[0][2].shape[0]
    hist = np.zeros((n, 4), f32); restart = None; since = 0
    for k, (cam, surf, sample, guides) in enumerate(frames):
        prev_cam, prev_guides = (frames[k - 1][0], frames[k - 1][3]) if k else (cam, guides)
        hist = T.reproject(QUALITY["size"], cam, prev_cam, surf, sample, prev_guides[0], prev_guides[1], hist, **params)
        since = 0 if k in QUALITY["moves"] or k == 0 else since + 1
        restart = sample[:, 0:3] if since == 0 else (sample[:, 0:3] + restart * f32(since)) / f32(since + 1)
    return hist[:, 0:3], restart, frames[-1][2][:, 0:3]


def rmse(a, b):
    return float(np.sqrt(((a[:, 0:3].astype(np.float64) - b[:, 0:3].astype(np.float64)) ** 2).mean()))
