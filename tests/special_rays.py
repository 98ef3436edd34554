"""Ray families at the points where slab tests are most fragile — TEST INFRASTRUCTURE, no test in here (tests/test_special_rays_cpu.py checks the reference side on
every family without a GPU, tests/test_special_rays.py sends them through every entry that takes caller rays).

Almost every ray of the rest of the suite is normalize(target - origin) with three non-zero components.  Here:

  F1  sign patterns       every direction of {-1, -0.0, +0.0, +1}^3 with at least one +-1 (56 patterns), normalised, the zeros keeping their sign bit
  F2  tiny components     F1 with every zero replaced by +- a denormal, or a value on either side of the 1e-20 clamp of the box tests' reciprocal
  F3  origins on geometry axis-parallel rays (both zero signs) whose free origin coordinates are a mesh vertex's, and rays lying exactly in the floor's plane y = 0
  F4  interval edges      rays with a known hit distance t and min_distance / max_distance at t, one float either side of it, 0, and an empty interval
  F5  instance-induced -0 a two-level scene of its own: world rays with +0 components only whose OBJECT-space direction gets a -0 from the instance's rows

A family is a Family(name, rays, tags): rays (n, 8) float32 [ox, oy, oz, tmin, dx, dy, dz, tmax], read-only, from fixed seeds; tags (n,) strings.
`case(mrt, orc, two_level)` builds scene, oracle, float64 triangles, the families and their reference answers once; nothing in it is ever modified."""
import collections
import functools
import itertools

import numpy as np

import f64_reference as F
from test_fuzz_geometry import _rays, _scene

f32 = np.float32
FIELDS = ("type", "distance", "instance_id", "geometry_id", "primitive_id", "u", "v")
SIZE, SEED = (32, 32), 1          # test_fuzz_geometry._scene(seed 1): 2 834 triangles — pole fans, soup, coincident sheets, the floor

Family = collections.namedtuple("Family", "name rays tags")


def _family(name, rays, tags):
    rays = np.ascontiguousarray(rays, f32); tags = np.asarray(tags)
    assert rays.shape == (len(tags), 8)
    rays.setflags(write=False); tags.setflags(write=False)
    return Family(name, rays, tags)


def neg_zero(x):
    return (x == 0) & np.signbit(x)


def carries_neg_zero(rays):
    """per ray: a direction component is -0.0"""
    return neg_zero(np.asarray(rays)[:, 4:7]).any(1)


def _pack(o, d, tmin=0.0, tmax=np.inf):
    r = np.zeros((len(o), 8), f32)
    r[:, 0:3] = o; r[:, 3] = tmin; r[:, 4:7] = d; r[:, 7] = tmax
    return r


# ---------------------------------------------------------------- F1
PATTERNS = [p for p in itertools.product((-1.0, -0.0, 0.0, 1.0), repeat=3) if any(abs(c) == 1.0 for c in p)]
PER_PATTERN = 40


def _pattern_name(p):
    return ",".join(("-" if np.signbit(c) else "+") + ("1" if c else "0") for c in p)          # "-0,+0,-1"


def f1_sign_patterns():
    assert len(PATTERNS) == 56
    rng = np.random.default_rng(7)
    n = len(PATTERNS) * PER_PATTERN
    target = np.c_[rng.uniform(-1.8, 1.8, n), rng.uniform(0, 1.8, n), rng.uniform(-1.5, 2.0, n)]
    p = np.repeat(np.array(PATTERNS, np.float64), PER_PATTERN, axis=0)
    d = np.copysign(p / np.linalg.norm(p, axis=1, keepdims=True), p).astype(f32)          # the zeros' sign bits put back
    o = (target - 6.0 * d.astype(np.float64)).astype(f32)
    tags = np.repeat([_pattern_name(q) for q in PATTERNS], PER_PATTERN)
    fam = _family("F1", _pack(o, d), tags)
    assert carries_neg_zero(fam.rays).sum() == 30 * PER_PATTERN
    return fam


# ---------------------------------------------------------------- F2
# either side of `fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d` (traverse.h safe_inv / box_inv), and denormals
_C = f32(1e-20)
TINY = collections.OrderedDict([("denorm_min", f32(1e-45)), ("1e-38", f32(1e-38)), ("1e-21", f32(1e-21)), ("below_clamp", np.nextafter(_C, f32(0))), ("clamp", _C),
                                ("above_clamp", np.nextafter(_C, f32(1))), ("1e-19", f32(1e-19))])


def f2_tiny_components(f1):
    assert TINY["denorm_min"] > 0 and TINY["denorm_min"] == np.nextafter(f32(0), f32(1)) and TINY["1e-38"] < np.finfo(f32).tiny
    d = f1.rays[:, 4:7]
    keep = np.flatnonzero((d == 0).any(1))
    rays = np.array(f1.rays[keep])
    names = list(TINY)
    which = np.arange(len(keep)) % len(names)
    val = np.array([TINY[k] for k in names], f32)[which]
    dd = rays[:, 4:7]
    rays[:, 4:7] = np.where(dd == 0, np.copysign(val[:, None], dd), dd)
    return _family("F2", rays, np.array(names)[which])


# ---------------------------------------------------------------- F3
def f3_origins_on_geometry(tris):
    """tris: f64_reference.Triangles of the scene (world space).  Axis-parallel rays through a vertex: the two coordinates the ray does not move along are the vertex's own
    float32 bits, so the ray runs exactly along box planes and triangle edges that pass through that vertex; both zero signs.  Then rays in the floor's plane."""
    rng = np.random.default_rng(11)
    verts = np.concatenate([tris.v0, tris.v1, tris.v2]).astype(f32)
    verts = verts[np.abs(verts).max(1) < 5.0]                    # not the floor's corners (10 units out)
    verts = verts[rng.choice(len(verts), 60, replace=False)]
    o, d, tags = [], [], []
    for v in verts:
        for axis in range(3):
            for sign in (-1.0, 1.0):
                for za, zb in itertools.product((0.0, -0.0), repeat=2):
                    dd = np.zeros(3, f32); dd[axis] = sign
                    dd[(axis + 1) % 3] = za; dd[(axis + 2) % 3] = zb
                    oo = v.copy(); oo[axis] = v[axis] - f32(sign * 3.0)
                    o.append(oo); d.append(dd); tags.append("vertex")
    # in the floor's plane y = 0: the floor's own determinant is 0 for these, whatever crosses the plane must still be hit
    n = 160
    ang = rng.uniform(0, 2 * np.pi, n)
    target = np.c_[rng.uniform(-1.5, 1.5, n), np.zeros(n), rng.uniform(-1.2, 1.8, n)]
    origin = np.c_[5.0 * np.cos(ang), np.zeros(n), 5.0 * np.sin(ang)]
    dir_ = target - origin; dir_ /= np.linalg.norm(dir_, axis=1, keepdims=True)
    for k in range(n):
        for zy in (0.0, -0.0):
            dd = dir_[k].astype(f32); dd[1] = zy
            o.append(origin[k].astype(f32)); d.append(dd); tags.append("in_plane")
    for k in range(40):                                              # ... and axis-parallel within it
        axis, sign = (0, 2)[k % 2], (-1.0, 1.0)[(k // 2) % 2]
        for zy, zo in itertools.product((0.0, -0.0), repeat=2):
            dd = np.zeros(3, f32); dd[axis] = sign; dd[1] = zy; dd[2 - axis] = zo
            oo = np.zeros(3, f32); oo[axis] = -sign * 5.0; oo[2 - axis] = f32(target[k, 2 - axis])
            o.append(oo); d.append(dd); tags.append("in_plane")
    return _family("F3", _pack(np.array(o), np.array(d)), tags)


# ---------------------------------------------------------------- F4
F4_CASES = ("base", "max=t", "max=t+", "max=t-", "max=0", "min=t", "min=t+", "min=t-", "min=max=t", "min>max")
F4_NO_MIN = ("base", "max=t", "max=t+", "max=t-", "max=0")          # what the stream kernels can take: min_distance == 0
F4_BASE = 150


def f4_base_rays(f1):
    """candidates: 120 rays of F1 that carry a zero (every fifth of them), then 120 ordinary ones; case() keeps the first 75 of each part that hit"""
    z = np.flatnonzero((f1.rays[:, 4:7] == 0).any(1))
    return np.concatenate([f1.rays[z[::5][:120]], _rays(np.random.default_rng(12), 120)]).astype(f32)


def f4_interval_edges(base, t):
    """base: rays whose closest hit (interval [0, inf]) is at the float32 distance t > 0, by the oracle's brute force.  Every case for every base ray."""
    assert len(base) == len(t) and (t > 0).all() and np.isfinite(t).all()
    up, dn = np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))
    inf = np.full(len(t), np.inf, f32); zero = np.zeros(len(t), f32)
    bounds = {"base": (zero, inf), "max=t": (zero, t), "max=t+": (zero, up), "max=t-": (zero, dn), "max=0": (zero, zero),
              "min=t": (t, inf), "min=t+": (up, inf), "min=t-": (dn, inf), "min=max=t": (t, t), "min>max": (t, dn)}
    rays, tags = [], []
    for name in F4_CASES:
        r = np.array(base); r[:, 3], r[:, 7] = bounds[name]
        rays.append(r); tags += [name] * len(r)
    return _family("F4", np.concatenate(rays), tags)


# ---------------------------------------------------------------- F5
F5_ROTATIONS_DEG = (200.0, 225.0, 250.0)
F5_DIRECTIONS = [(0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),
                 (0.6, 0.0, 0.8), (-0.8, 0.0, 0.6), (0.0, -0.8, 0.6), (0.6, -0.8, 0.0), (0.0, -0.6, -0.8), (-0.6, -0.8, 0.0)]          # +0 only


def f5_scene(mrt, size=SIZE, lights=None):
    """the floor, one unrotated sphere (sphere.obj: 4 900 triangles — above 8, so its BLAS has nodes to test) and three instances of it turned about y"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [mrt.Model(name="plane", position=[0, 0, 0], scale=10),
                           mrt.Model(name="sphere", position=[-1.3, 0.0, 0.9], scale=0.8),
                           mrt.Model(name="sphere", position=[0.2, 0.4, 0.6], rotation=[0, np.radians(F5_ROTATIONS_DEG[0]), 0], scale=0.9),
                           mrt.Model(name="sphere", position=[1.5, 0.1, -0.3], rotation=[0, np.radians(F5_ROTATIONS_DEG[1]), 0], scale=0.7),
                           mrt.Model(name="sphere", position=[-0.4, 0.2, -1.2], rotation=[0, np.radians(F5_ROTATIONS_DEG[2]), 0], scale=1.0)]
            if lights is not None: self.lights = lights
    return S(size)


def world_to_object_rows(mrt, xf16):
    """the instance's world -> object rows (3, 4) as the library computes them (mrt_debug_instance_box; pinned by tests/test_wide_encode_cpu.py)"""
    from metal_raytracing_amd._ffi import ptr
    xf = np.ascontiguousarray(xf16, f32).reshape(16)
    lo, hi = -np.ones(3, f32), np.ones(3, f32)
    rows = np.zeros((3, 4), f32); box = np.zeros(6, f32)
    assert mrt.lib.mrt_debug_instance_box(ptr(xf), ptr(lo), ptr(hi), ptr(rows), ptr(box)) == 0
    return rows


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64; the sum is rounded to float64, then to float32 — which can differ from fmaf in the last bit of a
    non-zero result, never in whether the result is zero or in a zero's sign, which is all the tags below read"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def object_direction(rows, d):
    """to_object_dir (traverse_instanced.h): fma(c, dz, fma(b, dy, a * dx)) per row, float32; d (n, 3) -> (n, 3)"""
    d = np.asarray(d, f32)
    out = np.zeros_like(d)
    for r in range(3):
        a, b, c = (np.full(len(d), rows[r, k], f32) for k in range(3))
        out[:, r] = _fma32(c, d[:, 2], _fma32(b, d[:, 1], a * d[:, 0]))
    return out


def f5_instance_neg_zero(mrt, sc):
    """-> (Family, pairs): world rays aimed at every sphere from every direction of F5_DIRECTIONS; pairs (n, number of meshes) bool: the object-space direction of ray i in
    instance j has a -0.0 component (the floor, an instance of <= 8 triangles, has no node to test: its column stays False)"""
    meshes = mrt.flatten_scene(sc)
    rng = np.random.default_rng(13)
    o, d, tags = [], [], []
    for j, (pos, _, xf, _) in enumerate(meshes):
        if j == 0: continue
        M = np.asarray(xf, np.float64).reshape(4, 4).T
        P = np.asarray(pos, np.float64) @ M[:3, :3].T + M[:3, 3]
        centre, radius = 0.5 * (P.min(0) + P.max(0)), 0.5 * (P.max(0) - P.min(0)).min()
        for k, dirn in enumerate(F5_DIRECTIONS):
            dd = np.array(dirn, f32)
            for _ in range(12):
                off = rng.uniform(-0.6, 0.6, 3) * radius
                target = centre + off
                o.append((target - 4.0 * dd.astype(np.float64)).astype(f32)); d.append(dd); tags.append(f"inst{j}:dir{k}")
    rays = _pack(np.array(o), np.array(d))
    assert not np.signbit(rays[:, 4:7][rays[:, 4:7] == 0]).any(), "the world rays hold +0 only"
    pairs = np.zeros((len(rays), len(meshes)), bool)
    for j, (pos, _, xf, _) in enumerate(meshes):
        if j == 0: continue
        pairs[:, j] = neg_zero(object_direction(world_to_object_rows(mrt, xf), rays[:, 4:7])).any(1)
    pairs.setflags(write=False)
    return _family("F5", rays, tags), pairs


# ---------------------------------------------------------------- the float64 judge
def grazes(tris, o, d, t_end, eps=1e-4):
    """per ray: within [0, t_end] the ray crosses the plane of some triangle at a point whose smallest barycentric coordinate lies within eps of 0 — on or beside that
    triangle's boundary; or the ray lies (all but) IN the plane of some triangle: at an angle below eps to it, not exactly parallel (den == 0 is a miss on every side:
    the floor for the rays in y = 0), and starting within 10 eps of it — a ray along x through a vertex of test_fuzz_geometry's sheets, whose plane holds the x direction.
    float64, the arithmetic of f64_reference.Triangles.intersect."""
    out = np.zeros(len(o), bool)
    ok_tri = tris.gdet > 0
    nlen = np.sqrt((tris.n * tris.n).sum(1))
    chunk = int(max(8, min(2048, 8_000_000 // max(1, len(tris)))))
    for a in range(0, len(o), chunk):
        oo, dd = o[a:a + chunk, None, :], d[a:a + chunk, None, :]
        den = (tris.n[None] * dd).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (tris.n[None] * (tris.v0[None] - oo)).sum(-1) / den
            p = oo + t[..., None] * dd - tris.v0[None]
            b1, b2 = (p * tris.e1[None]).sum(-1), (p * tris.e2[None]).sum(-1)
            u = (tris.g22 * b1 - tris.g12 * b2) / tris.gdet
            v = (tris.g11 * b2 - tris.g12 * b1) / tris.gdet
            near = ok_tri[None] & (den != 0) & (t >= 0) & (t <= t_end[a:a + chunk, None]) & (np.abs(np.minimum(np.minimum(u, v), 1 - u - v)) <= eps)
            dist = (tris.n[None] * (tris.v0[None] - oo)).sum(-1)
            flat = ok_tri[None] & (den != 0) & (np.abs(den) < eps * nlen[None] * np.sqrt((dd * dd).sum(-1))) & (np.abs(dist) < 10 * eps * nlen[None])
        out[a:a + chunk] = near.any(1) | flat.any(1)
    return out


def judge64(tris, rays, no_grazing=False):
    """f64_reference.Triangles.intersect for the rays' [0, max_distance] (min_distance is not looked at) -> dict: t, u, v, tri, t2, hit, and `decided` — test_independent_f64.py's
    mask: the hit is clear of its triangle's edges (margin > 1e-4) and of a runner-up at nearly the same distance (relative separation > 1e-4); a miss counts as decided there too.
    no_grazing (F3, whose rays are AIMED at vertices): a ray that passes within 1e-4 (barycentric) of any triangle's boundary on its way to the hit, or anywhere when it
    misses, is not decided either — float64 sees the float32 vertex a rounding away from where the float32 transform puts it, so it cannot say on which side such a ray passes."""
    rays = np.asarray(rays)
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    with np.errstate(invalid="ignore"):          # (a ray in a triangle's plane: 0 / 0 inside intersect, which it treats as a miss)
        t, u, v, ti, t2 = tris.intersect(o, d, rays[:, 7].astype(np.float64))
    hit = ti >= 0
    edge = np.where(hit, np.minimum(np.minimum(u, v), 1 - u - v), 1.0)
    with np.errstate(invalid="ignore"):
        sep = np.where(hit, (t2 - t) / np.maximum(t, 1e-9), 1.0)
    decided = (edge > 1e-4) & (sep > 1e-4)
    if no_grazing:
        decided &= ~grazes(tris, o, d, np.where(hit, t * (1 + 1e-4), rays[:, 7].astype(np.float64)))
    out = dict(t=t, u=u, v=v, tri=ti, t2=t2, hit=hit, decided=decided)
    for a in out.values(): a.setflags(write=False)
    return out


def assert_matches_f64(tris, j, rec, what, only=None):
    """a closest-hit record array against judge64's answer on the decided rays (`only`: a further mask), with test_independent_f64.py's figures"""
    m = j["decided"] if only is None else j["decided"] & only
    agree = (rec["type"] == 1) == j["hit"]
    assert agree[m].all(), f"{what}: {(~agree & m).sum()} decided rays disagree with float64 on hit / miss, first {np.flatnonzero(~agree & m)[0]}"
    h = m & j["hit"]
    ids = tris.ids[j["tri"][h]]
    assert np.array_equal(rec["instance_id"][h], ids[:, 0]) and np.array_equal(rec["geometry_id"][h], ids[:, 1]) and np.array_equal(rec["primitive_id"][h], ids[:, 2]), f"{what}: ids"
    dt = np.abs(rec["distance"][h].astype(np.float64) - j["t"][h])
    assert (dt <= 1e-6 + 2e-5 * np.abs(j["t"][h])).all(), f"{what}: distance off by up to {dt.max():.3g}"
    if h.any():
        assert np.abs(rec["u"][h] - j["u"][h]).max() < 5e-4 and np.abs(rec["v"][h] - j["v"][h]).max() < 5e-4, f"{what}: u, v"
    return int(h.sum())


# ---------------------------------------------------------------- everything once
Case = collections.namedtuple("Case", "scene oracle tris families closest occluded judged pairs")


@functools.lru_cache(maxsize=None)
def case(mrt, orc, two_level):
    """F1 .. F4 on test_fuzz_geometry._scene(seed 1), flattened or two-level: the scene, its oracle, its float64 triangles, {name: Family}, and per family the oracle's
    brute-force closest records and any-hit answers and judge64's verdict.  Computed once per scene form and never modified."""
    sc = _scene(mrt, SIZE, SEED)
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=two_level), sc.lights, instancing=two_level)
    tris = F.Triangles(mrt.flatten_scene(sc))
    f1 = f1_sign_patterns()
    base = f4_base_rays(f1)
    b = osc.intersect_closest(base, brute=True)
    ok = (b["type"] == 1) & (b["distance"] > 0)
    hit = np.concatenate([np.flatnonzero(ok[:120])[:F4_BASE // 2], 120 + np.flatnonzero(ok[120:])[:F4_BASE // 2]])
    fams = {"F1": f1, "F2": f2_tiny_components(f1), "F3": f3_origins_on_geometry(tris), "F4": f4_interval_edges(base[hit], b["distance"][hit])}
    return _finish(sc, osc, tris, fams, None)


@functools.lru_cache(maxsize=None)
def case_f5(mrt, orc):
    sc = f5_scene(mrt)
    osc = orc.OracleScene(mrt.flatten_scene(sc, share=True), sc.lights, instancing=True)
    tris = F.Triangles(mrt.flatten_scene(sc))
    fam, pairs = f5_instance_neg_zero(mrt, sc)
    return _finish(sc, osc, tris, {"F5": fam}, pairs)


def _finish(sc, osc, tris, fams, pairs):
    closest, occluded, judged = {}, {}, {}
    for name, fam in fams.items():
        closest[name] = osc.intersect_closest(fam.rays, brute=True); occluded[name] = osc.intersect_any(fam.rays, brute=True)
        closest[name].setflags(write=False); occluded[name].setflags(write=False)
        judged[name] = judge64(tris, fam.rays, no_grazing=name == "F3")
    return Case(sc, osc, tris, fams, closest, occluded, judged, pairs)


def judged_mask(name, fam):
    """which rays of a family float64 may judge: all — but of F4 only the base rays: every other case puts an end of the interval ON the float32 hit distance, where the
    answer is the float32 test's by definition (the oracle's brute force defines it)"""
    return fam.tags == "base" if name == "F4" else np.ones(len(fam.tags), bool)
