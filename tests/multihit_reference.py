"""numpy restatement of the all-hits query (include/mrt_abi.h mrt_scene_intersect_all_device; csrc/multihit.hip): per ray the K smallest hits under the key
(distance, global triangle id), ascending, found by testing EVERY triangle against every ray — no tree, no bound, no list that could lose a candidate.

TEST INFRASTRUCTURE.  Built from the host Scene alone (flatten_scene's tuples: positions, transforms, index lists), float32 throughout:
  * world-space triangles as the flatten step makes them: p' = fma(c2, z, fma(c1, y, c0 * x)) + c3 per axis, then v0, e1 = v1 - v0, e2 = v2 - v0;
  * tri_test (csrc/traverse.h) in its exact operation order, including the explicit fused multiply-adds of fdot / fcross (csrc/device_math.h);
  * global ids instance-major, then geometry, then primitive; keys sorted; the first K kept.
tests/test_multihit_cpu.py pins it to the oracle's brute-force closest hit for K = 1 with no GPU; tests/test_multihit_device.py compares the kernels with it bit for bit.

The fused multiply-add.  numpy has none, and float32(float64(a) * b + c) is NOT one: the float64 sum is rounded before the float32 rounding, and the two roundings
together can differ from the single rounding of the exact value (double rounding).  fma() below is exact, by this argument:
  1. p = float64(a) * float64(b) is exact: two 24-bit significands give at most 48 bits, and the exponent range of a float32 product lies inside float64's.
  2. s = p + float64(c) is rounded once to float64, and two-sum gives its error e = (p + c) - s exactly (Knuth; no overflow possible at these magnitudes).
  3. Rounding to float32 is monotonic, so float32(s) differs from float32(p + c) only when a rounding boundary of float32 — a midpoint between two neighbouring float32
     values — lies between s and the exact sum p + c, s included.  A midpoint is itself a float64 value (25 significant bits, or a multiple of 2^-150 below the normal
     range), and s is the float64 NEAREST to the exact sum; so a midpoint strictly between them would be a float64 nearer than s: impossible.  The only case left is s
     sitting exactly ON a midpoint while the exact sum does not (e != 0): ties-to-even then decides by parity what the exact sum decides by the sign of e.
  4. In that case s is moved one float64 ulp towards the sign of e: the moved value lies on the exact sum's side of the midpoint and no other midpoint is that near, so
     its float32 rounding is the exact sum's.
Results that overflow float32 round to infinity either way; NaN and infinite operands give what the fused instruction gives (the sum is then NaN or infinite in float64 too)."""
import numpy as np

f32 = np.float32
INTERSECTION_DTYPE = np.dtype([("type", np.int32), ("distance", np.float32), ("instance_id", np.int32), ("geometry_id", np.int32),
                               ("primitive_id", np.int32), ("u", np.float32), ("v", np.float32), ("_pad", np.int32)])
_TWO_149 = np.float64(2.0) ** 149
_MIN_NORMAL = np.float64(2.0) ** -126


def miss_record():
    m = np.zeros((), INTERSECTION_DTYPE)
    m["distance"] = -1.0; m["instance_id"] = m["geometry_id"] = m["primitive_id"] = -1
    return m


def _on_f32_midpoint(s):
    """s float64, finite -> True where s lies exactly halfway between two neighbouring float32 values"""
    a = np.abs(s)
    normal = a >= _MIN_NORMAL
    bits = a.view(np.uint64) & np.uint64((1 << 29) - 1)              # the 29 bits float32 drops: a midpoint has exactly the first of them set
    mid = normal & (bits == np.uint64(1 << 28))
    if not normal.all():                                             # below the normal range float32 values are the multiples of 2^-149
        x = a[~normal] * _TWO_149                                    # (exact: a power of two, no underflow)
        mid[~normal] = (x - np.floor(x)) == 0.5
    return mid


def fma(a, b, c):
    """float32(a * b + c) with ONE rounding, elementwise on float32 arrays (the argument is in the module's docstring)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    if a.ndim == 0: return fma(a.reshape(1), b.reshape(1), c.reshape(1))[0]
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        fix = np.isfinite(s)
        fix[fix] = _on_f32_midpoint(s[fix])
        if fix.any():
            pf, cf, sf = p[fix], c64[fix], s[fix]
            bv = sf - pf                                             # two-sum: e = (p + c) - s exactly
            e = (pf - (sf - bv)) + (cf - bv)
            s = s.copy()
            s[fix] = np.where(e > 0, np.nextafter(sf, np.inf), np.where(e < 0, np.nextafter(sf, -np.inf), sf))
        return s.astype(f32)


def _fdot(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def _fcross(a, b):
    return (fma(a[1], b[2], -(a[2] * b[1])), fma(a[2], b[0], -(a[0] * b[2])), fma(a[0], b[1], -(a[1] * b[0])))


def _xorsign(v, sgn):
    return (v.view(np.uint32) ^ sgn).view(f32)


class MultihitReference:
    def __init__(self, entries):
        """entries: flatten_scene(scene) tuples (positions, normals, transform16 column-major, [(indices, Material)])"""
        self.entries = [dict(positions=np.asarray(e[0], f32).reshape(-1, 3), xf=np.asarray(e[2], f32).reshape(16).copy(),
                             indices=[np.asarray(i, np.uint32).reshape(-1, 3) for i, _ in e[3]]) for e in entries]
        self._flatten()

    def set_mesh(self, mesh_id, positions):
        self.entries[mesh_id]["positions"] = np.asarray(positions, f32).reshape(-1, 3)
        self._flatten()

    def _flatten(self):
        v0, e1, e2, ids = [], [], [], []
        for i, e in enumerate(self.entries):
            p, m = e["positions"], e["xf"]
            w = np.stack([fma(m[8 + k], p[:, 2], fma(m[4 + k], p[:, 1], m[k] * p[:, 0])) + m[12 + k] for k in range(3)], axis=1).astype(f32)
            for g, ix in enumerate(e["indices"]):
                a = w[ix[:, 0]]
                v0.append(a); e1.append(w[ix[:, 1]] - a); e2.append(w[ix[:, 2]] - a)
                ids.append(np.stack([np.full(len(ix), i, np.int32), np.full(len(ix), g, np.int32), np.arange(len(ix), dtype=np.int32)], axis=1))
        cat = lambda parts, width, kind: np.concatenate(parts).astype(kind) if parts else np.zeros((0, width), kind)
        self.v0, self.e1, self.e2, self.ids = cat(v0, 3, f32), cat(e1, 3, f32), cat(e2, 3, f32), cat(ids, 3, np.int32)

    @property
    def triangles(self):
        return self.v0.shape[0]

    def _tri_test(self, ri, ti, o, d, tmin, tmax):
        """tri_test for the pairs (ray ri[k], triangle ti[k]), its rejections in its order -> (indices into the pairs that hit, t, U, V, ad of those)"""
        keep = np.arange(ri.size)
        with np.errstate(all="ignore"):
            d_ = [d[ri, k] for k in range(3)]; e2 = [self.e2[ti, k] for k in range(3)]; e1 = [self.e1[ti, k] for k in range(3)]
            pv = _fcross(d_, e2)
            det = _fdot(e1, pv)
            ok = det != 0
            keep = keep[ok]; ri = ri[ok]; ti = ti[ok]; det = det[ok]; pv = [c[ok] for c in pv]
            ad = np.abs(det)
            sgn = det.view(np.uint32) & np.uint32(0x80000000)
            tv = [o[ri, k] - self.v0[ti, k] for k in range(3)]
            U = _xorsign(_fdot(tv, pv), sgn)
            ok = (U >= 0) & (U <= ad)
            keep = keep[ok]; ri = ri[ok]; ti = ti[ok]; ad = ad[ok]; sgn = sgn[ok]; U = U[ok]; tv = [c[ok] for c in tv]
            e1 = [self.e1[ti, k] for k in range(3)]
            q = _fcross(tv, e1)
            V = _xorsign(_fdot([d[ri, k] for k in range(3)], q), sgn)
            ok = (V >= 0) & (U + V <= ad)
            keep = keep[ok]; ri = ri[ok]; ti = ti[ok]; ad = ad[ok]; sgn = sgn[ok]; U = U[ok]; V = V[ok]; q = [c[ok] for c in q]
            T = _xorsign(_fdot([self.e2[ti, k] for k in range(3)], q), sgn)
            t = T / ad
            ok = (t >= tmin[ri]) & (t <= tmax[ri])
        return keep[ok], t[ok], U[ok], V[ok], ad[ok]

    def intersect_all(self, rays, max_hits, pairs_per_chunk=1 << 22):
        """rays (n, 8) float32 -> (hits (n, max_hits) INTERSECTION_DTYPE, counts (n,) int32)"""
        rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
        n, T, K = rays.shape[0], self.triangles, int(max_hits)
        hits = np.empty((n, K), INTERSECTION_DTYPE); hits[:] = miss_record()
        counts = np.zeros(n, np.int32)
        if n == 0 or T == 0: return hits, counts
        o, d, tmin, tmax = rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
        step = max(1, pairs_per_chunk // T)
        tri = np.arange(T, dtype=np.int64)
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            ri = np.repeat(np.arange(r0, r1, dtype=np.int64), T); ti = np.tile(tri, r1 - r0)
            k, t, U, V, ad = self._tri_test(ri, ti, o, d, tmin, tmax)
            ri, ti = ri[k], ti[k]
            order = np.lexsort((ti, t, ri))                          # by ray, then distance, then global id
            ri, ti, t, U, V, ad = ri[order], ti[order], t[order], U[order], V[order], ad[order]
            first = np.searchsorted(ri, ri)                          # position of the ray's first hit
            rank = np.arange(ri.size) - first
            sel = rank < K
            ri, ti, t, U, V, ad, rank = ri[sel], ti[sel], t[sel], U[sel], V[sel], ad[sel], rank[sel]
            rec = np.zeros(ri.size, INTERSECTION_DTYPE)
            rec["type"] = 1; rec["distance"] = t
            rec["instance_id"] = self.ids[ti, 0]; rec["geometry_id"] = self.ids[ti, 1]; rec["primitive_id"] = self.ids[ti, 2]
            with np.errstate(all="ignore"):
                rec["u"] = U / ad; rec["v"] = V / ad
            hits[ri, rank] = rec
            np.add.at(counts, ri, 1)
        return hits, counts


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b):
    """number of records of two structured arrays of one shape that differ in any bit"""
    x = np.ascontiguousarray(a).view(np.uint8).reshape(-1, a.dtype.itemsize); y = np.ascontiguousarray(b).view(np.uint8).reshape(-1, b.dtype.itemsize)
    return int((x != y).any(-1).sum())


# ---------------------------------------------------------------- scenes the two test files share
class _Raw:
    """stands in for Model: one mesh from arrays, under the identity"""
    def __init__(self, mrt, name, pos, nrm, idx, material):
        self.name = name
        self.meshes = [mrt.Mesh(name, pos, nrm, [mrt.Submesh(name, idx, material)], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 1.0)]


def raw_scene(mrt, meshes):
    """a Scene of the meshes [(positions, indices, Material)], in that order, each under the identity"""
    class Raw(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = [_Raw(mrt, f"mesh{k}", np.asarray(p, f32), np.tile(np.array([0, 0, -1], f32), (len(p), 1)), np.asarray(i, np.uint32), m) for k, (p, i, m) in enumerate(meshes)]
    sc = Raw((8, 8))
    assert all(np.array_equal(m.transform, np.eye(4, dtype=f32)) for m in sc.meshes)
    return sc


def _plain(mrt, dissolve=1.0, ior=1.0):
    m = mrt.Material()
    m.baseColor = mrt.Float3(0.5, 0.5, 0.5); m.dissolve = float(dissolve); m.refractionIndex = float(ior)
    return m


def quad(z):
    """the unit quad at height z: two triangles sharing the diagonal (0,0) - (1,1); triangle 0 holds x >= y, triangle 1 x <= y"""
    return np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], f32), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def quad_stack(mrt, layers, dissolve=None):
    """`layers` axis-aligned unit quads at z = 1 .. layers, one mesh each: power-of-two coordinates, so every distance along +z is exact.  Quad k (0-based) holds the
    global ids 2k and 2k + 1.  dissolve: per quad, optional (with a refraction index: the materials extension's partial transparency)."""
    return raw_scene(mrt, [(*quad(float(k + 1)), _plain(mrt) if dissolve is None else _plain(mrt, dissolve[k], 1.5)) for k in range(layers)])
