"""numpy restatement of the surface entries (include/mrt_abi.h mrt_scene_resolve_hits_device / mrt_scene_interpolate_device; csrc/surface.hip): what the reference's
kernel does right after its intersector call — interpolateVertexAttribute, the instance transform of the normal, the resource-table lookup (Raytracing.metal:63-72,
:261-269).

TEST INFRASTRUCTURE.  float32 throughout, every operation in the order written here (numpy rounds each one: no contraction).  Built from the host Scene alone — meshes,
transforms and materials as flatten_scene hands them over, as denoise_reference.guides_from_dump builds its colour table — so it knows neither flattened nor two-level
layouts.  tests/test_surface_device_cpu.py pins it to the oracle's stage dumps with no GPU; tests/test_surface_device.py compares the kernels with it bit for bit."""
import functools

import numpy as np

f32 = np.float32
SURFACE_DTYPE = np.dtype([("position", np.float32, 3), ("distance", np.float32), ("normal", np.float32, 3), ("type", np.int32),
                          ("base_color", np.float32, 3), ("resource_slot", np.int32),
                          ("instance_id", np.int32), ("geometry_id", np.int32), ("primitive_id", np.int32), ("_pad", np.int32)])


def miss_record():
    m = np.zeros((), SURFACE_DTYPE)
    m["distance"] = -1.0; m["resource_slot"] = -1; m["instance_id"] = m["geometry_id"] = m["primitive_id"] = -1
    return m


class SurfaceReference:
    def __init__(self, entries):
        """entries: flatten_scene(scene, share=True) 5-tuples (positions, normals, transform16 column-major, [(indices, Material)], source) — or 4-tuples"""
        self.entries = []
        for e in entries:
            src = e[4] if len(e) > 4 else -1
            pos, nrm, xf, subs = e[:4] if src < 0 else entries[src][:4]
            self.entries.append(dict(normals=np.asarray(nrm, f32).reshape(-1, 3), positions=np.asarray(pos, f32).reshape(-1, 3), xf=np.asarray(e[2], f32).reshape(16).copy(),
                                     indices=[np.asarray(i, np.uint32).reshape(-1, 3) for i, _ in subs],
                                     colors=[np.asarray(m.baseColor.tolist()[:3], f32) for _, m in subs], source=int(src)))
        self.max_sub = max([len(e["indices"]) for e in self.entries] + [1])
        # the caller's vertex numbering: source meshes concatenated in mesh-id order, an instance sharing its source's rows
        self.offsets = np.zeros(len(self.entries) + 1, np.uint64)
        V = 0
        for i, e in enumerate(self.entries):
            if e["source"] < 0:
                self.offsets[i] = V; V += e["normals"].shape[0]
        for i, e in enumerate(self.entries):
            if e["source"] >= 0: self.offsets[i] = self.offsets[e["source"]]
        self.offsets[-1] = V

    def set_mesh(self, mesh_id, positions, normals):
        for i, e in enumerate(self.entries):
            if i == mesh_id or e["source"] == mesh_id:
                e["positions"] = np.asarray(positions, f32).reshape(-1, 3); e["normals"] = np.asarray(normals, f32).reshape(-1, 3)

    def set_transform(self, mesh_id, xf16):
        self.entries[mesh_id]["xf"] = np.asarray(xf16, f32).reshape(16).copy()

    def attribute(self, what):
        """the scene's own per-vertex `normals` or `positions` in the caller's numbering: (V, 3)"""
        return np.concatenate([e[what] for e in self.entries if e["source"] < 0] or [np.zeros((0, 3), f32)]).astype(f32)

    def _triangles(self, hits):
        """-> valid (n,) bool and, per valid record in order, (mesh entry index, vertex ids (3,))"""
        n = hits.shape[0]
        valid = np.zeros(n, bool)
        tri = np.zeros((n, 3), np.int64)
        I = len(self.entries)
        for k in range(n):
            h = hits[k]
            i, g, p = int(h["instance_id"]), int(h["geometry_id"]), int(h["primitive_id"])
            if int(h["type"]) != 1 or not 0 <= i < I or not 0 <= g < len(self.entries[i]["indices"]) or not 0 <= p < self.entries[i]["indices"][g].shape[0]:
                continue
            valid[k] = True
            tri[k] = self.entries[i]["indices"][g][p]
        return valid, tri

    def resolve(self, rays, hits):
        """rays (n, 8) float32, hits (n,) INTERSECTION_DTYPE -> (n,) SURFACE_DTYPE, shade_entry's expressions in its order"""
        rays = np.asarray(rays, f32).reshape(-1, 8)
        n = hits.shape[0]
        out = np.empty(n, SURFACE_DTYPE); out[:] = miss_record()
        valid, tri = self._triangles(hits)
        idx = np.flatnonzero(valid)
        if idx.size == 0: return out
        inst = hits["instance_id"][idx].astype(np.int64); geom = hits["geometry_id"][idx].astype(np.int64)
        t = hits["distance"][idx].astype(f32); bu = hits["u"][idx].astype(f32); bv = hits["v"][idx].astype(f32)
        P = rays[idx, 0:3] + rays[idx, 4:7] * t[:, None]                                       # :261
        bw = f32(1.0) - bu - bv                                                                # :63-64
        n0 = np.empty((idx.size, 3), f32); n1 = np.empty_like(n0); n2 = np.empty_like(n0); cols = np.empty((idx.size, 16), f32); col = np.empty((idx.size, 3), f32)
        for j, k in enumerate(idx):
            e = self.entries[inst[j]]
            n0[j], n1[j], n2[j] = e["normals"][tri[k, 0]], e["normals"][tri[k, 1]], e["normals"][tri[k, 2]]
            cols[j] = e["xf"]; col[j] = e["colors"][geom[j]]
        n_obj = (bu[:, None] * n1 + bv[:, None] * n2) + bw[:, None] * n0                       # :66-72
        c0, c1, c2 = cols[:, 0:3], cols[:, 4:7], cols[:, 8:11]
        n_w = (c0 * n_obj[:, 0:1] + c1 * n_obj[:, 1:2]) + c2 * n_obj[:, 2:3]                   # :267
        with np.errstate(all="ignore"):
            d = (n_w[:, 0] * n_w[:, 0] + n_w[:, 1] * n_w[:, 1]) + n_w[:, 2] * n_w[:, 2]
            inv = f32(1.0) / np.sqrt(d)
            nrm = n_w * inv[:, None]                                                           # :268
        out["position"][idx] = P; out["distance"][idx] = t; out["normal"][idx] = nrm; out["type"][idx] = 1
        out["base_color"][idx] = col; out["resource_slot"][idx] = (inst * self.max_sub + geom).astype(np.int32)
        out["instance_id"][idx] = inst; out["geometry_id"][idx] = geom; out["primitive_id"][idx] = hits["primitive_id"][idx]; out["_pad"][idx] = 0
        return out

    def interpolate(self, hits, attributes):
        """attributes (V, C) float32 in the caller's numbering -> (n, C): (u * a[i1] + v * a[i2]) + ((1 - u) - v) * a[i0]; zeros for a miss or an invalid id"""
        a = np.asarray(attributes, f32)
        assert a.shape[0] == int(self.offsets[-1])
        out = np.zeros((hits.shape[0], a.shape[1]), f32)
        valid, tri = self._triangles(hits)
        idx = np.flatnonzero(valid)
        if idx.size == 0: return out
        rows = tri[idx] + self.offsets[hits["instance_id"][idx].astype(np.int64)].astype(np.int64)[:, None]
        u = hits["u"][idx].astype(f32)[:, None]; v = hits["v"][idx].astype(f32)[:, None]
        out[idx] = (u * a[rows[:, 1]] + v * a[rows[:, 2]]) + ((f32(1.0) - u) - v) * a[rows[:, 0]]
        return out


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b):
    """number of records of two structured arrays that differ in any bit"""
    x = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], a.dtype.itemsize); y = np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], b.dtype.itemsize)
    return int((x != y).any(-1).sum())


# ---------------------------------------------------------------- the three scenes of the surface tests and the oracle's stage dump of each, made once
SEED = 3
CASES = {"cornell": (64, 64, False), "two_level": (64, 48, True), "no_dragon": (96, 54, False)}


def make_scene(mrt, name):
    w, h, _ = CASES[name]
    if name == "cornell": return mrt.CornellScene((w, h))
    if name == "two_level":
        from test_instancing import _scene
        return _scene(mrt, (w, h))
    sc = mrt.DragonScene((w, h))                                   # rotated, scaled, six submeshes (the train)
    sc.models = [m for m in sc.models if m.name != "dragon"]
    return sc


@functools.lru_cache(maxsize=None)
def case(mrt, orc, name):
    """-> dict: scene, entries (share=True), ref, dump (h, w, bounces, 16), per bounce b: rays[b] (m, 8), hits[b] (oracle records), pixels[b] (flat pixel indices of the
    records the dump holds at that bounce)"""
    w, h, instancing = CASES[name]
    sc = make_scene(mrt, name)
    shared = mrt.flatten_scene(sc, share=True)
    osc = orc.OracleScene(shared if instancing else mrt.flatten_scene(sc), sc.lights, instancing=instancing)
    orr = orc.OracleRenderer(osc, w, h, seed=SEED, max_bounces=3, camera=sc.camera)
    dump = orr.render(1, dump=True)
    out = dict(scene=sc, entries=shared, ref=SurfaceReference(shared), dump=dump, rays=[], hits=[], pixels=[], w=w, h=h, instancing=instancing)
    for b in range(dump.shape[2]):
        rec = dump[:, :, b, :].reshape(-1, 16)
        held = np.flatnonzero((rec[:, 3:6] != 0).any(-1))               # a bounce the path never reached leaves its record all zero
        rays = np.zeros((held.size, 8), f32)
        rays[:, 0:3] = rec[held, 0:3]; rays[:, 4:7] = rec[held, 3:6]; rays[:, 7] = np.inf
        hits = osc.intersect_closest(rays)
        for a in (rays, hits): a.setflags(write=False)
        out["rays"].append(rays); out["hits"].append(hits); out["pixels"].append(held)
    orr.close(); osc.close()
    return out
