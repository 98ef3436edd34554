// surface.hip — hit records resolved to surface data on device buffers, ordered on a stream of the caller's (mrt_scene_resolve_hits_device /
// mrt_scene_interpolate_device).  The step the reference's kernel takes right after its intersector call: interpolateVertexAttribute, the
// instance transform of the normal and the resource-table lookup (Raytracing.metal:63-72, :261-269) — shade_entry's expressions (shade.h) in its order, on the
// caller's own rays and hit records.  No traversal, no shading kernel and no builder is touched.
//
//   k_resolve_hits   one thread per hit: 2 + 2 x 16 B of ray and record, one 16-byte row of the slot table, the triangle's shading record, three normals, three
//                    columns, one colour — all 16-byte gathers — and four 16-byte stores
//   k_interpolate    one thread per (hit, group of four channels): the lanes of a hit read consecutive dwords of the same three rows (one 64-byte request per
//                    row at 16 channels) and the wave's stores are contiguous; at three channels there is one group per hit and the kernel IS one thread per hit
//
// A caller's record is never trusted with an address: instance and geometry are checked against the table's extent, the primitive against its slot's triangle
// count, before anything is indexed with them.  The table (SurfaceWorkspace) restates what the commit knows on the host — per resource slot the first shading
// record, the triangle count, the vertex base of the instance's normals and the distance from the library's vertex numbering to the caller's — so both scene
// forms and every layout take the same path: the tree is not read at all.
#include "scene_device.h"
#include "device_math.h"
#include <algorithm>

namespace mrt {
namespace {

struct SurfaceView {
    const uint4 *slots;          // per resource slot: {first shading record, triangles, vertex base in `normals`, caller row - library vertex id}
    const uint4 *tri_shade;
    const float4 *normals, *inst_cols, *base_color;
    uint32_t instances, max_sub;
};

// the record's ids checked against the table; on success the slot and its row
MRT_DEV bool surface_slot(const SurfaceView &s, const uint4 h0, const uint4 h1, uint32_t &rslot, uint4 &row) {
    const uint32_t inst = h0.z, geom = h0.w;          // (a negative id is a large unsigned one)
    if (h0.x != 1u || inst >= s.instances || geom >= s.max_sub) return false;
    rslot = inst * s.max_sub + geom;
    row = s.slots[rslot];
    return h1.x < row.y;
}

// `count` (here and in k_interpolate): null, or the caller's device-side row count — read once, as a uniform scalar load; the rows at and past min(cap, *count) are not touched
__global__ void __launch_bounds__(256) k_resolve_hits(const SurfaceView s, const float4 *__restrict__ rays, const uint4 *__restrict__ hits, const uint32_t cap, const uint32_t *__restrict__ count,
                                                      float4 *__restrict__ out) {
    const uint32_t n = count ? min(cap, *count) : cap;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint4 h0 = hits[2 * (size_t)i], h1 = hits[2 * (size_t)i + 1];
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, -1.0f), o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o2 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    float4 o3 = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), 0.0f);
    uint32_t rslot; uint4 row;
    if (surface_slot(s, h0, h1, rslot, row)) {
        const float4 A = rays[2 * (size_t)i], B = rays[2 * (size_t)i + 1];
        const float t = __uint_as_float(h0.y), bu = __uint_as_float(h1.y), bv = __uint_as_float(h1.z);
        const uint32_t inst = h0.z, vb = row.z;
        const f3 P = mk3(A) + mk3(B) * t;                                // :261
        const float bw = 1.0f - bu - bv;                                 // :63-64
        const uint4 ts = s.tri_shade[row.x + h1.x];
        const f3 n_obj = (bu * mk3(s.normals[vb + ts.y]) + bv * mk3(s.normals[vb + ts.z])) + bw * mk3(s.normals[vb + ts.x]);   // :66-72
        const f3 c0 = mk3(s.inst_cols[inst * 4 + 0]), c1 = mk3(s.inst_cols[inst * 4 + 1]), c2 = mk3(s.inst_cols[inst * 4 + 2]);
        const f3 n_w = mk3((c0.x * n_obj.x + c1.x * n_obj.y) + c2.x * n_obj.z,
                           (c0.y * n_obj.x + c1.y * n_obj.y) + c2.y * n_obj.z,
                           (c0.z * n_obj.x + c1.z * n_obj.y) + c2.z * n_obj.z);   // :267
        const f3 nrm = normalize3(n_w);                                  // :268
        const float4 surf = s.base_color[rslot];                         // :262-269
        o0 = make_float4(P.x, P.y, P.z, t);
        o1 = make_float4(nrm.x, nrm.y, nrm.z, __int_as_float(1));
        o2 = make_float4(surf.x, surf.y, surf.z, __uint_as_float(rslot));
        o3 = make_float4(__uint_as_float(inst), __uint_as_float(h0.w), __uint_as_float(h1.x), 0.0f);
    }
    float4 *const o = out + 4 * (size_t)i;
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

// VEC: attribute rows, output rows and both bases are 16-byte aligned and the channel count is a multiple of four — one 16-byte load per row, one 16-byte store
template <bool VEC>
__global__ void __launch_bounds__(256) k_interpolate(const SurfaceView s, const uint4 *__restrict__ hits, const uint32_t cap, const uint32_t *__restrict__ count, const uint32_t groups,
                                                     const uint32_t channels, const char *__restrict__ attr, const size_t attr_stride, char *__restrict__ out, const size_t out_stride) {
    const uint64_t work = (uint64_t)(count ? min(cap, *count) : cap) * groups;
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w >= work) return;
    const uint32_t i = (uint32_t)(w / groups), c0 = 4u * (uint32_t)(w % groups);
    const uint32_t nc = channels - c0 < 4u ? channels - c0 : 4u;
    const uint4 h0 = hits[2 * (size_t)i], h1 = hits[2 * (size_t)i + 1];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t rslot; uint4 row;
    if (surface_slot(s, h0, h1, rslot, row)) {
        const float bu = __uint_as_float(h1.y), bv = __uint_as_float(h1.z);
        const float bw = (1.0f - bu) - bv;
        const uint4 ts = s.tri_shade[row.x + h1.x];
        const float *const a0 = reinterpret_cast<const float *>(attr + (size_t)(ts.x + row.w) * attr_stride) + c0;
        const float *const a1 = reinterpret_cast<const float *>(attr + (size_t)(ts.y + row.w) * attr_stride) + c0;
        const float *const a2 = reinterpret_cast<const float *>(attr + (size_t)(ts.z + row.w) * attr_stride) + c0;
        float x0[4], x1[4], x2[4];
        if (VEC) {
            const float4 q0 = *reinterpret_cast<const float4 *>(a0), q1 = *reinterpret_cast<const float4 *>(a1), q2 = *reinterpret_cast<const float4 *>(a2);
            x0[0] = q0.x; x0[1] = q0.y; x0[2] = q0.z; x0[3] = q0.w; x1[0] = q1.x; x1[1] = q1.y; x1[2] = q1.z; x1[3] = q1.w; x2[0] = q2.x; x2[1] = q2.y; x2[2] = q2.z; x2[3] = q2.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) { const bool on = k < nc; x0[k] = on ? a0[k] : 0.0f; x1[k] = on ? a1[k] : 0.0f; x2[k] = on ? a2[k] : 0.0f; }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = (bu * x1[k] + bv * x2[k]) + bw * x0[k];          // :66-72
    }
    float *const o = reinterpret_cast<float *>(out + (size_t)i * out_stride) + c0;
    if (VEC) *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (k < nc) o[k] = v[k];
    }
}

SurfaceView surface_view(const DeviceScene &sc) {
    const SurfaceWorkspace &w = *sc.surface_ws;
    SurfaceView v;
    v.slots = w.slots.p; v.tri_shade = sc.tri_shade.p; v.normals = sc.normals.p; v.inst_cols = sc.inst_cols.p; v.base_color = sc.base_color.p;
    v.instances = w.instances; v.max_sub = w.max_sub;
    return v;
}

}  // namespace

// The caller's vertex numbering: source meshes concatenated in mesh-id order, an instance sharing its source's rows.  meshes + 1 entries, the last one the total.
void surface_vertex_offsets(const std::vector<HostMesh> &meshes, std::vector<uint64_t> &offsets) {
    offsets.assign(meshes.size() + 1, 0);
    uint64_t V = 0;
    for (size_t i = 0; i < meshes.size(); i++) if (meshes[i].source < 0) { offsets[i] = V; V += meshes[i].positions.size() / 3; }
    for (size_t i = 0; i < meshes.size(); i++) if (meshes[i].source >= 0) offsets[i] = offsets[(size_t)meshes[i].source];
    offsets[meshes.size()] = V;
}

// The slot table of a committed scene, made on first use (it allocates, uploads and blocks) and dropped by the next commit.
int surface_prepare(const std::vector<HostMesh> &meshes, DeviceScene &sc) {
    if (sc.surface_ws) return MRT_OK;
    const size_t I = meshes.size(), max_sub = (size_t)std::max(sc.stats.max_submeshes, 1);
    const bool two_level = sc.num_inst != 0;
    if (sc.base_color.n != std::max<size_t>(I * max_sub, 1) || (two_level && (sc.h_inst.size() != I || sc.num_inst != I)) || I >= 65536 || max_sub >= 65536) {
        set_error("surface tables: the resident scene is not this scene's"); return MRT_ERR_STATE;
    }
    std::vector<uint64_t> offs; surface_vertex_offsets(meshes, offs);
    if (offs[I] >= 0xFFFFFFF0ull) { set_error("surface tables: too many vertices"); return MRT_ERR_UNSUPPORTED; }
    std::vector<uint4> rows(std::max<size_t>(I * max_sub, 1), make_uint4(0, 0, 0, 0));
    uint32_t gid = 0, vflat = 0;          // flattened scenes: the running global triangle id and vertex base, instance-major as build_flat lays them out
    for (size_t i = 0; i < I; i++) {
        const HostMesh &g = meshes[i].source >= 0 ? meshes[(size_t)meshes[i].source] : meshes[i];
        if (g.sub_indices.size() > max_sub) { set_error("surface tables: the resident scene is not this scene's"); return MRT_ERR_STATE; }
        uint32_t rec = two_level ? sc.h_inst[i].ts_base : gid;          // a two-level scene's shading records belong to the BLAS, numbered geometry-major inside it
        for (size_t s = 0; s < g.sub_indices.size(); s++) {
            const uint32_t nt = (uint32_t)(g.sub_indices[s].size() / 3);
            rows[i * max_sub + s] = two_level ? make_uint4(rec, nt, sc.h_inst[i].vbase, (uint32_t)offs[i])          // BLAS-local vertex ids
                                              : make_uint4(rec, nt, 0u, (uint32_t)offs[i] - vflat);                // ids already carry the flattened instance's base (mod 2^32)
            rec += nt;
        }
        if (!two_level) { gid = rec; vflat += (uint32_t)(g.positions.size() / 3); }
    }
    const size_t records = two_level ? sc.tri_shade.n : (size_t)gid;
    if (!two_level && records > sc.tri_shade.n) { set_error("surface tables: the resident scene is not this scene's"); return MRT_ERR_STATE; }
    if (two_level) for (size_t i = 0; i < I; i++) if ((size_t)sc.h_inst[i].ts_base + sc.h_inst[i].ntri > records) { set_error("surface tables: the resident scene is not this scene's"); return MRT_ERR_STATE; }
    std::unique_ptr<SurfaceWorkspace> w(new SurfaceWorkspace());
    MRT_HIP(w->slots.alloc(rows.size()));
    MRT_HIP(hipMemcpy(w->slots.p, rows.data(), rows.size() * sizeof(uint4), hipMemcpyHostToDevice));
    w->instances = (uint32_t)I; w->max_sub = (uint32_t)max_sub; w->vertices = offs[I];
    sc.surface_ws = std::move(w);
    return MRT_OK;
}

void drop_surface_workspace(DeviceScene &sc) { sc.surface_ws.reset(); }

int resolve_hits_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, const void *d_count) {
    hipLaunchKernelGGL(k_resolve_hits, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, surface_view(sc), static_cast<const float4 *>(d_rays), static_cast<const uint4 *>(d_hits),
                       (uint32_t)n, static_cast<const uint32_t *>(d_count), static_cast<float4 *>(d_surfaces));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int interpolate_device(const DeviceScene &sc, hipStream_t stream, const void *d_hits, size_t n, const void *d_attr, size_t attr_stride, uint32_t channels, void *d_out, size_t out_stride,
                       const void *d_count) {
    const uint32_t groups = (channels + 3) / 4;
    const uint64_t work = (uint64_t)n * groups;          // n < 2^31, groups <= 16: 2^27 workgroups at the most (the grid is sized by the capacity, whatever the count)
    const uint32_t *const cnt = static_cast<const uint32_t *>(d_count);
    const bool vec = channels % 4 == 0 && attr_stride % 16 == 0 && out_stride % 16 == 0 && (uintptr_t)d_attr % 16 == 0 && (uintptr_t)d_out % 16 == 0;
    const dim3 grid((uint32_t)((work + 255) / 256));
    if (vec) hipLaunchKernelGGL(k_interpolate<true>, grid, dim3(256), 0, stream, surface_view(sc), static_cast<const uint4 *>(d_hits), (uint32_t)n, cnt, groups, channels, static_cast<const char *>(d_attr), attr_stride, static_cast<char *>(d_out), out_stride);
    else hipLaunchKernelGGL(k_interpolate<false>, grid, dim3(256), 0, stream, surface_view(sc), static_cast<const uint4 *>(d_hits), (uint32_t)n, cnt, groups, channels, static_cast<const char *>(d_attr), attr_stride, static_cast<char *>(d_out), out_stride);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
