// build_common.h — what the two translation units of the builder share: bvh_build.hip (the build kernels and the build driver) and bvh_refit.hip (the refit of the
// resident layouts, blocking and stream-ordered).  File-local in each of them (anonymous namespace): k_flatten is a kernel of both.
#pragma once
#include "scene_device.h"
#include "device_math.h"
#include <algorithm>
#include <cstring>
#include <cmath>
#include <vector>

namespace mrt {
namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;

struct SubRec { uint32_t tri_begin, tri_count, index_offset, vbase, inst, geom; };

__device__ __forceinline__ uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ float ord2f(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; memcpy(&f, &u, 4); return f;
#endif
}

__device__ __forceinline__ float wave_min(float v) { for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }

// ------------------------------------------------------------------ flatten
__global__ void k_flatten(const SubRec *__restrict__ recs, int nrec, const float *__restrict__ pos,
                          const uint32_t *__restrict__ indices, const float4 *__restrict__ inst_cols, uint32_t T,
                          float4 *__restrict__ tri_world, uint4 *__restrict__ tri_shade,
                          float4 *__restrict__ leaf_lo, float4 *__restrict__ leaf_hi, uint32_t *__restrict__ cbounds) {
    uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    float c[3] = {0, 0, 0};
    bool valid = gid < T;
    if (valid) {
        int lo = 0, hi = nrec - 1;                       // last record with tri_begin <= gid
        while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (recs[mid].tri_begin <= gid) lo = mid; else hi = mid - 1; }
        SubRec r = recs[lo];
        uint32_t p = gid - r.tri_begin;
        const uint32_t *ix = indices + r.index_offset + 3 * (size_t)p;
        uint32_t i0 = ix[0] + r.vbase, i1 = ix[1] + r.vbase, i2 = ix[2] + r.vbase;
        float4 c0 = inst_cols[r.inst * 4 + 0], c1 = inst_cols[r.inst * 4 + 1], c2 = inst_cols[r.inst * 4 + 2], c3 = inst_cols[r.inst * 4 + 3];
        f3 w[3];
        uint32_t vi[3] = {i0, i1, i2};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float x = pos[3 * (size_t)vi[k]], y = pos[3 * (size_t)vi[k] + 1], z = pos[3 * (size_t)vi[k] + 2];
            // world = M * (p,1), fused form of mrt-math v1
            w[k].x = __builtin_fmaf(c2.x, z, __builtin_fmaf(c1.x, y, c0.x * x)) + c3.x;
            w[k].y = __builtin_fmaf(c2.y, z, __builtin_fmaf(c1.y, y, c0.y * x)) + c3.y;
            w[k].z = __builtin_fmaf(c2.z, z, __builtin_fmaf(c1.z, y, c0.z * x)) + c3.z;
        }
        f3 e1 = w[1] - w[0], e2 = w[2] - w[0];
        tri_world[3 * (size_t)gid + 0] = make_float4(w[0].x, w[0].y, w[0].z, __uint_as_float(gid));
        tri_world[3 * (size_t)gid + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
        tri_world[3 * (size_t)gid + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
        tri_shade[gid] = make_uint4(i0, i1, i2, (r.inst << 16) | r.geom);
        float blo[3], bhi[3];
        blo[0] = fminf(w[0].x, fminf(w[1].x, w[2].x)); bhi[0] = fmaxf(w[0].x, fmaxf(w[1].x, w[2].x));
        blo[1] = fminf(w[0].y, fminf(w[1].y, w[2].y)); bhi[1] = fmaxf(w[0].y, fmaxf(w[1].y, w[2].y));
        blo[2] = fminf(w[0].z, fminf(w[1].z, w[2].z)); bhi[2] = fmaxf(w[0].z, fmaxf(w[1].z, w[2].z));
#pragma unroll
        for (int k = 0; k < 3; k++) {   // pad: the slab test must never reject what the triangle test accepts
            float m = fmaxf(fabsf(blo[k]), fabsf(bhi[k]));
            float e = 1e-5f * m + 1e-6f;
            blo[k] -= e; bhi[k] += e;
            c[k] = 0.5f * (blo[k] + bhi[k]);
        }
        leaf_lo[gid] = make_float4(blo[0], blo[1], blo[2], 0.0f);
        leaf_hi[gid] = make_float4(bhi[0], bhi[1], bhi[2], 0.0f);
    }
    // bounds of the centres: wave, then workgroup (LDS), then one set of atomics per workgroup — the six words take ~90 atomics per microsecond, and one set per
    // wave (14 K waves for 885 K triangles) was the whole duration of this kernel (0.95 ms)
    const float BIG = 3.0e38f;
    __shared__ float smn[3][16], smx[3][16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float mn = wave_min(valid ? c[k] : BIG), mx = wave_max(valid ? c[k] : -BIG);
        if (lane == 0) { smn[k][wv] = mn; smx[k][wv] = mx; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        float mn = BIG, mx = -BIG;
        for (uint32_t i = 0; i < nw; i++) { mn = fminf(mn, smn[k][i]); mx = fmaxf(mx, smx[k][i]); }
        if (mn <= mx) { atomicMin(&cbounds[k], f2ord(mn)); atomicMax(&cbounds[3 + k], f2ord(mx)); }
    }
}

__device__ __forceinline__ float box_area(float4 lo, float4 hi) {
    float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
    return 2.0f * (dx * dy + dy * dz + dz * dx);
}

// 16-byte write-through stores and sc1 loads: the hand-off of the bottom-up passes (bvh_build.hip k_refit, where it is explained; bvh_refit.hip k_rope_refit)
typedef unsigned int refit_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t refit_rsrc(const void *p) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)0xFFFFFFF0u, 0x00020000); }
__device__ __forceinline__ float4 refit_ld_wt(__amdgpu_buffer_rsrc_t r, uint32_t index) {
    const refit_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, index * 16u, 0, 16);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void refit_st_wt(__amdgpu_buffer_rsrc_t r, uint32_t index, float4 a) {
    refit_u32x4 v; v.x = __float_as_uint(a.x); v.y = __float_as_uint(a.y); v.z = __float_as_uint(a.z); v.w = __float_as_uint(a.w);
    __builtin_amdgcn_raw_buffer_store_b128(v, r, index * 16u, 0, 16);
}

// ------------------------------------------------------------------ host helpers
struct EventPair {           // destroyed on every return path
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// empty bounds as order-preserving uints (f2ord): what atomicMin / atomicMax start from (k_flatten's cbounds, k_wide_cost's rbox)
const uint32_t BOUNDS_EMPTY[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};

static inline void set_root_box(float lo[3], float hi[3], float4 a, float4 b) { lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z; }

// first node of every level of an 8-wide tree whose levels (BFS numbering) hold levels[L] nodes and whose root is node `base`
static inline std::vector<uint32_t> level_first(const std::vector<uint32_t> &levels, uint32_t base) {
    std::vector<uint32_t> first(levels.size(), base);
    for (size_t L = 1; L < levels.size(); L++) first[L] = first[L - 1] + levels[L - 1];
    return first;
}

}  // namespace
}  // namespace mrt
