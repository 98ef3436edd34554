// tlas_rebuild.hip — the topology of both TLAS forms of a two-level scene rebuilt on the caller's stream, for gfx950.
//
//   mrt_scene_rebuild_tlas_device   TlasBuilder and WideTlasBuilder (two_level.hip) split a range [first, first + count) at count / 2, so WHERE every range of the tree lies
//                                   depends on the instance count alone: node indices, the words a and b, escape links, depths and the refit's launch sizes are the last
//                                   commit's.  WHAT goes into each half is decided by a strict total order — (lo + hi on the axis, instance id), the axis the widest extent
//                                   of 0.5f * (lo + hi) over the range, y and z taking over only when strictly wider —, so the instance SET of every range is unique whatever
//                                   permutation the range held before.  A rebuild is therefore a re-sort of the instance ids under the skeleton: the full recursive median
//                                   order `ids`, down to ranges of one instance, from the world boxes the device holds (inst_box), then tlas_index[p] = ids[p],
//                                   wtlas_index[i] = ids[wide_pos[i]], then the refit of tlas_refit.hip.  The rope TLAS is the tree a commit would build, bit for bit; the
//                                   8-wide TLAS keeps the collapse choices of the last commit and gets fresh sets under them.
//
// A range of at most TLAS_RESORT_LDS_LIMIT = 1024 instances is finished by one workgroup in LDS, all its levels in one launch (k_resort_lds): 16 bytes per instance — the three
// sums lo + hi and the id —, 16 KB per workgroup.  Scenes up to that size are re-sorted by ONE launch.  Above it the upper levels take one step each, ping-pong between two id
// buffers of the workspace: k_resort_extent (one workgroup per range: its axis), k_resort_rank (rank by counting, the range tiled through LDS, and the scatter to first + rank).
// Counting is quadratic in the range, which is why TLAS_RESORT_MAX = 65 536 instances is the limit (the ABI's own is 65 535).  Every launch size is computed on the host from
// the count; nothing is allocated, copied from the host or waited for.
#include "scene_device.h"

namespace mrt {
namespace {

constexpr uint32_t RS_BLOCK = 256, RS_PER_THREAD = TLAS_RESORT_LDS_LIMIT / RS_BLOCK;
static_assert(RS_PER_THREAD * RS_BLOCK == TLAS_RESORT_LDS_LIMIT, "the LDS limit is a whole number of elements per thread");

// {lo + hi per axis (the builders' sort key; half of it is the centre their extents are taken of), id}
__device__ __forceinline__ float4 sums_of(const float4 *__restrict__ inst_box, uint32_t id) {
    const float4 lo = inst_box[4 * (size_t)id + 2], hi = inst_box[4 * (size_t)id + 3];
    return make_float4(lo.x + hi.x, lo.y + hi.y, lo.z + hi.z, __uint_as_float(id));
}
__device__ __forceinline__ float on_axis(const float4 &q, int ax) { return ax == 0 ? q.x : ax == 1 ? q.y : q.z; }
// the builders' comparator: x before y
__device__ __forceinline__ bool before(float kx, uint32_t x, float ky, uint32_t y) { return kx < ky || (kx == ky && x < y); }
// the builders' axis choice from the extents of the centres
__device__ __forceinline__ int widest_axis(const float clo[3], const float chi[3]) {
    int ax = 0;
    if (chi[1] - clo[1] > chi[ax] - clo[ax]) ax = 1;
    if (chi[2] - clo[2] > chi[ax] - clo[ax]) ax = 2;
    return ax;
}
// range `seg` of level `level` (its bits, most significant first, are the turns from the root: 1 = the upper half)
__device__ __forceinline__ void range_of_segment(uint32_t n, uint32_t level, uint32_t seg, uint32_t &first, uint32_t &count) {
    first = 0; count = n;
    for (uint32_t l = level; l-- > 0;) {
        const uint32_t half = count / 2;
        if ((seg >> l) & 1u) { first += half; count -= half; } else count = half;
    }
}

// ------------------------------------------------------------------ a range that fits one workgroup: every level below it, in LDS
// Workgroup b takes range b of level `level` of src[0, n) (count <= TLAS_RESORT_LDS_LIMIT by the host's choice of level) and writes its final order to dst — src == dst is
// fine, a workgroup reads its whole range before it writes — and, with wide_of_pos, to the 8-wide form's index array.
__global__ __launch_bounds__(RS_BLOCK) void k_resort_lds(const uint32_t *src, uint32_t *dst, uint32_t n, uint32_t level, const float4 *__restrict__ inst_box,
                                                         const uint32_t *__restrict__ wide_of_pos, uint32_t *__restrict__ wtlas_index) {
    __shared__ float4 arr[TLAS_RESORT_LDS_LIMIT];
    uint32_t first, count;
    range_of_segment(n, level, blockIdx.x, first, count);
    if (count > TLAS_RESORT_LDS_LIMIT) return;          // (never: the host picks the level; a wrong launch must not leave the array)
    for (uint32_t p = threadIdx.x; p < count; p += RS_BLOCK) arr[p] = sums_of(inst_box, src[first + p]);
    __syncthreads();
    for (uint32_t dl = 0; ((count - 1u) >> dl) >= 1u; dl++) {          // while the largest range of the local level, ceil(count / 2^dl), holds two or more
        float4 me[RS_PER_THREAD]; uint32_t to[RS_PER_THREAD];
        for (uint32_t i = 0; i < RS_PER_THREAD; i++) {
            const uint32_t p = threadIdx.x + i * RS_BLOCK;
            to[i] = p;
            if (p >= count) continue;
            me[i] = arr[p];
            uint32_t lf = 0, lc = count;          // the range of p at this level: count / 2 down from the workgroup's range
            for (uint32_t l = 0; l < dl && lc >= 2u; l++) {
                const uint32_t half = lc / 2;
                if (p < lf + half) lc = half; else { lf += half; lc -= half; }
            }
            if (lc < 2u) continue;
            const float BIG = 3.0e38f;
            float clo[3] = {BIG, BIG, BIG}, chi[3] = {-BIG, -BIG, -BIG};
            for (uint32_t j = lf; j < lf + lc; j++) {
                const float4 q = arr[j];
                const float c[3] = {0.5f * q.x, 0.5f * q.y, 0.5f * q.z};
                for (int k = 0; k < 3; k++) { clo[k] = fminf(clo[k], c[k]); chi[k] = fmaxf(chi[k], c[k]); }
            }
            const int ax = widest_axis(clo, chi);
            const float key = on_axis(me[i], ax); const uint32_t id = __float_as_uint(me[i].w);
            uint32_t rank = 0;
            for (uint32_t j = lf; j < lf + lc; j++) { const float4 q = arr[j]; rank += before(on_axis(q, ax), __float_as_uint(q.w), key, id) ? 1u : 0u; }
            to[i] = lf + rank;          // (< lf + lc: an element is not before itself)
        }
        __syncthreads();
        for (uint32_t i = 0; i < RS_PER_THREAD; i++) if (threadIdx.x + i * RS_BLOCK < count) arr[to[i]] = me[i];
        __syncthreads();
    }
    for (uint32_t p = threadIdx.x; p < count; p += RS_BLOCK) {
        const uint32_t id = __float_as_uint(arr[p].w);
        dst[first + p] = id;
        if (wide_of_pos) wtlas_index[wide_of_pos[first + p]] = id;
    }
}

// ------------------------------------------------------------------ ranges above the limit: one level per step
// one workgroup per range of the level: the axis its members are split on
__global__ __launch_bounds__(RS_BLOCK) void k_resort_extent(const uint32_t *__restrict__ src, uint32_t n, uint32_t level, const float4 *__restrict__ inst_box, uint32_t *__restrict__ seg_axis) {
    __shared__ float red[6][RS_BLOCK];
    uint32_t first, count;
    range_of_segment(n, level, blockIdx.x, first, count);
    const float BIG = 3.0e38f;
    float clo[3] = {BIG, BIG, BIG}, chi[3] = {-BIG, -BIG, -BIG};
    for (uint32_t p = threadIdx.x; p < count; p += RS_BLOCK) {
        const float4 q = sums_of(inst_box, src[first + p]);
        const float c[3] = {0.5f * q.x, 0.5f * q.y, 0.5f * q.z};
        for (int k = 0; k < 3; k++) { clo[k] = fminf(clo[k], c[k]); chi[k] = fmaxf(chi[k], c[k]); }
    }
    for (int k = 0; k < 3; k++) { red[k][threadIdx.x] = clo[k]; red[3 + k][threadIdx.x] = chi[k]; }
    __syncthreads();
    for (uint32_t s = RS_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) for (int k = 0; k < 3; k++) {
            red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]); red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float lo[3] = {red[0][0], red[1][0], red[2][0]}, hi[3] = {red[3][0], red[4][0], red[5][0]};
        seg_axis[blockIdx.x] = (uint32_t)widest_axis(lo, hi);
    }
}

// blockIdx.y = the range, blockIdx.x = a tile of 256 of its members: each member's rank under (key on the range's axis, id) by counting over the range, 256 members at a time
// through LDS, and the scatter dst[first + rank] = id.  src and dst are different buffers.
__global__ __launch_bounds__(RS_BLOCK) void k_resort_rank(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n, uint32_t level, const float4 *__restrict__ inst_box,
                                                          const uint32_t *__restrict__ seg_axis) {
    __shared__ float2 tile[RS_BLOCK];
    uint32_t first, count;
    range_of_segment(n, level, blockIdx.y, first, count);
    if (blockIdx.x * RS_BLOCK >= count) return;          // (the whole workgroup: the grid is sized for the level's largest range)
    const int ax = (int)seg_axis[blockIdx.y];
    const uint32_t p = blockIdx.x * RS_BLOCK + threadIdx.x;
    const bool live = p < count;
    float key = 0.0f; uint32_t id = 0;
    if (live) { const float4 q = sums_of(inst_box, src[first + p]); key = on_axis(q, ax); id = __float_as_uint(q.w); }
    uint32_t rank = 0;
    for (uint32_t t = 0; t < count; t += RS_BLOCK) {
        const uint32_t m = count - t < RS_BLOCK ? count - t : RS_BLOCK;
        if (threadIdx.x < m) { const float4 q = sums_of(inst_box, src[first + t + threadIdx.x]); tile[threadIdx.x] = make_float2(on_axis(q, ax), q.w); }
        __syncthreads();
        if (live) for (uint32_t j = 0; j < m; j++) { const float2 q = tile[j]; rank += before(q.x, __float_as_uint(q.y), key, id) ? 1u : 0u; }
        __syncthreads();
    }
    if (live) dst[first + rank] = id;          // (rank < count: an element is not before itself)
}

}  // namespace

int tlas_rebuild_supported(const DeviceScene &sc, const char *who) {
    if (sc.tlas_instances <= TLAS_RESORT_MAX) return MRT_OK;
    set_error(std::string(who) + ": more than " + std::to_string(TLAS_RESORT_MAX) + " instances in the TLAS: mrt_scene_commit rebuilds it");
    return MRT_ERR_UNSUPPORTED;
}

int device_rebuild_tlas(DeviceScene &sc, hipStream_t stream) {
    InstanceWorkspace &ws = *sc.inst_ws;
    const uint32_t n = sc.tlas_instances;
    const uint32_t *src = sc.tlas_index.p;
    uint32_t level = 0;
    for (; ((n - 1u) >> level) >= TLAS_RESORT_LDS_LIMIT; level++) {          // the largest range of the level, ceil(n / 2^level), is above the limit
        const uint32_t segs = 1u << level, largest = ((n - 1u) >> level) + 1u;
        uint32_t *dst = ws.ids[level & 1u].p;
        hipLaunchKernelGGL(k_resort_extent, dim3(segs), dim3(RS_BLOCK), 0, stream, src, n, level, (const float4 *)sc.inst_box.p, ws.seg_axis.p);
        hipLaunchKernelGGL(k_resort_rank, dim3((largest + RS_BLOCK - 1) / RS_BLOCK, segs), dim3(RS_BLOCK), 0, stream, src, dst, n, level, (const float4 *)sc.inst_box.p, (const uint32_t *)ws.seg_axis.p);
        src = dst;
    }
    const bool wide = sc.num_wnodes != 0 && ws.wide_of_pos.p != nullptr;
    hipLaunchKernelGGL(k_resort_lds, dim3(1u << level), dim3(RS_BLOCK), 0, stream, src, sc.tlas_index.p, n, level, (const float4 *)sc.inst_box.p,
                       wide ? (const uint32_t *)ws.wide_of_pos.p : (const uint32_t *)nullptr, wide ? sc.wtlas_index.p : (uint32_t *)nullptr);
    MRT_HIP(hipGetLastError());
    return device_refit_instances(sc, stream);          // both forms' boxes over the new sets; records ev_last
}

}  // namespace mrt
