// queues.hip — row queues on device buffers, ordered on a stream of the caller's (mrt_context_compact_rows_device): the rows of up to eight columns whose
// keep byte is set, moved to the front of the columns' destinations IN THEIR ORDER, and their number left in a word on the device.  What a wavefront integrator does between
// two stages: the surviving paths, or the wanted shadow rays, become a dense queue and the next stage takes its length from that word (the *_device_counted entries).
// A translation unit of its own: no traversal, no shading kernel and no builder is compiled here.
//
//   k_queue_count   one workgroup per COMPACT_ROWS rows: eight byte loads per thread (a wave's load covers 64 consecutive bytes), ballot and popcount per wave, the four
//                   waves' sums through LDS, one dword store: the workgroup's total in the caller's workspace
//   k_queue_scan    ONE workgroup of COMPACT_SCAN_THREADS threads: the exclusive prefix of the totals, in place, COMPACT_SCAN_THREADS at a step with a carry, and the
//                   grand total into *d_count_out
//   k_queue_move    the count kernel's loads and ballots again (the second 1-byte read costs nothing beside the rows), the rank of a kept row = the workgroup's prefix +
//                   the (iteration, wave) groups before it (32 counts through LDS) + the kept lanes below it in the wave (mbcnt); then one thread per kept row and column,
//                   16-byte vectors where the row allows it and dwords otherwise.  Source rows of a wave lie in one range of 64 rows, its destination rows are consecutive.
//                   (A form that held the loads of four rows in flight before the first store took 100 VGPRs for 64 and was no faster: the kernel is bound by the lines it
//                   touches — with a keep mask scattered row by row nearly every 128-byte line of every source column — not by a thread's chain of latencies.)
//
// No workgroup waits for another: three launches in stream order, no look-back, no ticket, no flag.  No atomics; 0 bytes of scratch.  Every index is below m = min(n, *count_in)
// on the source side and below the number of kept rows (<= m <= n) on the destination side, whatever the bytes of d_keep and the count word hold.
#include "scene_device.h"
#include <algorithm>

namespace mrt {
namespace {

constexpr uint32_t COMPACT_THREADS = 256, COMPACT_ITERS = 8, COMPACT_WAVES = COMPACT_THREADS / 64;
static_assert(COMPACT_THREADS * COMPACT_ITERS == COMPACT_ROWS, "a workgroup of the count and move kernels owns COMPACT_ROWS rows");

struct ColumnTable {          // the caller's columns, as a kernel argument
    const char *src[COMPACT_MAX_COLUMNS];
    char *dst[COMPACT_MAX_COLUMNS];
    uint32_t row_bytes[COMPACT_MAX_COLUMNS];
    int32_t ncolumns;
};

__device__ __forceinline__ uint32_t rows_in_use(const uint32_t n, const uint32_t *__restrict__ count_in) {
    return count_in ? min(n, *count_in) : n;          // one uniform scalar load; the word is unsigned: a count that is too large (or negative) is clamped
}

// the kept lanes of the wave for row i (a row at or past m is not read and not kept)
__device__ __forceinline__ unsigned long long keep_ballot(const uint8_t *__restrict__ keep, const uint32_t i, const uint32_t m) {
    return __ballot(i < m && keep[i] != 0);
}

__global__ void __launch_bounds__(COMPACT_THREADS) k_queue_count(const uint8_t *__restrict__ keep, const uint32_t n, const uint32_t *__restrict__ count_in, uint32_t *__restrict__ totals) {
    __shared__ uint32_t wave_sum[COMPACT_WAVES];
    const uint32_t m = rows_in_use(n, count_in);
    const uint32_t base = blockIdx.x * COMPACT_ROWS;
    uint32_t c = 0;
    if (base < m) {
#pragma unroll
        for (uint32_t k = 0; k < COMPACT_ITERS; k++) c += (uint32_t)__popcll(keep_ballot(keep, base + k * COMPACT_THREADS + threadIdx.x, m));
    }
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) totals[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

__global__ void __launch_bounds__(COMPACT_SCAN_THREADS) k_queue_scan(uint32_t *__restrict__ totals, const uint32_t groups, uint32_t *__restrict__ count_out) {
    constexpr uint32_t WAVES = COMPACT_SCAN_THREADS / 64;
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < groups; first += COMPACT_SCAN_THREADS) {          // (the bound is uniform: every thread takes every step and both barriers)
        const uint32_t g = first + threadIdx.x;
        const uint32_t v = g < groups ? totals[g] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (lane >= d) incl += up; }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) { const uint32_t s = wave_sum[w]; before += w < wave ? s : 0u; all += s; }
        if (g < groups) totals[g] = carry + before + (incl - v);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = carry;
}

template <class V>
__device__ __forceinline__ void move_row(const char *__restrict__ src, char *__restrict__ dst, const uint32_t vecs) {
    const V *__restrict__ s = reinterpret_cast<const V *>(src);
    V *__restrict__ d = reinterpret_cast<V *>(dst);
    for (uint32_t v = 0; v < vecs; v++) d[v] = s[v];
}

__global__ void __launch_bounds__(COMPACT_THREADS) k_queue_move(const ColumnTable t, const uint8_t *__restrict__ keep, const uint32_t n, const uint32_t *__restrict__ count_in,
                                                               const uint32_t *__restrict__ offsets) {
    __shared__ uint32_t group_sum[COMPACT_ITERS * COMPACT_WAVES];          // kept rows per (iteration, wave), in row order
    const uint32_t m = rows_in_use(n, count_in);
    const uint32_t base = blockIdx.x * COMPACT_ROWS;
    if (base >= m) return;          // (uniform: the whole workgroup leaves)
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t below[COMPACT_ITERS];          // kept lanes of this wave below this one, per iteration
    uint32_t kept = 0;                      // bit k: this thread's row of iteration k is kept
#pragma unroll
    for (uint32_t k = 0; k < COMPACT_ITERS; k++) {
        const unsigned long long b = keep_ballot(keep, base + k * COMPACT_THREADS + threadIdx.x, m);
        below[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        kept |= (uint32_t)((b >> (threadIdx.x & 63u)) & 1ull) << k;
        if ((threadIdx.x & 63u) == 0) group_sum[k * COMPACT_WAVES + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    uint32_t run = offsets[blockIdx.x];          // the kept rows of the workgroups before this one
#pragma unroll
    for (uint32_t k = 0; k < COMPACT_ITERS; k++) {
        uint32_t mine = run;
#pragma unroll
        for (uint32_t w = 0; w < COMPACT_WAVES; w++) { const uint32_t s = group_sum[k * COMPACT_WAVES + w]; mine += w < wave ? s : 0u; run += s; }
        below[k] += mine;          // now the row's place in the queue
    }
    if (kept == 0) return;
    for (int32_t c = 0; c < t.ncolumns; c++) {
        const uint32_t rb = t.row_bytes[c];
        const char *__restrict__ const src = t.src[c];
        char *__restrict__ const dst = t.dst[c];
        const bool vec = (rb & 15u) == 0;
#pragma unroll
        for (uint32_t k = 0; k < COMPACT_ITERS; k++) {
            if (!((kept >> k) & 1u)) continue;
            const size_t from = (size_t)(base + k * COMPACT_THREADS + threadIdx.x) * rb, to = (size_t)below[k] * rb;
            if (vec) move_row<uint4>(src + from, dst + to, rb >> 4);
            else move_row<uint32_t>(src + from, dst + to, rb >> 2);
        }
    }
}

}  // namespace

size_t compact_workspace_bytes(size_t n) {
    const size_t groups = (n + COMPACT_ROWS - 1) / COMPACT_ROWS;
    return std::max<size_t>(16, (groups * sizeof(uint32_t) + 15) & ~size_t(15));
}

// Three launches on `stream`, nothing else.  n < 2^31; the arguments were checked by the caller (api.cpp).
int compact_rows_device(hipStream_t stream, const void *d_keep, size_t n, const void *d_count_in, const MRTRowColumn *columns, int ncolumns, void *d_count_out, void *d_workspace) {
    const uint32_t groups = (uint32_t)((n + COMPACT_ROWS - 1) / COMPACT_ROWS);
    uint32_t *const totals = static_cast<uint32_t *>(d_workspace);
    const uint8_t *const keep = static_cast<const uint8_t *>(d_keep);
    const uint32_t *const count_in = static_cast<const uint32_t *>(d_count_in);
    if (groups) {
        hipLaunchKernelGGL(k_queue_count, dim3(groups), dim3(COMPACT_THREADS), 0, stream, keep, (uint32_t)n, count_in, totals);
        MRT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_queue_scan, dim3(1), dim3(COMPACT_SCAN_THREADS), 0, stream, totals, groups, static_cast<uint32_t *>(d_count_out));          // (no group: writes 0)
    MRT_HIP(hipGetLastError());
    if (groups && ncolumns > 0) {
        ColumnTable t = {};
        for (int c = 0; c < ncolumns; c++) { t.src[c] = static_cast<const char *>(columns[c].src); t.dst[c] = static_cast<char *>(columns[c].dst); t.row_bytes[c] = columns[c].row_bytes; }
        t.ncolumns = ncolumns;
        hipLaunchKernelGGL(k_queue_move, dim3(groups), dim3(COMPACT_THREADS), 0, stream, t, keep, (uint32_t)n, count_in, totals);
        MRT_HIP(hipGetLastError());
    }
    return MRT_OK;
}

}  // namespace mrt
