// paths.hip — the integrator's path state on device buffers, ordered on a stream of the caller's (mrt_context_reset_paths_device / _advance_paths_device /
// _deposit_light_device / _fold_sample_device): what lies BETWEEN the stage entries of §10c–§10k — throughput x colour, emission along the path, the two
// keep masks of the compactions, radiance += light x throughput where the shadow ray got through, and the reference's running average (Raytracing.metal:339, :371-373,
// :395-401).  A translation unit of its own: no traversal, no shading kernel and no builder is compiled here, and no kernel reads a scene.
//
//   k_paths_reset     one thread per row and per pixel: throughput = 1, pixel = row, radiance = 0 — one 16-byte store, one dword store, one 16-byte store
//   k_paths_advance   <MATERIALS, KEEP_PATH> one thread per row.  Diffuse form: the normal | type and base_color | slot groups of the surface row, the light row and the
//                     throughput row as 16-byte loads, one 16-byte store, one or two byte stores.  Materials form: the two groups of the lobe row in place of the surface,
//                     the pixel word, and where the row is a surface one 16-byte load and store of its pixel's radiance row (emission x the throughput before its update)
//   k_paths_deposit   one thread per row: occluded, pixel, light and throughput; where the shadow ray got through, one 16-byte load and store of the pixel's radiance row
//   k_paths_fold      <CLEAR> one thread per pixel: sample and accumulation as 16-byte loads (frame 0 reads no accumulation), one 16-byte store, a second one of zeros to
//                     the sample row with CLEAR
//
// The count word is read once, as a uniform scalar load behind a uniform null test, as k_scatter reads it; a workgroup past the count leaves at once.  A thread owns a whole
// row, so a wave's 16-byte access covers 1 KiB of consecutive bytes and its byte store 64 consecutive bytes.  No LDS, no atomics, no cross-lane traffic, no scratch.
// The radiance row is addressed by a caller's word: it is read as unsigned and compared with npixels before it is used, so nothing outside the image is touched whatever a
// row holds.  A pixel occurs at most once among the rows of a call (the caller's part, true of every queue of §10k): the deposit is then a plain load, add and store.
// Arithmetic: float32, one rounding per * and per +, IEEE divide (the file is compiled with -ffp-contract=off like the rest).
#include "paths.h"

namespace mrt {
namespace {

constexpr uint32_t PATH_THREADS = 256;

__device__ __forceinline__ uint32_t rows_in_use(const uint32_t n, const uint32_t *__restrict__ count) {
    return count ? min(n, *count) : n;          // one uniform scalar load; the word is unsigned: a count that is too large (or negative) is clamped
}

__global__ void __launch_bounds__(PATH_THREADS) k_paths_reset(const uint32_t n, const uint32_t npix, float4 *__restrict__ thr, uint32_t *__restrict__ pixel, float4 *__restrict__ radiance) {
    const uint32_t i = blockIdx.x * PATH_THREADS + threadIdx.x;
    if (i < n) {
        thr[i] = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        pixel[i] = i;
    }
    if (radiance && i < npix) radiance[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// MATERIALS: the rows are lobe rows (else surface rows); KEEP_PATH: the second mask is wanted (not the last bounce)
template <bool MATERIALS, bool KEEP_PATH>
__global__ void __launch_bounds__(PATH_THREADS) k_paths_advance(const uint32_t cap, const uint32_t *__restrict__ count, const float4 *__restrict__ rows, const float4 *__restrict__ light,
                                                                float4 *__restrict__ thr, const uint32_t *__restrict__ pixel, float4 *__restrict__ radiance, const uint32_t npix,
                                                                uint8_t *__restrict__ keep_shadow, uint8_t *__restrict__ keep_path) {
    const uint32_t m = rows_in_use(cap, count);
    const uint32_t i = blockIdx.x * PATH_THREADS + threadIdx.x;
    if (i >= m) return;
    float4 t = thr[i];
    const bool wanted = light[i].w == 1.0f;
    if (MATERIALS) {
        const float4 w = rows[2 * (size_t)i], e = rows[2 * (size_t)i + 1];          // weight | lobe, emission | -
        const int lobe = __float_as_int(w.w);
        if (lobe != 0) {
            const uint32_t p = pixel[i];
            if (p < npix) {
                float4 r = radiance[p];
                r.x = r.x + t.x * e.x; r.y = r.y + t.y * e.y; r.z = r.z + t.z * e.z;          // the throughput before its update
                radiance[p] = r;
            }
        }
        t.x = t.x * w.x; t.y = t.y * w.y; t.z = t.z * w.z;
        thr[i] = t;
        keep_shadow[i] = wanted ? 1 : 0;
        if (KEEP_PATH) keep_path[i] = (lobe >= 1 && lobe <= 4) ? 1 : 0;
    } else {
        const float4 q1 = rows[4 * (size_t)i + 1], q2 = rows[4 * (size_t)i + 2];    // normal | type, base_color | slot
        const bool on = __float_as_int(q1.w) == 1;
        t.x = t.x * q2.x; t.y = t.y * q2.y; t.z = t.z * q2.z;                         // :339
        thr[i] = t;
        keep_shadow[i] = (on && wanted) ? 1 : 0;
        if (KEEP_PATH) keep_path[i] = on ? 1 : 0;
    }
}

__global__ void __launch_bounds__(PATH_THREADS) k_paths_deposit(const uint32_t cap, const uint32_t *__restrict__ count, const int32_t *__restrict__ occluded, const float4 *__restrict__ light,
                                                                const float4 *__restrict__ thr, const uint32_t *__restrict__ pixel, float4 *__restrict__ radiance, const uint32_t npix) {
    const uint32_t m = rows_in_use(cap, count);
    const uint32_t i = blockIdx.x * PATH_THREADS + threadIdx.x;
    if (i >= m) return;
    const int32_t occ = occluded[i];
    const uint32_t p = pixel[i];
    const float4 l = light[i], t = thr[i];
    if (occ != 0 || p >= npix) return;
    float4 r = radiance[p];
    r.x = r.x + l.x * t.x; r.y = r.y + l.y * t.y; r.z = r.z + l.z * t.z;              // :371-373
    radiance[p] = r;
}

template <bool CLEAR>
__global__ void __launch_bounds__(PATH_THREADS) k_paths_fold(const uint32_t npix, float4 *__restrict__ sample, float4 *__restrict__ accum, const uint32_t frame) {
    const uint32_t i = blockIdx.x * PATH_THREADS + threadIdx.x;
    if (i >= npix) return;
    const float4 s = sample[i];
    float4 c = make_float4(s.x, s.y, s.z, 1.0f);
    if (frame > 0) {                                                                   // (uniform) :395-401, as k_accumulate_planes folds a frame
        const float4 a = accum[i];
        const float fi = (float)frame, den = (float)(frame + 1u);
        c.x = (s.x + a.x * fi) / den; c.y = (s.y + a.y * fi) / den; c.z = (s.z + a.z * fi) / den;
    }
    accum[i] = c;
    if (CLEAR) sample[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

inline dim3 grid_for(size_t n) { return dim3((uint32_t)((n + PATH_THREADS - 1) / PATH_THREADS)); }

}  // namespace

// One launch each on `stream`, nothing else.  n and npixels are below 2^31 and not 0 where a launch depends on them; the arguments were checked by the caller (api.cpp).
int reset_paths_device(hipStream_t stream, size_t n, void *d_throughput, void *d_pixel, void *d_radiance, size_t npixels) {
    const size_t rows = d_radiance ? (n > npixels ? n : npixels) : n;
    hipLaunchKernelGGL(k_paths_reset, grid_for(rows), dim3(PATH_THREADS), 0, stream, (uint32_t)n, (uint32_t)npixels, static_cast<float4 *>(d_throughput), static_cast<uint32_t *>(d_pixel),
                       static_cast<float4 *>(d_radiance));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int advance_paths_device(hipStream_t stream, size_t n, const void *d_count, const void *d_surfaces, const void *d_lobes, const void *d_light, void *d_throughput, const void *d_pixel,
                         void *d_radiance, size_t npixels, void *d_keep_shadow, void *d_keep_path) {
    const bool materials = d_lobes != nullptr;
    auto kernel = materials ? (d_keep_path ? k_paths_advance<true, true> : k_paths_advance<true, false>) : (d_keep_path ? k_paths_advance<false, true> : k_paths_advance<false, false>);
    hipLaunchKernelGGL(kernel, grid_for(n), dim3(PATH_THREADS), 0, stream, (uint32_t)n, static_cast<const uint32_t *>(d_count), static_cast<const float4 *>(materials ? d_lobes : d_surfaces),
                       static_cast<const float4 *>(d_light), static_cast<float4 *>(d_throughput), static_cast<const uint32_t *>(d_pixel), static_cast<float4 *>(d_radiance), (uint32_t)npixels,
                       static_cast<uint8_t *>(d_keep_shadow), static_cast<uint8_t *>(d_keep_path));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int deposit_light_device(hipStream_t stream, size_t n, const void *d_count, const void *d_occluded, const void *d_light, const void *d_throughput, const void *d_pixel, void *d_radiance,
                         size_t npixels) {
    hipLaunchKernelGGL(k_paths_deposit, grid_for(n), dim3(PATH_THREADS), 0, stream, (uint32_t)n, static_cast<const uint32_t *>(d_count), static_cast<const int32_t *>(d_occluded),
                       static_cast<const float4 *>(d_light), static_cast<const float4 *>(d_throughput), static_cast<const uint32_t *>(d_pixel), static_cast<float4 *>(d_radiance), (uint32_t)npixels);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int fold_sample_device(hipStream_t stream, size_t npixels, void *d_sample, void *d_accum, uint32_t frame_index, bool clear_sample) {
    hipLaunchKernelGGL(clear_sample ? k_paths_fold<true> : k_paths_fold<false>, grid_for(npixels), dim3(PATH_THREADS), 0, stream, (uint32_t)npixels, static_cast<float4 *>(d_sample),
                       static_cast<float4 *>(d_accum), frame_index);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
