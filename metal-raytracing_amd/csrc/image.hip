// image.hip — from a composed frame to an image a host can show, on device buffers and on a stream of the caller's (mrt_context_fold_guides_device / _denoise_device /
// _tonemap_device): what a frame composed from the stages of §10c–§10m still took a Renderer for.  A translation unit of its own: no traversal, no shading
// kernel and no builder is compiled here, no kernel reads a scene, and the filter's kernels stay in denoise.hip — denoise_enqueue is called as it stands.
//
//   k_fold_guides     <FIRST> one thread per pixel: the four 16-byte groups of the bounce-0 surface row and (not FIRST) the pixel's two guide averages as 16-byte loads;
//                     three 16-byte stores.  guides.h:41-74 for one frame with the hit taken from the row instead of a walk: a row that is no surface (type != 1)
//                     contributes zeros and the miss ids whatever its other words hold — they are selected away, never computed with.  144 B per pixel, 112 B with FIRST
//                     (frame_index == 0: the averages are replaced and the old ones not read).  The compiler leaves the words nobody uses — position, slot, pad —
//                     out of the row's loads (44 of its 64 bytes, in three loads); the cache lines, and with them the floor, are the same.
//   k_tonemap_image   one thread per pixel of the RGBA8 image in its own order (top row first): thread i writes pixel i and reads pixel x of row h - 1 - y.  A wave's
//                     dword store covers 256 consecutive bytes and its 16-byte load 1 KiB of consecutive bytes per image row it touches (one, or two where the wave
//                     straddles a row end), whatever the width.  renderer.hip's k_tonemap expression by expression.
//
// A thread owns a whole row / pixel.  No LDS, no atomics, no cross-lane traffic, no scratch.  Arithmetic: float32, one rounding per *, + and /, IEEE divide (the file is
// compiled with -ffp-contract=off like the rest).
#include "image.h"
#include "renderer.h"          // denoise_enqueue

namespace mrt {
namespace {

constexpr uint32_t IMAGE_THREADS = 256;

template <bool FIRST>
__global__ void __launch_bounds__(IMAGE_THREADS) k_fold_guides(const uint32_t npix, const float4 *__restrict__ rows, float4 *__restrict__ g_nd, float4 *__restrict__ g_alb,
                                                               int4 *__restrict__ g_ids, const uint32_t frame) {
    const uint32_t i = blockIdx.x * IMAGE_THREADS + threadIdx.x;
    if (i >= npix) return;
    const float4 q0 = rows[4 * (size_t)i], q1 = rows[4 * (size_t)i + 1], q2 = rows[4 * (size_t)i + 2], q3 = rows[4 * (size_t)i + 3];   // position | distance, normal | type, base_color | slot, ids
    const bool on = __float_as_int(q1.w) == 1;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 n_new = on ? make_float4(q1.x, q1.y, q1.z, q0.w) : zero;
    const float4 a_new = on ? make_float4(q2.x, q2.y, q2.z, 1.0f) : zero;
    const int4 ids = on ? make_int4(1, __float_as_int(q3.x), __float_as_int(q3.y), __float_as_int(q3.z)) : make_int4(0, -1, -1, -1);
    float4 nd = n_new, al = a_new;
    if (!FIRST) {                                                                      // Raytracing.metal:395-401, per component, as k_guides folds a frame
        const float4 n_old = g_nd[i], a_old = g_alb[i];
        const float fi = (float)frame, den = (float)(frame + 1u);
        nd = make_float4((n_new.x + n_old.x * fi) / den, (n_new.y + n_old.y * fi) / den, (n_new.z + n_old.z * fi) / den, (n_new.w + n_old.w * fi) / den);
        al = make_float4((a_new.x + a_old.x * fi) / den, (a_new.y + a_old.y * fi) / den, (a_new.z + a_old.z * fi) / den, (a_new.w + a_old.w * fi) / den);
    }
    g_nd[i] = nd; g_alb[i] = al; g_ids[i] = ids;
}

__device__ __forceinline__ unsigned char tonemap_channel(const float c) {            // Shaders.metal:39-52
    float v = c / (1.0f + c);
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return (unsigned char)(v * 255.0f + 0.5f);
}

__global__ void __launch_bounds__(IMAGE_THREADS) k_tonemap_image(const float4 *__restrict__ image, const uint32_t w, const uint32_t h, uchar4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * IMAGE_THREADS + threadIdx.x;
    if (i >= w * h) return;                                                            // (w * h is below 2^30)
    const uint32_t y = i / w, x = i - y * w;
    const float4 a = image[(size_t)(h - 1u - y) * w + x];                              // the vertical flip (the blit's uv, :35)
    out[i] = make_uchar4(tonemap_channel(a.x), tonemap_channel(a.y), tonemap_channel(a.z), 255);
}

inline dim3 grid_for(size_t n) { return dim3((uint32_t)((n + IMAGE_THREADS - 1) / IMAGE_THREADS)); }

}  // namespace

// One launch each on `stream` (the filter: the launches of denoise_enqueue), nothing else.  The arguments were checked by the caller (api.cpp).
int fold_guides_device(hipStream_t stream, size_t npixels, const void *d_surfaces, void *d_normal_depth, void *d_albedo, void *d_ids, uint32_t frame_index) {
    hipLaunchKernelGGL(frame_index == 0 ? k_fold_guides<true> : k_fold_guides<false>, grid_for(npixels), dim3(IMAGE_THREADS), 0, stream, (uint32_t)npixels,
                       static_cast<const float4 *>(d_surfaces), static_cast<float4 *>(d_normal_depth), static_cast<float4 *>(d_albedo), static_cast<int4 *>(d_ids), frame_index);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int denoise_image_device(hipStream_t stream, int width, int height, const void *d_image, const void *d_normal_depth, const void *d_albedo, void *d_workspace, void *d_out,
                         const MRTDenoiseParams &p) {
    float4 *s0 = static_cast<float4 *>(d_workspace);
    return denoise_enqueue(stream, width, height, static_cast<const float4 *>(d_image), static_cast<const float4 *>(d_normal_depth), static_cast<const float4 *>(d_albedo), s0,
                           s0 + (size_t)width * (size_t)height, static_cast<float4 *>(d_out), p);
}

int tonemap_image_device(hipStream_t stream, int width, int height, const void *d_image, void *d_rgba8) {
    hipLaunchKernelGGL(k_tonemap_image, grid_for((size_t)width * (size_t)height), dim3(IMAGE_THREADS), 0, stream, static_cast<const float4 *>(d_image), (uint32_t)width, (uint32_t)height,
                       static_cast<uchar4 *>(d_rgba8));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
