// variance.hip — the variance-guided a-trous filter on device buffers, on a stream of the caller's (mrt_context_moments_sample_device, mrt_context_denoise_variance_device;
// DESIGN.md §10t): the spatial step of SVGF (Schied, Kaplanyan, Wyman, Patney, Chaitanya, Burgess, Liu, Dachsbacher, Lefohn, Salvi 2017) after the temporal one of
// temporal.hip.  A translation unit of its own: denoise.hip stays as it is and its four one-line helpers are restated here.  The definition is the comment block of
// include/mrt_abi.h; tests/variance_reference.py restates it in numpy, op for op, and this file follows it — float32, no contraction (-ffp-contract=off), IEEE divide,
// correctly rounded sqrt — so the result is that restatement's bit for bit.
//
//   k_moments_sample      {l, l * l, 0, 0} of a sample: one thread per pixel, two 16-byte loads, one 16-byte store
//   k_var_prepass         working entry {image.rgb / A, v}: v = -1 where the pixel is not covered, max(0, m2 - m1 m1) with a history of MRT_VARIANCE_MIN_HISTORY frames,
//                         else the guided 7 x 7 estimate of the moments with SVGF's boost — direct gathers, only on the short-history pixels
//   k_var_atrous_tile     steps 1 and 2: a 16 x 16 tile and its halo of 2 x step of {I, v} and {n, t} staged in LDS as k_dn_atrous_tile does (20 x 20 x 32 B = 12.5 KB,
//                         24 x 24 x 32 B = 18 KB: eight workgroups per CU); the 3 x 3 of v behind the colour term lies inside that halo: nine LDS reads of one word
//   k_var_atrous          larger steps: direct gathers; the nine neighbours of g are one more run of cache lines per row
// The variance rides in the word where denoise.hip keeps coverage: a tap is skipped iff its v < 0 or it lies outside the image (staged as v = -1).  Iterations ping-pong
// between the two workspace images; the last one multiplies the albedo back and writes the output (LAST).  No atomics, no cross-lane traffic, no scratch.
#include "variance.h"

namespace mrt {
namespace {

constexpr int VAR_TILE = 16;
constexpr float VAR_MIN_HISTORY = MRT_VARIANCE_MIN_HISTORY, VAR_EPSILON = MRT_VARIANCE_EPSILON;

struct VarParams { int w, h; float sigma_color, sigma_normal, sigma_depth, fstep; int demodulate; };

// denoise.hip's dn_lum, dn_k, dn_albedo and dn_b
__device__ __forceinline__ float var_lum(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ float var_k(const float x) { return fmaxf(0.0f, 1.0f - x); }
__device__ __forceinline__ float3 var_albedo(const float4 al, const int demodulate) {
    return (demodulate && al.w != 0.0f) ? make_float3(fmaxf(al.x, 1e-3f), fmaxf(al.y, 1e-3f), fmaxf(al.z, 1e-3f)) : make_float3(1.0f, 1.0f, 1.0f);
}
__device__ __forceinline__ constexpr float var_b(const int k) { return (k == 0 || k == 4) ? 1.0f / 16.0f : (k == 1 || k == 3) ? 1.0f / 4.0f : 3.0f / 8.0f; }
__device__ __forceinline__ constexpr float var_g(const int dy, const int dx) { return (dy == 0 ? 1.0f / 2.0f : 1.0f / 4.0f) * (dx == 0 ? 1.0f / 2.0f : 1.0f / 4.0f); }      // 1/4 centre, 1/8 edges, 1/16 corners

// k(xn)^2 and k(xz)^2 of a tap: the filter's normal and depth terms
__device__ __forceinline__ void var_guide(const float4 Np, const float4 Nq, const float sigma_normal, const float zden, float &kn2, float &kz2) {
    const float dot = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    const float xn = (1.0f - fmaxf(0.0f, dot)) / sigma_normal;
    const float xz = fabsf(Np.w - Nq.w) / zden;
    const float kn = var_k(xn), kz = var_k(xz);
    kn2 = kn * kn; kz2 = kz * kz;
}

// one tap that is not the centre: skipped when outside the image (the caller passes v = -1) or not covered
__device__ __forceinline__ void var_tap(const float h, const float4 Np, const float lum_p, const float zden, const float den, const VarParams &P, const float4 Iq, const float4 Nq,
                                        float3 &sum, float &vs, float &wsum) {
    if (Iq.w < 0.0f) return;
    float kn2, kz2;
    var_guide(Np, Nq, P.sigma_normal, zden, kn2, kz2);
    const float xc = fabsf(lum_p - var_lum(Iq)) / den;
    const float kc = var_k(xc);
    const float w = ((h * kn2) * kz2) * (kc * kc);
    sum.x = sum.x + w * Iq.x; sum.y = sum.y + w * Iq.y; sum.z = sum.z + w * Iq.z;
    vs = vs + (w * w) * Iq.w;
    wsum = wsum + w;
}

template <bool LAST>
__device__ __forceinline__ void var_write(const VarParams &P, const float4 *__restrict__ albedo, float4 *__restrict__ out, const size_t p, const float3 I, const float v) {
    if (LAST) { const float3 A = var_albedo(albedo[p], P.demodulate); out[p] = make_float4(I.x * A.x, I.y * A.y, I.z * A.z, 1.0f); }
    else out[p] = make_float4(I.x, I.y, I.z, v);
}

__global__ void __launch_bounds__(256) k_moments_sample(const float4 *__restrict__ sample, const float4 *__restrict__ albedo, float4 *__restrict__ out, uint32_t npix, int demodulate) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 s = sample[p];
    const float3 A = var_albedo(albedo[p], demodulate);
    const float l = var_lum(make_float4(s.x / A.x, s.y / A.y, s.z / A.z, 0.0f));
    out[p] = make_float4(l, l * l, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(256) k_var_prepass(const float4 *__restrict__ image, const float4 *__restrict__ moments, const float4 *__restrict__ nd, const float4 *__restrict__ albedo,
                                                     float4 *__restrict__ sig, VarParams P) {
    const int x = (int)(blockIdx.x * 32 + (threadIdx.x & 31)), y = (int)(blockIdx.y * 8 + (threadIdx.x >> 5));
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.w + x;
    const float4 a = image[p], al = albedo[p];
    const float3 A = var_albedo(al, P.demodulate);
    const float3 I = make_float3(a.x / A.x, a.y / A.y, a.z / A.z);
    if (al.w == 0.0f) { sig[p] = make_float4(I.x, I.y, I.z, -1.0f); return; }
    const float4 m = moments[p];
    float v;
    if (m.w >= VAR_MIN_HISTORY) v = fmaxf(0.0f, m.y - m.x * m.x);          // (a NaN length is a short one)
    else {
        const float4 Np = nd[p];
        const float zden = (P.sigma_depth * Np.w) * 1.0f;
        float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
#pragma unroll 1
        for (int dy = -3; dy <= 3; dy++) {
            const int qy = y + dy;
#pragma unroll
            for (int dx = -3; dx <= 3; dx++) {
                if (dy == 0 && dx == 0) { s1 = s1 + m.x; s2 = s2 + m.y; sw = sw + 1.0f; continue; }
                const int qx = x + dx;
                if (qx < 0 || qx >= P.w || qy < 0 || qy >= P.h) continue;
                const size_t q = (size_t)qy * P.w + qx;
                if (albedo[q].w == 0.0f) continue;
                const float4 mq = moments[q];
                float kn2, kz2;
                var_guide(Np, nd[q], P.sigma_normal, zden, kn2, kz2);
                const float w = kn2 * kz2;
                s1 = s1 + w * mq.x; s2 = s2 + w * mq.y; sw = sw + w;
            }
        }
        const float M1 = s1 / sw, M2 = s2 / sw;
        v = fmaxf(0.0f, M2 - M1 * M1) * (4.0f / fmaxf(m.w, 1.0f));
    }
    sig[p] = make_float4(I.x, I.y, I.z, v);
}

template <bool LAST>
__global__ void __launch_bounds__(256) k_var_atrous(const float4 *__restrict__ sig, const float4 *__restrict__ nd, const float4 *__restrict__ albedo, float4 *__restrict__ out, VarParams P, int step) {
    const int x = (int)(blockIdx.x * 32 + (threadIdx.x & 31)), y = (int)(blockIdx.y * 8 + (threadIdx.x >> 5));
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.w + x;
    const float4 Ip = sig[p];
    if (Ip.w < 0.0f) { var_write<LAST>(P, albedo, out, p, make_float3(Ip.x, Ip.y, Ip.z), Ip.w); return; }
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= P.w || qy < 0 || qy >= P.h) continue;
            const float vq = (dy == 0 && dx == 0) ? Ip.w : sig[(size_t)qy * P.w + qx].w;
            if (vq < 0.0f) continue;
            gs = gs + var_g(dy, dx) * vq; gw = gw + var_g(dy, dx);
        }
    }
    const float den = P.sigma_color * sqrtf(gs / gw) + VAR_EPSILON;
    const float4 Np = nd[p];
    const float lum_p = var_lum(Ip), zden = (P.sigma_depth * Np.w) * P.fstep;
    float3 sum = make_float3(0.0f, 0.0f, 0.0f); float vs = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = var_b(dy + 2) * var_b(dx + 2);
            if (dy == 0 && dx == 0) { sum.x = sum.x + h * Ip.x; sum.y = sum.y + h * Ip.y; sum.z = sum.z + h * Ip.z; vs = vs + (h * h) * Ip.w; wsum = wsum + h; continue; }
            const int qx = x + dx * step, qy = y + dy * step;
            if (qx < 0 || qx >= P.w || qy < 0 || qy >= P.h) continue;
            const size_t q = (size_t)qy * P.w + qx;
            var_tap(h, Np, lum_p, zden, den, P, sig[q], nd[q], sum, vs, wsum);
        }
    }
    var_write<LAST>(P, albedo, out, p, make_float3(sum.x / wsum, sum.y / wsum, sum.z / wsum), vs / (wsum * wsum));
}

template <int STEP, bool LAST>
__global__ void __launch_bounds__(256) k_var_atrous_tile(const float4 *__restrict__ sig, const float4 *__restrict__ nd, const float4 *__restrict__ albedo, float4 *__restrict__ out, VarParams P) {
    constexpr int HALO = 2 * STEP, T = VAR_TILE + 2 * HALO;
    __shared__ float4 sI[T * T], sN[T * T];
    const int bx = (int)blockIdx.x * VAR_TILE, by = (int)blockIdx.y * VAR_TILE;
    for (int i = (int)threadIdx.x; i < T * T; i += 256) {
        const int ly = i / T, lx = i - ly * T, gx = bx - HALO + lx, gy = by - HALO + ly;
        const bool in = gx >= 0 && gx < P.w && gy >= 0 && gy < P.h;
        const size_t q = in ? (size_t)gy * P.w + gx : 0;
        sI[i] = in ? sig[q] : make_float4(0.0f, 0.0f, 0.0f, -1.0f);          // outside the image: v = -1 — the tap is skipped
        sN[i] = in ? nd[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 15), ty = (int)(threadIdx.x >> 4), x = bx + tx, y = by + ty;
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.w + x;
    const int c = (ty + HALO) * T + (tx + HALO);
    const float4 Ip = sI[c];
    if (Ip.w < 0.0f) { var_write<LAST>(P, albedo, out, p, make_float3(Ip.x, Ip.y, Ip.z), Ip.w); return; }
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const float vq = sI[c + dy * T + dx].w;
            if (vq < 0.0f) continue;
            gs = gs + var_g(dy, dx) * vq; gw = gw + var_g(dy, dx);
        }
    }
    const float den = P.sigma_color * sqrtf(gs / gw) + VAR_EPSILON;
    const float4 Np = sN[c];
    const float lum_p = var_lum(Ip), zden = (P.sigma_depth * Np.w) * P.fstep;
    float3 sum = make_float3(0.0f, 0.0f, 0.0f); float vs = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = var_b(dy + 2) * var_b(dx + 2);
            if (dy == 0 && dx == 0) { sum.x = sum.x + h * Ip.x; sum.y = sum.y + h * Ip.y; sum.z = sum.z + h * Ip.z; vs = vs + (h * h) * Ip.w; wsum = wsum + h; continue; }
            const int q = c + dy * STEP * T + dx * STEP;
            var_tap(h, Np, lum_p, zden, den, P, sI[q], sN[q], sum, vs, wsum);
        }
    }
    var_write<LAST>(P, albedo, out, p, make_float3(sum.x / wsum, sum.y / wsum, sum.z / wsum), vs / (wsum * wsum));
}

inline uint32_t cdiv_u(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

// One launch on `stream`, nothing else.  The arguments were checked by the caller (api.cpp).
int moments_sample_device(hipStream_t stream, int width, int height, const void *d_sample, const void *d_albedo, int demodulate, void *d_out) {
    const size_t npix = (size_t)width * (size_t)height;
    hipLaunchKernelGGL(k_moments_sample, dim3(cdiv_u(npix, 256)), dim3(256), 0, stream, static_cast<const float4 *>(d_sample), static_cast<const float4 *>(d_albedo),
                       static_cast<float4 *>(d_out), (uint32_t)npix, demodulate);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

// 1 + iterations launches on `stream`, nothing else
int denoise_variance_device(hipStream_t stream, int width, int height, const void *d_image, const void *d_moments, const void *d_normal_depth, const void *d_albedo,
                            void *d_workspace, void *d_out, const MRTDenoiseParams &p) {
    const float4 *nd = static_cast<const float4 *>(d_normal_depth), *albedo = static_cast<const float4 *>(d_albedo);
    float4 *s0 = static_cast<float4 *>(d_workspace), *s1 = s0 + (size_t)width * (size_t)height, *out = static_cast<float4 *>(d_out);
    const dim3 gt(cdiv_u(width, VAR_TILE), cdiv_u(height, VAR_TILE)), gd(cdiv_u(width, 32), cdiv_u(height, 8));
    VarParams P{width, height, p.sigma_color, p.sigma_normal, p.sigma_depth, 1.0f, p.demodulate};
    hipLaunchKernelGGL(k_var_prepass, gd, dim3(256), 0, stream, static_cast<const float4 *>(d_image), static_cast<const float4 *>(d_moments), nd, albedo, s0, P);
    const float4 *src = s0; float4 *scratch[2] = {s1, s0};
    for (int it = 0; it < p.iterations; it++) {
        const int step = 1 << it;
        const bool last = it + 1 == p.iterations;
        float4 *dst = last ? out : scratch[it & 1];
        P.fstep = (float)step;
        if (step == 1) { if (last) hipLaunchKernelGGL((k_var_atrous_tile<1, true>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); else hipLaunchKernelGGL((k_var_atrous_tile<1, false>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); }
        else if (step == 2) { if (last) hipLaunchKernelGGL((k_var_atrous_tile<2, true>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); else hipLaunchKernelGGL((k_var_atrous_tile<2, false>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); }
        else if (last) hipLaunchKernelGGL(k_var_atrous<true>, gd, dim3(256), 0, stream, src, nd, albedo, dst, P, step);
        else hipLaunchKernelGGL(k_var_atrous<false>, gd, dim3(256), 0, stream, src, nd, albedo, dst, P, step);
        src = dst;
    }
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
