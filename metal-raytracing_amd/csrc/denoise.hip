// denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) of the accumulation buffer, guided by the
// first-hit normal / depth and albedo buffers (guides.h).  No counterpart in the reference: it shows the 1-spp accumulation as it is
// (Renderer.swift:284-351).  The definition is in include/mrt_abi.h (mrt_renderer_denoise) and, as numpy, in tests/denoise_reference.py; the
// kernels follow it operation by operation — float32, no contraction (-ffp-contract=off), IEEE divide — so the result is that restatement's
// bit for bit.
//
//   k_dn_prepass        signal = {accum.rgb / A, coverage}: a tap then costs two 16-byte loads (signal, normal | depth)
//   k_dn_atrous_tile    steps 1 and 2: a 16 x 16 tile and its halo of 2 x step staged in LDS (24 x 24 x 32 B = 18 KB at step 2: eight workgroups,
//                       32 waves, per CU) — every signal / guide entry is fetched once per workgroup instead of up to 25 times
//   k_dn_atrous         larger steps: direct gathers — the taps of neighbouring pixels no longer share cache lines with each other's, and the
//                       three images of a 1080p frame (33 MB each) stay in the 256 MB Infinity Cache between the iterations
// Iterations ping-pong between two scratch images; the last one multiplies the albedo back and writes the output (LAST).
#include "renderer.h"

namespace mrt {
namespace {

constexpr int DN_TILE = 16;

struct DnParams { int w, h; float sc, sigma_normal, sigma_depth, fstep; int demodulate; };

__device__ __forceinline__ float dn_lum(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ float dn_k(const float x) { return fmaxf(0.0f, 1.0f - x); }
__device__ __forceinline__ float3 dn_albedo(const float4 al, const int demodulate) {
    // (a pixel that never hit anything has no albedo: A = 1, so that accum / A * A is accum to the bit — (x / 1e-3f) * 1e-3f is not, for one float in fifty)
    return (demodulate && al.w != 0.0f) ? make_float3(fmaxf(al.x, 1e-3f), fmaxf(al.y, 1e-3f), fmaxf(al.z, 1e-3f)) : make_float3(1.0f, 1.0f, 1.0f);
}

// one tap that is not the centre: skipped when outside the image (the caller passes coverage 0) or never hit
__device__ __forceinline__ void dn_tap(const float h, const float4 Np, const float lum_p, const float zden, const DnParams &P, const float4 Iq, const float4 Nq, float3 &sum, float &wsum) {
    if (Iq.w == 0.0f) return;
    const float dot = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;
    const float xn = (1.0f - fmaxf(0.0f, dot)) / P.sigma_normal;
    const float xz = fabsf(Np.w - Nq.w) / zden;
    const float xc = fabsf(lum_p - dn_lum(Iq)) / P.sc;
    const float kn = dn_k(xn), kz = dn_k(xz), kc = dn_k(xc);
    const float w = ((h * (kn * kn)) * (kz * kz)) * (kc * kc);
    sum.x = sum.x + w * Iq.x; sum.y = sum.y + w * Iq.y; sum.z = sum.z + w * Iq.z;
    wsum = wsum + w;
}

template <bool LAST>
__device__ __forceinline__ void dn_write(const DnParams &P, const float4 *__restrict__ albedo, float4 *__restrict__ out, const size_t p, const float3 I, const float cov) {
    if (LAST) { const float3 A = dn_albedo(albedo[p], P.demodulate); out[p] = make_float4(I.x * A.x, I.y * A.y, I.z * A.z, 1.0f); }
    else out[p] = make_float4(I.x, I.y, I.z, cov);
}

__global__ void __launch_bounds__(256) k_dn_prepass(const float4 *__restrict__ accum, const float4 *__restrict__ albedo, float4 *__restrict__ sig, uint32_t npix, int demodulate) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 a = accum[p], al = albedo[p];
    const float3 A = dn_albedo(al, demodulate);
    sig[p] = make_float4(a.x / A.x, a.y / A.y, a.z / A.z, al.w);
}

__device__ __forceinline__ constexpr float dn_b(const int k) { return (k == 0 || k == 4) ? 1.0f / 16.0f : (k == 1 || k == 3) ? 1.0f / 4.0f : 3.0f / 8.0f; }      // the B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16}

template <bool LAST>
__global__ void __launch_bounds__(256) k_dn_atrous(const float4 *__restrict__ sig, const float4 *__restrict__ nd, const float4 *__restrict__ albedo, float4 *__restrict__ out, DnParams P, int step) {
    const int x = (int)(blockIdx.x * 32 + (threadIdx.x & 31)), y = (int)(blockIdx.y * 8 + (threadIdx.x >> 5));
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.w + x;
    const float4 Ip = sig[p];
    if (Ip.w == 0.0f) { dn_write<LAST>(P, albedo, out, p, make_float3(Ip.x, Ip.y, Ip.z), 0.0f); return; }
    const float4 Np = nd[p];
    const float lum_p = dn_lum(Ip), zden = (P.sigma_depth * Np.w) * P.fstep;
    float3 sum = make_float3(0.0f, 0.0f, 0.0f); float wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = dn_b(dy + 2) * dn_b(dx + 2);
            if (dy == 0 && dx == 0) { sum.x = sum.x + h * Ip.x; sum.y = sum.y + h * Ip.y; sum.z = sum.z + h * Ip.z; wsum = wsum + h; continue; }
            const int qx = x + dx * step, qy = y + dy * step;
            if (qx < 0 || qx >= P.w || qy < 0 || qy >= P.h) continue;
            const size_t q = (size_t)qy * P.w + qx;
            dn_tap(h, Np, lum_p, zden, P, sig[q], nd[q], sum, wsum);
        }
    }
    dn_write<LAST>(P, albedo, out, p, make_float3(sum.x / wsum, sum.y / wsum, sum.z / wsum), Ip.w);
}

template <int STEP, bool LAST>
__global__ void __launch_bounds__(256) k_dn_atrous_tile(const float4 *__restrict__ sig, const float4 *__restrict__ nd, const float4 *__restrict__ albedo, float4 *__restrict__ out, DnParams P) {
    constexpr int HALO = 2 * STEP, T = DN_TILE + 2 * HALO;
    __shared__ float4 sI[T * T], sN[T * T];
    const int bx = (int)blockIdx.x * DN_TILE, by = (int)blockIdx.y * DN_TILE;
    for (int i = (int)threadIdx.x; i < T * T; i += 256) {
        const int ly = i / T, lx = i - ly * T, gx = bx - HALO + lx, gy = by - HALO + ly;
        const bool in = gx >= 0 && gx < P.w && gy >= 0 && gy < P.h;
        const size_t q = in ? (size_t)gy * P.w + gx : 0;
        sI[i] = in ? sig[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);          // outside the image: coverage 0 — the tap is skipped
        sN[i] = in ? nd[q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 15), ty = (int)(threadIdx.x >> 4), x = bx + tx, y = by + ty;
    if (x >= P.w || y >= P.h) return;
    const size_t p = (size_t)y * P.w + x;
    const int c = (ty + HALO) * T + (tx + HALO);
    const float4 Ip = sI[c];
    if (Ip.w == 0.0f) { dn_write<LAST>(P, albedo, out, p, make_float3(Ip.x, Ip.y, Ip.z), 0.0f); return; }
    const float4 Np = sN[c];
    const float lum_p = dn_lum(Ip), zden = (P.sigma_depth * Np.w) * P.fstep;
    float3 sum = make_float3(0.0f, 0.0f, 0.0f); float wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const float h = dn_b(dy + 2) * dn_b(dx + 2);
            if (dy == 0 && dx == 0) { sum.x = sum.x + h * Ip.x; sum.y = sum.y + h * Ip.y; sum.z = sum.z + h * Ip.z; wsum = wsum + h; continue; }
            const int q = c + dy * STEP * T + dx * STEP;
            dn_tap(h, Np, lum_p, zden, P, sI[q], sN[q], sum, wsum);
        }
    }
    dn_write<LAST>(P, albedo, out, p, make_float3(sum.x / wsum, sum.y / wsum, sum.z / wsum), Ip.w);
}

static inline uint32_t cdiv_u(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }

}  // namespace

int denoise_enqueue(hipStream_t stream, int width, int height, const float4 *accum, const float4 *nd, const float4 *albedo, float4 *s0, float4 *s1, float4 *out, const MRTDenoiseParams &p) {
    const size_t npix = (size_t)width * height;
    hipLaunchKernelGGL(k_dn_prepass, dim3(cdiv_u(npix, 256)), dim3(256), 0, stream, accum, albedo, s0, (uint32_t)npix, p.demodulate);
    const float4 *src = s0; float4 *scratch[2] = {s1, s0};
    for (int it = 0; it < p.iterations; it++) {
        const int step = 1 << it;
        const bool last = it + 1 == p.iterations;
        float4 *dst = last ? out : scratch[it & 1];
        DnParams P{width, height, p.sigma_color / (float)step, p.sigma_normal, p.sigma_depth, (float)step, p.demodulate};
        const dim3 gt(cdiv_u(width, DN_TILE), cdiv_u(height, DN_TILE)), gd(cdiv_u(width, 32), cdiv_u(height, 8));
        if (step == 1) { if (last) hipLaunchKernelGGL((k_dn_atrous_tile<1, true>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); else hipLaunchKernelGGL((k_dn_atrous_tile<1, false>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); }
        else if (step == 2) { if (last) hipLaunchKernelGGL((k_dn_atrous_tile<2, true>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); else hipLaunchKernelGGL((k_dn_atrous_tile<2, false>), gt, dim3(256), 0, stream, src, nd, albedo, dst, P); }
        else if (last) hipLaunchKernelGGL(k_dn_atrous<true>, gd, dim3(256), 0, stream, src, nd, albedo, dst, P, step);
        else hipLaunchKernelGGL(k_dn_atrous<false>, gd, dim3(256), 0, stream, src, nd, albedo, dst, P, step);
        src = dst;
    }
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
