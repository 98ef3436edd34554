// renderer.hip — the per-frame hot path as CDNA4 kernels + the host frame driver.
//
// Replaces `raytracingKernel` (Raytracing.metal:156-405) and the frame driver around it
// (Renderer.draw / update / updateUniforms / createTextures, Renderer.swift:216-357).
// The reference is one megakernel over Apple's opaque intersector; here the frame is a wavefront
// pipeline over ray / hit records in HBM:
//
//   primary rays  Halton-jittered, traced to their closest hit                                (Raytracing.metal:171-247)
//   k_shade       normal interpolation, light pick + evaluation, throughput, NEE shadow-ray emit,
//                 cosine-hemisphere bounce; wave-ballot compaction of both output queues      (:249-391)
//   traversal     bounce rays (closest hit) and shadow rays (any hit) of that shade, ONE launch (:244, :367)
//   accumulate    running average with the previous target                                    (:394-403)
//
// The DEFAULT pass carries up to eight frames and runs
//   k_shade<.., TRACE0>          primary rays generated, traced (last frame's hit as a hint) and shaded in one launch
//   k_trace_mixed_wide_persist   per bounce: its bounce rays (closest hit) and shadow rays (any hit) in ONE launch of persistent waves on the
//                                8-wide layout (traverse_wide.h); a shadow ray that gets through sets one byte
//   k_shade                      bounces 1, 2: the light's contribution goes to a per-bounce plane, the throughput is rebuilt from resource slots
//   k_accumulate_planes          contributions whose byte is set, summed in bounce order; running average (the last passes of a draw: one launch)
// on up to six streams; instanced scenes walk both levels with the same kernels (<TWO_LEVEL>).  Scenes without the 8-wide layout (scene option wide = 0, a tree
// deeper than WIDE_STACK_MAX) and the materials extension / more than three bounces take the general form of the same pipeline (k_trace_primary, k_trace_mixed, k_accumulate).
//
// Record layout (all 16-byte lanes, one dwordx4 per lane per access, fully coalesced):
//   rayA = {origin.xyz, tmax}   rayB = {direction.xyz, pixel}   thr = {throughput.rgb, -}   (path rays)
//   hit  = {t, U/|det|, V/|det|, gid}                                                        (16 B; traverse.h hit_record)
//   shadow rays reuse rayA/rayB with tmax = lightDistance - 1e-3; con = {Lc*throughput, -}
// The wide traversal launches read a bounce's combined queue [bounce rays | shadow rays] through MixedQueue (traverse_wide.h).  The scene queries of the
// C ABI (mrt_scene_intersect_*, mrt_debug_*) are query.hip; the device-function probes at the end of this file stay here: they use k_seed.
#include <hip/hip_ext.h>
#include "renderer.h"
#include "device_math.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "traverse_instanced.h"
#include "shade.h"
#include "two_level_passes.h"
#include <cstdlib>
#include <cstring>
#include <algorithm>

namespace mrt {
namespace {

__global__ void k_halton_table(float *__restrict__ tab, uint32_t w0, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) tab[MRT_HALTON_INTERLEAVED ? (size_t)j * HALTON_TAB_DIMS + blockIdx.y : (size_t)blockIdx.y * n + j] = halton_dev((int)(w0 + j), (int)blockIdx.y + 1);
}

// seeds[s * n + i] = hash(seed, i) + s: sub-frame s of a batch reads its Halton offset with the sub-frame index already added
__global__ void k_seed(uint32_t *__restrict__ seeds, uint32_t n, uint32_t seed) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) seeds[(size_t)blockIdx.y * n + i] = seed_hash_dev(seed, i) + blockIdx.y;
}

// the renderer's seed table: by sample index (sub-frame * capacity + slot of this shard), seeds[...] = hash(seed, pixel of the slot) + sub-frame
__global__ void k_seed_slots(uint32_t *__restrict__ seeds, FrameParams fp, uint32_t seed) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= fp.capacity) return;
    int x, y;
    seeds[(size_t)blockIdx.y * fp.capacity + slot] = slot_to_pixel(fp, slot, x, y) ? seed_hash_dev(seed, (uint32_t)y * (uint32_t)fp.width + (uint32_t)x) + blockIdx.y : 0u;
}

// ------------------------------------------------------------------ traversal launches of the pipeline
// Fewer, fatter traversal launches: every launch ends in a latency-bound tail (a handful of waves walking
// the longest rays), so the frame runs  primary -> shade -> [shadow(b) + extend(b+1)] -> shade -> ... .
//   k_trace_primary : primary-ray generation (Raytracing.metal:171-221) fused with the first closest-hit query
//   k_trace_mixed   : one launch over two queues — the next-bounce rays (closest hit -> hit records) and the
//                     shadow rays of the same shade pass (any hit -> sample accumulation).  The two kinds share
//                     the loop; a shadow lane simply stops at its first hit.
// WIDE (flattened scenes with the 8-wide layout): one ray per lane on that layout (traverse_wide_lane), the wave's stack in dynamic LDS; the hint then names a packet of wpackets
template <bool TWO_LEVEL, bool WIDE = false>
__global__ void __launch_bounds__(64) k_trace_primary(SceneView s, FrameParams fp, const uint32_t *__restrict__ seeds, float4 *__restrict__ hits, float4 *__restrict__ dirs, uint32_t *__restrict__ hint) {
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x, sub = blockIdx.y;      // grid = (local tiles, sub-frames of the batch)
    float4 *__restrict__ hits_s = hits + (size_t)sub * fp.capacity;
    int x, y;
    if (!slot_to_pixel(fp, slot, x, y)) {
        if ((int)(slot >> 6) < fp.tiles_local) hits_s[slot] = miss_record();
        return;
    }
    f3 org, dir;
    primary_ray(fp, seeds, sub * fp.capacity + slot, x, y, org, dir);
    // the direction goes to HBM (16 B per pixel: the memory system has headroom, the vector ALUs do not — k_shade reads it back
    // instead of repeating two Halton values, two divisions and a normalisation per pixel)
    qstore(&dirs[(size_t)sub * fp.capacity + slot], make_float4(dir.x, dir.y, dir.z, __uint_as_float(sub * fp.capacity + slot)));
    TravHit h;
    bool hit;
    if (WIDE && !TWO_LEVEL) {
        extern __shared__ uint32_t stk_dyn[];
        if (hint != nullptr) {
            const uint32_t pixel = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
            const uint32_t guess = hint[pixel];
            float t0 = __builtin_inff(); uint32_t seed = 0xFFFFFFFFu;
            if (guess < s.num_wpackets) {
                const float4 *__restrict__ pk = s.wpackets + WPK * (size_t)guess;
                float t, U, V, ad;
                if (tri_test(pk[0], pk[1], pk[2], org, dir, 0.0f, __builtin_inff(), t, U, V, ad)) { t0 = t; seed = guess; }
            }
            hit = traverse_wide_lane<true>(s, org, dir, t0, seed, h, stk_dyn);
            if (h.pk != guess) hint[pixel] = h.pk;
        }
        else hit = traverse_wide_lane<false>(s, org, dir, __builtin_inff(), 0xFFFFFFFFu, h, stk_dyn);
    }
    else if (!TWO_LEVEL && hint != nullptr) {
        // the triangle this pixel hit in an earlier frame is tested first: the jittered ray most often hits it again, and the walk then starts with
        // the right distance bound instead of discovering it.  Any packet is a legal guess (a wrong one is one wasted test); the result is unchanged.
        const uint32_t pixel = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
        const uint32_t guess = hint[pixel];
        h.t = __builtin_inff(); h.U = 0.0f; h.V = 0.0f; h.ad = 1.0f; h.gid = 0xFFFFFFFFu; h.pk = 0xFFFFFFFFu;
        if (guess < s.num_tris) {
            const float4 *__restrict__ pk = s.packets + 3 * (size_t)guess;
            const float4 q0 = pk[0];
            float t, U, V, ad;
            if (tri_test(q0, pk[1], pk[2], org, dir, 0.0f, __builtin_inff(), t, U, V, ad)) { h.t = t; h.U = U; h.V = V; h.ad = ad; h.gid = __float_as_uint(q0.w); h.pk = guess; }
        }
        hit = traverse<false, false, false, true>(s, org, dir, 0.0f, h.t, h);
        if (h.pk != guess) hint[pixel] = h.pk;
    }
    else hit = TWO_LEVEL ? traverse_instanced<false>(s, org, dir, 0.0f, __builtin_inff(), h) : traverse<false>(s, org, dir, 0.0f, __builtin_inff(), h);
    qstore(&hits_s[slot], hit_record(hit, h));
}

template <bool TWO_LEVEL>
__global__ void __launch_bounds__(64) k_trace_mixed(SceneView s, const float4 *__restrict__ rayA, const float4 *__restrict__ rayB, float4 *__restrict__ hits,
                                                    const float4 *__restrict__ srayA, const float4 *__restrict__ srayB, const float4 *__restrict__ scon,
                                                    const unsigned long long *__restrict__ counts, float4 *__restrict__ sample) {
    const unsigned long long c = *counts;
    const uint32_t n_next = (uint32_t)c, n_shadow = (uint32_t)(c >> 32);
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_next + n_shadow) return;
    const bool shadow = i >= n_next;
    const uint32_t j = shadow ? i - n_next : i;
    float4 A = shadow ? srayA[j] : rayA[j]; const float4 B = shadow ? srayB[j] : rayB[j];
    if (!shadow) A.w = __builtin_inff();          // a bounce ray's tmax word may carry the throughput chain
    TravHit h;
    bool hit = TWO_LEVEL ? traverse_instanced<false, true>(s, mk3(A), mk3(B), 0.0f, A.w, h, shadow) : traverse<false, false, true>(s, mk3(A), mk3(B), 0.0f, A.w, h, nullptr, shadow);
    if (shadow) {
        if (!hit) {
            uint32_t pix = __float_as_uint(B.w);
            float4 cc = scon[j], a = sample[pix];
            sample[pix] = make_float4(a.x + cc.x, a.y + cc.y, a.z + cc.z, 0.0f);   // one shadow ray per pixel per bounce: no atomics
        }
    } else {
        hits[j] = hit_record(hit, h);
    }
}

// ------------------------------------------------------------------ 8-wide layout (LDS stack, traverse_wide.h)
// One wave walks `rays_per_wave` consecutive rays of the combined queue
// [next-bounce rays | shadow rays] with lane refill (traverse_wide_stream).  Longer ranges amortise the drain at the end
// of a wave's range, shorter ones keep the launch's tail short and the grid large; the host picks the range from the
// size of the launch (stream_rays_per_wave): one frame per pass (4 M slots): 384 measured best (256: -2 %, 512: -1 %,
// 1024: -7 %); four frames per pass (17 M slots): 1024 (384: -4.5 %, 768: -1.5 %, 2048: equal on the full frame, -3 % on
// primary + shadow).
#ifdef MRT_WIDE_STREAM_RAYS
constexpr uint32_t WIDE_STREAM_RAYS_FIXED = MRT_WIDE_STREAM_RAYS;     // tuning builds
#else
constexpr uint32_t WIDE_STREAM_RAYS_FIXED = 0;
#endif
static inline uint32_t stream_rays_per_wave(size_t slots) {
    if (WIDE_STREAM_RAYS_FIXED) return WIDE_STREAM_RAYS_FIXED;
    const size_t batches = slots / 64 / 10240;                             // 64-ray batches per wave if the launch had ~10 K waves
    return 64u * (uint32_t)std::min<size_t>(16, std::max<size_t>(6, batches));
}
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(64, TWO_LEVEL ? MRT_TWO_LEVEL_WAVES : MRT_WIDE_STREAM_WAVES) k_trace_mixed_wide_stream(SceneView s, const float4 *__restrict__ rayA, const float4 *__restrict__ rayB, float4 *__restrict__ hits,
                                                                const float4 *__restrict__ srayA, const float4 *__restrict__ srayB, const float4 *__restrict__ scon,
                                                                const unsigned long long *__restrict__ counts, float4 *__restrict__ sample, uint32_t rays_per_wave, uint8_t *__restrict__ lit, uint32_t even_waves) {
    extern __shared__ uint32_t stk_dyn[];
    const unsigned long long c = *counts;
    const uint32_t n_next = (uint32_t)c, n_shadow = (uint32_t)(c >> 32), n = n_next + n_shadow;
    // even_waves (renderer option stream_even): the launch has that many waves and the rays the queue really holds are split evenly among them (whole 64-ray
    // batches) instead of rays_per_wave each to the first n / rays_per_wave waves of a grid sized for the queue's capacity
    if (even_waves) rays_per_wave = max(64u, ((n + even_waves - 1u) / even_waves + 63u) & ~63u);
    const uint32_t begin = blockIdx.x * rays_per_wave;
    if (begin >= n) return;
    const MixedQueue<false, false> q{rayA, rayB, srayA, srayB, scon, hits, sample, lit, n_next};
    traverse_wide_stream<TWO_LEVEL>(s, OneRange{begin, min(n, begin + rays_per_wave)}, stk_dyn,
        [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) { q.fetch(i, A, B, tag, is_any); },
        [&](uint32_t j, bool is_any, bool hit, const TravHit &h) { q.emit(j, is_any, hit, h); });
}

#ifdef MRT_WAVE_TIMES      // diagnostics build (tools/archive/wave_times.py): when does every wave of the first traversal launch of a pass start and end?
__device__ unsigned long long g_wave_times[2 * 8192];
__device__ uint32_t g_wave_iters[4 * 8192];      // per wave of that launch: iterations | drain iterations + longest iteration << 12 | live lanes summed over the drain iterations | drain start tick
__device__ unsigned long long g_drain_probe[2][9];      // StreamStats::dr_*, summed over the waves of that launch: [at most 16 | at most 4 live lanes][6 stack-depth bins, hit children pending, triangles pending, samples]
// Leaves a wave's record behind when the kernel returns, on whichever path (tag: only the launch tagged 0 reports).  DRAIN: the drain probe's sums too.
template <bool DRAIN> struct WaveTimes {
    unsigned long long t0; uint32_t tag; StreamStats &st;
    __device__ ~WaveTimes() {
        if ((threadIdx.x & 63) == 0 && tag == 0 && blockIdx.x < 8192) {
            g_wave_times[2 * blockIdx.x] = t0; g_wave_times[2 * blockIdx.x + 1] = wall_clock64();
            g_wave_iters[4 * blockIdx.x] = st.iters | (st.drain_le8 << 16); g_wave_iters[4 * blockIdx.x + 1] = st.drain_iters | (st.maxdt << 12); g_wave_iters[4 * blockIdx.x + 2] = st.drain_live; g_wave_iters[4 * blockIdx.x + 3] = (uint32_t)st.drain_t0;
        }
        if (DRAIN && (threadIdx.x & 63) == 0 && tag == 0) for (int c_ = 0; c_ < 2; c_++) {
            for (int d_ = 0; d_ < 6; d_++) atomicAdd(&g_drain_probe[c_][d_], (unsigned long long)st.dr_hist[c_][d_]);
            atomicAdd(&g_drain_probe[c_][6], (unsigned long long)st.dr_kids[c_]); atomicAdd(&g_drain_probe[c_][7], (unsigned long long)st.dr_tris[c_]); atomicAdd(&g_drain_probe[c_][8], (unsigned long long)st.dr_n[c_]);
        }
    }
};
#endif
// Persistent variant: the grid is the number of wave slots of the chip (or fewer for a small queue) and every wave pulls
// `chunk` consecutive rays of the combined queue at a time from `work` (zeroed by k_accumulate at the end of the previous pass).
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(64, TWO_LEVEL ? MRT_TWO_LEVEL_WAVES : MRT_WIDE_STREAM_WAVES) k_trace_mixed_wide_persist(SceneView s, const float4 *__restrict__ rayA, const float4 *__restrict__ rayB, float4 *__restrict__ hits,
                                                                const float4 *__restrict__ srayA, const float4 *__restrict__ srayB, const float4 *__restrict__ scon,
                                                                const unsigned long long *__restrict__ counts, float4 *__restrict__ sample, uint32_t *__restrict__ work, uint32_t chunk, uint8_t *__restrict__ lit, uint32_t subframes /* > 0: XCD regions (XcdRegions), the pass's sub-frames */) {
    extern __shared__ uint32_t stk_dyn[];
    const unsigned long long c = *counts;
    const uint32_t n_next = (uint32_t)c, n_shadow = (uint32_t)(c >> 32), n = n_next + n_shadow;
#ifdef MRT_WAVE_TIMES
    const uint32_t wt_tag = chunk >> 24; chunk &= 0xFFFFFFu;
    const unsigned long long wt0 = wall_clock64();
    StreamStats wst{0, 0, 0, 0, 0, 0};
    const WaveTimes<false> wt{wt0, wt_tag, wst};
#endif
    if (blockIdx.x * chunk >= n) return;            // more waves than chunks (small queue): the surplus leaves at once
    const MixedQueue<false, false> q{rayA, rayB, srayA, srayB, scon, hits, sample, lit, n_next};
    const auto fetch = [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) { q.fetch(i, A, B, tag, is_any); };
    const auto emit = [&](uint32_t j, bool is_any, bool hit, const TravHit &h) { q.emit(j, is_any, hit, h); };
#ifdef MRT_WAVE_TIMES
    StreamStats *const wss = wt_tag == 0 ? &wst : nullptr;
#else
    StreamStats *const wss = nullptr;
#endif
    // two-level scenes keep the one counter (the first of the eight): the per-XCD form measured no gain there and costs the in-loop walk five spilled registers
    if constexpr (TWO_LEVEL) traverse_wide_stream<true>(s, SharedCounter{work, n, chunk}, stk_dyn, fetch, emit, wss);
    else traverse_wide_stream<false>(s, XcdRegions{work, n_next, n, chunk, subframes, blockIdx.x & 7u}, stk_dyn, fetch, emit, wss);
}

// The pulling launch of flattened scenes with the hit words in LDS (traverse_wide.h StreamExt; renderer option hit_lds, default): every wave has its own hit
// words (1 KB + the root's hit bits of the prefetched batch) in front of its stack.  Shadow planes only (`lit`): the default path of the pipeline.
// SEG: a segmented pass (SegRegions) — `counts` is segment 0's tail word, `subframes` the segments' capacity, and a ray's index is physical with SEG_SHADOW_BIT for a shadow ray.
template <bool SEG>
__global__ void __launch_bounds__(64, MRT_WIDE_STREAM_WAVES) k_trace_mixed_wide_persist_x(SceneView s, const float4 *__restrict__ rayA, const float4 *__restrict__ rayB, float4 *__restrict__ hits,
                                                                const float4 *__restrict__ srayA, const float4 *__restrict__ srayB, const unsigned long long *__restrict__ counts,
                                                                uint32_t *__restrict__ work, uint32_t chunk, uint8_t *__restrict__ lit, uint32_t subframes) {
    extern __shared__ uint32_t lds_dyn[];
    unsigned long long c = *counts;
    if (SEG) for (uint32_t x = 1; x < QUEUE_SEGMENTS; x++) c += counts[(size_t)x * SEG_TAIL_STRIDE];          // (neither half carries: a pass queues fewer than 2^31 rays of a kind)
    const uint32_t n_next = (uint32_t)c, n_shadow = (uint32_t)(c >> 32), n = n_next + n_shadow;
    if ((unsigned long long)blockIdx.x * chunk >= (unsigned long long)n + (SEG ? 2ull * QUEUE_SEGMENTS * chunk : 0ull)) return;            // more waves than chunks (small queue; SEG: every segment rounds its two parts up): the surplus leaves at once
    const MixedQueue<SEG, true> q{rayA, rayB, srayA, srayB, nullptr, hits, nullptr, lit, n_next};
    const auto fetch = [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) { q.fetch(i, A, B, tag, is_any); };
    const auto emit = [&](uint32_t j, bool is_any, bool hit, const TravHit &h) { q.emit(j, is_any, hit, h); };
    StreamExt<true> ext{reinterpret_cast<float *>(lds_dyn), lds_dyn + 256u};
    if constexpr (SEG) traverse_wide_stream<false, false, false, NoPairs, StreamExt<true>>(s, SegRegions{work, counts, subframes, chunk, blockIdx.x & 7u}, lds_dyn + HIT_LDS_WORDS, fetch, emit, nullptr, NoPairs{}, ext);
    else traverse_wide_stream<false, false, false, NoPairs, StreamExt<true>>(s, XcdRegions{work, n_next, n, chunk, subframes, blockIdx.x & 7u}, lds_dyn + HIT_LDS_WORDS, fetch, emit, nullptr, NoPairs{}, ext);
}

// The static split of small launches (k_trace_mixed_wide_stream) with the hit words in LDS (renderer option hit_lds): flattened scenes, shadow planes.
__global__ void __launch_bounds__(64, MRT_WIDE_STREAM_WAVES) k_trace_mixed_wide_stream_x(SceneView s, const float4 *__restrict__ rayA, const float4 *__restrict__ rayB, float4 *__restrict__ hits,
                                                                const float4 *__restrict__ srayA, const float4 *__restrict__ srayB, const unsigned long long *__restrict__ counts,
                                                                uint32_t rays_per_wave, uint8_t *__restrict__ lit, uint32_t even_waves) {
    extern __shared__ uint32_t lds_dyn[];
    const unsigned long long c = *counts;
    const uint32_t n_next = (uint32_t)c, n_shadow = (uint32_t)(c >> 32), n = n_next + n_shadow;
#ifdef MRT_WAVE_TIMES
    const uint32_t wt_tag = rays_per_wave >> 24; rays_per_wave &= 0xFFFFFFu;
    StreamStats wst{0, 0, 0, 0, 0, 0};
    const WaveTimes<true> wt{(unsigned long long)wall_clock64(), wt_tag, wst};
    StreamStats *const wss = wt_tag == 0 ? &wst : nullptr;
#else
    StreamStats *const wss = nullptr;
#endif
    const bool strided = (even_waves >> 31) != 0u; even_waves &= 0x7FFFFFFFu;
    if (even_waves) rays_per_wave = max(64u, ((n + even_waves - 1u) / even_waves + 63u) & ~63u);
    const uint32_t begin = blockIdx.x * rays_per_wave;
    if (begin >= n) return;
    StreamExt<true> ext{reinterpret_cast<float *>(lds_dyn), lds_dyn + 256u};
    // stream_stride: the (n + rays_per_wave - 1) / rays_per_wave waves that have work take the queue's 64-ray batches round-robin instead of one contiguous range each
    const BatchStride src = strided ? BatchStride{blockIdx.x * 64u, 64u * ((n + rays_per_wave - 1u) / rays_per_wave), n} : BatchStride{begin, 64u, min(n, begin + rays_per_wave)};
    const MixedQueue<false, true> q{rayA, rayB, srayA, srayB, nullptr, hits, nullptr, lit, n_next};
    traverse_wide_stream<false, false, false, NoPairs, StreamExt<true>>(s, src, lds_dyn + HIT_LDS_WORDS,
        [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) { q.fetch(i, A, B, tag, is_any); },
        [&](uint32_t j, bool is_any, bool hit, const TravHit &h) { q.emit(j, is_any, hit, h); }, wss, NoPairs{}, ext);
}

#include "megakernel.h"            // k_megakernel: one launch per frame
#include "guides.h"                // k_guides: first-hit guide buffers (renderer option guides)

// Primary rays on the wide layout with lane refill (experiment: the rope kernel is VALU-bound on primary rays; measured
// equal on the full frame, 7 % slower on the primary + shadow workload).
template <bool TWO_LEVEL, bool SEED>
__global__ void __launch_bounds__(64, 5) k_trace_primary_wide_stream(SceneView s, FrameParams fp, const uint32_t *__restrict__ seeds, float4 *__restrict__ hits, float4 *__restrict__ dirs, uint32_t capacity, uint32_t rays_per_wave,
                                                                     uint32_t *__restrict__ hint /* SEED: per pixel, the (packet | instance << 24) its primary ray hit last */) {
    extern __shared__ uint32_t stk_dyn[];
    const uint32_t begin = blockIdx.x * rays_per_wave, sub = blockIdx.y;
    if (begin >= capacity) return;
    hits += (size_t)sub * capacity; dirs += (size_t)sub * capacity;
    auto make_ray = [&](uint32_t slot, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any, f3 &org, f3 &dir, int &x, int &y) -> bool {
        is_any = 0u; tag = slot;
        if (slot_to_pixel(fp, slot, x, y)) {
            primary_ray(fp, seeds, sub * fp.capacity + slot, x, y, org, dir);
            A = make_float4(org.x, org.y, org.z, __builtin_inff()); B = make_float4(dir.x, dir.y, dir.z, 0.0f);
            dirs[slot] = make_float4(dir.x, dir.y, dir.z, __uint_as_float(sub * fp.capacity + slot));   // read back by k_shade
            return true;
        }
        A = make_float4(0.0f, 0.0f, 0.0f, -1.0f); B = make_float4(0.0f, 0.0f, 1.0f, 0.0f);                // partial-tile slot: tmax < 0 -> miss
        return false;
    };
    if constexpr (SEED) {
        // the triangle this pixel hit in an earlier frame is tested first (in its instance's object space: the arithmetic of the walk itself): the jittered ray most
        // often hits it again and the walk starts with the right distance bound.  A guess is legal when its packet belongs to its instance's BLAS (a stale one —
        // another scene, moved instances — is then one wasted test or none); the result is the minimum over (t, id) either way.
        traverse_wide_stream<TWO_LEVEL, true>(s, OneRange{begin, min(capacity, begin + rays_per_wave)}, stk_dyn,
            [&](uint32_t slot, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any, uint32_t &seed) {
                f3 org, dir; int x, y;
                seed = 0xFFFFFFFFu;
                if (!make_ray(slot, A, B, tag, is_any, org, dir, x, y)) return;
                const uint32_t guess = hint[(uint32_t)y * (uint32_t)fp.width + (uint32_t)x];
                const uint32_t pk = TWO_LEVEL ? (guess & 0xFFFFFFu) : guess, in = TWO_LEVEL ? guess >> 24 : 0u;
                if (guess == 0xFFFFFFFFu) return;
                float t, U, V, ad;
                if (TWO_LEVEL) {
                    if (in >= s.num_inst) return;
                    const InstanceDev &I = s.inst[in];
                    if (pk - I.packet_base >= I.ntri) return;
                    const float4 *__restrict__ q = s.wpackets + WPK * (size_t)pk;
                    if (tri_test(q[0], q[1], q[2], to_object_point(I, org), to_object_dir(I, dir), 0.0f, __builtin_inff(), t, U, V, ad)) { A.w = t; seed = guess; }
                } else {
                    if (pk >= s.num_tris) return;
                    const float4 *__restrict__ q = s.wpackets + WPK * (size_t)pk;
                    if (tri_test(q[0], q[1], q[2], org, dir, 0.0f, __builtin_inff(), t, U, V, ad)) { A.w = t; seed = guess; }
                }
            },
            [&](uint32_t slot, bool, bool hit, const TravHit &h) {
                hits[slot] = hit_record(hit, h);
                int x, y;
                if (hit && slot_to_pixel(fp, slot, x, y)) hint[(uint32_t)y * (uint32_t)fp.width + (uint32_t)x] = h.pk;
            });
    } else {
        traverse_wide_stream<TWO_LEVEL>(s, OneRange{begin, min(capacity, begin + rays_per_wave)}, stk_dyn,
            [&](uint32_t slot, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) { f3 org, dir; int x, y; (void)make_ray(slot, A, B, tag, is_any, org, dir, x, y); },
            [&](uint32_t slot, bool, bool hit, const TravHit &h) {
                hits[slot] = hit_record(hit, h);
            });
    }
}

// ------------------------------------------------------------------ accumulate (Raytracing.metal:394-403)
// Also the frame's bookkeeping (block 0, thread 0): per-bounce queue counters {next rays, shadow rays} are
// folded into the running totals and zeroed for the next frame.
constexpr size_t WORK_COUNTERS = 128, WORK_COUNTERS_PER_BOUNCE = 8 * XCD_COUNTER_STRIDE / 2;      // in 64-bit words of FrameLane::bounce_counts
constexpr size_t SEG_TAILS = WORK_COUNTERS + 32 * WORK_COUNTERS_PER_BOUNCE, SEG_TAILS_PER_BOUNCE = QUEUE_SEGMENTS * SEG_TAIL_STRIDE;      // a segmented pass's tail words {next, shadow}: per bounce, one per segment on its own 128-byte line
// The pass's bookkeeping of bounce b (one thread): {next rays, shadow rays} queued — on the one word or on the segments' — and every counter of the bounce back to zero.
MRT_DEV unsigned long long fold_bounce_counters(unsigned long long *__restrict__ bounce_counts, int b) {
    unsigned long long c = bounce_counts[b];
    unsigned long long *const tails = bounce_counts + SEG_TAILS + (size_t)b * SEG_TAILS_PER_BOUNCE;
    for (uint32_t x = 0; x < QUEUE_SEGMENTS; x++) { c += tails[x * SEG_TAIL_STRIDE]; tails[x * SEG_TAIL_STRIDE] = 0; }      // (a pass uses the one word or the eight; neither half carries)
    bounce_counts[b] = 0;
    bounce_counts[32 + b] = 0;               // work counter of the TLAS pass of this bounce (two-level scenes, binned)
    for (int x = 0; x < 8; x++) reinterpret_cast<uint32_t *>(bounce_counts + WORK_COUNTERS + (size_t)b * WORK_COUNTERS_PER_BOUNCE)[x * XCD_COUNTER_STRIDE] = 0;      // work counters of the persistent trace launch of this bounce (one per XCD region)
    bounce_counts[65 + b] = 0;               // two-level scenes, binned: {pairs queued (lo), work counter of the BLAS pass (hi)}
    return c;
}
#ifdef MRT_PROBE_SHADE_TAILS
constexpr size_t PROBE_TAIL_WORDS = 32 * 8 * 16;      // the probe build's eight reservation words per bounce, 128 bytes apart, behind the work counters (probe_tails_mask below)
#else
constexpr size_t PROBE_TAIL_WORDS = 0;
#endif
__global__ void __launch_bounds__(64) k_accumulate(FrameParams fp, const float4 *__restrict__ sample, const float4 *__restrict__ prev, float4 *__restrict__ dst,
                                                   unsigned long long *__restrict__ bounce_counts, unsigned long long *__restrict__ totals, uint32_t primary) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long closest = primary, shadow = 0;
        for (int b = 0; b < fp.max_bounces; b++) {
            const unsigned long long c = fold_bounce_counters(bounce_counts, b);
            if (b + 1 < fp.max_bounces) closest += (uint32_t)c;
            shadow += c >> 32;
        }
        atomicAdd(&totals[0], closest); atomicAdd(&totals[1], shadow); atomicAdd(&totals[2], (unsigned long long)primary);      // (the tile groups of a pass accumulate side by side)
    }
    uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    int x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    uint32_t pix = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int sub = 0; sub < fp.batch; sub++) {                           // the batch's frames, in frame order
        const float4 sm = qload(&sample[(size_t)sub * fp.capacity + slot]);
        const uint32_t frame = fp.frameIndex + (uint32_t)sub;
        if (frame > 0) {
            const float4 p = sub == 0 ? q2load(&prev[pix]) : c;
            float fi = (float)frame;
            float den = (float)(frame + 1);
            c.x = (sm.x + p.x * fi) / den; c.y = (sm.y + p.y * fi) / den; c.z = (sm.z + p.z * fi) / den;
        } else c = sm;
    }
    q2store(&dst[pix], make_float4(c.x, c.y, c.z, 1.0f));
}

// Shadow planes (default): shade(b) leaves the light's contribution in con[b][pixel], a shadow ray that gets
// through sets lit[pixel][b] (one byte of the four a pixel has per frame), and the pixel's sample is the sum of the contributions whose byte is set, in bounce order — the additions of
// Raytracing.metal:371-373 on the same floats in the same order as the read-modify-write of one sample buffer made them (0 + c0, + c1, + c2).  Per shadow ray
// that is 16 bytes written and one byte instead of 32 bytes through the queue and a 32-byte read-modify-write inside the traversal loop.
MRT_DEV float4 planes_sample(const float4 *const (&con)[3], const uint8_t *__restrict__ lit, int max_bounces, size_t sp) {
    float4 sm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t flags = reinterpret_cast<const uint32_t *>(lit)[sp];      // byte b: the shadow ray of bounce b got through
#pragma unroll
    for (int b = 0; b < 3; b++)
        if (b < max_bounces && ((flags >> (8 * b)) & 0xFFu) != 0u) { const float4 cc = qload(&con[b][sp]); sm = make_float4(sm.x + cc.x, sm.y + cc.y, sm.z + cc.z, 0.0f); }
    return sm;
}
__global__ void __launch_bounds__(64) k_accumulate_planes(FrameParams fp, const float4 *__restrict__ con0, const float4 *__restrict__ con1, const float4 *__restrict__ con2, const uint8_t *__restrict__ lit,
                                                          const float4 *__restrict__ prev, float4 *__restrict__ dst, unsigned long long *__restrict__ bounce_counts, unsigned long long *__restrict__ totals, uint32_t primary) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long closest = primary, shadow = 0;
        for (int b = 0; b < fp.max_bounces; b++) {
            const unsigned long long c = fold_bounce_counters(bounce_counts, b);
            if (b + 1 < fp.max_bounces) closest += (uint32_t)c;
            shadow += c >> 32;
        }
        atomicAdd(&totals[0], closest); atomicAdd(&totals[1], shadow); atomicAdd(&totals[2], (unsigned long long)primary);
    }
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    int x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t pix = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
    const float4 *const con[3] = {con0, con1, con2};
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int sub = 0; sub < fp.batch; sub++) {                           // the batch's frames, in frame order
        const float4 sm = planes_sample(con, lit, fp.max_bounces, (size_t)sub * fp.capacity + slot);
        const uint32_t frame = fp.frameIndex + (uint32_t)sub;
        if (frame > 0) {
            const float4 p = sub == 0 ? q2load(&prev[pix]) : c;
            const float fi = (float)frame, den = (float)(frame + 1);
            c.x = (sm.x + p.x * fi) / den; c.y = (sm.y + p.y * fi) / den; c.z = (sm.z + p.z * fi) / den;
        } else c = sm;
    }
    q2store(&dst[pix], make_float4(c.x, c.y, c.z, 1.0f));
}

// The last passes of a draw, accumulated in ONE launch on the main stream (Renderer::tail_accumulate): their accumulate launches would otherwise run one after the other at the very
// end of the call — each reads the previous one's output — when nothing else is left to overlap them with (rocprofv3, the driver's 20 steps: five launches of 60-90 us plus their
// gaps, 0.6 of 12.8 ms).  Same folds in the same order (pass by pass, frame by frame); the accumulation target is read once and written once.
struct AccPass { const float4 *con0, *con1, *con2; const uint8_t *lit; unsigned long long *counts; uint32_t frameIndex; int32_t batch; uint32_t primary; uint32_t pad; };
struct AccGroup { AccPass p[MAX_FRAMES_IN_FLIGHT]; int32_t n; };
__global__ void __launch_bounds__(64) k_accumulate_planes_group(FrameParams fp, AccGroup g, const float4 *__restrict__ prev, float4 *__restrict__ dst, unsigned long long *__restrict__ totals) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long closest = 0, shadow = 0, primary = 0;
        for (int p = 0; p < MAX_FRAMES_IN_FLIGHT; p++) {
            if (p >= g.n) break;
            closest += g.p[p].primary; primary += g.p[p].primary;
            for (int b = 0; b < fp.max_bounces; b++) {
                const unsigned long long c = fold_bounce_counters(g.p[p].counts, b);
                if (b + 1 < fp.max_bounces) closest += (uint32_t)c;
                shadow += c >> 32;
            }
        }
        totals[0] += closest; totals[1] += shadow; totals[2] += primary;
    }
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    int x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t pix = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool first = true;
    for (int p = 0; p < MAX_FRAMES_IN_FLIGHT; p++) {
        if (p >= g.n) break;
        const float4 *const con[3] = {g.p[p].con0, g.p[p].con1, g.p[p].con2};
        for (int sub = 0; sub < g.p[p].batch; sub++) {
            const float4 sm = planes_sample(con, g.p[p].lit, fp.max_bounces, (size_t)sub * fp.capacity + slot);
            const uint32_t frame = g.p[p].frameIndex + (uint32_t)sub;
            if (frame > 0) {
                const float4 q = first ? q2load(&prev[pix]) : c;
                const float fi = (float)frame, den = (float)(frame + 1);
                c.x = (sm.x + q.x * fi) / den; c.y = (sm.y + q.y * fi) / den; c.z = (sm.z + q.z * fi) / den;
            } else c = sm;
            first = false;
        }
    }
    q2store(&dst[pix], make_float4(c.x, c.y, c.z, 1.0f));
}

// A shard's own pixels as a compact buffer, and back (the compact assemble of a tile-sharded image: mrt_renderer_pack_owned_tiles / _unpack_tiles, mrt_group reduce mode 2).
// Layout: tiles_local x 64 RGBA32F — tile lt of shard (rank, world) is tile lt * world + rank of the image, its 8 x 8 pixels row-major; pixels of an edge tile
// outside the image are 0 in the buffer and skipped on the way back.  1 / world of the image instead of the full frame the reduce(sum) moves per rank.
template <bool PACK>
__global__ void k_tiles(float4 *__restrict__ image, int w, int h, int tiles_x, int rank, int world, uint32_t tiles_local, float4 *__restrict__ compact) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x, lt = slot >> 6, k = slot & 63u;
    if (lt >= tiles_local) return;
    const uint32_t tile = lt * (uint32_t)world + (uint32_t)rank, ty = tile / (uint32_t)tiles_x, tx = tile - ty * (uint32_t)tiles_x;
    const int x = (int)(tx * 8u + (k & 7u)), y = (int)(ty * 8u + (k >> 3));
    const bool in = x < w && y < h;
    if (PACK) compact[slot] = in ? image[(size_t)y * w + x] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    else if (in) image[(size_t)y * w + x] = compact[slot];
}

// Shaders.metal:39-52 — Reinhard + vertical flip (the blit's uv, :35), RGBA8
__global__ void k_tonemap(const float4 *__restrict__ accum, int w, int h, uchar4 *__restrict__ out) {
    int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    float4 a = accum[(size_t)(h - 1 - y) * w + x];
    float c[3] = {a.x, a.y, a.z};
    unsigned char o[3];
    for (int k = 0; k < 3; k++) { float v = c[k] / (1.0f + c[k]); v = saturatef(v); o[k] = (unsigned char)(v * 255.0f + 0.5f); }
    out[(size_t)y * w + x] = make_uchar4(o[0], o[1], o[2], 255);
}

// ------------------------------------------------------------------ device-function probes
__global__ void k_probe_halton(const int32_t *i, const int32_t *d, uint32_t n, float *out) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = halton_dev(i[k], d[k]);
}
__global__ void k_probe_hemisphere(const float *u2, const float *n3, uint32_t n, float *out3) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    f3 v = align_hemisphere_dev(sample_cosine_hemisphere_dev(u2[2 * k], u2[2 * k + 1]), mk3(n3[3 * k], n3[3 * k + 1], n3[3 * k + 2]));
    out3[3 * k] = v.x; out3[3 * k + 1] = v.y; out3[3 * k + 2] = v.z;
}

// Launch with the kernel's own start/stop events when `ev` is given (bench.py's live roofline measurement).
template <class... KArgs, class... Args>
static inline void launch_timed(EvPair *ev, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t shmem, hipStream_t st, Args... args) {
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shmem, st, ev->a, ev->b, 0, static_cast<KArgs>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, shmem, st, static_cast<KArgs>(args)...);
}

}  // namespace

#ifdef MRT_WAVE_TIMES
int read_wave_times(unsigned long long *out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), sizeof(g_wave_times)) == hipSuccess ? MRT_OK : MRT_ERR_HIP; }
int read_wave_iters(uint32_t *out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_iters), sizeof(g_wave_iters)) == hipSuccess ? MRT_OK : MRT_ERR_HIP; }
int read_drain_probe(unsigned long long *out18, int reset) {
    if (hipMemcpyFromSymbol(out18, HIP_SYMBOL(g_drain_probe), sizeof(g_drain_probe)) != hipSuccess) return MRT_ERR_HIP;
    if (reset) { static const unsigned long long z[18] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_drain_probe), z, sizeof z) != hipSuccess) return MRT_ERR_HIP; }
    return MRT_OK;
}
#endif

// ====================================================================== Renderer (host)
// The table of bounce 0's Halton values (FrameParams::halton_tab) for the indices [w0, w0 + HALTON_TAB_SPAN): a pass needs offset + sampleIndex + sub-frame for offsets below 2^20.
// Once per draw, on the MAIN stream ahead of the fork: every lane of this draw starts behind it (the fork event), and every pass of earlier draws has been joined into the main stream
// — no host or device synchronisation (until round 6 a window move drained the whole device from inside the enqueue loop).  The window follows the draw's first frame when the draw's
// first pass would leave it; what a very long draw reaches beyond the window falls back to the recurrence per index (halton_b0), bit-identical either way.
int Renderer::ensure_halton_table(uint32_t sample_index, uint32_t frames) {
    const uint64_t first_pass = std::min<uint64_t>(frames, MAX_FRAME_BATCH);
    const bool fits = halton_tab.p != nullptr && sample_index >= halton_w0 && (uint64_t)sample_index + first_pass + (1u << 20) <= (uint64_t)halton_w0 + HALTON_TAB_SPAN;
    if (fits) return MRT_OK;
    if (!halton_tab.p) MRT_HIP(halton_tab.alloc((size_t)HALTON_TAB_DIMS * HALTON_TAB_SPAN));
    halton_w0 = sample_index;
    hipLaunchKernelGGL(k_halton_table, dim3(cdiv(HALTON_TAB_SPAN, 256), HALTON_TAB_DIMS), dim3(256), 0, stream, halton_tab.p, halton_w0, HALTON_TAB_SPAN);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int Renderer::init(hipStream_t st, const DeviceScene *sc, int w, int h, uint32_t seed_, int max_bounces_) {
    stream = st; scene = sc; seed = seed_; max_bounces = max_bounces_;
    MRT_HIP(hipEventCreate(&ev_begin)); MRT_HIP(hipEventCreate(&ev_end));
    MRT_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    for (auto &e : ev_ext) { MRT_HIP(hipEventCreate(&e.a)); MRT_HIP(hipEventCreate(&e.b)); }
    for (auto &L : lanes) {
        MRT_HIP(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        MRT_HIP(hipEventCreateWithFlags(&L.accumulated, hipEventDisableTiming));
        // per bounce b: [b] queue counts {next rays (lo 32), shadow rays (hi 32)}; [32 + b] work counter of the TLAS pass and [65 + b] {pairs queued, work counter of the BLAS pass} (two-level scenes, binned);
        // from WORK_COUNTERS on: the eight work counters of the pulling traversal launch, 128 bytes apart (XcdRegions); from SEG_TAILS on: the eight tail words of a segmented pass
        MRT_HIP(L.bounce_counts.alloc(SEG_TAILS + 32 * SEG_TAILS_PER_BOUNCE + PROBE_TAIL_WORDS));
        MRT_HIP(hipMemsetAsync(L.bounce_counts.p, 0, L.bounce_counts.bytes(), stream));
    }
    MRT_HIP(totals.alloc(4));
    MRT_HIP(hipMemsetAsync(totals.p, 0, totals.bytes(), stream));
    return resize(w, h);
}

Renderer::~Renderer() {
    if (ev_begin) (void)hipEventDestroy(ev_begin);
    if (ev_end) (void)hipEventDestroy(ev_end);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    for (auto &e : ev_ext) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    for (auto &pd : passes_pending) (void)hipEventDestroy(pd.ev);
    for (auto e : pass_events_free) (void)hipEventDestroy(e);
    if (guide_stream) { (void)hipStreamSynchronize(guide_stream); (void)hipStreamDestroy(guide_stream); }
    if (guide_done) (void)hipEventDestroy(guide_done);
    if (guide_fork) (void)hipEventDestroy(guide_fork);
    for (auto &L : lanes) {
        if (L.stream) { (void)hipStreamSynchronize(L.stream); (void)hipStreamDestroy(L.stream); }
        if (L.accumulated) (void)hipEventDestroy(L.accumulated);
    }
}

// frame_batch = 0: a pass carries about as many pixel-frames as eight 1080p frames, whatever the image — a launch over 256 x 256 pixels x 8 frames is a sixteenth of one the kernels were
// tuned on and the pipeline is launch-bound there (Cornell 256^2: 6.7 Grays/s in 8-frame passes, 9.8-10.8 in 32-frame ones; 640 x 360: 9.0 -> 10.4; 960 x 540: 10.9 -> 11.5).  The rule a
// tile-sharded rank follows (distributed.py shard_frame_batch: 8 x world) is the same rule: its pixels are a world-th of the image.
int Renderer::batch_wanted() const {
    if (frame_batch > 0) return std::min(frame_batch, MAX_FRAME_BATCH);
    const size_t owned = std::max<size_t>(1, (size_t)std::max(width, 1) * (size_t)std::max(height, 1) / (size_t)std::max(shard_world, 1));
    const size_t ref = (size_t)DEFAULT_FRAME_BATCH * 1920 * 1080;
    return (int)std::min<size_t>(MAX_FRAME_BATCH, std::max<size_t>(DEFAULT_FRAME_BATCH, (ref + owned - 1) / owned));
}

int Renderer::resize(int w, int h) {                                   // Renderer.swift:353-356 → createTextures :231-275
    width = w; height = h;
    const size_t npix = (size_t)w * h;
    const int B = batch_wanted();
    alloc_batch = B;
    MRT_HIP(hint.alloc(npix));
    MRT_HIP(hipMemsetAsync(hint.p, 0xFF, hint.bytes(), stream));
    MRT_HIP(accum[0].alloc(npix)); MRT_HIP(accum[1].alloc(npix));
    MRT_HIP(hipMemsetAsync(accum[0].p, 0, accum[0].bytes(), stream));
    MRT_HIP(hipMemsetAsync(accum[1].p, 0, accum[1].bytes(), stream));
    default_camera(w, h, &camera);
    frame_index = 0; cur = 0;
    MRT_HIP(hipMemsetAsync(totals.p, 0, totals.bytes(), stream));
    frames_rendered = 0;
    for (auto &pd : passes_pending) pass_events_free.push_back(pd.ev);      // the caller synchronised (mrt_renderer_resize)
    passes_pending.clear(); frames_completed_known = 0;
    denoised_valid = false;
    if (guides && !guides_keep) {          // the guides restart with the accumulation (new size: new buffers at the next draw)
        if (guide_nd.p && guide_nd.n != npix) { guide_nd.release(); guide_albedo.release(); guide_ids.release(); }
        for (auto &b : dn_scratch) b.release();
        denoised.release();
        if (int rc = clear_guides()) return rc;
    }
    return alloc_queues();
}

int Renderer::note_pass(hipStream_t st) {
    // more than 1024 passes queued ahead of the GPU: the newest entry absorbs further passes (its event is re-recorded)
    if (passes_pending.size() < 1024 || passes_pending.empty()) {
        hipEvent_t e = nullptr;
        if (!pass_events_free.empty()) { e = pass_events_free.back(); pass_events_free.pop_back(); }
        else MRT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        passes_pending.push_back(PassDone{e, frames_rendered});
    } else passes_pending.back().frames_through = frames_rendered;
    MRT_HIP(hipEventRecord(passes_pending.back().ev, st));
    return MRT_OK;
}
int Renderer::poll_completed(uint64_t *out) {
    while (!passes_pending.empty()) {
        const hipError_t q = hipEventQuery(passes_pending.front().ev);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (q != hipSuccess) return hip_fail(q, "hipEventQuery", __FILE__, __LINE__);
        frames_completed_known = passes_pending.front().frames_through;
        pass_events_free.push_back(passes_pending.front().ev);
        passes_pending.pop_front();
    }
    *out = frames_completed_known;
    return MRT_OK;
}

int Renderer::alloc_queues() {
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const int tiles = tiles_x * tiles_y;
    tiles_local = (tiles - shard_rank + shard_world - 1) / shard_world;
    if (tiles_local < 0) tiles_local = 0;
    capacity = (uint32_t)tiles_local * 64u;
    {   // the seed table, by sample index (sub-frame * capacity + slot): this shard's pixels only
        const int B = std::max(1, alloc_batch);
        MRT_HIP(seeds.alloc((size_t)std::max<uint32_t>(capacity, 1u) * B));
        FrameParams sp{}; sp.width = width; sp.height = height; sp.shard_rank = shard_rank; sp.shard_world = shard_world; sp.tiles_x = tiles_x; sp.tiles_local = tiles_local; sp.capacity = capacity;
        if (capacity) hipLaunchKernelGGL(k_seed_slots, dim3(cdiv(capacity, 256), B), dim3(256), 0, stream, seeds.p, sp, seed);
    }
    tgroups_for = 0;            // the tile groups' seed tables follow the shard and the image size: rebuilt at the next draw that uses groups
    // lanes get their buffers when first used (alloc_lane): 16 lanes x 4-frame queues would pin 23 GB at 1080p, 94 GB at 4K
    lanes_ready = 0;
    for (auto &L : lanes) release_lane(L);
    // pixels owned by this shard (edge tiles may be partial)
    uint64_t owned = 0;
    for (int lt = 0; lt < tiles_local; lt++) {
        int tile = lt * shard_world + shard_rank, ty = tile / tiles_x, tx = tile % tiles_x;
        int pw = std::min(8, width - tx * 8), ph = std::min(8, height - ty * 8);
        owned += (uint64_t)pw * ph;
    }
    owned_pixels = owned;
    return MRT_OK;
}

constexpr int PLANES_MAX_BOUNCES = 3;        // shadow planes: sample + two more contribution planes, three flag bytes of the pixel's word

// Segments of a bundled pass of B frames over `capacity` slots (PassPlan::segs): what its shade(0) launch looks like and what a segment can receive.
// INVARIANT: segment x receives the entries of shade(0)'s blocks j = x (mod 8) — `blocks_per_seg` of them at most, each emitting at most `per_block` entries per queue (its
// active lanes) — so seg_cap = blocks_per_seg x per_block holds bounce 0; a packing block of a later bounce reads one segment and writes the same one, one entry per queue at
// most for each entry read, so no later bounce can hold more.  When bundle_groups x bundle_w == B (passes of 7, 8, 16, 32 frames), 8 x seg_cap exceeds capacity x B by less
// than QUEUE_SEGMENTS x SHADE_THREADS entries: the slack alloc_lane adds.  plan_pass checks 8 x seg_cap against the allocation and keeps one queue otherwise.
SegmentSizing segment_sizing(uint32_t capacity, int B) {
    SegmentSizing z;
    z.bundle_groups = ((uint32_t)B + 7u) / 8u; z.bundle_w = ((uint32_t)B + z.bundle_groups - 1u) / z.bundle_groups; z.bundle_per_wave = 64u / z.bundle_w;
    const uint64_t waves = cdiv((uint64_t)capacity * z.bundle_groups, (uint64_t)z.bundle_per_wave);
    z.blocks = cdiv(waves * 64u, (uint64_t)SHADE_THREADS);
    z.per_block = (uint32_t)SHADE_WAVES * z.bundle_per_wave * z.bundle_w;
    z.seg_cap = cdiv(z.blocks, (uint64_t)QUEUE_SEGMENTS) * z.per_block;
    return z;
}
size_t queue_entries(uint32_t capacity, int alloc_batch) {
    size_t qcap = (size_t)capacity * (size_t)std::max(1, alloc_batch);      // a batch of frames shares one set of queues
    qcap += (size_t)QUEUE_SEGMENTS * SHADE_THREADS;      // segmented passes: the rounding of eight segments' capacities (segment_sizing)
#ifdef MRT_PROBE_SHADE_TAILS
    qcap += 8 * (size_t)SHADE_PACK_RANGE;      // the probe's disjoint segments: eight times the rounding of a segment's capacity (enqueue_shade)
#endif
    return qcap;
}
size_t Renderer::lane_bytes() const {
    const size_t qcap = queue_entries(capacity, alloc_batch);
    const bool need_thr = !(throughput_chain && !materials && max_bounces <= 3);
    const size_t spix = (size_t)std::max<uint32_t>(capacity, 1u) * (size_t)std::max(1, alloc_batch);      // sample indices of a pass: sub-frame * capacity + slot
    const size_t planes_bytes = shadow_planes ? 2 * spix * sizeof(float4) + spix * 4 : 0;
    const bool need_scon = need_thr || !shadow_planes;
    const size_t pairs_bytes = (scene && scene->num_inst && scene->num_wnodes && tl_pairs && shadow_planes && !need_thr) ? 2 * PairQueue::WORDS * qcap * sizeof(uint4) : 0;      // two-level scenes: the (ray, instance) queue of the binned walk
    return ((need_thr ? 9 : 7) * qcap + (need_scon ? qcap : 0) + spix) * sizeof(float4) + planes_bytes + pairs_bytes;
}
void Renderer::release_lane(FrameLane &L) {
    for (int k = 0; k < 2; k++) { L.rayA[k].release(); L.rayB[k].release(); L.thr[k].release(); L.f_con[k].release(); }
    L.hits.release(); L.srayA.release(); L.srayB.release(); L.scon.release(); L.sample.release(); L.f_lit.release(); L.pairs.release();
}
int Renderer::alloc_planes(FrameLane &L) {
    const size_t spix = (size_t)std::max<uint32_t>(capacity, 1u) * (size_t)std::max(1, alloc_batch);      // sample indices of a pass: sub-frame * capacity + slot
    for (int k = 0; k < 2; k++) MRT_HIP(L.f_con[k].alloc(spix));
    MRT_HIP(L.f_lit.alloc(spix * 4));          // [sub-frame][pixel][bounce]: one 32-bit word per pixel and frame
    return MRT_OK;
}
int Renderer::alloc_lane(FrameLane &L) {
    const size_t qcap = queue_entries(capacity, alloc_batch);
    const bool need_thr = !(throughput_chain && !materials && max_bounces <= 3);      // else on demand (prepare_lane)
    for (int k = 0; k < 2; k++) { MRT_HIP(L.rayA[k].alloc(qcap)); MRT_HIP(L.rayB[k].alloc(qcap)); if (need_thr) MRT_HIP(L.thr[k].alloc(qcap)); }
    MRT_HIP(L.hits.alloc(qcap)); MRT_HIP(L.srayA.alloc(qcap)); MRT_HIP(L.srayB.alloc(qcap));
    if (need_thr || !shadow_planes) MRT_HIP(L.scon.alloc(qcap));          // the contribution queue: with shadow planes only the passes they do not cover need it (allocated then, prepare_lane)
    MRT_HIP(L.sample.alloc((size_t)std::max<uint32_t>(capacity, 1u) * (size_t)std::max(1, alloc_batch)));
    MRT_HIP(hipMemsetAsync(L.sample.p, 0, L.sample.bytes(), stream));
    if (shadow_planes && !need_thr) { if (int rc = alloc_planes(L)) return rc; }
    return MRT_OK;
}

// The G tile groups of this renderer's shard (renderer.h TileGroup) and their seed tables, built on the main stream (every lane forks from it at the next draw).
int Renderer::ensure_tile_groups(int G) {
    const int Bq = std::max(1, alloc_batch);
    if (tgroups_for == G && tgroups_batch == Bq) return MRT_OK;
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8, tiles = tiles_x * tiles_y;
    for (int g = 0; g < G; g++) {
        TileGroup &T = tgroups[g];
        T.rank = g * shard_world + shard_rank; T.world = G * shard_world;
        T.tiles_local = std::max(0, (tiles - T.rank + T.world - 1) / T.world);
        T.capacity = (uint32_t)T.tiles_local * 64u;
        T.owned = 0;
        for (int lt = 0; lt < T.tiles_local; lt++) {
            const int tile = lt * T.world + T.rank, ty = tile / tiles_x, tx = tile % tiles_x;
            T.owned += (uint64_t)std::min(8, width - tx * 8) * (uint64_t)std::min(8, height - ty * 8);
        }
        MRT_HIP(seeds_g[g].alloc((size_t)std::max<uint32_t>(T.capacity, 1u) * Bq));
        FrameParams sp{}; sp.width = width; sp.height = height; sp.shard_rank = T.rank; sp.shard_world = T.world; sp.tiles_x = tiles_x; sp.tiles_local = T.tiles_local; sp.capacity = T.capacity;
        if (T.capacity) hipLaunchKernelGGL(k_seed_slots, dim3(cdiv(T.capacity, 256), Bq), dim3(256), 0, stream, seeds_g[g].p, sp, seed);
        T.seeds = seeds_g[g].p;
    }
    tgroups_for = G; tgroups_batch = Bq;
    return MRT_OK;
}

int Renderer::set_shard(int rank, int world) {
    if (world < 1 || rank < 0 || rank >= world) { set_error("invalid shard"); return MRT_ERR_INVALID_ARGUMENT; }
    shard_rank = rank; shard_world = world;
    MRT_HIP(hipStreamSynchronize(stream));
    MRT_HIP(hipMemsetAsync(accum[0].p, 0, accum[0].bytes(), stream));
    MRT_HIP(hipMemsetAsync(accum[1].p, 0, accum[1].bytes(), stream));
    frame_index = 0; cur = 0;
    if (int rc = clear_guides()) return rc;
    return alloc_queues();
}

// ---- guide buffers (guides.h)
int Renderer::clear_guides() {
    guides_valid = false; denoised_valid = false;
    if (guide_nd.p) {
        MRT_HIP(hipMemsetAsync(guide_nd.p, 0, guide_nd.bytes(), stream)); MRT_HIP(hipMemsetAsync(guide_albedo.p, 0, guide_albedo.bytes(), stream));
        MRT_HIP(hipMemsetAsync(guide_ids.p, 0, guide_ids.bytes(), stream));
    }
    return MRT_OK;
}
int Renderer::set_guides(bool on) {
    if (on == guides) return MRT_OK;
    guides = on;
    if (!on) {          // off: nothing stays allocated
        MRT_HIP(hipStreamSynchronize(stream));
        guide_nd.release(); guide_albedo.release(); guide_ids.release(); denoised.release();
        for (auto &b : dn_scratch) b.release();
        guides_valid = false; denoised_valid = false;
    }
    return MRT_OK;
}
int Renderer::ensure_guides() {
    const size_t npix = (size_t)width * height;
    if (!guide_stream) { MRT_HIP(hipStreamCreateWithFlags(&guide_stream, hipStreamNonBlocking)); MRT_HIP(hipEventCreateWithFlags(&guide_done, hipEventDisableTiming)); MRT_HIP(hipEventCreateWithFlags(&guide_fork, hipEventDisableTiming)); }
    if (guide_nd.p && guide_nd.n == npix) return MRT_OK;
    MRT_HIP(guide_nd.alloc(npix)); MRT_HIP(guide_albedo.alloc(npix)); MRT_HIP(guide_ids.alloc(npix));
    return clear_guides();
}
int Renderer::read_guide(int which, void *out, size_t nbytes) {
    if (which < 0 || which >= MRT_GUIDE_COUNT) { set_error("read_guide: which must be MRT_GUIDE_NORMAL_DEPTH, MRT_GUIDE_ALBEDO or MRT_GUIDE_IDS"); return MRT_ERR_INVALID_ARGUMENT; }
    if (nbytes != (size_t)width * height * 16) { set_error("read_guide: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!guides || !guides_valid) { set_error("read_guide: no guide buffers (renderer option guides = 1, then render)"); return MRT_ERR_STATE; }
    int rc = wait(); if (rc) return rc;
    MRT_HIP(hipMemcpy(out, which == MRT_GUIDE_NORMAL_DEPTH ? (const void *)guide_nd.p : which == MRT_GUIDE_ALBEDO ? (const void *)guide_albedo.p : (const void *)guide_ids.p, nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}
int Renderer::copy_guide_to_device(int which, void *dptr, size_t nbytes) {
    if (which < 0 || which >= MRT_GUIDE_COUNT) { set_error("copy_guide_to_device: which must be MRT_GUIDE_NORMAL_DEPTH, MRT_GUIDE_ALBEDO or MRT_GUIDE_IDS"); return MRT_ERR_INVALID_ARGUMENT; }
    if (nbytes != (size_t)width * height * 16) { set_error("copy_guide_to_device: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!guides || !guides_valid) { set_error("copy_guide_to_device: no guide buffers (renderer option guides = 1, then render)"); return MRT_ERR_STATE; }
    MRT_HIP(hipMemcpyAsync(dptr, which == MRT_GUIDE_NORMAL_DEPTH ? (const void *)guide_nd.p : which == MRT_GUIDE_ALBEDO ? (const void *)guide_albedo.p : (const void *)guide_ids.p, nbytes, hipMemcpyDeviceToDevice, stream));
    return MRT_OK;
}
int Renderer::enqueue_denoise(const MRTDenoiseParams *params) {
    MRTDenoiseParams p{};
    if (params) p = *params;
    else { p.iterations = MRT_DENOISE_DEFAULT_ITERATIONS; p.sigma_color = MRT_DENOISE_DEFAULT_SIGMA_COLOR; p.sigma_normal = MRT_DENOISE_DEFAULT_SIGMA_NORMAL; p.sigma_depth = MRT_DENOISE_DEFAULT_SIGMA_DEPTH; p.demodulate = 1; }
    if (p.iterations < 1 || p.iterations > 8) { set_error("denoise: iterations must be in [1,8]"); return MRT_ERR_INVALID_ARGUMENT; }
    const float big = 3.0e38f;
    if (!(p.sigma_color > 0.0f && p.sigma_color < big) || !(p.sigma_normal > 0.0f && p.sigma_normal < big) || !(p.sigma_depth > 0.0f && p.sigma_depth < big)) { set_error("denoise: sigma_color, sigma_normal and sigma_depth must be finite and > 0"); return MRT_ERR_INVALID_ARGUMENT; }
    if (p.demodulate != 0 && p.demodulate != 1) { set_error("denoise: demodulate must be 0 or 1"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!guides || !guides_valid) { set_error("denoise: no guide buffers (renderer option guides = 1, then render)"); return MRT_ERR_STATE; }
    if (shard_world > 1) { set_error("denoise: a sharded renderer holds only its own tiles and the filter needs a pixel's neighbours"); return MRT_ERR_STATE; }
    const size_t npix = (size_t)width * height;
    for (auto &b : dn_scratch) MRT_HIP(b.alloc(npix));
    MRT_HIP(denoised.alloc(npix));
    if (int rc = denoise_enqueue(stream, width, height, accum[cur].p, guide_nd.p, guide_albedo.p, dn_scratch[0].p, dn_scratch[1].p, denoised.p, p)) return rc;
    denoised_valid = true;
    return MRT_OK;
}
int Renderer::read_denoised(float *rgba, size_t nbytes) {
    if (nbytes != (size_t)width * height * 16) { set_error("read_denoised: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!denoised_valid) { set_error("read_denoised: no denoised image (mrt_renderer_denoise first)"); return MRT_ERR_STATE; }
    int rc = wait(); if (rc) return rc;
    MRT_HIP(hipMemcpy(rgba, denoised.p, nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}
int Renderer::copy_denoised_to_device(void *dptr, size_t nbytes) {
    if (nbytes != (size_t)width * height * 16) { set_error("copy_denoised_to_device: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!denoised_valid) { set_error("copy_denoised_to_device: no denoised image (mrt_renderer_denoise first)"); return MRT_ERR_STATE; }
    MRT_HIP(hipMemcpyAsync(dptr, denoised.p, nbytes, hipMemcpyDeviceToDevice, stream));
    return MRT_OK;
}
int Renderer::read_denoised_tonemapped(uint8_t *rgba, size_t nbytes) {
    if (nbytes != (size_t)width * height * 4) { set_error("read_denoised_tonemapped: nbytes must be width*height*4"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!denoised_valid) { set_error("read_denoised_tonemapped: no denoised image (mrt_renderer_denoise first)"); return MRT_ERR_STATE; }
    DevBuf<uchar4> tmp; MRT_HIP(tmp.alloc((size_t)width * height));
    hipLaunchKernelGGL(k_tonemap, dim3(cdiv(width, 16), cdiv(height, 16)), dim3(16, 16), 0, stream, (const float4 *)denoised.p, width, height, tmp.p);
    int rc = wait(); if (rc) return rc;
    MRT_HIP(hipMemcpy(rgba, tmp.p, nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}

// ---- the frame driver (Renderer.draw(in:) :284-351, n times).  A draw is decided first — plan_draw: passes, lanes, tile groups; plan_pass: kernels, grids, what it can be refused
// for — by host arithmetic alone, and enqueued then: the enqueue_* steps read the plans and decide nothing.
#ifdef MRT_DIAGNOSTICS
// measuring aid of the diagnostics build only (tools/build_variant.sh diag "-DMRT_DIAGNOSTICS"; tools/archive/gpu_stage_ablation.sh): MRT_ABLATE=1 skips the primary launches, =2 the
// bounce / shadow traversal launches — the other kernels then run on the stale but well-formed queues of an earlier pass, so their load is realistic and the frame time shows
// what the skipped stage costs under overlap.  Images are garbage; the release library does not read the variable.
static inline int ablate_mask() { static const int mask = getenv("MRT_ABLATE") ? atoi(getenv("MRT_ABLATE")) : 0; return mask; }
#else
static constexpr int ablate_mask() { return 0; }
#endif
#ifdef MRT_PROBE_SHADE_TAILS
// timing probe of the shade kernels' queue reservation (tools/build_variant.sh tails "-DMRT_PROBE_SHADE_TAILS"; tools/shade_tail_probe.py): MRT_PROBE_TAILS is a mask of bounces whose
// shade launch reserves on eight words, 128 bytes apart, behind the lane's counters (block j on word j & 7) instead of on bounce_counts[b].  The eight words are zeroed ahead of the
// launch, so no ticket exceeds what the one word would have handed out and every store stays inside the queues; bounce_counts[b] stays 0, so the stages behind the probed launch
// find empty queues.  Images are garbage; only the probed launch's time is read (MRT_PROBE_LOG=1: wait() prints every timed launch of the draw, in enqueue order).
static inline int probe_disjoint() { static const int v = getenv("MRT_PROBE_DISJOINT") ? atoi(getenv("MRT_PROBE_DISJOINT")) : 0; return v; }
__global__ void k_probe_tails_init(unsigned long long *__restrict__ words, uint32_t seg_cap) {
    if (threadIdx.x < 8u) { const unsigned long long v = (unsigned long long)seg_cap * threadIdx.x; words[threadIdx.x * 16u] = v | (v << 32); }
}
static inline int probe_tails_mask() { static const int mask = getenv("MRT_PROBE_TAILS") ? atoi(getenv("MRT_PROBE_TAILS")) : 0; return mask; }
#endif
// MRT_WAVE_TIMES builds: a traversal launch carries its bounce in the top byte of its chunk / rays-per-wave argument
static inline uint32_t tag_bounce(uint32_t arg, int b) {
#ifdef MRT_WAVE_TIMES
    return arg | ((uint32_t)b << 24);
#else
    (void)b; return arg;
#endif
}

// What the steps of one draw share: the plans, the uniforms of the pass being enqueued, and what a pass hands to the next
struct DrawCtx {
    SceneView sv;
    DrawPlan dp;
    FrameParams fp;                      // begin_draw: the draw's uniforms on the renderer's own shard; enqueue_pass sets the pass's and the tile group's fields
    FrameParams gp;                      // the guide launch's (the call's first frame)
    hipEvent_t last_acc, last_acc_g[MAX_TILE_GROUPS];      // the accumulate that the next one waits for (tile groups: the same group's of the pass before)
    AccGroup tail;                       // the passes accumulated together after the join
};

// Resident 64-thread workgroups of `kernel` per compute unit at this LDS size (0: it does not fit); x cu_count = the wave slots of the chip for it.  One occupancy query per
// LDS size, one device lookup per renderer.
template <class K>
static int wave_slots_for(K kernel, size_t lds_bytes, SlotCache &cache, int &cu_count) {
    if (cu_count == 0) { int dev = 0; hipDeviceProp_t prop; MRT_HIP(hipGetDevice(&dev)); MRT_HIP(hipGetDeviceProperties(&prop, dev)); cu_count = prop.multiProcessorCount; }
    if (cache.lds_bytes != lds_bytes) { MRT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&cache.per_cu, kernel, 64, lds_bytes)); cache.lds_bytes = lds_bytes; }
    return MRT_OK;
}

// traversal launches carry their own start/stop events (hipExtLaunchKernelGGL: the dispatch packet's timestamps, the
// same clock rocprofv3 reads): plain hipEventRecord pairs on a stream also count the time a launch waits behind the
// other frames in flight (+12 % at 12 frames)
EvPair *Renderer::timed(int kind) { if (ext_used >= (int)ev_ext.size()) return nullptr; ev_ext[ext_used].kind = kind; return &ev_ext[ext_used++]; }

DrawPlan Renderer::plan_draw(int n_frames) const {
    DrawPlan dp;
    dp.n_frames = n_frames; dp.mega = megakernel; dp.equal = equal_passes != 0; dp.tail = tail_accumulate;
    // passes larger than the default (sharded renderers ask for up to 32 frames so that a shard's launches stay large) never take more than a third of the draw:
    // a short draw keeps about three passes to run side by side (a rank of eight over 20 frames: 7.1 Grays/s as 7 + 7 + 6, 6.0 as one pass of 20)
    const int batch_cap = alloc_batch > DEFAULT_FRAME_BATCH ? std::min(alloc_batch, std::max(DEFAULT_FRAME_BATCH, (n_frames + 2) / 3)) : alloc_batch;
    dp.batch_max = megakernel ? 1 : batch_cap;
    dp.n_passes = (n_frames + dp.batch_max - 1) / dp.batch_max;
    dp.lanes = dp.lanes_plain = std::max(1, std::min(frames_in_flight, MAX_FRAMES_IN_FLIGHT));
    // tile groups: a pass as G groups of tiles on G lanes (renderer.h TileGroup); the one-launch-per-frame mode has no passes to split.
    if (!megakernel && tile_groups != 1 && tiles_local >= 64) {
        const int in_flight = std::max(1, std::min(dp.lanes, dp.n_passes));
        // by the draw (0): only passes of ONE frame — the launch-bound regimes: a frame alone 1.53 -> 1.42 ms as two or three groups (four: 1.53), three one-frame passes in flight
        // 0.85-0.91 -> 0.82-0.83 ms per frame as two groups each; a pass of seven or eight frames is better left whole (the driver's 20 frames as 3 x 2 groups: -4 %; profiles/r05_tile_groups.txt)
        const int by_draw = tile_groups >= 2 ? tile_groups : dp.batch_max > 1 ? 1 : in_flight == 1 ? 3 : in_flight <= 3 ? 2 : 1;
        dp.G = std::max(1, std::min(by_draw, std::min(MAX_FRAMES_IN_FLIGHT / in_flight, tiles_local / 32)));
        if (dp.G > 1) dp.lanes = in_flight * dp.G;          // lanes this draw runs on: G per pass in flight
    }
    return dp;
}

void DrawPlan::settle(int lanes_ready) {
    if (G > 1 && lanes_ready < lanes) { G = 1; lanes = lanes_plain; }      // not enough memory for the groups' lanes: the plain form
    lanes = std::min(lanes, lanes_ready);
    Fp = G > 1 ? lanes / G : lanes;
    tail_from = (tail && G == 1) ? n_passes - std::min(lanes, n_passes) : n_passes;
    long_call = n_passes >= 2 * lanes;
}

// The grid of a pulling launch.  Rays per pull: at least four pulls per wave slot on a queue of this size (so that the launch ends evenly), at most
// persist_chunk; 128-ray pulls of a one-frame launch are ~78 atomics per microsecond on the one counter word (limit ~88)
PullGrid Renderer::pull_grid(size_t slots, size_t slots_of_chip, size_t min_chunk, bool long_call) const {
    PullGrid pg;
    pg.chunk = (uint32_t)std::min<size_t>((size_t)persist_chunk, std::max<size_t>(min_chunk, slots / (slots_of_chip * 4) / 64 * 64));
    // a long call (every lane gets several passes) runs its traversal launches on HALF the wave slots: the other passes' shade, primary
    // and accumulate blocks then find free slots instead of queueing behind persistent waves that only leave when their queue is empty
    // (measured, 240 steps: 4 lanes 9.86 -> 10.06, 6 lanes 10.08 -> 10.32, 12 lanes 10.38 -> 10.55 Grays/s; a 20-step call, whose five
    // passes move in lock step, loses 3 % and keeps the full grid)
    pg.grid_slots = (!wave_slots_user && long_call) ? std::max<size_t>(1, slots_of_chip / 2) : slots_of_chip;
    pg.waves = (uint32_t)std::max<size_t>(1, std::min<size_t>(cdiv(slots, pg.chunk), pg.grid_slots));
    return pg;
}

int Renderer::plan_pass(const DrawPlan &dp, const SceneView &sv, const TileGroup &TG, int B, PassPlan &pp) const {
    pp = PassPlan{};
    pp.B = B; pp.two_level = sv.num_inst > 0;          // instanced scene: TLAS + BLASes walked by the same kernels (<TWO_LEVEL>)
    pp.grid_tiles = std::max<uint32_t>(1u, (uint32_t)TG.tiles_local); pp.grid_shade = std::max<uint32_t>(1u, cdiv(TG.capacity, SHADE_THREADS));
    pp.wave_slots = wave_slots;
    const bool two_level = pp.two_level;
    const size_t wide_stack = (size_t)scene->wide_depth * WIDE_STACK_LEVEL_BYTES;
    if (dp.mega) {
        if (two_level || materials || sv.num_wnodes == 0) {          // the one-launch-per-frame mode exists for flattened scenes on the 8-wide layout, diffuse kernel: say so instead of quietly rendering through the pipeline
            set_error(std::string("megakernel = 1 renders flattened scenes with the 8-wide layout and the reference's diffuse kernel only; this renderer has ") + (two_level ? "a two-level scene (scene option instancing = 1)" : materials ? "materials = 1" : "a scene without the 8-wide layout") + ": set megakernel = 0");
            return MRT_ERR_UNSUPPORTED;
        }
        pp.stack_bytes = wide_stack;
        if (int rc = wave_slots_for(k_megakernel, wide_stack, mega_cache, cu_count)) return rc;
        pp.mega_waves = (uint32_t)std::min<size_t>(std::max<size_t>(1, cdiv(TG.capacity, 64)), (size_t)(std::max(1, mega_cache.per_cu) * cu_count));
        return MRT_OK;
    }
    // the pipeline: primary trace -> per bounce { shade, trace } ; bounce rays and shadow rays of a shade share one traversal launch
    pp.on_wide = wide_bounce && sv.num_wnodes > 0;          // no 8-wide layout (scene option wide = 0, a tree deeper than WIDE_STACK_MAX): the rope kernels
    // two-level scenes walk TLAS and BLASes with the same kernels (traverse_wide_stream<true>); their LDS also parks the lanes' world rays
    pp.stack_bytes = wide_stack + (two_level ? WIDE_WORLD_RAY_BYTES : 0);
    if (pp.on_wide && persistent != 0) {       // wave slots of the chip for this kernel at this LDS size
        if (int rc = two_level ? wave_slots_for(k_trace_mixed_wide_persist<true>, pp.stack_bytes, persist_cache, cu_count) : wave_slots_for(k_trace_mixed_wide_persist<false>, pp.stack_bytes, persist_cache, cu_count)) return rc;
        if (!wave_slots_user) pp.wave_slots = std::max(1, persist_cache.per_cu) * cu_count;
    }
    pp.chain = throughput_chain && !materials && max_bounces <= 3 && (uint64_t)scene->stats.instances * (uint64_t)std::max(1, scene->stats.max_submeshes) <= 65536ull;
    const size_t slots = 2 * (size_t)TG.capacity * B;          // the combined queue [next-bounce rays | shadow rays] of a bounce
    pp.rpw_p = stream_rays_per_wave((size_t)TG.capacity * B); pp.rpw_m = stream_rays_per_wave(slots);
    // shadow planes: contribution per pixel and bounce + one byte per shadow ray that got through, instead of the contribution queue and the read-modify-write of the sample buffer
    pp.planes = shadow_planes != 0 && pp.chain && pp.on_wide && !materials && max_bounces <= PLANES_MAX_BOUNCES && !ablate_mask();
    // two-level scenes: the binned walk (TLAS pass + BLAS pass over (ray, instance) pairs) for the bounce / shadow rays of planes passes
    pp.pairs = two_level && pp.planes && tl_pairs != 0 && sv.tri_packet != nullptr;
    pp.pair_cap = 2 * (size_t)capacity * (size_t)std::max(1, alloc_batch);          // one pair per virtual ray of the combined queue; a push beyond it walks its instance in place
    // few instances: the TLAS pass has no tree (every lane visits every instance: nothing diverges; two_level_passes.h k_tl_top_flat)
    pp.tl_flat = pp.pairs && sv.num_inst <= TL_FLAT_MAX_INSTANCES && tl_pairs != 2;
    pp.pair_cap_used = (uint32_t)std::min<size_t>(tl_pair_cap > 0 ? std::min<size_t>((size_t)tl_pair_cap, pp.pair_cap) : pp.pair_cap, 0xFFFFFFFFu);
    // the primary trace inside shade(0): flattened scenes, planes passes
    // (not for one frame alone on the chip, fuse_primary = 1: there the primary kernel's 48 registers and 64-thread workgroups fill the chip better than shade's 76 and 256 — 1.71 against 1.81 ms;
    // fuse_primary = 2 fuses always)
    // which layout the primary rays of a flattened scene walk: the 8-wide one when the scene has it (primary_wide = 2, default: one ray per lane inside shade(0) or in its own launch;
    // = 1: the stream kernel with lane refill, A/B), the rope layout otherwise — or on request (primary_wide = 0; needs scene option rope = 1)
    pp.prim_rope = !two_level && (!sv.num_wnodes || primary_wide == 0);
    if (pp.prim_rope && sv.num_nodes == 0 && sv.num_tris != 0) { set_error("primary_wide = 0 walks the rope layout: commit the scene with scene option rope = 1"); return MRT_ERR_STATE; }
    if (!pp.on_wide && !two_level && sv.num_nodes == 0 && sv.num_tris != 0) { set_error("wide_bounce = 0 walks the rope layout: commit the scene with scene option rope = 1"); return MRT_ERR_STATE; }
    pp.trace0_pass = pp.planes && fuse_primary != 0 && primary_wide != 1 && !(two_level && primary_wide == 0) && (fuse_primary == 2 || dp.lanes > 1 || B > 1 || two_level);      // (two-level scenes always: their own-launch form is the stream kernel, 0.88 ms for one 1080p frame of dragon x 4)
    pp.trace0_wide = pp.trace0_pass && !pp.prim_rope;          // (planes implies the 8-wide layout)
    // the hint of two-level scenes is (packet | instance << 24): scenes of at most 255 instances and 2^24 packets
    pp.trace0_hint = primary_hint && (!two_level || (sv.num_inst <= 255u && scene->wpackets.n / WPK < ((size_t)1 << 24)));
    pp.primary = ((ablate_mask() & 1) || pp.trace0_pass) ? PrimaryForm::none
               : ((two_level && pp.on_wide) || (primary_wide == 1 && sv.num_wnodes && !two_level)) ? PrimaryForm::stream
               : (two_level || pp.prim_rope) ? PrimaryForm::rope : PrimaryForm::lane_wide;
    pp.primary_hinted = pp.trace0_hint && !(two_level && pp.primary == PrimaryForm::rope);          // (k_trace_primary<true> takes no hint)
    pp.bundle = frame_bundle && pp.trace0_wide && B > 1;
    // entries per packing workgroup: SHADE_PACK_RANGE when the queue is long, less when that would leave fewer than ~2048 workgroups (a one-frame pass, a tile group, a shard) — never less than two rounds' worth
    pp.pack_range = (uint32_t)std::min<size_t>(SHADE_PACK_RANGE, std::max<size_t>(2 * SHADE_THREADS, (size_t)TG.capacity * B / 2048 / SHADE_THREADS * SHADE_THREADS));
    // persistent = 2 (auto): pull chunks when every wave slot would otherwise own >= 1024 rays (4-frame passes at 1080p: +7...+11 % with
    // one stream, +2.5 % with 12); one-frame launches keep the static split (384 rays per wave, no atomics: 3 frames in flight 6.5 vs 5.4 Grays/s)
    // [r3] smaller launches pull as well when five or more passes are in flight (6 lanes x one-frame passes: 9.33 against 8.76 Grays/s; a rank of eight over 240 frames
    // in 8-frame passes: 9.43 against 8.56); with one to three passes in flight they do better on the even static split (one frame alone 1.51 against 1.76 ms, 3 x 1 frame
    // 7.63 against 7.20 Grays/s, a rank of eight over the driver's 20 frames 6.65 against 5.73): stream_even below
    pp.pull = persistent == 1 || (persistent == 2 && (slots >= (size_t)pp.wave_slots * 1024 || (std::min(dp.lanes, dp.G > 1 ? dp.Fp * dp.G : dp.n_passes) >= 5 && slots >= (size_t)pp.wave_slots * 256)));      // (below 256 slots per wave slot — Cornell 256^2 in 8-frame passes — the even split: 6.46 against 5.40 Grays/s)
    const bool takes_x = !two_level && pp.planes && hit_lds;          // the kernels with the hit words in LDS; k_trace_mixed_wide_stream_x is also the one kernel that deals batches round-robin (BatchStride)
    pp.trace = pp.pairs ? TraceForm::pairs : !pp.on_wide ? TraceForm::rope : pp.pull ? (takes_x ? TraceForm::pull_x : TraceForm::pull) : (takes_x ? TraceForm::static_x : TraceForm::static_split);
    pp.trace_lds = pp.trace == TraceForm::rope ? 0 : pp.stack_bytes + (takes_x ? (size_t)HIT_LDS_WORDS * 4 : 0);
    // segmented queues: the default pass only — shade(0) as one row of bundled k_shade_primary<2> blocks, packed shades, the pulling launch with hit words in LDS and per-XCD
    // counters (flattened scene, planes, chain) — and only when eight segments fit the lane's queues (segment_sizing); every other pass keeps one queue and one word
    pp.segs = 1; pp.seg_cap = 0;
    if (queue_segments == (int)QUEUE_SEGMENTS && pp.trace == TraceForm::pull_x && pp.trace0_wide && !two_level && pp.bundle && shade_pack && pp.chain && xcd_counters && max_bounces <= 3) {
        const SegmentSizing z = segment_sizing(TG.capacity, B);
        const uint64_t all = (uint64_t)QUEUE_SEGMENTS * z.seg_cap;
        if (all <= (uint64_t)queue_entries(capacity, alloc_batch) && all < (uint64_t)SEG_SHADOW_BIT) { pp.segs = (int)QUEUE_SEGMENTS; pp.seg_cap = (uint32_t)z.seg_cap; }
    }
#ifdef MRT_PROBE_SHADE_TAILS
    if (probe_tails_mask()) { pp.segs = 1; pp.seg_cap = 0; }          // the probe times the one-queue form
#endif
    if (pp.trace == TraceForm::pairs) pp.pg = pull_grid(slots, (size_t)pp.wave_slots, 64, dp.long_call);
    else if (pp.trace == TraceForm::pull) pp.pg = pull_grid(slots, (size_t)pp.wave_slots, 128, dp.long_call);
    else if (pp.trace == TraceForm::pull_x) {
        // the variant with the hit words in LDS: its own LDS size, hence its own count of wave slots
        // (the instantiation this pass launches: pp.segs is decided above)
        SlotCache &xc = pp.segs > 1 ? persist_xs_cache : persist_x_cache;
        if (int rc = pp.segs > 1 ? wave_slots_for(k_trace_mixed_wide_persist_x<true>, pp.trace_lds, xc, cu_count) : wave_slots_for(k_trace_mixed_wide_persist_x<false>, pp.trace_lds, xc, cu_count)) return rc;
        if (xc.per_cu < 1) { set_error("hit_lds: the traversal kernel does not fit a compute unit with " + std::to_string(pp.trace_lds) + " bytes of LDS"); return MRT_ERR_UNSUPPORTED; }
        pp.pg = pull_grid(slots, wave_slots_user ? (size_t)pp.wave_slots : (size_t)(xc.per_cu * cu_count), 128, dp.long_call);
    }
    else if (pp.trace != TraceForm::rope) {
        // a shard's launches (a rank of eight over the driver's 20 frames: three passes of its 1/8 of the tiles in flight) do better with ONE round of waves that take the queue's
        // 64-ray batches round-robin — every rank of eight timed: 2.00 against 2.21 ms on average, the slowest 2.13-2.18 against 2.46-2.50 (profiles/r05_shard_stride.txt); a whole
        // image's one-frame launches do not (one frame alone 1.38 = 1.38 ms, three in flight 0.775 against 0.765)
        const bool shard_auto = stream_stride == 2 && stream_even == 200 && shard_world > 1 && dp.G == 1 && takes_x;          // (one round of waves was measured with the strided deal only)
        pp.strided = stream_stride == 1 || shard_auto;
        const int even_pct = shard_auto ? 100 : stream_even;
        pp.even = even_pct > 0 ? (uint32_t)std::max<size_t>(1, std::min<size_t>(cdiv(slots, 64), (size_t)pp.wave_slots * (size_t)even_pct / 100)) : 0u;     // stream_even: percent of the wave slots
        pp.static_grid = pp.even ? pp.even : cdiv(slots, pp.rpw_m);
    }
    return MRT_OK;
}

// a shard that owns no tile (more ranks than 8 x 8 tiles: rank 2 of 3 of a 9 x 5 image) has no pixel to render and its buffers stay 0; the launches sized
// by its queues would be empty grids (the shading of bounces >= 1: cdiv(capacity x batch, ...) = 0), which HIP refuses.  The frames count as drawn.
int Renderer::draw_nothing(int n_frames) {
    if (guides) { if (int rc = ensure_guides()) return rc; guides_valid = true; }
    MRT_HIP(hipEventRecord(ev_begin, stream));
    frame_index += (uint32_t)n_frames; frames_rendered += (uint64_t)n_frames;
    ext_used = 0;
    if (int rc = note_pass(stream)) return rc;
    MRT_HIP(hipEventRecord(ev_end, stream));
    pending_timing = true;
    return MRT_OK;
}

// the frame_batch option (or the shard, under frame_batch = 0) changed since the buffers were sized: size them again; image, frame count, totals and guides survive
int Renderer::rebuild_for_batch() {
    MRT_HIP(hipStreamSynchronize(stream));
    const uint32_t keep_frame = frame_index; const int keep_cur = cur; const uint64_t keep_rendered = frames_rendered;
    DevBuf<float4> keep; MRT_HIP(keep.alloc(accum[cur].n));
    MRT_HIP(hipMemcpyAsync(keep.p, accum[cur].p, accum[cur].bytes(), hipMemcpyDeviceToDevice, stream));
    const MRTCamera keep_cam = camera;
    unsigned long long keep_totals[3] = {0, 0, 0};
    MRT_HIP(hipMemcpy(keep_totals, totals.p, sizeof keep_totals, hipMemcpyDeviceToHost));
    const bool keep_denoised = denoised_valid;
    guides_keep = true;
    int rc = resize(width, height);
    guides_keep = false; denoised_valid = keep_denoised;
    if (rc) return rc;
    MRT_HIP(hipMemcpyAsync(totals.p, keep_totals, sizeof keep_totals, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(accum[keep_cur].p, keep.p, keep.bytes(), hipMemcpyDeviceToDevice, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    frame_index = keep_frame; cur = keep_cur; frames_rendered = keep_rendered; frames_completed_known = keep_rendered; camera = keep_cam;
    return MRT_OK;
}

// the first draw sizes the lanes in use.  A lane's queues take ~163 B x pixels x frame_batch (1080p, 8-frame passes: 2.7 GB); when the
// device cannot hold all the lanes asked for, the renderer runs on the ones it got (>= 1) instead of failing in the middle of a draw
int Renderer::ensure_lanes(int want) {
    for (; lanes_ready < want; lanes_ready++) {
        const size_t need = lane_bytes() + (lanes_ready == 0 && !halton_tab.p ? (size_t)HALTON_TAB_DIMS * HALTON_TAB_SPAN * sizeof(float) : 0);      // (+ the renderer's one Halton table, allocated at its first bundled draw)
        size_t free_b = 0, total_b = 0;
        const bool fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b > need + (size_t(1) << 30);      // keep 1 GiB of slack for the caller
        int rc = fits ? alloc_lane(lanes[lanes_ready]) : MRT_ERR_OUT_OF_MEMORY;
        if (rc == MRT_ERR_OUT_OF_MEMORY && lanes_ready >= 1) { (void)hipGetLastError(); release_lane(lanes[lanes_ready]); break; }
        if (rc == MRT_ERR_OUT_OF_MEMORY) { set_error("not enough device memory for one pass in flight: " + std::to_string(need >> 20) + " MiB of ray queues needed (" + std::to_string(width) + "x" + std::to_string(height) + ", frame_batch " + std::to_string(alloc_batch) + "); lower frame_batch"); return rc; }
        if (rc) return rc;
    }
    return MRT_OK;
}

// the draw's uniforms on the renderer's own shard (updateUniforms :216-229), and the guide launch's: the call's first frame
void Renderer::begin_draw(DrawCtx &d) const {
    FrameParams &fp = d.fp;
    fp = FrameParams{};
    fp.width = width; fp.height = height; fp.lightCount = light_count_limit > 0 ? std::min(light_count_limit, d.sv.light_count) : d.sv.light_count;
    fp.cam_pos = make_float4(camera.position.x, camera.position.y, camera.position.z, 0);
    fp.cam_right = make_float4(camera.right.x, camera.right.y, camera.right.z, 0);
    fp.cam_up = make_float4(camera.up.x, camera.up.y, camera.up.z, 0);
    fp.cam_fwd = make_float4(camera.forward.x, camera.forward.y, camera.forward.z, 0);
    fp.shard_rank = shard_rank; fp.shard_world = shard_world;
    fp.tiles_x = (width + 7) / 8; fp.tiles_local = tiles_local; fp.max_bounces = max_bounces;
    d.gp = fp;
    d.gp.frameIndex = frame_index; d.gp.sampleIndex = frame_index + sample_offset; d.gp.npix = (uint32_t)((size_t)width * height); d.gp.capacity = capacity; d.gp.batch = 1;
    fp.npix = (uint32_t)((size_t)width * height); fp.capacity = capacity;
    d.last_acc = nullptr;
    for (hipEvent_t &e : d.last_acc_g) e = nullptr;
    d.tail.n = 0;
}

// the buffers that only some passes need, allocated by the first such pass on the lane (a lane's buffers are sized for the renderer's whole shard, whatever tile group uses it now)
int Renderer::prepare_lane(FrameLane &L, const TileGroup &TG, const PassPlan &pp) {
    const size_t shard_qcap = (size_t)capacity * (size_t)std::max(1, alloc_batch);
    if (!pp.chain && !L.thr[0].p) {           // this draw needs the throughput queues after all (materials, more than three bounces, a very large resource table)
        for (int k = 0; k < 2; k++) MRT_HIP(L.thr[k].alloc(shard_qcap));
    }
    if (pp.planes) {
        if (!L.f_lit.p) { if (int rc = alloc_planes(L)) return rc; }
        MRT_HIP(hipMemsetAsync(L.f_lit.p, 0, 4 * (size_t)TG.capacity * (size_t)pp.B, L.stream));
    }
    if (pp.pairs && !L.pairs.p) MRT_HIP(L.pairs.alloc(std::max<size_t>(PairQueue::WORDS * pp.pair_cap, 1)));
    if (!pp.planes && !L.scon.p) MRT_HIP(L.scon.alloc(shard_qcap));
    return MRT_OK;
}

// one launch per frame on the pass's stream; frames are sequential (a path's last act is the running average with the previous target)
int Renderer::enqueue_megakernel_pass(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp) {
    FrameParams &fp = d.fp;
    uint32_t *work = reinterpret_cast<uint32_t *>(L.bounce_counts.p + 64);      // its own word: the pipeline's per-bounce work counters must stay zero between passes
    for (int sub = 0; sub < pp.B; sub++) {
        fp.frameIndex = frame_index + (uint32_t)sub; fp.sampleIndex = frame_index + (uint32_t)sub + sample_offset; fp.batch = 1;
        if (d.last_acc) { MRT_HIP(hipStreamWaitEvent(L.stream, d.last_acc, 0)); d.last_acc = nullptr; }
        MRT_HIP(hipMemsetAsync(work, 0, 4, L.stream));
        launch_timed(timed(MRT_KERNEL_TRACE), k_megakernel, dim3(pp.mega_waves), dim3(64), pp.stack_bytes, L.stream, d.sv, fp, TG.seeds, accum[cur].p, accum[1 - cur].p, work, totals.p, (uint32_t)TG.owned);
        cur = 1 - cur;
    }
    MRT_HIP(hipEventRecord(L.accumulated, L.stream));
    d.last_acc = L.accumulated;
    frame_index += (uint32_t)pp.B; frames_rendered += (uint64_t)pp.B;
    return note_pass(L.stream);
}

// the primary rays in a launch of their own (PrimaryForm::none: shade(0) traces them)
void Renderer::enqueue_primary(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp) {
    if (pp.primary == PrimaryForm::none) return;
    float4 *const dirs = L.rayB[1].p;
    uint32_t *const hint_p = pp.primary_hinted ? hint.p : nullptr;
    if (pp.primary == PrimaryForm::stream) {
        const auto kernel = pp.two_level ? (pp.primary_hinted ? k_trace_primary_wide_stream<true, true> : k_trace_primary_wide_stream<true, false>)
                                         : (pp.primary_hinted ? k_trace_primary_wide_stream<false, true> : k_trace_primary_wide_stream<false, false>);
        launch_timed(timed(MRT_KERNEL_PRIMARY), kernel, dim3(cdiv(TG.capacity, pp.rpw_p), pp.B), dim3(64), pp.stack_bytes, L.stream, d.sv, d.fp, TG.seeds, L.hits.p, dirs, TG.capacity, pp.rpw_p, hint_p);
        return;
    }
    const bool lane_wide = pp.primary == PrimaryForm::lane_wide;
    auto kernel = k_trace_primary<true>;
    if (!pp.two_level) kernel = lane_wide ? k_trace_primary<false, true> : k_trace_primary<false>;
    launch_timed(timed(MRT_KERNEL_PRIMARY), kernel, dim3(pp.grid_tiles, pp.B), dim3(64), lane_wide ? pp.stack_bytes : 0, L.stream, d.sv, d.fp, TG.seeds, L.hits.p, dirs, hint_p);
}

using ShadeKernel = void (*)(SceneView, FrameParams, const uint32_t *, const float4 *, const float4 *, const float4 *, const float4 *, const unsigned long long *, uint32_t, float4 *, float4 *, float4 *, float4 *, float4 *, float4 *,
                             unsigned long long *, float4 *, float4 *, uint32_t *);
static ShadeKernel shade_kernel_for(const PassPlan &pp, bool materials, bool pack, int b) {
    if (pack) return materials ? (ShadeKernel)k_shade_pack<true, false, false, false>
                   : pp.pairs ? (ShadeKernel)k_shade_pack<false, true, true, true>
                   : pp.planes ? (ShadeKernel)k_shade_pack<false, true, true, false>
                   : pp.chain ? (ShadeKernel)k_shade_pack<false, true, false, false> : (ShadeKernel)k_shade_pack<false, false, false, false>;
    return materials ? (ShadeKernel)k_shade<true, false, false, false>
         : (pp.pairs && b > 0) ? (ShadeKernel)k_shade<false, true, true, true>
         : (pp.trace0_wide && b == 0 && pp.two_level) ? (ShadeKernel)k_shade_primary<3>
         : (pp.trace0_wide && b == 0) ? (ShadeKernel)k_shade_primary<2>
         : (pp.trace0_pass && b == 0) ? (ShadeKernel)k_shade_primary<1>
         : pp.planes ? (ShadeKernel)k_shade<false, true, true, false>
         : pp.chain ? (ShadeKernel)k_shade<false, true, false, false> : (ShadeKernel)k_shade<false, false, false, false>;
}

// shade(b) reads the queue shade(b - 1) wrote (b & 1 ^ 1) and writes next rays into queue b & 1
void Renderer::enqueue_shade(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp, int b) {
    FrameParams &fp = d.fp;
    const int q = b & 1, B = pp.B;
    unsigned long long *const bc = L.bounce_counts.p;                     // [bounce] {next rays (lo), shadow rays (hi)}, zero at frame start
    fp.bounce = b;
    // bounce 0 reads no ray queue (it regenerates the primary ray); bounce b > 0 reads the queue shade(b-1) wrote
    // bounce 0: one grid row per sub-frame of the batch over the primary slots; later bounces: the compact queue of the whole batch
    const bool pack = shade_pack && b > 0;          // bounces >= 1 read a queue half of whose rays missed: its hits are compacted in LDS and shaded on full waves (k_shade_pack)
    fp.pack_range = pp.pack_range;
    const bool seg = pp.segs > 1;
    fp.segs = (uint32_t)pp.segs; fp.seg_cap = pp.seg_cap;
    fp.frame_bundle = (pp.bundle && b == 0) ? 1 : 0;
    if (fp.frame_bundle) {
        fp.bundle_groups = ((uint32_t)B + 7u) / 8u; fp.bundle_w = ((uint32_t)B + fp.bundle_groups - 1u) / fp.bundle_groups;
        fp.bundle_per_wave = 64u / fp.bundle_w; fp.bundle_magic = (65536u + fp.bundle_w - 1u) / fp.bundle_w;
    }
    fp.halton_tab = nullptr; fp.halton_w0 = 0; fp.halton_n = 0;
    if (fp.frame_bundle && fp.bundle_w >= 4u && halton_table && halton_tab.p) {          // a wave reads bundle_w consecutive values per load: the table pays from four on (indices outside its window: the recurrence)
        fp.halton_tab = halton_tab.p; fp.halton_w0 = halton_w0; fp.halton_n = HALTON_TAB_SPAN;
    }
    const dim3 gs = b == 0 ? (fp.frame_bundle ? dim3(cdiv(cdiv((size_t)TG.capacity * fp.bundle_groups, fp.bundle_per_wave) * 64, SHADE_THREADS), 1) : dim3(pp.grid_shade, B)) : (seg && pack) ? dim3(QUEUE_SEGMENTS * cdiv(pp.seg_cap, fp.pack_range)) : dim3(cdiv((size_t)TG.capacity * B, pack ? fp.pack_range : (uint32_t)SHADE_THREADS));
    float4 *const con_b = !pp.planes ? L.scon.p : b == 0 ? L.sample.p : L.f_con[b - 1].p;         // PLANES: this bounce's contribution plane in place of the queue
    const size_t shade_lds = (pp.trace0_wide && b == 0) ? (size_t)SHADE_WAVES * (scene->wide_depth * WIDE_STACK_LEVEL_BYTES + (MRT_LANE_HIT_LDS ? 1024 : 0)) : 0;
    // (segmented pass: segment 0's tail word of the bounce read and of the bounce written; pp.segs > 1 implies packed shades)
    unsigned long long *count_out = seg ? bc + SEG_TAILS + (size_t)b * SEG_TAILS_PER_BOUNCE : bc + b;
    const unsigned long long *const count_in = b == 0 ? nullptr : seg ? bc + SEG_TAILS + (size_t)(b - 1) * SEG_TAILS_PER_BOUNCE : bc + (b - 1);
#ifdef MRT_PROBE_SHADE_TAILS
    fp.probe_tails = (probe_tails_mask() >> b) & 1;
    if (fp.probe_tails) {
        count_out = bc + SEG_TAILS + 32 * SEG_TAILS_PER_BOUNCE + (size_t)b * 8 * 16;
        // MRT_PROBE_DISJOINT=1: word x starts at x * seg_cap in both halves, seg_cap = what the blocks of one word can emit together — eight disjoint segments, the full write
        // footprint of the real queues (overlapping segments write one eighth of it); alloc_lane's probe slack holds the rounding
        const uint32_t per_block = pack ? fp.pack_range : (uint32_t)SHADE_THREADS, seg_cap = (probe_disjoint() && pp.planes && pp.chain && gs.y == 1u) ? cdiv(gs.x, 8u) * per_block : 0u;
        hipLaunchKernelGGL(k_probe_tails_init, dim3(1), dim3(64), 0, L.stream, count_out, seg_cap);
    }
#endif
    // (two-level, binned, b > 0: L.hits holds the 64-bit keys of the TLAS / BLAS passes)
    launch_timed(timed(MRT_KERNEL_SHADE), shade_kernel_for(pp, materials, pack, b), gs, dim3(SHADE_THREADS), shade_lds, L.stream, d.sv, fp, TG.seeds, L.rayA[1 - q].p, L.rayB[1 - q].p, L.thr[1 - q].p, L.hits.p,
                 count_in, TG.capacity, L.rayA[q].p, L.rayB[q].p, L.thr[q].p, L.srayA.p, L.srayB.p, con_b, count_out, b == 0 ? L.sample.p : nullptr, L.sample.p,
                 (b == 0 && pp.trace0_pass && pp.trace0_hint) ? hint.p : nullptr);
}

// the bounce rays and the shadow rays that shade(b) queued, in one traversal launch (pairs: two)
void Renderer::enqueue_trace(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp, int b) {
    if (ablate_mask() & 2) return;
    const int q = b & 1;
    hipStream_t st = L.stream;
    unsigned long long *const bc = L.bounce_counts.p;
    const unsigned long long *const counts = bc + b;
    uint32_t *const work = reinterpret_cast<uint32_t *>(bc + WORK_COUNTERS + (size_t)b * WORK_COUNTERS_PER_BOUNCE);
    uint8_t *const lit_b = pp.planes ? L.f_lit.p + b : nullptr;
    const float4 *const rayA = L.rayA[q].p, *const rayB = L.rayB[q].p, *const srayA = L.srayA.p, *const srayB = L.srayB.p;
    const uint32_t xcd_frames = xcd_counters ? (uint32_t)pp.B : 0u;
    switch (pp.trace) {
    case TraceForm::pairs: {
        unsigned long long *const keys = reinterpret_cast<unsigned long long *>(L.hits.p);
        uint32_t *const pc = reinterpret_cast<uint32_t *>(bc + 65 + b);          // two-level, binned: {pairs queued, work counter of the BLAS pass}
        const uint32_t stack_words = (uint32_t)(pp.stack_bytes / 4);
        // few instances: the TLAS pass without a tree; many: the stream walk of the 8-wide TLAS
        if (pp.tl_flat) launch_timed(timed(MRT_KERNEL_TRACE), k_tl_top_flat, dim3((uint32_t)std::max<size_t>(1, std::min<size_t>(cdiv(2 * (size_t)TG.capacity * pp.B, 64), 2 * pp.pg.grid_slots))), dim3(64), pp.stack_bytes + 8, st, d.sv, rayA, rayB, keys, srayA, srayB,
                                     counts, lit_b, L.pairs.p, pc, pp.pair_cap_used, stack_words);
        else launch_timed(timed(MRT_KERNEL_TRACE), k_tl_top, dim3(pp.pg.waves), dim3(64), pp.stack_bytes + 8, st, d.sv, rayA, rayB, keys, srayA, srayB,
                          counts, reinterpret_cast<uint32_t *>(bc + 32 + b), pp.pg.chunk, lit_b, L.pairs.p, pc, pp.pair_cap_used, stack_words);
        // the pairs' count is on the device: the launch has the wave slots it may use and the surplus leaves at once
        launch_timed(timed(MRT_KERNEL_TRACE), k_tl_blas, dim3((uint32_t)pp.pg.grid_slots), dim3(64), (size_t)scene->wide_depth * WIDE_STACK_LEVEL_BYTES, st, d.sv, rayA, rayB, keys, srayA, srayB,
                     counts, pc + 1, 256u, lit_b, (const uint4 *)L.pairs.p, (const uint32_t *)pc, pp.pair_cap_used);
        break;
    }
    case TraceForm::pull_x:
        if (pp.segs > 1) launch_timed(timed(MRT_KERNEL_TRACE), k_trace_mixed_wide_persist_x<true>, dim3(pp.pg.waves), dim3(64), pp.trace_lds, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB,
                                      (const unsigned long long *)(bc + SEG_TAILS + (size_t)b * SEG_TAILS_PER_BOUNCE), work, pp.pg.chunk, lit_b, pp.seg_cap);
        else launch_timed(timed(MRT_KERNEL_TRACE), k_trace_mixed_wide_persist_x<false>, dim3(pp.pg.waves), dim3(64), pp.trace_lds, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB, counts, work, pp.pg.chunk, lit_b, xcd_frames);
        break;
    case TraceForm::pull:
        launch_timed(timed(MRT_KERNEL_TRACE), pp.two_level ? k_trace_mixed_wide_persist<true> : k_trace_mixed_wide_persist<false>, dim3(pp.pg.waves), dim3(64), pp.trace_lds, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB, L.scon.p,
                     counts, L.sample.p, work, tag_bounce(pp.pg.chunk, b), lit_b, xcd_frames);
        break;
    case TraceForm::static_x:
        launch_timed(timed(MRT_KERNEL_TRACE), k_trace_mixed_wide_stream_x, dim3(pp.static_grid), dim3(64), pp.trace_lds, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB, counts, tag_bounce(pp.rpw_m, b), lit_b, pp.even | (pp.strided ? 0x80000000u : 0u));
        break;
    case TraceForm::static_split:
        launch_timed(timed(MRT_KERNEL_TRACE), pp.two_level ? k_trace_mixed_wide_stream<true> : k_trace_mixed_wide_stream<false>, dim3(pp.static_grid), dim3(64), pp.trace_lds, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB, L.scon.p,
                     counts, L.sample.p, pp.rpw_m, lit_b, pp.even);
        break;
    case TraceForm::rope:
        launch_timed(timed(MRT_KERNEL_TRACE), pp.two_level ? k_trace_mixed<true> : k_trace_mixed<false>, dim3(2 * pp.grid_tiles * (uint32_t)pp.B), dim3(64), 0, st, d.sv, rayA, rayB, L.hits.p, srayA, srayB, L.scon.p, counts, L.sample.p);
        break;
    }
}

// accumulation is the only frame-to-frame dependency (prev target = the previous frame's output)
int Renderer::enqueue_accumulate(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp, int pass, int g) {
    const int B = pp.B;
    hipStream_t st = L.stream;
    unsigned long long *const bc = L.bounce_counts.p;
    const uint32_t primary = (uint32_t)(TG.owned * (uint64_t)B);
    if (pp.planes && pass >= d.dp.tail_from && d.tail.n < MAX_FRAMES_IN_FLIGHT) {          // deferred: with the draw's other last passes, after the join
        AccPass &P = d.tail.p[d.tail.n++];
        P.con0 = L.sample.p; P.con1 = L.f_con[0].p; P.con2 = L.f_con[1].p; P.lit = L.f_lit.p; P.counts = bc; P.frameIndex = d.fp.frameIndex; P.batch = B; P.primary = primary; P.pad = 0;
        MRT_HIP(hipEventRecord(L.accumulated, st));       // (here: traced — the join below waits for it, the accumulation follows on the main stream)
        frame_index += (uint32_t)B; frames_rendered += (uint64_t)B;
        return MRT_OK;
    }
    const bool grouped = d.dp.G > 1;
    if (grouped) { if (d.last_acc_g[g] && d.last_acc_g[g] != L.accumulated) MRT_HIP(hipStreamWaitEvent(st, d.last_acc_g[g], 0)); }      // this group's pixels of the previous target: written by the same group of the pass before
    else if (d.last_acc) MRT_HIP(hipStreamWaitEvent(st, d.last_acc, 0));
    if (pp.planes) launch_timed(timed(MRT_KERNEL_ACCUMULATE), k_accumulate_planes, dim3(pp.grid_tiles), dim3(64), 0, st, d.fp, L.sample.p, L.f_con[0].p, L.f_con[1].p, L.f_lit.p, accum[cur].p, accum[1 - cur].p, bc, totals.p, primary);
    else launch_timed(timed(MRT_KERNEL_ACCUMULATE), k_accumulate, dim3(pp.grid_tiles), dim3(64), 0, st, d.fp, L.sample.p, accum[cur].p, accum[1 - cur].p, bc, totals.p, primary);
    MRT_HIP(hipEventRecord(L.accumulated, st));
    if (grouped) { d.last_acc_g[g] = L.accumulated; return MRT_OK; }          // (render() swaps the targets and counts the frames once every group of the pass is enqueued)
    d.last_acc = L.accumulated;
    cur = 1 - cur;                                                  // ping-pong swap :332-334 (once per batch: the batch's frames are applied in one kernel)
    frame_index += (uint32_t)B; frames_rendered += (uint64_t)B;
    return note_pass(st);
}

// one pass of pp.B frames over the tiles of TG (G = 1: the renderer's own shard) on lane L
int Renderer::enqueue_pass(DrawCtx &d, FrameLane &L, const TileGroup &TG, const PassPlan &pp, int pass, int g) {
    FrameParams &fp = d.fp;
    fp.batch = pp.B;
    fp.frameIndex = frame_index;                                    // updateUniforms :216-229 (first frame of the batch)
    fp.sampleIndex = frame_index + sample_offset;
    fp.shard_rank = TG.rank; fp.shard_world = TG.world; fp.tiles_local = TG.tiles_local; fp.capacity = TG.capacity;
    if (d.dp.mega) return enqueue_megakernel_pass(d, L, TG, pp);
    if (int rc = prepare_lane(L, TG, pp)) return rc;
    fp.bounce = 0; fp.chain = pp.chain ? 1 : 0;
    fp.wide_stack_words = (uint32_t)((size_t)scene->wide_depth * WIDE_STACK_LEVEL_BYTES / 4);
    enqueue_primary(d, L, TG, pp);
    for (int b = 0; b < max_bounces; b++) { enqueue_shade(d, L, TG, pp, b); enqueue_trace(d, L, TG, pp, b); }
    return enqueue_accumulate(d, L, TG, pp, pass, g);
}

// one launch over this renderer's own pixels and all the call's frames, on a stream of its own beside the passes just enqueued; joined like a lane
int Renderer::enqueue_guides(DrawCtx &d) {
    const bool two_level = d.sv.num_inst > 0;
    const size_t lds = d.sv.num_wnodes ? (size_t)scene->wide_depth * WIDE_STACK_LEVEL_BYTES : 0;
    const auto kernel = two_level ? (d.sv.num_wnodes ? k_guides<3> : k_guides<0>) : (d.sv.num_wnodes ? k_guides<2> : k_guides<1>);
    hipLaunchKernelGGL(kernel, dim3(std::max<uint32_t>(1u, (uint32_t)tiles_local)), dim3(64), lds, guide_stream, d.sv, d.gp, (const uint32_t *)seeds.p, (uint32_t)d.dp.n_frames, guide_nd.p, guide_albedo.p, guide_ids.p);
    const hipError_t le = hipGetLastError();
    // the join comes whatever the launch said: nothing on this stream outlives the call unjoined
    (void)hipEventRecord(guide_done, guide_stream);
    (void)hipStreamWaitEvent(stream, guide_done, 0);
    if (le != hipSuccess) return hip_fail(le, "k_guides launch", __FILE__, __LINE__);
    guides_valid = true;
    return MRT_OK;
}

int Renderer::render(int n_frames) {
    if (!scene) { set_error("renderer has no scene"); return MRT_ERR_STATE; }
    DrawCtx d;
    d.sv = scene->view();
    if (d.sv.light_count < 1) { set_error("scene has no lights (lightCount must be >= 1, Raytracing.metal:273)"); return MRT_ERR_STATE; }
    if (tiles_local == 0) return draw_nothing(n_frames);
    if (alloc_batch != batch_wanted()) { if (int rc = rebuild_for_batch()) return rc; return render(n_frames); }
    // decide: the passes, the lanes the device has memory for, and what each pass launches.  All passes but the last have the size of the first, so two rows of plans
    // serve the draw.  What a draw can be refused for is found here: nothing is enqueued and no lane forked yet
    DrawPlan &dp = d.dp;
    dp = plan_draw(n_frames);
    if (int rc = ensure_lanes(dp.lanes)) return rc;
    dp.settle(lanes_ready);
    lanes_used = dp.lanes; groups_used = dp.G;
    if (dp.G > 1) { if (int rc = ensure_tile_groups(dp.G)) return rc; }
    const TileGroup self_group{shard_rank, shard_world, tiles_local, capacity, owned_pixels, seeds.p};
    PassPlan plans[2][MAX_TILE_GROUPS];
    for (int k = 0; k < 2; k++)
        for (int g = 0; g < dp.G; g++) { if (int rc = plan_pass(dp, d.sv, dp.G > 1 ? tgroups[g] : self_group, dp.pass_size(k == 0 ? 0 : dp.n_passes - 1), plans[k][g])) return rc; }
    wave_slots = plans[0][0].wave_slots;          // (the option reads back what the grids were sized for)
    segments_used = plans[0][0].segs;
    begin_draw(d);
    ext_used = 0;
    if (halton_table && frame_bundle && !megakernel && n_frames > 1) { if (int rc = ensure_halton_table(frame_index + sample_offset, (uint32_t)n_frames)) return rc; }      // (ahead of the fork: see there)
    MRT_HIP(hipEventRecord(ev_begin, stream));
    // fork: every lane starts after whatever the caller queued on the main stream (resize, camera, ...)
    MRT_HIP(hipEventRecord(ev_fork, stream));
    for (int k = 0; k < dp.lanes; k++) MRT_HIP(hipStreamWaitEvent(lanes[k].stream, ev_fork, 0));
    // the guide buffers of the call's frames (guides.h): what can fail on the host happens here, the launch follows the pass loop — no error return of the
    // loop leaves a guide kernel in flight that the main stream has not joined
    if (guides) {
        if (int rc = ensure_guides()) return rc;
        MRT_HIP(hipEventRecord(guide_fork, stream));       // the guide stream starts behind whatever the caller queued on the main stream (the clears of ensure_guides included), not behind the passes
        MRT_HIP(hipStreamWaitEvent(guide_stream, guide_fork, 0));
    }
    for (int pass = 0; pass < dp.n_passes; pass++) {
        const int B = dp.pass_size(pass);
        for (int g = 0; g < dp.G; g++) {
            const TileGroup &TG = dp.G > 1 ? tgroups[g] : self_group;
            if (dp.G > 1 && TG.capacity == 0) continue;
            FrameLane &L = lanes[dp.G > 1 ? (pass % dp.Fp) * dp.G + g : pass % dp.lanes];
            if (int rc = enqueue_pass(d, L, TG, plans[B == plans[0][g].B ? 0 : 1][g], pass, g)) return rc;
        }
        if (dp.G > 1) { cur = 1 - cur; frame_index += (uint32_t)B; frames_rendered += (uint64_t)B; }      // every group read accum[cur] and wrote accum[1 - cur] at its own pixels
    }
    // join: the main stream continues after every lane has drained
    for (int k = 0; k < (dp.G > 1 ? std::min(dp.Fp, dp.n_passes) * dp.G : std::min(dp.lanes, dp.n_passes)); k++) MRT_HIP(hipStreamWaitEvent(stream, lanes[k].accumulated, 0));
    if (guides) { if (int rc = enqueue_guides(d)) return rc; }
    if (dp.G > 1) { if (int rc = note_pass(stream)) return rc; }      // (tile groups: completion is reported per draw)
    if (d.tail.n > 0) {          // the draw's last passes, accumulated in one launch over the shard's tiles
        launch_timed(timed(MRT_KERNEL_ACCUMULATE), k_accumulate_planes_group, dim3(std::max<uint32_t>(1u, (uint32_t)tiles_local)), dim3(64), 0, stream, d.fp, d.tail, accum[cur].p, accum[1 - cur].p, totals.p);
        cur = 1 - cur;
        if (int rc = note_pass(stream)) return rc;
    }
    MRT_HIP(hipEventRecord(ev_end, stream));
    MRT_HIP(hipGetLastError());
    pending_timing = true;
    return MRT_OK;
}

int Renderer::wait() {
    MRT_HIP(hipStreamSynchronize(stream));
    if (int rc = check_bounds_record()) return rc;
    { uint64_t done = 0; if (int rc = poll_completed(&done)) return rc; }
    if (pending_timing) {
        float ms = 0;
        MRT_HIP(hipEventElapsedTime(&ms, ev_begin, ev_end));
        ms_last = ms;
        float ext = 0; uint32_t next = 0;
        kernel_times = MRTKernelTimes{};
        for (int k = 0; k < ext_used; k++) {
            float e = 0; MRT_HIP(hipEventElapsedTime(&e, ev_ext[k].a, ev_ext[k].b));
            const int kind = ev_ext[k].kind;
            kernel_times.ms[kind] += e; kernel_times.launches[kind]++;
#ifdef MRT_PROBE_SHADE_TAILS
            if (getenv("MRT_PROBE_LOG")) fprintf(stderr, "probe_launch %d kind %d ms %.5f\n", k, kind, e);
#endif
            if (kind == MRT_KERNEL_PRIMARY || kind == MRT_KERNEL_TRACE) { ext += e; next++; }
        }
        ms_extend_last = ext; extend_launches_last = next;
        pending_timing = false;
    }
    return MRT_OK;
}

int Renderer::read_accum(float *rgba, size_t nbytes) {
    if (nbytes != (size_t)width * height * 16) { set_error("read_accum: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    int rc = wait(); if (rc) return rc;
    MRT_HIP(hipMemcpy(rgba, accum[cur].p, nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}
int Renderer::copy_accum_to_device(void *dptr, size_t nbytes) {
    if (nbytes != (size_t)width * height * 16) { set_error("copy_accum_to_device: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    MRT_HIP(hipMemcpyAsync(dptr, accum[cur].p, nbytes, hipMemcpyDeviceToDevice, stream));
    return MRT_OK;
}
int Renderer::write_accum_from_device(const void *dptr, size_t nbytes) {
    if (nbytes != (size_t)width * height * 16) { set_error("write_accum_from_device: nbytes must be width*height*16"); return MRT_ERR_INVALID_ARGUMENT; }
    MRT_HIP(hipMemcpyAsync(accum[cur].p, dptr, nbytes, hipMemcpyDeviceToDevice, stream));
    return MRT_OK;
}
uint32_t shard_tiles(int width, int height, int rank, int world) {
    const int tiles = ((width + 7) / 8) * ((height + 7) / 8);
    return (uint32_t)std::max(0, (tiles - rank + world - 1) / world);
}
int unpack_tiles_into(float4 *image, int width, int height, const void *compact, size_t nbytes, int rank, int world, hipStream_t st) {
    if (world < 1 || rank < 0 || rank >= world) { set_error("unpack_tiles: invalid shard"); return MRT_ERR_INVALID_ARGUMENT; }
    const uint32_t tl = shard_tiles(width, height, rank, world);
    if (nbytes != (size_t)tl * 64 * sizeof(float4)) { set_error("unpack_tiles: nbytes must be tiles x 64 x 16 for that shard (mrt_renderer_shard_tiles)"); return MRT_ERR_INVALID_ARGUMENT; }
    if (tl) hipLaunchKernelGGL(k_tiles<false>, dim3(cdiv((size_t)tl * 64, 256)), dim3(256), 0, st, image, width, height, (width + 7) / 8, rank, world, tl, (float4 *)const_cast<void *>(compact));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}
int Renderer::pack_owned_tiles(void *dptr, size_t nbytes) {
    const uint32_t tl = shard_tiles(width, height, shard_rank, shard_world);
    if (nbytes != (size_t)tl * 64 * sizeof(float4)) { set_error("pack_owned_tiles: nbytes must be tiles x 64 x 16 for this renderer's shard (mrt_renderer_shard_tiles)"); return MRT_ERR_INVALID_ARGUMENT; }
    if (tl) hipLaunchKernelGGL(k_tiles<true>, dim3(cdiv((size_t)tl * 64, 256)), dim3(256), 0, stream, accum[cur].p, width, height, (width + 7) / 8, shard_rank, shard_world, tl, (float4 *)dptr);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}
int Renderer::unpack_tiles(const void *dptr, size_t nbytes, int rank, int world) { return unpack_tiles_into(accum[cur].p, width, height, dptr, nbytes, rank, world, stream); }
int Renderer::read_tonemapped(uint8_t *rgba, size_t nbytes) {
    if (nbytes != (size_t)width * height * 4) { set_error("read_tonemapped: nbytes must be width*height*4"); return MRT_ERR_INVALID_ARGUMENT; }
    DevBuf<uchar4> tmp; MRT_HIP(tmp.alloc((size_t)width * height));
    hipLaunchKernelGGL(k_tonemap, dim3(cdiv(width, 16), cdiv(height, 16)), dim3(16, 16), 0, stream, accum[cur].p, width, height, tmp.p);
    int rc = wait(); if (rc) return rc;
    MRT_HIP(hipMemcpy(rgba, tmp.p, nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
}

int Renderer::stats(MRTRenderStats *out) {
    int rc = wait(); if (rc) return rc;
    unsigned long long t[4];
    MRT_HIP(hipMemcpy(t, totals.p, sizeof t, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->frames = frames_rendered; out->closest_rays = t[0]; out->shadow_rays = t[1]; out->primary_rays = t[2];
    // 96 B per closest ray, 72 B per shadow ray, 36 B per pixel (20 on frame 0), + one read of the scene per frame
    uint64_t px = owned_pixels;
    uint64_t per_frame_px = px * 36;
    out->bytes_alg = t[0] * 96 + t[1] * 72 + frames_rendered * per_frame_px + frames_rendered * scene->stats.scene_bytes;
    out->ms_gpu_last = ms_last; out->ms_extend_last = ms_extend_last; out->extend_launches_last = extend_launches_last;
    return MRT_OK;
}
int Renderer::reset_stats() {
    MRT_HIP(hipMemsetAsync(totals.p, 0, totals.bytes(), stream));
    MRT_HIP(hipStreamSynchronize(stream));       // frames_completed counts from here: nothing of the old count may still be in flight
    for (auto &pd : passes_pending) pass_events_free.push_back(pd.ev);
    passes_pending.clear(); frames_completed_known = 0;
    frames_rendered = 0;
    return MRT_OK;
}

// ---- device-function probes
int probe_halton(hipStream_t stream, const int32_t *i, const int32_t *d, size_t n, float *out) {
    if (n == 0) return MRT_OK;
    DevBuf<int32_t> di, dd; DevBuf<float> dout;
    MRT_HIP(di.alloc(n)); MRT_HIP(dd.alloc(n)); MRT_HIP(dout.alloc(n));
    MRT_HIP(hipMemcpyAsync(di.p, i, n * 4, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(dd.p, d, n * 4, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_probe_halton, dim3(cdiv(n, 256)), dim3(256), 0, stream, di.p, dd.p, (uint32_t)n, dout.p);
    MRT_HIP(hipMemcpyAsync(out, dout.p, n * 4, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    return MRT_OK;
}
int probe_hemisphere(hipStream_t stream, const float *u2, const float *n3, size_t n, float *out3) {
    if (n == 0) return MRT_OK;
    DevBuf<float> du, dn, dout;
    MRT_HIP(du.alloc(2 * n)); MRT_HIP(dn.alloc(3 * n)); MRT_HIP(dout.alloc(3 * n));
    MRT_HIP(hipMemcpyAsync(du.p, u2, n * 8, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(dn.p, n3, n * 12, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_probe_hemisphere, dim3(cdiv(n, 256)), dim3(256), 0, stream, du.p, dn.p, (uint32_t)n, dout.p);
    MRT_HIP(hipMemcpyAsync(out3, dout.p, n * 12, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    return MRT_OK;
}
int probe_seeds(hipStream_t stream, uint32_t seed, int w, int h, uint32_t *out) {
    size_t n = (size_t)w * h;
    if (n == 0) return MRT_OK;
    DevBuf<uint32_t> d; MRT_HIP(d.alloc(n));
    hipLaunchKernelGGL(k_seed, dim3(cdiv(n, 256)), dim3(256), 0, stream, d.p, (uint32_t)n, seed);
    MRT_HIP(hipMemcpyAsync(out, d.p, n * 4, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    return MRT_OK;
}

}  // namespace mrt
