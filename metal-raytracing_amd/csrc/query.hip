// query.hip — ray queries against a committed scene: the C-ABI's mrt_scene_intersect_closest / _any (host rays), their stream-ordered forms on caller device
// buffers (_closest_device / _any_device) and the traversal diagnostics of mrt_debug.h (per-ray statistics, the render kernels' stream walk on caller rays).
// Replaces the direct uses of `intersector.intersect` outside the frame (Raytracing.metal:244 closest, :367 any).  Siblings: multihit.hip, masked.hip, surface.hip.
// The kernels here are held to the instructions they had inside renderer.hip (docs/HISTORY.md §22), and which of them share an LDS array name decides that
// (k_query_stream_stats): after adding or changing a stream kernel in this unit, compare the listings again with tools/isa_diff.py.
#include "renderer.h"
#include "device_math.h"
#include "traverse.h"
#include "traverse_wide.h"
#include "traverse_instanced.h"

namespace mrt {
namespace {

// ------------------------------------------------------------------ query kernels (C-ABI intersect_*)
// the record of a closest-hit query: ids by hit_ids, u = U / |det|, v = V / |det|; a miss is {0, -1.0f, -1, -1, -1, 0, 0}
MRT_DEV MRTIntersection closest_record(const SceneView &s, bool two_level, bool hit, const TravHit &h) {
    MRTIntersection o;
    o._pad = 0; o.type = 0; o.distance = -1.0f; o.instance_id = o.geometry_id = o.primitive_id = -1; o.u = o.v = 0.0f;
    if (hit) {
        uint32_t inst, geom, prim;
        hit_ids(s, two_level, h.gid, inst, geom, prim);
        o.type = 1; o.distance = h.t; o.instance_id = (int32_t)inst; o.geometry_id = (int32_t)geom; o.primitive_id = (int32_t)prim;
        o.u = h.U / h.ad; o.v = h.V / h.ad;
    }
    return o;
}
template <bool WIDE>
__global__ void __launch_bounds__(64) k_query_closest(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, MRTIntersection *__restrict__ out) {
    extern __shared__ uint32_t stk[];      // WIDE: the scene's wide-tree depth x WIDE_STACK_LEVEL_BYTES, sized by the host
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    MRTRay r = rays[i];
    TravHit h;
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    bool hit = s.num_inst ? traverse_instanced<false>(s, ro, rd, r.min_distance, r.max_distance, h)
             : WIDE ? traverse_wide<false>(s, ro, rd, r.min_distance, r.max_distance, h, stk) : traverse<false>(s, ro, rd, r.min_distance, r.max_distance, h);
    out[i] = closest_record(s, s.num_inst != 0, hit, h);
}
template <bool WIDE>
__global__ void __launch_bounds__(64) k_query_any(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, int32_t *__restrict__ out) {
    extern __shared__ uint32_t stk[];      // WIDE: the scene's wide-tree depth x WIDE_STACK_LEVEL_BYTES, sized by the host
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    MRTRay r = rays[i];
    TravHit h;
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    out[i] = (s.num_inst ? traverse_instanced<true>(s, ro, rd, r.min_distance, r.max_distance, h)
              : WIDE ? traverse_wide<true>(s, ro, rd, r.min_distance, r.max_distance, h, stk) : traverse<true>(s, ro, rd, r.min_distance, r.max_distance, h)) ? 1 : 0;
}

// per-ray traversal statistics (steps, leaf visits, triangle tests) — diagnostics only
template <bool WIDE>
__global__ void __launch_bounds__(64) k_query_stats(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, int any, uint32_t *__restrict__ out) {
    extern __shared__ uint32_t stk[];      // WIDE: the scene's wide-tree depth x WIDE_STACK_LEVEL_BYTES, sized by the host
    uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    MRTRay r = rays[i];
    TravHit h; TravCounters tc{0, 0, 0, 0};
    tc.alu_dup = (any >> 8) & 0xFF; tc.mem_dup = (any >> 16) & 0xFF; any &= 1;
    f3 o = mk3(r.origin[0], r.origin[1], r.origin[2]), d = mk3(r.direction[0], r.direction[1], r.direction[2]);
    unsigned long long t0 = wall_clock64();
    if (WIDE) { if (any) traverse_wide<true, true>(s, o, d, r.min_distance, r.max_distance, h, stk, &tc); else traverse_wide<false, true>(s, o, d, r.min_distance, r.max_distance, h, stk, &tc); }
    else { if (any) traverse<true, true>(s, o, d, r.min_distance, r.max_distance, h, &tc); else traverse<false, true>(s, o, d, r.min_distance, r.max_distance, h, &tc); }
    unsigned long long t1 = wall_clock64();
    out[8 * i + 0] = tc.steps; out[8 * i + 1] = tc.leaves; out[8 * i + 2] = tc.tris; out[8 * i + 3] = h.gid;
    out[8 * i + 4] = (uint32_t)t0; out[8 * i + 5] = (uint32_t)t1; out[8 * i + 6] = tc.wave_iters;   // 100 MHz ticks
    out[8 * i + 7] = (tc.alu_dup | tc.mem_dup) ? __float_as_uint(tc.sink) : (tc.empty & 0xFFFFu) | (tc.stale << 16);    // 8-wide layout: empty visits | stale visits << 16
}

// stream-traversal lane accounting (diagnostics): per wave {iterations, sum of live lanes, node lanes, tri lanes, refills, refilled lanes}
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(64) k_query_stream_stats(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, int any, uint32_t per_wave, uint32_t depth, uint32_t *__restrict__ out) {
    // (a name of its own for the wave's LDS: were it stk_dyn in every two-level stream kernel of this unit, the optimiser would specialise the helpers they share
    // for that one address, and their instructions would no longer be those of the same walk in renderer.hip — tools/isa_diff.py, docs/HISTORY.md §22)
    extern __shared__ uint32_t stats_stk[];
    const uint32_t begin = blockIdx.x * per_wave;
    if (begin >= n) return;
    const uint32_t end = min(n, begin + per_wave);
    StreamStats ss{0, 0, 0, 0, 0, 0};
    uint32_t sink = 0;
#if defined(MRT_STATS_PROBE) && MRT_STATS_PROBE == 1
    {   // BFS numbering, children contiguous: level L + 1 starts where level L ends and holds the internal children (imask bits) of level L's nodes
        uint32_t lo = 0, hi = 1;
        for (int L = 0; L < 3; L++) {
            uint32_t kids = 0;
            for (uint32_t i = lo; i < hi; i++) kids += (uint32_t)__popc(__float_as_uint(s.wnodes[WNODE_STRIDE * (size_t)i].w) >> 24);
            lo = hi; hi += kids; ss.level_end[L] = hi;
        }
    }
#endif
    traverse_wide_stream<TWO_LEVEL>(s, OneRange{begin, end}, stats_stk,
        [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) {
            MRTRay r = rays[i]; tag = i & 0x7FFFFFFFu;
            A = make_float4(r.origin[0], r.origin[1], r.origin[2], r.max_distance); B = make_float4(r.direction[0], r.direction[1], r.direction[2], 0.0f); is_any = (uint32_t)any;
        },
        [&](uint32_t, bool, bool hit, const TravHit &) { sink += hit ? 1u : 0u; }, &ss);
    if ((threadIdx.x & 63) == 0) {
        uint32_t *o = out + 8 * (size_t)blockIdx.x;
        o[0] = ss.iters; o[1] = ss.live_sum; o[2] = ss.node_sum; o[3] = ss.tri_sum; o[4] = ss.refills; o[5] = ss.refill_lanes; o[6] = sink; o[7] = end - begin;
#ifdef MRT_STATS_PROBE
        o[4] = ss.probe[0]; o[5] = ss.probe[1]; o[6] = ss.probe[2];
#endif
    }
}

// the render kernels' traversal (8-wide stream with lane refill; both levels of an instanced scene) on caller rays — parity tests of that path
template <bool TWO_LEVEL>
__global__ void __launch_bounds__(64) k_query_stream(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, int any, uint32_t per_wave, MRTIntersection *__restrict__ out) {
    extern __shared__ uint32_t stk_dyn[];
    const uint32_t begin = blockIdx.x * per_wave;
    if (begin >= n) return;
    traverse_wide_stream<TWO_LEVEL>(s, OneRange{begin, min(n, begin + per_wave)}, stk_dyn,
        [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) {
            MRTRay r = rays[i]; tag = i & 0x7FFFFFFFu; is_any = (uint32_t)any;
            A = make_float4(r.origin[0], r.origin[1], r.origin[2], r.max_distance); B = make_float4(r.direction[0], r.direction[1], r.direction[2], 0.0f);
        },
        [&](uint32_t i, bool is_any, bool hit, const TravHit &h) {
            MRTIntersection o = closest_record(s, TWO_LEVEL, hit && !is_any, h);
            o.type = hit ? 1 : 0;
            out[i] = o;
        });
}

// ------------------------------------------------------------------ stream-ordered queries on caller buffers (mrt_scene_intersect_*_device)
// Two launches on the caller's stream, no allocation, no copy, no synchronisation.  Every ray is answered by exactly one of them, and both decide with the same
// expression (min_distance != 0), so every record is written exactly once whatever the rays hold:
//   k_query_stream_device   rays with min_distance == 0 on the 8-wide layout: the render kernels' walk (traverse_wide_stream, lane refill, both levels of a two-level
//                           scene on one stack).  Its scaled node test has tmin = 0 built in, so a ray with another min_distance enters the loop as the inert ray of a
//                           partial-tile slot (tmax < 0 -> miss: one refill slot, no node visit) and its result is not written.
//   k_query_lane_device     the other rays — and all rays of a scene without the 8-wide layout — one per lane with the walks of mrt_scene_intersect_closest / _any,
//                           which carry tmin.  A lane whose ray the stream kernel answered leaves after reading min_distance.
constexpr uint32_t QUERY_STREAM_RAYS = 256;      // rays per wave of the static split, as k_query_stream
template <bool TWO_LEVEL, bool ANY>
__global__ void __launch_bounds__(64, TWO_LEVEL ? MRT_TWO_LEVEL_WAVES : MRT_WIDE_STREAM_WAVES) k_query_stream_device(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, const uint32_t *__restrict__ count, void *__restrict__ out) {
    extern __shared__ uint32_t stk_dyn[];
    if (count) n = min(n, *count);      // the caller's device-side ray count (null: every ray), read once as a uniform scalar load: the rays at and past it are not touched
    const uint32_t begin = blockIdx.x * QUERY_STREAM_RAYS;
    if (begin >= n) return;
    traverse_wide_stream<TWO_LEVEL>(s, OneRange{begin, min(n, begin + QUERY_STREAM_RAYS)}, stk_dyn,
        [&](uint32_t i, float4 &A, float4 &B, uint32_t &tag, uint32_t &is_any) {
            const MRTRay r = rays[i]; tag = i; is_any = ANY ? 1u : 0u;
            if (r.min_distance != 0.0f) { A = make_float4(0.0f, 0.0f, 0.0f, -1.0f); B = make_float4(0.0f, 0.0f, 1.0f, 0.0f); }      // the lane kernel's ray: inert here (tmax < 0 -> miss)
            else { A = make_float4(r.origin[0], r.origin[1], r.origin[2], r.max_distance); B = make_float4(r.direction[0], r.direction[1], r.direction[2], 0.0f); }
        },
        [&](uint32_t i, bool, bool hit, const TravHit &h) {
            if (rays[i].min_distance != 0.0f) return;
            if (ANY) static_cast<int32_t *>(out)[i] = hit ? 1 : 0;
            else static_cast<MRTIntersection *>(out)[i] = closest_record(s, TWO_LEVEL, hit, h);
        });
}
template <bool WIDE, bool ANY>
__global__ void __launch_bounds__(64) k_query_lane_device(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, const uint32_t *__restrict__ count, void *__restrict__ out) {
    extern __shared__ uint32_t stk[];      // WIDE: the scene's wide-tree depth x WIDE_STACK_LEVEL_BYTES, sized by the host
    if (count) n = min(n, *count);      // (as k_query_stream_device)
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    const bool mine = i < n && (s.num_wnodes == 0 || rays[i].min_distance != 0.0f);      // without the 8-wide layout no stream kernel ran: every ray is answered here
    if (__ballot(mine) == 0ull) return;      // nothing for this wave: a uniform branch to the end
    if (!mine) return;
    const MRTRay r = rays[i];
    TravHit h;
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    const bool hit = s.num_inst ? traverse_instanced<ANY>(s, ro, rd, r.min_distance, r.max_distance, h)
                   : WIDE ? traverse_wide<ANY>(s, ro, rd, r.min_distance, r.max_distance, h, stk) : traverse<ANY>(s, ro, rd, r.min_distance, r.max_distance, h);
    if (ANY) static_cast<int32_t *>(out)[i] = hit ? 1 : 0;
    else static_cast<MRTIntersection *>(out)[i] = closest_record(s, s.num_inst != 0, hit, h);
}

// The round trip of the host-pointer entries: n rays up, launch(d_rays, d_out) on `stream`, n_out elements down, synchronised.
template <class T, class Launch>
int round_trip(hipStream_t stream, const MRTRay *rays, size_t n, T *out, size_t n_out, Launch launch) {
    DevBuf<MRTRay> d_r; DevBuf<T> d_o;
    MRT_HIP(d_r.alloc(n)); MRT_HIP(d_o.alloc(n_out));
    MRT_HIP(hipMemcpyAsync(d_r.p, rays, n * sizeof(MRTRay), hipMemcpyHostToDevice, stream));
    if (int rc = launch(d_r.p, d_o.p)) return rc;
    MRT_HIP(hipMemcpyAsync(out, d_o.p, n_out * sizeof(T), hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace

int query_closest(const DeviceScene &sc, hipStream_t stream, const MRTRay *rays, size_t n, MRTIntersection *out) {
    if (n == 0) return MRT_OK;
    return round_trip(stream, rays, n, out, n, [&](const MRTRay *d_r, MRTIntersection *d_o) {
        if (sc.num_wnodes) hipLaunchKernelGGL(k_query_closest<true>, dim3(cdiv(n, 64)), dim3(64), (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES, stream, sc.view(), d_r, (uint32_t)n, d_o);
        else hipLaunchKernelGGL(k_query_closest<false>, dim3(cdiv(n, 64)), dim3(64), 0, stream, sc.view(), d_r, (uint32_t)n, d_o);
        return MRT_OK;
    });
}
int query_any(const DeviceScene &sc, hipStream_t stream, const MRTRay *rays, size_t n, int32_t *out) {
    if (n == 0) return MRT_OK;
    return round_trip(stream, rays, n, out, n, [&](const MRTRay *d_r, int32_t *d_o) {
        if (sc.num_wnodes) hipLaunchKernelGGL(k_query_any<true>, dim3(cdiv(n, 64)), dim3(64), (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES, stream, sc.view(), d_r, (uint32_t)n, d_o);
        else hipLaunchKernelGGL(k_query_any<false>, dim3(cdiv(n, 64)), dim3(64), 0, stream, sc.view(), d_r, (uint32_t)n, d_o);
        return MRT_OK;
    });
}

int query_stats(const DeviceScene &sc, hipStream_t stream, const MRTRay *rays, size_t n, int any, uint32_t *out4) {
    if (n == 0) return MRT_OK;
    return round_trip(stream, rays, n, out4, 8 * n, [&](const MRTRay *d_r, uint32_t *d_o) {
        if (sc.num_wnodes) hipLaunchKernelGGL(k_query_stats<true>, dim3(cdiv(n, 64)), dim3(64), (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES, stream, sc.view(), d_r, (uint32_t)n, any, d_o);
        else hipLaunchKernelGGL(k_query_stats<false>, dim3(cdiv(n, 64)), dim3(64), 0, stream, sc.view(), d_r, (uint32_t)n, any, d_o);
        return MRT_OK;
    });
}

int query_stream_stats(const DeviceScene &sc, hipStream_t stream, const MRTRay *rays, size_t n, int any, uint32_t per_wave, uint32_t *out8, size_t nwaves) {
    if (n == 0 || sc.num_wnodes == 0) return MRT_OK;
    return round_trip(stream, rays, n, out8, 8 * nwaves, [&](const MRTRay *d_r, uint32_t *d_o) -> int {
        MRT_HIP(hipMemsetAsync(d_o, 0, 32 * nwaves, stream));      // a wave without rays writes nothing
        const size_t lds = (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES + (sc.num_inst ? WIDE_WORLD_RAY_BYTES : 0);
        if (sc.num_inst) hipLaunchKernelGGL(k_query_stream_stats<true>, dim3((uint32_t)nwaves), dim3(64), lds, stream, sc.view(), d_r, (uint32_t)n, any, per_wave, (uint32_t)sc.wide_depth, d_o);
        else hipLaunchKernelGGL(k_query_stream_stats<false>, dim3((uint32_t)nwaves), dim3(64), lds, stream, sc.view(), d_r, (uint32_t)n, any, per_wave, (uint32_t)sc.wide_depth, d_o);
        return MRT_OK;
    });
}

int query_stream(const DeviceScene &sc, hipStream_t stream, const MRTRay *rays, size_t n, int any, MRTIntersection *out) {
    if (n == 0) return MRT_OK;
    if (sc.num_wnodes == 0) { set_error("the scene has no 8-wide layout"); return MRT_ERR_UNSUPPORTED; }
    for (size_t i = 0; i < n; i++) if (rays[i].min_distance != 0.0f) { set_error("the stream traversal starts every ray at distance 0 (min_distance must be 0)"); return MRT_ERR_INVALID_ARGUMENT; }
    if (n >= (size_t(1) << 31)) { set_error("too many rays"); return MRT_ERR_INVALID_ARGUMENT; }
    const int rc = round_trip(stream, rays, n, out, n, [&](const MRTRay *d_r, MRTIntersection *d_o) {
        const uint32_t per_wave = QUERY_STREAM_RAYS;
        const size_t lds = (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES + (sc.num_inst ? WIDE_WORLD_RAY_BYTES : 0);
        if (sc.num_inst) hipLaunchKernelGGL(k_query_stream<true>, dim3(cdiv(n, per_wave)), dim3(64), lds, stream, sc.view(), d_r, (uint32_t)n, any, per_wave, d_o);
        else hipLaunchKernelGGL(k_query_stream<false>, dim3(cdiv(n, per_wave)), dim3(64), lds, stream, sc.view(), d_r, (uint32_t)n, any, per_wave, d_o);
        return MRT_OK;
    });
    return rc ? rc : check_bounds_record();      // (this unit's record: k_query_stream is its kernel)
}

// The stream-ordered entries (mrt_scene_intersect_closest_device / _any_device): both launches on the caller's stream, nothing else.
template <bool ANY>
static int query_device_t(const DeviceScene &sc, hipStream_t stream, const MRTRay *d_rays, size_t n, void *d_out, const void *d_count) {
    const SceneView sv = sc.view();
    const uint32_t *const cnt = static_cast<const uint32_t *>(d_count);      // (grids are sized by n, the capacity: a workgroup past the count leaves at once)
    const uint32_t n32 = (uint32_t)n;
    if (sc.num_wnodes) {
        const size_t lds = (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES + (sc.num_inst ? WIDE_WORLD_RAY_BYTES : 0);
        if (sc.num_inst) hipLaunchKernelGGL((k_query_stream_device<true, ANY>), dim3(cdiv(n, QUERY_STREAM_RAYS)), dim3(64), lds, stream, sv, d_rays, n32, cnt, d_out);
        else hipLaunchKernelGGL((k_query_stream_device<false, ANY>), dim3(cdiv(n, QUERY_STREAM_RAYS)), dim3(64), lds, stream, sv, d_rays, n32, cnt, d_out);
        MRT_HIP(hipGetLastError());
    }
    if (sc.num_wnodes) hipLaunchKernelGGL((k_query_lane_device<true, ANY>), dim3(cdiv(n, 64)), dim3(64), (size_t)sc.wide_depth * WIDE_STACK_LEVEL_BYTES, stream, sv, d_rays, n32, cnt, d_out);
    else hipLaunchKernelGGL((k_query_lane_device<false, ANY>), dim3(cdiv(n, 64)), dim3(64), 0, stream, sv, d_rays, n32, cnt, d_out);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}
int query_closest_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, size_t n, void *d_out, const void *d_count) { return query_device_t<false>(sc, stream, static_cast<const MRTRay *>(d_rays), n, d_out, d_count); }
int query_any_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, size_t n, void *d_occluded, const void *d_count) { return query_device_t<true>(sc, stream, static_cast<const MRTRay *>(d_rays), n, d_occluded, d_count); }

}  // namespace mrt
