// traverse.h — stackless rope traversal + Möller–Trumbore for gfx950 (replaces the two uses of Apple's
// opaque `intersector.intersect`, Raytracing.metal:244 closest / :367 any).
#pragma once
#include <type_traits>
#include "scene_device.h"
#include "device_math.h"

namespace mrt {
namespace {

struct TravHit { float t, U, V, ad; uint32_t gid; uint32_t pk = 0xFFFFFFFFu; };      // pk: packet of the hit (read after traverse<SEED> and the lane walks only)
// The 16-byte hit record of the pipeline's `hits` queues: {t, u = U / |det|, v = V / |det|, global triangle id (bits)}; a miss is {-1, 0, 0, ~0}.
MRT_DEV float4 miss_record() { return make_float4(-1.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu)); }
MRT_DEV float4 hit_record(bool hit, const TravHit &h) { return hit ? make_float4(h.t, h.U / h.ad, h.V / h.ad, __uint_as_float(h.gid)) : miss_record(); }

MRT_DEV float safe_inv(float d) {
    float a = fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d;
    return 1.0f / a;
}

// 1 / d for the slab tests of the stream and the two-level traversal: v_rcp_f32 (1 ulp) + one Newton step instead of the IEEE division sequence (13 instead of
// 37 issue cycles, three per refilled ray).  Only box tests see it — they have to be conservative, not exact: the error (< 1 ulp) is two
// orders of magnitude below the build-time padding of the leaf boxes (1e-5 |coord| + 1e-6) and the far side is widened by 4 ulp.  The
// triangle test, hence the image, does not depend on it.
MRT_DEV float box_inv(float d) {
    const float a = fabsf(d) < 1e-20f ? copysignf(1e-20f, d) : d;
    const float r = __builtin_amdgcn_rcpf(a);
    return __builtin_fmaf(r, __builtin_fmaf(-a, r, 1.0f), r);
}

// One triangle, Möller–Trumbore in the fused mrt-math form; division only after the barycentric
// tests pass.  Returns true when 0 <= tmin <= t <= lim.
MRT_DEV bool tri_test(float4 p0, float4 p1, float4 p2, f3 o, f3 d, float tmin, float lim, float &t, float &U, float &V, float &ad) {
    f3 v0 = mk3(p0), e1 = mk3(p1), e2 = mk3(p2);
    f3 pv = fcross(d, e2);
    float det = fdot(e1, pv);
    if (!(det != 0.0f)) return false;
    ad = fabsf(det);
    uint32_t sgn = __float_as_uint(det) & 0x80000000u;
    f3 tv = o - v0;
    U = xorsign(fdot(tv, pv), sgn);
    if (!(U >= 0.0f && U <= ad)) return false;
    f3 q = fcross(tv, e1);
    V = xorsign(fdot(d, q), sgn);
    if (!(V >= 0.0f && U + V <= ad)) return false;
    float T = xorsign(fdot(e2, q), sgn);
    t = T / ad;
    return t >= tmin && t <= lim;
}

struct TravCounters { uint32_t steps, leaves, tris, wave_iters; int alu_dup = 0, mem_dup = 0; float sink = 0.0f;
                      uint32_t empty = 0, stale = 0; };     // 8-wide layout: node visits in which no child was hit / whose own grid box already lay beyond the best hit

// ---- filters: which candidates a ray may see.  The masked queries' is Visibility (lane_walk.h); every other walk sees all.
struct SeesAll {              // no table, no instruction
    MRT_DEV bool mesh(uint32_t) const { return true; }
    MRT_DEV bool triangle(uint32_t) const { return true; }
};

// ---- sinks: what a walk does with a hit.  A sink holds the walk's bound `lim` — what goes into tri_test and, widened, into the node tests — and
// take(t, U, V, |det|, packet, global id) of a visible hit with tmin <= t <= lim; true = the walk is over.
struct AnySink {
    float lim; bool hit = false;
    MRT_DEV bool take(float, float, float, float, uint32_t, uint32_t) { hit = true; return true; }
};
// Closest hit = global min t, ties to the lowest global id (t <= lim in take), so the result does not depend on the visiting order.  lim = the closest hit's distance.
// Made from a TravHit the sink starts with that hit as the one to beat (traverse<SEED>); pk tracks the packet of the winner and is dropped where nobody reads it.
struct ClosestSink {
    float lim; float U = 0.0f, V = 0.0f, ad = 1.0f; uint32_t gid = 0xFFFFFFFFu, pk = 0xFFFFFFFFu;
    MRT_DEV ClosestSink(float tmax) : lim(tmax) {}
    MRT_DEV ClosestSink(const TravHit &h) : lim(h.t), U(h.U), V(h.V), ad(h.ad), gid(h.gid), pk(h.pk) {}
    MRT_DEV bool take(float t, float U_, float V_, float ad_, uint32_t p, uint32_t g) {
        if (t < lim || g < gid) { lim = t; U = U_; V = V_; ad = ad_; gid = g; pk = p; }
        return false;
    }
    MRT_DEV bool into(TravHit &h) const { h.t = lim; h.U = U; h.V = V; h.ad = ad; h.gid = gid; h.pk = pk; return gid != 0xFFFFFFFFu; }
};
// The closest hit, or — `any` is a run-time flag, per lane — the first one, which ends the walk
struct ClosestOrAnySink : ClosestSink {
    bool any;
    MRT_DEV ClosestOrAnySink(float tmax, bool any_) : ClosestSink(tmax), any(any_) {}
    MRT_DEV bool take(float t, float U_, float V_, float ad_, uint32_t p, uint32_t g) { ClosestSink::take(t, U_, V_, ad_, p, g); return any; }
};

// slab test of one rope node (lo | a, hi | b) against a ray given as (1/d, -o/d): one fma per plane, t = plane * inv - o * inv.  The extra rounding (<= 1 ulp of o*inv, i.e.
// <= 6e-8 * |o| along the axis) is far inside the build-time padding of the boxes (1e-6 + 1e-5 * |coord|).  Conservative: the far side is widened by ~4 ulp (Ize 2013), and the
// limit like it: a box whose entry rounds past the closest hit may still hold a hit at that t (a lower id, an any-hit limit one float past it).
MRT_DEV bool rope_box_hit(const float4 r0, const float4 r1, float ix, float iy, float iz, float nox, float noy, float noz, float tmin, float tmax) {
    const float tx0 = __builtin_fmaf(r0.x, ix, nox), tx1 = __builtin_fmaf(r1.x, ix, nox);
    const float ty0 = __builtin_fmaf(r0.y, iy, noy), ty1 = __builtin_fmaf(r1.y, iy, noy);
    const float tz0 = __builtin_fmaf(r0.z, iz, noz), tz1 = __builtin_fmaf(r1.z, iz, noz);
    const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tmin));
    const float tf = fminf(fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1)) * 1.0000005f, tmax * 1.0000005f);
    return tn <= tf;
}

// Stackless traversal of the rope layout (scene_device.h).  State per ray: the next node, the pending
// triangle range of the current leaf and the sink — no stack, no parent walk.
//
// Loop shape: ONE kind of iteration.  Every iteration each live lane issues the same three 16-byte
// loads from its own base — a node (box lo|a, box hi|b, the escape quad of its octant) or one triangle
// packet (v0|gid, e1, e2) — so a wave iteration is exactly one memory round trip in which EVERY lane
// advances (a box test or a triangle test).  Measured on MI355X the wave time is (iterations of its
// slowest lane) x (round-trip latency); a split inner-node / leaf loop made the slowest wave iterate
// 4x more often than any of its lanes needed.
// A candidate that passed tri_test is shown to the filter, then to the sink; its packet index counts from s.packets.  STATS: counters and probes of k_query_stats (diagnostics).
template <bool STATS = false, class Filter, class Sink>
MRT_DEV void walk_rope(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k, TravCounters *tc = nullptr) {
    if (s.num_nodes == 0) return;
    const float ix = safe_inv(d.x), iy = safe_inv(d.y), iz = safe_inv(d.z);
    const float nox = -(o.x * ix), noy = -(o.y * iy), noz = -(o.z * iz);
    const uint32_t oct = (ix < 0.0f ? 1u : 0u) | (iy < 0.0f ? 2u : 0u) | (iz < 0.0f ? 4u : 0u);      // the reciprocal's sign: -0 counts as negative, as it does in 1 / d
    const uint32_t esc_off = 32u + ((oct >> 2) << 4), esc_lane = oct & 3u;
    // nodes and packets live in one allocation: one wave-uniform base + a 32-bit byte offset per lane
    const char *__restrict__ base = reinterpret_cast<const char *>(s.nodes);
    const uint32_t pk0 = (uint32_t)(reinterpret_cast<const char *>(s.packets) - base);
    uint32_t cur = 0;                 // next node, NODE_TERM when the walk is over
    uint32_t tri = 0, tri_end = 0;    // pending packets of the current leaf
    for (;;) {
        const bool do_tri = tri < tri_end;
        if (!do_tri && cur == NODE_TERM) break;
        if (STATS) { if (do_tri) tc->tris++; else tc->steps++; if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) tc->wave_iters++; }
        const uint32_t off = do_tri ? pk0 + tri * 48u : cur << 6;
        const float4 r0 = *reinterpret_cast<const float4 *>(base + off);
        const float4 r1 = *reinterpret_cast<const float4 *>(base + off + 16u);
        const float4 r2 = *reinterpret_cast<const float4 *>(base + off + (do_tri ? 32u : esc_off));
        if (do_tri) {
            tri++;
            float t, U, V, ad;
            if (tri_test(r0, r1, r2, o, d, tmin, k.lim, t, U, V, ad)) {
                const uint32_t gid = __float_as_uint(r0.w);
                if (vis.triangle(gid) && k.take(t, U, V, ad, tri - 1u, gid)) return;
            }
        } else {
            const bool hit = rope_box_hit(r0, r1, ix, iy, iz, nox, noy, noz, tmin, k.lim);
            if (STATS) {      // bottleneck probes: repeat the box arithmetic / the node fetch
                for (int r = 0; r < tc->alu_dup; r++) {
                    float e = 1e-9f * (float)(r + 1);
                    float ux0 = (r0.x - o.x + e) * ix, ux1 = (r1.x - o.x - e) * ix, uy0 = (r0.y - o.y + e) * iy, uy1 = (r1.y - o.y - e) * iy, uz0 = (r0.z - o.z + e) * iz, uz1 = (r1.z - o.z - e) * iz;
                    float un = fmaxf(fmaxf(fminf(ux0, ux1), fminf(uy0, uy1)), fmaxf(fminf(uz0, uz1), tmin));
                    float uf = fminf(fminf(fmaxf(ux0, ux1), fmaxf(uy0, uy1)), fmaxf(uz0, uz1)) * 1.0000005f;
                    tc->sink += (un <= fminf(uf, k.lim)) ? 1.0f : 0.0f;
                }
                for (int r = 0; r < tc->mem_dup; r++) {
                    const float4 *__restrict__ rr = s.nodes + 4 * (size_t)((cur + 7919u * (r + 1)) % s.num_nodes);
                    tc->sink += rr[0].x + rr[1].y + rr[2].z;
                }
            }
            const uint32_t a = __float_as_uint(r0.w), b = __float_as_uint(r1.w);
            const float escf = esc_lane == 0 ? r2.x : esc_lane == 1 ? r2.y : esc_lane == 2 ? r2.z : r2.w;
            const uint32_t esc = __float_as_uint(escf);
            const bool leaf = (a & NODE_LEAF) != 0;
            const uint32_t child = ((b >> (24 + oct)) & 1u) ? (b & NODE_INDEX_MASK) : a;
            cur = (hit && !leaf) ? child : esc;
            if (hit && leaf) { if (STATS) tc->leaves++; tri = a & 0x7FFFFFFFu; tri_end = tri + b; }
        }
    }
}

// What a walk<Sink> left in its sink, as the callers of traverse<>, traverse_instanced<> and traverse_wide<> take it: the closest hit in `h` — on a miss t = tmax, U = V = 0,
// ad = 1, gid = none — and whether there is one.  A compile-time any-hit walk leaves `h` at its miss values; a ray that is any-hit by the run-time flag leaves the hit
// that ended its walk there (its callers read the answer only).
template <bool ANY, bool RUNTIME_ANY>
using TravSink = std::conditional_t<ANY, AnySink, std::conditional_t<RUNTIME_ANY, ClosestOrAnySink, ClosestSink>>;
template <bool ANY, bool RUNTIME_ANY>
MRT_DEV TravSink<ANY, RUNTIME_ANY> trav_sink(float tmax, bool any_rt) {
    if constexpr (ANY) return {tmax}; else if constexpr (RUNTIME_ANY) return {tmax, any_rt}; else return {tmax};
}
MRT_DEV bool trav_result(const AnySink &k, float tmax, TravHit &h) { h.t = tmax; h.U = 0.0f; h.V = 0.0f; h.ad = 1.0f; h.gid = 0xFFFFFFFFu; return k.hit; }
MRT_DEV bool trav_result(const ClosestSink &k, float, TravHit &h) { return k.into(h); }

// SEED: `h` already holds a candidate hit (or t = tmax, gid = none) that the walk has to beat — a correct guess makes every box behind it a miss
// from the first step on; the result is the same minimum over (t, id) either way.  h.pk then tracks the packet of the winner.
template <bool ANY, bool STATS = false, bool RUNTIME_ANY = false, bool SEED = false>
MRT_DEV bool traverse(const SceneView &s, f3 o, f3 d, float tmin, float tmax, TravHit &h, TravCounters *tc = nullptr, bool any_rt = false) {
    if constexpr (SEED) { ClosestSink k(h); walk_rope(s, SeesAll{}, o, d, tmin, k); return k.into(h); }
    else { auto k = trav_sink<ANY, RUNTIME_ANY>(tmax, any_rt); walk_rope<STATS>(s, SeesAll{}, o, d, tmin, k, tc); return trav_result(k, tmax, h); }
}

}  // namespace
}  // namespace mrt
