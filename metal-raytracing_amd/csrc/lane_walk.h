// lane_walk.h — the one-ray-per-lane walks of the device queries that are not the render path's: all hits in order (multihit.hip) and the three queries with
// a visibility mask (masked.hip; §10p).  Each walk is written ONCE per layout, for every query and with or without masks (§10q):
//
//   walk_wide         the 8-wide layout: traverse_wide<ANY>'s loop (traverse_wide.h; it carries tmin), the wave's stack in dynamic LDS
//   walk_rope         the rope layout (scene option wide = 0) and the empty scene: traverse<ANY>'s stackless loop (traverse.h)
//   walk_instanced    two-level scenes: traverse_instanced<ANY>'s flat loop (traverse_instanced.h)
//
// What a query does with a hit is its SINK: it holds the walk's bound `lim` — what goes into tri_test and into the node tests where the closest hit's distance goes in the
// walks named above; both node tests widen it as they widen that distance, so a child entered exactly at the bound is still visited — and takes a candidate.  Which
// candidates a ray may see is its FILTER.  It sits in the walk, between the triangle test and the sink: a candidate that passed tri_test is looked up — its global id is word 3
// of the packet the walk holds, its mesh tri_shade[gid].w >> 16 — and an invisible one is dropped before the sink sees it, so it can neither end an any-hit walk, nor lower a
// bound, nor decide a tie, nor take a list slot.  Two dependent small gathers per ACCEPTED candidate, none per test.  In a two-level scene the instance's mask is tested when its
// id is taken from tlas_index, before the ray is transformed: a skipped instance costs one table read, and nothing inside a BLAS is tested (every triangle of an instance has
// its mask).  The unmasked queries walk with SeesAll, which is true at compile time.
// traverse<>, traverse_instanced<> and traverse_wide<> themselves are not built from these: they carry STATS, SEED, RUNTIME_ANY and a root, and are inlined into the render kernels.
#pragma once
#include "traverse_wide.h"

namespace mrt {
namespace {

enum Form : uint32_t { WIDE = 0, ROPE = 1, INSTANCED = 2 };

// ---- filters
struct Visibility {
    const uint4 *__restrict__ tri_shade; const uint32_t *__restrict__ mesh_masks; uint32_t ray_mask;
    MRT_DEV bool mesh(uint32_t id) const { return (mesh_masks[id] & ray_mask) != 0u; }
    MRT_DEV bool triangle(uint32_t gid) const { return mesh(tri_shade[gid].w >> 16); }      // flattened scenes: tri_shade is indexed by the global id
};
struct SeesAll {              // no table, no instruction
    MRT_DEV bool mesh(uint32_t) const { return true; }
    MRT_DEV bool triangle(uint32_t) const { return true; }
};

// ---- sinks.  take(t, U, V, |det|, packet, global id) of a visible hit with tmin <= t <= lim; true = the walk is over.
struct AnySink {
    float lim; bool hit = false;
    MRT_DEV bool take(float, float, float, float, uint32_t, uint32_t) { hit = true; return true; }
};
struct ClosestSink {          // lim = the closest visible hit's distance; ties to the lowest global id, as every closest-hit walk decides them (t <= lim here)
    float lim; float U = 0.0f, V = 0.0f, ad = 1.0f; uint32_t gid = 0xFFFFFFFFu;
    MRT_DEV bool take(float t, float U_, float V_, float ad_, uint32_t, uint32_t g) {
        if (t < lim || g < gid) { lim = t; U = U_; V = V_; ad = ad_; gid = g; }
        return false;
    }
};
// All hits: the lane's K smallest under the key (distance, global id), ascending.  While the list holds fewer than K entries lim is the ray's max_distance, once it is full the
// K-th entry's distance.  A wave's lists lie in LDS (behind its stack): per slot 64 distances then 64 packet indices ([slot][2][64 lanes]: a wave's access to one slot is 64
// consecutive words, no bank conflict), 512 B per slot, 8 KB at K = 16.  An entry keeps the packet, not U, V and |det|: emit_list_row tests the winners again, which costs K
// packet reads per ray once and saves three words per entry for the whole walk.  The id is not kept either: it is needed only where two distances are EQUAL (a shared edge,
// coincident faces, two references of one pre-split triangle), and is then read from the packet.  No private array anywhere: nothing is indexed at run time but LDS.
constexpr uint32_t LIST_SLOT_WORDS = 128;
MRT_DEV float list_t(const float *list, uint32_t lane, uint32_t j) { return list[j * LIST_SLOT_WORDS + lane]; }
MRT_DEV uint32_t list_pk(const float *list, uint32_t lane, uint32_t j) { return __float_as_uint(list[j * LIST_SLOT_WORDS + 64u + lane]); }
MRT_DEV void list_set(float *list, uint32_t lane, uint32_t j, float t, uint32_t pk) { list[j * LIST_SLOT_WORDS + lane] = t; list[j * LIST_SLOT_WORDS + 64u + lane] = __uint_as_float(pk); }
// pkts / STRIDE: the packet array the walk reads (the id of an entry is word 3 of its packet).  c: entries held.  The entries above a candidate move up one slot, a full list
// drops its last one.  A candidate equal in distance AND id to an entry is the same triangle met through another reference of a pre-split triangle: dropped.
template <uint32_t STRIDE>
struct ListSink {
    float lim; float *list; const float4 *__restrict__ pkts; uint32_t K; uint32_t c = 0;
    MRT_DEV bool take(float t, float, float, float, uint32_t pk, uint32_t gid) {
        const uint32_t lane = threadIdx.x & 63;
        uint32_t j = c;      // the candidate's slot: behind every entry with a smaller key
        while (j > 0u) {
            const float tj = list_t(list, lane, j - 1u);
            if (tj < t) break;
            if (tj == t) {
                const uint32_t gj = __float_as_uint(pkts[STRIDE * (size_t)list_pk(list, lane, j - 1u)].w);
                if (gj == gid) return false;
                if (gj < gid) break;
            }
            j--;
        }
        if (j == K) return false;      // as far as the full list's last entry, with a higher id
        for (uint32_t k = c < K ? c : K - 1u; k > j; k--) list_set(list, lane, k, list_t(list, lane, k - 1u), list_pk(list, lane, k - 1u));
        list_set(list, lane, j, t, pk);
        if (c < K) c++;
        if (c == K) lim = list_t(list, lane, K - 1u);
        return false;
    }
};
template <Form FORM> constexpr uint32_t PACKET_STRIDE = FORM == WIDE ? WPK : 3u;
template <Form FORM>          // the list of a ray that walks layout FORM
MRT_DEV ListSink<PACKET_STRIDE<FORM>> list_sink(const SceneView &s, float tmax, float *list, uint32_t K) { return {tmax, list, FORM == WIDE ? s.wpackets : s.packets, K}; }

// ---- walks
// stack: depth x WIDE_STACK_LEVEL_BYTES of LDS
template <class Filter, class Sink>
MRT_DEV void walk_wide(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k, uint32_t *stack) {
    if (s.num_wnodes == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const float ix = safe_inv(d.x), iy = safe_inv(d.y), iz = safe_inv(d.z);
    const bool nx = d.x < 0.0f, ny = d.y < 0.0f, nz = d.z < 0.0f;
    const uint32_t oct = (nx ? 1u : 0u) | (ny ? 2u : 0u) | (nz ? 4u : 0u);
    uint32_t sp = 0;
    uint32_t g_base = 0, g_mask = 0;      // node group: (permuted hit bits << 8) | imask
    uint32_t t_base = 0, t_mask = 0;      // triangle group: bit k = packet t_base + k still to test
    uint32_t pending = 0; bool have_pending = true;     // start by entering the root
    for (;;) {
        const bool do_tri = t_mask != 0;
        if (!do_tri && !have_pending) {
            if ((g_mask >> 8) == 0) {
                if (sp == 0) break;
                sp--;
                wstack_pop(stack, sp, lane, g_base, g_mask);
            }
            pending = take_nearest_child(g_base, g_mask, oct);
            have_pending = true;
        }
        if (do_tri) {
            uint32_t pk = t_base + (uint32_t)__ffs((int)t_mask) - 1u;
            t_mask &= t_mask - 1u;
            float4 r0, r1, r2;
            MRT_LOAD_PACKET(s, pk, r0, r1, r2);
            float t, U, V, ad;
            if (tri_test(r0, r1, r2, o, d, tmin, k.lim, t, U, V, ad)) {
                const uint32_t gid = __float_as_uint(r0.w);
                if (vis.triangle(gid) && k.take(t, U, V, ad, pk, gid)) return;
            }
        } else {
            float4 n0, n1, n2, n3, n4;
            MRT_LOAD_NODE(s, pending, n0, n1, n2, n3, n4);
            have_pending = false;
            uint32_t node_hits, tri_hits;
            wide_node_test(n0, n1, n2, n3, n4, o, ix, iy, iz, nx, ny, nz, oct, tmin, k.lim, node_hits, tri_hits);
            if ((g_mask >> 8) != 0) { wstack_push(stack, sp, lane, g_base, g_mask); sp++; }     // siblings still to visit
            g_base = __float_as_uint(n1.x); g_mask = (node_hits << 8) | (__float_as_uint(n0.w) >> 24);
            t_base = __float_as_uint(n1.y); t_mask = tri_hits;
        }
    }
}

// the packets are the rope layout's own copy, indexed from s.packets
template <class Filter, class Sink>
MRT_DEV void walk_rope(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k) {
    if (s.num_nodes == 0) return;
    const float ix = safe_inv(d.x), iy = safe_inv(d.y), iz = safe_inv(d.z);
    const float nox = -(o.x * ix), noy = -(o.y * iy), noz = -(o.z * iz);
    const uint32_t oct = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
    const uint32_t esc_off = 32u + ((oct >> 2) << 4), esc_lane = oct & 3u;
    const char *__restrict__ base = reinterpret_cast<const char *>(s.nodes);
    const uint32_t pk0 = (uint32_t)(reinterpret_cast<const char *>(s.packets) - base);
    uint32_t cur = 0;                 // next node, NODE_TERM when the walk is over
    uint32_t tri = 0, tri_end = 0;    // pending packets of the current leaf
    for (;;) {
        const bool do_tri = tri < tri_end;
        if (!do_tri && cur == NODE_TERM) break;
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
            const uint32_t a = __float_as_uint(r0.w), b = __float_as_uint(r1.w);
            const float escf = esc_lane == 0 ? r2.x : esc_lane == 1 ? r2.y : esc_lane == 2 ? r2.z : r2.w;
            const uint32_t esc = __float_as_uint(escf);
            const bool leaf = (a & NODE_LEAF) != 0;
            const uint32_t child = ((b >> (24 + oct)) & 1u) ? (b & NODE_INDEX_MASK) : a;
            cur = (hit && !leaf) ? child : esc;
            if (hit && leaf) { tri = a & 0x7FFFFFFFu; tri_end = tri + b; }
        }
    }
}

// one flat loop over TLAS nodes, instance entries, BLAS nodes and triangles.  The candidate's id is the GLOBAL one.
template <class Filter, class Sink>
MRT_DEV void walk_instanced(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k) {
    if (s.num_nodes == 0 || s.num_inst == 0) return;
    const float ix = safe_inv(d.x), iy = safe_inv(d.y), iz = safe_inv(d.z);
    const float nox = -(o.x * ix), noy = -(o.y * iy), noz = -(o.z * iz);
    const char *__restrict__ bbase = reinterpret_cast<const char *>(s.bnodes);
    const uint32_t bpk0 = (uint32_t)(reinterpret_cast<const char *>(s.bpackets) - bbase);
    uint32_t cur = 0;                 // next TLAS node
    uint32_t li = 0, li_end = 0;      // pending instances of the current TLAS leaf
    bool in_blas = false;
    f3 oo = o, dd = d; float jx = ix, jy = iy, jz = iz, mox = nox, moy = noy, moz = noz;
    uint32_t node_base = 0, packet_base = 0, gid_base = 0, oct = 0;
    uint32_t bc = NODE_TERM, tri = 0, tri_end = 0;
    for (;;) {
        const bool do_tri = tri < tri_end;
        if (!do_tri && in_blas && bc == NODE_TERM) in_blas = false;            // this instance is finished: back to the TLAS
        if (!do_tri && !in_blas) {
            if (li < li_end) {                                                  // the next instance of the TLAS leaf: entered only if the ray may see it
                const uint32_t id = s.tlas_index[li++];
                if (!vis.mesh(id)) continue;
                const InstanceDev I = s.inst[id];
                oo = to_object_point(I, o); dd = to_object_dir(I, d);
                jx = box_inv(dd.x); jy = box_inv(dd.y); jz = box_inv(dd.z);
                mox = -(oo.x * jx); moy = -(oo.y * jy); moz = -(oo.z * jz);
                oct = (dd.x < 0.0f ? 1u : 0u) | (dd.y < 0.0f ? 2u : 0u) | (dd.z < 0.0f ? 4u : 0u);
                node_base = I.node_base; packet_base = I.packet_base; gid_base = I.gid_base;
                bc = 0; in_blas = true;
                continue;
            }
            if (cur == NODE_TERM) break;
            const float4 *__restrict__ nd = s.nodes + 4 * (size_t)cur;         // a TLAS node
            const float4 r0 = nd[0], r1 = nd[1], r2 = nd[2];
            const uint32_t a = __float_as_uint(r0.w), b = __float_as_uint(r1.w), esc = __float_as_uint(r2.x);    // the host TLAS has one escape link for all octants
            const bool hit = rope_box_hit(r0, r1, ix, iy, iz, nox, noy, noz, tmin, k.lim);
            if (hit && (a & NODE_LEAF)) { li = a & 0x7FFFFFFFu; li_end = li + b; cur = esc; }
            else cur = hit ? a : esc;
            continue;
        }
        const uint32_t esc_off = 32u + ((oct >> 2) << 4), esc_lane = oct & 3u;
        const uint32_t off = do_tri ? bpk0 + (packet_base + tri) * 48u : (node_base + bc) << 6;
        const float4 q0 = *reinterpret_cast<const float4 *>(bbase + off);
        const float4 q1 = *reinterpret_cast<const float4 *>(bbase + off + 16u);
        const float4 q2 = *reinterpret_cast<const float4 *>(bbase + off + (do_tri ? 32u : esc_off));
        if (do_tri) {
            tri++;
            float t, U, V, ad;
            if (tri_test(q0, q1, q2, oo, dd, tmin, k.lim, t, U, V, ad) && k.take(t, U, V, ad, packet_base + tri - 1u, gid_base + __float_as_uint(q0.w))) return;
        } else {
            const uint32_t a = __float_as_uint(q0.w), b = __float_as_uint(q1.w);
            const float escf = esc_lane == 0 ? q2.x : esc_lane == 1 ? q2.y : esc_lane == 2 ? q2.z : q2.w;
            const uint32_t esc = __float_as_uint(escf);
            const bool hit = rope_box_hit(q0, q1, jx, jy, jz, mox, moy, moz, tmin, k.lim);
            const bool leaf = (a & NODE_LEAF) != 0;
            const uint32_t child = ((b >> (24 + oct)) & 1u) ? (b & NODE_INDEX_MASK) : a;
            bc = (hit && !leaf) ? child : esc;
            if (hit && leaf) { tri = a & 0x7FFFFFFFu; tri_end = tri + b; }
        }
    }
}

template <Form FORM, class Filter, class Sink>
MRT_DEV void walk(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k, uint32_t *stack) {
    if constexpr (FORM == WIDE) walk_wide(s, vis, o, d, tmin, k, stack);
    else if constexpr (FORM == ROPE) walk_rope(s, vis, o, d, tmin, k);
    else walk_instanced(s, vis, o, d, tmin, k);
}

// ---- records: the ids by closest_record's arithmetic (renderer.hip), u = U / |det|, v = V / |det|.  Q4 is what a record is stored as, twice: uint4 — two 16-byte stores, the
// all-hits rows, 16-byte aligned — or Word4 — words, the closest record, which may lie at any multiple of 4 bytes as the unmasked entry's does.
struct Word4 { uint32_t x, y, z, w; };
template <class Q4> MRT_DEV Q4 four(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { Q4 q; q.x = x; q.y = y; q.z = z; q.w = w; return q; }
template <class Q4>
MRT_DEV void store_miss(Q4 *__restrict__ rec) {          // {0, -1.0f, -1, -1, -1, 0, 0, 0}
    rec[0] = four<Q4>(0u, __float_as_uint(-1.0f), 0xFFFFFFFFu, 0xFFFFFFFFu); rec[1] = four<Q4>(0xFFFFFFFFu, 0u, 0u, 0u);
}
template <class Q4>
MRT_DEV void store_hit(const SceneView &s, Q4 *__restrict__ rec, float t, float U, float V, float ad, uint32_t gid) {
    uint32_t inst, geom;
    if (s.num_inst) { inst = instance_of_gid(s, gid); const InstanceDev &I = s.inst[inst]; geom = s.tri_shade[I.ts_base + (gid - I.gid_base)].w & 0xFFFFu; }
    else { const uint4 ts = s.tri_shade[gid]; inst = ts.w >> 16; geom = ts.w & 0xFFFFu; }
    rec[0] = four<Q4>(1u, __float_as_uint(t), inst, geom);
    rec[1] = four<Q4>(gid - s.geom_base[inst * (uint32_t)s.max_sub + geom], __float_as_uint(U / ad), __float_as_uint(V / ad), 0u);
}
// The row of a ray whose walk is over: the list's entries as records — each winner tested again for its U, V and |det| (retest_winner's way: the walk's own arithmetic, hence
// its bits) — then miss records up to K, then the count.  A record is put together in registers and stored from ONE place, two 16-byte stores that the lanes with a hit and
// the lanes that pad share: stored on either side of the branch it is six narrower stores per slot, 0.08 ms per call at K = 8 on 2^22 rays (§10q).
template <uint32_t STRIDE>
MRT_DEV void emit_list_row(const SceneView &s, const ListSink<STRIDE> &k, const f3 o, const f3 d, uint4 *__restrict__ row, int32_t *__restrict__ count_out) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t j = 0; j < k.K; j++) {
        uint4 rec[2];
        if (j < k.c) {
            const float4 *__restrict__ p = k.pkts + STRIDE * (size_t)list_pk(k.list, lane, j);
            const float4 q0 = p[0];
            float t_, U, V, ad;
            (void)tri_test(q0, p[1], p[2], o, d, 0.0f, __builtin_inff(), t_, U, V, ad);
            store_hit(s, rec, list_t(k.list, lane, j), U, V, ad, __float_as_uint(q0.w));
        } else store_miss(rec);
        row[2u * j] = rec[0]; row[2u * j + 1u] = rec[1];
    }
    *count_out = (int32_t)k.c;
}

}  // namespace
}  // namespace mrt
