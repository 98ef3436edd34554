// lane_walk.h — what the device queries that are not the render path's need on top of the one-ray-per-lane walks: all hits in order (multihit.hip) and the
// three queries with a visibility mask (masked.hip; §10p).  The walks themselves are their layouts', each written ONCE for every caller (§10q, §10s):
//
//   walk_wide         the 8-wide layout (traverse_wide.h; it carries tmin), the wave's stack in dynamic LDS
//   walk_rope         the rope layout (scene option wide = 0) and the empty scene: the stackless loop (traverse.h)
//   walk_instanced    two-level scenes: the flat loop (traverse_instanced.h)
//
// What a query does with a hit is its SINK: it holds the walk's bound `lim` — what goes into tri_test and into the node tests; both node tests widen it as they widen a box's
// far side, so a child entered exactly at the bound is still visited — and takes a candidate.  Which
// candidates a ray may see is its FILTER.  It sits in the walk, between the triangle test and the sink: a candidate that passed tri_test is looked up — its global id is word 3
// of the packet the walk holds, its mesh tri_shade[gid].w >> 16 — and an invisible one is dropped before the sink sees it, so it can neither end an any-hit walk, nor lower a
// bound, nor decide a tie, nor take a list slot.  Two dependent small gathers per ACCEPTED candidate, none per test.  In a two-level scene the instance's mask is tested when its
// id is taken from tlas_index, before the ray is transformed: a skipped instance costs one table read, and nothing inside a BLAS is tested (every triangle of an instance has
// its mask).  The unmasked queries walk with SeesAll, which is true at compile time.
// traverse<>, traverse_instanced<> and traverse_wide<> are the same walks with SeesAll and the closest or the any sink (traverse.h).  Here: Visibility, the list sink, walk<FORM>
// and the records.
#pragma once
#include "traverse_wide.h"

namespace mrt {
namespace {

enum Form : uint32_t { WIDE = 0, ROPE = 1, INSTANCED = 2 };

// ---- the filter of a masked query (SeesAll: traverse.h)
struct Visibility {
    const uint4 *__restrict__ tri_shade; const uint32_t *__restrict__ mesh_masks; uint32_t ray_mask;
    MRT_DEV bool mesh(uint32_t id) const { return (mesh_masks[id] & ray_mask) != 0u; }
    MRT_DEV bool triangle(uint32_t gid) const { return mesh(tri_shade[gid].w >> 16); }      // flattened scenes: tri_shade is indexed by the global id
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

template <Form FORM, class Filter, class Sink>
MRT_DEV void walk(const SceneView &s, const Filter &vis, const f3 o, const f3 d, const float tmin, Sink &k, uint32_t *stack) {
    if constexpr (FORM == WIDE) walk_wide(s, vis, o, d, tmin, k, stack);
    else if constexpr (FORM == ROPE) walk_rope(s, vis, o, d, tmin, k);
    else walk_instanced(s, vis, o, d, tmin, k);
}

// ---- records: the ids by hit_ids (traverse_instanced.h), u = U / |det|, v = V / |det|.  Q4 is what a record is stored as, twice: uint4 — two 16-byte stores, the
// all-hits rows, 16-byte aligned — or Word4 — words, the closest record, which may lie at any multiple of 4 bytes as the unmasked entry's does.
struct Word4 { uint32_t x, y, z, w; };
template <class Q4> MRT_DEV Q4 four(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { Q4 q; q.x = x; q.y = y; q.z = z; q.w = w; return q; }
template <class Q4>
MRT_DEV void store_miss(Q4 *__restrict__ rec) {          // {0, -1.0f, -1, -1, -1, 0, 0, 0}
    rec[0] = four<Q4>(0u, __float_as_uint(-1.0f), 0xFFFFFFFFu, 0xFFFFFFFFu); rec[1] = four<Q4>(0xFFFFFFFFu, 0u, 0u, 0u);
}
template <class Q4>
MRT_DEV void store_hit(const SceneView &s, Q4 *__restrict__ rec, float t, float U, float V, float ad, uint32_t gid) {
    uint32_t inst, geom, prim;
    hit_ids(s, s.num_inst != 0, gid, inst, geom, prim);
    rec[0] = four<Q4>(1u, __float_as_uint(t), inst, geom);
    rec[1] = four<Q4>(prim, __float_as_uint(U / ad), __float_as_uint(V / ad), 0u);
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
