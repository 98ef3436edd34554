// multihit.hip — all-hits ray queries on device buffers, ordered on a stream of the caller's (mrt_scene_intersect_all_device): per ray the
// max_hits smallest hits under the key (distance, global triangle id), ascending — the order MRT_CLOSER_HIT already decides ties by — each triangle at most once.
//
//   k_intersect_all<true>    the 8-wide layout: one ray per lane in the form of traverse_wide<false> (it carries tmin), the wave's stack in dynamic LDS
//   k_intersect_all<false>   the rope layout (scene option wide = 0) and the empty scene: traverse<false>'s stackless walk
//
// Both walks are the closest-hit walks with ONE change, their bound: while a ray's list holds fewer than K entries the limit is the ray's max_distance, once it is
// full the limit is the K-th entry's distance.  It goes into tri_test and into the node test exactly where the closest hit's distance goes in those walks; the node
// tests widen it as they widen that distance, so a child entered exactly at the bound — a tie at the K-th distance with a lower id — is still visited.
//
// The candidate list of a wave lies in LDS behind the stack: per slot 64 distances then 64 packet indices ([slot][2][64 lanes]: a wave's access to one slot is 64
// consecutive words, no bank conflict), 512 B per slot, 8 KB at K = 16.  An entry keeps the packet, not U, V and |det|: the emit step tests the K winners again
// with tri_test (retest_winner's way — the same arithmetic, hence the same bits), which costs K packet reads per ray once and saves three words per entry for the
// whole walk.  The id is not kept either: it is needed only where two distances are EQUAL (a shared edge, coincident faces, two references of one pre-split
// triangle), and is then read from the packet.  No private array anywhere: nothing is indexed at run time but LDS.
#include "traverse_wide.h"

namespace mrt {
namespace {

constexpr uint32_t MH_SLOT_WORDS = 128;      // one list slot of a wave: 64 distances, 64 packet indices

MRT_DEV float mh_t(const float *list, uint32_t lane, uint32_t j) { return list[j * MH_SLOT_WORDS + lane]; }
MRT_DEV uint32_t mh_pk(const float *list, uint32_t lane, uint32_t j) { return __float_as_uint(list[j * MH_SLOT_WORDS + 64u + lane]); }
MRT_DEV void mh_set(float *list, uint32_t lane, uint32_t j, float t, uint32_t pk) { list[j * MH_SLOT_WORDS + lane] = t; list[j * MH_SLOT_WORDS + 64u + lane] = __uint_as_float(pk); }

// A hit (t <= lim, so it is not beyond a full list's last entry) goes into the lane's sorted list: the entries above it move up one slot, a full list drops its
// last one.  A candidate equal in distance AND id to an entry is the same triangle met through another reference: dropped.  pkts / STRIDE: the packet array the
// walk reads (the id of an entry is word 3 of its packet).  c: entries held; lim: the walk's bound, lowered to the K-th distance once the list is full.
template <uint32_t STRIDE>
MRT_DEV void mh_insert(float *list, uint32_t lane, const float4 *__restrict__ pkts, uint32_t K, uint32_t &c, float &lim, float t, uint32_t pk, uint32_t gid) {
    uint32_t j = c;      // the candidate's slot: behind every entry with a smaller key
    while (j > 0u) {
        const float tj = mh_t(list, lane, j - 1u);
        if (tj < t) break;
        if (tj == t) {
            const uint32_t gj = __float_as_uint(pkts[STRIDE * (size_t)mh_pk(list, lane, j - 1u)].w);
            if (gj == gid) return;
            if (gj < gid) break;
        }
        j--;
    }
    if (j == K) return;      // as far as the full list's last entry, with a higher id
    for (uint32_t k = c < K ? c : K - 1u; k > j; k--) mh_set(list, lane, k, mh_t(list, lane, k - 1u), mh_pk(list, lane, k - 1u));
    mh_set(list, lane, j, t, pk);
    if (c < K) c++;
    if (c == K) lim = mh_t(list, lane, K - 1u);
}

// traverse_wide<false> (traverse_wide.h) with the list in place of the one closest hit; returns the number of entries.  stack: depth x WIDE_STACK_LEVEL_BYTES of LDS
MRT_DEV uint32_t multihit_wide(const SceneView &s, const f3 o, const f3 d, const float tmin, const float tmax, const uint32_t K, uint32_t *stack, float *list) {
    uint32_t c = 0; float lim = tmax;
    if (s.num_wnodes == 0) return 0u;
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
            if (tri_test(r0, r1, r2, o, d, tmin, lim, t, U, V, ad)) mh_insert<WPK>(list, lane, s.wpackets, K, c, lim, t, pk, __float_as_uint(r0.w));
        } else {
            float4 n0, n1, n2, n3, n4;
            MRT_LOAD_NODE(s, pending, n0, n1, n2, n3, n4);
            have_pending = false;
            uint32_t node_hits, tri_hits;
            wide_node_test(n0, n1, n2, n3, n4, o, ix, iy, iz, nx, ny, nz, oct, tmin, lim, node_hits, tri_hits);
            if ((g_mask >> 8) != 0) { wstack_push(stack, sp, lane, g_base, g_mask); sp++; }     // siblings still to visit
            g_base = __float_as_uint(n1.x); g_mask = (node_hits << 8) | (__float_as_uint(n0.w) >> 24);
            t_base = __float_as_uint(n1.y); t_mask = tri_hits;
        }
    }
    return c;
}

// traverse<false> (traverse.h) with the list; the packets are the rope layout's own copy, indexed from s.packets
MRT_DEV uint32_t multihit_rope(const SceneView &s, const f3 o, const f3 d, const float tmin, const float tmax, const uint32_t K, float *list) {
    uint32_t c = 0; float lim = tmax;
    if (s.num_nodes == 0) return 0u;
    const uint32_t lane = threadIdx.x & 63;
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
            if (tri_test(r0, r1, r2, o, d, tmin, lim, t, U, V, ad)) mh_insert<3u>(list, lane, s.packets, K, c, lim, t, tri - 1u, __float_as_uint(r0.w));
        } else {
            float tx0 = __builtin_fmaf(r0.x, ix, nox), tx1 = __builtin_fmaf(r1.x, ix, nox);
            float ty0 = __builtin_fmaf(r0.y, iy, noy), ty1 = __builtin_fmaf(r1.y, iy, noy);
            float tz0 = __builtin_fmaf(r0.z, iz, noz), tz1 = __builtin_fmaf(r1.z, iz, noz);
            float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tmin));
            float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1)) * 1.0000005f;
            tf = fminf(tf, lim * 1.0000005f);      // the limit widened like the far side, as traverse widens the closest hit's distance
            const uint32_t a = __float_as_uint(r0.w), b = __float_as_uint(r1.w);
            const float escf = esc_lane == 0 ? r2.x : esc_lane == 1 ? r2.y : esc_lane == 2 ? r2.z : r2.w;
            const uint32_t esc = __float_as_uint(escf);
            const bool hit = tn <= tf;
            const bool leaf = (a & NODE_LEAF) != 0;
            const uint32_t child = ((b >> (24 + oct)) & 1u) ? (b & NODE_INDEX_MASK) : a;
            cur = (hit && !leaf) ? child : esc;
            if (hit && leaf) { tri = a & 0x7FFFFFFFu; tri_end = tri + b; }
        }
    }
    return c;
}

// The row of ray i: the list's entries as records — each winner tested again for its U, V and |det| (retest_winner's way), the ids by closest_record's arithmetic
// (flattened scenes), u = U / |det|, v = V / |det| — then miss records up to K, two 16-byte stores per record, then the count.
template <uint32_t STRIDE>
MRT_DEV void mh_emit(const SceneView &s, const float4 *__restrict__ pkts, const float *list, const f3 o, const f3 d, const uint32_t K, const uint32_t c, uint4 *__restrict__ row, int32_t *__restrict__ count_out) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t j = 0; j < K; j++) {
        uint4 a = make_uint4(0u, __float_as_uint(-1.0f), 0xFFFFFFFFu, 0xFFFFFFFFu), b = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);      // {0, -1.0f, -1, -1, -1, 0, 0, 0}
        if (j < c) {
            const float4 *__restrict__ p = pkts + STRIDE * (size_t)mh_pk(list, lane, j);
            const float4 q0 = p[0];
            float t_, U, V, ad;
            (void)tri_test(q0, p[1], p[2], o, d, 0.0f, __builtin_inff(), t_, U, V, ad);
            const uint32_t gid = __float_as_uint(q0.w);
            const uint4 ts = s.tri_shade[gid];
            const uint32_t inst = ts.w >> 16, geom = ts.w & 0xFFFFu;
            a = make_uint4(1u, __float_as_uint(mh_t(list, lane, j)), inst, geom);
            b = make_uint4(gid - s.geom_base[inst * (uint32_t)s.max_sub + geom], __float_as_uint(U / ad), __float_as_uint(V / ad), 0u);
        }
        row[2u * j] = a; row[2u * j + 1u] = b;
    }
    *count_out = (int32_t)c;
}

// lds: WIDE: the wave's stack (stack_words, from the scene's wide-tree depth), then the list (K slots); sized by the host.  `count`: null, or the caller's
// device-side ray count, read once as a uniform scalar load: the rows at and past it are touched in neither output.
template <bool WIDE>
__global__ void __launch_bounds__(64) k_intersect_all(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, const uint32_t *__restrict__ count, const uint32_t K, const uint32_t stack_words,
                                                      uint4 *__restrict__ out, int32_t *__restrict__ counts) {
    extern __shared__ uint32_t lds[];
    if (count) n = min(n, *count);
    if (blockIdx.x * 64u >= n) return;      // a wave without a ray: a uniform branch to the end
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const MRTRay r = rays[i];
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    float *list = reinterpret_cast<float *>(lds + (WIDE ? stack_words : 0u));
    uint4 *row = out + 2u * ((size_t)i * K);
    if (WIDE) {
        const uint32_t c = multihit_wide(s, ro, rd, r.min_distance, r.max_distance, K, lds, list);
        mh_emit<WPK>(s, s.wpackets, list, ro, rd, K, c, row, counts + i);
    } else {
        const uint32_t c = multihit_rope(s, ro, rd, r.min_distance, r.max_distance, K, list);
        mh_emit<3u>(s, s.packets, list, ro, rd, K, c, row, counts + i);
    }
}

}  // namespace

// One launch on the caller's stream, nothing else.  Flattened scenes only (the caller has refused the others); the 8-wide layout where it is resident, as the
// other lane walks choose.
int intersect_all_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, size_t n, int max_hits, void *d_out, void *d_hit_counts, const void *d_count) {
    const uint32_t K = (uint32_t)max_hits, stack_words = sc.num_wnodes ? (uint32_t)sc.wide_depth * (WIDE_STACK_LEVEL_BYTES / 4u) : 0u;
    const size_t lds = (size_t)stack_words * 4u + (size_t)K * MH_SLOT_WORDS * 4u;
    const dim3 grid((uint32_t)((n + 63) / 64));
    if (sc.num_wnodes) hipLaunchKernelGGL(k_intersect_all<true>, grid, dim3(64), lds, stream, sc.view(), static_cast<const MRTRay *>(d_rays), (uint32_t)n, static_cast<const uint32_t *>(d_count), K, stack_words,
                                          static_cast<uint4 *>(d_out), static_cast<int32_t *>(d_hit_counts));
    else hipLaunchKernelGGL(k_intersect_all<false>, grid, dim3(64), lds, stream, sc.view(), static_cast<const MRTRay *>(d_rays), (uint32_t)n, static_cast<const uint32_t *>(d_count), K, stack_words,
                            static_cast<uint4 *>(d_out), static_cast<int32_t *>(d_hit_counts));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
