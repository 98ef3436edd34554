// masked.hip — the three device queries with a visibility mask (mrt_scene_intersect_closest_masked_device / _any_ / _all_): a triangle of mesh m is visible
// to a ray with mask r iff (mesh_masks[m] & r) != 0, and the result is what the unmasked entry returns on a scene that holds the visible meshes only.
//
//   k_masked<WIDE, Q>         flattened scenes with the 8-wide layout: one ray per lane in the form of traverse_wide<ANY> (it carries tmin), the wave's stack in dynamic LDS
//   k_masked<ROPE, Q>         the rope layout (scene option wide = 0) and the empty scene: traverse<ANY>'s stackless walk
//   k_masked<INSTANCED, Q>    two-level scenes: traverse_instanced's flat loop; Q = closest, any
//
// The walks are restated here, as multihit.hip restates them, so that no existing kernel's code changes; each is written ONCE for the three queries.  What a query does with a
// hit is its sink: it holds the walk's bound `lim` (what goes into tri_test and into the node tests where the closest hit's distance goes in the walks restated) and takes a
// candidate.  The filter sits in the walk, between the triangle test and the sink: a candidate that passed tri_test is looked up — its global id is word 3 of the packet the
// walk holds, its mesh tri_shade[gid].w >> 16 — and an invisible one is dropped before the sink sees it, so it can neither end an any-hit walk, nor lower a bound, nor decide a
// tie, nor take a list slot.  Two dependent small gathers per ACCEPTED candidate, none per test.  In a two-level scene the instance's mask is tested when its id is taken from
// tlas_index, before the ray is transformed: a skipped instance costs one table read, and nothing inside a BLAS is tested (every triangle of an instance has its mask).
// SceneView and InstanceDev are not changed: the table is one more kernel argument.
#include "traverse_wide.h"

namespace mrt {
namespace {

enum Form : uint32_t { WIDE = 0, ROPE = 1, INSTANCED = 2 };

struct Visibility {
    const uint4 *__restrict__ tri_shade; const uint32_t *__restrict__ mesh_masks; uint32_t ray_mask;
    MRT_DEV bool mesh(uint32_t id) const { return (mesh_masks[id] & ray_mask) != 0u; }
    MRT_DEV bool triangle(uint32_t gid) const { return mesh(tri_shade[gid].w >> 16); }      // flattened scenes: tri_shade is indexed by the global id
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
// The all-hits list of multihit.hip, restated: per slot 64 distances then 64 packet indices in LDS; lim falls to the K-th distance once the list is full; a candidate equal in
// distance and id to an entry is the same triangle met through another reference of a pre-split triangle: dropped.
constexpr uint32_t ML_SLOT_WORDS = 128;
MRT_DEV float ml_t(const float *list, uint32_t lane, uint32_t j) { return list[j * ML_SLOT_WORDS + lane]; }
MRT_DEV uint32_t ml_pk(const float *list, uint32_t lane, uint32_t j) { return __float_as_uint(list[j * ML_SLOT_WORDS + 64u + lane]); }
MRT_DEV void ml_set(float *list, uint32_t lane, uint32_t j, float t, uint32_t pk) { list[j * ML_SLOT_WORDS + lane] = t; list[j * ML_SLOT_WORDS + 64u + lane] = __uint_as_float(pk); }
template <uint32_t STRIDE>
struct ListSink {
    float lim; float *list; const float4 *__restrict__ pkts; uint32_t K; uint32_t c = 0;
    MRT_DEV bool take(float t, float, float, float, uint32_t pk, uint32_t gid) {
        const uint32_t lane = threadIdx.x & 63;
        uint32_t j = c;      // the candidate's slot: behind every entry with a smaller key
        while (j > 0u) {
            const float tj = ml_t(list, lane, j - 1u);
            if (tj < t) break;
            if (tj == t) {
                const uint32_t gj = __float_as_uint(pkts[STRIDE * (size_t)ml_pk(list, lane, j - 1u)].w);
                if (gj == gid) return false;
                if (gj < gid) break;
            }
            j--;
        }
        if (j == K) return false;      // as far as the full list's last entry, with a higher id
        for (uint32_t k = c < K ? c : K - 1u; k > j; k--) ml_set(list, lane, k, ml_t(list, lane, k - 1u), ml_pk(list, lane, k - 1u));
        ml_set(list, lane, j, t, pk);
        if (c < K) c++;
        if (c == K) lim = ml_t(list, lane, K - 1u);
        return false;
    }
};

// ---- walks
// traverse_wide<ANY> (traverse_wide.h); stack: depth x WIDE_STACK_LEVEL_BYTES of LDS
template <class Sink>
MRT_DEV void walk_wide(const SceneView &s, const Visibility &vis, const f3 o, const f3 d, const float tmin, Sink &k, uint32_t *stack) {
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

// traverse<ANY> (traverse.h); the packets are the rope layout's own copy, indexed from s.packets
template <class Sink>
MRT_DEV void walk_rope(const SceneView &s, const Visibility &vis, const f3 o, const f3 d, const float tmin, Sink &k) {
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

// traverse_instanced<ANY> (traverse_instanced.h): one flat loop over TLAS nodes, instance entries, BLAS nodes and triangles.  The candidate's id is the GLOBAL one.
template <class Sink>
MRT_DEV void walk_instanced(const SceneView &s, const Visibility &vis, const f3 o, const f3 d, const float tmin, Sink &k) {
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

template <Form FORM, class Sink>
MRT_DEV void walk(const SceneView &s, const Visibility &vis, const f3 o, const f3 d, const float tmin, Sink &k, uint32_t *stack) {
    if constexpr (FORM == WIDE) walk_wide(s, vis, o, d, tmin, k, stack);
    else if constexpr (FORM == ROPE) walk_rope(s, vis, o, d, tmin, k);
    else walk_instanced(s, vis, o, d, tmin, k);
}

// ---- records: the ids by closest_record's arithmetic (renderer.hip), u = U / |det|, v = V / |det|.  Q4 is what a record is stored as, twice: uint4 — two 16-byte stores, the
// all-hits rows, 16-byte aligned as multihit.hip's — or Word4 — words, the closest record, which may lie at any multiple of 4 bytes as the unmasked entry's does.
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

// One ray per lane.  ray_masks: null (ray_mask holds for every ray), or a word per ray.  count: null, or the caller's device-side ray count, read once as a uniform scalar
// load: the rows at and past it are touched in no output.  lds: WIDE — the wave's stack (stack_words, from the scene's wide-tree depth) —, then MASKED_ALL's list (K slots).
// A lane whose ray sees nothing (mask 0) writes its miss without a walk.
template <Form FORM, MaskedQuery Q>
__global__ void __launch_bounds__(64) k_masked(SceneView s, const uint32_t *__restrict__ mesh_masks, const MRTRay *__restrict__ rays, const uint32_t *__restrict__ ray_masks, const uint32_t ray_mask,
                                               uint32_t n, const uint32_t *__restrict__ count, const uint32_t K, const uint32_t stack_words, void *__restrict__ out, int32_t *__restrict__ counts) {
    extern __shared__ uint32_t lds[];
    if (count) n = min(n, *count);
    if (blockIdx.x * 64u >= n) return;      // a wave without a ray: a uniform branch to the end
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const MRTRay r = rays[i];
    const Visibility vis{s.tri_shade, mesh_masks, ray_masks ? ray_masks[i] : ray_mask};
    const bool blind = vis.ray_mask == 0u;
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    if constexpr (Q == MASKED_ANY) {
        AnySink k{r.max_distance};
        if (!blind) walk<FORM>(s, vis, ro, rd, r.min_distance, k, lds);
        static_cast<int32_t *>(out)[i] = k.hit ? 1 : 0;
    } else if constexpr (Q == MASKED_CLOSEST) {
        ClosestSink k{r.max_distance};
        if (!blind) walk<FORM>(s, vis, ro, rd, r.min_distance, k, lds);
        Word4 *rec = static_cast<Word4 *>(out) + 2u * (size_t)i;
        if (k.gid != 0xFFFFFFFFu) store_hit(s, rec, k.lim, k.U, k.V, k.ad, k.gid); else store_miss(rec);
    } else {
        constexpr uint32_t STRIDE = FORM == WIDE ? WPK : 3u;
        const float4 *__restrict__ pkts = FORM == WIDE ? s.wpackets : s.packets;
        ListSink<STRIDE> k{r.max_distance, reinterpret_cast<float *>(lds + (FORM == WIDE ? stack_words : 0u)), pkts, K};
        if (!blind) walk<FORM>(s, vis, ro, rd, r.min_distance, k, lds);
        const uint32_t lane = threadIdx.x & 63;
        uint4 *row = static_cast<uint4 *>(out) + 2u * ((size_t)i * K);
        for (uint32_t j = 0; j < K; j++) {
            if (j < k.c) {          // the winners tested again for U, V and |det| (retest_winner's way: the walk's own arithmetic, hence its bits)
                const float4 *__restrict__ p = pkts + STRIDE * (size_t)ml_pk(k.list, lane, j);
                const float4 q0 = p[0];
                float t_, U, V, ad;
                (void)tri_test(q0, p[1], p[2], ro, rd, 0.0f, __builtin_inff(), t_, U, V, ad);
                store_hit(s, row + 2u * j, ml_t(k.list, lane, j), U, V, ad, __float_as_uint(q0.w));
            } else store_miss(row + 2u * j);
        }
        counts[i] = (int32_t)k.c;
    }
}

template <Form FORM, MaskedQuery Q>
int launch_masked(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, uint32_t K, void *d_out, void *d_hit_counts, const void *d_count) {
    const uint32_t stack_words = FORM == WIDE ? (uint32_t)sc.wide_depth * (WIDE_STACK_LEVEL_BYTES / 4u) : 0u;
    const size_t lds = (size_t)stack_words * 4u + (Q == MASKED_ALL ? (size_t)K * ML_SLOT_WORDS * 4u : 0u);
    hipLaunchKernelGGL((k_masked<FORM, Q>), dim3((uint32_t)((n + 63) / 64)), dim3(64), lds, stream, sc.view(), sc.mesh_masks.p, static_cast<const MRTRay *>(d_rays),
                       static_cast<const uint32_t *>(d_ray_masks), ray_mask, (uint32_t)n, static_cast<const uint32_t *>(d_count), K, stack_words, d_out, static_cast<int32_t *>(d_hit_counts));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}
template <MaskedQuery Q>
int launch_masked_form(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, uint32_t K, void *d_out, void *d_hit_counts, const void *d_count) {
    if (sc.num_inst) return launch_masked<INSTANCED, Q == MASKED_ALL ? MASKED_CLOSEST : Q>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);      // (MASKED_ALL never comes here: the entry has refused it)
    if (sc.num_wnodes) return launch_masked<WIDE, Q>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);
    return launch_masked<ROPE, Q>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);
}

}  // namespace

// One launch on the caller's stream, nothing else: the 8-wide layout where it is resident, as the other lane walks choose; two-level scenes by the rope walk of both levels.
int intersect_masked_device(const DeviceScene &sc, hipStream_t stream, MaskedQuery query, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, int max_hits, void *d_out,
                            void *d_hit_counts, const void *d_count) {
    if (!sc.mesh_masks.p) { set_error("the scene has no mask table (commit it)"); return MRT_ERR_STATE; }
    if (query == MASKED_ALL && sc.num_inst) { set_error("all-hits queries take flattened scenes only"); return MRT_ERR_UNSUPPORTED; }
    const uint32_t K = (uint32_t)max_hits;
    switch (query) {
    case MASKED_CLOSEST: return launch_masked_form<MASKED_CLOSEST>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);
    case MASKED_ANY: return launch_masked_form<MASKED_ANY>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);
    default: return launch_masked_form<MASKED_ALL>(sc, stream, d_rays, d_ray_masks, ray_mask, n, K, d_out, d_hit_counts, d_count);
    }
}

}  // namespace mrt
