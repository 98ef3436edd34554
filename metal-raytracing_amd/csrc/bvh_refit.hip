// bvh_refit.hip — refit of the resident layouts for deformed geometry (same topology, new vertices), for gfx950.
//
// The tree bvh_build.hip made keeps its shape; its packets and boxes follow the vertices.  One enqueue (enqueue_refit) and one recipe per scene form serve the four ways in:
//   a flattened scene (flat_refit_target; apply_refit_result writes its statistics): a commit after mrt_scene_update_mesh alone (bvh_build.hip FlatBuild::refit_resident), and
//     mrt_scene_update_mesh_device / mrt_scene_refit_device (device_refit)
//   a BLAS of a two-level scene (enqueue_blas_refit; fold_blas_stats writes the scene's statistics): a commit, per updated mesh (refit_blas, called by two_level.hip refit_two_level), and
//     mrt_scene_update_blas_device / mrt_scene_refit_blas_device (device_refit_blas)
// The device entries' update calls share one vertex ingest (enqueue_vertex_ingest) and, with the instance moves of tlas_refit.hip, one gate (UpdateGate, retire_gate).
#include "build_common.h"
#include "wide_encode.h"

namespace mrt {
namespace {

// ------------------------------------------------------------------ refit of the 8-wide layout (deformed geometry, same topology: mrt_scene_update_mesh + commit)
// The reference rebuilds nothing per frame (Renderer.swift:184-214 runs once); Metal's refit of a primitive acceleration structure is what this stands for.
// The tree keeps its shape: every packet takes its triangle's new vertices (k_flatten's records, by the id the packet carries), then the levels are walked bottom-up —
// one thread per node: the boxes of its leaf children from their triangles' padded boxes (k_flatten's, the build's own leaves; a pre-split triangle's references all get
// the whole triangle's box), those of its internal children from the level below, the node's grid and the children's planes by the encoder k_wide_level
// built them with (wide_encode.h wide_encode_node).
__global__ void k_refit_wide_packets(const float4 *__restrict__ tri_world, float4 *__restrict__ wpackets, uint32_t n) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t gid = __float_as_uint(wpackets[WPK * (size_t)p].w);
    for (int j = 0; j < 3; j++) wpackets[WPK * (size_t)p + j] = tri_world[3 * (size_t)gid + j];
}
// A leaf child none of whose triangles moved (its instance's mesh was not updated) keeps the box it has — decoded from its planes on the node's old grid: the box the BUILD gave
// that reference, clipped to its slab if the triangle was pre-split (walls and floor: 32 references each; with the whole triangle's box on every one of them the refitted
// DragonScene rendered 14 % slower than a fresh build at a deformation of half a percent of the dragon's size).
__global__ void k_refit_wide_level(float4 *__restrict__ wnodes, const float4 *__restrict__ wpackets, const float4 *__restrict__ tri_lo, const float4 *__restrict__ tri_hi,
                                   const uint4 *__restrict__ tri_shade, const uint8_t *__restrict__ inst_dirty, float4 *__restrict__ nbox, uint32_t first, uint32_t count, double *__restrict__ growth /* [0] += area of the moved leaf children's boxes as they were, [1] += as they are now */) {
    __shared__ double s_g[2];          // (one wave per workgroup) the workgroup's two sums: one pair of global atomics per 64 nodes
    if (threadIdx.x == 0) { s_g[0] = 0.0; s_g[1] = 0.0; }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double g_old = 0.0, g_new = 0.0;
    const size_t w = WNODE_STRIDE * (size_t)(first + i);
    const float4 n0 = wnodes[w], n1 = wnodes[w + 1];
    const uint32_t imask = __float_as_uint(n0.w) >> 24, cbase = __float_as_uint(n1.x), tbase = __float_as_uint(n1.y), meta[2] = {__float_as_uint(n1.z), __float_as_uint(n1.w)};
    const float BIG = 3.0e38f;
    float clo[8][3], chi[8][3]; bool occ[8];
    float nl[3] = {BIG, BIG, BIG}, nh[3] = {-BIG, -BIG, -BIG};
    uint32_t rank = 0; bool any = false;
    for (int sl = 0; sl < 8; sl++) {
        float lo[3] = {BIG, BIG, BIG}, hi[3] = {-BIG, -BIG, -BIG};
        occ[sl] = false;
        if ((imask >> sl) & 1u) {
            const uint32_t c = cbase + rank++;
            const float4 a = nbox[2 * (size_t)c], b = nbox[2 * (size_t)c + 1];
            lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z; occ[sl] = true;
        } else {
            const uint32_t m = (meta[sl >> 2] >> (8 * (sl & 3))) & 0xFFu, cnt = m >> 5, off = m & 31u;
            bool moved = false;
            for (uint32_t r = 0; r < cnt; r++) {
                const uint32_t gid = __float_as_uint(wpackets[WPK * (size_t)(tbase + off + r)].w);
                moved = moved || inst_dirty[tri_shade[gid].w >> 16] != 0;
                const float4 a = tri_lo[gid], b = tri_hi[gid];
                lo[0] = fminf(lo[0], a.x); lo[1] = fminf(lo[1], a.y); lo[2] = fminf(lo[2], a.z);
                hi[0] = fmaxf(hi[0], b.x); hi[1] = fmaxf(hi[1], b.y); hi[2] = fmaxf(hi[2], b.z);
                occ[sl] = true;
            }
            if (cnt != 0u) {          // the box this child has: planes q * 2^e + p on the node's grid as it stands (rounded outwards when they were written)
                const uint32_t ew = __float_as_uint(n0.w);
                const float org[3] = {n0.x, n0.y, n0.z};
                const float4 p2 = wnodes[w + 2], p3 = wnodes[w + 3], p4 = wnodes[w + 4];
                const uint32_t pl[6][2] = {{__float_as_uint(p2.x), __float_as_uint(p2.y)}, {__float_as_uint(p2.z), __float_as_uint(p2.w)}, {__float_as_uint(p3.x), __float_as_uint(p3.y)},
                                           {__float_as_uint(p3.z), __float_as_uint(p3.w)}, {__float_as_uint(p4.x), __float_as_uint(p4.y)}, {__float_as_uint(p4.z), __float_as_uint(p4.w)}};
                float had_lo[3], had_hi[3], now_lo[3], now_hi[3];          // the child's box as it was, and the new one rounded outwards onto the SAME (old) grid: like with like
                for (int a = 0; a < 3; a++) {
                    const float st = __builtin_ldexpf(1.0f, (int)(int8_t)((ew >> (8 * a)) & 0xFFu));
                    const float ql = (float)((pl[a][sl >> 2] >> (8 * (sl & 3))) & 0xFFu), qh = (float)((pl[3 + a][sl >> 2] >> (8 * (sl & 3))) & 0xFFu);
                    // (exact: a plane is p + q * 2^e with q < 256)  Never beyond its triangles' own boxes: a moving sibling changes the node's grid with every refit, and a box
                    // re-rounded outwards onto each new grid would creep; an unsplit triangle's leaf thus keeps exactly its box, a pre-split reference at worst ends at its triangle's
                    had_lo[a] = __builtin_fmaf(ql, st, org[a]); had_hi[a] = __builtin_fmaf(qh, st, org[a]);
                    now_lo[a] = __builtin_fmaf(floorf((lo[a] - org[a]) / st), st, org[a]); now_hi[a] = __builtin_fmaf(ceilf((hi[a] - org[a]) / st), st, org[a]);
                    if (!moved) { lo[a] = fmaxf(lo[a], had_lo[a]); hi[a] = fminf(hi[a], had_hi[a]); }
                }
                if (moved) {          // what the refit does to the moved meshes' leaves: their boxes' area before and after (MRTSceneStats.leaf_growth)
                    const float ox = fmaxf(had_hi[0] - had_lo[0], 0.0f), oy = fmaxf(had_hi[1] - had_lo[1], 0.0f), oz = fmaxf(had_hi[2] - had_lo[2], 0.0f);
                    const float nx_ = fmaxf(now_hi[0] - now_lo[0], 0.0f), ny_ = fmaxf(now_hi[1] - now_lo[1], 0.0f), nz_ = fmaxf(now_hi[2] - now_lo[2], 0.0f);
                    g_old += (double)(ox * oy + oy * oz + oz * ox); g_new += (double)(nx_ * ny_ + ny_ * nz_ + nz_ * nx_);
                }
            }
        }
        for (int a = 0; a < 3; a++) { clo[sl][a] = lo[a]; chi[sl][a] = hi[a]; if (occ[sl]) { nl[a] = fminf(nl[a], lo[a]); nh[a] = fmaxf(nh[a], hi[a]); } }
        any = any || occ[sl];
    }
    if (growth) {          // (the lanes of the wave are together here)
        if (g_new > 0.0) { atomicAdd(&s_g[0], g_old); atomicAdd(&s_g[1], g_new); }
        __syncthreads();
        if (threadIdx.x == 0 && s_g[1] > 0.0) { atomicAdd(&growth[0], s_g[0]); atomicAdd(&growth[1], s_g[1]); }
    }
    if (!any) { nbox[2 * (size_t)(first + i)] = make_float4(n0.x, n0.y, n0.z, 0.0f); nbox[2 * (size_t)(first + i) + 1] = make_float4(n0.x, n0.y, n0.z, 0.0f); return; }      // (a node without children: nothing to move)
    wide_encode_node(wnodes + w, nl, nh, clo, chi, occ, imask);        // the node's grid and the children's planes: k_wide_level's encoder
    nbox[2 * (size_t)(first + i)] = make_float4(nl[0], nl[1], nl[2], 0.0f); nbox[2 * (size_t)(first + i) + 1] = make_float4(nh[0], nh[1], nh[2], 0.0f);
}

// ------------------------------------------------------------------ refit of a rope layout (the BLASes of a two-level scene keep one: the query API and the in-place fallbacks walk it)
// Same topology, new boxes: every internal node notes itself as its children's parent; then one thread per LEAF takes its box from its triangles' padded boxes (by the id each
// packet carries) and climbs — the second thread to arrive at a node (a counter per node) unions the children's boxes and goes on.  The hand-off is k_refit's: 16-byte
// write-through stores, drained before the agent-scope arrival, sc1 loads after it.  The near-child masks are the build's and only order the walk; the escape links are
// the build's too and ARE correctness (a wrong link skips or repeats a subtree for the rays of one octant): the refit must write neither, it rewrites words 3 and 7 of a node
// from the copy k_rope_prepare took and never touches words 8 .. 15 (tests/rope_audit.py links_kept).
__global__ void k_rope_refit(float4 *nodes, uint32_t n, const float4 *__restrict__ packets, const float4 *__restrict__ tri_lo, const float4 *__restrict__ tri_hi,
                             const uint32_t *__restrict__ parent, const uint2 *__restrict__ ab /* per node: its {a, b} words, copied before the pass */, uint32_t *__restrict__ arrived,
                             const uint4 *__restrict__ tri_shade, const uint8_t *__restrict__ inst_dirty /* both or neither: a leaf none of whose triangles' instances moved keeps the box it has (the clipped boxes of pre-split references survive) */) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint2 w = ab[i];
    if (!(w.x & NODE_LEAF)) return;
    const __amdgpu_buffer_rsrc_t rn = refit_rsrc(nodes);
    const float BIG = 3.0e38f;
    float4 lo = make_float4(BIG, BIG, BIG, 0.0f), hi = make_float4(-BIG, -BIG, -BIG, 0.0f);
    bool moved = inst_dirty == nullptr;
    for (uint32_t r = 0; r < w.y; r++) {
        const uint32_t gid = __float_as_uint(packets[3 * (size_t)((w.x & 0x7FFFFFFFu) + r)].w);
        if (inst_dirty) moved = moved || inst_dirty[tri_shade[gid].w >> 16] != 0;
        const float4 l = tri_lo[gid], h = tri_hi[gid];
        lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z); hi.x = fmaxf(hi.x, h.x); hi.y = fmaxf(hi.y, h.y); hi.z = fmaxf(hi.z, h.z);
    }
    if (!moved) { lo = nodes[4 * (size_t)i]; hi = nodes[4 * (size_t)i + 1]; }          // (written by the build or an earlier refit, long before this launch)
    for (;;) {
        lo.w = __uint_as_float(w.x); hi.w = __uint_as_float(w.y);
        refit_st_wt(rn, 4u * i, lo); refit_st_wt(rn, 4u * i + 1u, hi);
        const uint32_t p = parent[i];
        if (p == NONE) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                   // this node's stores have left the CU ...
        const uint32_t old = __hip_atomic_fetch_add(&arrived[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ... before the arrival is counted
        if (old == 0u) return;                       // the sibling subtree finishes this node
        asm volatile("" ::: "memory");
        w = ab[p];
        const uint32_t l = w.x, r = w.y & NODE_INDEX_MASK;
        const float4 llo = refit_ld_wt(rn, 4u * l), lhi = refit_ld_wt(rn, 4u * l + 1u), rlo = refit_ld_wt(rn, 4u * r), rhi = refit_ld_wt(rn, 4u * r + 1u);
        lo = make_float4(fminf(llo.x, rlo.x), fminf(llo.y, rlo.y), fminf(llo.z, rlo.z), 0.0f);
        hi = make_float4(fmaxf(lhi.x, rhi.x), fmaxf(lhi.y, rhi.y), fmaxf(lhi.z, rhi.z), 0.0f);
        i = p;
    }
}
// {a, b} of every rope node, and its children's parent links, in one pass
__global__ void k_rope_prepare(const float4 *__restrict__ nodes, uint32_t n, uint32_t *__restrict__ parent, uint2 *__restrict__ ab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t a = __float_as_uint(nodes[4 * (size_t)i].w), b = __float_as_uint(nodes[4 * (size_t)i + 1].w);
    ab[i] = make_uint2(a, b);
    if (i == 0) parent[0] = NONE;
    if (!(a & NODE_LEAF)) { parent[a] = i; parent[b & NODE_INDEX_MASK] = i; }
}

// SAH cost of the 8-wide tree AS IT LIES IN MEMORY — what a refit changes and the build's sah_cost (the binary tree's) cannot show: the sum over all child boxes, decoded from
// their planes as the traversal decodes them, of area x (c_node for an internal child: one more node visit; c_tri per triangle for a leaf child).  The root's own visit and the
// normalisation by the root's area are the host's (wide_tree_cost).  *sum = that sum; rbox[0 .. 5] = the box of node `root` (the union of its children's boxes), as order-preserving
// uints (f2ord) through atomicMin / atomicMax.
__global__ void k_wide_cost(const float4 *__restrict__ wnodes, uint32_t first, uint32_t count, uint32_t root, float c_node, float c_tri, double *__restrict__ sum, uint32_t *__restrict__ rbox) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double mine = 0.0;
    if (i < count) {
        const size_t w = WNODE_STRIDE * (size_t)(first + i);
        const float4 n0 = wnodes[w], n1 = wnodes[w + 1], p2 = wnodes[w + 2], p3 = wnodes[w + 3], p4 = wnodes[w + 4];
        const uint32_t ew = __float_as_uint(n0.w), imask = ew >> 24, meta[2] = {__float_as_uint(n1.z), __float_as_uint(n1.w)};
        const float org[3] = {n0.x, n0.y, n0.z};
        const uint32_t pl[6][2] = {{__float_as_uint(p2.x), __float_as_uint(p2.y)}, {__float_as_uint(p2.z), __float_as_uint(p2.w)}, {__float_as_uint(p3.x), __float_as_uint(p3.y)},
                                   {__float_as_uint(p3.z), __float_as_uint(p3.w)}, {__float_as_uint(p4.x), __float_as_uint(p4.y)}, {__float_as_uint(p4.z), __float_as_uint(p4.w)}};
        float st[3];
        for (int a = 0; a < 3; a++) st[a] = __builtin_ldexpf(1.0f, (int)(int8_t)((ew >> (8 * a)) & 0xFFu));
        for (int sl = 0; sl < 8; sl++) {
            const uint32_t m = (meta[sl >> 2] >> (8 * (sl & 3))) & 0xFFu, cnt = m >> 5;
            const bool inner = ((imask >> sl) & 1u) != 0u;
            if (!inner && cnt == 0u) continue;
            float lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                lo[a] = __builtin_fmaf((float)((pl[a][sl >> 2] >> (8 * (sl & 3))) & 0xFFu), st[a], org[a]);
                hi[a] = __builtin_fmaf((float)((pl[3 + a][sl >> 2] >> (8 * (sl & 3))) & 0xFFu), st[a], org[a]);
            }
            const float dx = fmaxf(hi[0] - lo[0], 0.0f), dy = fmaxf(hi[1] - lo[1], 0.0f), dz = fmaxf(hi[2] - lo[2], 0.0f);
            const float area = 2.0f * (dx * dy + dy * dz + dz * dx);
            mine += (double)area * (inner ? (double)c_node : (double)c_tri * (double)cnt);
            if (first + i == root) for (int a = 0; a < 3; a++) { atomicMin(&rbox[a], f2ord(lo[a])); atomicMax(&rbox[3 + a], f2ord(hi[a])); }
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine != 0.0) atomicAdd(sum, mine);
}

// diagnostics: how full are the 8-wide nodes?  out[c] = nodes with c children (c = 0..8), out[9] = internal children, out[10] = leaf children, out[11] = triangles
__global__ void k_wide_histogram(const float4 *__restrict__ wnodes, uint32_t n, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 n0 = wnodes[WNODE_STRIDE * (size_t)i], n1 = wnodes[WNODE_STRIDE * (size_t)i + 1];
    const uint32_t imask = __float_as_uint(n0.w) >> 24, meta[2] = {__float_as_uint(n1.z), __float_as_uint(n1.w)};
    uint32_t leaves = 0, tris = 0;
    for (int k = 0; k < 8; k++) { const uint32_t cnt = ((meta[k >> 2] >> (8 * (k & 3))) & 0xFFu) >> 5; if (cnt) { leaves++; tris += cnt; } }
    const uint32_t inner = (uint32_t)__popc(imask);
    atomicAdd(&out[inner + leaves], 1u); atomicAdd(&out[9], inner); atomicAdd(&out[10], leaves); atomicAdd(&out[11], tris);
}

// ------------------------------------------------------------------ vertices from device memory (mrt_scene_update_mesh_device)
// What mrt_scene_update_mesh checks on the host — no NaN, no infinity in a position or a normal — cannot be known here before the whole input is read, and a call whose input
// fails it must change nothing.  So a call is TWO launches on the caller's stream: k_ingest_check reads everything and notes the call's sequence number in words[0] when it
// finds such a value; k_ingest_write, behind it in stream order (the kernel boundary is the grid-wide decision: every store of the first launch is visible to the second),
// writes only when the word does not name this call.  One launch with a grid barrier would save the second read of the input (it comes from L2 for all but the largest
// meshes) at the price of a co-resident grid and a spin; the sequence number instead of a flag means the word is never cleared, so calls queue up without a memset between them.
__device__ __forceinline__ uint32_t not_finite(uint32_t bits) { return ((bits & 0x7F800000u) + 0x00800000u) >> 31; }      // exponent all ones (all_finite, api.cpp)
__global__ void k_ingest_check(const uint8_t *__restrict__ pos, size_t pos_stride, const uint8_t *__restrict__ nrm, size_t nrm_stride, uint32_t nv, uint32_t seq, uint32_t *__restrict__ words) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (v < nv) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(pos + (size_t)v * pos_stride), *n = reinterpret_cast<const uint32_t *>(nrm + (size_t)v * nrm_stride);
        for (int k = 0; k < 3; k++) bad |= not_finite(p[k]) | not_finite(n[k]);
    }
    if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63u) == 0u) atomicExch(&words[0], seq);      // (every wave that finds one writes the same value)
}
// Every flattened instance of the mesh has its own vertex range in g_pos / normals (bvh_build.hip FlatBuild::fill_staging): all of them take the new vertices and are marked dirty.
__global__ void k_ingest_write(const uint8_t *__restrict__ pos, size_t pos_stride, const uint8_t *__restrict__ nrm, size_t nrm_stride, uint32_t nv, uint32_t seq, const uint32_t *words,
                               unsigned long long *__restrict__ rejected, const uint2 *__restrict__ refs, uint32_t nrefs, float *__restrict__ g_pos, float4 *__restrict__ normals, uint8_t *__restrict__ inst_dirty) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (words[0] == seq) { if (v == 0u) atomicAdd(rejected, 1ull); return; }      // the scene keeps what it had; the caller learns of it from mrt_scene_device_updates_rejected
    if (v >= nv) return;
    const float *p = reinterpret_cast<const float *>(pos + (size_t)v * pos_stride), *n = reinterpret_cast<const float *>(nrm + (size_t)v * nrm_stride);
    const float px = p[0], py = p[1], pz = p[2];
    const float4 n4 = make_float4(n[0], n[1], n[2], 0.0f);
    for (uint32_t r = 0; r < nrefs; r++) {
        const uint2 e = refs[r];
        const size_t d = (size_t)e.y + v;
        g_pos[3 * d] = px; g_pos[3 * d + 1] = py; g_pos[3 * d + 2] = pz;
        normals[d] = n4;
        if (v == 0u) inst_dirty[e.x] = 1;
    }
}
// end of a stream-ordered refit: this refit's growth sums into the chained leaf_growth (the host arithmetic of a refitting commit, FlatBuild::refit_resident: the same operations in the same precision), sums cleared
__global__ void k_refit_fold(double *__restrict__ growth, float *__restrict__ leaf_growth) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    const double g0 = growth[0], g1 = growth[1];
    *leaf_growth = *leaf_growth * (g0 > 0.0 ? (float)(g1 / g0) : 1.0f);
    growth[0] = 0.0; growth[1] = 0.0;
}

}  // namespace

// The refit of whatever `tg` names, in the scratch `s`: the 8-wide packets by the id each carries, the 8-wide levels bottom-up, the rope packets, the rope nodes' parent links
// and their boxes.  Five kernels and nothing else — what is cleared before them (growth, arrived), timed around them and read back after them is the caller's.
void enqueue_refit(const RefitTarget &tg, const RefitScratch &s, hipStream_t stream) {
    const int B = 256;
    if (tg.wnodes) {
        hipLaunchKernelGGL(k_refit_wide_packets, dim3(cdiv(tg.packets, B)), dim3(B), 0, stream, s.tri_world, tg.wpackets + WPK * (size_t)tg.wpacket_first, tg.packets);
        for (size_t L = tg.levels; L-- > 0;)
            hipLaunchKernelGGL(k_refit_wide_level, dim3(cdiv(tg.level_count[L], 64)), dim3(64), 0, stream, tg.wnodes, (const float4 *)tg.wpackets, s.tri_lo, s.tri_hi, tg.tri_shade, tg.dirty, s.nbox, tg.level_first[L], tg.level_count[L], s.growth);
    }
    if (tg.rope_packets) {          // the rope layout beside it (rope = 1, a BLAS) or alone (wide = 0): packets by the id they carry, boxes by k_rope_refit
        hipLaunchKernelGGL(k_refit_wide_packets, dim3(cdiv(tg.packets, B)), dim3(B), 0, stream, s.tri_world, tg.rope_packets, tg.packets);
        if (tg.rope_nodes_n) {
            hipLaunchKernelGGL(k_rope_prepare, dim3(cdiv(tg.rope_nodes_n, B)), dim3(B), 0, stream, (const float4 *)tg.rope_nodes, tg.rope_nodes_n, s.parent, s.ab);
            hipLaunchKernelGGL(k_rope_refit, dim3(cdiv(tg.rope_nodes_n, B)), dim3(B), 0, stream, tg.rope_nodes, tg.rope_nodes_n, (const float4 *)tg.rope_packets, s.tri_lo, s.tri_hi, (const uint32_t *)s.parent, (const uint2 *)s.ab, s.arrived,
                               tg.rope_every_leaf ? (const uint4 *)nullptr : tg.tri_shade, tg.rope_every_leaf ? (const uint8_t *)nullptr : tg.dirty);
        }
    }
}

// cost of the subtree of 8-wide nodes [first, first + count) rooted at `root`, per unit of the root's area: (c_node x area(root) + k_wide_cost's sum) / area(root).  Blocks.
int wide_tree_cost(const float4 *wnodes, uint32_t first, uint32_t count, uint32_t root, float c_node, float c_tri, hipStream_t stream, void *scratch32, float *out) {
    *out = 0.0f;
    if (count == 0) return MRT_OK;
    // (its 8 + 24 bytes are the caller's — a piece of the build's arena or of the scene's refit workspace: a hipMalloc / hipFree pair of its own cost more than the kernel, and hipFree waits for the device)
    double *const d_sum = static_cast<double *>(scratch32); uint32_t *const d_box = reinterpret_cast<uint32_t *>(d_sum + 1);
    MRT_HIP(hipMemsetAsync(d_sum, 0, 8, stream));
    MRT_HIP(hipMemcpyAsync(d_box, BOUNDS_EMPTY, sizeof BOUNDS_EMPTY, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_wide_cost, dim3(cdiv(count, 256)), dim3(256), 0, stream, wnodes, first, count, root, c_node, c_tri, d_sum, d_box);
    double h_sum = 0.0; uint32_t h_box[6];
    MRT_HIP(hipMemcpyAsync(&h_sum, d_sum, 8, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipMemcpyAsync(h_box, d_box, sizeof h_box, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    MRT_HIP(hipGetLastError());
    float b[6];
    for (int k = 0; k < 6; k++) b[k] = ord2f(h_box[k]);
    const double dx = std::max(0.0f, b[3] - b[0]), dy = std::max(0.0f, b[4] - b[1]), dz = std::max(0.0f, b[5] - b[2]);
    const double area = 2.0 * (dx * dy + dy * dz + dz * dx);
    *out = area > 0.0 ? (float)((c_node * area + h_sum) / area) : 0.0f;
    return MRT_OK;
}

// What a refit of a flattened scene leaves in the statistics — the one writer, for the refitting commit (FlatBuild::refit_resident) and for the stream-ordered refits
// (resolve_device_refits): the time, the 8-wide tree's cost as it lies now against the build's (MRTSceneStats.wide_cost / wide_cost_built) with sah_cost — the build's
// binary-tree figure — scaled alike, the refits since the build (sc.refits, counted by the caller), leaf_growth and the root box.  `wide`: the 8-wide layout was refitted.  Blocks.
int apply_refit_result(DeviceScene &sc, const BuildOptions &opt, bool wide, float ms, const float4 box[2], float leaf_growth, void *scratch32, hipStream_t stream) {
    sc.stats.build_ms = ms;
    if (wide) { if (int rc = wide_tree_cost(sc.wnodes.p, 0, sc.num_wnodes, 0, opt.wide_cost_node, opt.wide_cost_tri, stream, scratch32, &sc.stats.wide_cost)) return rc; }
    if (sc.stats.wide_cost_built > 0.0f) sc.stats.sah_cost = sc.sah_cost_built * (sc.stats.wide_cost / sc.stats.wide_cost_built);
    sc.stats.refits = sc.refits;
    // the moved meshes' leaf boxes against what they were before this refit, chained over the refits since the build: the view-independent cost above hardly moves when a small,
    // finely tessellated mesh in a large room loosens (DragonScene, 2 % deformation: wide_cost x 1.014, rate x 0.85) — this does
    sc.stats.leaf_growth = leaf_growth;
    set_root_box(sc.root_lo, sc.root_hi, box[0], box[1]);
    return MRT_OK;
}

// What a refit of a flattened scene works on: the resident layouts `layouts` names, whole; a leaf keeps its box unless an instance marked in `dirty` has a triangle in it.
RefitTarget flat_refit_target(const DeviceScene &sc, RefitLayouts layouts, const uint32_t *level_first, const uint8_t *dirty) {
    RefitTarget tg;
    if (layouts.wide) { tg.wnodes = sc.wnodes.p; tg.wpackets = sc.wpackets.p; tg.level_first = level_first; tg.level_count = sc.wide_levels.data(); tg.levels = sc.wide_levels.size(); }
    if (layouts.rope) { tg.rope_nodes = sc.nodes.p; tg.rope_packets = sc.nodes.p + sc.packets_offset; tg.rope_nodes_n = sc.rope_nodes; }          // the rope layout beside it (rope = 1) or alone (wide = 0)
    tg.packets = sc.num_packets; tg.tri_shade = sc.tri_shade.p; tg.dirty = dirty;
    return tg;
}
// ... and of ONE BLAS in a two-level scene's shared arrays, both layouts: the 8-wide levels start at the BLAS's first node (level_first: absolute), its packets at packet_base in both packet arrays; every rope leaf is
// recomputed (the BLAS's one mesh moved), the rope packets are rewritten whether or not the BLAS has rope nodes.  tri_shade and dirty are of the BLAS's own numbering (k_flatten under the identity; one "instance", marked).
static RefitTarget blas_refit_target(const DeviceScene &sc, const BlasRange &br, const uint32_t *level_first, const uint4 *tri_shade, const uint8_t *dirty) {
    RefitTarget tg;
    tg.wnodes = sc.wnodes.p; tg.wpackets = sc.wpackets.p; tg.wpacket_first = br.packet_base; tg.level_first = level_first; tg.level_count = br.wide_levels.data(); tg.levels = br.wide_levels.size();
    tg.rope_nodes = sc.bnodes.p + 4 * (size_t)br.node_base; tg.rope_packets = sc.bnodes.p + sc.bpackets_offset + 3 * (size_t)br.packet_base; tg.rope_nodes_n = br.rope_nodes;
    tg.packets = br.ntri; tg.tri_shade = tri_shade; tg.dirty = dirty; tg.rope_every_leaf = true;
    return tg;
}
// The refit of one BLAS from its object-space geometry on the device: the mesh's triangles by k_flatten under the identity, then enqueue_refit on blas_refit_target.  The one sequence of a refitting commit (refit_blas:
// an arena filled per call) and of the stream-ordered BLAS refit (device_refit_blas: the resident BlasWorkspace); what is cleared before it, timed around it and read back after it is the caller's.
struct BlasRefitInputs {
    const uint32_t *recs; int nrec; const float *pos; const uint32_t *idx; const float4 *cols;      // the BLAS's SubRecs, its mesh's positions and indices, the identity
    uint4 *tri_shade; uint32_t *cbounds; const uint8_t *dirty; RefitScratch scratch; const uint32_t *level_first;      // k_flatten's shading records and centroid bounds (scratch: written, never read), the marked "instance", ...
};
static void enqueue_blas_refit(const DeviceScene &sc, const BlasRange &br, const BlasRefitInputs &in, hipStream_t stream) {
    static_assert(WPK == 3, "k_refit_wide_packets serves both packet arrays at a stride of three float4");
    hipLaunchKernelGGL(k_flatten, dim3(cdiv(br.ntri, 1024)), dim3(1024), 0, stream, reinterpret_cast<const SubRec *>(in.recs), in.nrec, in.pos, in.idx, in.cols, br.ntri, in.scratch.tri_world, in.tri_shade, in.scratch.tri_lo, in.scratch.tri_hi, in.cbounds);
    enqueue_refit(blas_refit_target(sc, br, in.level_first, in.tri_shade, in.dirty), in.scratch, stream);
}

static const float4 ident[4] = {make_float4(1, 0, 0, 0), make_float4(0, 1, 0, 0), make_float4(0, 0, 1, 0), make_float4(0, 0, 0, 0)};      // k_flatten's instance columns for a BLAS: object space
static size_t piece(size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; }      // what a ScratchArena hands out for `bytes`

// The index list and the submesh records of a BLAS's mesh in the BLAS's own numbering (one "instance", vertices from 0), appended to `recs` / `idx` with index offsets
// relative to where this mesh's indices start: what k_flatten reads in refit_blas and in the stream-ordered BLAS refit.  Returns the triangle count.
static size_t blas_geometry(const HostMesh &g, std::vector<SubRec> &recs, std::vector<uint32_t> &idx) {
    const size_t idx0 = idx.size();
    size_t tb = 0;
    for (size_t s = 0; s < g.sub_indices.size(); s++) {
        const auto &ix = g.sub_indices[s];
        if (ix.empty()) continue;
        recs.push_back(SubRec{(uint32_t)tb, (uint32_t)(ix.size() / 3), (uint32_t)(idx.size() - idx0), 0u, 0u, (uint32_t)s});
        idx.insert(idx.end(), ix.begin(), ix.end()); tb += ix.size() / 3;
    }
    return tb;
}

// Refit of ONE BLAS of a two-level scene in the scene's shared arrays (two_level.hip refit_two_level): the mesh's new object-space triangles (k_flatten under the identity),
// the BLAS's packets of both layouts rewritten by the id each carries, its 8-wide nodes [wnode_base, + wnodes) bottom-up level by level (k_refit_wide_level: child and packet
// indices in there are absolute, the triangle arrays are the BLAS's own), its rope nodes by k_rope_refit, its normals.  Leaves the BLAS's root box (object space) in root_lo / root_hi.
int refit_blas(const HostMesh &g, const BlasRange &br, hipStream_t stream, DeviceScene &out, float root_lo[3], float root_hi[3], float *ms_out, float *growth_out) {
    const size_t nv = g.positions.size() / 3, T = br.ntri;
    if (T == 0 || br.wnodes == 0 || g.normals.size() != g.positions.size()) { set_error("refit_blas: nothing to refit"); return MRT_ERR_STATE; }
    std::vector<SubRec> recs; std::vector<uint32_t> idx; idx.reserve(3 * T);
    if (blas_geometry(g, recs, idx) != T) { set_error("refit_blas: the mesh's triangle count changed"); return MRT_ERR_STATE; }
    std::vector<float4> h_nrm(nv);
    for (size_t v = 0; v < nv; v++) h_nrm[v] = make_float4(g.normals[3 * v], g.normals[3 * v + 1], g.normals[3 * v + 2], 0.0f);
    RefitBuffers w;          // (its scratch and its event pair: the host marks are the resident workspaces')
    w.arena.chunk_bytes = ((size_t)T * (48 + 16 + 32 + 12) + nv * 12 + (size_t)out.wnodes.n / WNODE_STRIDE * 32 + (size_t)br.rope_nodes * 16 + ((size_t)1 << 20) + 255) & ~(size_t)255;
    DevBuf<float> d_pos; DevBuf<uint32_t> d_idx, d_recs; DevBuf<float4> cols; DevBuf<uint4> ts_tmp; DevBuf<uint8_t> dirty;
    MRT_HIP(d_pos.alloc_in(w.arena, 3 * nv)); MRT_HIP(d_idx.alloc_in(w.arena, idx.size())); MRT_HIP(d_recs.alloc_in(w.arena, 6 * recs.size())); MRT_HIP(w.cbounds.alloc_in(w.arena, 6)); MRT_HIP(cols.alloc_in(w.arena, 4));
    MRT_HIP(w.tri_world.alloc_in(w.arena, 3 * T)); MRT_HIP(w.tri_lo.alloc_in(w.arena, T)); MRT_HIP(w.tri_hi.alloc_in(w.arena, T)); MRT_HIP(ts_tmp.alloc_in(w.arena, T));
    MRT_HIP(w.nbox.alloc_in(w.arena, 2 * (out.wnodes.n / WNODE_STRIDE))); MRT_HIP(dirty.alloc_in(w.arena, 4));
    MRT_HIP(w.growth.alloc_in(w.arena, 2)); MRT_HIP(hipMemsetAsync(w.growth.p, 0, 16, stream));
    MRT_HIP(w.parent.alloc_in(w.arena, std::max<size_t>(br.rope_nodes, 1))); MRT_HIP(w.arrived.alloc_in(w.arena, std::max<size_t>(br.rope_nodes, 1))); MRT_HIP(w.ab.alloc_in(w.arena, std::max<size_t>(br.rope_nodes, 1)));
    MRT_HIP(hipEventCreate(&w.ev_begin)); MRT_HIP(hipEventCreate(&w.ev_end));
    MRT_HIP(hipMemcpyAsync(d_pos.p, g.positions.data(), 12 * nv, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(d_recs.p, recs.data(), recs.size() * sizeof(SubRec), hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemcpyAsync(cols.p, ident, sizeof ident, hipMemcpyHostToDevice, stream));
    MRT_HIP(hipMemsetAsync(dirty.p, 1, 4, stream));                       // the one "instance" of the BLAS's own triangle arrays moved
    MRT_HIP(hipMemsetAsync(w.cbounds.p, 0, 24, stream));
    MRT_HIP(hipMemsetAsync(w.arrived.p, 0, w.arrived.bytes(), stream));
    MRT_HIP(hipEventRecord(w.ev_begin, stream));
    const std::vector<uint32_t> first = level_first(br.wide_levels, br.wnode_base);
    enqueue_blas_refit(out, br, BlasRefitInputs{d_recs.p, (int)recs.size(), d_pos.p, d_idx.p, cols.p, ts_tmp.p, w.cbounds.p, dirty.p, w.scratch(), first.data()}, stream);
    MRT_HIP(hipEventRecord(w.ev_end, stream));
    MRT_HIP(hipMemcpyAsync(out.normals.p + br.vbase, h_nrm.data(), nv * 16, hipMemcpyHostToDevice, stream));
    float4 h_box[2];
    MRT_HIP(hipMemcpyAsync(h_box, w.nbox.p + 2 * (size_t)br.wnode_base, sizeof h_box, hipMemcpyDeviceToHost, stream));
    double h_growth[2] = {0.0, 0.0};
    MRT_HIP(hipMemcpyAsync(h_growth, w.growth.p, sizeof h_growth, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    if (growth_out) *growth_out = h_growth[0] > 0.0 ? (float)(h_growth[1] / h_growth[0]) : 1.0f;
    MRT_HIP(hipGetLastError());
    float ms = 0; MRT_HIP(hipEventElapsedTime(&ms, w.ev_begin, w.ev_end));
    if (ms_out) *ms_out = ms;
    set_root_box(root_lo, root_hi, h_box[0], h_box[1]);
    return MRT_OK;
}

int wide_histogram(const DeviceScene &sc, hipStream_t stream, uint32_t out12[12]) {
    memset(out12, 0, 48);
    if (sc.num_wnodes == 0) return MRT_OK;
    DevBuf<uint32_t> d; MRT_HIP(d.alloc(12));
    MRT_HIP(hipMemsetAsync(d.p, 0, 48, stream));
    hipLaunchKernelGGL(k_wide_histogram, dim3(cdiv(sc.num_wnodes, 256)), dim3(256), 0, stream, sc.wnodes.p, sc.num_wnodes, d.p);
    MRT_HIP(hipMemcpyAsync(out12, d.p, 48, hipMemcpyDeviceToHost, stream));
    MRT_HIP(hipStreamSynchronize(stream));
    return MRT_OK;
}

// which of the resident layouts a refit works on: the one predicate of a refitting commit (bvh_build.hip FlatBuild::choose_refit) and of the stream-ordered refit (which keeps the answer in its workspace)
RefitLayouts refit_layouts(const DeviceScene &sc, const BuildOptions &opt) {
    RefitLayouts l;
    l.wide = opt.wide && sc.num_wnodes != 0 && sc.wnodes.p && sc.wpackets.p && !sc.wide_levels.empty();
    l.rope = sc.nodes.p != nullptr && sc.rope_nodes != 0;
    return l;
}

// ------------------------------------------------------------------ the stream-ordered refit (mrt_scene_update_mesh_device / mrt_scene_refit_device)
// The refit of a commit (bvh_build.hip FlatBuild::refit_resident) with nothing of the host in it: the vertices are already in g_pos / normals (k_ingest_write), the dirty bytes already on the device, the scratch the
// scene's own (RefitWorkspace), the launch parameters of every level from the host's wide_levels.  What the blocking path reads back at once — the growth sums, the root box,
// the event pair, the tree's cost — stays on the device until somebody asks (resolve_device_refits).
int device_refit_supported(const DeviceScene &sc, const BuildOptions &opt, const char *who) {
    const uint64_t T = sc.stats.triangles;
    const RefitLayouts there = refit_layouts(sc, opt);
    const bool wide_there = there.wide, rope_there = there.rope;
    const char *why = nullptr;
    if (opt.instancing || sc.num_inst) why = "two-level scenes (instancing = 1) are not refitted by this entry: mrt_scene_update_blas_device + mrt_scene_refit_blas_device deform their meshes";
    else if (!opt.refit) why = "scene option refit = 0: every change builds the tree again (mrt_scene_update_mesh + mrt_scene_commit)";
    else if (T == 0 || sc.refit_triangles != T || !(wide_there || rope_there) || !(wide_there || !opt.wide) || !sc.g_pos.p || !sc.g_idx.p || !sc.g_recs.p || !sc.normals.p || !sc.tri_shade.p)
        why = "the resident tree cannot be refitted (an empty scene, or one that lost its 8-wide layout): mrt_scene_update_mesh + mrt_scene_commit builds it";
    if (!why) return MRT_OK;
    set_error(std::string(who) + ": " + why);
    return MRT_ERR_UNSUPPORTED;
}

void retire_gate(DeviceScene &sc, UpdateGate &gate) {          // a workspace goes: what its gate counted stays with the scene (a count that cannot be read is dropped with the error)
    uint64_t h = 0;
    if (gate.rejected_so_far(&h) == hipSuccess) sc.rejected_before += h; else (void)hipGetLastError();
}
void drop_refit_workspace(DeviceScene &sc) {
    if (sc.refit_ws) retire_gate(sc, sc.refit_ws->gate);
    sc.refit_ws.reset();
}
int refit_workspace_after_commit(DeviceScene &sc) {
    if (!sc.refit_ws) return MRT_OK;
    MRT_HIP(hipMemcpy(sc.refit_ws->leaf_growth.p, &sc.stats.leaf_growth, 4, hipMemcpyHostToDevice));
    MRT_HIP(hipMemset(sc.refit_ws->inst_dirty.p, 0, sc.refit_ws->inst_dirty.bytes()));
    return MRT_OK;
}
void host_vertices_are_newer(DeviceScene &sc, size_t mesh) {
    if (sc.refit_ws && mesh < sc.refit_ws->host_stale.size()) sc.refit_ws->host_stale[mesh] = 0;
    if (sc.blas_ws && mesh < sc.blas_ws->blas_of_mesh.size() && sc.blas_ws->blas_of_mesh[mesh] >= 0) sc.blas_ws->host_stale[(size_t)sc.blas_ws->blas_of_mesh[mesh]] = 0;
}

int device_updates_rejected(DeviceScene &sc, uint64_t *count) {
    *count = sc.rejected_before;
    // every workspace that exists has a gate of its own: set calls refused by k_inst_check (tlas_refit.hip), update calls refused by k_ingest_check for a flattened scene
    // (refit_ws) or for the BLASes of a two-level one (blas_ws)
    for (const UpdateGate *g : {sc.inst_ws ? &sc.inst_ws->gate : nullptr, sc.blas_ws ? &sc.blas_ws->gate : nullptr, sc.refit_ws ? &sc.refit_ws->gate : nullptr}) {
        uint64_t h = 0;
        if (g) MRT_HIP(g->rejected_so_far(&h));
        *count += h;
    }
    return MRT_OK;
}

int device_refit_prepare(const std::vector<HostMesh> &meshes, const BuildOptions &opt, DeviceScene &sc) {
    if (sc.refit_ws) return MRT_OK;
    const size_t I = meshes.size(), T = sc.stats.triangles;
    // where the build (FlatBuild::fill_staging) put every flattened instance's vertices: in mesh order, an instance with its source's count
    std::vector<uint32_t> vbase(I, 0u); size_t V = 0;
    for (size_t mi = 0; mi < I; mi++) { const HostMesh &g = meshes[mi].source >= 0 ? meshes[(size_t)meshes[mi].source] : meshes[mi]; vbase[mi] = (uint32_t)V; V += g.positions.size() / 3; }
    if (sc.g_pos.n != std::max<size_t>(V * 3, 3) || sc.normals.n != std::max<size_t>(V, 1) || sc.stats.instances != (int32_t)I) { set_error("mrt_scene_update_mesh_device: the resident geometry is not this scene's"); return MRT_ERR_STATE; }
    std::unique_ptr<RefitWorkspace> w(new RefitWorkspace());
    w->instances = (uint32_t)I; w->mesh_vbase = vbase; w->layouts = refit_layouts(sc, opt);          // (device_refit_supported has accepted them; the tree stays until the workspace goes)
    w->ref_first.assign(I, 0u); w->ref_count.assign(I, 0u); w->host_stale.assign(I, 0); w->pending.assign(I, 0);
    std::vector<uint2> table; table.reserve(I);
    for (size_t mi = 0; mi < I; mi++) {
        if (meshes[mi].source >= 0) continue;
        w->ref_first[mi] = (uint32_t)table.size();
        for (size_t r = 0; r < I; r++) if (r == mi || meshes[r].source == (int)mi) table.push_back(make_uint2((uint32_t)r, vbase[r]));
        w->ref_count[mi] = (uint32_t)table.size() - w->ref_first[mi];
    }
    w->level_first = level_first(sc.wide_levels, 0u);
    const size_t nw = std::max<uint32_t>(sc.num_wnodes, 1u), nr = std::max<uint32_t>(sc.rope_nodes, 1u);
    // one allocation: 80 B per triangle + 32 B per 8-wide node + 16 B per rope node, every piece below rounded up as the arena hands it out (a piece added below and forgotten
    // here costs a second chunk, nothing else)
    const size_t nref = std::max<size_t>(table.size(), 1), ninst = std::max<size_t>(I, 1);
    w->arena.chunk_bytes = piece(48 * T) + 2 * piece(16 * T) + piece(32 * nw) + 2 * piece(4 * nr) + piece(8 * nr) + piece(sizeof(uint2) * nref) + piece(ninst)
                         + piece(6 * 4) + piece(4 * 4) + piece(6 * 8) + piece(8) + piece(4);
    MRT_HIP(w->tri_world.alloc_in(w->arena, 3 * T)); MRT_HIP(w->tri_lo.alloc_in(w->arena, T)); MRT_HIP(w->tri_hi.alloc_in(w->arena, T)); MRT_HIP(w->nbox.alloc_in(w->arena, 2 * nw));
    MRT_HIP(w->parent.alloc_in(w->arena, nr)); MRT_HIP(w->arrived.alloc_in(w->arena, nr)); MRT_HIP(w->ab.alloc_in(w->arena, nr));
    MRT_HIP(w->ref_table.alloc_in(w->arena, nref)); MRT_HIP(w->inst_dirty.alloc_in(w->arena, ninst));
    MRT_HIP(w->cbounds.alloc_in(w->arena, 6)); MRT_HIP(w->gate.words.alloc_in(w->arena, 4)); MRT_HIP(w->growth.alloc_in(w->arena, 6)); MRT_HIP(w->gate.rejected.alloc_in(w->arena, 1)); MRT_HIP(w->leaf_growth.alloc_in(w->arena, 1));
    MRT_HIP(hipEventCreate(&w->ev_begin)); MRT_HIP(hipEventCreate(&w->ev_end)); MRT_HIP(hipEventCreateWithFlags(&w->gate.ev_last, hipEventDisableTiming));
    if (!table.empty()) MRT_HIP(hipMemcpy(w->ref_table.p, table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice));
    MRT_HIP(hipMemset(w->inst_dirty.p, 0, w->inst_dirty.bytes())); MRT_HIP(hipMemset(w->gate.words.p, 0, w->gate.words.bytes())); MRT_HIP(hipMemset(w->growth.p, 0, w->growth.bytes())); MRT_HIP(hipMemset(w->gate.rejected.p, 0, 8));
    MRT_HIP(hipMemcpy(w->leaf_growth.p, &sc.stats.leaf_growth, 4, hipMemcpyHostToDevice));
    MRT_HIP(hipDeviceSynchronize());          // (the first call after a build may block: from here on the caller's stream finds the workspace as the lines above left it)
    MRT_HIP(hipEventRecord(w->gate.ev_last, nullptr));
    sc.refit_ws = std::move(w);
    return MRT_OK;
}

// One update call's two launches on the caller's stream, the gate's event behind them: nverts rows into dst_pos / normals at every vertex base refs[0 .. nrefs) names, the instances it names marked in `dirty`.  (gate.next() is the caller's.)
struct VertexRows { const void *pos; size_t pos_stride; const void *nrm; size_t nrm_stride; };
static int enqueue_vertex_ingest(UpdateGate &gate, const VertexRows &rows, size_t nverts, const uint2 *refs, uint32_t nrefs, float *dst_pos, float4 *normals, uint8_t *dirty, hipStream_t stream) {
    const uint32_t nv = (uint32_t)nverts;
    const dim3 grid(cdiv(nv, 256)), block(256);
    const uint8_t *pos = static_cast<const uint8_t *>(rows.pos), *nrm = static_cast<const uint8_t *>(rows.nrm);
    hipLaunchKernelGGL(k_ingest_check, grid, block, 0, stream, pos, rows.pos_stride, nrm, rows.nrm_stride, nv, gate.seq, gate.words.p);
    hipLaunchKernelGGL(k_ingest_write, grid, block, 0, stream, pos, rows.pos_stride, nrm, rows.nrm_stride, nv, gate.seq, (const uint32_t *)gate.words.p, gate.rejected.p, refs, nrefs, dst_pos, normals, dirty);
    MRT_HIP(hipGetLastError());
    MRT_HIP(hipEventRecord(gate.ev_last, stream));
    return MRT_OK;
}

int device_update_mesh(DeviceScene &sc, size_t mesh, const void *d_pos, size_t pos_stride, const void *d_nrm, size_t nrm_stride, size_t nverts, hipStream_t stream) {
    RefitWorkspace &ws = *sc.refit_ws;
    ws.gate.next();
    if (nverts != 0 && ws.ref_count[mesh] != 0) { if (int rc = enqueue_vertex_ingest(ws.gate, VertexRows{d_pos, pos_stride, d_nrm, nrm_stride}, nverts, ws.ref_table.p + ws.ref_first[mesh], ws.ref_count[mesh], sc.g_pos.p, sc.normals.p, ws.inst_dirty.p, stream)) return rc; }
    // (set for a call the device refuses too: the host cannot know without a read-back.  The bits on the device are then the old ones, so all it costs is a download of
    // vertices the host already has and a refit of an unchanged mesh at the next commit)
    ws.host_stale[mesh] = 1; ws.pending[mesh] = 1;
    return MRT_OK;
}

int device_refit(DeviceScene &sc, hipStream_t stream) {
    RefitWorkspace &ws = *sc.refit_ws;
    const uint32_t T32 = (uint32_t)sc.stats.triangles;
    const int nrec = (int)(sc.g_recs.n / 6);
    MRT_HIP(hipMemsetAsync(ws.cbounds.p, 0, 24, stream));          // (k_flatten's centroid bounds: written, never read here)
    if (ws.layouts.rope) MRT_HIP(hipMemsetAsync(ws.arrived.p, 0, (size_t)sc.rope_nodes * 4, stream));
    MRT_HIP(hipEventRecord(ws.ev_begin, stream));
    hipLaunchKernelGGL(k_flatten, dim3(cdiv(T32, 1024)), dim3(1024), 0, stream, reinterpret_cast<const SubRec *>(sc.g_recs.p), nrec, (const float *)sc.g_pos.p, (const uint32_t *)sc.g_idx.p, (const float4 *)sc.inst_cols.p, T32,
                       ws.tri_world.p, sc.tri_shade.p, ws.tri_lo.p, ws.tri_hi.p, ws.cbounds.p);
    enqueue_refit(flat_refit_target(sc, ws.layouts, ws.level_first.data(), ws.inst_dirty.p), ws.scratch(), stream);
    hipLaunchKernelGGL(k_refit_fold, dim3(1), dim3(64), 0, stream, ws.growth.p, ws.leaf_growth.p);
    MRT_HIP(hipMemsetAsync(ws.inst_dirty.p, 0, ws.inst_dirty.bytes(), stream));          // the marks are spent
    MRT_HIP(hipEventRecord(ws.ev_end, stream));
    MRT_HIP(hipEventRecord(ws.gate.ev_last, stream));
    MRT_HIP(hipGetLastError());
    std::fill(ws.pending.begin(), ws.pending.end(), 0);
    sc.refits++; ws.unresolved = true;
    return MRT_OK;
}

// The statistics of the refits enqueued since they were last read (apply_refit_result): blocks on the last one's end.
int resolve_device_refits(DeviceScene &sc, const BuildOptions &opt, hipStream_t stream) {
    if (!sc.refit_ws || !sc.refit_ws->unresolved) return MRT_OK;
    RefitWorkspace &ws = *sc.refit_ws;
    const bool wide_there = ws.layouts.wide;
    MRT_HIP(hipEventSynchronize(ws.ev_end));
    float ms = 0; MRT_HIP(hipEventElapsedTime(&ms, ws.ev_begin, ws.ev_end));
    float4 h_box[2]; float h_growth = 1.0f;
    MRT_HIP(hipMemcpy(h_box, wide_there ? ws.nbox.p : sc.nodes.p, sizeof h_box, hipMemcpyDeviceToHost));
    MRT_HIP(hipMemcpy(&h_growth, ws.leaf_growth.p, 4, hipMemcpyDeviceToHost));
    if (int rc = apply_refit_result(sc, opt, wide_there, ms, h_box, h_growth, ws.growth.p + 2, stream)) return rc;
    ws.unresolved = false;
    return MRT_OK;
}

static int download_mesh_vertices(HostMesh &m, const float *d_pos, const float4 *d_nrm) {          // a mesh's host copy from where the device keeps its vertices (packed positions, float4 normals); blocks
    const size_t nv = m.positions.size() / 3;
    if (!nv) return MRT_OK;
    std::vector<float4> n4(nv);
    MRT_HIP(hipMemcpy(m.positions.data(), d_pos, nv * 12, hipMemcpyDeviceToHost));
    MRT_HIP(hipMemcpy(n4.data(), d_nrm, nv * 16, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < nv; v++) { m.normals[3 * v] = n4[v].x; m.normals[3 * v + 1] = n4[v].y; m.normals[3 * v + 2] = n4[v].z; }
    return MRT_OK;
}

// The scene's host copy of a mesh is stale once its vertices were replaced on the device: whoever reads HostMesh::positions / normals (a commit, the replication of a scene
// for a device group) calls this first.  A mesh updated and not yet refitted counts as changed for the commit that follows.
int download_stale_meshes(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *pending_found) {
    if (pending_found) *pending_found = false;
    if (!sc.refit_ws) return MRT_OK;
    RefitWorkspace &ws = *sc.refit_ws;
    // meshes are only ever appended (mrt_scene_add_mesh / _add_instance / _add_obj), and the resident arrays keep their layout until the next build: the meshes the workspace
    // knows are the first host_stale.size() of the scene, whatever was added behind them since
    const size_t known = std::min(ws.host_stale.size(), meshes.size());
    bool waited = false;
    for (size_t mi = 0; mi < known; mi++) {
        if (ws.pending[mi]) { meshes[mi].dirty = true; ws.pending[mi] = 0; if (pending_found) *pending_found = true; }
        if (!ws.host_stale[mi]) continue;
        if (!waited) { MRT_HIP(hipEventSynchronize(ws.gate.ev_last)); waited = true; }
        if (int rc = download_mesh_vertices(meshes[mi], sc.g_pos.p + 3 * (size_t)ws.mesh_vbase[mi], sc.normals.p + ws.mesh_vbase[mi])) return rc;
        ws.host_stale[mi] = 0;
    }
    return MRT_OK;
}

// ------------------------------------------------------------------ meshes of two-level scenes deformed on the stream (mrt_scene_update_blas_device / mrt_scene_refit_blas_device)
// refit_two_level with nothing of the host in it.  The vertices of a mesh exist once, in its BLAS: k_ingest_write puts them into the workspace's resident positions and the
// scene's normals (a one-row reference table per BLAS).  The refit then runs refit_blas's sequence (enqueue_blas_refit) per updated BLAS, from the resident geometry — so nodes and packets
// come out as a refitting commit leaves them —, hands the new root box to the BLAS's instances (tlas_refit.hip k_blas_instance_boxes) and refits both TLAS forms with their
// topology kept (device_refit_instances).  What the host path reads back at once — root boxes, growth sums, the trees' costs — waits on the device for resolve_blas_refits.
int blas_device_supported(const DeviceScene &sc, const BuildOptions &opt, size_t meshes, const char *who) {
    const char *why = nullptr;
    if (!opt.instancing || sc.num_inst == 0)
        why = "flattened scenes (instancing = 0) have no BLAS: mrt_scene_update_mesh_device + mrt_scene_refit_device refit them";
    else if (!opt.refit) why = "scene option refit = 0: every change builds the scene again (mrt_scene_update_mesh + mrt_scene_commit)";
    else if (!two_level_refittable(sc, meshes) || !sc.normals.p || !sc.bnodes.p || !sc.inst_box.p)
        why = "the scene's BLASes cannot be refitted (not every one has the 8-wide layout, e.g. wide = 0): mrt_scene_update_mesh + mrt_scene_commit builds them";
    if (!why) return MRT_OK;
    set_error(std::string(who) + ": " + why);
    return MRT_ERR_UNSUPPORTED;
}

void drop_blas_workspace(DeviceScene &sc) {
    if (sc.blas_ws) retire_gate(sc, sc.blas_ws->gate);
    sc.blas_ws.reset();
}

int blas_device_prepare(const std::vector<HostMesh> &meshes, DeviceScene &sc) {
    if (sc.blas_ws) return MRT_OK;
    const size_t B = sc.blas_ranges.size(), I = sc.h_inst.size();
    std::unique_ptr<BlasWorkspace> w(new BlasWorkspace());
    w->blas_of_mesh.assign(meshes.size(), -1);
    w->idx_first.assign(B, 0u); w->rec_first.assign(B, 0u); w->rec_count.assign(B, 0u); w->inst_first.assign(B, 0u); w->inst_count.assign(B, 0u); w->level_first.resize(B);
    w->host_stale.assign(B, 0); w->pending.assign(B, 0); w->refitted.assign(B, 0);
    // the host copies are truthful here (a commit is behind us and nothing changed since): every BLAS's geometry as refit_blas would upload it
    std::vector<SubRec> recs; std::vector<uint32_t> idx; std::vector<uint2> table(std::max<size_t>(B, 1), make_uint2(0u, 0u)); std::vector<float> lg(std::max<size_t>(B, 1), 1.0f);
    size_t V = 0, maxT = 1, maxR = 1;
    for (size_t b = 0; b < B; b++) {
        const BlasRange &r = sc.blas_ranges[b];
        const HostMesh &g = meshes[r.src_mesh];
        const size_t nv = g.positions.size() / 3;
        w->blas_of_mesh[r.src_mesh] = (int)b;
        w->idx_first[b] = (uint32_t)idx.size(); w->rec_first[b] = (uint32_t)recs.size();
        if (blas_geometry(g, recs, idx) != r.ntri || g.normals.size() != g.positions.size()) { set_error("mrt_scene_update_blas_device: the resident BLASes are not this scene's"); return MRT_ERR_STATE; }
        w->rec_count[b] = (uint32_t)recs.size() - w->rec_first[b];
        w->level_first[b] = level_first(r.wide_levels, r.wnode_base);
        table[b] = make_uint2(0u, r.vbase); lg[b] = r.leaf_growth;
        V = std::max(V, (size_t)r.vbase + nv); maxT = std::max<size_t>(maxT, r.ntri); maxR = std::max<size_t>(maxR, r.rope_nodes);
    }
    if (V > sc.normals.n) { set_error("mrt_scene_update_blas_device: the resident normals are not this scene's"); return MRT_ERR_STATE; }
    std::vector<float> h_pos(std::max<size_t>(3 * V, 3), 0.0f);
    for (size_t b = 0; b < B; b++) { const HostMesh &g = meshes[sc.blas_ranges[b].src_mesh]; if (!g.positions.empty()) memcpy(&h_pos[3 * (size_t)sc.blas_ranges[b].vbase], g.positions.data(), g.positions.size() * 4); }
    std::vector<uint32_t> list(std::max<size_t>(I, 1), 0u);          // the instances grouped by BLAS (InstanceDev::blas is the build's: it stays until the next build)
    for (size_t i = 0; i < I; i++) if (sc.h_inst[i].blas < B) w->inst_count[sc.h_inst[i].blas]++;
    for (size_t b = 1; b < B; b++) w->inst_first[b] = w->inst_first[b - 1] + w->inst_count[b - 1];
    { std::vector<uint32_t> at = w->inst_first; for (size_t i = 0; i < I; i++) if (sc.h_inst[i].blas < B) list[at[sc.h_inst[i].blas]++] = (uint32_t)i; }
    const size_t nw = std::max<size_t>(sc.wnodes.n / WNODE_STRIDE, 1), nrec = std::max<size_t>(recs.size(), 1), nidx = std::max<size_t>(idx.size(), 3);
    w->arena.chunk_bytes = piece(4 * h_pos.size()) + piece(4 * nidx) + piece(sizeof(SubRec) * nrec) + piece(64) + piece(48 * maxT) + 3 * piece(16 * maxT) + piece(32 * nw) + 2 * piece(4 * maxR) + piece(8 * maxR)
                         + piece(8 * table.size()) + piece(4 * list.size()) + piece(6 * 4) + piece(4 * 4) + piece(8 * (2 * B + 4)) + piece(8) + piece(4 * lg.size()) + piece(4);
    MRT_HIP(w->pos.alloc_in(w->arena, h_pos.size())); MRT_HIP(w->idx.alloc_in(w->arena, nidx)); MRT_HIP(w->recs.alloc_in(w->arena, 6 * nrec)); MRT_HIP(w->cols.alloc_in(w->arena, 4));
    MRT_HIP(w->tri_world.alloc_in(w->arena, 3 * maxT)); MRT_HIP(w->tri_lo.alloc_in(w->arena, maxT)); MRT_HIP(w->tri_hi.alloc_in(w->arena, maxT)); MRT_HIP(w->tri_shade.alloc_in(w->arena, maxT));
    MRT_HIP(w->nbox.alloc_in(w->arena, 2 * nw)); MRT_HIP(w->parent.alloc_in(w->arena, maxR)); MRT_HIP(w->arrived.alloc_in(w->arena, maxR)); MRT_HIP(w->ab.alloc_in(w->arena, maxR));
    MRT_HIP(w->ref_table.alloc_in(w->arena, table.size())); MRT_HIP(w->inst_list.alloc_in(w->arena, list.size()));
    MRT_HIP(w->cbounds.alloc_in(w->arena, 6)); MRT_HIP(w->gate.words.alloc_in(w->arena, 4)); MRT_HIP(w->growth.alloc_in(w->arena, 2 * B + 4)); MRT_HIP(w->gate.rejected.alloc_in(w->arena, 1));
    MRT_HIP(w->leaf_growth.alloc_in(w->arena, lg.size())); MRT_HIP(w->dirty.alloc_in(w->arena, 4));
    MRT_HIP(hipEventCreate(&w->ev_begin)); MRT_HIP(hipEventCreate(&w->ev_end)); MRT_HIP(hipEventCreateWithFlags(&w->gate.ev_last, hipEventDisableTiming));
    MRT_HIP(hipMemcpy(w->pos.p, h_pos.data(), h_pos.size() * 4, hipMemcpyHostToDevice));
    if (!idx.empty()) MRT_HIP(hipMemcpy(w->idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    if (!recs.empty()) MRT_HIP(hipMemcpy(w->recs.p, recs.data(), recs.size() * sizeof(SubRec), hipMemcpyHostToDevice));
    MRT_HIP(hipMemcpy(w->cols.p, ident, sizeof ident, hipMemcpyHostToDevice));
    MRT_HIP(hipMemcpy(w->ref_table.p, table.data(), table.size() * sizeof(uint2), hipMemcpyHostToDevice));
    MRT_HIP(hipMemcpy(w->inst_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    MRT_HIP(hipMemcpy(w->leaf_growth.p, lg.data(), lg.size() * 4, hipMemcpyHostToDevice));
    MRT_HIP(hipMemset(w->dirty.p, 1, 4)); MRT_HIP(hipMemset(w->gate.words.p, 0, w->gate.words.bytes())); MRT_HIP(hipMemset(w->growth.p, 0, w->growth.bytes())); MRT_HIP(hipMemset(w->gate.rejected.p, 0, 8));
    MRT_HIP(hipDeviceSynchronize());          // (the first call after a commit may block: from here on the caller's stream finds the workspace as the lines above left it)
    MRT_HIP(hipEventRecord(w->gate.ev_last, nullptr));
    sc.blas_ws = std::move(w);
    return MRT_OK;
}

int device_update_blas(DeviceScene &sc, size_t blas, const void *d_pos, size_t pos_stride, const void *d_nrm, size_t nrm_stride, size_t nverts, hipStream_t stream) {
    BlasWorkspace &ws = *sc.blas_ws;
    ws.gate.next();
    if (int rc = enqueue_vertex_ingest(ws.gate, VertexRows{d_pos, pos_stride, d_nrm, nrm_stride}, nverts, ws.ref_table.p + blas, 1u, ws.pos.p, sc.normals.p, ws.dirty.p, stream)) return rc;
    ws.host_stale[blas] = 1; ws.pending[blas] = 1;          // (for a call the device refuses too, as device_update_mesh)
    return MRT_OK;
}

int device_refit_blas(DeviceScene &sc, hipStream_t stream) {
    BlasWorkspace &ws = *sc.blas_ws;
    MRT_HIP(hipEventRecord(ws.ev_begin, stream));
    for (size_t b = 0; b < sc.blas_ranges.size(); b++) {
        if (!ws.pending[b]) continue;
        const BlasRange &br = sc.blas_ranges[b];
        MRT_HIP(hipMemsetAsync(ws.cbounds.p, 0, 24, stream));          // (k_flatten's centroid bounds: written, never read here)
        if (br.rope_nodes) MRT_HIP(hipMemsetAsync(ws.arrived.p, 0, (size_t)br.rope_nodes * 4, stream));
        enqueue_blas_refit(sc, br, BlasRefitInputs{ws.recs.p + 6 * (size_t)ws.rec_first[b], (int)ws.rec_count[b], ws.pos.p + 3 * (size_t)br.vbase, ws.idx.p + ws.idx_first[b], ws.cols.p, ws.tri_shade.p, ws.cbounds.p,
                                                   ws.dirty.p, ws.scratch(2 * b), ws.level_first[b].data()}, stream);
        hipLaunchKernelGGL(k_refit_fold, dim3(1), dim3(64), 0, stream, ws.growth.p + 2 * b, ws.leaf_growth.p + b);
        enqueue_blas_instance_boxes(sc, ws.nbox.p, br.wnode_base, ws.inst_list.p + ws.inst_first[b], ws.inst_count[b], stream);
        MRT_HIP(hipGetLastError());
        ws.pending[b] = 0; ws.refitted[b] = 1;
    }
    if (int rc = device_refit_instances(sc, stream)) return rc;          // both TLAS forms follow the instances' world boxes (and whatever poses were set since the last refit)
    MRT_HIP(hipEventRecord(ws.ev_end, stream));
    MRT_HIP(hipEventRecord(ws.gate.ev_last, stream));
    sc.refits++; ws.unresolved = true;
    return MRT_OK;
}

// The scene's figures after BLAS refits, from the BlasRanges in their order: the loosest BLAS's chained leaf_growth, the mean of the trees' costs as they lie now and of their build-time SAH figures scaled alike (double
// sums, float results), the refits so far (counted by the caller) and their time.  The one writer, for the refitting commit (two_level.hip refit_two_level) and for the stream-ordered refits (resolve_blas_refits).
void fold_blas_stats(DeviceScene &sc, float ms) {
    float growth_max = 1.0f; double sah = 0, wcost = 0;
    for (const BlasRange &r : sc.blas_ranges) { growth_max = std::max(growth_max, r.leaf_growth); wcost += r.wide_cost; sah += r.wide_cost_built > 0.0f ? r.sah_cost_built * (r.wide_cost / r.wide_cost_built) : r.sah_cost_built; }
    const size_t B = sc.blas_ranges.size();
    sc.stats.build_ms = ms; sc.stats.wide_cost = (float)(wcost / (double)B); sc.stats.sah_cost = (float)(sah / (double)B);
    sc.stats.refits = sc.refits; sc.stats.leaf_growth = growth_max;
}

// What refit_two_level reads back at once, read when somebody asks: per refitted BLAS its root box (update_tlas builds the next TLAS from blas_lo / blas_hi), its chained
// leaf_growth and its tree's cost as it lies now; then the scene's figures by refit_two_level's fold (fold_blas_stats).  Blocks on the last refit's end.
// wide_tree_cost runs on the context's stream, ordered behind the caller's stream only by the host's wait for ev_end: that rests on no refit being enqueued between the wait
// and the cost kernel (the caller owes it: one thread drives a scene), and on update calls touching neither wnodes nor the cost words — they write pos and normals only.
int resolve_blas_refits(DeviceScene &sc, const BuildOptions &opt, hipStream_t stream) {
    if (!sc.blas_ws || !sc.blas_ws->unresolved) return MRT_OK;
    BlasWorkspace &ws = *sc.blas_ws;
    const size_t B = sc.blas_ranges.size();
    MRT_HIP(hipEventSynchronize(ws.ev_end));
    float ms = 0; MRT_HIP(hipEventElapsedTime(&ms, ws.ev_begin, ws.ev_end));
    for (size_t b = 0; b < B; b++) {
        BlasRange &r = sc.blas_ranges[b];
        if (ws.refitted[b]) {
            float4 h_box[2];
            MRT_HIP(hipMemcpy(h_box, ws.nbox.p + 2 * (size_t)r.wnode_base, sizeof h_box, hipMemcpyDeviceToHost));
            MRT_HIP(hipMemcpy(&r.leaf_growth, ws.leaf_growth.p + b, 4, hipMemcpyDeviceToHost));
            set_root_box(&sc.blas_lo[3 * b], &sc.blas_hi[3 * b], h_box[0], h_box[1]);
            if (int rc = wide_tree_cost(sc.wnodes.p, r.wnode_base, r.wnodes, r.wnode_base, opt.wide_cost_node, opt.wide_cost_tri, stream, ws.growth.p + 2 * B, &r.wide_cost)) return rc;
            ws.refitted[b] = 0;
        }
    }
    fold_blas_stats(sc, ms);
    ws.unresolved = false;
    return MRT_OK;
}

// download_stale_meshes for a two-level scene: the HostMesh copies of meshes updated on the device, from the workspace's positions and the scene's normals.  A mesh updated
// and not refitted since counts as changed for the commit that follows (refit_two_level then refits it from the host copy this call brings up to date).
int download_stale_blas_meshes(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *pending_found) {
    if (pending_found) *pending_found = false;
    if (!sc.blas_ws) return MRT_OK;
    BlasWorkspace &ws = *sc.blas_ws;
    bool waited = false;
    for (size_t b = 0; b < sc.blas_ranges.size() && b < ws.host_stale.size(); b++) {
        const BlasRange &r = sc.blas_ranges[b];
        if (r.src_mesh >= meshes.size()) continue;
        HostMesh &m = meshes[r.src_mesh];
        if (ws.pending[b]) { m.dirty = true; ws.pending[b] = 0; if (pending_found) *pending_found = true; }
        if (!ws.host_stale[b]) continue;
        if (!waited) { MRT_HIP(hipEventSynchronize(ws.gate.ev_last)); waited = true; }
        if (int rc = download_mesh_vertices(m, ws.pos.p + 3 * (size_t)r.vbase, sc.normals.p + r.vbase)) return rc;
        ws.host_stale[b] = 0;
    }
    return MRT_OK;
}

}  // namespace mrt
