// tlas_refit.hip — instances of a two-level scene moved from device buffers, ordered on the caller's stream, for gfx950.
//
//   mrt_scene_set_instance_transforms_device   k_inst_check + k_inst_write: new object->world matrices from device memory; per instance its columns (inst_cols), its
//                                              world->object rows (InstanceDev::w2o) and its padded world box (inst_box) rewritten in place — by cofactors_of, rows_of
//                                              and instance_box of instance_math.h, the functions update_tlas (two_level.hip) calls on the host: the host's bits.
//   mrt_scene_refit_instances_device           k_tlas_rope_level per depth, k_tlas_wide_level per level, bottom-up: the boxes of both TLAS forms follow the instances'
//                                              world boxes.  The topology is the last commit's (update_tlas); a commit builds the tree again.
//   mrt_scene_refit_blas_device (bvh_refit.hip)  k_blas_instance_boxes between its BLAS refits and the TLAS refit above: the instances of a refitted BLAS take its new root box.
// The launch boundary is the only grid-wide ordering used here: one launch per depth / level, each over at most a few thousand nodes.
#include "scene_device.h"
#include "instance_math.h"
#include "wide_encode.h"
#include <algorithm>

namespace mrt {
namespace {

inline uint32_t blocks_of(size_t n, size_t per) { return (uint32_t)((n + per - 1) / per); }

__device__ __forceinline__ uint32_t not_finite(uint32_t bits) { return ((bits & 0x7F800000u) + 0x00800000u) >> 31; }      // exponent all ones

// ------------------------------------------------------------------ matrices from device memory
// What mrt_scene_set_instance_transform and update_tlas refuse on the host — a NaN or an infinity anywhere in the 16 floats, a matrix invert_affine does not take — is known here
// only after every matrix was read, and a call that holds one must change nothing: a half-applied pose set is worse than none, and an instance cannot leave the tree without a
// rebuild.  So a call is two launches, as §10d's ingest: k_inst_check notes the call's sequence number in words[0], k_inst_write behind it writes only when the word names another call.
__global__ void k_inst_check(const uint8_t *__restrict__ src, size_t stride, uint32_t count, uint32_t seq, uint32_t *__restrict__ words) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (j < count) {
        const uint32_t *u = reinterpret_cast<const uint32_t *>(src + (size_t)j * stride);
        float xf[16];
        for (int k = 0; k < 16; k++) { bad |= not_finite(u[k]); xf[k] = __uint_as_float(u[k]); }
        if (!bad && !invertible(cofactors_of(xf).det)) bad = 1u;
    }
    if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63u) == 0u) atomicExch(&words[0], seq);      // (every wave that finds one writes the same value)
}
__global__ void k_inst_write(const uint8_t *__restrict__ src, size_t stride, uint32_t first, uint32_t count, uint32_t seq, const uint32_t *words, unsigned long long *__restrict__ rejected,
                             float4 *__restrict__ inst_cols, InstanceDev *__restrict__ inst, float4 *__restrict__ inst_box) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (words[0] == seq) { if (j == 0u) atomicAdd(rejected, 1ull); return; }      // the scene keeps what it had; the caller learns of it from mrt_scene_device_updates_rejected
    if (j >= count) return;
    const size_t i = (size_t)first + j;
    const float *s = reinterpret_cast<const float *>(src + (size_t)j * stride);
    float xf[16];
    for (int k = 0; k < 16; k++) xf[k] = s[k];
    xf[3] = xf[7] = xf[11] = 0.0f; xf[15] = 1.0f;          // (mrt_scene_set_instance_transform forces the last row)
    float rows[3][4];
    rows_of(xf, cofactors_of(xf), rows);
    const float4 blo = inst_box[4 * i], bhi = inst_box[4 * i + 1];          // the root box of its BLAS, object space: resident since the commit
    const float lo_in[3] = {blo.x, blo.y, blo.z}, hi_in[3] = {bhi.x, bhi.y, bhi.z};
    const Box b = instance_box(xf, lo_in, hi_in, rows);
    for (int c = 0; c < 4; c++) inst_cols[4 * i + c] = make_float4(xf[c * 4 + 0], xf[c * 4 + 1], xf[c * 4 + 2], 0.0f);
    for (int r = 0; r < 3; r++) inst[i].w2o[r] = make_float4(rows[r][0], rows[r][1], rows[r][2], rows[r][3]);
    inst_box[4 * i + 2] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f); inst_box[4 * i + 3] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
}

// ------------------------------------------------------------------ a BLAS refitted on the stream (mrt_scene_refit_blas_device)
// Its root box changed, so what update_tlas would compute on the host for each of its instances changes with it: the object box is the BLAS's new root box (the refit's
// nbox[2 * root], as refit_blas reads it back), the padded world box is instance_box (instance_math.h) of it under the instance's CURRENT columns and world->object rows — a pose set by
// k_inst_write is honoured.  An instance outside the TLAS of the last commit (no triangles, a singular matrix then) has the empty box update_tlas gave it, lo > hi, and keeps it.
__global__ void k_blas_instance_boxes(const float4 *__restrict__ nbox, uint32_t root, const uint32_t *__restrict__ inst_list, uint32_t count, const float4 *__restrict__ inst_cols,
                                      const InstanceDev *__restrict__ inst, float4 *__restrict__ inst_box) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const size_t i = inst_list[j];
    if (inst_box[4 * i].x > inst_box[4 * i + 1].x) return;
    const float4 blo = nbox[2 * (size_t)root], bhi = nbox[2 * (size_t)root + 1];
    float xf[16], rows[3][4];
    for (int c = 0; c < 4; c++) { const float4 q = inst_cols[4 * i + c]; xf[c * 4 + 0] = q.x; xf[c * 4 + 1] = q.y; xf[c * 4 + 2] = q.z; xf[c * 4 + 3] = c == 3 ? 1.0f : 0.0f; }
    for (int r = 0; r < 3; r++) { const float4 q = inst[i].w2o[r]; rows[r][0] = q.x; rows[r][1] = q.y; rows[r][2] = q.z; rows[r][3] = q.w; }
    const float lo_in[3] = {blo.x, blo.y, blo.z}, hi_in[3] = {bhi.x, bhi.y, bhi.z};
    const Box b = instance_box(xf, lo_in, hi_in, rows);
    inst_box[4 * i] = make_float4(blo.x, blo.y, blo.z, 0.0f); inst_box[4 * i + 1] = make_float4(bhi.x, bhi.y, bhi.z, 0.0f);
    inst_box[4 * i + 2] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f); inst_box[4 * i + 3] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
}

// ------------------------------------------------------------------ the rope TLAS (nodes, tlas_index): one launch per depth, deepest first
// order[0 .. count): the nodes of one depth.  A leaf takes the union of the world boxes of its one or two instances, an internal node the union of its children's boxes, which
// the launch before this one wrote.  The words a and b, and the escape links, are the build's.
__global__ void k_tlas_rope_level(float4 *__restrict__ nodes, const uint32_t *__restrict__ order, uint32_t count, const uint32_t *__restrict__ tlas_index, const float4 *__restrict__ inst_box) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const size_t n = order[j];
    float4 lo = nodes[4 * n], hi = nodes[4 * n + 1];
    const uint32_t a = __float_as_uint(lo.w), b = __float_as_uint(hi.w);
    const float BIG = 3.0e38f;
    float l[3] = {BIG, BIG, BIG}, h[3] = {-BIG, -BIG, -BIG};
    if (a & NODE_LEAF) {
        const uint32_t first = a & 0x7FFFFFFFu;
        for (uint32_t r = 0; r < b; r++) {
            const size_t i = tlas_index[first + r];
            const float4 ql = inst_box[4 * i + 2], qh = inst_box[4 * i + 3];
            l[0] = fminf(l[0], ql.x); l[1] = fminf(l[1], ql.y); l[2] = fminf(l[2], ql.z); h[0] = fmaxf(h[0], qh.x); h[1] = fmaxf(h[1], qh.y); h[2] = fmaxf(h[2], qh.z);
        }
    } else {
        const size_t c[2] = {a, b & NODE_INDEX_MASK};
        for (int s = 0; s < 2; s++) {
            const float4 ql = nodes[4 * c[s]], qh = nodes[4 * c[s] + 1];
            l[0] = fminf(l[0], ql.x); l[1] = fminf(l[1], ql.y); l[2] = fminf(l[2], ql.z); h[0] = fmaxf(h[0], qh.x); h[1] = fmaxf(h[1], qh.y); h[2] = fmaxf(h[2], qh.z);
        }
    }
    lo.x = l[0]; lo.y = l[1]; lo.z = l[2]; hi.x = h[0]; hi.y = h[1]; hi.z = h[2];
    nodes[4 * n] = lo; nodes[4 * n + 1] = hi;
}

// ------------------------------------------------------------------ the 8-wide TLAS (wnodes[0, tlas_wcap), wtlas_index): one launch per level, deepest first
// One thread per node: the box of a leaf child is its instance's world box, that of an internal child the box the level below left in nbox; the node's origin,
// its power-of-two grid and the children's planes by wide_encode_node, the encoder WideTlasBuilder built them with (wide_encode.h).  Slot assignment, imask, meta, child_base and tri_base stay.
// (The slot loop is k_refit_wide_level's but for the box of a leaf child.  It stays written out in both: as one template over that box each kernel took more registers,
// docs/HISTORY.md §20.)
__global__ void k_tlas_wide_level(float4 *__restrict__ wnodes, const uint32_t *__restrict__ wtlas_index, const float4 *__restrict__ inst_box, float4 *__restrict__ nbox, uint32_t first, uint32_t count) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const size_t node = (size_t)first + j, w = WNODE_STRIDE * node;
    const float4 n0 = wnodes[w], n1 = wnodes[w + 1];
    const uint32_t imask = __float_as_uint(n0.w) >> 24, cbase = __float_as_uint(n1.x), tbase = __float_as_uint(n1.y), meta[2] = {__float_as_uint(n1.z), __float_as_uint(n1.w)};
    const float BIG = 3.0e38f;
    float clo[8][3], chi[8][3]; bool occ[8];
    float nl[3] = {BIG, BIG, BIG}, nh[3] = {-BIG, -BIG, -BIG};
    uint32_t rank = 0; bool any = false;
    for (int sl = 0; sl < 8; sl++) {
        float4 a = make_float4(0, 0, 0, 0), b = a;
        occ[sl] = false;
        if ((imask >> sl) & 1u) {
            const size_t c = (size_t)cbase + rank++;
            a = nbox[2 * c]; b = nbox[2 * c + 1]; occ[sl] = true;
        } else {
            const uint32_t m = (meta[sl >> 2] >> (8 * (sl & 3))) & 0xFFu;
            if (m >> 5) {          // a leaf child of the TLAS is one instance
                const size_t i = wtlas_index[tbase + (m & 31u)];
                a = inst_box[4 * i + 2]; b = inst_box[4 * i + 3]; occ[sl] = true;
            }
        }
        clo[sl][0] = a.x; clo[sl][1] = a.y; clo[sl][2] = a.z; chi[sl][0] = b.x; chi[sl][1] = b.y; chi[sl][2] = b.z;
        if (occ[sl]) for (int k = 0; k < 3; k++) { nl[k] = fminf(nl[k], clo[sl][k]); nh[k] = fmaxf(nh[k], chi[sl][k]); }
        any = any || occ[sl];
    }
    if (!any) { nbox[2 * node] = make_float4(n0.x, n0.y, n0.z, 0.0f); nbox[2 * node + 1] = make_float4(n0.x, n0.y, n0.z, 0.0f); return; }      // (a node without children: nothing to move)
    wide_encode_node(wnodes + w, nl, nh, clo, chi, occ, imask);
    nbox[2 * node] = make_float4(nl[0], nl[1], nl[2], 0.0f); nbox[2 * node + 1] = make_float4(nh[0], nh[1], nh[2], 0.0f);
}

}  // namespace

int instances_device_supported(const DeviceScene &sc, const BuildOptions &opt, const char *who) {
    const char *why = nullptr;
    if (!opt.instancing)
        why = "flattened scenes (instancing = 0) bake their transforms into world-space triangles: mrt_scene_set_instance_transform + mrt_scene_commit builds them again";
    else if (sc.num_inst == 0 || sc.h_inst.size() != sc.num_inst || sc.in_tlas.size() != sc.num_inst || sc.tlas_rope_order.empty())
        why = "the scene has no instance in its TLAS";
    if (!why) return MRT_OK;
    set_error(std::string(who) + ": " + why);
    return MRT_ERR_UNSUPPORTED;
}

void enqueue_blas_instance_boxes(DeviceScene &sc, const float4 *nbox, uint32_t root, const uint32_t *inst_list, uint32_t count, hipStream_t stream) {
    if (count == 0) return;
    hipLaunchKernelGGL(k_blas_instance_boxes, dim3(blocks_of(count, 64)), dim3(64), 0, stream, nbox, root, inst_list, count, (const float4 *)sc.inst_cols.p, (const InstanceDev *)sc.inst.p, sc.inst_box.p);
}

void drop_instance_workspace(DeviceScene &sc) {
    if (sc.inst_ws) retire_gate(sc, sc.inst_ws->gate);
    sc.inst_ws.reset();
}
void host_transform_is_newer(DeviceScene &sc, size_t mesh) { if (sc.inst_ws && mesh < sc.inst_ws->moved.size()) sc.inst_ws->moved[mesh] = 0; }

int instances_device_prepare(DeviceScene &sc) {
    if (sc.inst_ws) return MRT_OK;
    std::unique_ptr<InstanceWorkspace> w(new InstanceWorkspace());
    w->moved.assign(sc.num_inst, 0);
    uint32_t at = 0;
    for (uint32_t n : sc.tlas_rope_levels) { w->rope_first.push_back(at); at += n; }
    at = 0;
    for (uint32_t n : sc.tlas_wide_levels) { w->wide_first.push_back(at); at += n; }
    MRT_HIP(w->gate.words.alloc(4)); MRT_HIP(w->gate.rejected.alloc(1));
    MRT_HIP(w->rope_order.alloc(sc.tlas_rope_order.size())); MRT_HIP(w->nbox.alloc(2 * std::max<size_t>(at, 1)));
    MRT_HIP(hipMemset(w->gate.words.p, 0, w->gate.words.bytes())); MRT_HIP(hipMemset(w->gate.rejected.p, 0, 8));
    if (!sc.tlas_rope_order.empty()) MRT_HIP(hipMemcpy(w->rope_order.p, sc.tlas_rope_order.data(), sc.tlas_rope_order.size() * 4, hipMemcpyHostToDevice));
    // what mrt_scene_rebuild_tlas_device adds (tlas_rebuild.hip): 4 bytes per instance, and 8 more above the LDS limit
    const uint32_t live = sc.tlas_instances;
    if (!sc.tlas_wide_pos.empty()) {
        std::vector<uint32_t> inv(sc.tlas_wide_pos.size());
        for (size_t i = 0; i < inv.size(); i++) inv[sc.tlas_wide_pos[i]] = (uint32_t)i;
        MRT_HIP(w->wide_of_pos.alloc(inv.size()));
        MRT_HIP(hipMemcpy(w->wide_of_pos.p, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
    }
    if (live > TLAS_RESORT_LDS_LIMIT && live <= TLAS_RESORT_MAX) {
        MRT_HIP(w->ids[0].alloc(live)); MRT_HIP(w->ids[1].alloc(live));
        MRT_HIP(w->seg_axis.alloc((live + TLAS_RESORT_LDS_LIMIT - 1) / TLAS_RESORT_LDS_LIMIT));          // (a level handled one step at a time has fewer ranges than that)
    }
    MRT_HIP(hipEventCreateWithFlags(&w->gate.ev_last, hipEventDisableTiming));
    MRT_HIP(hipDeviceSynchronize());          // (the first call after a commit may block: from here on the caller's stream finds the workspace as the lines above left it)
    MRT_HIP(hipEventRecord(w->gate.ev_last, nullptr));
    sc.inst_ws = std::move(w);
    return MRT_OK;
}

int device_set_instance_transforms(DeviceScene &sc, uint32_t first, uint32_t count, const void *d_xf, size_t stride, hipStream_t stream) {
    InstanceWorkspace &ws = *sc.inst_ws;
    const uint32_t seq = ws.gate.next();
    const dim3 grid(blocks_of(count, 64)), block(64);
    hipLaunchKernelGGL(k_inst_check, grid, block, 0, stream, static_cast<const uint8_t *>(d_xf), stride, count, seq, ws.gate.words.p);
    hipLaunchKernelGGL(k_inst_write, grid, block, 0, stream, static_cast<const uint8_t *>(d_xf), stride, first, count, seq, (const uint32_t *)ws.gate.words.p, ws.gate.rejected.p, sc.inst_cols.p, sc.inst.p, sc.inst_box.p);
    MRT_HIP(hipGetLastError());
    MRT_HIP(hipEventRecord(ws.gate.ev_last, stream));
    // (marked for a call the device refuses too: the host cannot know without a read-back, and the columns it then reads back are the ones it has)
    std::fill(ws.moved.begin() + first, ws.moved.begin() + first + count, (uint8_t)1);
    return MRT_OK;
}

int device_refit_instances(DeviceScene &sc, hipStream_t stream) {
    InstanceWorkspace &ws = *sc.inst_ws;
    for (size_t d = sc.tlas_rope_levels.size(); d-- > 0;)
        hipLaunchKernelGGL(k_tlas_rope_level, dim3(blocks_of(sc.tlas_rope_levels[d], 64)), dim3(64), 0, stream, sc.nodes.p, (const uint32_t *)(ws.rope_order.p + ws.rope_first[d]), sc.tlas_rope_levels[d],
                           (const uint32_t *)sc.tlas_index.p, (const float4 *)sc.inst_box.p);
    if (sc.num_wnodes)          // the 8-wide TLAS is resident (update_tlas)
        for (size_t L = sc.tlas_wide_levels.size(); L-- > 0;)
            hipLaunchKernelGGL(k_tlas_wide_level, dim3(blocks_of(sc.tlas_wide_levels[L], 64)), dim3(64), 0, stream, sc.wnodes.p, (const uint32_t *)sc.wtlas_index.p, (const float4 *)sc.inst_box.p, ws.nbox.p,
                               ws.wide_first[L], sc.tlas_wide_levels[L]);
    MRT_HIP(hipGetLastError());
    MRT_HIP(hipEventRecord(ws.gate.ev_last, stream));
    return MRT_OK;
}

// HostMesh::xf of an instance moved on the device is stale: whoever reads it (a commit in all its branches, the replication of a scene for a device group) calls this first.
int download_moved_transforms(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *moved_found) {
    if (moved_found) *moved_found = false;
    if (!sc.inst_ws) return MRT_OK;
    InstanceWorkspace &ws = *sc.inst_ws;
    const size_t known = std::min(ws.moved.size(), meshes.size());          // (meshes are only ever appended)
    if (std::find(ws.moved.begin(), ws.moved.begin() + known, (uint8_t)1) == ws.moved.begin() + known) return MRT_OK;
    MRT_HIP(hipEventSynchronize(ws.gate.ev_last));
    std::vector<float4> cols(4 * known);
    MRT_HIP(hipMemcpy(cols.data(), sc.inst_cols.p, cols.size() * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < known; i++) {
        if (!ws.moved[i]) continue;
        float *xf = meshes[i].xf;
        for (int c = 0; c < 4; c++) { xf[c * 4 + 0] = cols[4 * i + c].x; xf[c * 4 + 1] = cols[4 * i + c].y; xf[c * 4 + 2] = cols[4 * i + c].z; xf[c * 4 + 3] = c == 3 ? 1.0f : 0.0f; }
        ws.moved[i] = 0;
    }
    if (moved_found) *moved_found = true;
    return MRT_OK;
}

}  // namespace mrt
