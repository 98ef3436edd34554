// scene_device.h — HBM data layout of a committed scene, shared by the BVH builder (bvh_build.hip, bvh_refit.hip)
// and the render kernels (renderer.hip, traverse.h, traverse_wide.h).  DESIGN.md §4 documents every array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/mrt_abi.h"

namespace mrt {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define MRT_HIP(call)                                                              \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) return ::mrt::hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

// ---- traversal node: 64 B, one per box ("rope" layout: every node carries, for each of the 8
// ray-direction octants, the node to continue with once its subtree is finished).
//   word 0..2  lo.xyz     word 3  a : leaf ? (NODE_LEAF | first packet) : index of the left child
//   word 4..6  hi.xyz     word 7  b : leaf ? triangle count : (near-mask << 24) | index of the right child
//   word 8..15 esc[8]                 : next node per octant, NODE_TERM = traversal finished
// near-mask bit o = 1 when the RIGHT child is visited first by rays of octant o
// (octant bit k set <=> direction component k negative).
constexpr uint32_t NODE_LEAF = 0x80000000u;
constexpr uint32_t NODE_TERM = 0xFFFFFFFFu;
constexpr uint32_t NODE_INDEX_MASK = 0x00FFFFFFu;

// ---- triangle packet: 48 B, leaf-contiguous, already in world space and in Möller–Trumbore form
//   {v0.xyz, gid} {e1.xyz, -} {e2.xyz, -}
// ---- shading record per global triangle id (16 B): vertex ids into `normals` + (instance<<16 | geometry)

// ---- wide node: 80 B = 5 x float4, eight children with 8-bit quantised boxes (after Ylitie, Karras, Laine
// 2017, "Efficient Incoherent Ray Traversal on GPUs Through Compressed Wide BVHs"):
//   f4 0: origin p.xyz | ex | ey<<8 | ez<<16 | imask<<24      child box = p + q * 2^e (e: int8); imask bit i = child i is a node
//   f4 1: child_base | tri_base | meta[0..3] | meta[4..7]      node child i -> child_base + popc(imask & ((1<<i)-1));
//                                                              leaf child i -> packets tri_base + (meta&31) .. + (meta>>5) - 1
//   f4 2: qlo_x[8] qlo_y[8]      f4 3: qlo_z[8] qhi_x[8]      f4 4: qhi_y[8] qhi_z[8]      (empty slot: qlo=255, qhi=0)
// Slot bit k set = the child lies on the + side of the node centre along axis k, so children are entered
// front to back in the order of (slot ^ ray octant).
// (A six-children-in-64-bytes variant of this node, -DMRT_WIDE6, measured worse in round 4 and was removed in round 6: profiles/r04_wide6_ab.txt.)
#ifndef MRT_WNODE_STRIDE
#define MRT_WNODE_STRIDE 5
#endif
constexpr int WIDE_N = 8;                             // children per wide node
constexpr uint32_t WNODE_STRIDE = MRT_WNODE_STRIDE;   // float4 units between wide nodes in HBM (5 = packed 80 B; 8 = one 128-B line each)
#ifndef MRT_WPACKET_STRIDE
#define MRT_WPACKET_STRIDE 3
#endif
constexpr uint32_t WPK = MRT_WPACKET_STRIDE;          // float4 units between the triangle packets of the 8-wide layout (3 = packed 48 B; 4 = one 64-byte sector each, never straddling two)
constexpr int WIDE_STACK_MAX = 96;   // deepest 8-wide tree the traversal kernels walk: their LDS stack is sized per launch from the scene's depth (320 B per wave and level: 4.2 KB at DragonScene's 13
                                     // levels, 7.7 KB at 24 — five instead of six waves per SIMD —, 30 KB at 96: what a radix tree over 63-bit keys + 26 levels of index splits can need at most); the agglomerative
                                     // builder's deeper trees (a chain of nested triangles) are built again as radix trees (build_flat); only a tree deeper than this keeps the rope layout, and MRTSceneStats::wide_layout says so
constexpr int WIDE_DEPTH_REBUILD = 48;     // an 8-wide tree from the agglomerative builder deeper than this is built again from the radix tree (build_flat)
constexpr int WIDE_STACK_TWO_LEVEL = 30;   // two-level scenes: TLAS levels + 1 (the TLAS group parked at instance entry) + the deepest BLAS; 5-bit depth fields
constexpr uint32_t WIDE_WORLD_RAY_BYTES = 6 * 64 * 4;   // two-level stream traversal: the world-space ray of every lane (o.xyz, d.xyz) parked in LDS in front of the stack
constexpr uint32_t WIDE_STACK_LEVEL_BYTES = 320;   // per wave and level: 64 x 4 B {child_base << 8 | hit bits} + 64 x 1 B {imask}

struct LightDev {            // 96 B, derived once per mrt_scene_set_lights from the 128-B MRTLight
    float4 position;         // .w = type (as int bits)
    float4 color;
    float4 forward;          // area light (un-normalised, as the reference uses it)
    float4 right;
    float4 up;
    float4 dirn;             // spot: normalize(direction), .w = cos(coneAngle); sun: normalize(direction)
};

// ---- two-level scenes (scene option instancing = 1; two_level.hip): one BLAS per distinct mesh, built in OBJECT space by the same
// pipeline as the flattened scene, one record per instance, and a TLAS (rope nodes again, built on the host over the instances'
// world boxes) whose leaves are ranges of `tlas_index`.  Replaces MTLAccelerationStructureInstanceDescriptor + the instance
// acceleration structure of Renderer.swift:193-213.  A ray is taken into object space at the instance boundary WITHOUT
// renormalising its direction, so the hit distance t is the world-space t.
struct InstanceDev {          // 80 B
    float4 w2o[3];            // rows of the world->object 3x4: p_obj.k = fma(r.z, p.z, fma(r.y, p.y, r.x * p.x)) + r.w (directions: without r.w)
    uint32_t node_base;       // first rope node of its BLAS in `bnodes`
    uint32_t packet_base;     // first triangle packet of its BLAS in `bpackets`
    uint32_t gid_base;        // global id of its first triangle: instance-major, then geometry, then primitive — the numbering of the flattened scene
    uint32_t ts_base;         // first shading record of its BLAS in `tri_shade`
    uint32_t vbase;           // first vertex of its mesh in `normals`
    uint32_t ntri, blas;
    uint32_t wroot;           // root of its BLAS in the shared 8-wide array `wnodes` (child / packet indices in there are absolute)
};

struct SceneView {           // passed by value to kernels
    const float4 *nodes;         // 4 x float4 per node
    const float4 *packets;       // 3 x float4 per triangle, leaf order
    const uint4 *tri_shade;      // per gid
    const float4 *normals;       // object space, concatenated over meshes (float3 stride 16, Mesh.swift:27-29)
    const float4 *base_color;    // per resource slot = instance*max_sub + geometry (Renderer.swift:139)
    const float4 *materials;     // per resource slot, 3 x float4: baseColor | dissolve, specular | specularExponent, emission | refractionIndex (materials extension)
    const float4 *inst_cols;     // 3 x float4 per instance: columns 0..2 of the 4x3 transform
    const uint32_t *geom_base;   // per resource slot: first gid
    const LightDev *lights;
    // 8-wide compressed layout (WideNode below) for the LDS-stack traversal backend; num_wnodes == 0 → not built
    const float4 *wnodes;        // 5 x float4 per wide node
    const float4 *wpackets;      // 3 x float4 per triangle, grouped per wide node
    // two-level scenes: `nodes` is the TLAS; num_inst == 0 -> flattened scene
    const InstanceDev *inst;
    const uint32_t *tlas_index;  // instance ids, TLAS leaf order
    const uint32_t *wtlas_index; // instance ids in the leaf order of the 8-wide TLAS (wnodes[0 ..]: its leaf children are single instances)
    const float4 *inst_box;      // two-level scenes: per instance four float4 — the box of its BLAS in OBJECT space (lo, hi: what the BLAS pass tests a fetched pair's ray against) and the instance's padded WORLD box (lo, hi: what the flat TLAS pass, k_tl_top_flat, queues pairs on)
    const uint32_t *tri_packet;  // two-level scenes with the 8-wide layout: per shading record (InstanceDev::ts_base + triangle of the BLAS) its packet in wpackets — how k_shade<.., PAIRS> finds the triangle a key names
    const float4 *bnodes;        // rope nodes of all BLASes, 4 x float4 each; followed, in the same allocation, by
    const float4 *bpackets;      // their triangle packets (object space), 3 x float4 each
    uint32_t num_inst;
    uint32_t num_wpackets, num_wtlas;   // entries of wpackets / wtlas_index (the -DMRT_DEBUG_BOUNDS build checks every index against these)
    uint32_t num_wnodes;
    uint32_t num_nodes;
    uint32_t num_tris;
    int32_t light_count;
    int32_t max_sub;
};

// Scratch memory of one build: a few large allocations handed out in 256-byte-aligned pieces and freed together (a build used to make ~60 hipMalloc / hipFree
// pairs, each a few tens of microseconds and the frees device-synchronising).  Declare it before the buffers that borrow from it.
struct ScratchArena {
    std::vector<void *> chunks; uint8_t *cur = nullptr; size_t left = 0, chunk_bytes = (size_t)1 << 20;
    ScratchArena() = default;
    ScratchArena(const ScratchArena &) = delete; ScratchArena &operator=(const ScratchArena &) = delete;
    ~ScratchArena() { for (void *c : chunks) (void)hipFree(c); }
    hipError_t take(void **out, size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes > left) {
            const size_t c = bytes > chunk_bytes ? bytes : chunk_bytes;
            void *m = nullptr;
            hipError_t e = hipMalloc(&m, c);
            if (e != hipSuccess) return e;
            chunks.push_back(m); cur = (uint8_t *)m; left = c;
        }
        *out = cur; cur += bytes; left -= bytes;
#ifdef MRT_POISON_ALLOC      // diagnostics build: no allocation starts out as zeros (every dword = 1: a counter that was assumed 0 is off by one, an index stays inside its array)
        (void)hipDeviceSynchronize(); (void)hipMemsetD32((hipDeviceptr_t)*out, 1, bytes / 4); (void)hipDeviceSynchronize();
#endif
        return hipSuccess;
    }
};

template <class T> struct DevBuf {
    T *p = nullptr; size_t n = 0; bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p && owned) (void)hipFree(p); p = nullptr; n = 0; owned = true; }
    hipError_t alloc(size_t count, unsigned flags = 0 /* hipDeviceMallocDefault; hipDeviceMallocUncached for streamed buffers (experiment) */) {
        if (count == 0) count = 1;
        if (p && owned && n == count && !flags) return hipSuccess;          // same size as before (a re-commit, a resize back): keep the allocation, the caller overwrites it
        release();
        hipError_t e = flags ? hipExtMallocWithFlags((void **)&p, count * sizeof(T), flags) : hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
#ifdef MRT_POISON_ALLOC
        if (e == hipSuccess) { (void)hipDeviceSynchronize(); (void)hipMemsetD32((hipDeviceptr_t)p, 1, count * sizeof(T) / 4); (void)hipDeviceSynchronize(); }
#endif
        return e;
    }
    hipError_t alloc_in(ScratchArena &a, size_t count) {       // a piece of the arena: not freed here, gone with the arena
        release();
        if (count == 0) count = 1;
        hipError_t e = a.take((void **)&p, count * sizeof(T));
        if (e == hipSuccess) { n = count; owned = false; } else p = nullptr;
        return e;
    }
    size_t bytes() const { return n * sizeof(T); }
};
static inline uint32_t cdiv(size_t a, size_t b) { return (uint32_t)((a + b - 1) / b); }      // grid sizes

// Pinned host memory that only grows: the staging area of a scene's uploads.  A commit concatenates the caller's arrays straight into it (one pass, no zero fill)
// and the copies to the device are DMA from pinned pages; it stays with the scene, so the commits of an animated scene pay no allocation.
struct PinnedBuf {
    void *p = nullptr; size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        const size_t want = (bytes + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
};

struct HostMesh {                  // what the caller handed over through mrt_scene_add_mesh / _add_submesh / _add_instance
    int source = -1;               // >= 0: an instance of that mesh (shares its vertex arrays, submeshes and materials; its own arrays stay empty)
    std::vector<float> positions;  // packed xyz, object space
    std::vector<float> normals;    // packed xyz, object space
    float xf[16];                  // column-major, last row forced to (0,0,0,1)
    std::vector<std::vector<uint32_t>> sub_indices;
    std::vector<MRTMaterial> sub_materials;
    bool dirty = false;            // vertices replaced by mrt_scene_update_mesh since the last commit (a refit recomputes the boxes of such meshes' triangles only)
};

struct BuildOptions {
    int builder = 1;          // 0 = Karras radix tree (plain LBVH), 1 = PLOC agglomeration over the Morton order, 2 = binned SAH built on the host (quality yardstick, seconds)
    int max_leaf = 4;         // SAH leaf collapse limit
    float cost_trav = 1.0f;   // SAH constants
    float cost_isect = 1.0f;
    int ploc_radius = 16;
    int wide = 1;             // build the 8-wide compressed layout: every ray of the pipeline walks it
    int rope = 0;             // 1: also emit the rope layout (binary nodes with escape links + its own copy of the packets); 0: only when the scene cannot have the 8-wide layout
    int wide_collapse = 1;    // 8-wide layout: 0 = greedy collapse of the binary tree (largest child first), 1 = SAH-optimal collapse by dynamic programming (k_wide_dp)
    float wide_cost_node = 1.0f, wide_cost_tri = 0.5f;      // its constants: a node visit (eight box tests + an iteration) against one triangle test — ~250 against ~125 VALU instructions in the stream loop; 0.3 until round 5
                                                            // (0.45 ... 1.0 measured +1 ... +2 % on DragonScene, 0.5 against 0.3: garden 4K +1 %, dragon x 4 +3 ... +4 %, hostile +1.5 %, Cornell 256^2 +8 ... +13 %; profiles/r05_wide_cost_tri.txt)
    float presplit = 4.0f;    // > 0: a triangle whose box is longer than presplit x the mean triangle extent enters the build as several references (k_split_emit); 0 = off
    int refit = 1;            // a commit after mrt_scene_update_mesh alone (same topology, new vertex positions / normals) REFITS the 8-wide tree of a flattened scene — packets rewritten, boxes recomputed bottom-up, the tree's shape kept — instead of building it again; 0: always build
    float refit_max_cost_ratio = 0.0f;      // > 0: a commit whose refit leaves MRTSceneStats.wide_cost above this factor of wide_cost_built builds the tree again instead (0 = the caller decides, from those two numbers)
    int refit_fenced = 0;     // 1: the bottom-up pass of the build with __threadfence() hand-offs instead of write-through stores (the slow reference form; same tree bit for bit)
    int validate = 1;         // check every index of the committed layout on the host (validate_layout), once per commit
    int instancing = 0;       // 0: flatten every instance into one world-space BVH (default; the reference never shares a primitive AS);
                              // 1: two-level — a BLAS per distinct mesh shared by its instances + a TLAS; transform changes rebuild only the TLAS
};

// One BLAS of a two-level scene inside the scene's shared arrays: what a refit of that BLAS (mrt_scene_update_mesh on its mesh + commit) needs to find it again
struct BlasRange {
    uint32_t src_mesh = 0;                                   // the mesh it was built from (index into the scene's mesh list)
    uint32_t wnode_base = 0, wnodes = 0;                     // its 8-wide nodes in `wnodes` (absolute child / packet indices inside)
    uint32_t packet_base = 0, ntri = 0;                      // its packets in `wpackets` and in `bpackets` (one per triangle: BLASes are built without pre-splitting)
    uint32_t node_base = 0, rope_nodes = 0;                  // its rope nodes in `bnodes`
    uint32_t ts_base = 0, vbase = 0;
    std::vector<uint32_t> wide_levels;                       // nodes per level of its 8-wide tree (BFS numbering)
    float wide_cost_built = 0.0f, sah_cost_built = 0.0f;     // as its build left them (MRTSceneStats)
    float wide_cost = 0.0f, leaf_growth = 1.0f;              // leaf_growth: its leaf boxes' area against the build's, chained over its refits
};

struct RefitLayouts { bool wide = false, rope = false; };          // which resident layouts a refit works on (refit_layouts)
// One refit enqueue (enqueue_refit, bvh_refit.hip) for the commit of a flattened scene, a BLAS of a two-level scene and the stream-ordered refit: what is refitted ...
struct RefitTarget {
    float4 *wnodes = nullptr, *wpackets = nullptr;         // the 8-wide arrays as its nodes index them (null wnodes: no 8-wide layout to refit)
    uint32_t wpacket_first = 0;                            // the tree's first packet in wpackets (a BLAS in the shared array)
    const uint32_t *level_first = nullptr, *level_count = nullptr; size_t levels = 0;      // per level of the 8-wide tree: its first node and its node count
    float4 *rope_nodes = nullptr, *rope_packets = nullptr; // the tree's own first rope node and first rope packet (null rope_packets: no rope layout to refit)
    uint32_t rope_nodes_n = 0;                             // 0: only the rope packets are rewritten
    uint32_t packets = 0;                                  // triangle packets per layout
    const uint4 *tri_shade = nullptr; const uint8_t *dirty = nullptr;      // a leaf none of whose triangles' instances (tri_shade[gid].w >> 16) is dirty keeps its box
    bool rope_every_leaf = false;                          // k_rope_refit recomputes every leaf (it gets neither tri_shade nor dirty)
};
// ... and the scratch it works in: k_flatten's outputs, a box per 8-wide node, the two growth sums, and per rope node its parent, arrival counter (zeroed) and {a, b} words
struct RefitScratch { float4 *tri_world, *tri_lo, *tri_hi, *nbox; double *growth; uint32_t *parent, *arrived; uint2 *ab; };
// What the three stream-ordered update families share: how an update call's check kernel refuses its input, and what a blocking reader waits for.
// The owner allocates the two buffers (from its arena, or by alloc) and creates the event; the gate waits for the event before it goes.
struct UpdateGate {
    DevBuf<uint32_t> words;                                // [0]: sequence number of the last update call the device refused (k_ingest_check or k_inst_check)
    DevBuf<unsigned long long> rejected;                   // update calls refused on the device since the workspace was made (sticky)
    hipEvent_t ev_last = nullptr;                          // behind the last update or refit enqueued: what a blocking reader waits for
    uint32_t seq = 0;                                      // update calls so far
    ~UpdateGate() { if (ev_last) { (void)hipEventSynchronize(ev_last); (void)hipEventDestroy(ev_last); } }
    uint32_t next() { if (++seq == 0u) seq = 1u; return seq; }          // (0 is what words[0] starts as)
    hipError_t rejected_so_far(uint64_t *count) const {    // blocks on ev_last
        *count = 0;
        const hipError_t e = hipEventSynchronize(ev_last);
        return e != hipSuccess ? e : hipMemcpy(count, rejected.p, 8, hipMemcpyDeviceToHost);
    }
};
// The scratch of a refit, resident for a flattened scene (RefitWorkspace) and for the BLASes of a two-level one (BlasWorkspace): k_flatten's outputs (tri_world 48 B, tri_lo /
// tri_hi 32 B per triangle), the refit's node boxes (32 B per 8-wide node), the rope refit's parent / arrived / ab (16 B per rope node), and what both keep per mesh on the host.
struct RefitBuffers {
    ScratchArena arena;                                    // before the buffers that borrow from it
    DevBuf<float4> tri_world, tri_lo, tri_hi, nbox;
    DevBuf<uint32_t> cbounds, parent, arrived; DevBuf<uint2> ab;
    DevBuf<double> growth;                                 // k_refit_wide_level's two sums per refitted tree (folded and cleared by k_refit_fold), then wide_tree_cost's 8 + 24 bytes
    DevBuf<float> leaf_growth;                             // MRTSceneStats.leaf_growth (per BLAS: BlasRange::leaf_growth), chained on the device over the refits
    std::vector<uint8_t> host_stale, pending;              // per mesh / BLAS: the HostMesh copy is older than the device's vertices; updated on the device and not yet refitted
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;       // around the last refit (MRTSceneStats.build_ms)
    bool unresolved = false;                               // refits enqueued whose results the host has not read yet (resolve_device_refits, resolve_blas_refits)
    ~RefitBuffers() { for (hipEvent_t e : {ev_begin, ev_end}) if (e) (void)hipEventDestroy(e); }
    RefitScratch scratch(size_t growth_at = 0) const { return RefitScratch{tri_world.p, tri_lo.p, tri_hi.p, nbox.p, growth.p + growth_at, parent.p, arrived.p, ab.p}; }
};
// What the stream-ordered refit (mrt_scene_update_mesh_device / mrt_scene_refit_device) keeps on the device between calls, so that a call allocates nothing, copies nothing from the host and
// waits for nothing: the scratch above, the dirty byte per flattened instance and a handful of words.  Made by the first device update after a build (which may allocate), dropped by the next build and by mrt_scene_destroy.
struct RefitWorkspace : RefitBuffers {                     // growth: [0 .. 1] the sums, [2 .. 5] wide_tree_cost's
    DevBuf<uint2> ref_table;                               // {flattened instance, its first vertex in g_pos / normals}, grouped by source mesh
    DevBuf<uint8_t> inst_dirty;                            // per flattened instance: its vertices were replaced since the last refit
    std::vector<uint32_t> ref_first, ref_count, mesh_vbase;   // per mesh of the scene: its range of ref_table (instances: empty), its first vertex
    std::vector<uint32_t> level_first;                     // first node of every level of the 8-wide tree
    uint32_t instances = 0;
    RefitLayouts layouts;                                  // refit_layouts() of the tree the workspace was made for
    UpdateGate gate;                                       // (last: its destructor waits for the stream before anything above is freed)
};

// What the stream-ordered instance moves (mrt_scene_set_instance_transforms_device / mrt_scene_refit_instances_device, tlas_refit.hip) keep between calls.
// Made by the first such call after a commit (which may allocate and block), dropped by the next commit's update_tlas and by mrt_scene_destroy.
struct InstanceWorkspace {
    DevBuf<uint32_t> rope_order;                           // the rope TLAS's nodes grouped by depth (DeviceScene::tlas_rope_order)
    DevBuf<float4> nbox;                                   // the 8-wide TLAS refit's box per node (lo, hi)
    std::vector<uint32_t> rope_first;                      // first entry of every depth in rope_order
    std::vector<uint32_t> wide_first;                      // first node of every level of the 8-wide TLAS
    std::vector<uint8_t> moved;                            // per instance: the HostMesh::xf copy is older than the device's inst_cols
    DevBuf<uint32_t> wide_of_pos;                          // mrt_scene_rebuild_tlas_device (tlas_rebuild.hip): per leaf position of the binary median order, the entry of wtlas_index that names it (the inverse of DeviceScene::tlas_wide_pos)
    DevBuf<uint32_t> ids[2], seg_axis;                     // ... and, above TLAS_RESORT_LDS_LIMIT instances only, the ping-pong id buffers of its one-level-per-step part and the split axis per range of a level
    UpdateGate gate;                                       // (last, as RefitWorkspace's)
};

// What the stream-ordered BLAS refit of a two-level scene (mrt_scene_update_blas_device / mrt_scene_refit_blas_device) keeps between calls: the object-space
// geometry build_two_level's scratch scenes took with them (packed positions, indices and submesh records per BLAS, as refit_blas assembles them), ONE set of refit scratch sized
// for the largest BLAS (the BLASes are refitted in sequence on the stream), a box per 8-wide node of the whole shared array (refit indices are absolute) and a few words per
// BLAS.  Made by the first such call after a commit from the HostMesh copies (which may allocate and block), kept by a transforms-only commit (update_tlas), dropped by
// build_two_level, by refit_two_level (whose uploads would leave `pos` stale) and by mrt_scene_destroy.
struct BlasWorkspace : RefitBuffers {                      // growth: [2b, 2b + 1] the sums of BLAS b, [2B .. 2B + 3] wide_tree_cost's; leaf_growth: per BLAS
    DevBuf<float> pos;                                     // packed positions of every BLAS's mesh, at 3 * BlasRange::vbase
    DevBuf<uint32_t> idx, recs;                            // per BLAS: its index list (at idx_first) and its SubRecs (at rec_first), BLAS-local as refit_blas uploads them
    DevBuf<float4> cols;                                   // the identity, for k_flatten
    DevBuf<uint4> tri_shade;                               // k_flatten's shading records of the BLAS's own numbering (scratch: the scene's are the build's)
    DevBuf<uint2> ref_table;                               // ref_table[b] = {0, vbase of BLAS b}: k_ingest_write's one-row table
    DevBuf<uint32_t> inst_list;                            // instance ids grouped by BLAS (inst_first / inst_count)
    DevBuf<uint8_t> dirty;                                 // 4 bytes of 1: the one "instance" of a BLAS's own triangle arrays moved
    std::vector<int> blas_of_mesh;                         // per mesh known at the commit: its BLAS, -1 for an instance
    std::vector<uint32_t> idx_first, rec_first, rec_count, inst_first, inst_count;      // per BLAS
    std::vector<std::vector<uint32_t>> level_first;        // per BLAS: first node of every level of its 8-wide tree (absolute)
    std::vector<uint8_t> refitted;                         // per BLAS: refitted since the host last read its root box and statistics
    UpdateGate gate;                                       // (last, as RefitWorkspace's)
};

// What the surface entries (mrt_scene_resolve_hits_device / mrt_scene_interpolate_device, surface.hip) keep between calls: one row per resource slot —
// {first shading record, triangle count, vertex base in `normals`, caller's vertex row minus the library's vertex id} — restated from the host's mesh list, so that a record's
// ids are checked against sizes before anything is indexed with them and both scene forms resolve alike.  Made by the first such call after a commit (it allocates, uploads
// and blocks), dropped by the next mrt_scene_commit and by mrt_scene_destroy.
struct SurfaceWorkspace {
    DevBuf<uint4> slots;
    uint32_t instances = 0, max_sub = 1;
    uint64_t vertices = 0;                                 // rows of the caller's numbering (mrt_scene_vertex_offsets' last entry)
};

struct DeviceScene {
    DevBuf<float4> nodes, packets, normals, base_color, materials, inst_cols, wnodes, wpackets;
    uint32_t num_wnodes = 0; int wide_depth = 0;
    std::vector<uint32_t> wide_levels;           // flattened scenes: nodes per level of the 8-wide tree (BFS numbering) — what a refit walks bottom-up
    uint32_t refits = 0;                         // commits served by a refit since the last build
    float sah_cost_built = 0.0f;                 // stats.sah_cost as the last build left it (a refit scales it by the 8-wide tree's cost ratio)
    uint64_t refit_triangles = 0;                // triangles of the build that made the 8-wide layout (a refit needs the same count)
    uint32_t num_packets = 0;        // triangle packets per layout = build references (stats.triangles, or more when long triangles were pre-split)
    uint32_t rope_nodes = 0;         // surviving rope nodes (stats.bvh_nodes reports the 8-wide node count when that layout is built)
    size_t packets_offset = 0;       // packets start at nodes.p + packets_offset (float4 units); `packets` itself is unused
    DevBuf<uint4> tri_shade;
    DevBuf<uint32_t> geom_base;
    DevBuf<LightDev> lights;
    int light_count = 0;
    MRTSceneStats stats{};
    float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};     // box of the whole tree (padded leaf boxes)
    // two-level scenes (two_level.hip)
    DevBuf<InstanceDev> inst; DevBuf<uint32_t> tlas_index, wtlas_index, tri_packet; DevBuf<float4> bnodes, inst_box;
    uint32_t tlas_wcap = 0; int blas_wdepth = 0;               // 8-wide layout: node slots reserved for the TLAS in front of the BLASes, deepest BLAS (0: rope only)
    size_t bpackets_offset = 0; uint32_t num_inst = 0;
    std::vector<InstanceDev> h_inst;                           // host copy: transform updates rewrite the rows and rebuild the TLAS only
    std::vector<BlasRange> blas_ranges;                        // per BLAS: where it lies in the shared arrays (refit_two_level)
    bool blas_all_wide = false;                                // every BLAS has the 8-wide layout (the shared wnodes / wpackets exist)
    std::vector<float> blas_lo, blas_hi;                       // per BLAS root box (object space), 3 floats each
    float tlas_ms = 0;                                         // host + upload time of the last TLAS build
    std::vector<uint8_t> in_tlas;                              // per instance: it is a leaf of the last TLAS build (ntri > 0, invertible then)
    std::vector<uint32_t> tlas_rope_order, tlas_rope_levels;   // rope TLAS: node indices grouped by depth (root first), nodes per depth — what refit_instances walks bottom-up
    std::vector<uint32_t> tlas_wide_levels;                    // 8-wide TLAS, when resident: nodes per level (BFS numbering from node 0)
    std::vector<uint32_t> tlas_wide_pos;                       // 8-wide TLAS, when resident: per entry of wtlas_index, the leaf position of its instance in the binary median order (WideTlasBuilder::pos)
    uint32_t tlas_instances = 0;                               // instances in the TLAS of the last commit: the live entries of tlas_index (and of wtlas_index)
    std::unique_ptr<InstanceWorkspace> inst_ws;                // null until the first mrt_scene_set_instance_transforms_device / _refit_instances_device after a commit
    bool validate = true, validated_blas = false;              // commit-time index validation (two_level.hip validate_layout); BLAS part already checked
    DevBuf<float> g_pos; DevBuf<uint32_t> g_idx, g_recs;       // flattened build: packed object-space positions, indices and submesh records as uploaded (kept: a commit that only changes transforms does not upload them again)
    PinnedBuf stage;                                           // upload staging of build_flat (grow-only, reused by every commit of this scene)
    double commit_ms[6] = {0, 0, 0, 0, 0, 0};                    // host wall time of the last flat build, by phase: staging (reserve + fill), device allocations + upload enqueue, topology (sort .. refit, incl. its read-backs), 8-wide emit, rope emit, validation (mrt_debug_commit_times)
    std::unique_ptr<RefitWorkspace> refit_ws;                    // the stream-ordered refit's resident scratch (null until the first mrt_scene_update_mesh_device after a build)
    std::unique_ptr<BlasWorkspace> blas_ws;                      // two-level scenes: the stream-ordered BLAS refit's resident geometry and scratch (null until the first mrt_scene_update_blas_device / _refit_blas_device after a commit)
    DevBuf<double> cost_words;                                   // wide_tree_cost's 8 + 24 bytes for refit_two_level (made once, kept: no hipMalloc / hipFree pair per commit)
    std::unique_ptr<SurfaceWorkspace> surface_ws;                // the surface entries' slot table (null until the first mrt_scene_resolve_hits_device / _interpolate_device after a commit)
    uint64_t rejected_before = 0;                                // device updates refused in the lifetimes of earlier workspaces of this scene
    DevBuf<uint32_t> mesh_masks;                                 // visibility mask per mesh id: a buffer of its own, written by mrt_scene_set_mesh_masks and by a commit whose mesh count changed, read by the masked queries alone (masked.hip, through lane_walk.h's Visibility) — no build, refit or view() knows it
    SceneView view() const;
};

// bvh_build.hip
void pack_material(const MRTMaterial &m, float4 *out3);
int layout_limits(uint64_t triangles, uint64_t nodes);    // MRT_OK, or MRT_ERR_UNSUPPORTED when the traversal layouts cannot address such a scene
int build_scene(const std::vector<HostMesh> &meshes, const BuildOptions &opt, hipStream_t stream, DeviceScene &out, bool geometry_unchanged = false, bool refit = false);      // flattened scenes, as build_flat: geometry_unchanged: only transforms changed since the commit before (the geometry on the device is kept); refit: only vertices did
// bvh_host_sah.cpp (builder = 2): binned-SAH topology over n reference boxes, built on the host
void host_sah_topology(const float4 *lo, const float4 *hi, uint32_t n, std::vector<uint32_t> &order, std::vector<uint32_t> &left, std::vector<uint32_t> &right, std::vector<uint32_t> &parent);
struct MeshRef { const HostMesh *g; const float *xf; };         // geometry + object->world matrix (column-major 4x4)
int build_flat(const std::vector<MeshRef> &refs, const BuildOptions &opt, hipStream_t stream, DeviceScene &out, PinnedBuf *stage = nullptr, bool geometry_unchanged = false, bool refit = false);      // stage: the upload staging to use instead of out.stage (the BLAS builds of a two-level scene share their scene's)
// two_level.hip
int build_two_level(const std::vector<HostMesh> &meshes, const BuildOptions &opt, hipStream_t stream, DeviceScene &out);
int refit_two_level(const std::vector<HostMesh> &meshes, const BuildOptions &opt, hipStream_t stream, DeviceScene &out);      // after mrt_scene_update_mesh alone: the BLASes of the updated meshes refitted in place (both layouts) + the TLAS; MRT_ERR_UNSUPPORTED (no message): the scene cannot be refitted, build it
// what refit_two_level takes, for the commit and for the stream-ordered BLAS refit alike: the scene (every BLAS with the 8-wide layout, the mesh list of the build) ...
inline bool two_level_refittable(const DeviceScene &sc, size_t meshes) { return sc.blas_all_wide && sc.num_inst == meshes && !sc.blas_ranges.empty() && sc.h_inst.size() == meshes; }
// ... and one BLAS of it whose mesh (of nverts vertices) changed
inline bool blas_refittable(const BlasRange &r, size_t nverts) { return r.wnodes != 0 && !r.wide_levels.empty() && nverts != 0; }
int refit_blas(const HostMesh &g, const BlasRange &br, hipStream_t stream, DeviceScene &out, float root_lo[3], float root_hi[3], float *ms_out, float *growth_out);      // bvh_refit.hip
int update_tlas(const std::vector<HostMesh> &meshes, hipStream_t stream, DeviceScene &out);      // after transform changes: instance rows + TLAS, BLASes untouched
int validate_layout(const DeviceScene &sc, hipStream_t stream, bool tlas_only, const float4 *wnodes_override = nullptr);      // wnodes_override: a device copy of the 8-wide nodes to check in place of the scene's (mrt_debug_validate_patched)
         // every index of the 8-wide layout / instance rows inside its array; MRT_ERR_STATE + message otherwise
// bvh_refit.hip: the refit of resident layouts
int wide_histogram(const DeviceScene &sc, hipStream_t stream, uint32_t out12[12]);      // diagnostics: children per 8-wide node
int wide_tree_cost(const float4 *wnodes, uint32_t first, uint32_t count, uint32_t root, float c_node, float c_tri, hipStream_t stream, void *scratch32, float *out);      // SAH cost of the 8-wide subtree [first, first + count) rooted at `root`, as it lies in memory, per unit of root area; scratch32: 32 bytes of device memory, 8-byte aligned (the caller's arena or workspace)
RefitLayouts refit_layouts(const DeviceScene &sc, const BuildOptions &opt);
void enqueue_refit(const RefitTarget &tg, const RefitScratch &s, hipStream_t stream);      // the five refit kernels on the stream, nothing else
RefitTarget flat_refit_target(const DeviceScene &sc, RefitLayouts layouts, const uint32_t *level_first, const uint8_t *dirty);      // what a refit of a flattened scene works on: a refitting commit's and the stream-ordered refit's
void fold_blas_stats(DeviceScene &sc, float ms);      // what BLAS refits leave in a two-level scene's statistics, from its BlasRanges: refit_two_level's and resolve_blas_refits'
void retire_gate(DeviceScene &sc, UpdateGate &gate);      // blocks; a workspace goes: its rejected count is kept in sc.rejected_before
int apply_refit_result(DeviceScene &sc, const BuildOptions &opt, bool wide, float ms, const float4 box[2], float leaf_growth, void *scratch32, hipStream_t stream);      // what a refit of a flattened scene leaves in sc.stats and the root box; blocks (wide_tree_cost)
// the stream-ordered refit (bvh_refit.hip)
int device_refit_supported(const DeviceScene &sc, const BuildOptions &opt, const char *who);      // MRT_OK, or MRT_ERR_UNSUPPORTED + message: what a refitting commit (build_flat) would not take
int device_refit_prepare(const std::vector<HostMesh> &meshes, const BuildOptions &opt, DeviceScene &sc);      // makes sc.refit_ws if it is not there (allocates, uploads its tables, blocks)
int device_update_mesh(DeviceScene &sc, size_t mesh, const void *d_pos, size_t pos_stride, const void *d_nrm, size_t nrm_stride, size_t nverts, hipStream_t stream);
int device_refit(DeviceScene &sc, hipStream_t stream);
int resolve_device_refits(DeviceScene &sc, const BuildOptions &opt, hipStream_t stream);      // blocks on the last refit and brings sc.stats up to date (no-op when nothing is pending)
int download_stale_meshes(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *pending_found = nullptr);      // blocks; the HostMesh copies of meshes updated on the device, read back from g_pos / normals; pending_found: a mesh was updated on the device and not refitted since (it is marked dirty)
int device_updates_rejected(DeviceScene &sc, uint64_t *count);      // blocks
void drop_refit_workspace(DeviceScene &sc);      // (a build: the tree the workspace was made for is gone)
int refit_workspace_after_commit(DeviceScene &sc);      // a commit that kept sc.refit_ws (a refit): its chained leaf_growth goes on from the commit's, its dirty marks are spent; blocks
void host_vertices_are_newer(DeviceScene &sc, size_t mesh);      // mrt_scene_update_mesh after an update on the device (either form): the next sync leaves the mesh's host copy alone
// tlas_refit.hip: instance moves from device buffers, ordered on the caller's stream
int instances_device_supported(const DeviceScene &sc, const BuildOptions &opt, const char *who);      // MRT_OK, or MRT_ERR_UNSUPPORTED + message: a flattened scene, a scene without an instance
int instances_device_prepare(DeviceScene &sc);      // makes sc.inst_ws if it is not there (allocates, uploads the level tables, blocks)
int device_set_instance_transforms(DeviceScene &sc, uint32_t first, uint32_t count, const void *d_xf, size_t stride, hipStream_t stream);
int device_refit_instances(DeviceScene &sc, hipStream_t stream);
int download_moved_transforms(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *moved_found = nullptr);      // blocks; HostMesh::xf of the instances moved on the device, read back from inst_cols
void enqueue_blas_instance_boxes(DeviceScene &sc, const float4 *nbox, uint32_t root, const uint32_t *inst_list, uint32_t count, hipStream_t stream);      // the instances inst_list[0 .. count) of one BLAS take nbox[2 * root] as their object box and a world box recomputed from it (k_blas_instance_boxes)
// tlas_rebuild.hip: the topology of both TLAS forms rebuilt on the caller's stream
constexpr uint32_t TLAS_RESORT_LDS_LIMIT = 1024;      // instances one workgroup re-sorts in LDS, all levels in one launch: 16 bytes each (the three centre sums and the id)
constexpr uint32_t TLAS_RESORT_MAX = 65536;           // instances mrt_scene_rebuild_tlas_device takes: above the LDS limit a level ranks its ranges by counting, quadratic in the range
int tlas_rebuild_supported(const DeviceScene &sc, const char *who);      // MRT_OK, or MRT_ERR_UNSUPPORTED + message: more than TLAS_RESORT_MAX instances in the TLAS
int device_rebuild_tlas(DeviceScene &sc, hipStream_t stream);      // needs sc.inst_ws (instances_device_prepare); ends with device_refit_instances
int tlas_host_build(const float *lo4, const float *hi4, uint32_t n, uint32_t *rope_order, uint32_t *rope_links, uint32_t *wide_order, uint32_t *wide_pos, uint32_t *counts);      // two_level.hip: mrt_debug_tlas_host_build
void wide_encode_host(const float *child_lo4, const float *child_hi4, uint32_t occupied_mask, uint32_t imask, uint32_t *out_words20);      // two_level.hip: mrt_debug_wide_encode (wide_encode.h on the host)
bool instance_box_host(const float *xf16, const float *obj_lo3, const float *obj_hi3, float *rows12, float *world_box6);      // two_level.hip: mrt_debug_instance_box (instance_math.h on the host)
void host_transform_is_newer(DeviceScene &sc, size_t mesh);      // mrt_scene_set_instance_transform after a move on the device: the next sync leaves HostMesh::xf alone
void drop_instance_workspace(DeviceScene &sc);      // (update_tlas: the TLAS the workspace was made for is gone; the rejected count is kept)
// bvh_refit.hip: meshes of two-level scenes deformed from device buffers, ordered on the caller's stream
int blas_device_supported(const DeviceScene &sc, const BuildOptions &opt, size_t meshes, const char *who);      // MRT_OK, or MRT_ERR_UNSUPPORTED + message: a flattened scene, refit = 0, a scene refit_two_level would not take
int blas_device_prepare(const std::vector<HostMesh> &meshes, DeviceScene &sc);      // makes sc.blas_ws if it is not there (allocates, uploads the meshes' geometry, blocks)
int device_update_blas(DeviceScene &sc, size_t blas, const void *d_pos, size_t pos_stride, const void *d_nrm, size_t nrm_stride, size_t nverts, hipStream_t stream);
int device_refit_blas(DeviceScene &sc, hipStream_t stream);      // needs sc.inst_ws too (instances_device_prepare)
int resolve_blas_refits(DeviceScene &sc, const BuildOptions &opt, hipStream_t stream);      // blocks on the last refit; blas_lo / blas_hi, the BlasRanges' and the scene's statistics brought up to date (no-op when nothing is pending)
int download_stale_blas_meshes(std::vector<HostMesh> &meshes, DeviceScene &sc, bool *pending_found = nullptr);      // blocks; as download_stale_meshes, from the BLAS workspace
void drop_blas_workspace(DeviceScene &sc);      // (the rejected count is kept)
// surface.hip: hit records resolved to surface data on the caller's stream
void surface_vertex_offsets(const std::vector<HostMesh> &meshes, std::vector<uint64_t> &offsets);      // the caller's vertex numbering: meshes + 1 entries
int surface_prepare(const std::vector<HostMesh> &meshes, DeviceScene &sc);      // makes sc.surface_ws if it is not there (allocates, uploads the slot table, blocks)
// (d_count, here and in the stage entries below: null, or one uint32 on the device — the kernel then handles the rows below min(n, *d_count) and touches no other)
int resolve_hits_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, const void *d_count = nullptr);      // one launch, nothing else; needs sc.surface_ws
int interpolate_device(const DeviceScene &sc, hipStream_t stream, const void *d_hits, size_t n, const void *d_attr, size_t attr_stride, uint32_t channels, void *d_out, size_t out_stride,
                       const void *d_count = nullptr);
void drop_surface_workspace(DeviceScene &sc);      // (a commit: the table restates the mesh list of the commit before)
int upload_lights(const MRTLight *lights, int count, hipStream_t stream, DeviceScene &out);
// multihit.hip: per ray the max_hits smallest hits under (distance, triangle id), on the caller's stream (the walks and the list: lane_walk.h, §10q)
int intersect_all_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, size_t n, int max_hits, void *d_out, void *d_hit_counts, const void *d_count = nullptr);      // one launch, nothing else; flattened scenes, max_hits in [1, MRT_MAX_HITS]
// masked.hip: the three device queries with a visibility mask per call or per ray (the walks, the sinks and the filter: lane_walk.h, §10q)
enum MaskedQuery { MASKED_CLOSEST = 0, MASKED_ANY = 1, MASKED_ALL = 2 };
int intersect_masked_device(const DeviceScene &sc, hipStream_t stream, MaskedQuery query, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, int max_hits, void *d_out,
                            void *d_hit_counts, const void *d_count);      // one launch, nothing else; needs sc.mesh_masks; MASKED_ALL: flattened scenes, max_hits in [1, MRT_MAX_HITS]
// stages.hip: what follows a surface in the reference's kernel, on the caller's stream
int scatter_device(const DeviceScene &sc, hipStream_t stream, const void *d_surfaces, const void *d_halton_index, size_t n, int bounce, int light_count, void *d_shadow_rays, void *d_light,
                   void *d_next_rays, const void *d_count = nullptr);      // one launch, nothing else; light_count in [1, sc.light_count], bounce in [0, 18]
// stages_materials.hip: the same step with the materials extension on
int scatter_materials_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int bounce, int max_bounces,
                             int light_count, void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes, const void *d_count = nullptr);      // one launch, nothing else; light_count in [1, sc.light_count], max_bounces in [1, 16], bounce in [0, max_bounces)
// queues.hip: stable compaction of the rows of up to eight columns on the caller's stream, the count left on the device
constexpr uint32_t COMPACT_ROWS = 2048;               // rows per workgroup of the count and move kernels
constexpr uint32_t COMPACT_SCAN_THREADS = 1024;       // per-workgroup totals the one scan workgroup takes at a step
constexpr int COMPACT_MAX_COLUMNS = 8;
size_t compact_workspace_bytes(size_t n);             // one uint32 per workgroup, rounded up to 16 bytes (at least 16)
int compact_rows_device(hipStream_t stream, const void *d_keep, size_t n, const void *d_count_in, const MRTRowColumn *columns, int ncolumns, void *d_count_out, void *d_workspace);      // three launches, nothing else

}  // namespace mrt
