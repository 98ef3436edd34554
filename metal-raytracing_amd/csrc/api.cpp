// api.cpp — implementation of include/mrt_abi.h.  Every entry point validates its arguments,
// catches C++ exceptions and returns a status code; nothing throws or aborts across the ABI.
// There is no CPU fallback: without a HIP device mrt_context_create fails (MRT_ERR_NO_DEVICE).
#include "api_types.h"
#include "abi_check.h"
#include "paths.h"
#include "image.h"
#include "temporal.h"
#include "variance.h"
#include "../../include/mrt_debug.h"
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <memory>
#include <new>

namespace mrt {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    g_err = buf;
    return e == hipErrorOutOfMemory ? MRT_ERR_OUT_OF_MEMORY : MRT_ERR_HIP;
}
}  // namespace mrt

static int bind_device(MRTContext ctx) { MRT_HIP(hipSetDevice(ctx->device)); return MRT_OK; }

// HostMesh copies brought up to date.  What the three families of device updates left for the next commit — vertices nobody refitted (§10d flattened, §10f per BLAS), instances
// moved (§10e) — is reported to scene->changes, which decides what that makes of the commit (scene_changes.h).
static int sync_host_meshes(MRTScene scene) {
    bool flat_vertices = false, blas_vertices = false, moved = false;
    int rc = mrt::download_stale_meshes(scene->meshes, scene->dev, &flat_vertices);
    // a two-level scene whose BLASes were refitted on the device (mrt_scene_refit_blas_device): their root boxes — update_tlas builds the TLAS from them — and statistics first,
    // then the vertices of the meshes updated there, then the matrices of the instances moved there
    if (!rc) rc = mrt::resolve_blas_refits(scene->dev, scene->opt, scene->ctx->stream);
    if (!rc) rc = mrt::download_stale_blas_meshes(scene->meshes, scene->dev, &blas_vertices);
    if (!rc) rc = mrt::download_moved_transforms(scene->meshes, scene->dev, &moved);
    scene->changes.device_changes_found(flat_vertices, blas_vertices, moved);          // (also where a later read-back failed: the workspaces have forgotten what they reported)
    return rc;
}

// The meshes' host copies as the device has them now (a scene whose vertices were replaced by mrt_scene_update_mesh_device, or whose instances were moved by
// mrt_scene_set_instance_transforms_device): for readers of MRTScene_::meshes outside this file.
// Leaves the calling thread's current device as it found it.
int mrt_scene_sync_host_meshes(MRTScene scene) {
    if (!scene->dev.refit_ws && !scene->dev.inst_ws && !scene->dev.blas_ws) return MRT_OK;
    int before = 0; MRT_HIP(hipGetDevice(&before));
    int rc = bind_device(scene->ctx);
    if (!rc) rc = sync_host_meshes(scene);
    (void)hipSetDevice(before);
    return rc;
}

// Visibility masks.  The host list is the truth and is as long as the mesh list once someone has asked for it; the device table restates it.  No build, refit or
// update touches the table, and DevBuf::alloc keeps an allocation of the same size, so a commit uploads it only when the mesh count changed or masks were set while the scene was
// not committed (`force`: mrt_scene_set_mesh_masks on a committed scene).  Blocks, as a commit does.
static std::vector<uint32_t> &mesh_masks_of(MRTScene scene) {
    if (scene->mesh_masks.size() != scene->meshes.size()) scene->mesh_masks.resize(scene->meshes.size(), 0xFFFFFFFFu);
    return scene->mesh_masks;
}
static int upload_mesh_masks(MRTScene scene, bool force) {
    const std::vector<uint32_t> &m = mesh_masks_of(scene);
    mrt::DevBuf<uint32_t> &table = scene->dev.mesh_masks;
    if (!force && !scene->masks_stale && table.p && scene->masks_uploaded == m.size()) return MRT_OK;          // (the entries written, not the allocation: an empty scene's table is one word nobody wrote)
    MRT_HIP(table.alloc(m.size()));
    if (!m.empty()) {
        MRT_HIP(hipMemcpyAsync(table.p, m.data(), m.size() * sizeof(uint32_t), hipMemcpyHostToDevice, scene->ctx->stream));
        MRT_HIP(hipStreamSynchronize(scene->ctx->stream));
    }
    scene->masks_stale = false; scene->masks_uploaded = m.size();
    return MRT_OK;
}

extern "C" {

const char *mrt_last_error(void) { return mrt::g_err.c_str(); }
int mrt_abi_version(void) { return MRT_ABI_VERSION; }

// ---------------------------------------------------------------- context
int mrt_context_create(int device_id, MRTContext *out) {
    MRT_TRY
    REQUIRE(out, "mrt_context_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) { mrt::set_error("no HIP device available (GPU not available — there is no CPU fallback)"); return MRT_ERR_NO_DEVICE; }
    REQUIRE(device_id >= 0 && device_id < count, "mrt_context_create: device_id out of range");
    std::unique_ptr<MRTContext_> c(new MRTContext_());
    c->device = device_id;
    MRT_HIP(hipSetDevice(device_id));
    MRT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
     // (without it the whole upload rides on `stream`)
    hipDeviceProp_t prop;
    MRT_HIP(hipGetDeviceProperties(&prop, device_id));
    snprintf(c->name, sizeof c->name, "%s (%s)", prop.name, prop.gcnArchName);
    *out = c.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_context_destroy(MRTContext ctx) {
    if (!ctx) return MRT_OK;
    // the reference's objects are reference-counted (ARC); a C handle is not, so the order is checked instead: a context outlives its scenes and renderers, a scene its renderers
    if (ctx->live != 0) { mrt::set_error("mrt_context_destroy: " + std::to_string(ctx->live) + " scene(s) / renderer(s) of this context are still alive: destroy them first"); return MRT_ERR_STATE; }
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream && ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    delete ctx;
    return MRT_OK;
}
int mrt_context_set_stream(MRTContext ctx, void *hip_stream) {
    MRT_TRY
    REQUIRE(ctx, "mrt_context_set_stream: ctx is NULL");
    int rc = bind_device(ctx); if (rc) return rc;
    if (ctx->own_stream && ctx->stream) { MRT_HIP(hipStreamSynchronize(ctx->stream)); MRT_HIP(hipStreamDestroy(ctx->stream)); }
    if (hip_stream) { ctx->stream = (hipStream_t)hip_stream; ctx->own_stream = false; }
    else { MRT_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    return MRT_OK;
    MRT_CATCH
}
int mrt_context_get_stream(MRTContext ctx, void **hip_stream) {
    REQUIRE(ctx && hip_stream, "mrt_context_get_stream: bad argument");
    *hip_stream = (void *)ctx->stream;
    return MRT_OK;
}
int mrt_context_device_name(MRTContext ctx, char *buf, size_t buflen) {
    REQUIRE(ctx && buf && buflen, "mrt_context_device_name: bad argument");
    snprintf(buf, buflen, "%s", ctx->name);
    return MRT_OK;
}

// ---------------------------------------------------------------- scene
int mrt_scene_create(MRTContext ctx, MRTScene *out) {
    MRT_TRY
    REQUIRE(ctx && out, "mrt_scene_create: bad argument");
    MRTScene s = new MRTScene_(); s->ctx = ctx; *out = s; ctx->live++;
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_destroy(MRTScene scene) {
    if (!scene) return MRT_OK;
    if (scene->renderers != 0) { mrt::set_error("mrt_scene_destroy: " + std::to_string(scene->renderers) + " renderer(s) still use this scene: destroy them first"); return MRT_ERR_STATE; }
    scene->ctx->live--;
    (void)hipSetDevice(scene->ctx->device);
    (void)hipStreamSynchronize(scene->ctx->stream);
    delete scene;
    return MRT_OK;
}
// What the device is handed must be finite: a NaN or an infinity in a position, a normal or a transform is refused here, with the call that brought it, instead of as a
// builder that "made no progress" or as NaN radiance (the reference never sees one: ModelIO's importer produces its meshes, Model.swift:16-21).
static bool all_finite(const float *p, size_t stride_bytes, size_t n, int comps) {
    uint32_t bad = 0;          // exponent field all ones = NaN or infinity; integer ops, no branch and no floating-point dependency chain in the loop
    for (size_t i = 0; i < n; i++) {
        const char *q = (const char *)p + i * stride_bytes;
        for (int k = 0; k < comps; k++) { uint32_t b; memcpy(&b, q + 4 * k, 4); bad |= ((b & 0x7F800000u) + 0x00800000u) >> 31; }
    }
    return bad == 0;
}
static void mark_changed(MRTScene scene) { scene->changes.host_changed(mrt::Pending::rebuild); }      // a mesh, a submesh or an option changed: the next commit builds
static void grow_stage(MRTScene scene, size_t bytes) {          // the pinned staging area of the commit's uploads (see mrt_mesh_add_submesh)
    scene->stage_need += bytes;
    if (scene->stage_need > scene->dev.stage.cap && bind_device(scene->ctx) == MRT_OK) { if (scene->dev.stage.reserve(std::max(scene->stage_need, 2 * scene->dev.stage.cap)) != hipSuccess) (void)hipGetLastError(); }
}
// nverts rows of positions and normals, any multiple of 4 bytes apart, into a mesh's packed arrays
static void copy_vertex_rows(mrt::HostMesh &m, const float *positions, size_t pos_stride, const float *normals, size_t nrm_stride, size_t nverts) {
    for (size_t i = 0; i < nverts; i++) {
        const float *p = (const float *)((const char *)positions + i * pos_stride);
        const float *n = (const float *)((const char *)normals + i * nrm_stride);
        for (int k = 0; k < 3; k++) { m.positions[i * 3 + k] = p[k]; m.normals[i * 3 + k] = n[k]; }
    }
}
// What mrt_scene_update_mesh, _update_mesh_device and _update_blas_device ask of their rows, in this order: the mesh exists, the strides, the buffers' alignment (device_ptrs: the two device pointers, or null for host arrays, which may lie anywhere), the mesh has vertices of its own, and as many as before.
static int check_vertex_rows(const char *who, MRTScene scene, int32_t mesh_id, size_t pos_stride, size_t nrm_stride, size_t nverts, const void *const *device_ptrs) {
    REQUIRE(mesh_id >= 0 && (size_t)mesh_id < scene->meshes.size(), std::string(who) + ": mesh_id out of range");
    REQUIRE(pos_stride >= 12 && nrm_stride >= 12 && pos_stride % 4 == 0 && nrm_stride % 4 == 0, std::string(who) + ": strides must be multiples of 4 and >= 12");
    REQUIRE(!device_ptrs || ((uintptr_t)device_ptrs[0] % 4 == 0 && (uintptr_t)device_ptrs[1] % 4 == 0), std::string(who) + ": buffers must be 4-byte aligned");
    const mrt::HostMesh &m = scene->meshes[(size_t)mesh_id];
    REQUIRE(m.source < 0, std::string(who) + ": an instance has no vertices of its own (update its source mesh)");
    REQUIRE(nverts * 3 == m.positions.size(), std::string(who) + ": the vertex count must stay the same (the topology is kept)");
    return MRT_OK;
}
int mrt_scene_add_mesh(MRTScene scene, const float *positions, size_t pos_stride, const float *normals, size_t nrm_stride,
                       size_t nverts, const float *xf, int32_t *mesh_id) {
    MRT_TRY
    REQUIRE(scene && xf, "mrt_scene_add_mesh: bad argument");
    REQUIRE(nverts == 0 || (positions && normals), "mrt_scene_add_mesh: NULL vertex arrays");
    REQUIRE(pos_stride >= 12 && nrm_stride >= 12 && pos_stride % 4 == 0 && nrm_stride % 4 == 0, "mrt_scene_add_mesh: strides must be multiples of 4 and >= 12");
    REQUIRE(scene->meshes.size() < 65535, "mrt_scene_add_mesh: too many meshes");
    REQUIRE(all_finite(xf, 64, 1, 16), "mrt_scene_add_mesh: the transform holds a NaN or an infinity");
    REQUIRE(nverts == 0 || (all_finite(positions, pos_stride, nverts, 3) && all_finite(normals, nrm_stride, nverts, 3)), "mrt_scene_add_mesh: a position or a normal is NaN or infinite");
    mrt::HostMesh m;
    m.positions.resize(nverts * 3); m.normals.resize(nverts * 3);
    copy_vertex_rows(m, positions, pos_stride, normals, nrm_stride, nverts);
    memcpy(m.xf, xf, 64);
    m.xf[3] = m.xf[7] = m.xf[11] = 0.0f; m.xf[15] = 1.0f;              // matrix4x4_drop_last_row (Utilities.swift:92-101)
    scene->meshes.push_back(std::move(m));
    mark_changed(scene);
    if (mesh_id) *mesh_id = (int32_t)scene->meshes.size() - 1;
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_add_instance(MRTScene scene, int32_t source_mesh_id, const float *xf, int32_t *mesh_id) {
    MRT_TRY
    REQUIRE(scene && xf, "mrt_scene_add_instance: bad argument");
    REQUIRE(source_mesh_id >= 0 && (size_t)source_mesh_id < scene->meshes.size(), "mrt_scene_add_instance: source_mesh_id out of range");
    REQUIRE(scene->meshes.size() < 65535, "mrt_scene_add_instance: too many meshes");
    REQUIRE(all_finite(xf, 64, 1, 16), "mrt_scene_add_instance: the transform holds a NaN or an infinity");
    mrt::HostMesh m;
    const int src = scene->meshes[source_mesh_id].source;
    m.source = src >= 0 ? src : source_mesh_id;                         // instances of an instance share the original's geometry
    memcpy(m.xf, xf, 64);
    m.xf[3] = m.xf[7] = m.xf[11] = 0.0f; m.xf[15] = 1.0f;
    const int geometry_of = m.source;
    scene->meshes.push_back(std::move(m));
    mark_changed(scene);
    if (mesh_id) *mesh_id = (int32_t)scene->meshes.size() - 1;
    if (!scene->opt.instancing) {           // a flattened scene stages a copy of the source's geometry per instance: the pinned area grows here (see mrt_mesh_add_submesh)
        const mrt::HostMesh &g = scene->meshes[geometry_of];
        size_t bytes = g.positions.size() / 3 * 28 + 4096;
        for (auto &ix : g.sub_indices) bytes += ix.size() * 4;
        grow_stage(scene, bytes);
    }
    return MRT_OK;
    MRT_CATCH
}
int mrt_mesh_add_submesh(MRTScene scene, int32_t mesh_id, const uint32_t *indices, size_t ntris, const MRTMaterial *material, int32_t *geometry_id) {
    MRT_TRY
    REQUIRE(scene && material, "mrt_mesh_add_submesh: bad argument");
    REQUIRE(mesh_id >= 0 && (size_t)mesh_id < scene->meshes.size(), "mrt_mesh_add_submesh: mesh_id out of range");
    REQUIRE(ntris == 0 || indices, "mrt_mesh_add_submesh: NULL indices");
    mrt::HostMesh &m = scene->meshes[mesh_id];
    REQUIRE(m.source < 0, "mrt_mesh_add_submesh: the mesh is an instance (mrt_scene_add_instance) and shares its source's submeshes");
    REQUIRE(m.sub_indices.size() < 65535, "mrt_mesh_add_submesh: too many submeshes");
    size_t nv = m.positions.size() / 3;
    for (size_t i = 0; i < ntris * 3; i++) REQUIRE(indices[i] < nv, "mrt_mesh_add_submesh: vertex index out of range");
    m.sub_indices.emplace_back(indices, indices + ntris * 3);
    m.sub_materials.push_back(*material);
    mark_changed(scene);
    if (geometry_id) *geometry_id = (int32_t)m.sub_indices.size() - 1;
    // the pinned staging area the commit uploads from grows HERE, as the geometry is handed over (by doubling: a handful of allocations whatever the mesh count), not inside
    // mrt_scene_commit: pinning 25 MB is ~1.1 ms, a fifth of DragonScene's commit.  Flattened scenes stage every instance's copy; a failure here is not an error (the commit retries).
    if (!scene->opt.instancing || m.source < 0) grow_stage(scene, ntris * 12 + (m.sub_indices.size() == 1 ? nv * 28 : 0) + 4096);
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_add_obj(MRTScene scene, const char *obj_path, const float position[3], const float rotation[3], float scale, int32_t *mesh_id) {
    MRT_TRY
    REQUIRE(scene && obj_path && position && rotation, "mrt_scene_add_obj: bad argument");
    mrt::MeshData md;
    if (!mrt::load_obj(obj_path, md)) return MRT_ERR_IO;
    float xf[16];
    mrt::make_transform(position, rotation, scale, xf);
    int32_t id = -1;
    int rc = mrt_scene_add_mesh(scene, md.positions.data(), 12, md.normals.data(), 12, md.positions.size() / 3, xf, &id);
    if (rc) return rc;
    for (auto &s : md.submeshes) { rc = mrt_mesh_add_submesh(scene, id, s.indices.data(), s.indices.size() / 3, &s.material, nullptr); if (rc) return rc; }
    if (mesh_id) *mesh_id = id;
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_set_lights(MRTScene scene, const MRTLight *lights, int32_t count) {
    MRT_TRY
    REQUIRE(scene && count >= 0 && (count == 0 || lights), "mrt_scene_set_lights: bad argument");
    scene->lights.assign(lights, lights + count);
    if (scene->changes.committed()) { int rc = bind_device(scene->ctx); if (rc) return rc; return mrt::upload_lights(scene->lights.data(), count, scene->ctx->stream, scene->dev); }
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_set_option(MRTScene scene, const char *key, double value) {
    MRT_TRY
    REQUIRE(scene && key, "mrt_scene_set_option: bad argument");
    std::string k(key);
    if (k == "builder") { REQUIRE(value == 0 || value == 1 || value == 2, "builder must be 0 (Karras LBVH), 1 (PLOC) or 2 (binned SAH on the host)"); scene->opt.builder = (int)value; }
    else if (k == "max_leaf") { REQUIRE(value >= 1 && value <= 16, "max_leaf must be in [1,16]"); scene->opt.max_leaf = (int)value; }
    else if (k == "cost_trav") scene->opt.cost_trav = (float)value;
    else if (k == "cost_isect") scene->opt.cost_isect = (float)value;
    else if (k == "wide") scene->opt.wide = (int)value;
    else if (k == "rope") { REQUIRE(value == 0 || value == 1, "rope must be 0 (the rope layout only for scenes without the 8-wide one) or 1 (always)"); scene->opt.rope = (int)value; }
    else if (k == "presplit") { REQUIRE(value >= 0, "presplit must be >= 0 (0 = off; k: triangles longer than k x the mean extent are split into references)"); scene->opt.presplit = (float)value; }
    else if (k == "refit_fenced") { REQUIRE(value == 0 || value == 1, "refit_fenced must be 0 or 1"); scene->opt.refit_fenced = (int)value; }
    else if (k == "validate") { REQUIRE(value == 0 || value == 1, "validate must be 0 or 1"); scene->opt.validate = (int)value; }
    else if (k == "wide_collapse") { REQUIRE(value == 0 || value == 1, "wide_collapse must be 0 (greedy) or 1 (SAH-optimal)"); scene->opt.wide_collapse = (int)value; }
    else if (k == "wide_cost_node") { REQUIRE(value > 0, "wide_cost_node must be positive"); scene->opt.wide_cost_node = (float)value; }
    else if (k == "wide_cost_tri") { REQUIRE(value > 0, "wide_cost_tri must be positive"); scene->opt.wide_cost_tri = (float)value; }
    else if (k == "instancing") { REQUIRE(value == 0 || value == 1, "instancing must be 0 (flatten) or 1 (two-level: shared BLAS per mesh + TLAS)"); scene->opt.instancing = (int)value; }
    else if (k == "refit") scene->opt.refit = value != 0;
    else if (k == "refit_max_cost_ratio") { REQUIRE(value == 0 || value >= 1, "refit_max_cost_ratio must be 0 (off) or >= 1"); scene->opt.refit_max_cost_ratio = (float)value; }
    else if (k == "ploc_radius") { REQUIRE(value >= 1 && value <= 256, "ploc_radius must be in [1,256]"); scene->opt.ploc_radius = (int)value; }
    else { mrt::set_error("mrt_scene_set_option: unknown key " + k); return MRT_ERR_INVALID_ARGUMENT; }
    mark_changed(scene);
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_commit(MRTScene scene) {
    MRT_TRY
    REQUIRE(scene, "mrt_scene_commit: scene is NULL");
    int rc = bind_device(scene->ctx); if (rc) return rc;
    mrt::drop_surface_workspace(scene->dev);          // (the surface entries' slot table restates the mesh list of the commit before; the next such call makes it again)
    // vertices replaced on the device since the last commit (mrt_scene_update_mesh_device): the statistics of those refits are read first (a refit below chains on them), then the
    // meshes' host copies, which everything below reads, are brought up to date
    rc = mrt::resolve_device_refits(scene->dev, scene->opt, scene->ctx->stream); if (rc) return rc;
    rc = sync_host_meshes(scene); if (rc) return rc;
    switch (scene->changes.recipe(scene->opt.instancing, scene->opt.refit, scene->dev.num_inst == scene->meshes.size())) {
    case mrt::CommitRecipe::tlas_only: rc = mrt::update_tlas(scene->meshes, scene->ctx->stream, scene->dev); break;          // instance rows + TLAS; the BLASes stay (the refit of an animated scene)
    case mrt::CommitRecipe::refit_blas_else_build:          // the changed meshes' BLASes refitted in place + the TLAS
        rc = mrt::refit_two_level(scene->meshes, scene->opt, scene->ctx->stream, scene->dev);
        if (rc == MRT_ERR_UNSUPPORTED) rc = mrt::build_scene(scene->meshes, scene->opt, scene->ctx->stream, scene->dev);
        break;
    case mrt::CommitRecipe::build_keep_geometry: rc = mrt::build_scene(scene->meshes, scene->opt, scene->ctx->stream, scene->dev, true, false); break;
    case mrt::CommitRecipe::build_refit: rc = mrt::build_scene(scene->meshes, scene->opt, scene->ctx->stream, scene->dev, false, true); break;
    case mrt::CommitRecipe::build: rc = mrt::build_scene(scene->meshes, scene->opt, scene->ctx->stream, scene->dev); break;
    }
    if (rc) return rc;
    for (auto &m : scene->meshes) m.dirty = false;
    rc = mrt::refit_workspace_after_commit(scene->dev); if (rc) return rc;
    rc = mrt::upload_lights(scene->lights.data(), (int)scene->lights.size(), scene->ctx->stream, scene->dev); if (rc) return rc;
    rc = upload_mesh_masks(scene, false); if (rc) return rc;
    scene->changes.commit_done();
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_update_mesh(MRTScene scene, int32_t mesh_id, const float *positions, size_t pos_stride, const float *normals, size_t nrm_stride, size_t nverts) {
    MRT_TRY
    REQUIRE(scene && positions && normals, "mrt_scene_update_mesh: bad argument");
    if (int rc = check_vertex_rows("mrt_scene_update_mesh", scene, mesh_id, pos_stride, nrm_stride, nverts, nullptr)) return rc;
    mrt::HostMesh &m = scene->meshes[(size_t)mesh_id];
    REQUIRE(all_finite(positions, pos_stride, nverts, 3) && all_finite(normals, nrm_stride, nverts, 3), "mrt_scene_update_mesh: a position or a normal is NaN or infinite (the mesh keeps what it had)");
    copy_vertex_rows(m, positions, pos_stride, normals, nrm_stride, nverts);
    mrt::host_vertices_are_newer(scene->dev, (size_t)mesh_id);          // (replaced on the device before: this copy is the newer one now)
    // a committed scene in which nothing else changes until the next commit keeps its tree: that commit refits (flattened scenes with the 8-wide layout; others build again)
    m.dirty = true;
    scene->changes.host_changed(mrt::Pending::vertices);
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_set_instance_transform(MRTScene scene, int32_t mesh_id, const float *xf) {
    MRT_TRY
    REQUIRE(scene && xf, "mrt_scene_set_instance_transform: bad argument");
    REQUIRE(mesh_id >= 0 && (size_t)mesh_id < scene->meshes.size(), "mrt_scene_set_instance_transform: mesh_id out of range");
    REQUIRE(all_finite(xf, 64, 1, 16), "mrt_scene_set_instance_transform: the transform holds a NaN or an infinity (the instance keeps what it had)");
    float *m = scene->meshes[mesh_id].xf;
    memcpy(m, xf, 64);
    mrt::host_transform_is_newer(scene->dev, (size_t)mesh_id);          // (moved on the device before: this matrix is the newer one now)
    m[3] = m[7] = m[11] = 0.0f; m[15] = 1.0f;
    // flattened scene: the world-space BVH is rebuilt by the next mrt_scene_commit (22 ms for 885 K triangles);
    // two-level scene: the next commit rewrites the instance rows and rebuilds the TLAS only
    scene->changes.host_changed(mrt::Pending::transforms);
    return MRT_OK;
    MRT_CATCH
}
int mrt_scene_stats(MRTScene scene, MRTSceneStats *out) {
    REQUIRE(scene && out, "mrt_scene_stats: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_scene_stats: scene not committed"); return MRT_ERR_STATE; }
    // refits enqueued by mrt_scene_refit_device or by mrt_scene_refit_blas_device: wait for the last one and read what it left (the only place this blocks)
    const bool unresolved[2] = {scene->dev.refit_ws && scene->dev.refit_ws->unresolved, scene->dev.blas_ws && scene->dev.blas_ws->unresolved};
    for (int k = 0; k < 2; k++) if (unresolved[k]) {
        int rc = bind_device(scene->ctx); if (rc) return rc;
        rc = (k == 0 ? mrt::resolve_device_refits : mrt::resolve_blas_refits)(scene->dev, scene->opt, scene->ctx->stream); if (rc) return rc;
    }
    *out = scene->dev.stats;
    out->wide_layout = scene->dev.num_wnodes > 0 ? 1 : 0; out->wide_depth = scene->dev.wide_depth;
    return MRT_OK;
}
int mrt_scene_instance_transform(MRTScene scene, int32_t mesh_id, float out[12]) {
    REQUIRE(scene && out, "mrt_scene_instance_transform: bad argument");
    REQUIRE(mesh_id >= 0 && (size_t)mesh_id < scene->meshes.size(), "mrt_scene_instance_transform: mesh_id out of range");
    const float *m = scene->meshes[mesh_id].xf;
    for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) out[c * 3 + r] = m[c * 4 + r];
    return MRT_OK;
}
int mrt_scene_intersect_closest(MRTScene scene, const MRTRay *rays, size_t n, MRTIntersection *out) {
    MRT_TRY
    REQUIRE(scene && (n == 0 || (rays && out)), "mrt_scene_intersect_closest: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_scene_intersect_closest: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::query_closest(scene->dev, scene->ctx->stream, rays, n, out);
    MRT_CATCH
}
int mrt_scene_intersect_any(MRTScene scene, const MRTRay *rays, size_t n, int32_t *occluded) {
    MRT_TRY
    REQUIRE(scene && (n == 0 || (rays && occluded)), "mrt_scene_intersect_any: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_scene_intersect_any: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::query_any(scene->dev, scene->ctx->stream, rays, n, occluded);
    MRT_CATCH
}
// The stream-ordered forms: device buffers, the caller's stream (0 = HIP's null stream), two launches and nothing else.
// The *_device_counted twins share their twin's body and pass one more pointer: the row count on the device, required there and looked at first.
static int check_count_word(const char *who, const void *d_count, bool counted) {
    if (!counted) return MRT_OK;
    REQUIRE(d_count, std::string(who) + ": d_count is NULL (one uint32 on the device; the entry without _counted takes none)");
    REQUIRE((uintptr_t)d_count % 4 == 0, std::string(who) + ": d_count must be 4-byte aligned");
    return MRT_OK;
}
static int intersect_device(const char *who, MRTScene scene, const void *d_rays, size_t n, void *d_out, void *hip_stream, bool any, const void *d_count = nullptr, bool counted = false) {
    if (int rc = check_count_word(who, d_count, counted)) return rc;
    if (!(scene && (n == 0 || (d_rays && d_out)))) { mrt::set_error(std::string(who) + ": bad argument"); return MRT_ERR_INVALID_ARGUMENT; }
    if (n >= (size_t(1) << 31)) { mrt::set_error(std::string(who) + ": too many rays (n must be below 2^31)"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene->changes.committed()) { mrt::set_error(std::string(who) + ": scene not committed"); return MRT_ERR_STATE; }
    if (n == 0) return MRT_OK;
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return any ? mrt::query_any_device(scene->dev, (hipStream_t)hip_stream, d_rays, n, d_out, d_count) : mrt::query_closest_device(scene->dev, (hipStream_t)hip_stream, d_rays, n, d_out, d_count);
}
int mrt_scene_intersect_closest_device_counted(MRTScene scene, const void *d_rays, size_t n, void *d_out, void *hip_stream, const void *d_count) {
    MRT_TRY
    return intersect_device("mrt_scene_intersect_closest_device_counted", scene, d_rays, n, d_out, hip_stream, false, d_count, true);
    MRT_CATCH
}
int mrt_scene_intersect_any_device_counted(MRTScene scene, const void *d_rays, size_t n, void *d_occluded, void *hip_stream, const void *d_count) {
    MRT_TRY
    return intersect_device("mrt_scene_intersect_any_device_counted", scene, d_rays, n, d_occluded, hip_stream, true, d_count, true);
    MRT_CATCH
}
int mrt_scene_intersect_closest_device(MRTScene scene, const void *d_rays, size_t n, void *d_out, void *hip_stream) {
    MRT_TRY
    return intersect_device("mrt_scene_intersect_closest_device", scene, d_rays, n, d_out, hip_stream, false);
    MRT_CATCH
}
int mrt_scene_intersect_any_device(MRTScene scene, const void *d_rays, size_t n, void *d_occluded, void *hip_stream) {
    MRT_TRY
    return intersect_device("mrt_scene_intersect_any_device", scene, d_rays, n, d_occluded, hip_stream, true);
    MRT_CATCH
}
// All hits in order (multihit.hip, its walk and list in lane_walk.h).  Plain arguments first, as the surface and stage entries check theirs, so that every one of these refusals needs no device; the scene last.
static int intersect_all_entry(const char *who_c, MRTScene scene, const void *d_rays, size_t n, int32_t max_hits, void *d_out, void *d_hit_counts, void *hip_stream, const void *d_count, bool counted) {
    const std::string who(who_c);
    if (int rc = check_count_word(who_c, d_count, counted)) return rc;
    REQUIRE(max_hits >= 1 && max_hits <= MRT_MAX_HITS, who + ": max_hits must be 1 .. " + std::to_string(MRT_MAX_HITS));
    REQUIRE(n < (size_t(1) << 31), who + ": too many rays (n must be below 2^31)");
    REQUIRE(n * (size_t)max_hits < (size_t(1) << 31), who + ": too many records (n * max_hits must be below 2^31)");
    REQUIRE(n == 0 || (d_rays && d_out && d_hit_counts), who + ": NULL buffers");
    REQUIRE((uintptr_t)d_rays % 4 == 0 && (uintptr_t)d_hit_counts % 4 == 0, who + ": rays and hit counts must be 4-byte aligned");
    REQUIRE((uintptr_t)d_out % 16 == 0, who + ": the records must be 16-byte aligned");
    if (!scene) { mrt::set_error(who + ": scene is NULL"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene->changes.committed()) { mrt::set_error(who + ": scene not committed"); return MRT_ERR_STATE; }
    if (scene->opt.instancing || scene->dev.num_inst) {
        mrt::set_error(who + ": two-level scenes (scene option instancing = 1) are not served: the walk across both levels is not written yet; flattened scenes in every layout are");
        return MRT_ERR_UNSUPPORTED;
    }
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(scene->ctx)) return rc;
    return mrt::intersect_all_device(scene->dev, (hipStream_t)hip_stream, d_rays, n, max_hits, d_out, d_hit_counts, d_count);
}
int mrt_scene_intersect_all_device(MRTScene scene, const void *d_rays, size_t n, int32_t max_hits, void *d_out, void *d_hit_counts, void *hip_stream) {
    MRT_TRY
    return intersect_all_entry("mrt_scene_intersect_all_device", scene, d_rays, n, max_hits, d_out, d_hit_counts, hip_stream, nullptr, false);
    MRT_CATCH
}
int mrt_scene_intersect_all_device_counted(MRTScene scene, const void *d_rays, size_t n, int32_t max_hits, void *d_out, void *d_hit_counts, void *hip_stream, const void *d_count) {
    MRT_TRY
    return intersect_all_entry("mrt_scene_intersect_all_device_counted", scene, d_rays, n, max_hits, d_out, d_hit_counts, hip_stream, d_count, true);
    MRT_CATCH
}

// Visibility masks (masked.hip, its walks and filter in lane_walk.h).  Setting masks is no change in the sense of scene_changes.h: the tree does not depend on them.
static int check_mask_range(const char *who_c, MRTScene scene, int32_t first, int32_t count, const void *masks) {
    const std::string who(who_c);
    REQUIRE(scene, who + ": scene is NULL");
    REQUIRE(first >= 0 && count >= 0 && (size_t)first + (size_t)count <= scene->meshes.size(), who + ": mesh ids out of range");
    REQUIRE(count == 0 || masks, who + ": masks is NULL");
    return MRT_OK;
}
int mrt_scene_set_mesh_masks(MRTScene scene, int32_t first_mesh_id, int32_t count, const uint32_t *masks) {
    MRT_TRY
    if (int rc = check_mask_range("mrt_scene_set_mesh_masks", scene, first_mesh_id, count, masks)) return rc;
    if (count == 0) return MRT_OK;
    std::copy(masks, masks + count, mesh_masks_of(scene).begin() + first_mesh_id);
    if (!scene->changes.committed()) { scene->masks_stale = true; return MRT_OK; }          // the commit that has to come uploads the table
    if (int rc = bind_device(scene->ctx)) return rc;
    return upload_mesh_masks(scene, true);
    MRT_CATCH
}
int mrt_scene_get_mesh_masks(MRTScene scene, int32_t first_mesh_id, int32_t count, uint32_t *masks) {
    MRT_TRY
    if (int rc = check_mask_range("mrt_scene_get_mesh_masks", scene, first_mesh_id, count, masks)) return rc;
    const std::vector<uint32_t> &m = mesh_masks_of(scene);
    std::copy(m.begin() + first_mesh_id, m.begin() + first_mesh_id + count, masks);
    return MRT_OK;
    MRT_CATCH
}
// The masked queries: plain arguments first, as intersect_all_entry checks its own, then the scene.  max_hits / d_hit_counts: MASKED_ALL only.
static int intersect_masked_entry(const char *who_c, mrt::MaskedQuery query, MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, int32_t max_hits, void *d_out,
                                  void *d_hit_counts, void *hip_stream, const void *d_count) {
    const std::string who(who_c);
    const bool all = query == mrt::MASKED_ALL, records = query != mrt::MASKED_ANY;
    REQUIRE((uintptr_t)d_count % 4 == 0, who + ": d_count must be 4-byte aligned");
    if (all) REQUIRE(max_hits >= 1 && max_hits <= MRT_MAX_HITS, who + ": max_hits must be 1 .. " + std::to_string(MRT_MAX_HITS));
    REQUIRE(n < (size_t(1) << 31), who + ": too many rays (n must be below 2^31)");
    if (all) REQUIRE(n * (size_t)max_hits < (size_t(1) << 31), who + ": too many records (n * max_hits must be below 2^31)");
    REQUIRE(n == 0 || (d_rays && d_out && (!all || d_hit_counts)), who + ": NULL buffers");
    REQUIRE((uintptr_t)d_rays % 4 == 0 && (uintptr_t)d_ray_masks % 4 == 0 && (uintptr_t)d_hit_counts % 4 == 0, who + ": rays, ray masks and hit counts must be 4-byte aligned");
    REQUIRE((uintptr_t)d_out % (all ? 16 : 4) == 0, all ? who + ": the records must be 16-byte aligned" : who + (records ? ": d_out must be 4-byte aligned" : ": d_occluded must be 4-byte aligned"));          // (as the unmasked twins: the list is written in 16-byte stores, a closest record in words)
    if (!scene) { mrt::set_error(who + ": scene is NULL"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene->changes.committed()) { mrt::set_error(who + ": scene not committed"); return MRT_ERR_STATE; }
    if (all && (scene->opt.instancing || scene->dev.num_inst)) {
        mrt::set_error(who + ": two-level scenes (scene option instancing = 1) are not served: the walk across both levels is not written yet; flattened scenes in every layout are");
        return MRT_ERR_UNSUPPORTED;
    }
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(scene->ctx)) return rc;
    return mrt::intersect_masked_device(scene->dev, (hipStream_t)hip_stream, query, d_rays, d_ray_masks, ray_mask, n, max_hits, d_out, d_hit_counts, d_count);
}
int mrt_scene_intersect_closest_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, void *d_out, void *hip_stream, const void *d_count) {
    MRT_TRY
    return intersect_masked_entry("mrt_scene_intersect_closest_masked_device", mrt::MASKED_CLOSEST, scene, d_rays, d_ray_masks, ray_mask, n, 1, d_out, nullptr, hip_stream, d_count);
    MRT_CATCH
}
int mrt_scene_intersect_any_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, void *d_occluded, void *hip_stream, const void *d_count) {
    MRT_TRY
    return intersect_masked_entry("mrt_scene_intersect_any_masked_device", mrt::MASKED_ANY, scene, d_rays, d_ray_masks, ray_mask, n, 1, d_occluded, nullptr, hip_stream, d_count);
    MRT_CATCH
}
int mrt_scene_intersect_all_masked_device(MRTScene scene, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, int32_t max_hits, void *d_out, void *d_hit_counts, void *hip_stream,
                                          const void *d_count) {
    MRT_TRY
    return intersect_masked_entry("mrt_scene_intersect_all_masked_device", mrt::MASKED_ALL, scene, d_rays, d_ray_masks, ray_mask, n, max_hits, d_out, d_hit_counts, hip_stream, d_count);
    MRT_CATCH
}

// The three families of stream-ordered updates (§10d - §10f) look at the scene before anything else: it exists, it is committed, nothing the host changed waits for a commit.  The family's *_supported call and bind_device follow at the call site.
static int device_entry_prologue(const char *who, MRTScene scene) {
    if (!scene) { mrt::set_error(std::string(who) + ": scene is NULL"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene->changes.committed()) {
        mrt::set_error(std::string(who) + (scene->changes.host_changes_pending() ? ": host-side changes are pending (mrt_scene_commit first)" : ": scene not committed"));
        return MRT_ERR_STATE;
    }
    return MRT_OK;
}
// The stream-ordered refit: vertices from device buffers, the refit kernels on the caller's stream (0 = HIP's null stream), nothing of the host in between.
int mrt_scene_update_mesh_device(MRTScene scene, int32_t mesh_id, const void *d_positions, size_t pos_stride, const void *d_normals, size_t nrm_stride, size_t nverts, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_update_mesh_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::device_refit_supported(scene->dev, scene->opt, who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    REQUIRE(d_positions && d_normals, "mrt_scene_update_mesh_device: NULL buffers");
    const void *const rows[2] = {d_positions, d_normals};
    if (int rc = check_vertex_rows(who, scene, mesh_id, pos_stride, nrm_stride, nverts, rows)) return rc;
    if (int rc = mrt::device_refit_prepare(scene->meshes, scene->opt, scene->dev)) return rc;          // (the first call after a build allocates the workspace; later ones find it)
    return mrt::device_update_mesh(scene->dev, (size_t)mesh_id, d_positions, pos_stride, d_normals, nrm_stride, nverts, (hipStream_t)hip_stream);
    MRT_CATCH
}
int mrt_scene_refit_device(MRTScene scene, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_refit_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::device_refit_supported(scene->dev, scene->opt, who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::device_refit_prepare(scene->meshes, scene->opt, scene->dev)) return rc;
    return mrt::device_refit(scene->dev, (hipStream_t)hip_stream);
    MRT_CATCH
}

// Instances of a two-level scene moved from device buffers (tlas_refit.hip)
int mrt_scene_set_instance_transforms_device(MRTScene scene, int32_t first_mesh_id, size_t count, const void *d_transforms, size_t stride_bytes, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_set_instance_transforms_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::instances_device_supported(scene->dev, scene->opt, who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    REQUIRE(first_mesh_id >= 0 && (size_t)first_mesh_id <= scene->dev.in_tlas.size() && count <= scene->dev.in_tlas.size() - (size_t)first_mesh_id, "mrt_scene_set_instance_transforms_device: mesh ids out of range");
    if (count == 0) return MRT_OK;
    REQUIRE(d_transforms, "mrt_scene_set_instance_transforms_device: NULL buffer");
    REQUIRE(stride_bytes >= 64 && stride_bytes % 4 == 0, "mrt_scene_set_instance_transforms_device: the stride must be a multiple of 4 and >= 64");
    REQUIRE((uintptr_t)d_transforms % 4 == 0, "mrt_scene_set_instance_transforms_device: the buffer must be 4-byte aligned");
    for (size_t i = (size_t)first_mesh_id; i < (size_t)first_mesh_id + count; i++)
        if (!scene->dev.in_tlas[i]) {
            mrt::set_error(std::string(who) + ": instance " + std::to_string(i) + " is not in the TLAS of the last commit (no triangles, or a singular matrix then): mrt_scene_set_instance_transform + mrt_scene_commit brings it in");
            return MRT_ERR_UNSUPPORTED;
        }
    if (int rc = mrt::instances_device_prepare(scene->dev)) return rc;          // (the first call after a commit allocates the workspace; later ones find it)
    return mrt::device_set_instance_transforms(scene->dev, (uint32_t)first_mesh_id, (uint32_t)count, d_transforms, stride_bytes, (hipStream_t)hip_stream);
    MRT_CATCH
}
int mrt_scene_refit_instances_device(MRTScene scene, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_refit_instances_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::instances_device_supported(scene->dev, scene->opt, who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::instances_device_prepare(scene->dev)) return rc;
    return mrt::device_refit_instances(scene->dev, (hipStream_t)hip_stream);
    MRT_CATCH
}
int mrt_scene_rebuild_tlas_device(MRTScene scene, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_rebuild_tlas_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::instances_device_supported(scene->dev, scene->opt, who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::tlas_rebuild_supported(scene->dev, who)) return rc;
    if (int rc = mrt::instances_device_prepare(scene->dev)) return rc;          // (the first call after a commit allocates the workspace; later ones find it)
    return mrt::device_rebuild_tlas(scene->dev, (hipStream_t)hip_stream);
    MRT_CATCH
}

// Meshes of a two-level scene deformed from device buffers (bvh_refit.hip, tlas_refit.hip)
int mrt_scene_update_blas_device(MRTScene scene, int32_t mesh_id, const void *d_positions, size_t pos_stride, const void *d_normals, size_t nrm_stride, size_t nverts, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_update_blas_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::blas_device_supported(scene->dev, scene->opt, scene->meshes.size(), who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    REQUIRE(d_positions && d_normals, "mrt_scene_update_blas_device: NULL buffers");
    const void *const rows[2] = {d_positions, d_normals};
    if (int rc = check_vertex_rows(who, scene, mesh_id, pos_stride, nrm_stride, nverts, rows)) return rc;
    size_t b = 0;
    while (b < scene->dev.blas_ranges.size() && scene->dev.blas_ranges[b].src_mesh != (uint32_t)mesh_id) b++;
    if (b == scene->dev.blas_ranges.size() || !mrt::blas_refittable(scene->dev.blas_ranges[b], nverts) || scene->dev.blas_ranges[b].ntri == 0) {
        mrt::set_error(std::string(who) + ": the BLAS of mesh " + std::to_string(mesh_id) + " has no 8-wide nodes or no triangles: there is nothing to refit");
        return MRT_ERR_UNSUPPORTED;
    }
    if (int rc = mrt::blas_device_prepare(scene->meshes, scene->dev)) return rc;          // (the first call after a commit allocates the workspace; later ones find it)
    return mrt::device_update_blas(scene->dev, b, d_positions, pos_stride, d_normals, nrm_stride, nverts, (hipStream_t)hip_stream);
    MRT_CATCH
}
int mrt_scene_refit_blas_device(MRTScene scene, void *hip_stream) {
    MRT_TRY
    const char *who = "mrt_scene_refit_blas_device";
    if (int rc = device_entry_prologue(who, scene)) return rc;
    if (int rc = mrt::blas_device_supported(scene->dev, scene->opt, scene->meshes.size(), who)) return rc;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::instances_device_supported(scene->dev, scene->opt, who)) return rc;          // (its last step is the TLAS refit of §10e)
    if (int rc = mrt::blas_device_prepare(scene->meshes, scene->dev)) return rc;
    if (int rc = mrt::instances_device_prepare(scene->dev)) return rc;
    return mrt::device_refit_blas(scene->dev, (hipStream_t)hip_stream);
    MRT_CATCH
}
int mrt_scene_device_updates_rejected(MRTScene scene, uint64_t *count) {
    MRT_TRY
    REQUIRE(scene && count, "mrt_scene_device_updates_rejected: bad argument");
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::device_updates_rejected(scene->dev, count);
    MRT_CATCH
}

// Hit records resolved to surface data on the caller's stream (surface.hip).  The plain arguments are checked before the scene is looked at: a refusal
// of theirs needs no device.
static int surface_prologue(const char *who, MRTScene scene, size_t n) {
    if (n >= (size_t(1) << 31)) { mrt::set_error(std::string(who) + ": too many hits (n must be below 2^31)"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene) { mrt::set_error(std::string(who) + ": scene is NULL"); return MRT_ERR_INVALID_ARGUMENT; }
    if (!scene->changes.committed()) { mrt::set_error(std::string(who) + ": scene not committed"); return MRT_ERR_STATE; }
    return MRT_OK;
}
static int resolve_hits_entry(const char *who, MRTScene scene, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, void *hip_stream, const void *d_count, bool counted) {
    if (int rc = check_count_word(who, d_count, counted)) return rc;
    REQUIRE(n == 0 || (d_rays && d_hits && d_surfaces), std::string(who) + ": NULL buffers");
    REQUIRE((uintptr_t)d_rays % 16 == 0 && (uintptr_t)d_hits % 16 == 0 && (uintptr_t)d_surfaces % 16 == 0, std::string(who) + ": buffers must be 16-byte aligned");
    if (int rc = surface_prologue(who, scene, n)) return rc;
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::surface_prepare(scene->meshes, scene->dev)) return rc;          // (the first call after a commit makes the slot table; later ones find it)
    return mrt::resolve_hits_device(scene->dev, (hipStream_t)hip_stream, d_rays, d_hits, n, d_surfaces, d_count);
}
int mrt_scene_resolve_hits_device(MRTScene scene, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, void *hip_stream) {
    MRT_TRY
    return resolve_hits_entry("mrt_scene_resolve_hits_device", scene, d_rays, d_hits, n, d_surfaces, hip_stream, nullptr, false);
    MRT_CATCH
}
int mrt_scene_resolve_hits_device_counted(MRTScene scene, const void *d_rays, const void *d_hits, size_t n, void *d_surfaces, void *hip_stream, const void *d_count) {
    MRT_TRY
    return resolve_hits_entry("mrt_scene_resolve_hits_device_counted", scene, d_rays, d_hits, n, d_surfaces, hip_stream, d_count, true);
    MRT_CATCH
}
static int interpolate_entry(const char *who_c, MRTScene scene, const void *d_hits, size_t n, const void *d_attributes, size_t attr_stride, int32_t channels, void *d_out, size_t out_stride, void *hip_stream,
                             const void *d_count, bool counted) {
    const std::string who(who_c);
    if (int rc = check_count_word(who_c, d_count, counted)) return rc;
    REQUIRE(channels >= 1 && channels <= 64, who + ": channels must be 1 .. 64");
    REQUIRE(attr_stride >= 4 * (size_t)channels && out_stride >= 4 * (size_t)channels, who + ": a row stride is below 4 x channels bytes");
    REQUIRE(attr_stride % 4 == 0 && out_stride % 4 == 0, who + ": row strides must be multiples of 4");
    REQUIRE(n == 0 || (d_hits && d_attributes && d_out), who + ": NULL buffers");
    REQUIRE((uintptr_t)d_hits % 16 == 0, who + ": the hit records must be 16-byte aligned");
    REQUIRE((uintptr_t)d_attributes % 4 == 0 && (uintptr_t)d_out % 4 == 0, who + ": attributes and output must be 4-byte aligned");
    if (int rc = surface_prologue(who_c, scene, n)) return rc;
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(scene->ctx)) return rc;
    if (int rc = mrt::surface_prepare(scene->meshes, scene->dev)) return rc;
    return mrt::interpolate_device(scene->dev, (hipStream_t)hip_stream, d_hits, n, d_attributes, attr_stride, (uint32_t)channels, d_out, out_stride, d_count);
}
int mrt_scene_interpolate_device(MRTScene scene, const void *d_hits, size_t n, const void *d_attributes, size_t attr_stride, int32_t channels, void *d_out, size_t out_stride, void *hip_stream) {
    MRT_TRY
    return interpolate_entry("mrt_scene_interpolate_device", scene, d_hits, n, d_attributes, attr_stride, channels, d_out, out_stride, hip_stream, nullptr, false);
    MRT_CATCH
}
int mrt_scene_interpolate_device_counted(MRTScene scene, const void *d_hits, size_t n, const void *d_attributes, size_t attr_stride, int32_t channels, void *d_out, size_t out_stride, void *hip_stream,
                                         const void *d_count) {
    MRT_TRY
    return interpolate_entry("mrt_scene_interpolate_device_counted", scene, d_hits, n, d_attributes, attr_stride, channels, d_out, out_stride, hip_stream, d_count, true);
    MRT_CATCH
}
int mrt_scene_vertex_offsets(MRTScene scene, uint64_t *offsets, size_t count) {
    MRT_TRY
    REQUIRE(scene && offsets, "mrt_scene_vertex_offsets: bad argument");
    REQUIRE(count == scene->meshes.size() + 1, "mrt_scene_vertex_offsets: count must be the number of meshes + 1");
    std::vector<uint64_t> o; mrt::surface_vertex_offsets(scene->meshes, o);
    std::copy(o.begin(), o.end(), offsets);
    return MRT_OK;
    MRT_CATCH
}

// What follows a surface, on the caller's stream (stages.hip).  Plain arguments first, as the surface entries: a refusal of theirs needs no device.
// What the two scatter entries share once their own buffers and bounce counts have passed (those come first, in each entry's order): light_count as a plain argument, the scene (surface_prologue), its lights, the exit for n = 0 (*done, with MRT_OK) and the device.
static int scatter_prologue(const char *who, MRTScene scene, size_t n, int32_t light_count, bool *done) {
    *done = true;
    REQUIRE(light_count >= 0, std::string(who) + ": light_count must be >= 0 (0 = every light of the scene)");
    if (int rc = surface_prologue(who, scene, n)) return rc;
    REQUIRE(light_count <= scene->dev.light_count, std::string(who) + ": light_count is above the number of lights of the scene");
    if (scene->dev.light_count < 1) { mrt::set_error(std::string(who) + ": scene has no lights (lightCount must be >= 1, Raytracing.metal:273)"); return MRT_ERR_STATE; }
    if (n == 0) return MRT_OK;
    *done = false;
    return bind_device(scene->ctx);
}
static int scatter_entry(const char *who_c, MRTScene scene, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t light_count, void *d_shadow_rays, void *d_light,
                         void *d_next_rays, void *hip_stream, const void *d_count, bool counted) {
    const std::string who(who_c);
    if (int rc = check_count_word(who_c, d_count, counted)) return rc;
    REQUIRE(n == 0 || (d_surfaces && d_halton_index && d_shadow_rays && d_light), who + ": NULL buffers (d_surfaces, d_halton_index, d_shadow_rays and d_light are required; only d_next_rays may be NULL)");
    REQUIRE((uintptr_t)d_surfaces % 16 == 0 && (uintptr_t)d_shadow_rays % 16 == 0 && (uintptr_t)d_light % 16 == 0 && (uintptr_t)d_next_rays % 16 == 0,
            who + ": d_surfaces, d_shadow_rays, d_light and d_next_rays must be 16-byte aligned");
    REQUIRE((uintptr_t)d_halton_index % 4 == 0, who + ": d_halton_index must be 4-byte aligned");
    REQUIRE(bounce >= 0 && bounce <= 18, who + ": bounce must be in [0, 18] (Halton dimensions 2 + 5 * bounce .. + 4 of a table of 100 primes)");
    bool done = false;
    if (const int rc = scatter_prologue(who_c, scene, n, light_count, &done); rc || done) return rc;
    return mrt::scatter_device(scene->dev, (hipStream_t)hip_stream, d_surfaces, d_halton_index, n, bounce, light_count > 0 ? light_count : scene->dev.light_count, d_shadow_rays, d_light, d_next_rays, d_count);
}
int mrt_scene_scatter_device(MRTScene scene, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t light_count, void *d_shadow_rays, void *d_light,
                             void *d_next_rays, void *hip_stream) {
    MRT_TRY
    return scatter_entry("mrt_scene_scatter_device", scene, d_surfaces, d_halton_index, n, bounce, light_count, d_shadow_rays, d_light, d_next_rays, hip_stream, nullptr, false);
    MRT_CATCH
}
int mrt_scene_scatter_device_counted(MRTScene scene, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t light_count, void *d_shadow_rays, void *d_light,
                                     void *d_next_rays, void *hip_stream, const void *d_count) {
    MRT_TRY
    return scatter_entry("mrt_scene_scatter_device_counted", scene, d_surfaces, d_halton_index, n, bounce, light_count, d_shadow_rays, d_light, d_next_rays, hip_stream, d_count, true);
    MRT_CATCH
}

// The same step with the materials extension on (stages_materials.hip): mrt_scene_scatter_device's rules, plus the incoming rays, the lobe rows and max_bounces
static int scatter_materials_entry(const char *who_c, MRTScene scene, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t max_bounces, int32_t light_count,
                                   void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes, void *hip_stream, const void *d_count, bool counted) {
    const std::string who(who_c);
    if (int rc = check_count_word(who_c, d_count, counted)) return rc;
    REQUIRE(n == 0 || (d_rays && d_surfaces && d_halton_index && d_shadow_rays && d_light && d_lobes),
            who + ": NULL buffers (d_rays, d_surfaces, d_halton_index, d_shadow_rays, d_light and d_lobes are required; only d_next_rays may be NULL)");
    REQUIRE((uintptr_t)d_rays % 16 == 0 && (uintptr_t)d_surfaces % 16 == 0 && (uintptr_t)d_shadow_rays % 16 == 0 && (uintptr_t)d_light % 16 == 0 && (uintptr_t)d_next_rays % 16 == 0 && (uintptr_t)d_lobes % 16 == 0,
            who + ": d_rays, d_surfaces, d_shadow_rays, d_light, d_next_rays and d_lobes must be 16-byte aligned");
    REQUIRE((uintptr_t)d_halton_index % 4 == 0, who + ": d_halton_index must be 4-byte aligned");
    REQUIRE(max_bounces >= 1 && max_bounces <= 16, who + ": max_bounces must be in [1, 16] (the lobe choice uses Halton dimension 2 + 5 * max_bounces + bounce of a table of 100 primes)");
    REQUIRE(bounce >= 0 && bounce < max_bounces, who + ": bounce must be in [0, max_bounces)");
    bool done = false;
    if (const int rc = scatter_prologue(who_c, scene, n, light_count, &done); rc || done) return rc;
    return mrt::scatter_materials_device(scene->dev, (hipStream_t)hip_stream, d_rays, d_surfaces, d_halton_index, n, bounce, max_bounces, light_count > 0 ? light_count : scene->dev.light_count,
                                         d_shadow_rays, d_light, d_next_rays, d_lobes, d_count);
}
int mrt_scene_scatter_materials_device(MRTScene scene, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t max_bounces, int32_t light_count,
                                       void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes, void *hip_stream) {
    MRT_TRY
    return scatter_materials_entry("mrt_scene_scatter_materials_device", scene, d_rays, d_surfaces, d_halton_index, n, bounce, max_bounces, light_count, d_shadow_rays, d_light, d_next_rays, d_lobes, hip_stream,
                                   nullptr, false);
    MRT_CATCH
}
int mrt_scene_scatter_materials_device_counted(MRTScene scene, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int32_t bounce, int32_t max_bounces, int32_t light_count,
                                               void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes, void *hip_stream, const void *d_count) {
    MRT_TRY
    return scatter_materials_entry("mrt_scene_scatter_materials_device_counted", scene, d_rays, d_surfaces, d_halton_index, n, bounce, max_bounces, light_count, d_shadow_rays, d_light, d_next_rays, d_lobes,
                                   hip_stream, d_count, true);
    MRT_CATCH
}

// Row queues on the caller's stream (queues.hip).  Plain arguments first, in the header's order, each message naming its argument; the context last.
size_t mrt_compact_workspace_bytes(size_t n) { return mrt::compact_workspace_bytes(n); }
int mrt_context_compact_rows_device(MRTContext ctx, const void *d_keep, size_t n, const void *d_count_in, const MRTRowColumn *columns, int32_t ncolumns, void *d_count_out, void *d_workspace,
                                    size_t workspace_bytes, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_compact_rows_device";
    REQUIRE(n < (size_t(1) << 31), who + ": too many rows (n must be below 2^31)");
    REQUIRE(n == 0 || d_keep, who + ": d_keep is NULL");
    REQUIRE(n == 0 || d_count_out, who + ": d_count_out is NULL");
    REQUIRE(n == 0 || d_workspace, who + ": d_workspace is NULL");
    REQUIRE((uintptr_t)d_count_in % 4 == 0, who + ": d_count_in must be 4-byte aligned");
    REQUIRE((uintptr_t)d_count_out % 4 == 0, who + ": d_count_out must be 4-byte aligned");
    REQUIRE(!d_count_out || d_count_out != d_count_in, who + ": d_count_out must not be d_count_in (the kernels read the one after the other was written)");
    REQUIRE(ncolumns >= 0 && ncolumns <= mrt::COMPACT_MAX_COLUMNS, who + ": ncolumns must be 0 .. 8");
    REQUIRE(ncolumns == 0 || columns, who + ": columns is NULL with ncolumns > 0");
    struct Range { uintptr_t lo, hi; const char *what; };
    auto overlap = [](const Range &a, const Range &b) { return a.lo < b.hi && b.lo < a.hi; };
    for (int c = 0; c < ncolumns; c++) {
        const MRTRowColumn &col = columns[c];
        const std::string name = who + ": columns[" + std::to_string(c) + "]";
        REQUIRE(col.row_bytes != 0 && col.row_bytes <= 64 && col.row_bytes % 4 == 0, name + ".row_bytes must be a multiple of 4 in 4 .. 64");
        const uintptr_t align = col.row_bytes % 16 == 0 ? 16 : 4;
        REQUIRE(n == 0 || (col.src && col.dst), name + ": src or dst is NULL");
        REQUIRE((uintptr_t)col.src % align == 0, name + ".src must be " + std::to_string(align) + "-byte aligned for rows of " + std::to_string(col.row_bytes) + " bytes");
        REQUIRE((uintptr_t)col.dst % align == 0, name + ".dst must be " + std::to_string(align) + "-byte aligned for rows of " + std::to_string(col.row_bytes) + " bytes");
    }
    for (int c = 0; c < ncolumns && n; c++) {
        const std::string name = who + ": columns[" + std::to_string(c) + "].dst";
        const Range dst = {(uintptr_t)columns[c].dst, (uintptr_t)columns[c].dst + n * columns[c].row_bytes, ""};
        const Range others[4] = {{(uintptr_t)columns[c].src, (uintptr_t)columns[c].src + n * columns[c].row_bytes, "its own src"}, {(uintptr_t)d_keep, (uintptr_t)d_keep + n, "d_keep"},
                                 {(uintptr_t)d_count_in, (uintptr_t)d_count_in + (d_count_in ? 4 : 0), "d_count_in"}, {(uintptr_t)d_count_out, (uintptr_t)d_count_out + 4, "d_count_out"}};
        for (const Range &o : others) REQUIRE(!overlap(dst, o), name + " overlaps " + o.what);
        for (int k = 0; k < c; k++) {
            const Range od = {(uintptr_t)columns[k].dst, (uintptr_t)columns[k].dst + n * columns[k].row_bytes, ""};
            REQUIRE(!overlap(dst, od), name + " overlaps columns[" + std::to_string(k) + "].dst");
        }
    }
    REQUIRE((uintptr_t)d_workspace % 16 == 0, who + ": d_workspace must be 16-byte aligned");
    REQUIRE(n == 0 || workspace_bytes >= mrt::compact_workspace_bytes(n), who + ": workspace_bytes is below mrt_compact_workspace_bytes(n)");
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0 && !d_count_out) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::compact_rows_device((hipStream_t)hip_stream, d_keep, n, d_count_in, columns, ncolumns, d_count_out, d_workspace);
    MRT_CATCH
}

// The integrator's path state on the caller's stream (paths.hip).  Plain arguments first, each message naming its argument; the context last.
#define REQUIRE_ALIGNED(ptr, bytes) REQUIRE((uintptr_t)(ptr) % (bytes) == 0, who + ": " #ptr " must be " #bytes "-byte aligned")
#define REQUIRE_GIVEN(ptr) REQUIRE(n == 0 || (ptr), who + ": " #ptr " is NULL")
int mrt_context_reset_paths_device(MRTContext ctx, size_t n, void *d_throughput, void *d_pixel, void *d_radiance, size_t npixels, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_reset_paths_device";
    REQUIRE(n < (size_t(1) << 31), who + ": too many rows (n must be below 2^31)");
    REQUIRE(npixels < (size_t(1) << 31), who + ": too many pixels (npixels must be below 2^31)");
    REQUIRE_GIVEN(d_throughput); REQUIRE_GIVEN(d_pixel);
    REQUIRE_ALIGNED(d_throughput, 16); REQUIRE_ALIGNED(d_pixel, 4); REQUIRE_ALIGNED(d_radiance, 16);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::reset_paths_device((hipStream_t)hip_stream, n, d_throughput, d_pixel, d_radiance, npixels);
    MRT_CATCH
}
int mrt_context_advance_paths_device(MRTContext ctx, size_t n, const void *d_count, const void *d_surfaces, const void *d_lobes, const void *d_light, void *d_throughput, const void *d_pixel,
                                     void *d_radiance, size_t npixels, void *d_keep_shadow, void *d_keep_path, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_advance_paths_device";
    REQUIRE(n < (size_t(1) << 31), who + ": too many rows (n must be below 2^31)");
    REQUIRE(npixels < (size_t(1) << 31), who + ": too many pixels (npixels must be below 2^31)");
    REQUIRE(!(d_surfaces && d_lobes), who + ": both d_surfaces and d_lobes are given (exactly one: the diffuse form or the materials form)");
    REQUIRE(n == 0 || d_surfaces || d_lobes, who + ": neither d_surfaces nor d_lobes is given (exactly one: the diffuse form or the materials form)");
    REQUIRE_GIVEN(d_light); REQUIRE_GIVEN(d_throughput); REQUIRE_GIVEN(d_keep_shadow);
    if (d_lobes) {
        REQUIRE(n == 0 || d_pixel, who + ": d_pixel is NULL (the materials form deposits emission)");
        REQUIRE(n == 0 || d_radiance, who + ": d_radiance is NULL (the materials form deposits emission)");
    }
    REQUIRE_ALIGNED(d_count, 4); REQUIRE_ALIGNED(d_surfaces, 16); REQUIRE_ALIGNED(d_lobes, 16); REQUIRE_ALIGNED(d_light, 16); REQUIRE_ALIGNED(d_throughput, 16);
    REQUIRE_ALIGNED(d_pixel, 4); REQUIRE_ALIGNED(d_radiance, 16);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::advance_paths_device((hipStream_t)hip_stream, n, d_count, d_surfaces, d_lobes, d_light, d_throughput, d_pixel, d_radiance, npixels, d_keep_shadow, d_keep_path);
    MRT_CATCH
}
int mrt_context_deposit_light_device(MRTContext ctx, size_t n, const void *d_count, const void *d_occluded, const void *d_light, const void *d_throughput, const void *d_pixel, void *d_radiance,
                                     size_t npixels, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_deposit_light_device";
    REQUIRE(n < (size_t(1) << 31), who + ": too many rows (n must be below 2^31)");
    REQUIRE(npixels < (size_t(1) << 31), who + ": too many pixels (npixels must be below 2^31)");
    REQUIRE_GIVEN(d_occluded); REQUIRE_GIVEN(d_light); REQUIRE_GIVEN(d_throughput); REQUIRE_GIVEN(d_pixel); REQUIRE_GIVEN(d_radiance);
    REQUIRE_ALIGNED(d_count, 4); REQUIRE_ALIGNED(d_occluded, 4); REQUIRE_ALIGNED(d_light, 16); REQUIRE_ALIGNED(d_throughput, 16); REQUIRE_ALIGNED(d_pixel, 4); REQUIRE_ALIGNED(d_radiance, 16);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::deposit_light_device((hipStream_t)hip_stream, n, d_count, d_occluded, d_light, d_throughput, d_pixel, d_radiance, npixels);
    MRT_CATCH
}
int mrt_context_fold_sample_device(MRTContext ctx, size_t npixels, void *d_sample, void *d_accum, uint32_t frame_index, int32_t clear_sample, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_fold_sample_device";
    const size_t n = npixels;
    REQUIRE(npixels < (size_t(1) << 31), who + ": too many pixels (npixels must be below 2^31)");
    REQUIRE(frame_index != 0xFFFFFFFFu, who + ": frame_index must be below 2^32 - 1 (the fold divides by frame_index + 1)");
    REQUIRE_GIVEN(d_sample); REQUIRE_GIVEN(d_accum);
    REQUIRE_ALIGNED(d_sample, 16); REQUIRE_ALIGNED(d_accum, 16);
    REQUIRE(!d_sample || d_sample != d_accum, who + ": d_sample must not be d_accum");
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::fold_sample_device((hipStream_t)hip_stream, npixels, d_sample, d_accum, frame_index, clear_sample != 0);
    MRT_CATCH
}

// From a composed frame to an image a host can show, on the caller's stream (image.hip).  The same order: plain arguments, each message naming its
// argument; the context last.
namespace {
struct ByteRange { uintptr_t lo, hi; const char *what; };
inline ByteRange byte_range(const void *p, size_t bytes, const char *what) { return {(uintptr_t)p, (uintptr_t)p + bytes, what}; }
inline bool ranges_overlap(const ByteRange &a, const ByteRange &b) { return a.lo < b.hi && b.lo < a.hi; }
}  // namespace
#define REQUIRE_IMAGE_SIZE() \
    REQUIRE(width > 0, who + ": width must be above 0"); REQUIRE(height > 0, who + ": height must be above 0"); \
    REQUIRE((uint64_t)width * (uint64_t)height < (uint64_t(1) << 30), who + ": too many pixels (width * height must be below 2^30)")
int mrt_context_fold_guides_device(MRTContext ctx, size_t npixels, const void *d_surfaces, void *d_normal_depth, void *d_albedo, void *d_ids, uint32_t frame_index, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_fold_guides_device";
    const size_t n = npixels;
    REQUIRE(npixels < (size_t(1) << 31), who + ": too many pixels (npixels must be below 2^31)");
    REQUIRE(frame_index != 0xFFFFFFFFu, who + ": frame_index must be below 2^32 - 1 (the fold divides by frame_index + 1)");
    REQUIRE_GIVEN(d_surfaces); REQUIRE_GIVEN(d_normal_depth); REQUIRE_GIVEN(d_albedo); REQUIRE_GIVEN(d_ids);
    REQUIRE_ALIGNED(d_surfaces, 16); REQUIRE_ALIGNED(d_normal_depth, 16); REQUIRE_ALIGNED(d_albedo, 16); REQUIRE_ALIGNED(d_ids, 16);
    const ByteRange bufs[4] = {byte_range(d_surfaces, 0, "d_surfaces"), byte_range(d_normal_depth, 0, "d_normal_depth"), byte_range(d_albedo, 0, "d_albedo"), byte_range(d_ids, 0, "d_ids")};
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) REQUIRE(!bufs[a].lo || bufs[a].lo != bufs[b].lo, who + ": " + bufs[a].what + " must not be " + bufs[b].what);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (n == 0) return MRT_OK;
    if (int rc = bind_device(ctx)) return rc;
    return mrt::fold_guides_device((hipStream_t)hip_stream, npixels, d_surfaces, d_normal_depth, d_albedo, d_ids, frame_index);
    MRT_CATCH
}
int mrt_denoise_workspace_bytes(int32_t width, int32_t height, size_t *bytes) {
    MRT_TRY
    const std::string who = "mrt_denoise_workspace_bytes";
    REQUIRE_IMAGE_SIZE();
    REQUIRE(bytes, who + ": bytes is NULL");
    *bytes = mrt::denoise_workspace_bytes(width, height);
    return MRT_OK;
    MRT_CATCH
}
int mrt_context_denoise_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, const void *d_normal_depth, const void *d_albedo, void *d_workspace, size_t workspace_bytes,
                               void *d_out, const MRTDenoiseParams *params, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_denoise_device";
    REQUIRE_IMAGE_SIZE();
    MRTDenoiseParams p{};
    if (params) p = *params;
    else { p.iterations = MRT_DENOISE_DEFAULT_ITERATIONS; p.sigma_color = MRT_DENOISE_DEFAULT_SIGMA_COLOR; p.sigma_normal = MRT_DENOISE_DEFAULT_SIGMA_NORMAL; p.sigma_depth = MRT_DENOISE_DEFAULT_SIGMA_DEPTH; p.demodulate = 1; }
    // Renderer::enqueue_denoise's checks and words
    REQUIRE(p.iterations >= 1 && p.iterations <= 8, who + ": denoise: iterations must be in [1,8]");
    const float big = 3.0e38f;
    REQUIRE((p.sigma_color > 0.0f && p.sigma_color < big) && (p.sigma_normal > 0.0f && p.sigma_normal < big) && (p.sigma_depth > 0.0f && p.sigma_depth < big),
            who + ": denoise: sigma_color, sigma_normal and sigma_depth must be finite and > 0");
    REQUIRE(p.demodulate == 0 || p.demodulate == 1, who + ": denoise: demodulate must be 0 or 1");
    const size_t n = (size_t)width * (size_t)height, image_bytes = n * 16, need = mrt::denoise_workspace_bytes(width, height);
    REQUIRE_GIVEN(d_image); REQUIRE_GIVEN(d_normal_depth); REQUIRE_GIVEN(d_albedo); REQUIRE_GIVEN(d_workspace); REQUIRE_GIVEN(d_out);
    REQUIRE_ALIGNED(d_image, 16); REQUIRE_ALIGNED(d_normal_depth, 16); REQUIRE_ALIGNED(d_albedo, 16); REQUIRE_ALIGNED(d_workspace, 16); REQUIRE_ALIGNED(d_out, 16);
    REQUIRE(workspace_bytes >= need, who + ": workspace_bytes is below mrt_denoise_workspace_bytes(width, height)");
    const ByteRange inputs[3] = {byte_range(d_image, image_bytes, "d_image"), byte_range(d_normal_depth, image_bytes, "d_normal_depth"), byte_range(d_albedo, image_bytes, "d_albedo")};
    const ByteRange work = byte_range(d_workspace, need, "d_workspace"), out = byte_range(d_out, image_bytes, "d_out");
    for (const ByteRange &in : inputs) {
        REQUIRE(!ranges_overlap(out, in), who + ": d_out overlaps " + in.what);
        REQUIRE(!ranges_overlap(work, in), who + ": d_workspace overlaps " + in.what);
    }
    REQUIRE(!ranges_overlap(out, work), who + ": d_out overlaps d_workspace");
    REQUIRE(ctx, who + ": ctx is NULL");
    if (int rc = bind_device(ctx)) return rc;
    return mrt::denoise_image_device((hipStream_t)hip_stream, width, height, d_image, d_normal_depth, d_albedo, d_workspace, d_out, p);
    MRT_CATCH
}
int mrt_context_tonemap_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, void *d_rgba8, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_tonemap_device";
    REQUIRE_IMAGE_SIZE();
    const size_t n = (size_t)width * (size_t)height;
    REQUIRE_GIVEN(d_image); REQUIRE_GIVEN(d_rgba8);
    REQUIRE_ALIGNED(d_image, 16); REQUIRE_ALIGNED(d_rgba8, 4);
    REQUIRE(!ranges_overlap(byte_range(d_rgba8, n * 4, ""), byte_range(d_image, n * 16, "")), who + ": d_rgba8 overlaps d_image");
    REQUIRE(ctx, who + ": ctx is NULL");
    if (int rc = bind_device(ctx)) return rc;
    return mrt::tonemap_image_device((hipStream_t)hip_stream, width, height, d_image, d_rgba8);
    MRT_CATCH
}
// Temporal reprojection of the accumulated image (temporal.hip).  The same order again.
int mrt_context_reproject_device(MRTContext ctx, int32_t width, int32_t height, const MRTCamera *camera, const MRTCamera *prev_camera, const void *d_surfaces,
                                 const void *d_prev_position, const void *d_prev_normal_depth, const void *d_prev_ids, const void *d_prev_history, const void *d_sample,
                                 void *d_out, const MRTReprojectParams *params, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_reproject_device";
    REQUIRE_IMAGE_SIZE();
    REQUIRE(width < (1 << 24), who + ": width must be below 2^24 (a column is a float)"); REQUIRE(height < (1 << 24), who + ": height must be below 2^24 (a row is a float)");
    REQUIRE(camera, who + ": camera is NULL"); REQUIRE(prev_camera, who + ": prev_camera is NULL");
    MRTReprojectParams p{};
    if (params) p = *params;
    else { p.max_history = MRT_REPROJECT_DEFAULT_MAX_HISTORY; p.min_cos_normal = MRT_REPROJECT_DEFAULT_MIN_COS_NORMAL; p.depth_tolerance = MRT_REPROJECT_DEFAULT_DEPTH_TOLERANCE; }
    REQUIRE(p.max_history >= 1.0f && p.max_history < 3.0e38f, who + ": max_history must be finite and at least 1");
    REQUIRE(p.min_cos_normal == p.min_cos_normal, who + ": min_cos_normal is NaN");
    REQUIRE(p.depth_tolerance >= 0.0f, who + ": depth_tolerance must be at least 0 and not NaN");
    const size_t n = (size_t)width * (size_t)height, image_bytes = n * 16;
    REQUIRE_GIVEN(d_surfaces); REQUIRE_GIVEN(d_prev_normal_depth); REQUIRE_GIVEN(d_prev_ids); REQUIRE_GIVEN(d_prev_history); REQUIRE_GIVEN(d_sample); REQUIRE_GIVEN(d_out);
    REQUIRE_ALIGNED(d_surfaces, 16); REQUIRE_ALIGNED(d_prev_position, 16); REQUIRE_ALIGNED(d_prev_normal_depth, 16); REQUIRE_ALIGNED(d_prev_ids, 16);
    REQUIRE_ALIGNED(d_prev_history, 16); REQUIRE_ALIGNED(d_sample, 16); REQUIRE_ALIGNED(d_out, 16);
    const ByteRange inputs[6] = {byte_range(d_surfaces, n * sizeof(MRTSurface), "d_surfaces"), byte_range(d_prev_position, d_prev_position ? image_bytes : 0, "d_prev_position"),
                                 byte_range(d_prev_normal_depth, image_bytes, "d_prev_normal_depth"), byte_range(d_prev_ids, image_bytes, "d_prev_ids"),
                                 byte_range(d_prev_history, image_bytes, "d_prev_history"), byte_range(d_sample, image_bytes, "d_sample")};
    const ByteRange out = byte_range(d_out, image_bytes, "d_out");
    for (const ByteRange &in : inputs) REQUIRE(!ranges_overlap(out, in), who + ": d_out overlaps " + in.what);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (int rc = bind_device(ctx)) return rc;
    return mrt::reproject_device((hipStream_t)hip_stream, width, height, *camera, *prev_camera, d_surfaces, d_prev_position, d_prev_normal_depth, d_prev_ids, d_prev_history, d_sample,
                                 d_out, p);
    MRT_CATCH
}
// The variance-guided filter and the sample image of its moments (variance.hip).  The same order again; the filter's checks are
// mrt_context_denoise_device's with d_moments a fourth input.
int mrt_context_moments_sample_device(MRTContext ctx, int32_t width, int32_t height, const void *d_sample, const void *d_albedo, int32_t demodulate, void *d_out, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_moments_sample_device";
    REQUIRE_IMAGE_SIZE();
    const size_t n = (size_t)width * (size_t)height, image_bytes = n * 16;
    REQUIRE_GIVEN(d_sample); REQUIRE_GIVEN(d_albedo); REQUIRE_GIVEN(d_out);
    REQUIRE_ALIGNED(d_sample, 16); REQUIRE_ALIGNED(d_albedo, 16); REQUIRE_ALIGNED(d_out, 16);
    const ByteRange inputs[2] = {byte_range(d_sample, image_bytes, "d_sample"), byte_range(d_albedo, image_bytes, "d_albedo")};
    const ByteRange out = byte_range(d_out, image_bytes, "d_out");
    for (const ByteRange &in : inputs) REQUIRE(!ranges_overlap(out, in), who + ": d_out overlaps " + in.what);
    REQUIRE(ctx, who + ": ctx is NULL");
    if (int rc = bind_device(ctx)) return rc;
    return mrt::moments_sample_device((hipStream_t)hip_stream, width, height, d_sample, d_albedo, demodulate != 0, d_out);
    MRT_CATCH
}
int mrt_context_denoise_variance_device(MRTContext ctx, int32_t width, int32_t height, const void *d_image, const void *d_moments, const void *d_normal_depth, const void *d_albedo,
                                        void *d_workspace, size_t workspace_bytes, void *d_out, const MRTDenoiseParams *params, void *hip_stream) {
    MRT_TRY
    const std::string who = "mrt_context_denoise_variance_device";
    REQUIRE_IMAGE_SIZE();
    REQUIRE(height <= MRT_VARIANCE_MAX_HEIGHT, who + ": height must be at most 524280 (rows of 8 pixels per workgroup, 65535 workgroups in y)");
    MRTDenoiseParams p{};
    if (params) p = *params;
    else { p.iterations = MRT_DENOISE_DEFAULT_ITERATIONS; p.sigma_color = MRT_DENOISE_DEFAULT_SIGMA_COLOR; p.sigma_normal = MRT_DENOISE_DEFAULT_SIGMA_NORMAL; p.sigma_depth = MRT_DENOISE_DEFAULT_SIGMA_DEPTH; p.demodulate = 1; }
    REQUIRE(p.iterations >= 1 && p.iterations <= 8, who + ": denoise: iterations must be in [1,8]");
    const float big = 3.0e38f;
    REQUIRE((p.sigma_color > 0.0f && p.sigma_color < big) && (p.sigma_normal > 0.0f && p.sigma_normal < big) && (p.sigma_depth > 0.0f && p.sigma_depth < big),
            who + ": denoise: sigma_color, sigma_normal and sigma_depth must be finite and > 0");
    REQUIRE(p.demodulate == 0 || p.demodulate == 1, who + ": denoise: demodulate must be 0 or 1");
    const size_t n = (size_t)width * (size_t)height, image_bytes = n * 16, need = mrt::denoise_workspace_bytes(width, height);
    REQUIRE_GIVEN(d_image); REQUIRE_GIVEN(d_moments); REQUIRE_GIVEN(d_normal_depth); REQUIRE_GIVEN(d_albedo); REQUIRE_GIVEN(d_workspace); REQUIRE_GIVEN(d_out);
    REQUIRE_ALIGNED(d_image, 16); REQUIRE_ALIGNED(d_moments, 16); REQUIRE_ALIGNED(d_normal_depth, 16); REQUIRE_ALIGNED(d_albedo, 16); REQUIRE_ALIGNED(d_workspace, 16); REQUIRE_ALIGNED(d_out, 16);
    REQUIRE(workspace_bytes >= need, who + ": workspace_bytes is below mrt_denoise_workspace_bytes(width, height)");
    const ByteRange inputs[4] = {byte_range(d_image, image_bytes, "d_image"), byte_range(d_moments, image_bytes, "d_moments"), byte_range(d_normal_depth, image_bytes, "d_normal_depth"),
                                 byte_range(d_albedo, image_bytes, "d_albedo")};
    const ByteRange work = byte_range(d_workspace, need, "d_workspace"), out = byte_range(d_out, image_bytes, "d_out");
    for (const ByteRange &in : inputs) {
        REQUIRE(!ranges_overlap(out, in), who + ": d_out overlaps " + in.what);
        REQUIRE(!ranges_overlap(work, in), who + ": d_workspace overlaps " + in.what);
    }
    REQUIRE(!ranges_overlap(out, work), who + ": d_out overlaps d_workspace");
    REQUIRE(ctx, who + ": ctx is NULL");
    if (int rc = bind_device(ctx)) return rc;
    return mrt::denoise_variance_device((hipStream_t)hip_stream, width, height, d_image, d_moments, d_normal_depth, d_albedo, d_workspace, d_out, p);
    MRT_CATCH
}
#undef REQUIRE_IMAGE_SIZE
#undef REQUIRE_ALIGNED
#undef REQUIRE_GIVEN

int mrt_debug_traversal_stats(MRTScene scene, const MRTRay *rays, size_t n, int32_t any_hit, uint32_t *out4) {
    MRT_TRY
    REQUIRE(scene && (n == 0 || (rays && out4)), "mrt_debug_traversal_stats: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_traversal_stats: scene not committed"); return MRT_ERR_STATE; }
    if (scene->dev.num_inst) { mrt::set_error("mrt_debug_traversal_stats: not available for two-level scenes"); return MRT_ERR_UNSUPPORTED; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::query_stats(scene->dev, scene->ctx->stream, rays, n, any_hit, out4);
    MRT_CATCH
}

int mrt_debug_stream_stats(MRTScene scene, const MRTRay *rays, size_t n, int32_t any_hit, uint32_t per_wave, uint32_t *out8, size_t nwaves) {
    MRT_TRY
    REQUIRE(scene && rays && out8 && per_wave >= 64 && nwaves * (size_t)per_wave >= n, "mrt_debug_stream_stats: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_stream_stats: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::query_stream_stats(scene->dev, scene->ctx->stream, rays, n, any_hit, per_wave, out8, nwaves);
    MRT_CATCH
}

int mrt_debug_intersect_stream(MRTScene scene, const MRTRay *rays, size_t n, int32_t any_hit, MRTIntersection *out) {
    MRT_TRY
    REQUIRE(scene && rays && out, "mrt_debug_intersect_stream: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_intersect_stream: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::query_stream(scene->dev, scene->ctx->stream, rays, n, any_hit ? 1 : 0, out);
    MRT_CATCH
}

#ifdef MRT_WAVE_TIMES
extern "C++" { namespace mrt { int read_wave_times(unsigned long long *out); int read_wave_iters(uint32_t *out); int read_drain_probe(unsigned long long *out18, int reset); } }
extern "C" int mrt_debug_drain_probe(unsigned long long *out18, int reset) { return mrt::read_drain_probe(out18, reset); }
extern "C" int mrt_debug_wave_times(unsigned long long *out16384) { return mrt::read_wave_times(out16384); }
extern "C" int mrt_debug_wave_iters(uint32_t *out32768) { return mrt::read_wave_iters(out32768); }
#endif

// ---------------------------------------------------------------- host geometry helpers
int mrt_obj_load(const char *obj_path, MRTMeshData *out) {
    MRT_TRY
    REQUIRE(obj_path && out, "mrt_obj_load: bad argument");
    std::unique_ptr<MRTMeshData_> m(new MRTMeshData_());
    if (!mrt::load_obj(obj_path, m->m)) return MRT_ERR_IO;
    *out = m.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_dragon_proxy(MRTMeshData *out) {
    MRT_TRY
    REQUIRE(out, "mrt_dragon_proxy: out is NULL");
    std::unique_ptr<MRTMeshData_> m(new MRTMeshData_());
    mrt::make_dragon_proxy(m->m);
    *out = m.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_dragon_proxy_irregular(MRTMeshData *out) {
    MRT_TRY
    REQUIRE(out, "mrt_dragon_proxy_irregular: out is NULL");
    std::unique_ptr<MRTMeshData_> m(new MRTMeshData_());
    mrt::make_dragon_proxy_irregular(m->m);
    *out = m.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_dragon_proxy_hostile(MRTMeshData *out) {
    MRT_TRY
    REQUIRE(out, "mrt_dragon_proxy_hostile: out is NULL");
    std::unique_ptr<MRTMeshData_> m(new MRTMeshData_());
    mrt::make_dragon_proxy_hostile(m->m);
    *out = m.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_bunny_proxy(MRTMeshData *out) {
    MRT_TRY
    REQUIRE(out, "mrt_bunny_proxy: out is NULL");
    std::unique_ptr<MRTMeshData_> m(new MRTMeshData_());
    mrt::make_bunny_proxy(m->m);
    *out = m.release();
    return MRT_OK;
    MRT_CATCH
}
int mrt_meshdata_free(MRTMeshData m) { delete m; return MRT_OK; }
int mrt_meshdata_counts(MRTMeshData m, size_t *nverts, int32_t *nsub) {
    REQUIRE(m, "mrt_meshdata_counts: NULL");
    if (nverts) *nverts = m->m.positions.size() / 3;
    if (nsub) *nsub = (int32_t)m->m.submeshes.size();
    return MRT_OK;
}
int mrt_meshdata_vertices(MRTMeshData m, float *positions, float *normals) {
    REQUIRE(m, "mrt_meshdata_vertices: NULL");
    if (positions) memcpy(positions, m->m.positions.data(), m->m.positions.size() * 4);
    if (normals) memcpy(normals, m->m.normals.data(), m->m.normals.size() * 4);
    return MRT_OK;
}
int mrt_meshdata_submesh(MRTMeshData m, int32_t sub, size_t *ntris, uint32_t *indices, MRTMaterial *material, char *name_buf, size_t name_buflen) {
    REQUIRE(m, "mrt_meshdata_submesh: NULL");
    REQUIRE(sub >= 0 && (size_t)sub < m->m.submeshes.size(), "mrt_meshdata_submesh: submesh out of range");
    const mrt::Submesh &s = m->m.submeshes[sub];
    if (ntris) *ntris = s.indices.size() / 3;
    if (indices) memcpy(indices, s.indices.data(), s.indices.size() * 4);
    if (material) *material = s.material;
    if (name_buf && name_buflen) snprintf(name_buf, name_buflen, "%s", s.name.c_str());
    return MRT_OK;
}
int mrt_make_transform(const float position[3], const float rotation[3], float scale, float out16[16]) {
    REQUIRE(position && rotation && out16, "mrt_make_transform: bad argument");
    mrt::make_transform(position, rotation, scale, out16);
    return MRT_OK;
}
int mrt_default_camera(int32_t width, int32_t height, MRTCamera *out) {
    REQUIRE(out && width > 0 && height > 0, "mrt_default_camera: bad argument");
    mrt::default_camera(width, height, out);
    return MRT_OK;
}

// ---------------------------------------------------------------- renderer
int mrt_renderer_create(MRTContext ctx, MRTScene scene, int32_t width, int32_t height, uint32_t seed, int32_t max_bounces, MRTRenderer *out) {
    MRT_TRY
    REQUIRE(ctx && scene && out, "mrt_renderer_create: bad argument");
    REQUIRE(width > 0 && height > 0 && (int64_t)width * height < (1ll << 30), "mrt_renderer_create: bad size");
    REQUIRE(max_bounces >= 1 && max_bounces <= 19, "mrt_renderer_create: max_bounces must be in [1,19] (Halton prime table holds 100 primes)");
    REQUIRE(scene->ctx == ctx, "mrt_renderer_create: scene belongs to another context");
    if (!scene->changes.committed()) { mrt::set_error("mrt_renderer_create: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(ctx); if (rc) return rc;
    std::unique_ptr<MRTRenderer_> r(new MRTRenderer_());
    r->ctx = ctx; r->scene = scene;
    rc = r->r.init(ctx->stream, &scene->dev, width, height, seed, max_bounces); if (rc) return rc;
    *out = r.release(); scene->renderers++; ctx->live++;
    return MRT_OK;
    MRT_CATCH
}
int mrt_renderer_destroy(MRTRenderer r) {
    if (!r) return MRT_OK;
    r->scene->renderers--; r->ctx->live--;
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(r->ctx->stream);
    delete r;
    return MRT_OK;
}
#define RENDERER_PROLOGUE(name)                                     \
    REQUIRE(r, name ": renderer is NULL");                          \
    { int rc_ = bind_device(r->ctx); if (rc_) return rc_; }         \
    r->r.stream = r->ctx->stream;

int mrt_renderer_resize(MRTRenderer r, int32_t width, int32_t height) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_resize")
    REQUIRE(width > 0 && height > 0 && (int64_t)width * height < (1ll << 30), "mrt_renderer_resize: bad size");
    MRT_HIP(hipStreamSynchronize(r->r.stream));
    return r->r.resize(width, height);
    MRT_CATCH
}
int mrt_renderer_set_camera(MRTRenderer r, const MRTCamera *camera) {
    REQUIRE(r && camera, "mrt_renderer_set_camera: bad argument");
    r->r.camera = *camera;
    return MRT_OK;
}
// updateUniforms (Renderer.swift:216-229) as ONE call: size, frame index, light count and camera.  blocksWide is derived (the reference
// computes it from the size, :222, and its kernel never reads it).
int mrt_renderer_set_uniforms(MRTRenderer r, const MRTUniforms *u) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_set_uniforms")
    REQUIRE(u, "mrt_renderer_set_uniforms: uniforms is NULL");
    REQUIRE(u->width > 0 && u->height > 0 && (int64_t)u->width * u->height < (1ll << 30), "mrt_renderer_set_uniforms: bad size");
    REQUIRE(u->lightCount >= 1 && u->lightCount <= r->scene->dev.light_count, "mrt_renderer_set_uniforms: lightCount must be in [1, lights of the scene]");
    if (u->width != r->r.width || u->height != r->r.height) {          // mtkView(_:drawableSizeWillChange:): new targets, new seeds (Renderer.swift:353-356)
        MRT_HIP(hipStreamSynchronize(r->r.stream));
        int rc = r->r.resize(u->width, u->height); if (rc) return rc;
    }
    r->r.frame_index = u->frameIndex;
    r->r.light_count_limit = u->lightCount == r->scene->dev.light_count ? 0 : u->lightCount;
    r->r.camera = u->camera;
    return MRT_OK;
    MRT_CATCH
}
int mrt_renderer_get_uniforms(MRTRenderer r, MRTUniforms *u) {
    REQUIRE(r && u, "mrt_renderer_get_uniforms: bad argument");
    memset(u, 0, sizeof *u);
    u->width = r->r.width; u->height = r->r.height; u->blocksWide = (r->r.width + 7) / 8;
    u->frameIndex = r->r.frame_index;
    u->lightCount = r->r.light_count_limit > 0 ? std::min(r->r.light_count_limit, r->scene->dev.light_count) : r->scene->dev.light_count;
    u->camera = r->r.camera;
    return MRT_OK;
}
// commandBuffer.addCompletedHandler (Renderer.swift:285-287) as a poll: frames (since create / resize / reset_stats) whose accumulation
// has finished on the device.  Never blocks; mrt_renderer_wait is the blocking form.
int mrt_renderer_frames_completed(MRTRenderer r, uint64_t *frames) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_frames_completed")
    REQUIRE(frames, "mrt_renderer_frames_completed: NULL");
    return r->r.poll_completed(frames);
    MRT_CATCH
}
// The host's knobs: the reference's own (the bounce count, Raytracing.metal:237; maxFramesInFlight, Renderer.swift:33; the shard's sample offset) + three of this implementation.
int mrt_renderer_set_option(MRTRenderer r, const char *key, double value) {
    MRT_TRY
    REQUIRE(r && key, "mrt_renderer_set_option: bad argument");
    std::string k(key);
    if (k == "max_bounces") { REQUIRE(value >= 1 && value <= (r->r.materials ? 16 : 19), "max_bounces must be in [1,19] ([1,16] with materials = 1)"); r->r.max_bounces = (int)value; }
    else if (k == "frames_in_flight") { REQUIRE(value >= 1 && value <= mrt::MAX_FRAMES_IN_FLIGHT, "frames_in_flight must be in [1,16]"); r->r.frames_in_flight = (int)value; }
    else if (k == "sample_offset") { REQUIRE(value >= 0 && value < 4294967296.0, "sample_offset out of range"); r->r.sample_offset = (uint32_t)value; }
    else if (k == "frame_batch") { REQUIRE(value >= 0 && value <= mrt::MAX_FRAME_BATCH, "frame_batch must be in [1,32], or 0 for the default (by image size)"); r->r.frame_batch = (int)value; }
    else if (k == "megakernel") r->r.megakernel = value != 0;
    else if (k == "guides") { REQUIRE(value == 0 || value == 1, "guides must be 0 or 1"); int rc = bind_device(r->ctx); if (rc) return rc; r->r.stream = r->ctx->stream; rc = r->r.set_guides(value != 0); if (rc) return rc; }
    else if (k == "materials") { REQUIRE(value == 0 || (value == 1 && r->r.max_bounces <= 16), "materials must be 0 or 1 (and max_bounces <= 16: the lobe choice uses Halton dimension 2 + 5 * max_bounces + bounce < 100)"); r->r.materials = value != 0; }
    else { mrt::set_error("mrt_renderer_set_option: unknown key " + k + " (keys: max_bounces, frames_in_flight, sample_offset, frame_batch, megakernel, materials, guides; the library's A/B switches are behind mrt_debug_renderer_set_option)"); return MRT_ERR_INVALID_ARGUMENT; }
    return MRT_OK;
    MRT_CATCH
}
int mrt_renderer_get_option(MRTRenderer r, const char *key, double *value) {
    MRT_TRY
    REQUIRE(r && key && value, "mrt_renderer_get_option: bad argument");
    std::string k(key);
    if (k == "max_bounces") *value = r->r.max_bounces;
    else if (k == "frames_in_flight") *value = r->r.frames_in_flight;
    else if (k == "sample_offset") *value = r->r.sample_offset;
    else if (k == "frame_batch") *value = r->r.batch_wanted();          // (what is in force: under the default, 8 at 1080p and above, up to 32 for smaller images and shards)
    else if (k == "megakernel") *value = r->r.megakernel ? 1 : 0;
    else if (k == "materials") *value = r->r.materials ? 1 : 0;
    else if (k == "guides") *value = r->r.guides ? 1 : 0;
    else if (k == "lanes_used") *value = r->r.lanes_used;
    else if (k == "lane_bytes") *value = (double)r->r.lane_bytes();
    else { mrt::set_error("mrt_renderer_get_option: unknown key " + k); return MRT_ERR_INVALID_ARGUMENT; }
    return MRT_OK;
    MRT_CATCH
}
// The library's A/B switches and launch-shape parameters (tests, tools/, bench.py --opt): every setting renders the same image bit for bit.  Not part of the host contract:
// keys come and go with the experiments that need them.  Also accepts the public keys.
int mrt_debug_renderer_set_option(MRTRenderer r, const char *key, double value) {
    MRT_TRY
    REQUIRE(r && key, "mrt_debug_renderer_set_option: bad argument");
    std::string k(key);
    if (k == "persistent") { REQUIRE(value == 0 || value == 1 || value == 2, "persistent must be 0 (never), 1 (always) or 2 (by launch size)"); r->r.persistent = (int)value; }
    else if (k == "xcd_counters") { REQUIRE(value == 0 || value == 1, "xcd_counters must be 0 or 1"); r->r.xcd_counters = (int)value; }
    else if (k == "queue_segments") { REQUIRE(value == 1 || value == 8, "queue_segments must be 1 or 8"); r->r.queue_segments = r->r.segments_used = (int)value; }
    else if (k == "tile_groups") { REQUIRE(value >= 0 && value <= mrt::MAX_TILE_GROUPS && value == (int)value, "tile_groups must be 0 (by the draw), 1 (never) or 2..4"); r->r.tile_groups = (int)value; }
    else if (k == "shade_pack") { REQUIRE(value == 0 || value == 1, "shade_pack must be 0 or 1"); r->r.shade_pack = (int)value; }
    else if (k == "hit_lds") { REQUIRE(value == 0 || value == 1, "hit_lds must be 0 or 1"); r->r.hit_lds = (int)value; }
    else if (k == "persist_chunk") { REQUIRE(value >= 64 && value <= 65536 && ((int)value % 64) == 0, "persist_chunk must be a multiple of 64 in [64, 65536]"); r->r.persist_chunk = (int)value; }
    else if (k == "wave_slots") { REQUIRE(value >= 1 && value <= (1 << 20), "wave_slots must be in [1, 2^20]"); r->r.wave_slots = (int)value; r->r.wave_slots_user = true; }
    else if (k == "stream_stride") { REQUIRE(value >= 0 && value <= 2, "stream_stride must be 0 (contiguous ranges), 1 (round-robin batches) or 2 (round-robin for a shard's launches)"); r->r.stream_stride = (int)value; }
    else if (k == "halton_table") r->r.halton_table = value != 0;
    else if (k == "equal_passes") r->r.equal_passes = value != 0;
    else if (k == "frame_bundle") { REQUIRE(value == 0 || value == 1, "frame_bundle must be 0 (off) or 1 (the sub-frames of a slot side by side in a wave)"); r->r.frame_bundle = (int)value; }
    else if (k == "stream_even") { REQUIRE(value >= 0 && value <= 1600, "stream_even must be in [0,1600] (percent of the wave slots; 0 = off)"); r->r.stream_even = (int)value; }
    else if (k == "primary_hint") r->r.primary_hint = value != 0;
    else if (k == "throughput_chain") r->r.throughput_chain = value != 0;
    else if (k == "shadow_planes") r->r.shadow_planes = value != 0 ? 1 : 0;
    else if (k == "tail_accumulate") r->r.tail_accumulate = value != 0;
    else if (k == "fuse_primary") { REQUIRE(value == 0 || value == 1 || value == 2, "fuse_primary must be 0, 1 (not for one frame alone) or 2 (always)"); r->r.fuse_primary = (int)value; }
    else if (k == "wide_bounce") r->r.wide_bounce = value != 0;
    else if (k == "tl_pair_cap") { REQUIRE(value >= 0 && value <= 4294967295.0, "tl_pair_cap out of range"); r->r.tl_pair_cap = (int)std::min(value, 2147483647.0); }
    else if (k == "tl_pairs") { REQUIRE(value == 0 || value == 1 || value == 2, "tl_pairs must be 0 (two-level scenes walked in one loop), 1 (TLAS pass + BLAS pass over (ray, instance) pairs) or 2 (the same, the TLAS pass always as a walk of the 8-wide TLAS)"); r->r.tl_pairs = (int)value; }
    else if (k == "primary_wide") { REQUIRE(value == 0 || value == 1 || value == 2, "primary_wide must be 0 (rope walk inside shade(0)), 1 (own launch of the 8-wide stream kernel) or 2 (8-wide walk inside shade(0))"); r->r.primary_wide = (int)value; }
    else return mrt_renderer_set_option(r, key, value);
    return MRT_OK;
    MRT_CATCH
}
int mrt_debug_renderer_get_option(MRTRenderer r, const char *key, double *value) {
    MRT_TRY
    REQUIRE(r && key && value, "mrt_debug_renderer_get_option: bad argument");
    std::string k(key);
    if (k == "persistent") *value = r->r.persistent;
    else if (k == "persist_chunk") *value = r->r.persist_chunk;
    else if (k == "hit_lds") *value = r->r.hit_lds;
    else if (k == "shade_pack") *value = r->r.shade_pack;
    else if (k == "tile_groups") *value = r->r.tile_groups;
    else if (k == "groups_used") *value = r->r.groups_used;
    else if (k == "xcd_counters") *value = r->r.xcd_counters;
    else if (k == "queue_segments") *value = r->r.segments_used;
    else if (k == "wave_slots") *value = r->r.wave_slots;
    else if (k == "stream_stride") *value = r->r.stream_stride;
    else if (k == "halton_table") *value = r->r.halton_table;
    else if (k == "frame_bundle") *value = r->r.frame_bundle;
    else if (k == "stream_even") *value = r->r.stream_even;
    else if (k == "primary_hint") *value = r->r.primary_hint ? 1 : 0;
    else if (k == "throughput_chain") *value = r->r.throughput_chain ? 1 : 0;
    else if (k == "shadow_planes") *value = r->r.shadow_planes;
    else if (k == "tail_accumulate") *value = r->r.tail_accumulate ? 1 : 0;
    else if (k == "fuse_primary") *value = r->r.fuse_primary;
    else if (k == "wide_bounce") *value = r->r.wide_bounce ? 1 : 0;
    else if (k == "tl_pairs") *value = r->r.tl_pairs;
    else if (k == "tl_pair_cap") *value = r->r.tl_pair_cap;
    else if (k == "primary_wide") *value = r->r.primary_wide;
    else return mrt_renderer_get_option(r, key, value);
    return MRT_OK;
    MRT_CATCH
}
int mrt_renderer_set_shard(MRTRenderer r, int32_t rank, int32_t world) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_set_shard")
    return r->r.set_shard(rank, world);
    MRT_CATCH
}
// Where the rays come from, on the caller's stream (stages.hip): reads the renderer's size, seed and camera, writes nothing of its own
int mrt_renderer_primary_rays_device(MRTRenderer r, uint32_t sample_index, void *d_rays, void *d_halton_index, void *hip_stream) {
    MRT_TRY
    REQUIRE(d_rays && d_halton_index, "mrt_renderer_primary_rays_device: NULL buffers (d_rays, d_halton_index)");
    REQUIRE((uintptr_t)d_rays % 16 == 0, "mrt_renderer_primary_rays_device: d_rays must be 16-byte aligned");
    REQUIRE((uintptr_t)d_halton_index % 4 == 0, "mrt_renderer_primary_rays_device: d_halton_index must be 4-byte aligned");
    REQUIRE(r, "mrt_renderer_primary_rays_device: renderer is NULL");
    if (int rc = bind_device(r->ctx)) return rc;
    return mrt::primary_rays_device(r->r, (hipStream_t)hip_stream, sample_index, d_rays, d_halton_index);
    MRT_CATCH
}
int mrt_renderer_set_frame_index(MRTRenderer r, uint32_t fi) { REQUIRE(r, "mrt_renderer_set_frame_index: NULL"); r->r.frame_index = fi; return MRT_OK; }
int mrt_renderer_frame_index(MRTRenderer r, uint32_t *fi) { REQUIRE(r && fi, "mrt_renderer_frame_index: bad argument"); *fi = r->r.frame_index; return MRT_OK; }
int mrt_renderer_render(MRTRenderer r, int32_t n_frames) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_render")
    REQUIRE(n_frames >= 0, "mrt_renderer_render: n_frames < 0");
    if (!r->scene->changes.committed()) { mrt::set_error("mrt_renderer_render: scene was modified and not re-committed"); return MRT_ERR_STATE; }
    if (n_frames == 0) return MRT_OK;
    return r->r.render(n_frames);
    MRT_CATCH
}
int mrt_renderer_wait(MRTRenderer r) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_wait")
    return r->r.wait();
    MRT_CATCH
}
int mrt_renderer_read_accum(MRTRenderer r, float *rgba, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_read_accum")
    REQUIRE(rgba, "mrt_renderer_read_accum: NULL buffer");
    return r->r.read_accum(rgba, nbytes);
    MRT_CATCH
}
int mrt_renderer_copy_accum_to_device(MRTRenderer r, void *dptr, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_copy_accum_to_device")
    REQUIRE(dptr, "mrt_renderer_copy_accum_to_device: NULL pointer");
    return r->r.copy_accum_to_device(dptr, nbytes);
    MRT_CATCH
}
int mrt_renderer_write_accum_from_device(MRTRenderer r, const void *dptr, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_write_accum_from_device")
    REQUIRE(dptr, "mrt_renderer_write_accum_from_device: NULL pointer");
    return r->r.write_accum_from_device(dptr, nbytes);
    MRT_CATCH
}
int mrt_renderer_shard_tiles(MRTRenderer r, int32_t rank, int32_t world, uint64_t *tiles) {
    REQUIRE(r && tiles && world >= 1 && rank >= 0 && rank < world, "mrt_renderer_shard_tiles: bad argument");
    *tiles = mrt::shard_tiles(r->r.width, r->r.height, rank, world);
    return MRT_OK;
}
int mrt_renderer_pack_owned_tiles(MRTRenderer r, void *dptr, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_pack_owned_tiles")
    REQUIRE(dptr || nbytes == 0, "mrt_renderer_pack_owned_tiles: NULL pointer");
    return r->r.pack_owned_tiles(dptr, nbytes);
    MRT_CATCH
}
int mrt_renderer_unpack_tiles(MRTRenderer r, const void *dptr, size_t nbytes, int32_t rank, int32_t world) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_unpack_tiles")
    REQUIRE(dptr || nbytes == 0, "mrt_renderer_unpack_tiles: NULL pointer");
    return r->r.unpack_tiles(dptr, nbytes, rank, world);
    MRT_CATCH
}
int mrt_renderer_unpack_tiles_into(MRTRenderer r, void *image, size_t image_nbytes, const void *dptr, size_t nbytes, int32_t rank, int32_t world) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_unpack_tiles_into")
    REQUIRE(dptr || nbytes == 0, "mrt_renderer_unpack_tiles_into: NULL pointer");
    REQUIRE(image && image_nbytes == (size_t)r->r.width * r->r.height * 16, "mrt_renderer_unpack_tiles_into: image must be width*height*16 bytes of device memory");
    return mrt::unpack_tiles_into((float4 *)image, r->r.width, r->r.height, dptr, nbytes, rank, world, r->r.stream);
    MRT_CATCH
}
int mrt_renderer_read_tonemapped_rgba8(MRTRenderer r, uint8_t *rgba, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_read_tonemapped_rgba8")
    REQUIRE(rgba, "mrt_renderer_read_tonemapped_rgba8: NULL buffer");
    return r->r.read_tonemapped(rgba, nbytes);
    MRT_CATCH
}
// ---- first-hit guide buffers and the denoiser (no counterpart in the reference; include/mrt_abi.h)
int mrt_renderer_read_guide(MRTRenderer r, int32_t which, void *out, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_read_guide")
    REQUIRE(out, "mrt_renderer_read_guide: NULL buffer");
    return r->r.read_guide(which, out, nbytes);
    MRT_CATCH
}
int mrt_renderer_copy_guide_to_device(MRTRenderer r, int32_t which, void *dptr, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_copy_guide_to_device")
    REQUIRE(dptr, "mrt_renderer_copy_guide_to_device: NULL pointer");
    return r->r.copy_guide_to_device(which, dptr, nbytes);
    MRT_CATCH
}
int mrt_renderer_denoise(MRTRenderer r, const MRTDenoiseParams *params) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_denoise")
    return r->r.enqueue_denoise(params);
    MRT_CATCH
}
int mrt_renderer_read_denoised(MRTRenderer r, float *rgba, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_read_denoised")
    REQUIRE(rgba, "mrt_renderer_read_denoised: NULL buffer");
    return r->r.read_denoised(rgba, nbytes);
    MRT_CATCH
}
int mrt_renderer_copy_denoised_to_device(MRTRenderer r, void *dptr, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_copy_denoised_to_device")
    REQUIRE(dptr, "mrt_renderer_copy_denoised_to_device: NULL pointer");
    return r->r.copy_denoised_to_device(dptr, nbytes);
    MRT_CATCH
}
int mrt_renderer_read_denoised_tonemapped_rgba8(MRTRenderer r, uint8_t *rgba, size_t nbytes) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_read_denoised_tonemapped_rgba8")
    REQUIRE(rgba, "mrt_renderer_read_denoised_tonemapped_rgba8: NULL buffer");
    return r->r.read_denoised_tonemapped(rgba, nbytes);
    MRT_CATCH
}
int mrt_renderer_stats(MRTRenderer r, MRTRenderStats *out) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_stats")
    REQUIRE(out, "mrt_renderer_stats: NULL");
    return r->r.stats(out);
    MRT_CATCH
}
int mrt_renderer_kernel_times(MRTRenderer r, MRTKernelTimes *out) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_kernel_times")
    REQUIRE(out, "mrt_renderer_kernel_times: NULL");
    int rc = r->r.wait(); if (rc) return rc;
    *out = r->r.kernel_times;
    return MRT_OK;
    MRT_CATCH
}
int mrt_renderer_reset_stats(MRTRenderer r) {
    MRT_TRY
    RENDERER_PROLOGUE("mrt_renderer_reset_stats")
    return r->r.reset_stats();
    MRT_CATCH
}

// ---------------------------------------------------------------- probes
int mrt_debug_halton(MRTContext ctx, const int32_t *i, const int32_t *d, size_t n, float *out) {
    MRT_TRY
    REQUIRE(ctx && (n == 0 || (i && d && out)), "mrt_debug_halton: bad argument");
    for (size_t k = 0; k < n; k++) REQUIRE(d[k] >= 0 && d[k] < 100, "mrt_debug_halton: 0 <= d < 100 required");
    int rc = bind_device(ctx); if (rc) return rc;
    return mrt::probe_halton(ctx->stream, i, d, n, out);
    MRT_CATCH
}
int mrt_debug_hemisphere(MRTContext ctx, const float *u2, const float *n3, size_t n, float *out3) {
    MRT_TRY
    REQUIRE(ctx && (n == 0 || (u2 && n3 && out3)), "mrt_debug_hemisphere: bad argument");
    int rc = bind_device(ctx); if (rc) return rc;
    return mrt::probe_hemisphere(ctx->stream, u2, n3, n, out3);
    MRT_CATCH
}
int mrt_debug_seeds(MRTContext ctx, uint32_t seed, int32_t width, int32_t height, uint32_t *out) {
    MRT_TRY
    REQUIRE(ctx && out && width > 0 && height > 0, "mrt_debug_seeds: bad argument");
    int rc = bind_device(ctx); if (rc) return rc;
    return mrt::probe_seeds(ctx->stream, seed, width, height, out);
    MRT_CATCH
}

int mrt_debug_wide_histogram(MRTScene scene, uint32_t *out12) {
    MRT_TRY
    REQUIRE(scene && out12, "mrt_debug_wide_histogram: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_wide_histogram: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::wide_histogram(scene->dev, scene->ctx->stream, out12);
    MRT_CATCH
}
// the 8-wide nodes of a committed scene as they lie in device memory (tests: two builds of one scene must agree bit for bit)
int mrt_debug_read_wnodes(MRTScene scene, void *out, size_t nbytes, uint64_t *num_nodes) {
    MRT_TRY
    REQUIRE(scene && num_nodes, "mrt_debug_read_wnodes: bad argument");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_read_wnodes: scene not committed"); return MRT_ERR_STATE; }
    *num_nodes = scene->dev.num_wnodes;
    const size_t have = (size_t)scene->dev.num_wnodes * mrt::WNODE_STRIDE * 16;
    if (out == nullptr) return MRT_OK;
    REQUIRE(nbytes == have, "mrt_debug_read_wnodes: nbytes must be num_nodes x 16 x the node stride (80 bytes per node)");
    int rc = bind_device(scene->ctx); if (rc) return rc;
    MRT_HIP(hipMemcpy(out, scene->dev.wnodes.p, have, hipMemcpyDeviceToHost));
    return MRT_OK;
    MRT_CATCH
}
// one array of the committed layouts as it lies in device memory (tests/bvh_audit.py decodes and checks every box of the 8-wide layout, tests/rope_audit.py every node of the rope layout)
int mrt_debug_read_layout(MRTScene scene, int32_t part, void *out, size_t nbytes, uint64_t *count) {
    MRT_TRY
    REQUIRE(scene && count, "mrt_debug_read_layout: bad argument");
    REQUIRE(part >= 0 && part <= 9, "mrt_debug_read_layout: part must be 0 .. 9");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_read_layout: scene not committed"); return MRT_ERR_STATE; }
    const mrt::DeviceScene &d = scene->dev;
    const size_t npk = d.wpackets.p ? d.wpackets.n / mrt::WPK : 0, ninst = d.num_inst, nwt = (d.num_inst && d.wtlas_index.p) ? d.wtlas_index.n : 0;
    uint32_t header[8] = {d.num_wnodes, d.num_inst ? d.tlas_wcap : 0u, d.num_inst, (uint32_t)d.wide_depth, (uint32_t)npk, (uint32_t)d.blas_wdepth, (uint32_t)nwt, mrt::WPK};
    const size_t nrope = d.num_inst ? d.rope_nodes : 0, ntl = d.num_inst ? d.tlas_instances : 0;          // the rope TLAS of a two-level scene: its nodes and its index array
    // the rope layout the traversal of traverse.h / traverse_instanced.h walks: the flattened scene's own (none when it was released: wide layout with rope = 0, the empty scene), or the BLASes' in bnodes
    size_t rnodes = 0, rpackets = 0; const float4 *rn = nullptr, *rp = nullptr;
    if (d.num_inst) {
        for (const mrt::BlasRange &r : d.blas_ranges) rpackets += r.ntri;
        rnodes = d.bpackets_offset / 4;
        if (d.bnodes.p) { rn = d.bnodes.p; rp = d.bnodes.p + d.bpackets_offset; } else { rnodes = 0; rpackets = 0; }
        if (4 * rnodes + 3 * rpackets > d.bnodes.n) { mrt::set_error("mrt_debug_read_layout: the BLAS ranges exceed bnodes"); return MRT_ERR_STATE; }
    } else if (d.nodes.p && d.rope_nodes) {
        rnodes = d.rope_nodes; rpackets = d.num_packets; rn = d.nodes.p; rp = d.nodes.p + d.packets_offset;
        if (d.packets_offset < 4 * rnodes || d.packets_offset + 3 * rpackets > d.nodes.n) { mrt::set_error("mrt_debug_read_layout: the rope layout exceeds its allocation"); return MRT_ERR_STATE; }
    }
    const size_t elem[10] = {16 * (size_t)mrt::WNODE_STRIDE, 16 * (size_t)mrt::WPK, sizeof(mrt::InstanceDev), 64, 4, 4, 64, 4, 64, 48};
    const size_t n[10] = {d.num_wnodes, npk, ninst, ninst, nwt, 8, nrope, ntl, rnodes, rpackets};
    const void *src[10] = {d.wnodes.p, d.wpackets.p, d.inst.p, d.inst_box.p, d.wtlas_index.p, header, d.nodes.p, d.tlas_index.p, rn, rp};
    *count = n[part];
    if (out == nullptr) return MRT_OK;
    REQUIRE(nbytes == n[part] * elem[part], "mrt_debug_read_layout: nbytes must be count x the element size of the part");
    if (n[part] == 0) return MRT_OK;
    if (part == 5) { memcpy(out, header, sizeof(header)); return MRT_OK; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    MRT_HIP(hipMemcpy(out, src[part], nbytes, hipMemcpyDeviceToHost));
    return MRT_OK;
    MRT_CATCH
}
// host wall time of the last commit of a flattened scene by phase (ms): staging, device allocations, topology, 8-wide emit, rope emit, validation
int mrt_debug_scene_refits(MRTScene scene, uint32_t *out) {
    REQUIRE(scene && out, "mrt_debug_scene_refits: bad argument");
    *out = scene->dev.refits;
    return MRT_OK;
}
int mrt_debug_commit_times(MRTScene scene, double *out6) {
    REQUIRE(scene && out6, "mrt_debug_commit_times: bad argument");
    for (int k = 0; k < 6; k++) out6[k] = scene->dev.commit_ms[k];
    return MRT_OK;
}
// the commit-time validator on demand, and a way for its test to break one word of one 8-wide node (tests/test_instancing.py)
int mrt_debug_validate(MRTScene scene) {
    MRT_TRY
    REQUIRE(scene, "mrt_debug_validate: scene is NULL");
    if (!scene->changes.committed()) { mrt::set_error("mrt_debug_validate: scene not committed"); return MRT_ERR_STATE; }
    int rc = bind_device(scene->ctx); if (rc) return rc;
    return mrt::validate_layout(scene->dev, scene->ctx->stream, false);
    MRT_CATCH
}
int mrt_debug_validate_patched(MRTScene scene, uint32_t node, uint32_t word, uint32_t value) {
    MRT_TRY
    REQUIRE(scene && scene->changes.committed() && node < scene->dev.num_wnodes && word < 4 * mrt::WNODE_STRIDE, "mrt_debug_validate_patched: bad argument");
    int rc = bind_device(scene->ctx); if (rc) return rc;
    mrt::DevBuf<float4> copy; MRT_HIP(copy.alloc(scene->dev.wnodes.n));
    MRT_HIP(hipMemcpy(copy.p, scene->dev.wnodes.p, scene->dev.wnodes.bytes(), hipMemcpyDeviceToDevice));
    MRT_HIP(hipMemcpy(reinterpret_cast<uint32_t *>(copy.p + (size_t)mrt::WNODE_STRIDE * node) + word, &value, 4, hipMemcpyHostToDevice));
    return mrt::validate_layout(scene->dev, scene->ctx->stream, false, copy.p);
    MRT_CATCH
}
#ifdef MRT_DIAGNOSTICS
int mrt_debug_poke_wnode(MRTScene scene, uint32_t node, uint32_t word, uint32_t value, uint32_t *old_value) {
    MRT_TRY
    REQUIRE(scene && scene->changes.committed() && node < scene->dev.num_wnodes && word < 4 * mrt::WNODE_STRIDE, "mrt_debug_poke_wnode: bad argument");
    int rc = bind_device(scene->ctx); if (rc) return rc;
    uint32_t *p = reinterpret_cast<uint32_t *>(scene->dev.wnodes.p + (size_t)mrt::WNODE_STRIDE * node) + word;
    if (old_value) MRT_HIP(hipMemcpy(old_value, p, 4, hipMemcpyDeviceToHost));
    MRT_HIP(hipMemcpy(p, &value, 4, hipMemcpyHostToDevice));
    return MRT_OK;
    MRT_CATCH
}
#endif
// builder = 2's host part on caller boxes (n x {lo.xyz, -} and {hi.xyz, -}): leaf order, left / right of the n - 1 internal nodes, parent of all 2n - 1 (no device needed)
int mrt_debug_host_sah(const float *lo4, const float *hi4, uint32_t n, uint32_t *order, uint32_t *left, uint32_t *right, uint32_t *parent) {
    MRT_TRY
    REQUIRE(lo4 && hi4 && n >= 1 && order && left && right && parent, "mrt_debug_host_sah: bad argument");
    std::vector<uint32_t> o, l, r, p;
    mrt::host_sah_topology(reinterpret_cast<const float4 *>(lo4), reinterpret_cast<const float4 *>(hi4), n, o, l, r, p);
    memcpy(order, o.data(), (size_t)n * 4); memcpy(parent, p.data(), (2 * (size_t)n - 1) * 4);
    if (n > 1) { memcpy(left, l.data(), (size_t)(n - 1) * 4); memcpy(right, r.data(), (size_t)(n - 1) * 4); }
    return MRT_OK;
    MRT_CATCH
}
// TlasBuilder and WideTlasBuilder on caller boxes (no device needed): what mrt_scene_rebuild_tlas_device rests on is checked against them (tests/test_tlas_rebuild_device_cpu.py)
int mrt_debug_tlas_host_build(const float *lo4, const float *hi4, uint32_t n, uint32_t *rope_order, uint32_t *rope_links, uint32_t *wide_order, uint32_t *wide_pos, uint32_t *counts68) {
    MRT_TRY
    REQUIRE(lo4 && hi4 && n >= 1 && n <= 65536 && rope_order && rope_links && wide_order && wide_pos && counts68, "mrt_debug_tlas_host_build: bad argument");
    return mrt::tlas_host_build(lo4, hi4, n, rope_order, rope_links, wide_order, wide_pos, counts68);
    MRT_CATCH
}
// the shared 8-wide encoder and the shared instance arithmetic on caller values (no device needed): what pins them without a GPU (tests/test_wide_encode_cpu.py)
int mrt_debug_wide_encode(const float *child_lo4, const float *child_hi4, uint32_t occupied_mask, uint32_t imask, uint32_t *out_words20) {
    MRT_TRY
    REQUIRE(child_lo4 && child_hi4 && out_words20 && occupied_mask >= 1 && occupied_mask <= 255 && (imask & ~occupied_mask) == 0, "mrt_debug_wide_encode: bad argument");
    mrt::wide_encode_host(child_lo4, child_hi4, occupied_mask, imask, out_words20);
    return MRT_OK;
    MRT_CATCH
}
int mrt_debug_instance_box(const float *xf16, const float *obj_lo3, const float *obj_hi3, float *rows12, float *world_box6) {
    MRT_TRY
    REQUIRE(xf16 && obj_lo3 && obj_hi3 && rows12 && world_box6, "mrt_debug_instance_box: bad argument");
    if (!mrt::instance_box_host(xf16, obj_lo3, obj_hi3, rows12, world_box6)) { mrt::set_error("mrt_debug_instance_box: the matrix is not invertible"); return MRT_ERR_INVALID_ARGUMENT; }
    return MRT_OK;
    MRT_CATCH
}
int mrt_debug_layout_limits(uint64_t triangles, uint64_t nodes) {
    MRT_TRY
    return mrt::layout_limits(triangles, nodes);
    MRT_CATCH
}
int mrt_debug_segment_sizing(uint32_t capacity, int32_t batch, uint64_t *out4) {
    MRT_TRY
    if (!out4 || batch < 1 || batch > mrt::MAX_FRAME_BATCH) { mrt::set_error("mrt_debug_segment_sizing: NULL output or batch outside 1 .. MAX_FRAME_BATCH"); return MRT_ERR_INVALID_ARGUMENT; }
    const mrt::SegmentSizing z = mrt::segment_sizing(capacity, batch);
    out4[0] = z.blocks; out4[1] = z.per_block; out4[2] = z.seg_cap; out4[3] = mrt::queue_entries(capacity, batch);
    return MRT_OK;
    MRT_CATCH
}
int mrt_debug_calibrate(MRTContext ctx, size_t table_bytes, double *out3) {
    MRT_TRY
    REQUIRE(ctx && out3 && table_bytes >= 4096 && table_bytes <= ((size_t)1 << 34), "mrt_debug_calibrate: bad argument");
    int rc = bind_device(ctx); if (rc) return rc;
    return mrt::calibrate(ctx->stream, table_bytes, out3);
    MRT_CATCH
}

}  // extern "C"
