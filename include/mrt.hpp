// mrt.hpp — C++17 host-side mirror of the reference's Swift classes over the C ABI (mrt_abi.h).
//
// The reference's host side is Swift (Scene.swift, DragonScene.swift, Model.swift, Mesh.swift,
// SubMesh.swift, Renderer.swift); no Swift toolchain exists in this environment, so the host layer above
// the C ABI is C++ (header only), with the same type names, initialiser arguments and properties:
//
//   Swift                                               here
//   Model(name:position:rotation:scale:on:)             mrt::Model(name, position, rotation, scale)
//   Mesh.transform / .submeshes                         mrt::Mesh::transform / submeshes
//   Submesh.material                                    mrt::Submesh::material
//   Scene.models / .camera / .lights                    mrt::Scene::models / camera / lights
//   Light.areaLight/sunLight/pointLight/spotLight       mrt::Light::areaLight/...
//   DragonScene(size:device:)                           mrt::DragonScene(width, height)
//   Renderer(metalView:) / draw(in:) / frameIndex       mrt::Renderer(width, height, scene) / draw() / frameIndex()
//
// Errors: the Swift code traps (fatalError, try!); here every failing ABI call throws mrt::Error.
#pragma once
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "mrt_abi.h"

namespace mrt {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error("mrt error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc) { if (rc != MRT_OK) throw Error(rc, mrt_last_error()); }

using Camera = MRTCamera;
using Material = MRTMaterial;

inline MRTFloat3 f3(float x, float y, float z) { return MRTFloat3{x, y, z, 0.0f}; }

struct Light : MRTLight {                                            // Scene.swift:70-107
    Light() { std::memset(static_cast<MRTLight *>(this), 0, sizeof(MRTLight)); }
    static Light areaLight(MRTFloat3 position, MRTFloat3 forward, MRTFloat3 right, MRTFloat3 up, MRTFloat3 color) {
        Light l; l.type = MRTLightTypeAreaLight; l.position = position; l.forward = forward; l.right = right; l.up = up; l.color = color; return l;
    }
    static Light sunLight(MRTFloat3 direction, MRTFloat3 color) { Light l; l.type = MRTLightTypeSunlight; l.direction = direction; l.color = color; return l; }
    static Light pointLight(MRTFloat3 position, MRTFloat3 color) { Light l; l.type = MRTLightTypePointlight; l.position = position; l.color = color; return l; }
    static Light spotLight(MRTFloat3 position, MRTFloat3 direction, float coneAngle, MRTFloat3 color) {
        Light l; l.type = MRTLightTypeSpotlight; l.position = position; l.direction = direction; l.coneAngle = coneAngle; l.color = color; return l;
    }
};

struct Submesh {                                                     // SubMesh.swift:10-33
    std::string name;
    std::vector<uint32_t> indices;                                   // 3 per triangle
    Material material{};
    size_t triangleCount() const { return indices.size() / 3; }
};

struct Mesh {                                                        // Mesh.swift:10-49
    std::vector<float> positions, normals;                           // packed xyz
    float transform[16];                                             // column-major T*R*S (Mesh.swift:24)
    std::vector<Submesh> submeshes;
};

// Directory searched for Resources/<name>.obj (Bundle.main in the reference, Model.swift:14)
inline std::string &resourceDirectory() { static std::string d = "assets/Resources"; return d; }

struct Model {                                                       // Model.swift:10-40
    std::string name;
    std::vector<Mesh> meshes;
    bool proxy = false;                                              // dragon / bunny stand-ins (absent upstream)
    Model(const std::string &name_, const float position[3], const float rotation[3], float scale) : name(name_) {
        MRTMeshData md = nullptr;
        std::string path = resourceDirectory() + "/" + name + ".obj";
        int rc = mrt_obj_load(path.c_str(), &md);
        if (rc == MRT_ERR_IO && name == "dragon") { check(mrt_dragon_proxy(&md)); proxy = true; }
        else if (rc == MRT_ERR_IO && name == "bunny") { check(mrt_bunny_proxy(&md)); proxy = true; }
        else check(rc);
        Mesh m;
        size_t nv = 0; int32_t ns = 0;
        check(mrt_meshdata_counts(md, &nv, &ns));
        m.positions.resize(nv * 3); m.normals.resize(nv * 3);
        check(mrt_meshdata_vertices(md, m.positions.data(), m.normals.data()));
        for (int32_t s = 0; s < ns; s++) {
            Submesh sm; size_t nt = 0; char buf[256];
            check(mrt_meshdata_submesh(md, s, &nt, nullptr, nullptr, nullptr, 0));
            sm.indices.resize(nt * 3);
            check(mrt_meshdata_submesh(md, s, &nt, sm.indices.data(), &sm.material, buf, sizeof buf));
            sm.name = buf;
            m.submeshes.push_back(std::move(sm));
        }
        mrt_meshdata_free(md);
        check(mrt_make_transform(position, rotation, scale, m.transform));
        meshes.push_back(std::move(m));
    }
    Model(const std::string &name_, std::initializer_list<float> position, float scale)
        : Model(name_, std::vector<float>(position).data(), std::vector<float>{0, 0, 0}.data(), scale) {}
    Model(const std::string &name_, std::initializer_list<float> position, std::initializer_list<float> rotation, float scale)
        : Model(name_, std::vector<float>(position).data(), std::vector<float>(rotation).data(), scale) {}
};

struct Scene {                                                       // Scene.swift:10-67
    std::vector<Model> models;
    Camera camera;
    std::vector<Light> lights;
    Scene(int width, int height) {
        camera = setupCamera(width, height);
        Light light1 = setupLight();
        Light light3 = Light::spotLight(f3(2, 1, 4), f3(-1.5f, -0.5f, -1.5f), 25.0f / 180.0f * 3.14159274f, f3(4, 4, 4));
        lights = {light1, light3};                                   // Scene.swift:30
    }
    virtual ~Scene() = default;
    // Stream-ordered queries of a committed MRTScene on device buffers (mrt_scene_intersect_closest_device / _any_device): n x MRTRay in, n x MRTIntersection or
    // n x int32 out, all in device memory; hipStream is a hipStream_t taken literally (nullptr = HIP's null stream; Renderer::stream() is the context's).
    // Nothing is allocated, copied or synchronised; keep the buffers alive until the stream has passed the call.
    static void intersectClosestDevice(MRTScene committed, const void *deviceRays, size_t n, void *deviceOut, void *hipStream) { check(mrt_scene_intersect_closest_device(committed, deviceRays, n, deviceOut, hipStream)); }
    static void intersectAnyDevice(MRTScene committed, const void *deviceRays, size_t n, void *deviceOccluded, void *hipStream) { check(mrt_scene_intersect_any_device(committed, deviceRays, n, deviceOccluded, hipStream)); }
    // All hits in order (mrt_scene_intersect_all_device): per ray the maxHits (1 .. MRT_MAX_HITS) smallest hits under (distance, triangle id), ascending, each triangle once ->
    // n x maxHits x MRTIntersection (16-byte aligned; misses pad a row) and n x int32 counts.  Flattened scenes; truncation is not reported (ask for one more).
    static void intersectAllDevice(MRTScene committed, const void *deviceRays, size_t n, int32_t maxHits, void *deviceOut, void *deviceHitCounts, void *hipStream) {
        check(mrt_scene_intersect_all_device(committed, deviceRays, n, maxHits, deviceOut, deviceHitCounts, hipStream));
    }
    static void intersectAllDeviceCounted(MRTScene committed, const void *deviceRays, size_t n, int32_t maxHits, void *deviceOut, void *deviceHitCounts, void *hipStream, const void *deviceCount) {
        check(mrt_scene_intersect_all_device_counted(committed, deviceRays, n, maxHits, deviceOut, deviceHitCounts, hipStream, deviceCount));
    }
    // Visibility masks (mrt_scene_set_mesh_masks; the reference's ShaderTypes.h:23-30): one 32-bit mask per mesh id, 0xFFFFFFFF until set; a ray with mask r sees mesh m iff
    // masks[m] & r.  Takes effect at once, commit or not; no build, refit or commit follows.  Draws ignore masks: the masked queries below honour them.
    static void setMeshMasks(MRTScene scene, int32_t firstMeshId, const std::vector<uint32_t> &masks) { check(mrt_scene_set_mesh_masks(scene, firstMeshId, (int32_t)masks.size(), masks.data())); }
    static std::vector<uint32_t> meshMasks(MRTScene scene, int32_t firstMeshId, int32_t count) {
        std::vector<uint32_t> m((size_t)count); check(mrt_scene_get_mesh_masks(scene, firstMeshId, count, m.data())); return m;
    }
    // The three queries above for rays that may not see everything: deviceRayMasks is nullptr (rayMask holds for every ray) or n x uint32 on the device (rayMask is ignored);
    // deviceCount is nullptr or the row count on the device.  One launch, one ray per lane; the records are those of a scene holding the visible meshes only.
    static void intersectClosestMaskedDevice(MRTScene committed, const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, void *deviceOut, void *hipStream, const void *deviceCount = nullptr) {
        check(mrt_scene_intersect_closest_masked_device(committed, deviceRays, deviceRayMasks, rayMask, n, deviceOut, hipStream, deviceCount));
    }
    static void intersectAnyMaskedDevice(MRTScene committed, const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, void *deviceOccluded, void *hipStream, const void *deviceCount = nullptr) {
        check(mrt_scene_intersect_any_masked_device(committed, deviceRays, deviceRayMasks, rayMask, n, deviceOccluded, hipStream, deviceCount));
    }
    static void intersectAllMaskedDevice(MRTScene committed, const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, int32_t maxHits, void *deviceOut, void *deviceHitCounts,
                                         void *hipStream, const void *deviceCount = nullptr) {
        check(mrt_scene_intersect_all_masked_device(committed, deviceRays, deviceRayMasks, rayMask, n, maxHits, deviceOut, deviceHitCounts, hipStream, deviceCount));
    }
    // Stream-ordered deformation of a committed flattened MRTScene (mrt_scene_update_mesh_device / mrt_scene_refit_device): strided float3 positions and normals in device
    // memory replace one mesh's vertices, then the resident tree is refitted, all on hipStream; updatesRejected() blocks and counts the updates refused for a NaN or an infinity.
    static void updateMeshDevice(MRTScene committed, int32_t meshId, const void *devicePositions, size_t positionStrideBytes, const void *deviceNormals, size_t normalStrideBytes, size_t vertexCount, void *hipStream) {
        check(mrt_scene_update_mesh_device(committed, meshId, devicePositions, positionStrideBytes, deviceNormals, normalStrideBytes, vertexCount, hipStream));
    }
    static void refitDevice(MRTScene committed, void *hipStream) { check(mrt_scene_refit_device(committed, hipStream)); }
    static uint64_t deviceUpdatesRejected(MRTScene scene) { uint64_t n = 0; check(mrt_scene_device_updates_rejected(scene, &n)); return n; }
    // Stream-ordered instance moves of a committed two-level MRTScene (mrt_scene_set_instance_transforms_device / mrt_scene_refit_instances_device): column-major float 4x4
    // matrices in device memory for the mesh ids firstMeshId .. + count - 1, then the TLAS boxes refitted (topology kept), all on hipStream
    static void setInstanceTransformsDevice(MRTScene committed, int32_t firstMeshId, size_t count, const void *deviceTransforms, size_t strideBytes, void *hipStream) {
        check(mrt_scene_set_instance_transforms_device(committed, firstMeshId, count, deviceTransforms, strideBytes, hipStream));
    }
    static void refitInstancesDevice(MRTScene committed, void *hipStream) { check(mrt_scene_refit_instances_device(committed, hipStream)); }
    // ... or, when instances have migrated, the topology of both TLAS forms rebuilt on hipStream and then refitted (mrt_scene_rebuild_tlas_device): instead of the refit above
    static void rebuildTlasDevice(MRTScene committed, void *hipStream) { check(mrt_scene_rebuild_tlas_device(committed, hipStream)); }
    // Stream-ordered deformation of a mesh inside a committed two-level MRTScene (mrt_scene_update_blas_device / mrt_scene_refit_blas_device): object-space vertices of a
    // source mesh from device memory, then its BLAS, its instances' boxes and the TLAS refitted on the stream.
    static void updateBlasDevice(MRTScene committed, int32_t meshId, const void *devicePositions, size_t positionStrideBytes, const void *deviceNormals, size_t normalStrideBytes,
                                 size_t vertexCount, void *hipStream) {
        check(mrt_scene_update_blas_device(committed, meshId, devicePositions, positionStrideBytes, deviceNormals, normalStrideBytes, vertexCount, hipStream));
    }
    static void refitBlasDevice(MRTScene committed, void *hipStream) { check(mrt_scene_refit_blas_device(committed, hipStream)); }
    // The step after the query, on device buffers and a stream (mrt_scene_resolve_hits_device / mrt_scene_interpolate_device): n x MRTRay and the n x MRTIntersection the
    // query wrote for them -> n x MRTSurface (position | distance, shading normal | type, base colour | resource slot, ids), read from what the device holds now; and any
    // per-vertex float data of the caller's (channels floats per vertex, numbered as vertexOffsets describes) interpolated at the hits.  The first call after a commit makes
    // a small table; later ones allocate, copy and wait for nothing.
    static void resolveHitsDevice(MRTScene committed, const void *deviceRays, const void *deviceHits, size_t n, void *deviceSurfaces, void *hipStream) {
        check(mrt_scene_resolve_hits_device(committed, deviceRays, deviceHits, n, deviceSurfaces, hipStream));
    }
    static void interpolateDevice(MRTScene committed, const void *deviceHits, size_t n, const void *deviceAttributes, size_t attributeStrideBytes, int32_t channels,
                                  void *deviceOut, size_t outStrideBytes, void *hipStream) {
        check(mrt_scene_interpolate_device(committed, deviceHits, n, deviceAttributes, attributeStrideBytes, channels, deviceOut, outStrideBytes, hipStream));
    }
    // What follows a surface in the reference's kernel, its diffuse path (mrt_scene_scatter_device; the materials extension is scatterMaterialsDevice): n x MRTSurface
    // and the n x int32 Halton indices of Renderer::primaryRaysDevice -> n x MRTRay shadow rays, n x 4 float light rows {colour | 1.0f where the shadow ray is wanted},
    // n x MRTRay bounce rays (deviceNextRays may be nullptr: the last bounce).  Row i in, row i out; zeros for a row that is no surface.  bounce 0 .. 18; lightCount 0 = all.
    static void scatterDevice(MRTScene committed, const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t lightCount, void *deviceShadowRays,
                              void *deviceLight, void *deviceNextRays, void *hipStream) {
        check(mrt_scene_scatter_device(committed, deviceSurfaces, deviceHaltonIndex, n, bounce, lightCount, deviceShadowRays, deviceLight, deviceNextRays, hipStream));
    }
    // The same step with the materials extension on (mrt_scene_scatter_materials_device): also takes the n x MRTRay that hit the surfaces and the integrator's maxBounces
    // (1 .. 16; 0 <= bounce < maxBounces), also writes n x MRTScatterLobe {weight | lobe, emission | 0}: lobe 0 none, 1 diffuse, 2 / 3 interface reflected / refracted,
    // 4 specular, 5 absorbed.  Diffuse rows as scatterDevice; the other lobes get zero shadow and light rows and continue along their own ray.
    static void scatterMaterialsDevice(MRTScene committed, const void *deviceRays, const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t maxBounces,
                                       int32_t lightCount, void *deviceShadowRays, void *deviceLight, void *deviceNextRays, void *deviceLobes, void *hipStream) {
        check(mrt_scene_scatter_materials_device(committed, deviceRays, deviceSurfaces, deviceHaltonIndex, n, bounce, maxBounces, lightCount, deviceShadowRays, deviceLight, deviceNextRays,
                                                 deviceLobes, hipStream));
    }
    // Row queues between the stages (mrt_context_compact_rows_device and the *_device_counted twins of the six entries above): the rows of up to eight columns whose keep
    // byte is not 0 moved to the front of the columns' destinations in their order, and their number left in *deviceCountOut, a uint32 ON THE DEVICE; the counted forms
    // then take n as the capacity and handle the rows below min(n, *deviceCount), touching no other.  No host read, no allocation, no wait; the workspace
    // (compactWorkspaceBytes(n) bytes, 16-byte aligned) is the caller's.  deviceCountIn may be nullptr (all n rows); `columns` is a host array of device pointers.
    static size_t compactWorkspaceBytes(size_t n) { return mrt_compact_workspace_bytes(n); }
    static void compactRowsDevice(MRTContext ctx, const void *deviceKeep, size_t n, const void *deviceCountIn, const MRTRowColumn *columns, int32_t columnCount, void *deviceCountOut,
                                  void *deviceWorkspace, size_t workspaceBytes, void *hipStream) {
        check(mrt_context_compact_rows_device(ctx, deviceKeep, n, deviceCountIn, columns, columnCount, deviceCountOut, deviceWorkspace, workspaceBytes, hipStream));
    }
    static void intersectClosestDeviceCounted(MRTScene committed, const void *deviceRays, size_t n, void *deviceOut, void *hipStream, const void *deviceCount) {
        check(mrt_scene_intersect_closest_device_counted(committed, deviceRays, n, deviceOut, hipStream, deviceCount));
    }
    static void intersectAnyDeviceCounted(MRTScene committed, const void *deviceRays, size_t n, void *deviceOccluded, void *hipStream, const void *deviceCount) {
        check(mrt_scene_intersect_any_device_counted(committed, deviceRays, n, deviceOccluded, hipStream, deviceCount));
    }
    static void resolveHitsDeviceCounted(MRTScene committed, const void *deviceRays, const void *deviceHits, size_t n, void *deviceSurfaces, void *hipStream, const void *deviceCount) {
        check(mrt_scene_resolve_hits_device_counted(committed, deviceRays, deviceHits, n, deviceSurfaces, hipStream, deviceCount));
    }
    static void interpolateDeviceCounted(MRTScene committed, const void *deviceHits, size_t n, const void *deviceAttributes, size_t attributeStrideBytes, int32_t channels, void *deviceOut,
                                         size_t outStrideBytes, void *hipStream, const void *deviceCount) {
        check(mrt_scene_interpolate_device_counted(committed, deviceHits, n, deviceAttributes, attributeStrideBytes, channels, deviceOut, outStrideBytes, hipStream, deviceCount));
    }
    static void scatterDeviceCounted(MRTScene committed, const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t lightCount, void *deviceShadowRays,
                                     void *deviceLight, void *deviceNextRays, void *hipStream, const void *deviceCount) {
        check(mrt_scene_scatter_device_counted(committed, deviceSurfaces, deviceHaltonIndex, n, bounce, lightCount, deviceShadowRays, deviceLight, deviceNextRays, hipStream, deviceCount));
    }
    static void scatterMaterialsDeviceCounted(MRTScene committed, const void *deviceRays, const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t maxBounces,
                                              int32_t lightCount, void *deviceShadowRays, void *deviceLight, void *deviceNextRays, void *deviceLobes, void *hipStream, const void *deviceCount) {
        check(mrt_scene_scatter_materials_device_counted(committed, deviceRays, deviceSurfaces, deviceHaltonIndex, n, bounce, maxBounces, lightCount, deviceShadowRays, deviceLight,
                                                         deviceNextRays, deviceLobes, hipStream, deviceCount));
    }
    // The integrator's path state between the stages (mrt_context_*_paths_device, _deposit_light_device, _fold_sample_device): one kernel each on
    // hipStream, no allocation, copy or wait.  deviceCount may be nullptr (all n rows); a pixel occurs at most once among the rows of a call.  advancePathsDevice takes
    // exactly one of deviceSurfaces (the diffuse form) and deviceLobes (the materials form, which needs devicePixel and deviceRadiance); deviceKeepPath may be nullptr.
    static void resetPathsDevice(MRTContext ctx, size_t n, void *deviceThroughput, void *devicePixel, void *deviceRadiance, size_t pixelCount, void *hipStream) {
        check(mrt_context_reset_paths_device(ctx, n, deviceThroughput, devicePixel, deviceRadiance, pixelCount, hipStream));
    }
    static void advancePathsDevice(MRTContext ctx, size_t n, const void *deviceCount, const void *deviceSurfaces, const void *deviceLobes, const void *deviceLight, void *deviceThroughput,
                                   const void *devicePixel, void *deviceRadiance, size_t pixelCount, void *deviceKeepShadow, void *deviceKeepPath, void *hipStream) {
        check(mrt_context_advance_paths_device(ctx, n, deviceCount, deviceSurfaces, deviceLobes, deviceLight, deviceThroughput, devicePixel, deviceRadiance, pixelCount, deviceKeepShadow,
                                               deviceKeepPath, hipStream));
    }
    static void depositLightDevice(MRTContext ctx, size_t n, const void *deviceCount, const void *deviceOccluded, const void *deviceLight, const void *deviceThroughput,
                                   const void *devicePixel, void *deviceRadiance, size_t pixelCount, void *hipStream) {
        check(mrt_context_deposit_light_device(ctx, n, deviceCount, deviceOccluded, deviceLight, deviceThroughput, devicePixel, deviceRadiance, pixelCount, hipStream));
    }
    static void foldSampleDevice(MRTContext ctx, size_t pixelCount, void *deviceSample, void *deviceAccum, uint32_t frameIndex, bool clearSample, void *hipStream) {
        check(mrt_context_fold_sample_device(ctx, pixelCount, deviceSample, deviceAccum, frameIndex, clearSample ? 1 : 0, hipStream));
    }
    // From a composed frame to an image a host can show (mrt_context_fold_guides_device, _denoise_device, _tonemap_device): the guide buffers folded from
    // the frame's bounce-0 MRTSurface rows (frameIndex 0 replaces them), Renderer::denoise's filter of any device image (params nullptr = the defaults; the workspace of
    // denoiseWorkspaceBytes(width, height) bytes is the caller's) and the tonemap into width x height RGBA8, top row first.  On hipStream; no allocation, copy or wait.
    static void foldGuidesDevice(MRTContext ctx, size_t pixelCount, const void *deviceSurfaces, void *deviceNormalDepth, void *deviceAlbedo, void *deviceIds, uint32_t frameIndex,
                                 void *hipStream) {
        check(mrt_context_fold_guides_device(ctx, pixelCount, deviceSurfaces, deviceNormalDepth, deviceAlbedo, deviceIds, frameIndex, hipStream));
    }
    static size_t denoiseWorkspaceBytes(int width, int height) { size_t n = 0; check(mrt_denoise_workspace_bytes(width, height, &n)); return n; }
    static void denoiseDevice(MRTContext ctx, int width, int height, const void *deviceImage, const void *deviceNormalDepth, const void *deviceAlbedo, void *deviceWorkspace,
                              size_t workspaceBytes, void *deviceOut, const MRTDenoiseParams *params, void *hipStream) {
        check(mrt_context_denoise_device(ctx, width, height, deviceImage, deviceNormalDepth, deviceAlbedo, deviceWorkspace, workspaceBytes, deviceOut, params, hipStream));
    }
    static void tonemapDevice(MRTContext ctx, int width, int height, const void *deviceImage, void *deviceRgba8, void *hipStream) {
        check(mrt_context_tonemap_device(ctx, width, height, deviceImage, deviceRgba8, hipStream));
    }
    // Temporal reprojection of the accumulated image (mrt_context_reproject_device): foldSampleDevice's running average kept up while the camera or an
    // instance moves.  This frame's bounce-0 MRTSurface rows and radiance sample, the PREVIOUS frame's own guide entries (foldGuidesDevice with frameIndex 0) and history
    // {rgb, length} -> deviceOut {rgb, length}, the next frame's history.  devicePrevPosition (where each visible point was a frame ago) may be nullptr: the geometry
    // did not move.  params nullptr = the defaults.  deviceOut overlaps no input.  One kernel on hipStream; no allocation, copy or wait.
    static void reprojectDevice(MRTContext ctx, int width, int height, const Camera &camera, const Camera &prevCamera, const void *deviceSurfaces, const void *devicePrevPosition,
                                const void *devicePrevNormalDepth, const void *devicePrevIds, const void *devicePrevHistory, const void *deviceSample, void *deviceOut,
                                const MRTReprojectParams *params, void *hipStream) {
        check(mrt_context_reproject_device(ctx, width, height, &camera, &prevCamera, deviceSurfaces, devicePrevPosition, devicePrevNormalDepth, devicePrevIds, devicePrevHistory,
                                           deviceSample, deviceOut, params, hipStream));
    }
    // The variance-guided a-trous filter and the sample image of its moments (mrt_context_moments_sample_device / _denoise_variance_device).
    // momentsSampleDevice writes {l, l * l, 0, 0} of a sample; a second reprojectDevice call of the frame with that image as deviceSample and its own previous output as
    // devicePrevHistory accumulates it into deviceMoments {m1, m2, ., length}.  denoiseVarianceDevice filters deviceImage (the colour's reprojectDevice output) with a
    // colour term in standard deviations (params->sigma_color; nullptr = the defaults); workspace and deviceOut as denoiseDevice.  On hipStream; no allocation, copy or wait.
    static void momentsSampleDevice(MRTContext ctx, int width, int height, const void *deviceSample, const void *deviceAlbedo, bool demodulate, void *deviceOut, void *hipStream) {
        check(mrt_context_moments_sample_device(ctx, width, height, deviceSample, deviceAlbedo, demodulate ? 1 : 0, deviceOut, hipStream));
    }
    static void denoiseVarianceDevice(MRTContext ctx, int width, int height, const void *deviceImage, const void *deviceMoments, const void *deviceNormalDepth, const void *deviceAlbedo,
                                      void *deviceWorkspace, size_t workspaceBytes, void *deviceOut, const MRTDenoiseParams *params, void *hipStream) {
        check(mrt_context_denoise_variance_device(ctx, width, height, deviceImage, deviceMoments, deviceNormalDepth, deviceAlbedo, deviceWorkspace, workspaceBytes, deviceOut, params,
                                                  hipStream));
    }
    // each mesh's first attribute row (an instance reports its source's) and, last, the number of rows: meshCount + 1 entries
    static std::vector<uint64_t> vertexOffsets(MRTScene scene, size_t meshCount) {
        std::vector<uint64_t> o(meshCount + 1); check(mrt_scene_vertex_offsets(scene, o.data(), o.size())); return o;
    }
    void updateUniforms(int width, int height) { camera = setupCamera(width, height); }   // Scene.swift:36-38
    static Camera setupCamera(int width, int height) { Camera c; check(mrt_default_camera(width, height, &c)); return c; }   // :40-57
    static Light setupLight() {                                      // :59-67
        return Light::areaLight(f3(0.0f, 1.98f, 0.0f), f3(0.0f, -1.0f, 0.0f), f3(0.25f, 0.0f, 0.0f), f3(0.0f, 0.0f, 0.25f), f3(4.0f, 4.0f, 4.0f));
    }
};

struct DragonScene : Scene {                                         // DragonScene.swift:10-34
    DragonScene(int width, int height) : Scene(width, height) {
        const float pi = 3.14159274f;
        models.emplace_back("train", std::initializer_list<float>{-0.3f, 0, 0.4f}, 0.5f);
        models.emplace_back("dragon", std::initializer_list<float>{0.3f, 0.38f, 2.5f}, std::initializer_list<float>{0, pi / 2 * 1.2f, 0}, 1.2f);
        models.emplace_back("treefir", std::initializer_list<float>{0.5f, 0, -0.2f}, 0.7f);
        models.emplace_back("plane", std::initializer_list<float>{0, 0, 0}, 10.0f);
        models.emplace_back("sphere", std::initializer_list<float>{-1.9f, 0.0f, 0.3f}, 1.0f);
        models.emplace_back("sphere", std::initializer_list<float>{2.9f, 0.0f, -0.5f}, 2.0f);
        models.emplace_back("plane-back", std::initializer_list<float>{0, 0, -1.5f}, 10.0f);
    }
};

// createBuffers / geometry descriptors (Renderer.swift:107-182, Mesh.swift:39-48): hand a Scene's models and lights to an MRTScene.
// instancing: models loaded from the same resource become instances of one mesh (mrt_scene_add_instance), committed two-level.
inline void uploadScene(MRTScene dst, const Scene &scene, bool instancing = false) {
    if (instancing) check(mrt_scene_set_option(dst, "instancing", 1));
    std::vector<std::pair<std::string, int32_t>> loaded;             // resource name -> mesh id of its first use
    for (const Model &model : scene.models)
        for (const Mesh &mesh : model.meshes) {
            int32_t id = -1, source = -1;
            if (instancing && model.meshes.size() == 1) for (auto &l : loaded) if (l.first == model.name) source = l.second;
            if (source >= 0) { check(mrt_scene_add_instance(dst, source, mesh.transform, &id)); continue; }
            check(mrt_scene_add_mesh(dst, mesh.positions.data(), 12, mesh.normals.data(), 12, mesh.positions.size() / 3, mesh.transform, &id));
            for (const Submesh &sm : mesh.submeshes) check(mrt_mesh_add_submesh(dst, id, sm.indices.data(), sm.triangleCount(), &sm.material, nullptr));
            loaded.emplace_back(model.name, id);
        }
    check(mrt_scene_set_lights(dst, scene.lights.data(), (int32_t)scene.lights.size()));
}

class Renderer {                                                     // Renderer.swift:12-357
  public:
    static constexpr int maxFramesInFlight = 3;                      // Renderer.swift:33 (here: setOption("frames_in_flight", n); library default: the same three, each a pass of up to 8 frames)
    // instancing = true: models loaded from the same resource become instances of one mesh (mrt_scene_add_instance) and the scene is committed
    // two-level — one BLAS per distinct mesh + a TLAS (the reference's instance acceleration structure, Renderer.swift:193-213)
    Renderer(int width, int height, const Scene &scene, int device = 0, uint32_t seed = 1, int max_bounces = 3, bool instancing = false) : w_(width), h_(height) {
        check(mrt_context_create(device, &ctx_));                    // MTLCreateSystemDefaultDevice + queue (:46-59)
        try {
            check(mrt_scene_create(ctx_, &scene_));
            uploadScene(scene_, scene, instancing);                  // createBuffers / geometry descriptors (:107-182, Mesh.swift:39-48)
            check(mrt_scene_commit(scene_));                         // createAccelerationStructures (:184-214)
            check(mrt_renderer_create(ctx_, scene_, width, height, seed, max_bounces, &r_));
            check(mrt_renderer_set_camera(r_, &scene.camera));
        } catch (...) { destroy(); throw; }
    }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;
    ~Renderer() { destroy(); }
    void draw(int frames = 1) { check(mrt_renderer_render(r_, frames)); }                   // draw(in:) (:284-351)
    void wait() { check(mrt_renderer_wait(r_)); }
    uint64_t framesCompleted() const { uint64_t f = 0; check(mrt_renderer_frames_completed(r_, &f)); return f; }   // the completion handler of :285-287 as a poll; never blocks
    // updateUniforms (:216-229): size, frameIndex, lightCount and camera as the one 96-byte block the reference binds at buffer index 0
    MRTUniforms uniforms() const { MRTUniforms u; check(mrt_renderer_get_uniforms(r_, &u)); return u; }
    void setUniforms(const MRTUniforms &u) { check(mrt_renderer_set_uniforms(r_, &u)); w_ = u.width; h_ = u.height; }
    void drawableSizeWillChange(int width, int height) { w_ = width; h_ = height; check(mrt_renderer_resize(r_, width, height)); }   // :353-356
    uint32_t frameIndex() const { uint32_t f = 0; check(mrt_renderer_frame_index(r_, &f)); return f; }
    void setFrameIndex(uint32_t f) { check(mrt_renderer_set_frame_index(r_, f)); }
    // animated transforms: new object->world matrix (column-major 4x4) for one mesh / instance, then commit(); a two-level scene rebuilds only its TLAS
    void setInstanceTransform(int32_t meshId, const float transform[16]) { check(mrt_scene_set_instance_transform(scene_, meshId, transform)); }
    /// deforming geometry: new object-space positions / normals (packed xyz) of one mesh's vertices, same count; commit() then refits the tree of a flattened scene
    void updateMesh(int32_t meshId, const float *positions, const float *normals, size_t vertexCount) { check(mrt_scene_update_mesh(scene_, meshId, positions, 12, normals, 12, vertexCount)); }
    // the checked form: one normal per vertex, or std::invalid_argument before anything is read
    void updateMesh(int32_t meshId, const std::vector<float> &positions, const std::vector<float> &normals) {
        if (positions.size() % 3 != 0 || normals.size() != positions.size()) throw std::invalid_argument("updateMesh: positions and normals must hold 3 floats per vertex, the same number of vertices");
        updateMesh(meshId, positions.data(), normals.data(), positions.size() / 3);
    }
    void commit() { check(mrt_scene_commit(scene_)); }
    // the committed scene's stream-ordered queries on device buffers (Scene::intersectClosestDevice) and the context's stream to order them with the draws
    MRTScene sceneHandle() const { return scene_; }
    void *stream() const { void *s = nullptr; check(mrt_context_get_stream(ctx_, &s)); return s; }
    void intersectClosestDevice(const void *deviceRays, size_t n, void *deviceOut, void *hipStream) { Scene::intersectClosestDevice(scene_, deviceRays, n, deviceOut, hipStream); }
    void intersectAnyDevice(const void *deviceRays, size_t n, void *deviceOccluded, void *hipStream) { Scene::intersectAnyDevice(scene_, deviceRays, n, deviceOccluded, hipStream); }
    // visibility masks per mesh id and the masked queries (Scene::setMeshMasks / intersectClosestMaskedDevice ...); draw() ignores masks
    void setMeshMasks(int32_t firstMeshId, const std::vector<uint32_t> &masks) { Scene::setMeshMasks(scene_, firstMeshId, masks); }
    std::vector<uint32_t> meshMasks(int32_t firstMeshId, int32_t count) const { return Scene::meshMasks(scene_, firstMeshId, count); }
    void intersectClosestMaskedDevice(const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, void *deviceOut, void *hipStream, const void *deviceCount = nullptr) {
        Scene::intersectClosestMaskedDevice(scene_, deviceRays, deviceRayMasks, rayMask, n, deviceOut, hipStream, deviceCount);
    }
    void intersectAnyMaskedDevice(const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, void *deviceOccluded, void *hipStream, const void *deviceCount = nullptr) {
        Scene::intersectAnyMaskedDevice(scene_, deviceRays, deviceRayMasks, rayMask, n, deviceOccluded, hipStream, deviceCount);
    }
    void intersectAllMaskedDevice(const void *deviceRays, const void *deviceRayMasks, uint32_t rayMask, size_t n, int32_t maxHits, void *deviceOut, void *deviceHitCounts, void *hipStream,
                                  const void *deviceCount = nullptr) {
        Scene::intersectAllMaskedDevice(scene_, deviceRays, deviceRayMasks, rayMask, n, maxHits, deviceOut, deviceHitCounts, hipStream, deviceCount);
    }
    // hit records resolved to surface data, and the caller's per-vertex data interpolated at the hits (Scene::resolveHitsDevice / interpolateDevice / vertexOffsets)
    void resolveHitsDevice(const void *deviceRays, const void *deviceHits, size_t n, void *deviceSurfaces, void *hipStream) { Scene::resolveHitsDevice(scene_, deviceRays, deviceHits, n, deviceSurfaces, hipStream); }
    void interpolateDevice(const void *deviceHits, size_t n, const void *deviceAttributes, size_t attributeStrideBytes, int32_t channels, void *deviceOut, size_t outStrideBytes, void *hipStream) {
        Scene::interpolateDevice(scene_, deviceHits, n, deviceAttributes, attributeStrideBytes, channels, deviceOut, outStrideBytes, hipStream);
    }
    // the path-tracing stages around them (mrt_renderer_primary_rays_device / Scene::scatterDevice): width x height primary rays and Halton indices of this renderer's image at
    // a sample index (pixel y * width + x, row 0 at the bottom; nothing of the renderer's is written), and light, shadow ray and bounce ray of resolved surfaces
    void primaryRaysDevice(uint32_t sampleIndex, void *deviceRays, void *deviceHaltonIndex, void *hipStream) { check(mrt_renderer_primary_rays_device(r_, sampleIndex, deviceRays, deviceHaltonIndex, hipStream)); }
    void scatterDevice(const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t lightCount, void *deviceShadowRays, void *deviceLight, void *deviceNextRays, void *hipStream) {
        Scene::scatterDevice(scene_, deviceSurfaces, deviceHaltonIndex, n, bounce, lightCount, deviceShadowRays, deviceLight, deviceNextRays, hipStream);
    }
    void scatterMaterialsDevice(const void *deviceRays, const void *deviceSurfaces, const void *deviceHaltonIndex, size_t n, int32_t bounce, int32_t maxBounces, int32_t lightCount,
                                void *deviceShadowRays, void *deviceLight, void *deviceNextRays, void *deviceLobes, void *hipStream) {
        Scene::scatterMaterialsDevice(scene_, deviceRays, deviceSurfaces, deviceHaltonIndex, n, bounce, maxBounces, lightCount, deviceShadowRays, deviceLight, deviceNextRays, deviceLobes, hipStream);
    }
    std::vector<uint64_t> vertexOffsets() const { MRTSceneStats st; check(mrt_scene_stats(scene_, &st)); return Scene::vertexOffsets(scene_, (size_t)st.instances); }
    // deformation from device buffers on a stream (Scene::updateMeshDevice): packed or strided float3 rows; refitDevice() after one or more updates
    void updateMeshDevice(int32_t meshId, const void *devicePositions, size_t positionStrideBytes, const void *deviceNormals, size_t normalStrideBytes, size_t vertexCount, void *hipStream) {
        Scene::updateMeshDevice(scene_, meshId, devicePositions, positionStrideBytes, deviceNormals, normalStrideBytes, vertexCount, hipStream);
    }
    void refitDevice(void *hipStream) { Scene::refitDevice(scene_, hipStream); }
    uint64_t deviceUpdatesRejected() const { return Scene::deviceUpdatesRejected(scene_); }
    // implementation knobs (mrt_abi.h): "frames_in_flight" (HIP streams, default 12), "frame_batch" (frames per pass, default 4), ...
    void setOption(const char *key, double value) { check(mrt_renderer_set_option(r_, key, value)); }
    double option(const char *key) const { double v = 0; check(mrt_renderer_get_option(r_, key, &v)); return v; }
    std::vector<float> accumulation() { std::vector<float> a((size_t)w_ * h_ * 4); check(mrt_renderer_read_accum(r_, a.data(), a.size() * 4)); return a; }
    std::vector<uint8_t> tonemapped() { std::vector<uint8_t> a((size_t)w_ * h_ * 4); check(mrt_renderer_read_tonemapped_rgba8(r_, a.data(), a.size())); return a; }
    // first-hit guide buffers and the denoiser (setOption("guides", 1) before drawing; no counterpart in the reference — mrt_abi.h)
    struct Guides { std::vector<float> normalDepth, albedo; std::vector<int32_t> ids; };      // w x h x 4 each, row 0 = bottom
    Guides guides() {
        Guides g; const size_t n = (size_t)w_ * h_ * 4;
        g.normalDepth.resize(n); g.albedo.resize(n); g.ids.resize(n);
        check(mrt_renderer_read_guide(r_, MRT_GUIDE_NORMAL_DEPTH, g.normalDepth.data(), n * 4));
        check(mrt_renderer_read_guide(r_, MRT_GUIDE_ALBEDO, g.albedo.data(), n * 4));
        check(mrt_renderer_read_guide(r_, MRT_GUIDE_IDS, g.ids.data(), n * 4));
        return g;
    }
    std::vector<float> denoise(const MRTDenoiseParams *params = nullptr) {                  // the a-trous filter of the accumulation buffer; nullptr = the defaults
        check(mrt_renderer_denoise(r_, params));
        std::vector<float> a((size_t)w_ * h_ * 4); check(mrt_renderer_read_denoised(r_, a.data(), a.size() * 4)); return a;
    }
    std::vector<uint8_t> denoisedTonemapped() { std::vector<uint8_t> a((size_t)w_ * h_ * 4); check(mrt_renderer_read_denoised_tonemapped_rgba8(r_, a.data(), a.size())); return a; }
    // the same three steps for an image the caller holds on the device, on a stream (Scene::foldGuidesDevice / denoiseDevice / tonemapDevice): images of this renderer's size
    void foldGuidesDevice(const void *deviceSurfaces, void *deviceNormalDepth, void *deviceAlbedo, void *deviceIds, uint32_t frameIndex, void *hipStream) {
        Scene::foldGuidesDevice(ctx_, (size_t)w_ * h_, deviceSurfaces, deviceNormalDepth, deviceAlbedo, deviceIds, frameIndex, hipStream);
    }
    size_t denoiseWorkspaceBytes() const { return Scene::denoiseWorkspaceBytes(w_, h_); }
    void denoiseDevice(const void *deviceImage, const void *deviceNormalDepth, const void *deviceAlbedo, void *deviceWorkspace, size_t workspaceBytes, void *deviceOut,
                       const MRTDenoiseParams *params, void *hipStream) {
        Scene::denoiseDevice(ctx_, w_, h_, deviceImage, deviceNormalDepth, deviceAlbedo, deviceWorkspace, workspaceBytes, deviceOut, params, hipStream);
    }
    void tonemapDevice(const void *deviceImage, void *deviceRgba8, void *hipStream) { Scene::tonemapDevice(ctx_, w_, h_, deviceImage, deviceRgba8, hipStream); }
    // the accumulation carried across a camera or instance move (Scene::reprojectDevice): images of this renderer's size; the cameras are the caller's to keep
    void reprojectDevice(const Camera &camera, const Camera &prevCamera, const void *deviceSurfaces, const void *devicePrevPosition, const void *devicePrevNormalDepth,
                         const void *devicePrevIds, const void *devicePrevHistory, const void *deviceSample, void *deviceOut, const MRTReprojectParams *params, void *hipStream) {
        Scene::reprojectDevice(ctx_, w_, h_, camera, prevCamera, deviceSurfaces, devicePrevPosition, devicePrevNormalDepth, devicePrevIds, devicePrevHistory, deviceSample, deviceOut,
                               params, hipStream);
    }
    // the moments' sample image and the variance-guided filter (Scene::momentsSampleDevice / denoiseVarianceDevice): images of this renderer's size
    void momentsSampleDevice(const void *deviceSample, const void *deviceAlbedo, bool demodulate, void *deviceOut, void *hipStream) {
        Scene::momentsSampleDevice(ctx_, w_, h_, deviceSample, deviceAlbedo, demodulate, deviceOut, hipStream);
    }
    void denoiseVarianceDevice(const void *deviceImage, const void *deviceMoments, const void *deviceNormalDepth, const void *deviceAlbedo, void *deviceWorkspace, size_t workspaceBytes,
                               void *deviceOut, const MRTDenoiseParams *params, void *hipStream) {
        Scene::denoiseVarianceDevice(ctx_, w_, h_, deviceImage, deviceMoments, deviceNormalDepth, deviceAlbedo, deviceWorkspace, workspaceBytes, deviceOut, params, hipStream);
    }
    MRTRenderStats stats() { MRTRenderStats s; check(mrt_renderer_stats(r_, &s)); return s; }
    MRTSceneStats sceneStats() { MRTSceneStats s; check(mrt_scene_stats(scene_, &s)); return s; }
    int width() const { return w_; }
    int height() const { return h_; }

  private:
    void destroy() {
        if (r_) mrt_renderer_destroy(r_);
        if (scene_) mrt_scene_destroy(scene_);
        if (ctx_) mrt_context_destroy(ctx_);
        r_ = nullptr; scene_ = nullptr; ctx_ = nullptr;
    }
    int w_, h_;
    MRTContext ctx_ = nullptr;
    MRTScene scene_ = nullptr;
    MRTRenderer r_ = nullptr;
};

// The same Renderer over the n GPUs of one node (one process): the scene is replicated, the image sharded by 8x8 screen tile
// (tile_id % n == rank), and gather() runs the ONE reduce(sum) per output image (RCCL over xGMI).  The reference creates a single
// MTLDevice (Renderer.swift:46-59); this widens that seam.  The assembled image is bit-identical to Renderer's.
class GroupRenderer {
  public:
    GroupRenderer(int width, int height, const Scene &scene, const std::vector<int> &devices, uint32_t seed = 1, int max_bounces = 3, bool instancing = false) : w_(width), h_(height) {
        check(mrt_group_create(devices.data(), (int32_t)devices.size(), &g_));
        try {
            MRTContext c0 = nullptr; check(mrt_group_context(g_, 0, &c0));
            check(mrt_scene_create(c0, &template_));
            uploadScene(template_, scene, instancing);               // the template is replicated and committed on every device
            check(mrt_group_renderer_create(g_, template_, width, height, seed, max_bounces, &gr_));
            check(mrt_group_set_camera(gr_, &scene.camera));
        } catch (...) { destroy(); throw; }
    }
    GroupRenderer(const GroupRenderer &) = delete;
    GroupRenderer &operator=(const GroupRenderer &) = delete;
    ~GroupRenderer() { destroy(); }
    int size() const { int32_t n = 0; check(mrt_group_size(g_, &n)); return n; }
    void draw(int frames = 1) { check(mrt_group_render(gr_, frames)); }                      // every device; returns at once
    void wait() { check(mrt_group_wait(gr_)); }
    uint64_t framesCompleted() const { uint64_t f = 0; check(mrt_group_frames_completed(gr_, &f)); return f; }
    void setOption(const char *key, double value) { check(mrt_group_set_option(gr_, key, value)); }
    std::vector<float> gather() { std::vector<float> a((size_t)w_ * h_ * 4); check(mrt_group_gather(gr_, a.data(), a.size() * 4)); return a; }   // the assembled image
    MRTRenderStats stats() { MRTRenderStats s; check(mrt_group_stats(gr_, &s)); return s; }
    std::string reduceMode() const { int32_t m = 0; char note[256]; check(mrt_group_reduce_mode(g_, &m, note, sizeof note)); return note; }

  private:
    void destroy() {
        if (gr_) mrt_group_renderer_destroy(gr_);
        if (template_) mrt_scene_destroy(template_);
        if (g_) mrt_group_destroy(g_);
        gr_ = nullptr; template_ = nullptr; g_ = nullptr;
    }
    int w_, h_;
    MRTGroup g_ = nullptr;
    MRTScene template_ = nullptr;
    MRTGroupRenderer gr_ = nullptr;
};

}  // namespace mrt
