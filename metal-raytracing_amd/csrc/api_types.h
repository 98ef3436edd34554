// api_types.h — what the opaque handles of include/mrt_abi.h point at (shared by api.cpp and group.hip).
#pragma once
#include "renderer.h"
#include "scene_changes.h"

struct MRTContext_ {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char name[256] = {0};
    int live = 0;                           // scenes and renderers made on this context and not yet destroyed: mrt_context_destroy refuses while any is left
};
struct MRTScene_ {
    MRTContext ctx = nullptr;
    std::vector<mrt::HostMesh> meshes;
    std::vector<MRTLight> lights;
    mrt::BuildOptions opt;
    mrt::DeviceScene dev;
    mrt::SceneChanges changes;              // committed or not, and what changed since the last commit: scene_changes.h decides what the next commit does
    int renderers = 0;                      // renderers made on this scene and not yet destroyed: mrt_scene_destroy refuses while any is left (they hold a pointer to `dev`)
    size_t stage_need = 0;                  // bytes the upload staging of the meshes added so far will take (mrt_mesh_add_submesh grows the pinned area)
    std::vector<uint32_t> mesh_masks;       // visibility mask per mesh id (mrt_scene_set_mesh_masks); shorter than `meshes` until someone asks: the missing entries are 0xFFFFFFFF
    bool masks_stale = false;               // masks set while the scene was not committed: the next commit uploads the table (otherwise only a commit that changes the mesh count does)
    size_t masks_uploaded = SIZE_MAX;       // entries of mesh_masks the device table holds (SIZE_MAX: never written; 0 after the commit of an empty scene, whose one-word allocation holds nothing)
};
struct MRTRenderer_ {
    MRTContext ctx = nullptr;
    MRTScene scene = nullptr;
    mrt::Renderer r;
};
struct MRTMeshData_ { mrt::MeshData m; };
int mrt_scene_sync_host_meshes(MRTScene scene);      // api.cpp: HostMesh copies brought up to date after mrt_scene_update_mesh_device (vertices) or mrt_scene_set_instance_transforms_device (matrices); blocks; no-op otherwise


#define MRT_TRY try {
#define MRT_CATCH                                                                      \
    } catch (const std::bad_alloc &) { mrt::set_error("out of host memory"); return MRT_ERR_OUT_OF_MEMORY; } \
    catch (const std::exception &e) { mrt::set_error(std::string("exception: ") + e.what()); return MRT_ERR_INVALID_ARGUMENT; } \
    catch (...) { mrt::set_error("unknown exception"); return MRT_ERR_INVALID_ARGUMENT; }
#define REQUIRE(cond, msg) do { if (!(cond)) { mrt::set_error(msg); return MRT_ERR_INVALID_ARGUMENT; } } while (0)
