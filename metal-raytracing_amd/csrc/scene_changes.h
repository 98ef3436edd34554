// scene_changes.h — what changed in a scene since its last commit, as one value, and what the next mrt_scene_commit has to do about it.
// Host only: no HIP, nothing of scene_device.h.  tests/sanitize/scene_changes_harness.cpp drives it alone.
#pragma once

namespace mrt {

// none < transforms, vertices < rebuild: the least work a commit may do.  `rebuild` is a mesh, a submesh or an option changed, or transforms AND vertices.
enum class Pending { none, transforms, vertices, rebuild };
constexpr Pending join(Pending a, Pending b) { return a == Pending::none ? b : (b == Pending::none || a == b) ? a : Pending::rebuild; }

enum class CommitRecipe {
    tlas_only,                // two-level: instance rows + TLAS, the BLASes stay (update_tlas)
    refit_blas_else_build,    // two-level: the changed meshes' BLASes refitted in place + the TLAS (refit_two_level); a scene it answers MRT_ERR_UNSUPPORTED for is built
    build_keep_geometry,      // flattened: built from the object-space geometry already on the device, under the new transforms
    build_refit,              // flattened: the resident tree refitted where build_flat can (same triangle count, a layout to refit), built otherwise
    build                     // everything
};
// same_instance_list: the device's instance rows are the scene's mesh list (update_tlas rewrites rows, it adds none).  A clean scene (none) committed again is built again.
constexpr CommitRecipe commit_recipe(Pending p, bool instancing, bool refit_option, bool same_instance_list) {
    return p == Pending::transforms ? (!instancing ? CommitRecipe::build_keep_geometry : same_instance_list ? CommitRecipe::tlas_only : CommitRecipe::build)
         : p == Pending::vertices && refit_option ? (instancing ? CommitRecipe::refit_blas_else_build : CommitRecipe::build_refit)
         : CommitRecipe::build;
}

// (Join is a parameter for one reader: the harness plants a wrong join and has the tests catch it)
template <Pending (*Join)(Pending, Pending)> class SceneChangesOver {
    bool committed_ = false;
    Pending pending_ = Pending::rebuild;
public:
    bool committed() const { return committed_; }
    // what the stream-ordered update entries say to a scene that is not committed: only transforms, or only vertices, wait for a commit
    bool host_changes_pending() const { return !committed_ && (pending_ == Pending::transforms || pending_ == Pending::vertices); }
    // the host changed the scene: transforms (mrt_scene_set_instance_transform), vertices (mrt_scene_update_mesh), rebuild (a mesh, a submesh, an option)
    void host_changed(Pending kind) { committed_ = false; pending_ = Join(pending_, kind); }
    // a sync of the host copies learned of changes made on the device and not yet refitted there (flattened vertices: §10d, BLAS vertices: §10f) or moved instances (§10e).
    // The scene stays committed if it was: what the device entries did is traversable as it is.
    // The one exception to the join: a flattened scene that waits for a commit with transforms alone keeps `transforms` when device-side vertices turn up.  build_keep_geometry
    // flattens g_pos and keeps `normals`, which is where mrt_scene_update_mesh_device wrote them: that build covers them, at less than a full build's cost.
    void device_changes_found(bool flat_vertices, bool blas_vertices, bool moved_instances) {
        if (flat_vertices && !(!committed_ && pending_ == Pending::transforms)) pending_ = Join(pending_, Pending::vertices);
        if (blas_vertices) pending_ = Join(pending_, Pending::vertices);
        if (moved_instances) pending_ = Join(pending_, Pending::transforms);
    }
    CommitRecipe recipe(bool instancing, bool refit_option, bool same_instance_list) const { return commit_recipe(pending_, instancing, refit_option, same_instance_list); }
    void commit_done() { committed_ = true; pending_ = Pending::none; }
    Pending pending() const { return pending_; }          // (for the harness and for messages: decisions go through recipe())
};
using SceneChanges = SceneChangesOver<join>;

}  // namespace mrt
