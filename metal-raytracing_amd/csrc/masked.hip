// masked.hip — the three device queries with a visibility mask (mrt_scene_intersect_closest_masked_device / _any_ / _all_): a triangle of mesh m is visible
// to a ray with mask r iff (mesh_masks[m] & r) != 0, and the result is what the unmasked entry returns on a scene that holds the visible meshes only.
//
//   k_masked<WIDE, Q>         flattened scenes with the 8-wide layout; the wave's stack in dynamic LDS
//   k_masked<ROPE, Q>         the rope layout (scene option wide = 0) and the empty scene
//   k_masked<INSTANCED, Q>    two-level scenes; Q = closest, any
//
// The walks, the sinks that make a query of a walk, the Visibility filter and the records live in lane_walk.h: this unit is the kernel that puts them together
// and its launch.  SceneView and InstanceDev are not changed: the mask table is one more kernel argument.
#include "lane_walk.h"

namespace mrt {
namespace {

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
        auto k = list_sink<FORM>(s, r.max_distance, reinterpret_cast<float *>(lds + (FORM == WIDE ? stack_words : 0u)), K);
        if (!blind) walk<FORM>(s, vis, ro, rd, r.min_distance, k, lds);
        emit_list_row(s, k, ro, rd, static_cast<uint4 *>(out) + 2u * ((size_t)i * K), counts + i);
    }
}

template <Form FORM, MaskedQuery Q>
int launch_masked(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_ray_masks, uint32_t ray_mask, size_t n, uint32_t K, void *d_out, void *d_hit_counts, const void *d_count) {
    const uint32_t stack_words = FORM == WIDE ? (uint32_t)sc.wide_depth * (WIDE_STACK_LEVEL_BYTES / 4u) : 0u;
    const size_t lds = (size_t)stack_words * 4u + (Q == MASKED_ALL ? (size_t)K * LIST_SLOT_WORDS * 4u : 0u);
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
