// multihit.hip — all-hits ray queries on device buffers, ordered on a stream of the caller's (mrt_scene_intersect_all_device): per ray the
// max_hits smallest hits under the key (distance, global triangle id), ascending — the order MRT_CLOSER_HIT already decides ties by — each triangle at most once.
//
//   k_intersect_all<true>    the 8-wide layout; the wave's stack in dynamic LDS
//   k_intersect_all<false>   the rope layout (scene option wide = 0) and the empty scene
//
// The walks, the list in LDS (ListSink) and the row emit live in lane_walk.h, where the masked all-hits query uses the same ones: a walk is the closest-hit
// walk with ONE change, its bound — the ray's max_distance while the list holds fewer than K entries, the K-th entry's distance once it is full.  Here the filter is SeesAll.
#include "lane_walk.h"

namespace mrt {
namespace {

// lds: WIDE: the wave's stack (stack_words, from the scene's wide-tree depth), then the list (K slots); sized by the host.  `count`: null, or the caller's
// device-side ray count, read once as a uniform scalar load: the rows at and past it are touched in neither output.
template <bool IS_WIDE>
__global__ void __launch_bounds__(64) k_intersect_all(SceneView s, const MRTRay *__restrict__ rays, uint32_t n, const uint32_t *__restrict__ count, const uint32_t K, const uint32_t stack_words,
                                                      uint4 *__restrict__ out, int32_t *__restrict__ counts) {
    extern __shared__ uint32_t lds[];
    if (count) n = min(n, *count);
    if (blockIdx.x * 64u >= n) return;      // a wave without a ray: a uniform branch to the end
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const MRTRay r = rays[i];
    const f3 ro = mk3(r.origin[0], r.origin[1], r.origin[2]), rd = mk3(r.direction[0], r.direction[1], r.direction[2]);
    constexpr Form FORM = IS_WIDE ? WIDE : ROPE;
    auto k = list_sink<FORM>(s, r.max_distance, reinterpret_cast<float *>(lds + (IS_WIDE ? stack_words : 0u)), K);
    walk<FORM>(s, SeesAll{}, ro, rd, r.min_distance, k, lds);
    emit_list_row(s, k, ro, rd, out + 2u * ((size_t)i * K), counts + i);
}

}  // namespace

// One launch on the caller's stream, nothing else.  Flattened scenes only (the caller has refused the others); the 8-wide layout where it is resident, as the
// other lane walks choose.
int intersect_all_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, size_t n, int max_hits, void *d_out, void *d_hit_counts, const void *d_count) {
    const uint32_t K = (uint32_t)max_hits, stack_words = sc.num_wnodes ? (uint32_t)sc.wide_depth * (WIDE_STACK_LEVEL_BYTES / 4u) : 0u;
    const size_t lds = (size_t)stack_words * 4u + (size_t)K * LIST_SLOT_WORDS * 4u;
    const dim3 grid((uint32_t)((n + 63) / 64));
    if (sc.num_wnodes) hipLaunchKernelGGL(k_intersect_all<true>, grid, dim3(64), lds, stream, sc.view(), static_cast<const MRTRay *>(d_rays), (uint32_t)n, static_cast<const uint32_t *>(d_count), K, stack_words,
                                          static_cast<uint4 *>(d_out), static_cast<int32_t *>(d_hit_counts));
    else hipLaunchKernelGGL(k_intersect_all<false>, grid, dim3(64), lds, stream, sc.view(), static_cast<const MRTRay *>(d_rays), (uint32_t)n, static_cast<const uint32_t *>(d_count), K, stack_words,
                            static_cast<uint4 *>(d_out), static_cast<int32_t *>(d_hit_counts));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
