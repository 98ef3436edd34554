// paths.h — the integrator's path state on the caller's stream (paths.hip): reset, advance (throughput, emission, the two keep masks), the light's
// deposit and the running average.  One launch each and nothing else: no allocation, no copy, no wait.  d_count: null, or one uint32 on the device — the kernel then
// handles the rows below min(n, *d_count) and touches no other (§10k).  The arguments are checked by the entries (api.cpp); n and npixels are below 2^31.
#pragma once
#include "scene_device.h"

namespace mrt {

int reset_paths_device(hipStream_t stream, size_t n, void *d_throughput, void *d_pixel, void *d_radiance, size_t npixels);      // d_radiance may be null
// exactly one of d_surfaces / d_lobes; d_keep_path may be null (the last bounce); the diffuse form reads neither d_pixel nor d_radiance
int advance_paths_device(hipStream_t stream, size_t n, const void *d_count, const void *d_surfaces, const void *d_lobes, const void *d_light, void *d_throughput, const void *d_pixel,
                         void *d_radiance, size_t npixels, void *d_keep_shadow, void *d_keep_path);
int deposit_light_device(hipStream_t stream, size_t n, const void *d_count, const void *d_occluded, const void *d_light, const void *d_throughput, const void *d_pixel, void *d_radiance,
                         size_t npixels);
int fold_sample_device(hipStream_t stream, size_t npixels, void *d_sample, void *d_accum, uint32_t frame_index, bool clear_sample);

}  // namespace mrt
