// variance.h — the variance-guided a-trous filter on device buffers and the sample image of its moments, on the caller's stream (variance.hip): the
// second luminance moment, a per-pixel variance estimate and a filter whose colour term is measured in standard deviations.  No allocation, no copy, no wait.  The
// arguments are checked by the entries (api.cpp): width x height below 2^30, the buffers given, aligned and apart, the parameters in range.
#pragma once
#include "scene_device.h"

namespace mrt {

int moments_sample_device(hipStream_t stream, int width, int height, const void *d_sample, const void *d_albedo, int demodulate, void *d_out);
// d_workspace: two images of width x height float4 (denoise_workspace_bytes); p was checked
int denoise_variance_device(hipStream_t stream, int width, int height, const void *d_image, const void *d_moments, const void *d_normal_depth, const void *d_albedo,
                            void *d_workspace, void *d_out, const MRTDenoiseParams &p);

}  // namespace mrt
