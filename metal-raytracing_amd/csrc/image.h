// image.h — what turns a composed frame into an image a host can show, on the caller's stream (image.hip): the first-hit guide buffers folded from the
// bounce-0 surface rows, the a-trous filter of denoise.hip on any image, Reinhard + flip into RGBA8.  No allocation, no copy, no wait.  The arguments are checked by the
// entries (api.cpp): npixels is below 2^31 and not 0, width x height below 2^30, the buffers aligned and apart.
#pragma once
#include "scene_device.h"

namespace mrt {

int fold_guides_device(hipStream_t stream, size_t npixels, const void *d_surfaces, void *d_normal_depth, void *d_albedo, void *d_ids, uint32_t frame_index);
// d_workspace: two images of width x height float4 (denoise_workspace_bytes); p was checked
int denoise_image_device(hipStream_t stream, int width, int height, const void *d_image, const void *d_normal_depth, const void *d_albedo, void *d_workspace, void *d_out,
                         const MRTDenoiseParams &p);
int tonemap_image_device(hipStream_t stream, int width, int height, const void *d_image, void *d_rgba8);
inline size_t denoise_workspace_bytes(int width, int height) { return 2 * ((size_t)width * (size_t)height) * 16; }

}  // namespace mrt
