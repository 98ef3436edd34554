// temporal.h — temporal reprojection of the accumulated image, on the caller's stream (temporal.hip): where each visible surface point was in the previous
// frame, the history fetched there if it is the same surface, and the running average carried on.  No allocation, no copy, no wait.  The arguments are checked by the
// entry (api.cpp): width and height in 1 .. 2^24 - 1, width x height below 2^30, the buffers given, aligned and d_out apart from every input, the parameters in range.
#pragma once
#include "scene_device.h"

namespace mrt {

// d_prev_position may be NULL: the geometry did not move, the surface row's own position is used
int reproject_device(hipStream_t stream, int width, int height, const MRTCamera &camera, const MRTCamera &prev_camera, const void *d_surfaces, const void *d_prev_position,
                     const void *d_prev_normal_depth, const void *d_prev_ids, const void *d_prev_history, const void *d_sample, void *d_out, const MRTReprojectParams &p);

}  // namespace mrt
