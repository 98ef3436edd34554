// stages.hip — the two steps of the reference's kernel that frame the query and the surface lookup, on device buffers and ordered on a stream of the caller's
// (mrt_renderer_primary_rays_device / mrt_scene_scatter_device): where the rays come from (Raytracing.metal:171-221) and what follows a surface
// (:272-391, the diffuse path: materials extension off).  The camera-ray direction, the light evaluation and the diffuse rows are camera_ray_dir, eval_light and
// scatter_diffuse_rows (scatter_math.h) — the functions primary_ray and shade_entry (shade.h) call, not copies of them; what is this file's own is the row format and the
// seed hash in place of the renderer's seed table.  A translation unit of its own: no traversal, no shading kernel and no builder is compiled here.
// With the query entries (§10c) and mrt_scene_resolve_hits_device (§10h) a caller writes the
// reference's integrator, or a variant of it, as five stream-ordered calls and element-wise arithmetic of their own.
//
//   k_primary_rays   one thread per pixel: the seed hash, Halton dimensions 0 and 1, the camera basis — two 16-byte stores (the ray) and one dword store (the index)
//   k_scatter        one thread per row: two 16-byte loads of the surface row (position and normal | type; colour and ids are not used, though the lines they lie on
//                    are fetched all the same) and one dword load, the Halton recurrence (three to five values), the light row as 16-byte gathers from a table of a
//                    few lines, up to five 16-byte stores
//
// A thread owns a whole row, so a wave's store instruction writes every second (ray rows) or every (light rows) 16 bytes of a contiguous range and the thread's next
// store fills the gaps: each 128-byte line is completed by two instructions issued back to back.  No LDS, no atomics, no cross-lane traffic.
// A caller's row is never trusted with an address: the one index made from it, the light pick, lies in [0, light_count) by construction (and is clamped).
#include "renderer.h"
#include "scatter_math.h"

namespace mrt {
namespace {

struct PrimaryParams {
    float4 cam_pos, cam_right, cam_up, cam_fwd;
    int32_t width, height;
    uint32_t seed, sample_index;
};

__global__ void __launch_bounds__(256) k_primary_rays(const PrimaryParams p, const uint32_t npix, float4 *__restrict__ rays, int32_t *__restrict__ halton_index) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const uint32_t y = i / (uint32_t)p.width, x = i - y * (uint32_t)p.width;
    const uint32_t offset = seed_hash_dev(p.seed, i);                    // :175, the renderer's seed table entry of sub-frame 0
    const int idx = (int)(offset + p.sample_index);
    const float r0 = halton_dev(idx, 0), r1 = halton_dev(idx, 1);        // :202-203
    const f3 dir = camera_ray_dir((int)x, (int)y, r0, r1, p.width, p.height, mk3(p.cam_right), mk3(p.cam_up), mk3(p.cam_fwd));
    float4 *const o = rays + 2 * (size_t)i;
    o[0] = make_float4(p.cam_pos.x, p.cam_pos.y, p.cam_pos.z, 0.0f);     // :214
    o[1] = make_float4(dir.x, dir.y, dir.z, __builtin_inff());
    halton_index[i] = idx;
}

// NEXT: the bounce ray is wanted (d_next_rays was given)
template <bool NEXT>
__global__ void __launch_bounds__(256) k_scatter(const LightDev *__restrict__ lights, const int lc, const int dim0, const float4 *__restrict__ surfaces, const int32_t *__restrict__ halton_index,
                                                 const uint32_t cap, const uint32_t *__restrict__ count, float4 *__restrict__ shadow_rays, float4 *__restrict__ light, float4 *__restrict__ next_rays) {
    const uint32_t n = count ? min(cap, *count) : cap;          // the caller's device-side row count (null: every row), read once as a uniform scalar load
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 s0 = zero, s1 = zero, lo = zero, n0 = zero, n1 = zero;
    const float4 q1 = surfaces[4 * (size_t)i + 1];
    if (__float_as_int(q1.w) == 1) {
        const float4 q0 = surfaces[4 * (size_t)i];
        const f3 P = mk3(q0), nrm = mk3(q1);
        const int idx = halton_index[i];
        const f3 org = P + nrm * 1e-3f;                                      // :350, :390
        const DiffuseRows r = scatter_diffuse_rows<NEXT>(lights, lc, idx, dim0, P, nrm, org);
        s0 = r.shadow0; s1 = r.shadow1; lo = r.light;
        if (NEXT) {
            n0 = make_float4(org.x, org.y, org.z, 0.0f);
            n1 = make_float4(r.next_dir.x, r.next_dir.y, r.next_dir.z, __builtin_inff());       // :391
        }
    }
    shadow_rays[2 * (size_t)i] = s0; shadow_rays[2 * (size_t)i + 1] = s1;
    light[i] = lo;
    if (NEXT) { next_rays[2 * (size_t)i] = n0; next_rays[2 * (size_t)i + 1] = n1; }
}

}  // namespace

int primary_rays_device(const Renderer &r, hipStream_t stream, uint32_t sample_index, void *d_rays, void *d_halton_index) {
    PrimaryParams p;
    p.cam_pos = make_float4(r.camera.position.x, r.camera.position.y, r.camera.position.z, 0);
    p.cam_right = make_float4(r.camera.right.x, r.camera.right.y, r.camera.right.z, 0);
    p.cam_up = make_float4(r.camera.up.x, r.camera.up.y, r.camera.up.z, 0);
    p.cam_fwd = make_float4(r.camera.forward.x, r.camera.forward.y, r.camera.forward.z, 0);
    p.width = r.width; p.height = r.height; p.seed = r.seed; p.sample_index = sample_index;
    const uint32_t npix = (uint32_t)((size_t)r.width * r.height);          // width x height < 2^30 (mrt_renderer_create / _resize)
    hipLaunchKernelGGL(k_primary_rays, dim3((npix + 255u) / 256u), dim3(256), 0, stream, p, npix, static_cast<float4 *>(d_rays), static_cast<int32_t *>(d_halton_index));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

int scatter_device(const DeviceScene &sc, hipStream_t stream, const void *d_surfaces, const void *d_halton_index, size_t n, int bounce, int light_count, void *d_shadow_rays, void *d_light,
                   void *d_next_rays, const void *d_count) {
    const dim3 grid((uint32_t)((n + 255) / 256));          // n < 2^31 (the capacity, whatever the count)
    const int dim0 = 2 + 5 * bounce;                         // dim0 + 4 < 100, the prime table's size: bounce <= 18
    hipLaunchKernelGGL(d_next_rays ? k_scatter<true> : k_scatter<false>, grid, dim3(256), 0, stream, sc.lights.p, light_count, dim0, static_cast<const float4 *>(d_surfaces),
                       static_cast<const int32_t *>(d_halton_index), (uint32_t)n, static_cast<const uint32_t *>(d_count), static_cast<float4 *>(d_shadow_rays), static_cast<float4 *>(d_light),
                       static_cast<float4 *>(d_next_rays));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
