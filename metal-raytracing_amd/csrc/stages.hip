// stages.hip — the two steps of the reference's kernel that frame the query and the surface lookup, on device buffers and ordered on a stream of the caller's
// (mrt_renderer_primary_rays_device / mrt_scene_scatter_device): where the rays come from (Raytracing.metal:171-221) and what follows a surface
// (:272-391, the diffuse path: materials extension off).  primary_ray's and shade_entry's expressions (shade.h) restated in their order in a translation unit of its
// own: no traversal, no shading kernel and no builder is touched.  With the query entries (§10c) and mrt_scene_resolve_hits_device (§10h) a caller writes the
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
#include "device_math.h"

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
    const float px = (float)(int)x + r0, py = (float)(int)y + r1;        // :204
    float uvx = px / (float)p.width, uvy = py / (float)p.height;         // :207
    uvx = uvx * 2.0f - 1.0f; uvy = uvy * 2.0f - 1.0f;                    // :208
    const f3 dir = normalize3((uvx * mk3(p.cam_right) + uvy * mk3(p.cam_up)) + mk3(p.cam_fwd));   // :216-218
    float4 *const o = rays + 2 * (size_t)i;
    o[0] = make_float4(p.cam_pos.x, p.cam_pos.y, p.cam_pos.z, 0.0f);     // :214
    o[1] = make_float4(dir.x, dir.y, dir.z, __builtin_inff());
    halton_index[i] = idx;
}

// NEXT: the bounce ray is wanted (d_next_rays was given)
template <bool NEXT>
__global__ void __launch_bounds__(256) k_scatter(const LightDev *__restrict__ lights, const int lc, const int dim0, const float4 *__restrict__ surfaces, const int32_t *__restrict__ halton_index,
                                                 const uint32_t n, float4 *__restrict__ shadow_rays, float4 *__restrict__ light, float4 *__restrict__ next_rays) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 s0 = zero, s1 = zero, lo = zero, n0 = zero, n1 = zero;
    const float4 q1 = surfaces[4 * (size_t)i + 1];
    if (__float_as_int(q1.w) == 1) {
        const float4 q0 = surfaces[4 * (size_t)i];
        const f3 P = mk3(q0), nrm = mk3(q1);
        const int idx = halton_index[i];
        const float ls = halton_dev(idx, dim0 + 0);                          // :272
        int li = min((int)(ls * (float)lc), lc - 1);                         // :273
        li = li < 0 ? 0 : li;
        const LightDev L = lights[li];
        const int ltype = __float_as_int(L.position.w);
        f3 ldir, lcol; float ldist;
        if (ltype == MRTLightTypeAreaLight) {                                // :281-290, :94-128
            const float ax = halton_dev(idx, dim0 + 1) * 2.0f - 1.0f;
            const float ay = halton_dev(idx, dim0 + 2) * 2.0f - 1.0f;
            const f3 sp = (mk3(L.position) + mk3(L.right) * ax) + mk3(L.up) * ay;
            ldir = sp - P;
            ldist = length3(ldir);
            const float inv = 1.0f / (ldist > 1e-3f ? ldist : 1e-3f);
            ldir = ldir * inv;
            lcol = mk3(L.color) * (inv * inv);
            lcol = lcol * saturatef(dot3(neg3(ldir), mk3(L.forward)));
        } else if (ltype == MRTLightTypeSpotlight) {                         // :292-316
            ldir = mk3(L.position) - P;
            ldist = length3(ldir);
            const float inv = 1.0f / (ldist > 1e-3f ? ldist : 1e-3f);
            ldir = ldir * inv;
            lcol = mk3(0, 0, 0);
            const float spot = dot3(neg3(ldir), mk3(L.dirn));
            if (spot > L.dirn.w) lcol = (mk3(L.color) * inv) * inv;
        } else if (ltype == MRTLightTypePointlight) {                        // :317-322
            ldir = mk3(L.position) - P;
            ldist = length3(ldir);
            const float inv = 1.0f / (ldist > 1e-3f ? ldist : 1e-3f);
            ldir = ldir * inv;
            lcol = (mk3(L.color) * inv) * inv;
        } else {                                                             // :323-327
            ldir = neg3(mk3(L.dirn));
            ldist = __builtin_inff();
            lcol = mk3(L.color);
        }
        lcol = lcol * saturatef(dot3(nrm, ldir));                            // :331
        lcol = lcol * (float)lc;                                             // :335
        const bool wants = length3(lcol) > 0.0001f;                          // :341
        const f3 org = P + nrm * 1e-3f;                                      // :350, :390
        lo = make_float4(lcol.x, lcol.y, lcol.z, wants ? 1.0f : 0.0f);
        if (wants) {
            s0 = make_float4(org.x, org.y, org.z, 0.0f);
            s1 = make_float4(ldir.x, ldir.y, ldir.z, ldist - 1e-3f);         // :356
        }
        if (NEXT) {
            const float hx = halton_dev(idx, dim0 + 3), hy = halton_dev(idx, dim0 + 4);         // :384-385
            const f3 nd = align_hemisphere_dev(sample_cosine_hemisphere_dev(hx, hy), nrm);      // :387-388
            n0 = make_float4(org.x, org.y, org.z, 0.0f);
            n1 = make_float4(nd.x, nd.y, nd.z, __builtin_inff());            // :391
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
                   void *d_next_rays) {
    const dim3 grid((uint32_t)((n + 255) / 256));          // n < 2^31
    const int dim0 = 2 + 5 * bounce;                         // dim0 + 4 < 100, the prime table's size: bounce <= 18
    if (d_next_rays) hipLaunchKernelGGL(k_scatter<true>, grid, dim3(256), 0, stream, sc.lights.p, light_count, dim0, static_cast<const float4 *>(d_surfaces), static_cast<const int32_t *>(d_halton_index),
                                        (uint32_t)n, static_cast<float4 *>(d_shadow_rays), static_cast<float4 *>(d_light), static_cast<float4 *>(d_next_rays));
    else hipLaunchKernelGGL(k_scatter<false>, grid, dim3(256), 0, stream, sc.lights.p, light_count, dim0, static_cast<const float4 *>(d_surfaces), static_cast<const int32_t *>(d_halton_index),
                            (uint32_t)n, static_cast<float4 *>(d_shadow_rays), static_cast<float4 *>(d_light), static_cast<float4 *>(nullptr));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
