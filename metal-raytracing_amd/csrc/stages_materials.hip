// stages_materials.hip — the scatter stage with the materials extension ON, on device buffers and ordered on a stream of the caller's (mrt_scene_scatter_materials_device;
// DESIGN.md §10j): what follows a surface when renderer option materials = 1 — emission, the lobe choice on Halton dimension 2 + 5 * max_bounces + bounce, the dielectric
// interface, the GGX specular lobe, and the reference's diffuse path with its albedo divided by the probability of having been chosen.  The lobe choice is
// choose_lobe and the diffuse rows are scatter_diffuse_rows (scatter_math.h) — the functions shade_entry<MATERIALS> (shade.h) and k_scatter (stages.hip) call, not copies
// of them; what is this file's own is the row format, the slot check and the raw emission.  A translation unit of its own: no traversal and no shading kernel is compiled here.
//
//   k_scatter_materials   one thread per row: three 16-byte loads of the surface row (position; normal | type; base colour | resource slot), the direction group of the
//                         incoming ray, one dword of Halton index, three 16-byte gathers from the material table at the row's slot, the light row as 16-byte gathers from
//                         a table of a few lines (diffuse rows only); the Halton recurrence (one value for the lobe choice, then two for a specular row or three to five
//                         for a diffuse one); up to seven 16-byte stores
//
// A thread owns a whole row: a wave's store instruction writes every second (ray and lobe rows) or every (light rows) 16 bytes of a contiguous range and the thread's next
// store fills the gaps.  No LDS, no atomics, no cross-lane traffic.  A caller's row is never trusted with an address: the resource slot is checked against the table's
// extent before the table is read (a slot outside it makes the row "no surface"), and the light pick lies in [0, light_count) by construction (and is clamped).
#include "scatter_math.h"

namespace mrt {
namespace {

// NEXT: the continuation ray is wanted (d_next_rays was given); without it the two normalisations and the cosine-hemisphere sample are not computed
template <bool NEXT>
__global__ void __launch_bounds__(256) k_scatter_materials(const LightDev *__restrict__ lights, const float4 *__restrict__ materials, const uint32_t slots, const int lc, const int dim0, const int dim_lobe,
                                                           const float4 *__restrict__ rays, const float4 *__restrict__ surfaces, const int32_t *__restrict__ halton_index, const uint32_t cap, const uint32_t *__restrict__ count,
                                                           float4 *__restrict__ shadow_rays, float4 *__restrict__ light, float4 *__restrict__ next_rays, float4 *__restrict__ lobes) {
    const uint32_t n = count ? min(cap, *count) : cap;          // the caller's device-side row count (null: every row), read once as a uniform scalar load
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 s0 = zero, s1 = zero, lo = zero, n0 = zero, n1 = zero, b0 = zero, b1 = zero;
    const float4 q1 = surfaces[4 * (size_t)i + 1], q2 = surfaces[4 * (size_t)i + 2];
    const uint32_t slot = __float_as_uint(q2.w);          // (a negative slot is a large unsigned one)
    if (__float_as_int(q1.w) == 1 && slot < slots) {
        const float4 q0 = surfaces[4 * (size_t)i];
        const f3 P = mk3(q0), nrm = mk3(q1);
        f3 surf = mk3(q2);                                                   // the row's base colour: kd and the diffuse weight
        const f3 dir = mk3(rays[2 * (size_t)i + 1]);
        const int idx = halton_index[i];
        const float4 *__restrict__ mp = materials + 3 * (size_t)slot;
        const float4 m0 = mp[0], m1 = mp[1], m2 = mp[2];
        const LobeChoice c = choose_lobe<NEXT>(m0, m1, m2, dir, P, nrm, idx, dim0, dim_lobe, surf);
        const f3 norg = c.org;
        f3 ndir = c.dir, weight = c.weight;
        const int lobe = c.lobe;
        if (lobe == 1) {                                                     // the diffuse path: k_scatter's rows (stages.hip), weighted by the albedo choose_lobe left in `surf`
            weight = surf;
            const DiffuseRows r = scatter_diffuse_rows<NEXT>(lights, lc, idx, dim0, P, nrm, norg);
            s0 = r.shadow0; s1 = r.shadow1; lo = r.light;
            ndir = r.next_dir;
        }
        if (NEXT && lobe != 5) {
            n0 = make_float4(norg.x, norg.y, norg.z, 0.0f);
            n1 = make_float4(ndir.x, ndir.y, ndir.z, __builtin_inff());          // :391
        }
        b0 = make_float4(weight.x, weight.y, weight.z, __int_as_float(lobe));
        b1 = make_float4(m2.x, m2.y, m2.z, 0.0f);                                // the raw emission: the throughput is the caller's
    }
    shadow_rays[2 * (size_t)i] = s0; shadow_rays[2 * (size_t)i + 1] = s1;
    light[i] = lo;
    if (NEXT) { next_rays[2 * (size_t)i] = n0; next_rays[2 * (size_t)i + 1] = n1; }
    lobes[2 * (size_t)i] = b0; lobes[2 * (size_t)i + 1] = b1;
}

}  // namespace

int scatter_materials_device(const DeviceScene &sc, hipStream_t stream, const void *d_rays, const void *d_surfaces, const void *d_halton_index, size_t n, int bounce, int max_bounces,
                             int light_count, void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes, const void *d_count) {
    const dim3 grid((uint32_t)((n + 255) / 256));          // n < 2^31 (the capacity, whatever the count)
    const int dim0 = 2 + 5 * bounce, dim_lobe = 2 + 5 * max_bounces + bounce;          // max_bounces <= 16, bounce < max_bounces: dim_lobe <= 97, below the prime table's 100
    const uint32_t slots = (uint32_t)(sc.materials.n / 3);          // instances x max_submeshes (three rows per resource slot)
    hipLaunchKernelGGL(d_next_rays ? k_scatter_materials<true> : k_scatter_materials<false>, grid, dim3(256), 0, stream, sc.lights.p, sc.materials.p, slots, light_count, dim0, dim_lobe,
                       static_cast<const float4 *>(d_rays), static_cast<const float4 *>(d_surfaces), static_cast<const int32_t *>(d_halton_index), (uint32_t)n, static_cast<const uint32_t *>(d_count),
                       static_cast<float4 *>(d_shadow_rays), static_cast<float4 *>(d_light), static_cast<float4 *>(d_next_rays), static_cast<float4 *>(d_lobes));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
