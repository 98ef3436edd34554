// stages_materials.hip — the scatter stage with the materials extension ON, on device buffers and ordered on a stream of the caller's (mrt_scene_scatter_materials_device;
// DESIGN.md §10j): what follows a surface when renderer option materials = 1 — emission, the lobe choice on Halton dimension 2 + 5 * max_bounces + bounce, the dielectric
// interface, the GGX specular lobe, and the reference's diffuse path with its albedo divided by the probability of having been chosen.  shade_entry<MATERIALS>'s block
// (shade.h) followed by k_scatter's diffuse path (stages.hip), each expression restated in its order, in a translation unit of its own: stages.hip, every shading kernel
// and every traversal kernel keep their code objects.
//
//   k_scatter_materials   one thread per row: three 16-byte loads of the surface row (position; normal | type; base colour | resource slot), the direction group of the
//                         incoming ray, one dword of Halton index, three 16-byte gathers from the material table at the row's slot, the light row as 16-byte gathers from
//                         a table of a few lines (diffuse rows only); the Halton recurrence (one value for the lobe choice, then two for a specular row or three to five
//                         for a diffuse one); up to seven 16-byte stores
//
// A thread owns a whole row: a wave's store instruction writes every second (ray and lobe rows) or every (light rows) 16 bytes of a contiguous range and the thread's next
// store fills the gaps.  No LDS, no atomics, no cross-lane traffic.  A caller's row is never trusted with an address: the resource slot is checked against the table's
// extent before the table is read (a slot outside it makes the row "no surface"), and the light pick lies in [0, light_count) by construction (and is clamped).
#include "scene_device.h"
#include "device_math.h"

namespace mrt {
namespace {

// NEXT: the continuation ray is wanted (d_next_rays was given); without it the two normalisations and the cosine-hemisphere sample are not computed
template <bool NEXT>
__global__ void __launch_bounds__(256) k_scatter_materials(const LightDev *__restrict__ lights, const float4 *__restrict__ materials, const uint32_t slots, const int lc, const int dim0, const int dim_lobe,
                                                           const float4 *__restrict__ rays, const float4 *__restrict__ surfaces, const int32_t *__restrict__ halton_index, const uint32_t n,
                                                           float4 *__restrict__ shadow_rays, float4 *__restrict__ light, float4 *__restrict__ next_rays, float4 *__restrict__ lobes) {
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
        f3 norg = P + nrm * 1e-3f;                                           // :350, :390
        f3 ndir = mk3(0, 0, 0), weight = mk3(0, 0, 0);
        int lobe = 1;
        const float ul = halton_dev(idx, dim_lobe);
        const f3 spec = mk3(m1);
        const float kd = fmaxf(surf.x, fmaxf(surf.y, surf.z)), ks = fmaxf(spec.x, fmaxf(spec.y, spec.z));
        const float dis = m0.w, ns = m1.w, ni = m2.w;
        const float trn = (dis > 0.0f && dis < 1.0f && ni > 0.0f) ? 1.0f - dis : 0.0f;
        if (ul < trn) {                                                      // dielectric interface
            const float u2 = ul / trn;
            const float cd = dot3(dir, nrm);
            const bool entering = cd < 0.0f;
            const f3 nn = entering ? nrm : neg3(nrm);
            const float eta = entering ? 1.0f / ni : ni;
            const float cosi = entering ? -cd : cd;
            const float sin2t = (eta * eta) * (1.0f - cosi * cosi);
            float r0 = (1.0f - ni) / (1.0f + ni); r0 = r0 * r0;
            float F = 1.0f, cost = 0.0f;
            if (sin2t < 1.0f) { cost = __builtin_sqrtf(1.0f - sin2t); const float c = entering ? cosi : cost; const float x = 1.0f - c; const float x2 = x * x; F = r0 + (1.0f - r0) * ((x2 * x2) * x); }
            f3 nd;
            if (u2 < F) { nd = dir + nn * (2.0f * cosi); norg = P + nn * 1e-3f; lobe = 2; }
            else { nd = dir * eta + nn * (eta * cosi - cost); norg = P + nn * -1e-3f; lobe = 3; }
            if (NEXT) ndir = normalize3(nd);
            weight = mk3(1.0f, 1.0f, 1.0f);
        } else {
            const float ud = trn > 0.0f ? (ul - trn) / (1.0f - trn) : ul;
            const float ps = (ks > 0.0f && ns > 0.0f) ? ks / (ks + kd) : 0.0f;
            if (ud < ps) {                                                   // specular lobe
                const float hx = halton_dev(idx, dim0 + 3), hy = halton_dev(idx, dim0 + 4);
                const float a2 = 2.0f / (ns + 2.0f);
                const float ct2 = (1.0f - hy) / (1.0f + (a2 - 1.0f) * hy);
                const float ct = __builtin_sqrtf(ct2), st = __builtin_sqrtf(1.0f - ct2);
                float sp_, cp_; sincos_2pi_dev(hx, sp_, cp_);
                const f3 hw = align_hemisphere_dev(mk3(st * cp_, ct, st * sp_), nrm);
                const float dh = dot3(dir, hw);
                const f3 wi = dir - hw * (2.0f * dh);
                lobe = 5;                                                    // sampled below the surface: the path is absorbed
                if (dot3(wi, nrm) > 0.0f) {
                    weight = spec * (1.0f / ps);
                    if (NEXT) ndir = normalize3(wi);
                    lobe = 4;
                }
            } else if (ps > 0.0f) surf = surf * (1.0f / (1.0f - ps));
        }
        if (lobe == 1) {                                                     // the diffuse path: k_scatter's, stages.hip
            weight = surf;
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
            lo = make_float4(lcol.x, lcol.y, lcol.z, wants ? 1.0f : 0.0f);
            if (wants) {
                s0 = make_float4(norg.x, norg.y, norg.z, 0.0f);                  // :350
                s1 = make_float4(ldir.x, ldir.y, ldir.z, ldist - 1e-3f);         // :356
            }
            if (NEXT) {
                const float hx = halton_dev(idx, dim0 + 3), hy = halton_dev(idx, dim0 + 4);         // :384-385
                ndir = align_hemisphere_dev(sample_cosine_hemisphere_dev(hx, hy), nrm);             // :387-388
            }
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
                             int light_count, void *d_shadow_rays, void *d_light, void *d_next_rays, void *d_lobes) {
    const dim3 grid((uint32_t)((n + 255) / 256));          // n < 2^31
    const int dim0 = 2 + 5 * bounce, dim_lobe = 2 + 5 * max_bounces + bounce;          // max_bounces <= 16, bounce < max_bounces: dim_lobe <= 97, below the prime table's 100
    const uint32_t slots = (uint32_t)(sc.materials.n / 3);          // instances x max_submeshes (three rows per resource slot)
    if (d_next_rays) hipLaunchKernelGGL(k_scatter_materials<true>, grid, dim3(256), 0, stream, sc.lights.p, sc.materials.p, slots, light_count, dim0, dim_lobe, static_cast<const float4 *>(d_rays),
                                        static_cast<const float4 *>(d_surfaces), static_cast<const int32_t *>(d_halton_index), (uint32_t)n, static_cast<float4 *>(d_shadow_rays),
                                        static_cast<float4 *>(d_light), static_cast<float4 *>(d_next_rays), static_cast<float4 *>(d_lobes));
    else hipLaunchKernelGGL(k_scatter_materials<false>, grid, dim3(256), 0, stream, sc.lights.p, sc.materials.p, slots, light_count, dim0, dim_lobe, static_cast<const float4 *>(d_rays),
                            static_cast<const float4 *>(d_surfaces), static_cast<const int32_t *>(d_halton_index), (uint32_t)n, static_cast<float4 *>(d_shadow_rays),
                            static_cast<float4 *>(d_light), static_cast<float4 *>(nullptr), static_cast<float4 *>(d_lobes));
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
