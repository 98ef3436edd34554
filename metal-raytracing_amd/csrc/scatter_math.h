// scatter_math.h — what follows a surface (Raytracing.metal:272-391) and where a camera ray points (:204-218), once: the expressions the frame's kernels (shade.h) and
// the device-buffer stages (stages.hip, stages_materials.hip) share.  Device functions only — no kernel, no state.  The arithmetic contract is bit-for-bit agreement
// with the oracle under -ffp-contract=off, so an operand order, a clamp or a light type changes HERE and nowhere else.
//
//   camera_ray_dir         pixel + jitter -> the primary ray's direction                                                            (:204-218)
//   eval_light             one light seen from a point: direction, distance, colour after the cosine and the light count           (:281-335)
//   choose_lobe            the materials extension's lobe choice: dielectric interface, GGX specular lobe, or the diffuse path
//   scatter_diffuse_rows   the diffuse rows of a stage: light pick, eval_light, the shadow-ray row, the cosine-hemisphere bounce   (:272-388)
//
// The shade kernels are tuned to the register (shade.h, MRT_SHADE_WAVES), and the SHAPE of these helpers is part of that: results come back by value in a small struct
// that the caller copies into its own variables, and Halton values are fetched through a callable at the place the reference draws them.  Outputs by reference, or
// Halton values computed ahead of the branch that wants them, cost k_shade_pack 16-20 bytes of spills and k_shade_primary its register headroom.
#pragma once
#include "device_math.h"
#include "scene_device.h"

namespace mrt {
namespace {

// Raytracing.metal:204-218: (x, y) the pixel, (r0, r1) its jitter
MRT_DEV f3 camera_ray_dir(const int x, const int y, const float r0, const float r1, const int width, const int height, const f3 right, const f3 up, const f3 fwd) {
    const float px = (float)x + r0, py = (float)y + r1;                      // :204
    float uvx = px / (float)width, uvy = py / (float)height;                 // :207
    uvx = uvx * 2.0f - 1.0f; uvy = uvy * 2.0f - 1.0f;                        // :208
    return normalize3((uvx * right + uvy * up) + fwd);                       // :216-218
}

struct LightSample { f3 dir, col; float dist; };

// The light L of `light_count` seen from P with normal nrm.  hal(k) is the Halton value of dimension dim0 + k of the caller's sample (k = 1, 2: the area light's point;
// called inside that branch only).  The light pick (:272-273) stays with the caller: whether its index can be trusted is the caller's to know.
template <class Hal>
MRT_DEV LightSample eval_light(const LightDev &L, const int light_count, const f3 P, const f3 nrm, Hal hal) {
    LightSample e;
    const int ltype = __float_as_int(L.position.w);
    if (ltype == MRTLightTypeAreaLight) {                                    // :281-290, :94-128
        const float ax = hal(1) * 2.0f - 1.0f;
        const float ay = hal(2) * 2.0f - 1.0f;
        const f3 sp = (mk3(L.position) + mk3(L.right) * ax) + mk3(L.up) * ay;
        e.dir = sp - P;
        e.dist = length3(e.dir);
        const float inv = 1.0f / (e.dist > 1e-3f ? e.dist : 1e-3f);
        e.dir = e.dir * inv;
        e.col = mk3(L.color) * (inv * inv);
        e.col = e.col * saturatef(dot3(neg3(e.dir), mk3(L.forward)));
    } else if (ltype == MRTLightTypeSpotlight) {                             // :292-316
        e.dir = mk3(L.position) - P;
        e.dist = length3(e.dir);
        const float inv = 1.0f / (e.dist > 1e-3f ? e.dist : 1e-3f);
        e.dir = e.dir * inv;
        e.col = mk3(0, 0, 0);
        const float spot = dot3(neg3(e.dir), mk3(L.dirn));
        if (spot > L.dirn.w) e.col = (mk3(L.color) * inv) * inv;
    } else if (ltype == MRTLightTypePointlight) {                            // :317-322
        e.dir = mk3(L.position) - P;
        e.dist = length3(e.dir);
        const float inv = 1.0f / (e.dist > 1e-3f ? e.dist : 1e-3f);
        e.dir = e.dir * inv;
        e.col = (mk3(L.color) * inv) * inv;
    } else {                                                                 // :323-327
        e.dir = neg3(mk3(L.dirn));
        e.dist = __builtin_inff();
        e.col = mk3(L.color);
    }
    e.col = e.col * saturatef(dot3(nrm, e.dir));                             // :331
    e.col = e.col * (float)light_count;                                      // :335
    return e;
}

// The materials extension (renderer option materials = 1; not in raytracingKernel — README.md:8 lists it as open work; the fields are ShaderTypes.h:99-107).  Semantics:
// DESIGN.md "Materials extension"; the CPU checker restates this function expression by expression.
//   lobe     MRTScatterLobe's code: 1 diffuse (the caller goes on with the reference's path on `surf`), 2 interface reflected, 3 interface refracted, 4 specular,
//            5 specular sampled below the surface — the path is absorbed
//   dir      the continuation ray's direction, lobes 2 .. 4 (NEXT only: without it the two normalisations are not computed)
//   org      its origin: on the side of the surface the ray leaves on
//   weight   the factor of the throughput: (1, 1, 1) at the interface, specular / ps for lobe 4, zeros for 1 and 5 (the diffuse weight is `surf`, which leaves
//            divided by the probability of the diffuse path having been chosen)
// m0 .. m2: the resource slot's rows of SceneView::materials; `in` the incoming ray's direction; dim_lobe the Halton dimension of the choice.
struct LobeChoice { int lobe; f3 dir, org, weight; };
template <bool NEXT>
MRT_DEV LobeChoice choose_lobe(const float4 m0, const float4 m1, const float4 m2, const f3 in, const f3 P, const f3 nrm, const int idx, const int dim0, const int dim_lobe, f3 &surf) {
    LobeChoice c;
    c.lobe = 1; c.dir = mk3(0, 0, 0); c.weight = mk3(0, 0, 0);
    c.org = P + nrm * 1e-3f;                                                 // :350, :390
    const float ul = halton_dev(idx, dim_lobe);
    const f3 spec = mk3(m1);
    const float kd = fmaxf(surf.x, fmaxf(surf.y, surf.z)), ks = fmaxf(spec.x, fmaxf(spec.y, spec.z));
    const float dis = m0.w, ns = m1.w, ni = m2.w;
    const float trn = (dis > 0.0f && dis < 1.0f && ni > 0.0f) ? 1.0f - dis : 0.0f;
    if (ul < trn) {                                                          // dielectric interface
        const float u2 = ul / trn;
        const float cd = dot3(in, nrm);
        const bool entering = cd < 0.0f;
        const f3 nn = entering ? nrm : neg3(nrm);
        const float eta = entering ? 1.0f / ni : ni;
        const float cosi = entering ? -cd : cd;
        const float sin2t = (eta * eta) * (1.0f - cosi * cosi);
        float r0 = (1.0f - ni) / (1.0f + ni); r0 = r0 * r0;
        float F = 1.0f, cost = 0.0f;
        if (sin2t < 1.0f) { cost = __builtin_sqrtf(1.0f - sin2t); const float c_ = entering ? cosi : cost; const float x = 1.0f - c_; const float x2 = x * x; F = r0 + (1.0f - r0) * ((x2 * x2) * x); }
        f3 nd;
        if (u2 < F) { nd = in + nn * (2.0f * cosi); c.org = P + nn * 1e-3f; c.lobe = 2; }
        else { nd = in * eta + nn * (eta * cosi - cost); c.org = P + nn * -1e-3f; c.lobe = 3; }
        if (NEXT) c.dir = normalize3(nd);
        c.weight = mk3(1.0f, 1.0f, 1.0f);
    } else {
        const float ud = trn > 0.0f ? (ul - trn) / (1.0f - trn) : ul;
        const float ps = (ks > 0.0f && ns > 0.0f) ? ks / (ks + kd) : 0.0f;
        if (ud < ps) {                                                       // specular lobe
            const float hx = halton_dev(idx, dim0 + 3), hy = halton_dev(idx, dim0 + 4);
            const float a2 = 2.0f / (ns + 2.0f);
            const float ct2 = (1.0f - hy) / (1.0f + (a2 - 1.0f) * hy);
            const float ct = __builtin_sqrtf(ct2), st = __builtin_sqrtf(1.0f - ct2);
            float sp_, cp_; sincos_2pi_dev(hx, sp_, cp_);
            const f3 hw = align_hemisphere_dev(mk3(st * cp_, ct, st * sp_), nrm);
            const float dh = dot3(in, hw);
            const f3 wi = in - hw * (2.0f * dh);
            c.lobe = 5;
            if (dot3(wi, nrm) > 0.0f) {
                c.weight = spec * (1.0f / ps);
                if (NEXT) c.dir = normalize3(wi);
                c.lobe = 4;
            }
        } else if (ps > 0.0f) surf = surf * (1.0f / (1.0f - ps));
    }
    return c;
}

// The diffuse rows of a scatter stage (mrt_scene_scatter_device's outputs, include/mrt_abi.h) for a surface at P with normal nrm: `org` is P + nrm * 1e-3, both rays'
// origin (:350, :390).  A caller's row is not trusted with an address: the light pick is clamped on both sides.  next_dir: NEXT only.
struct DiffuseRows { float4 shadow0, shadow1, light; f3 next_dir; };
template <bool NEXT>
MRT_DEV DiffuseRows scatter_diffuse_rows(const LightDev *__restrict__ lights, const int lc, const int idx, const int dim0, const f3 P, const f3 nrm, const f3 org) {
    DiffuseRows r;
    const float ls = halton_dev(idx, dim0 + 0);                              // :272
    int li = min((int)(ls * (float)lc), lc - 1);                             // :273
    li = li < 0 ? 0 : li;
    const LightDev L = lights[li];
    const LightSample e = eval_light(L, lc, P, nrm, [&](int k) { return halton_dev(idx, dim0 + k); });
    const bool wants = length3(e.col) > 0.0001f;                             // :341
    r.light = make_float4(e.col.x, e.col.y, e.col.z, wants ? 1.0f : 0.0f);
    r.shadow0 = r.shadow1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (wants) {
        r.shadow0 = make_float4(org.x, org.y, org.z, 0.0f);
        r.shadow1 = make_float4(e.dir.x, e.dir.y, e.dir.z, e.dist - 1e-3f);  // :356
    }
    r.next_dir = mk3(0, 0, 0);
    if (NEXT) {
        const float hx = halton_dev(idx, dim0 + 3), hy = halton_dev(idx, dim0 + 4);             // :384-385
        r.next_dir = align_hemisphere_dev(sample_cosine_hemisphere_dev(hx, hy), nrm);           // :387-388
    }
    return r;
}

}  // namespace
}  // namespace mrt
