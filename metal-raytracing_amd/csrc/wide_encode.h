// wide_encode.h — the one writer of the compressed 8-wide node (scene_device.h "wide node"), for host and device.
//
// Four places write such nodes and must agree bit for bit: the build (bvh_build.hip k_wide_level), the refit of a flattened scene or a BLAS (bvh_refit.hip k_refit_wide_level),
// the refit of the 8-wide TLAS (tlas_refit.hip k_tlas_wide_level) and the host TLAS build (two_level.hip WideTlasBuilder).  All of them call what is here and keep only what is
// their own: which children a node gets, where their boxes come from, words 1 (child_base, tri_base, meta).  Host and device are compiled with -ffp-contract=off (Makefile),
// so a __host__ __device__ function is the same arithmetic in both passes.
//   word 0            origin p = the node box's lo | the three exponents, unbiased (int8, e - 127) | imask << 24
//   words 2, 3, 4     qlo x, y, z then qhi x, y, z: eight bytes each, slot sl in byte sl; a plane is p + q * 2^e.  An empty slot holds qlo = 255, qhi = 0 on every axis.
// The clamp of a plane to 0 .. 255 is fminf(fmaxf(..)), as the three kernels always had it; the host builder's std::min(std::max(..)) differed only for a NaN plane, where
// its conversion to an integer was undefined anyway.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace mrt {

#define MRT_HD __host__ __device__ __forceinline__

MRT_HD uint32_t wide_bits_of(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
MRT_HD float wide_float_of(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// The node's grid: p = lo, step 2^e >= extent / 255 per axis (the exponent rounded up, kept to 1 .. 254 so that step and its inverse are normal numbers).
struct WideGrid { uint32_t eb[3]; float step[3], inv_step[3]; };
MRT_HD WideGrid wide_grid(const float nl[3], const float nh[3]) {
    WideGrid g;
    for (int a = 0; a < 3; a++) {
        const float sdiv = (nh[a] - nl[a]) / 255.0f;
        const uint32_t bits = wide_bits_of(sdiv);
        uint32_t e = (bits >> 23) + ((bits & 0x7FFFFFu) ? 1u : 0u);
        if (e < 1u) e = 1u;
        if (e > 254u) e = 254u;
        g.eb[a] = e; g.step[a] = wide_float_of(e << 23); g.inv_step[a] = wide_float_of((254u - e) << 23);          // 2^(e-127) and 2^-(e-127)
    }
    return g;
}

// One child's planes on that grid, rounded outwards; stepped once more where the float32 decode p + q * step fails to enclose the child after the rounding of (c - p).
MRT_HD void wide_quantise(const WideGrid &g, const float nl[3], const float clo[3], const float chi[3], uint32_t ql[3], uint32_t qh[3]) {
    for (int a = 0; a < 3; a++) {
        float fl = floorf((clo[a] - nl[a]) * g.inv_step[a]), fh = ceilf((chi[a] - nl[a]) * g.inv_step[a]);
        fl = fminf(fmaxf(fl, 0.0f), 255.0f); fh = fminf(fmaxf(fh, 0.0f), 255.0f);
        if (nl[a] + fl * g.step[a] > clo[a] && fl > 0.0f) fl -= 1.0f;
        if (nl[a] + fh * g.step[a] < chi[a] && fh < 255.0f) fh += 1.0f;
        ql[a] = (uint32_t)fl; qh[a] = (uint32_t)fh;
    }
}

// Slot sl's bytes into the six plane words q (zero before the first slot): the child's planes when it has one, the empty values otherwise.
MRT_HD void wide_slot_planes(const WideGrid &g, const float nl[3], int sl, bool occupied, const float clo[3], const float chi[3], uint32_t q[6][2]) {
    uint32_t ql[3] = {255, 255, 255}, qh[3] = {0, 0, 0};
    if (occupied) wide_quantise(g, nl, clo, chi, ql, qh);
    for (int a = 0; a < 3; a++) { q[a][sl >> 2] |= ql[a] << (8 * (sl & 3)); q[3 + a][sl >> 2] |= qh[a] << (8 * (sl & 3)); }
}

MRT_HD float4 wide_f4u(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return make_float4(wide_float_of(a), wide_float_of(b), wide_float_of(c), wide_float_of(d)); }

// Words 0, 2, 3 and 4 of the node at w; word 1 is the caller's.
MRT_HD void wide_write_node(float4 *w, const float nl[3], const WideGrid &g, uint32_t imask, const uint32_t q[6][2]) {
    // exponents are stored unbiased (int8, e - 127): the traversal scales 1/direction with v_ldexp_f32
    w[0] = make_float4(nl[0], nl[1], nl[2], wide_float_of(((g.eb[0] - 127u) & 0xFFu) | (((g.eb[1] - 127u) & 0xFFu) << 8) | (((g.eb[2] - 127u) & 0xFFu) << 16) | (imask << 24)));
    w[2] = wide_f4u(q[0][0], q[0][1], q[1][0], q[1][1]);
    w[3] = wide_f4u(q[2][0], q[2][1], q[3][0], q[3][1]);
    w[4] = wide_f4u(q[4][0], q[4][1], q[5][0], q[5][1]);
}

// A whole node from eight slot boxes (a refit; mrt_debug_wide_encode): grid, planes, words 0, 2, 3, 4.
MRT_HD void wide_encode_node(float4 *w, const float nl[3], const float nh[3], const float clo[8][3], const float chi[8][3], const bool occ[8], uint32_t imask) {
    const WideGrid g = wide_grid(nl, nh);
    uint32_t q[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
    for (int sl = 0; sl < 8; sl++) wide_slot_planes(g, nl, sl, occ[sl], clo[sl], chi[sl], q);
    wide_write_node(w, nl, g, imask, q);
}

// Slot assignment: a child prefers the octant of its centre about the node's (2 x centre compared, strictly greater = the upper half) and takes the free slot nearest
// to it by Hamming distance, the lowest such slot; children in their given order.  box_of(k, lo, hi) yields child k's box.
template <class BoxOf>
MRT_HD void wide_assign_slots(const float nl[3], const float nh[3], int nch, BoxOf box_of, int child_in_slot[8]) {
    for (int sl = 0; sl < 8; sl++) child_in_slot[sl] = -1;
    const float cx = nl[0] + nh[0], cy = nl[1] + nh[1], cz = nl[2] + nh[2];
    for (int k = 0; k < nch; k++) {
        float lo[3], hi[3];
        box_of(k, lo, hi);
        const int pref = ((lo[0] + hi[0]) > cx ? 1 : 0) | ((lo[1] + hi[1]) > cy ? 2 : 0) | ((lo[2] + hi[2]) > cz ? 4 : 0);
        int bs = -1, bd = 99;
        for (int sl = 0; sl < 8; sl++) if (child_in_slot[sl] < 0) { const int dd = __builtin_popcount((unsigned)(sl ^ pref)); if (dd < bd) { bd = dd; bs = sl; } }
        child_in_slot[bs] = k;
    }
}

#undef MRT_HD

}  // namespace mrt
