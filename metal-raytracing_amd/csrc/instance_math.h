// instance_math.h — the arithmetic of one instance of a two-level scene, for host and device: its world->object rows and its padded world box.
//
// The host computes them at a commit (two_level.hip update_tlas), the device when an instance moves or its BLAS is refitted on a stream (tlas_refit.hip k_inst_check,
// k_inst_write, k_blas_instance_boxes); both must give the same bits, and both call what is here.  Everything is evaluated in double, in exactly this operation order, and
// rounded to float once; host and device are compiled with -ffp-contract=off (Makefile), so a __host__ __device__ function is the same arithmetic in both passes.  The CPU
// oracle keeps its own, independent restatement of the rows: the two must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace mrt {

#define MRT_HD __host__ __device__ __forceinline__

// min / max by one explicit compare — what std::min / std::max do: the second argument only where it compares strictly beyond the first
template <class T> MRT_HD T h_min(T a, T b) { return b < a ? b : a; }
template <class T> MRT_HD T h_max(T a, T b) { return a < b ? b : a; }
// the float below / above x
MRT_HD float f_below(float x) { return nextafterf(x, -3.0e38f); }
MRT_HD float f_above(float x) { return nextafterf(x, 3.0e38f); }

struct Box { float lo[3], hi[3]; };

// The affine map p -> A p + t is given as a column-major 4x4 (last row 0 0 0 1).  The cofactors of A and its determinant first — the determinant decides whether the matrix
// is taken at all, and k_inst_check needs nothing else —, then the rows of [A^-1 | -A^-1 t].
struct Cofactors { double c[3][3], det; };
MRT_HD Cofactors cofactors_of(const float *xf) {
    const double a00 = xf[0], a10 = xf[1], a20 = xf[2], a01 = xf[4], a11 = xf[5], a21 = xf[6], a02 = xf[8], a12 = xf[9], a22 = xf[10];
    Cofactors k;
    k.c[0][0] = a11 * a22 - a12 * a21; k.c[0][1] = a02 * a21 - a01 * a22; k.c[0][2] = a01 * a12 - a02 * a11;
    k.c[1][0] = a12 * a20 - a10 * a22; k.c[1][1] = a00 * a22 - a02 * a20; k.c[1][2] = a02 * a10 - a00 * a12;
    k.c[2][0] = a10 * a21 - a11 * a20; k.c[2][1] = a01 * a20 - a00 * a21; k.c[2][2] = a00 * a11 - a01 * a10;
    k.det = a00 * k.c[0][0] + a01 * k.c[1][0] + a02 * k.c[2][0];
    return k;
}
MRT_HD bool invertible(double det) { return fabs(det) > 0.0 && __builtin_isfinite(det); }
MRT_HD void rows_of(const float *xf, const Cofactors &k, float rows[3][4]) {
    const double tx = xf[12], ty = xf[13], tz = xf[14];
    for (int r = 0; r < 3; r++) {
        const double i0 = k.c[r][0] / k.det, i1 = k.c[r][1] / k.det, i2 = k.c[r][2] / k.det;
        rows[r][0] = (float)i0; rows[r][1] = (float)i1; rows[r][2] = (float)i2;
        rows[r][3] = (float)(-(i0 * tx + i1 * ty + i2 * tz));
    }
}
// false, and rows untouched: a matrix that is not taken (a determinant of zero, an infinite one, a NaN)
MRT_HD bool invert_affine(const float *xf, float rows[3][4]) {
    const Cofactors k = cofactors_of(xf);
    if (!invertible(k.det)) return false;
    rows_of(xf, k, rows);
    return true;
}

// The corners of the box [lo, hi] through the object->world matrix and, with `mi`, through the exact inverse of the float32 rows too (the map the traversal's object-space
// ray really inverts); then padded like the leaf boxes of bvh_build.hip, four times over (4e-5 |coord| + 4e-6).
__host__ __device__ static inline Box corners_box(const float *xf, const double lo[3], const double hi[3], const double (*mi)[4]) {
    Box b;
    for (int k = 0; k < 3; k++) { b.lo[k] = 3.0e38f; b.hi[k] = -3.0e38f; }
    for (int c = 0; c < 8; c++) {
        const double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
        for (int k = 0; k < 3; k++) {
            const double w = (double)xf[k] * p[0] + (double)xf[4 + k] * p[1] + (double)xf[8 + k] * p[2] + (double)xf[12 + k];
            b.lo[k] = h_min(b.lo[k], (float)w); b.hi[k] = h_max(b.hi[k], (float)w);
            if (mi) {
                const double v = mi[k][0] * p[0] + mi[k][1] * p[1] + mi[k][2] * p[2] + mi[k][3];
                b.lo[k] = h_min(b.lo[k], f_below((float)v)); b.hi[k] = h_max(b.hi[k], f_above((float)v));
            }
        }
    }
    for (int k = 0; k < 3; k++) {
        const float m = h_max(fabsf(b.lo[k]), fabsf(b.hi[k])), e = 4e-5f * m + 4e-6f;
        b.lo[k] -= e; b.hi[k] += e;
    }
    return b;
}

// World box of an instance: the corners of its BLAS root box [lo_in, hi_in] through the matrix, padded (corners_box), plus the rounding of the ray's trip into object space.
// That rounding is bounded per object axis k by delta_k = gamma_4 (sum_j |R_kj| max|X_j| + |w_k|) for the float32 w2o rows (R | w) and world points X in the box: the root
// box is grown by delta before its corners are mapped (an instance translated 1e4 from the origin needs ~5e-3, far more than the relative pad gives).  The bound covers world
// points inside the box; the drift of the object-space DIRECTION, which grows with t and with the distance of the ray origin, is not bounded here.
// X depends on the box delta grows: iterate (a contraction unless cond(R) gamma_4 nears 1: a few rounds, then 10 % to spare).  Its constants: X and delta taken 10 % larger
// than computed, at most eight rounds of the fixed point.
__host__ __device__ static inline Box instance_box(const float *xf, const float lo_in[3], const float hi_in[3], const float rows[3][4]) {
    double lo[3] = {lo_in[0], lo_in[1], lo_in[2]}, hi[3] = {hi_in[0], hi_in[1], hi_in[2]};
    const double g4 = 4.0 * 0x1p-24 / (1.0 - 4.0 * 0x1p-24);
    Box cur = corners_box(xf, lo, hi, nullptr);
    for (int it = 0; it < 8; it++) {
        double X[3];
        for (int j = 0; j < 3; j++) X[j] = 1.1 * h_max(fabs((double)cur.lo[j]), fabs((double)cur.hi[j]));
        double glo[3], ghi[3];
        for (int k = 0; k < 3; k++) {
            const double dk = 1.1 * g4 * (fabs((double)rows[k][0]) * X[0] + fabs((double)rows[k][1]) * X[1] + fabs((double)rows[k][2]) * X[2] + fabs((double)rows[k][3]));
            lo[k] = (double)lo_in[k] - dk; hi[k] = (double)hi_in[k] + dk;
            glo[k] = (double)f_below((float)lo[k]); ghi[k] = (double)f_above((float)hi[k]);
        }
        const Box next = corners_box(xf, glo, ghi, nullptr);
        bool grew = false;
        for (int k = 0; k < 3; k++) grew = grew || next.lo[k] < cur.lo[k] || next.hi[k] > cur.hi[k];
        cur = next;
        if (!grew && it > 0) break;
    }
    double mi[3][4];
    {
        const double a[3][3] = {{rows[0][0], rows[0][1], rows[0][2]}, {rows[1][0], rows[1][1], rows[1][2]}, {rows[2][0], rows[2][1], rows[2][2]}};
        const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++)
            mi[r][c] = (a[(c + 1) % 3][(r + 1) % 3] * a[(c + 2) % 3][(r + 2) % 3] - a[(c + 1) % 3][(r + 2) % 3] * a[(c + 2) % 3][(r + 1) % 3]) / det;
        for (int r = 0; r < 3; r++) mi[r][3] = -(mi[r][0] * rows[0][3] + mi[r][1] * rows[1][3] + mi[r][2] * rows[2][3]);
    }
    return corners_box(xf, lo, hi, mi);
}

#undef MRT_HD

}  // namespace mrt
