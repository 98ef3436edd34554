// temporal.hip — temporal reprojection of the accumulated image on device buffers, on a stream of the caller's (mrt_context_reproject_device): the step
// that lets a frame composed from the stages keep averaging while the camera or an instance moves.  A translation unit of its own: no traversal, no shading kernel and
// no builder is compiled here, and no kernel reads a scene.  The definition is the comment block of include/mrt_abi.h; tests/temporal_reference.py restates it in numpy,
// op for op, and this file follows it.
//
//   k_reproject <MOVED>  one thread per pixel p = y * width + x.  Reads the pixel's sample (16 B) and the normal | type group of its surface row; a surface also the
//                        position and id groups (48 of the row's 64 bytes; base colour is not used) and, MOVED, its previous position (16 B).  Both points are projected
//                        — the basis terms nx, ny, nz, det of the two by-value cameras are wave-uniform and computed here, with the stated arithmetic — and up to four
//                        taps of the previous frame are gathered in dependency order: ids (16 B), then normal | depth (16 B), then history (16 B), each only if the one
//                        before let the tap through, so a rejected tap costs 16 or 32 bytes and its other words are never loaded, let alone computed with.  One 16-byte
//                        store.  A still world reads one tap: 64 + 16 + 48 + 16 = 144 B per pixel of cache lines touched, 160 with a previous position.
//
// A tap's row and column are tested against the image as floats before they are converted, so no index leaves the buffers whatever the inputs hold (NaN, infinities,
// motion of any size).  No LDS, no atomics, no cross-lane traffic, no scratch.  Arithmetic: float32, one rounding per *, +, - and /, IEEE divide, no square root (the
// file is compiled with -ffp-contract=off like the rest).
#include "temporal.h"
#include "device_math.h"

namespace mrt {
namespace {

constexpr uint32_t TEMPORAL_THREADS = 256;

// A 16-byte entry stays ONE load: left alone, the compiler cuts it along the branches that use its words (the type word now, the normal later; ids.on, then the ids)
// into two or three narrower loads of the same cache line.
MRT_DEV float4 whole(float4 v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); return v; }
MRT_DEV int4 whole(int4 v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); return v; }

struct CameraBasis { f3 pos, nx, ny, nz; float det; };
MRT_DEV CameraBasis camera_basis(const MRTCamera &c) {
    const f3 right = mk3(c.right.x, c.right.y, c.right.z), up = mk3(c.up.x, c.up.y, c.up.z), fwd = mk3(c.forward.x, c.forward.y, c.forward.z);
    CameraBasis b;
    b.pos = mk3(c.position.x, c.position.y, c.position.z);
    b.nx = cross3(up, fwd); b.ny = cross3(fwd, right); b.nz = cross3(right, up);
    b.det = dot3(right, b.nx);
    return b;
}

// scatter_math.h's camera_ray_dir inverted: q = pos + s * ((2 px / w - 1) right + (2 py / h - 1) up + fwd), s > 0
struct Projected { float px, py, d2; bool ok; };
MRT_DEV Projected project(const CameraBasis &b, const f3 q, const float fw, const float fh) {
    const f3 v = q - b.pos;
    const float a = dot3(v, b.nx) / b.det, bb = dot3(v, b.ny) / b.det, c = dot3(v, b.nz) / b.det;
    Projected r;
    r.px = ((a / c + 1.0f) * 0.5f) * fw;
    r.py = ((bb / c + 1.0f) * 0.5f) * fh;
    r.d2 = dot3(v, v);
    r.ok = c > 0.0f && fabsf(r.px) < __builtin_inff() && fabsf(r.py) < __builtin_inff();          // (a NaN fails each comparison)
    return r;
}

template <bool MOVED>
__global__ void __launch_bounds__(TEMPORAL_THREADS) k_reproject(const uint32_t w, const uint32_t h, const MRTCamera cam, const MRTCamera prev_cam, const float4 *__restrict__ rows,
                                                                const float4 *__restrict__ prev_pos, const float4 *__restrict__ prev_nd, const int4 *__restrict__ prev_ids,
                                                                const float4 *__restrict__ prev_hist, const float4 *__restrict__ sample, float4 *__restrict__ out,
                                                                const MRTReprojectParams par) {
    const uint32_t p = blockIdx.x * TEMPORAL_THREADS + threadIdx.x;
    if (p >= w * h) return;                                                            // (w * h is below 2^30)
    const uint32_t y = p / w, x = p - y * w;
    const float4 s = whole(sample[p]);
    const float4 q1 = whole(rows[4 * (size_t)p + 1]);                                  // normal | type
    float4 o = make_float4(s.x, s.y, s.z, 1.0f);
    if (__float_as_int(q1.w) == 1) {
        const float4 q0 = rows[4 * (size_t)p], q3 = rows[4 * (size_t)p + 3];           // position | distance, ids
        const int inst = __float_as_int(q3.x), geom = __float_as_int(q3.y);
        const f3 nrm = mk3(q1), cur = mk3(q0);
        const f3 was = MOVED ? mk3(whole(prev_pos[p])) : cur;
        const float fw = (float)w, fh = (float)h;
        const Projected P1 = project(camera_basis(cam), cur, fw, fh), P0 = project(camera_basis(prev_cam), was, fw, fh);
        if (P1.ok && P0.ok) {
            const float fx = (float)x + (P0.px - P1.px), fy = (float)y + (P0.py - P1.py);
            const float x0 = floorf(fx), y0 = floorf(fy);
            const float ax = fx - x0, ay = fy - y0;
            const float wmax = (float)(w - 1u), hmax = (float)(h - 1u);
            float sw = 0.0f, sl = 0.0f;
            f3 sc = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int t = 0; t < 4; t++) {                                              // (0,0), (1,0), (0,1), (1,1)
                const int i = t & 1, j = t >> 1;
                const float wt = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                const float cx = x0 + (float)i, cy = y0 + (float)j;
                if (wt == 0.0f || !(cx >= 0.0f && cx <= wmax && cy >= 0.0f && cy <= hmax)) continue;          // not read; inside decided in float
                const size_t q = (size_t)(uint32_t)cy * w + (uint32_t)cx;
                const int4 ids = whole(prev_ids[q]);
                if (!(ids.x == 1 && ids.y == inst && ids.z == geom)) continue;            // (the primitive is not compared: a point may cross a triangle edge)
                const float4 nd = whole(prev_nd[q]);
                if (!(dot3(mk3(nd), nrm) >= par.min_cos_normal && fabsf(nd.w * nd.w - P0.d2) <= par.depth_tolerance * P0.d2)) continue;
                const float4 hs = whole(prev_hist[q]);
                const bool valid = hs.w >= 1.0f;                                       // selected, not branched on: the entry is here already
                sw = valid ? sw + wt : sw;
                sc = valid ? sc + mk3(hs) * wt : sc;
                sl = valid ? sl + wt * hs.w : sl;
            }
            if (sw > 0.0f) {
                const float grown = sl / sw + 1.0f;
                const float len = grown < par.max_history ? grown : par.max_history;
                const float keep = len - 1.0f;
                o = make_float4((s.x + (sc.x / sw) * keep) / len, (s.y + (sc.y / sw) * keep) / len, (s.z + (sc.z / sw) * keep) / len, len);
            }
        }
    }
    out[p] = o;
}

}  // namespace

// One launch on `stream`, nothing else.  The arguments were checked by the caller (api.cpp).
int reproject_device(hipStream_t stream, int width, int height, const MRTCamera &camera, const MRTCamera &prev_camera, const void *d_surfaces, const void *d_prev_position,
                     const void *d_prev_normal_depth, const void *d_prev_ids, const void *d_prev_history, const void *d_sample, void *d_out, const MRTReprojectParams &p) {
    const size_t n = (size_t)width * (size_t)height;
    hipLaunchKernelGGL(d_prev_position ? k_reproject<true> : k_reproject<false>, dim3((uint32_t)((n + TEMPORAL_THREADS - 1) / TEMPORAL_THREADS)), dim3(TEMPORAL_THREADS), 0, stream,
                       (uint32_t)width, (uint32_t)height, camera, prev_camera, static_cast<const float4 *>(d_surfaces), static_cast<const float4 *>(d_prev_position),
                       static_cast<const float4 *>(d_prev_normal_depth), static_cast<const int4 *>(d_prev_ids), static_cast<const float4 *>(d_prev_history),
                       static_cast<const float4 *>(d_sample), static_cast<float4 *>(d_out), p);
    MRT_HIP(hipGetLastError());
    return MRT_OK;
}

}  // namespace mrt
