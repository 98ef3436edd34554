// guides.h — first-hit guide buffers (renderer option guides = 1; include/mrt_abi.h MRT_GUIDE_*): per pixel the shading normal and distance,
// the base colour and the ids of the PRIMARY hit, the first two averaged over the frames by the accumulation buffer's rule.  No counterpart in
// the reference (its kernel keeps none of this, Raytracing.metal:249-269); what an edge-avoiding filter needs (denoise.hip).
// Included by renderer.hip inside namespace mrt { namespace { ... } } after shade.h (FrameParams, primary_ray, slot_to_pixel) and traverse_wide.h.
//
// A kernel of its own that RE-TRACES the primary rays: the same ray (seed table, Halton index, camera) walked by the same one-ray-per-lane
// forms k_shade_primary / k_trace_primary use, so t, the barycentrics and the id are the floats the colour path sees — and no existing kernel
// gains a template axis, a register or a store (tests/test_kernel_resources.py keeps its meaning).  One thread per owned pixel takes ALL the
// frames of the render call in frame order with the running average in registers: the buffers are read once and written once per call, and
// the result is the frame-by-frame one for any split of the frames into calls, passes and lanes.  The launch runs on a stream of its own
// beside the pass lanes (Renderer::guide_stream) and is joined into the main stream with them.
//   WALK 0  two-level scene without the 8-wide layout (traverse_instanced)
//   WALK 1  the rope walk (scene option wide = 0)
//   WALK 2  one ray per lane on the 8-wide layout (traverse_wide_lane), the wave's stack in dynamic LDS: wide-tree depth x WIDE_STACK_LEVEL_BYTES
//   WALK 3  two-level scene on the 8-wide layout (traverse_wide_lane_two_level), same stack
// One wave per workgroup, as k_trace_primary: the stack is 320 B per level (4.2 KB at DragonScene's 13 levels), so LDS allows 38 such
// workgroups per CU where the wave slots allow 32 — occupancy is set by registers, not by the stack, up to 15 levels.
#pragma once

template <int WALK>
__global__ void __launch_bounds__(64) k_guides(SceneView s, FrameParams fp, const uint32_t *__restrict__ seeds, uint32_t n_frames,
                                               float4 *__restrict__ g_nd, float4 *__restrict__ g_alb, int4 *__restrict__ g_ids) {
    extern __shared__ uint32_t guide_stk[];
    const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
    int x, y;
    if (!slot_to_pixel(fp, slot, x, y)) return;
    const uint32_t pix = (uint32_t)y * (uint32_t)fp.width + (uint32_t)x;
    const uint32_t frame0 = fp.frameIndex, sample0 = fp.sampleIndex;
    float4 nd = make_float4(0.0f, 0.0f, 0.0f, 0.0f), al = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int4 ids = make_int4(0, -1, -1, -1);
    for (uint32_t f = 0; f < n_frames; f++) {
        fp.sampleIndex = sample0 + f;                       // the seed table's first sub-frame (+ 0) and the frame's own index: the Halton index of the colour path
        f3 org, dir;
        primary_ray(fp, seeds, slot, x, y, org, dir);
        TravHit h;
        bool hit;
        if (WALK == 3) hit = traverse_wide_lane_two_level<false>(s, org, dir, __builtin_inff(), 0xFFFFFFFFu, h, guide_stk);
        else if (WALK == 2) hit = traverse_wide_lane<false>(s, org, dir, __builtin_inff(), 0xFFFFFFFFu, h, guide_stk);
        else if (WALK == 1) hit = traverse<false>(s, org, dir, 0.0f, __builtin_inff(), h);
        else hit = traverse_instanced<false>(s, org, dir, 0.0f, __builtin_inff(), h);
        float4 n_new = make_float4(0.0f, 0.0f, 0.0f, 0.0f), a_new = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        ids = make_int4(0, -1, -1, -1);
        if (hit) {
            // shade_entry's normal (Raytracing.metal:63-72, :267-268) and resource slot (:262-269), expression by expression
            const uint32_t gid = h.gid;
            uint32_t inst = 0, rec = gid, vb = 0;
            if (s.num_inst) { inst = instance_of_gid(s, gid); const InstanceDev &I = s.inst[inst]; rec = I.ts_base + (gid - I.gid_base); vb = I.vbase; }
            const float bu = h.U / h.ad, bv = h.V / h.ad;
            const float bw = 1.0f - bu - bv;
            const uint4 ts = s.tri_shade[rec];
            if (!s.num_inst) inst = ts.w >> 16;
            const uint32_t geom = ts.w & 0xFFFFu;
            const f3 n_obj = (bu * mk3(s.normals[vb + ts.y]) + bv * mk3(s.normals[vb + ts.z])) + bw * mk3(s.normals[vb + ts.x]);
            const f3 c0 = mk3(s.inst_cols[inst * 4 + 0]), c1 = mk3(s.inst_cols[inst * 4 + 1]), c2 = mk3(s.inst_cols[inst * 4 + 2]);
            const f3 n_w = mk3((c0.x * n_obj.x + c1.x * n_obj.y) + c2.x * n_obj.z,
                               (c0.y * n_obj.x + c1.y * n_obj.y) + c2.y * n_obj.z,
                               (c0.z * n_obj.x + c1.z * n_obj.y) + c2.z * n_obj.z);
            const f3 nrm = normalize3(n_w);
            const uint32_t rslot = inst * (uint32_t)s.max_sub + geom;
            const float4 surf = s.base_color[rslot];
            n_new = make_float4(nrm.x, nrm.y, nrm.z, h.t);
            a_new = make_float4(surf.x, surf.y, surf.z, 1.0f);
            ids = make_int4(1, (int)inst, (int)geom, (int)(gid - s.geom_base[rslot]));
        }
        const uint32_t frame = frame0 + f;
        if (frame > 0) {                                    // Raytracing.metal:395-401, per component
            if (f == 0) { nd = q2load(&g_nd[pix]); al = q2load(&g_alb[pix]); }
            const float fi = (float)frame, den = (float)(frame + 1);
            nd = make_float4((n_new.x + nd.x * fi) / den, (n_new.y + nd.y * fi) / den, (n_new.z + nd.z * fi) / den, (n_new.w + nd.w * fi) / den);
            al = make_float4((a_new.x + al.x * fi) / den, (a_new.y + al.y * fi) / den, (a_new.z + al.z * fi) / den, (a_new.w + al.w * fi) / den);
        } else { nd = n_new; al = a_new; }
    }
    q2store(&g_nd[pix], nd); q2store(&g_alb[pix], al);
    g_ids[pix] = ids;
}
