"""Host-side mirror of Renderer (Renderer.swift:12-357) over the C ABI.

`Renderer(size, scene)` does what `Renderer.init?(metalView:)` does (device + queue, scene,
targets, buffers, acceleration structures); `draw()` is `draw(in:)` — one frame: uniforms,
dispatch, ping-pong swap.  There is no MTKView: the tonemap pass writes RGBA8 to host memory
instead of a drawable (`tonemapped()`).
"""
import time
import ctypes as C

import numpy as np

from ._ffi import Camera, Light, MRTError, RenderStats, SceneStats, check, lib, ptr
from .scene import DragonScene, Scene


class Context:
    """MTLCreateSystemDefaultDevice + makeCommandQueue (Renderer.swift:46-59)."""

    def __init__(self, device=0):
        self.handle = C.c_void_p()
        check(lib.mrt_context_create(int(device), C.byref(self.handle)))
        self.device = int(device)

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        check(lib.mrt_context_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def set_stream(self, hip_stream):
        check(lib.mrt_context_set_stream(self.handle, C.c_void_p(hip_stream) if hip_stream else None))

    @property
    def stream(self):
        """The hipStream_t handle (an int) the context's work is enqueued on: its own, or the one set_stream gave it."""
        s = C.c_void_p()
        check(lib.mrt_context_get_stream(self.handle, C.byref(s)))
        return s.value or 0

    def close(self):
        if self.handle:
            lib.mrt_context_destroy(self.handle)
            self.handle = C.c_void_p()


class DeviceScene:
    """The committed device-side scene: geometry upload + createAccelerationStructures
    (Renderer.swift:184-214)."""

    def __init__(self, ctx, scene, options=None):
        self.ctx = ctx
        self.handle = C.c_void_p()
        check(lib.mrt_scene_create(ctx.handle, C.byref(self.handle)))
        for k, v in (options or {}).items():
            check(lib.mrt_scene_set_option(self.handle, k.encode(), float(v)))
        from .scene import flatten_scene
        for pos, nrm, xf, subs, source in flatten_scene(scene, share=True):
            mid = C.c_int32()
            if source >= 0:                                   # same geometry as an earlier mesh: an instance of it
                check(lib.mrt_scene_add_instance(self.handle, source, ptr(xf), C.byref(mid)))
                continue
            pos = np.ascontiguousarray(pos, np.float32)
            nrm = np.ascontiguousarray(nrm, np.float32)
            check(lib.mrt_scene_add_mesh(self.handle, ptr(pos), 12, ptr(nrm), 12, pos.shape[0], ptr(xf), C.byref(mid)))
            for idx, mat in subs:
                idx = np.ascontiguousarray(idx, np.uint32)
                check(lib.mrt_mesh_add_submesh(self.handle, mid.value, ptr(idx), idx.shape[0], C.byref(mat), None))
        self.set_lights(scene.lights)
        t0 = time.perf_counter()
        check(lib.mrt_scene_commit(self.handle))
        self.commit_wall_ms = (time.perf_counter() - t0) * 1e3      # host wall time of the commit (uploads, build, validation); stats.build_ms is the device time of the build alone

    def set_instance_transform(self, mesh_id, transform):
        """Animated transforms: new object->world matrix for one instance; call commit() afterwards."""
        xf = np.ascontiguousarray(np.asarray(transform, np.float32).reshape(16))
        check(lib.mrt_scene_set_instance_transform(self.handle, int(mesh_id), ptr(xf)))

    def update_mesh(self, mesh_id, positions, normals):
        """Deforming geometry: new object-space positions / normals of one mesh's vertices (same count); call commit() afterwards — a flattened scene refits its tree."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3); nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm.shape[0] != pos.shape[0]:          # the C side reads vertex_count normals: a shorter array would be read past its end
            raise MRTError(1, f"update_mesh: {nrm.shape[0]} normals for {pos.shape[0]} positions (one normal per vertex)")
        check(lib.mrt_scene_update_mesh(self.handle, int(mesh_id), ptr(pos), 12, ptr(nrm), 12, pos.shape[0]))

    def set_mesh_masks(self, masks, first_mesh_id=0):
        """Visibility masks of the mesh ids first_mesh_id .. (the ids Intersection.instance_id reports; an instance has its own): 32-bit integers, 0xFFFFFFFF until set.  A ray
        with mask r (mask= of the intersect_*_device methods) sees the triangles of mesh m iff masks[m] & r.  Takes effect at once on a committed scene (it blocks, as a commit
        does) and needs no commit: the tree does not depend on masks, and nothing is built or refitted.  Masks survive every commit, update and refit.  DRAWS IGNORE MASKS: a
        Renderer traces every mesh; an integrator composed from the query and stage methods honours masks by passing mask= to its query calls."""
        m = np.asarray(masks)
        if m.ndim != 1 or m.dtype.kind not in "iu" or (m.size and (int(m.min()) < 0 or int(m.max()) > 0xFFFFFFFF)):
            raise ValueError("masks must be a 1-D sequence of integers 0 .. 0xFFFFFFFF")
        m = np.ascontiguousarray(m, np.uint32)
        check(lib.mrt_scene_set_mesh_masks(self.handle, int(first_mesh_id), m.shape[0], ptr(m)))

    def mesh_masks(self):
        """the visibility mask of every mesh id of the COMMITTED scene, numpy uint32 (meshes,): the count is the last commit's (stats.instances), so a mesh added through the C ABI
        since then appears after the next commit (set_mesh_masks can address it before)"""
        m = np.zeros(int(self.stats.instances), np.uint32)
        check(lib.mrt_scene_get_mesh_masks(self.handle, 0, m.shape[0], ptr(m)))
        return m

    @property
    def refits(self):
        v = C.c_uint32()
        check(lib.mrt_debug_scene_refits(self.handle, C.byref(v)))
        return v.value

    def commit(self):
        check(lib.mrt_scene_commit(self.handle))

    def set_lights(self, lights):
        arr = (Light * max(1, len(lights)))(*lights)
        check(lib.mrt_scene_set_lights(self.handle, arr, len(lights)))

    @property
    def stats(self):
        s = SceneStats()
        check(lib.mrt_scene_stats(self.handle, C.byref(s)))
        return s

    def intersect_closest(self, rays):
        """rays: (n, 8) float32 [ox,oy,oz,tmin,dx,dy,dz,tmax] → structured array of Intersection."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=INTERSECTION_DTYPE)
        check(lib.mrt_scene_intersect_closest(self.handle, ptr(rays), rays.shape[0], ptr(out)))
        return out

    def intersect_any(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=np.int32)
        check(lib.mrt_scene_intersect_any(self.handle, ptr(rays), rays.shape[0], ptr(out)))
        return out

    def intersect_stream(self, rays, any_hit=False):
        """The render kernels' traversal (8-wide stream, both levels of an instanced scene) on caller rays; min_distance must be 0."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=INTERSECTION_DTYPE)
        check(lib.mrt_debug_intersect_stream(self.handle, ptr(rays), rays.shape[0], 1 if any_hit else 0, ptr(out)))
        return out

    def _count_word(self, count, what="count"):
        """the count= argument of the *_device methods — a one-element torch.int32 or torch.uint32 tensor on the context's device — as a pointer; it is never read here"""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        kinds = tuple(k for k in (torch.int32, getattr(torch, "uint32", None)) if k is not None)
        if not isinstance(count, torch.Tensor) or count.device != dev or count.dtype not in kinds or count.numel() != 1:
            raise ValueError(f"{what} must be a torch.int32 or torch.uint32 tensor with one element on {dev}")
        return C.c_void_p(count.data_ptr())

    def _mask_args(self, mask, n):
        """the mask= argument of the three query methods as (d_ray_masks, ray_mask): a Python int is the mask of every ray; a contiguous torch.int32 / uint32 (n,) tensor on the
        context's device holds one mask per ray.  Anything else is a ValueError, before the library is called."""
        import torch
        if isinstance(mask, int) and not isinstance(mask, bool):
            if not 0 <= mask <= 0xFFFFFFFF:
                raise ValueError("mask must fit 32 bits: 0 .. 0xFFFFFFFF")
            return C.c_void_p(None), mask
        dev = torch.device("cuda", self.ctx.device)
        kinds = tuple(k for k in (torch.int32, getattr(torch, "uint32", None)) if k is not None)
        if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in kinds or tuple(mask.shape) != (n,) or not mask.is_contiguous():
            raise ValueError(f"mask must be None, an int, or a contiguous torch.int32 / torch.uint32 tensor of shape ({n},) on {dev}: one mask per ray")
        return C.c_void_p(mask.data_ptr() if n else None), 0

    def _device_query(self, fn, rays, out, stream, out_shape, count=None, mask=None, masked_fn=None):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(rays, torch.Tensor) or rays.device != dev:
            raise ValueError(f"rays must be a torch tensor on {dev}")
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous torch.float32 tensor of shape (n, 8): [ox, oy, oz, tmin, dx, dy, dz, tmax]")
        shape = (rays.shape[0], *out_shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.int32 tensor of shape {shape} on {dev}")
        n = rays.shape[0]
        if mask is not None:
            masks, word = self._mask_args(mask, n)
            check(masked_fn(self.handle, C.c_void_p(rays.data_ptr() if n else None), masks, word, n, C.c_void_p(out.data_ptr() if n else None), C.c_void_p(self._stream_handle(stream)),
                            None if count is None else self._count_word(count)))
            return out
        more = () if count is None else (self._count_word(count),)
        check(fn(self.handle, C.c_void_p(rays.data_ptr() if n else None), n, C.c_void_p(out.data_ptr() if n else None), C.c_void_p(self._stream_handle(stream)), *more))
        return out

    def intersect_closest_device(self, rays, out=None, stream=None, count=None, mask=None):
        """Closest hits of rays that live on the GPU, ordered on a stream: rays is a contiguous torch.float32 (n, 8) tensor on the context's device
        ([ox, oy, oz, tmin, dx, dy, dz, tmax]); returns torch.int32 (n, 8), one MRTIntersection per row (unpack_intersections gives the fields).  Nothing is
        allocated (but `out` when it is None), copied or synchronised.  stream: None = torch's current stream of that device; an integer handle (0 = the
        null stream) or a torch.cuda.Stream.  Keep rays and out alive until the stream has passed the call.
        count: None, or a one-element torch.int32 / uint32 tensor on that device — the length of the queue the rows hold, as compact_rows_device leaves it.  The rows
        below min(n, count) are handled exactly as without it; no row from there on is read or written.  The word is read on the GPU when the kernels start, never here
        (this holds for count= of every *_device method).
        mask: None — this call, every mesh visible — or which geometry the rays may see (set_mesh_masks): an int is the mask of every ray, a contiguous torch.int32 / uint32
        (n,) tensor on that device one mask per ray.  A triangle of mesh m is visible to a ray with mask r iff mesh_masks()[m] & r; the record is the one this method returns
        on a scene that holds the visible meshes only, with this scene's ids.  One ray per lane, one launch (mrt_scene_intersect_closest_masked_device; this holds for
        mask= of intersect_any_device and intersect_all_device too)."""
        return self._device_query(lib.mrt_scene_intersect_closest_device if count is None else lib.mrt_scene_intersect_closest_device_counted, rays, out, stream, (8,), count,
                                  mask, lib.mrt_scene_intersect_closest_masked_device)

    def intersect_any_device(self, rays, out=None, stream=None, count=None, mask=None):
        """Any-hit form of intersect_closest_device: torch.int32 (n,), 1 = occluded (mask: by a triangle the ray may see)."""
        return self._device_query(lib.mrt_scene_intersect_any_device if count is None else lib.mrt_scene_intersect_any_device_counted, rays, out, stream, (), count,
                                  mask, lib.mrt_scene_intersect_any_masked_device)

    def intersect_all_device(self, rays, max_hits, out=None, counts_out=None, stream=None, count=None, mask=None):
        """ALL hits of rays that live on the GPU, in order and ordered on a stream: rays as intersect_closest_device takes them, max_hits 1 .. 16 -> (hits, hit_counts):
        hits torch.int32 (n, max_hits, 8), per ray the max_hits smallest hits under (distance, triangle id), ascending, each triangle once, then miss records (every record
        of a row is written); hit_counts torch.int32 (n,), the number of hit records, 0 .. max_hits.  Row [i, 0] has the bits of intersect_closest_device, and
        hit_counts > 0 is intersect_any_device.  Truncation is not reported: ask for one more than needed to learn whether there are more.  Flattened scenes in every
        layout; a two-level scene raises MRTError (unsupported).  Nothing is allocated (but the outputs that are None), copied or synchronised.  stream, count: as
        intersect_closest_device takes them; rows at and past count are touched in neither output.  mask: as intersect_closest_device takes it — an invisible triangle
        takes no slot of the list.
        What follows: resolve_hits_device(rays.repeat_interleave(max_hits, 0), hits.view(-1, 8)) gives one MRTSurface per record (miss rows for the padding), whose
        resource_slot column leads to the slot's material — the product of its `dissolve` over a shadow ray's records is what the ray lets through."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(rays, torch.Tensor) or rays.device != dev:
            raise ValueError(f"rays must be a torch tensor on {dev}")
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous():
            raise ValueError("rays must be a contiguous torch.float32 tensor of shape (n, 8): [ox, oy, oz, tmin, dx, dy, dz, tmax]")
        if isinstance(max_hits, bool) or not isinstance(max_hits, int) or not 1 <= max_hits <= 16:
            raise ValueError("max_hits must be an integer 1 .. 16")
        n = rays.shape[0]
        outs = []
        for what, t, shape in (("out", out, (n, max_hits, 8)), ("counts_out", counts_out, (n,))):
            if t is None:
                t = torch.empty(shape, dtype=torch.int32, device=dev)
            elif not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous torch.int32 tensor of shape {shape} on {dev}")
            outs.append(t)
        if mask is not None:
            masks, word = self._mask_args(mask, n)
            check(lib.mrt_scene_intersect_all_masked_device(self.handle, C.c_void_p(rays.data_ptr() if n else None), masks, word, n, max_hits, C.c_void_p(outs[0].data_ptr() if n else None),
                                                            C.c_void_p(outs[1].data_ptr() if n else None), C.c_void_p(self._stream_handle(stream)),
                                                            None if count is None else self._count_word(count)))
            return outs[0], outs[1]
        fn, more = (lib.mrt_scene_intersect_all_device, ()) if count is None else (lib.mrt_scene_intersect_all_device_counted, (self._count_word(count),))
        check(fn(self.handle, C.c_void_p(rays.data_ptr() if n else None), n, max_hits, C.c_void_p(outs[0].data_ptr() if n else None), C.c_void_p(outs[1].data_ptr() if n else None),
                 C.c_void_p(self._stream_handle(stream)), *more))
        return outs[0], outs[1]

    def _hit_records(self, hits, what="hits"):
        """the (n, 8) torch.int32 tensor of MRTIntersection records intersect_closest_device returns, checked"""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(hits, torch.Tensor) or hits.device != dev:
            raise ValueError(f"{what} must be a torch tensor on {dev}")
        if hits.dtype != torch.int32 or hits.dim() != 2 or hits.shape[1] != 8 or not hits.is_contiguous():
            raise ValueError(f"{what} must be a contiguous torch.int32 tensor of shape (n, 8): the records of intersect_closest_device")
        return dev

    def resolve_hits_device(self, rays, hits, out=None, stream=None, count=None):
        """The step after intersect_closest_device, on the GPU and ordered on a stream: rays (n, 8) float32 and hits (n, 8) int32 as that method takes and returns them ->
        torch.float32 (n, 16), one MRTSurface per row: position | distance, shading normal | type, base colour | resource slot, instance / geometry / primitive ids
        (unpack_surfaces gives the fields).  The values are the ones the device holds now: vertices written by update_mesh_device / update_blas_device, poses written by
        set_instance_transforms_device.  A miss, and a record whose ids name nothing in the scene, gives the miss record.  After the first call (which makes a small
        table) nothing is allocated (but `out` when it is None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = self._hit_records(hits)
        if not isinstance(rays, torch.Tensor) or rays.device != dev:
            raise ValueError(f"rays must be a torch tensor on {dev}")
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous() or rays.shape[0] != hits.shape[0]:
            raise ValueError("rays must be a contiguous torch.float32 tensor of shape (n, 8), one row per hit record")
        n = rays.shape[0]
        if out is None:
            out = torch.empty((n, 16), dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (n, 16) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous torch.float32 tensor of shape {(n, 16)} on {dev}")
        fn, more = (lib.mrt_scene_resolve_hits_device, ()) if count is None else (lib.mrt_scene_resolve_hits_device_counted, (self._count_word(count),))
        check(fn(self.handle, C.c_void_p(rays.data_ptr() if n else None), C.c_void_p(hits.data_ptr() if n else None), n,
                 C.c_void_p(out.data_ptr() if n else None), C.c_void_p(self._stream_handle(stream)), *more))
        return out

    def interpolate_device(self, hits, attributes, out=None, stream=None, count=None):
        """Per-vertex data of the caller's interpolated at the hits, on the GPU and ordered on a stream: attributes is a torch.float32 (V, C) tensor on the context's
        device, 1 <= C <= 64, rows contiguous and any multiple of 4 bytes apart (a slice of a wider tensor is fine; nothing is copied), one row per vertex in the
        numbering vertex_offsets() describes -> torch.float32 (n, C): (u * a1 + v * a2) + ((1 - u) - v) * a0 over the hit triangle's vertices, zeros for a miss.
        out: an (n, C) float32 tensor with the same freedom of row stride; the elements between its rows are left alone.  stream: as intersect_closest_device takes it."""
        import torch
        dev = self._hit_records(hits)
        a = attributes
        if not isinstance(a, torch.Tensor) or a.device != dev:
            raise ValueError(f"attributes must be a torch tensor on {dev}")
        if a.dtype != torch.float32 or a.dim() != 2 or not 1 <= a.shape[1] <= 64 or a.stride(1) != 1 or (a.shape[0] > 1 and a.stride(0) < a.shape[1]):
            raise ValueError("attributes must be a torch.float32 tensor of shape (V, C), 1 <= C <= 64, with contiguous rows (a slice of a wider tensor is fine)")
        total = int(self.vertex_offsets()[-1])
        if a.shape[0] != total:          # the device reads a row per vertex of the scene: a shorter tensor would be read past its end
            raise MRTError(1, f"interpolate_device: {a.shape[0]} attribute rows for the scene's {total} vertices (vertex_offsets()[-1])")
        n, ch = hits.shape[0], a.shape[1]
        if out is None:
            out = torch.empty((n, ch), dtype=torch.float32, device=dev)
        elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (n, ch) or out.stride(1) != 1
              or (n > 1 and out.stride(0) < ch)):
            raise ValueError(f"out must be a torch.float32 tensor of shape {(n, ch)} on {dev} with contiguous rows")
        fn, more = (lib.mrt_scene_interpolate_device, ()) if count is None else (lib.mrt_scene_interpolate_device_counted, (self._count_word(count),))
        check(fn(self.handle, C.c_void_p(hits.data_ptr() if n else None), n, C.c_void_p(a.data_ptr() if n else None),
                 (a.stride(0) if a.shape[0] > 1 else ch) * 4, ch, C.c_void_p(out.data_ptr() if n else None), (out.stride(0) if n > 1 else ch) * 4,
                 C.c_void_p(self._stream_handle(stream)), *more))
        return out

    def scatter_device(self, surfaces, halton_index, bounce, light_count=0, next_rays=True, out=None, stream=None, count=None):
        """What follows a surface in the reference's kernel (its diffuse path; the materials extension is scatter_materials_device), on the GPU and ordered on a stream: surfaces
        (n, 16) float32 as resolve_hits_device returns them, halton_index (n,) int32 as Renderer.primary_rays_device returns it, bounce the path depth of these surfaces
        (0 .. 18), light_count Uniforms.lightCount (0 = every light of the scene) -> (shadow_rays (n, 8) float32, light (n, 4) float32, next_rays (n, 8) float32 or
        None).  Row i in gives row i out: light[i] = the picked light's colour at the surface | 1.0 where the reference traces a shadow ray (else 0.0),
        shadow_rays[i] that ray (zeros where it is not wanted), next_rays[i] the cosine-weighted bounce ray; a row that is no surface (type != 1) gives zeros
        everywhere — go by light[:, 3] and the surface's type, never by what a query answers for a zero ray.  next_rays=False (the last bounce) computes and writes
        no third buffer.  out: the tuple of tensors to write, (shadow_rays, light, next_rays) or (shadow_rays, light).  Nothing is allocated (but the outputs when
        out is None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(surfaces, torch.Tensor) or surfaces.device != dev or surfaces.dtype != torch.float32 or surfaces.dim() != 2 or surfaces.shape[1] != 16 or not surfaces.is_contiguous():
            raise ValueError(f"surfaces must be a contiguous torch.float32 tensor of shape (n, 16) on {dev}: the records of resolve_hits_device")
        n = surfaces.shape[0]
        h = halton_index
        if not isinstance(h, torch.Tensor) or h.device != dev or h.dtype != torch.int32 or tuple(h.shape) != (n,) or not h.is_contiguous():
            raise ValueError(f"halton_index must be a contiguous torch.int32 tensor of shape {(n,)} on {dev}")
        shapes = [(n, 8), (n, 4)] + ([(n, 8)] if next_rays else [])
        if out is None:
            out = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes)
        else:
            out = tuple(out)
            if len(out) != len(shapes) or any(not isinstance(o, torch.Tensor) or o.device != dev or o.dtype != torch.float32 or tuple(o.shape) != sh or not o.is_contiguous() for o, sh in zip(out, shapes)):
                raise ValueError(f"out must be {len(shapes)} contiguous torch.float32 tensors of shapes {shapes} on {dev}")
        p = [C.c_void_p(t.data_ptr() if n else None) for t in (surfaces, h) + out]
        fn, more = (lib.mrt_scene_scatter_device, ()) if count is None else (lib.mrt_scene_scatter_device_counted, (self._count_word(count),))
        check(fn(self.handle, p[0], p[1], n, int(bounce), int(light_count), p[2], p[3], p[4] if next_rays else None, C.c_void_p(self._stream_handle(stream)), *more))
        return (out[0], out[1], out[2] if next_rays else None)

    def scatter_materials_device(self, rays, surfaces, halton_index, bounce, max_bounces, light_count=0, next_rays=True, out=None, stream=None, count=None):
        """scatter_device with the materials extension on — what follows a surface when Renderer's option materials = 1 — on the GPU and ordered on a stream: rays (n, 8)
        float32, the rays that hit these surfaces (their direction is read); surfaces, halton_index, light_count as scatter_device takes them; max_bounces the path
        length of the integrator (1 .. 16) and 0 <= bounce < max_bounces: the lobe choice reads Halton dimension 2 + 5 * max_bounces + bounce -> (shadow_rays (n, 8),
        light (n, 4), next_rays (n, 8) or None, lobes (n, 8)), all float32.  lobes[i] = weight | lobe code (int32 bits), the material's emission | 0 (unpack_lobes gives
        the fields): lobe 0 = no surface, 1 = diffuse, 2 / 3 = dielectric interface reflected / refracted, 4 = specular, 5 = specular sampled below the surface
        (absorbed).  The material is the scene's at the row's resource slot, but the albedo is the row's base colour (a caller may substitute their own); a slot outside
        the scene's table makes the row no surface.  Diffuse rows get shadow_rays, light and next_rays exactly as scatter_device writes them; the other lobes make no
        next-event estimate (zeros there) and continue along their own ray; absorbed rows and rows that are no surface give zero rays.  A frame is, per bounce:
        radiance += throughput * emission; throughput *= weight; radiance += light[:, :3] * throughput where light[:, 3] == 1 and the shadow ray got through; the
        path goes on where lobe is 1 .. 4 — Renderer's image with materials = 1, bit for bit.  next_rays=False computes and writes no third buffer.  out: the tuple of
        tensors to write, (shadow_rays, light, next_rays, lobes) or (shadow_rays, light, lobes).  Nothing is allocated (but the outputs when out is None), copied or
        synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(surfaces, torch.Tensor) or surfaces.device != dev or surfaces.dtype != torch.float32 or surfaces.dim() != 2 or surfaces.shape[1] != 16 or not surfaces.is_contiguous():
            raise ValueError(f"surfaces must be a contiguous torch.float32 tensor of shape (n, 16) on {dev}: the records of resolve_hits_device")
        n = surfaces.shape[0]
        if not isinstance(rays, torch.Tensor) or rays.device != dev or rays.dtype != torch.float32 or tuple(rays.shape) != (n, 8) or not rays.is_contiguous():
            raise ValueError(f"rays must be a contiguous torch.float32 tensor of shape {(n, 8)} on {dev}: the rays that hit the surfaces")
        h = halton_index
        if not isinstance(h, torch.Tensor) or h.device != dev or h.dtype != torch.int32 or tuple(h.shape) != (n,) or not h.is_contiguous():
            raise ValueError(f"halton_index must be a contiguous torch.int32 tensor of shape {(n,)} on {dev}")
        shapes = [(n, 8), (n, 4)] + ([(n, 8)] if next_rays else []) + [(n, 8)]
        if out is None:
            out = tuple(torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes)
        else:
            out = tuple(out)
            if len(out) != len(shapes) or any(not isinstance(o, torch.Tensor) or o.device != dev or o.dtype != torch.float32 or tuple(o.shape) != sh or not o.is_contiguous() for o, sh in zip(out, shapes)):
                raise ValueError(f"out must be {len(shapes)} contiguous torch.float32 tensors of shapes {shapes} on {dev}")
        p = [C.c_void_p(t.data_ptr() if n else None) for t in (rays, surfaces, h) + out]
        fn, more = (lib.mrt_scene_scatter_materials_device, ()) if count is None else (lib.mrt_scene_scatter_materials_device_counted, (self._count_word(count),))
        check(fn(self.handle, p[0], p[1], p[2], n, int(bounce), int(max_bounces), int(light_count), p[3], p[4], p[5] if next_rays else None, p[-1],
                 C.c_void_p(self._stream_handle(stream)), *more))
        return (out[0], out[1], out[2] if next_rays else None, out[-1])

    def compact_rows_device(self, keep, columns, count=None, out=None, workspace=None, stream=None):
        """A queue made of the rows that go on, on the GPU and ordered on a stream: keep is a torch.bool or torch.uint8 tensor of shape (n,), columns a sequence of at most
        eight contiguous tensors with n rows each (a row — everything behind the first dimension — is a multiple of 4 bytes, at most 64) -> (outs, count_out).  With
        m = min(n, count) (n when count is None), outs[c][j] is columns[c]'s j-th row among the rows i < m with keep[i] set, in their order — what
        columns[c][:m][keep[:m]] gives — and count_out, a one-element torch.int32 tensor, is their number: hand it to the next stage as count=.  The rows of outs from
        count_out on keep what they held.  out: the tensors to write (shapes and dtypes of columns; none may be one of them), allocated when None; workspace: a torch.uint8
        tensor of at least compact_workspace_bytes(n) bytes, allocated when None; count: as every *_device method takes it.  Neither count is read on the host: nothing
        is copied or synchronised, and with out and workspace given nothing is allocated but the four bytes of count_out.  stream: as intersect_closest_device takes it."""
        import torch
        from ._ffi import RowColumn
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(keep, torch.Tensor) or keep.device != dev or keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1 or not keep.is_contiguous():
            raise ValueError(f"keep must be a contiguous torch.bool or torch.uint8 tensor of shape (n,) on {dev}")
        n = keep.shape[0]
        columns = list(columns)
        if len(columns) > 8:
            raise ValueError("at most eight columns")
        for c in columns:
            if not isinstance(c, torch.Tensor) or c.device != dev or c.dim() < 1 or c.shape[0] != n or not c.is_contiguous():
                raise ValueError(f"every column must be a contiguous torch tensor on {dev} with {n} rows")
        if out is None:
            out = [torch.empty_like(c) for c in columns]
        else:
            out = list(out)
            if len(out) != len(columns) or any(not isinstance(o, torch.Tensor) or o.device != dev or o.dtype != c.dtype or o.shape != c.shape or not o.is_contiguous() for o, c in zip(out, columns)):
                raise ValueError("out must hold one contiguous tensor per column, of that column's shape and dtype")
        need = int(lib.mrt_compact_workspace_bytes(n))
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise ValueError(f"workspace must be a contiguous torch.uint8 tensor on {dev} (compact_workspace_bytes(n) bytes)")
        table = (RowColumn * max(1, len(columns)))()
        for k, (c, o) in enumerate(zip(columns, out)):
            table[k].src, table[k].dst = c.data_ptr() if n else None, o.data_ptr() if n else None
            table[k].row_bytes = int(np.prod(c.shape[1:], dtype=np.int64)) * c.element_size()          # (the library refuses what is no multiple of 4 in 4 .. 64)
        count_out = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.mrt_context_compact_rows_device(self.ctx.handle, C.c_void_p(keep.data_ptr() if n else None), n, None if count is None else self._count_word(count), table, len(columns),
                                                  C.c_void_p(count_out.data_ptr()), C.c_void_p(workspace.data_ptr() if workspace.numel() else None), workspace.numel(),
                                                  C.c_void_p(self._stream_handle(stream))))
        return out, count_out

    @staticmethod
    def compact_workspace_bytes(n):
        """bytes of workspace compact_rows_device needs for n rows (never 0; it does not decrease with n)"""
        return int(lib.mrt_compact_workspace_bytes(int(n)))

    def _rows(self, t, what, dtype, shape):
        """a contiguous torch tensor of that dtype and shape on the context's device, checked (shape: a tuple, None for any number of rows) -> the tensor"""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype not in dtypes or t.dim() != len(shape) or not t.is_contiguous()
                or any(s is not None and s != have for s, have in zip(shape, t.shape))):
            names = " or ".join(str(d) for d in dtypes)
            raise ValueError(f"{what} must be a contiguous {names} tensor of shape {tuple('n' if s is None else s for s in shape)} on {dev}")
        return t

    @staticmethod
    def _index_kinds():
        import torch
        return tuple(k for k in (torch.int32, getattr(torch, "uint32", None)) if k is not None)

    def reset_paths_device(self, n, radiance=True, out=None, stream=None):
        """The path state before bounce 0, on the GPU and ordered on a stream -> (throughput (n, 4) float32 of ones, pixel (n,) int32 = 0 .. n - 1, radiance (n, 4)
        float32 of zeros or None).  radiance=False writes (and returns) no image.  out: the tuple of tensors to write, (throughput, pixel, radiance) or (throughput, pixel);
        a radiance tensor given there may have any number of rows (the image's pixels).  Nothing is allocated (but the outputs when out is None), copied or synchronised.
        stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        n = int(n)
        if out is None:
            out = (torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)) + ((torch.empty((n, 4), dtype=torch.float32, device=dev),) if radiance else ())
        out = tuple(out)
        if len(out) != (3 if radiance else 2):
            raise ValueError(f"out must hold {3 if radiance else 2} tensors: throughput, pixel" + (", radiance" if radiance else ""))
        thr = self._rows(out[0], "out[0] (throughput)", torch.float32, (n, 4))
        pix = self._rows(out[1], "out[1] (pixel)", self._index_kinds(), (n,))
        rad = self._rows(out[2], "out[2] (radiance)", torch.float32, (None, 4)) if radiance else None
        npix = rad.shape[0] if radiance else 0
        check(lib.mrt_context_reset_paths_device(self.ctx.handle, n, C.c_void_p(thr.data_ptr() if n else None), C.c_void_p(pix.data_ptr() if n else None),
                                                 C.c_void_p(rad.data_ptr() if npix else None), npix, C.c_void_p(self._stream_handle(stream))))
        return thr, pix, rad

    def advance_paths_device(self, light, throughput, pixel=None, radiance=None, surfaces=None, lobes=None, count=None, keep_path=True, out=None, stream=None):
        """The step after scatter, on the GPU and ordered on a stream: the throughput updated in place, emission deposited, the keep masks of the bounce's two
        compactions written -> (keep_shadow, keep_path), torch.uint8 (n,) holding 0 or 1 (keep_path None with keep_path=False, the last bounce).  Exactly one of surfaces
        and lobes.  surfaces (n, 16) float32, the rows of resolve_hits_device — the diffuse form: throughput.rgb *= base_color; keep_path = type == 1; keep_shadow =
        keep_path and light[:, 3] == 1.  lobes (n, 8) float32, the rows of scatter_materials_device — the materials form, which needs pixel (n,) int32 and radiance
        (pixels, 4) float32: radiance[pixel].rgb += throughput.rgb * emission where lobe != 0, with the throughput before its update; throughput.rgb *= weight; keep_path =
        1 <= lobe <= 4; keep_shadow = light[:, 3] == 1.  A pixel may occur at most once among the rows in use; a row whose pixel is outside the image deposits nothing.
        count: as every *_device method takes it — rows from min(n, count) on are neither read nor written, masks included.  out: the masks to write, (keep_shadow,
        keep_path) or (keep_shadow,).  Nothing is allocated (but the masks when out is None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if (surfaces is None) == (lobes is None):
            raise ValueError("exactly one of surfaces (the diffuse form) and lobes (the materials form) must be given")
        light = self._rows(light, "light", torch.float32, (None, 4))
        n = light.shape[0]
        thr = self._rows(throughput, "throughput", torch.float32, (n, 4))
        if surfaces is not None: self._rows(surfaces, "surfaces", torch.float32, (n, 16))
        else: self._rows(lobes, "lobes", torch.float32, (n, 8))
        if lobes is not None and (pixel is None or radiance is None):
            raise ValueError("the materials form needs pixel and radiance: it deposits emission")
        if pixel is not None: self._rows(pixel, "pixel", self._index_kinds(), (n,))
        if radiance is not None: self._rows(radiance, "radiance", torch.float32, (None, 4))
        npix = 0 if radiance is None else radiance.shape[0]
        want = 2 if keep_path else 1
        if out is None:
            out = tuple(torch.empty((n,), dtype=torch.uint8, device=dev) for _ in range(want))
        out = tuple(out)
        if len(out) != want:
            raise ValueError(f"out must hold {want} torch.uint8 tensors of shape {(n,)}")
        for k, o in enumerate(out): self._rows(o, f"out[{k}]", torch.uint8, (n,))

        def p(t, live=n):
            return C.c_void_p(t.data_ptr() if t is not None and live else None)

        check(lib.mrt_context_advance_paths_device(self.ctx.handle, n, None if count is None else self._count_word(count), p(surfaces), p(lobes), p(light), p(thr), p(pixel),
                                                   p(radiance, n and npix), npix, p(out[0]), p(out[1]) if keep_path else None, C.c_void_p(self._stream_handle(stream))))
        return out[0], (out[1] if keep_path else None)

    def deposit_light_device(self, occluded, light, throughput, pixel, radiance, count=None, stream=None):
        """The step after intersect_any_device on the compacted shadow queue, on the GPU and ordered on a stream: radiance[pixel].rgb += light.rgb * throughput.rgb for
        the rows in use with occluded == 0.  occluded (n,) int32, light and throughput (n, 4) float32, pixel (n,) int32, radiance (pixels, 4) float32 (its fourth
        component keeps its bits).  A pixel may occur at most once among the rows in use (plain load, add, store: no atomics); a row whose pixel is outside the image
        deposits nothing.  count: as every *_device method takes it.  Nothing is allocated, copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        occ = self._rows(occluded, "occluded", torch.int32, (None,))
        n = occ.shape[0]
        self._rows(light, "light", torch.float32, (n, 4)); self._rows(throughput, "throughput", torch.float32, (n, 4))
        self._rows(pixel, "pixel", self._index_kinds(), (n,)); self._rows(radiance, "radiance", torch.float32, (None, 4))
        npix = radiance.shape[0]
        if n and not npix:
            return                                                                                     # an image without pixels: no row can deposit
        p = [C.c_void_p(t.data_ptr() if n else None) for t in (occ, light, throughput, pixel, radiance)]
        check(lib.mrt_context_deposit_light_device(self.ctx.handle, n, None if count is None else self._count_word(count), *p, npix, C.c_void_p(self._stream_handle(stream))))

    def fold_sample_device(self, sample, accum, frame_index, clear_sample=False, stream=None):
        """The reference's running average on the GPU, ordered on a stream: sample and accum (pixels, 4) float32; frame_index 0: accum.rgb = sample.rgb, otherwise
        accum.rgb = (sample.rgb + accum.rgb * frame_index) / (frame_index + 1); accum[:, 3] = 1.  clear_sample=True leaves sample as zeros for the next frame, in the same
        pass.  accum is what Renderer.write_accum_from(accum.data_ptr(), nbytes) takes.  Nothing is allocated, copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        s = self._rows(sample, "sample", torch.float32, (None, 4))
        npix = s.shape[0]
        a = self._rows(accum, "accum", torch.float32, (npix, 4))
        frame_index = int(frame_index)
        if not 0 <= frame_index < 2 ** 32 - 1:
            raise ValueError("frame_index must be in [0, 2^32 - 1)")
        check(lib.mrt_context_fold_sample_device(self.ctx.handle, npix, C.c_void_p(s.data_ptr() if npix else None), C.c_void_p(a.data_ptr() if npix else None), frame_index,
                                                 1 if clear_sample else 0, C.c_void_p(self._stream_handle(stream))))

    def fold_guides_device(self, surfaces, frame_index, out=None, stream=None):
        """One frame folded into the first-hit guide buffers from its bounce-0 surface rows, on the GPU and ordered on a stream: surfaces (pixels, 16) float32, the rows
        resolve_hits_device wrote for the rays of Renderer.primary_rays_device (row p = pixel p) -> (normal_depth (pixels, 4) float32, albedo (pixels, 4) float32, ids
        (pixels, 4) int32), laid out as Renderer.guides() returns them.  A surface (type == 1) contributes normal | distance, base colour | 1 and {1, instance, geometry,
        primitive}; any other row zeros and {0, -1, -1, -1}, whatever else it holds.  frame_index 0 replaces the averages (what they held is not read), otherwise
        (new + old * frame_index) / (frame_index + 1); the ids are this frame's.  out: the triple to update in place — this is how the averages are carried from frame to
        frame; allocated when None.  Folding frames 0 .. f - 1 gives the guides of Renderer(guides = 1) after draw(f), bit for bit.  Nothing is allocated (but the outputs
        when out is None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        s = self._rows(surfaces, "surfaces", torch.float32, (None, 16))
        npix = s.shape[0]
        frame_index = int(frame_index)
        if not 0 <= frame_index < 2 ** 32 - 1:
            raise ValueError("frame_index must be in [0, 2^32 - 1)")
        if out is None:
            out = (torch.empty((npix, 4), dtype=torch.float32, device=dev), torch.empty((npix, 4), dtype=torch.float32, device=dev), torch.empty((npix, 4), dtype=torch.int32, device=dev))
        out = tuple(out)
        if len(out) != 3:
            raise ValueError("out must hold 3 tensors: normal_depth, albedo, ids")
        nd = self._rows(out[0], "out[0] (normal_depth)", torch.float32, (npix, 4))
        al = self._rows(out[1], "out[1] (albedo)", torch.float32, (npix, 4))
        ids = self._rows(out[2], "out[2] (ids)", torch.int32, (npix, 4))
        p = [C.c_void_p(t.data_ptr() if npix else None) for t in (s, nd, al, ids)]
        check(lib.mrt_context_fold_guides_device(self.ctx.handle, npix, *p, frame_index, C.c_void_p(self._stream_handle(stream))))
        return nd, al, ids

    @staticmethod
    def denoise_workspace_bytes(size):
        """bytes of workspace denoise_device needs for an image of size (width, height): two images of 16 bytes per pixel"""
        n = C.c_size_t(0)
        check(lib.mrt_denoise_workspace_bytes(int(size[0]), int(size[1]), C.byref(n)))
        return int(n.value)

    def denoise_device(self, image, normal_depth, albedo, size, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, out=None, workspace=None,
                       stream=None):
        """Renderer.denoise's filter of an image the caller holds, on the GPU and ordered on a stream: image, normal_depth and albedo are float32 tensors of width x height
        x 4 elements — (h, w, 4) or (h * w, 4), row 0 = bottom — size = (width, height) -> the denoised image, float32 of image's shape, alpha 1.  image[..., 3] is
        ignored and no input is modified.  The parameters and their defaults are Renderer.denoise's.  out: the tensor to write (image's shape; it may not overlap an
        input); workspace: a torch.uint8 tensor of at least denoise_workspace_bytes(size) bytes; both are allocated with torch when None.  Otherwise nothing is allocated,
        copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        from ._ffi import DENOISE_DEFAULTS, DenoiseParams
        dev = torch.device("cuda", self.ctx.device)
        w, h = int(size[0]), int(size[1])
        need = self.denoise_workspace_bytes((w, h))                                                     # (refuses a size that is not positive or too large)
        shapes = ((h, w, 4), (h * w, 4))

        def img(t, what):
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) not in shapes or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous torch.float32 tensor of shape {shapes[0]} or {shapes[1]} on {dev}")
            return t

        img(image, "image"); img(normal_depth, "normal_depth"); img(albedo, "albedo")
        if out is None:
            out = torch.empty_like(image)
        elif tuple(img(out, "out").shape) != tuple(image.shape):
            raise ValueError("out must have image's shape")
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise ValueError(f"workspace must be a contiguous torch.uint8 tensor on {dev} (denoise_workspace_bytes(size) bytes)")
        given = dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth, demodulate=demodulate)
        v = {k: (DENOISE_DEFAULTS[k] if x is None else x) for k, x in given.items()}
        p = DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]), int(v["demodulate"]))
        check(lib.mrt_context_denoise_device(self.ctx.handle, w, h, C.c_void_p(image.data_ptr()), C.c_void_p(normal_depth.data_ptr()), C.c_void_p(albedo.data_ptr()),
                                             C.c_void_p(workspace.data_ptr() if workspace.numel() else None), workspace.numel(), C.c_void_p(out.data_ptr()), C.byref(p),
                                             C.c_void_p(self._stream_handle(stream))))
        return out

    def _images(self, size, **tensors):
        """size = (width, height) and named image tensors -> (w, h, the device): each a contiguous float32 tensor of shape (h, w, 4) or (h * w, 4) on the context's device"""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        w, h = int(size[0]), int(size[1])
        self.denoise_workspace_bytes((w, h))                                                            # (refuses a size that is not positive or too large)
        shapes = ((h, w, 4), (h * w, 4))
        for what, t in tensors.items():
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) not in shapes or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous torch.float32 tensor of shape {shapes[0]} or {shapes[1]} on {dev}")
        return w, h, dev

    def moments_sample_device(self, sample, albedo, size, demodulate=None, out=None, stream=None):
        """The sample image of the luminance moments, on the GPU and ordered on a stream: sample and albedo float32 tensors of width x height x 4 elements — (h, w, 4) or
        (h * w, 4), row 0 = bottom — size = (width, height) -> float32 of sample's shape, {l, l * l, 0, 0} per pixel with l the luminance of sample.rgb / A and A the
        albedo term of denoise_device (demodulate, default 1; 0: A = 1).  A second reproject_device call of the frame — the same surfaces, previous guide entries, cameras,
        previous positions and parameters, this image as its sample and its own previous output as prev_history — accumulates it into the moments {m1, m2, 0, length}
        denoise_variance_device reads.  out: the tensor to write (sample's shape; it may not overlap an input), allocated when None.  Otherwise nothing is allocated,
        copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        from ._ffi import DENOISE_DEFAULTS
        w, h, _ = self._images(size, sample=sample, albedo=albedo)
        if out is None:
            out = torch.empty_like(sample)
        else:
            self._images(size, out=out)
            if tuple(out.shape) != tuple(sample.shape):
                raise ValueError("out must have sample's shape")
        demodulate = int(DENOISE_DEFAULTS["demodulate"] if demodulate is None else demodulate)
        check(lib.mrt_context_moments_sample_device(self.ctx.handle, w, h, C.c_void_p(sample.data_ptr()), C.c_void_p(albedo.data_ptr()), demodulate, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(self._stream_handle(stream))))
        return out

    def denoise_variance_device(self, image, moments, normal_depth, albedo, size, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, out=None,
                                workspace=None, stream=None):
        """The variance-guided a-trous filter (the spatial step of SVGF) of an image the caller holds, on the GPU and ordered on a stream: image, moments, normal_depth and
        albedo are float32 tensors of width x height x 4 elements — (h, w, 4) or (h * w, 4), row 0 = bottom — size = (width, height) -> the filtered image, float32 of
        image's shape, alpha 1.  image: rgb = the accumulated colour, reproject_device's output (image[..., 3] is ignored); moments: {m1, m2, ., length}, the output of the
        frame's second reproject_device call on moments_sample_device's image.  A pixel with a history of at least 4 frames takes its variance from its own two moments,
        a younger one from the moments of its 7 x 7 neighbourhood, boosted by 4 / length; every level measures a tap's luminance difference in standard deviations of
        the pixel (sigma_color, default 4, is in standard deviations here and is not divided by the step) and carries the variance on.  The other parameters and their
        defaults are denoise_device's, and so are out and workspace (denoise_workspace_bytes(size) bytes).  The definition is include/mrt_abi.h's.  No input is modified.
        Nothing is allocated (but out and workspace when None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        from ._ffi import DENOISE_DEFAULTS, DenoiseParams
        w, h, dev = self._images(size, image=image, moments=moments, normal_depth=normal_depth, albedo=albedo)
        need = self.denoise_workspace_bytes((w, h))
        if out is None:
            out = torch.empty_like(image)
        else:
            self._images(size, out=out)
            if tuple(out.shape) != tuple(image.shape):
                raise ValueError("out must have image's shape")
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise ValueError(f"workspace must be a contiguous torch.uint8 tensor on {dev} (denoise_workspace_bytes(size) bytes)")
        given = dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth, demodulate=demodulate)
        v = {k: (DENOISE_DEFAULTS[k] if x is None else x) for k, x in given.items()}
        p = DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]), int(v["demodulate"]))
        check(lib.mrt_context_denoise_variance_device(self.ctx.handle, w, h, C.c_void_p(image.data_ptr()), C.c_void_p(moments.data_ptr()), C.c_void_p(normal_depth.data_ptr()),
                                                      C.c_void_p(albedo.data_ptr()), C.c_void_p(workspace.data_ptr() if workspace.numel() else None), workspace.numel(),
                                                      C.c_void_p(out.data_ptr()), C.byref(p), C.c_void_p(self._stream_handle(stream))))
        return out

    def tonemap_device(self, image, size, out=None, stream=None):
        """Renderer.tonemapped() of an image the caller holds, left on the GPU and ordered on a stream: image a float32 tensor of shape (h, w, 4) or (h * w, 4), row 0 =
        bottom, size = (width, height) -> torch.uint8 (h, w, 4), top row first: Reinhard, saturate, round to 8 bits, alpha 255.  out: the tensor to write, allocated
        when None.  Nothing else is allocated, copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        w, h = int(size[0]), int(size[1])
        self.denoise_workspace_bytes((w, h))                                                            # (refuses a size that is not positive or too large)
        shapes = ((h, w, 4), (h * w, 4))
        if not isinstance(image, torch.Tensor) or image.device != dev or image.dtype != torch.float32 or tuple(image.shape) not in shapes or not image.is_contiguous():
            raise ValueError(f"image must be a contiguous torch.float32 tensor of shape {shapes[0]} or {shapes[1]} on {dev}")
        if out is None:
            out = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
        else:
            self._rows(out, "out", torch.uint8, (h, w, 4))
        check(lib.mrt_context_tonemap_device(self.ctx.handle, w, h, C.c_void_p(image.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(self._stream_handle(stream))))
        return out

    def reproject_device(self, surfaces, sample, prev_normal_depth, prev_ids, prev_history, size, camera, prev_camera, prev_position=None, max_history=None, min_cos_normal=None,
                         depth_tolerance=None, out=None, stream=None):
        """Temporal reprojection of the accumulated image, on the GPU and ordered on a stream: what fold_sample_device does for a still world, kept up while the camera or
        an instance moves.  surfaces (pixels, 16) float32, this frame's bounce-0 rows of resolve_hits_device (row p = pixel p = y * width + x, row 0 = bottom); sample
        (pixels, 4) float32, this frame's radiance (w ignored); prev_normal_depth (pixels, 4) float32 and prev_ids (pixels, 4) int32, the PREVIOUS frame's own guide
        entries — what fold_guides_device(previous surfaces, 0) returned, not averaged; prev_history (pixels, 4) float32, rgb = accumulated colour, w = history length in
        frames (zeros: no history); size = (width, height); camera and prev_camera the two frames' Camera -> out (pixels, 4) float32: rgb = the new accumulated colour, w
        = the new length — the next frame's prev_history.  prev_position (pixels, 4) float32, xyz used: where, in the previous frame, the surface point seen at p now was
        (None: the geometry did not move); the caller makes it, from the instance's two poses or interpolate_device over the previous vertices.  Each surface pixel is
        projected into both cameras, up to four bilinear taps of the history are fetched at pixel + (previous - current) and kept where instance, geometry, normal
        (dot >= min_cos_normal, 0.9), squared distance (relative depth_tolerance, 0.1) and a length >= 1 agree, and out = (sample + history * (len - 1)) / len with len
        = min(length + 1, max_history (32)); a pixel that misses, projects nowhere or keeps no tap restarts at {sample, 1}.  The definition is include/mrt_abi.h's.  out
        may not overlap an input; it is allocated when None.  Otherwise nothing is allocated, copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        from ._ffi import REPROJECT_DEFAULTS, ReprojectParams
        dev = torch.device("cuda", self.ctx.device)
        w, h = int(size[0]), int(size[1])
        self.denoise_workspace_bytes((w, h))                                                            # (refuses a size that is not positive or too large)
        n = w * h
        self._rows(surfaces, "surfaces", torch.float32, (n, 16)); self._rows(sample, "sample", torch.float32, (n, 4))
        self._rows(prev_normal_depth, "prev_normal_depth", torch.float32, (n, 4)); self._rows(prev_ids, "prev_ids", torch.int32, (n, 4))
        self._rows(prev_history, "prev_history", torch.float32, (n, 4))
        if prev_position is not None: self._rows(prev_position, "prev_position", torch.float32, (n, 4))
        if not isinstance(camera, Camera) or not isinstance(prev_camera, Camera):
            raise ValueError("camera and prev_camera must be Camera structures")
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        else:
            self._rows(out, "out", torch.float32, (n, 4))
        given = dict(max_history=max_history, min_cos_normal=min_cos_normal, depth_tolerance=depth_tolerance)
        v = {k: float(REPROJECT_DEFAULTS[k] if x is None else x) for k, x in given.items()}
        par = ReprojectParams(v["max_history"], v["min_cos_normal"], v["depth_tolerance"], 0)
        p = [C.c_void_p(None if t is None else t.data_ptr()) for t in (surfaces, prev_position, prev_normal_depth, prev_ids, prev_history, sample, out)]
        check(lib.mrt_context_reproject_device(self.ctx.handle, w, h, C.byref(camera), C.byref(prev_camera), *p, C.byref(par), C.c_void_p(self._stream_handle(stream))))
        return out

    def vertex_offsets(self):
        """The vertex numbering interpolate_device reads attributes in: (meshes + 1,) uint64 — each mesh's first row, the source meshes concatenated in mesh-id order and
        an instance reporting its source's; the last entry is the number of rows."""
        cached = getattr(self, "_vertex_offsets", None)          # (the mesh list of a DeviceScene is fixed at construction; asked once — stats may wait for a refit in flight)
        if cached is None:
            count = int(self.stats.instances) + 1
            cached = np.zeros(count, np.uint64)
            check(lib.mrt_scene_vertex_offsets(self.handle, cached.ctypes.data_as(C.POINTER(C.c_uint64)), count))
            self._vertex_offsets = cached
        return cached.copy()

    def _stream_handle(self, stream):
        """the stream argument of every *_device method as an integer handle: None = torch's current stream of the context's device, a torch.cuda.Stream, or the handle itself"""
        import torch
        if stream is None:
            return int(torch.cuda.current_stream(torch.device("cuda", self.ctx.device)).cuda_stream)
        return int(stream.cuda_stream if isinstance(stream, torch.cuda.Stream) else stream)

    def _vertex_rows(self, t, what):
        """a torch.float32 (n, 3) tensor on the context's device whose rows are contiguous and a multiple of 4 bytes apart -> (pointer, row stride in bytes): no copy"""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        if not isinstance(t, torch.Tensor) or t.device != dev:
            raise ValueError(f"{what} must be a torch tensor on {dev}")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 3):
            raise ValueError(f"{what} must be a torch.float32 tensor of shape (n, 3) with contiguous rows (a slice of a wider tensor is fine)")
        return t.data_ptr(), (t.stride(0) if t.shape[0] > 1 else 3) * 4

    def update_mesh_device(self, mesh_id, positions, normals, stream=None):
        """Deforming geometry that lives on the GPU, ordered on a stream: positions and normals are torch.float32 (n, 3) tensors on the context's device, n the mesh's
        vertex count; rows may be any multiple of 4 bytes apart (x[:, :3] of an (n, 4) tensor, two halves of one interleaved (n, 8) tensor), nothing is copied.  Call
        refit_device() afterwards (several updates may share one).  stream: None = torch's current stream of that device, an integer handle (0 = the null stream) or a
        torch.cuda.Stream.  A NaN or an infinity in the input leaves the scene as it was and is counted in device_updates_rejected.  Keep the tensors alive until the
        stream has passed the call.  A tensor that is not what the first sentence says raises ValueError; normals of another length than positions raise
        MRTError(MRT_ERR_INVALID_ARGUMENT), as update_mesh does for the same mistake."""
        p, ps = self._vertex_rows(positions, "positions"); n, ns = self._vertex_rows(normals, "normals")
        if normals.shape[0] != positions.shape[0]:          # the device reads vertex_count normals: a shorter tensor would be read past its end
            raise MRTError(1, f"update_mesh_device: {normals.shape[0]} normals for {positions.shape[0]} positions (one normal per vertex)")
        check(lib.mrt_scene_update_mesh_device(self.handle, int(mesh_id), C.c_void_p(p), ps, C.c_void_p(n), ns, positions.shape[0], C.c_void_p(self._stream_handle(stream))))

    def refit_device(self, stream=None):
        """The refit of the resident tree after update_mesh_device, enqueued on the stream (as a commit after update_mesh computes it, without the commit's copies and waits)."""
        check(lib.mrt_scene_refit_device(self.handle, C.c_void_p(self._stream_handle(stream))))

    def set_instance_transforms_device(self, first_mesh_id, transforms, stream=None):
        """Instances of a two-level scene (option instancing = 1) moved from the GPU, ordered on a stream: transforms is a torch.float32 (n, 16) tensor on the context's
        device, column-major like set_instance_transform, for the mesh ids first_mesh_id .. first_mesh_id + n - 1; rows are contiguous and any multiple of 4 bytes apart
        (x[:, :16] of an (n, 20) tensor is fine), nothing is copied.  Call refit_instances_device() afterwards (several set calls may share one).  A NaN, an infinity or
        a singular matrix anywhere in the call leaves the scene as it was and is counted in device_updates_rejected.  The TLAS keeps the shape of the last commit;
        commit() builds it again from the poses the device holds.  stream: as update_mesh_device takes it.  Anything else than such a tensor raises ValueError."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        t = transforms
        if not isinstance(t, torch.Tensor) or t.device != dev:
            raise ValueError(f"transforms must be a torch tensor on {dev}")
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 16 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 16):
            raise ValueError("transforms must be a torch.float32 tensor of shape (n, 16) with contiguous rows (a slice of a wider tensor is fine)")
        n = t.shape[0]
        check(lib.mrt_scene_set_instance_transforms_device(self.handle, int(first_mesh_id), n, C.c_void_p(t.data_ptr() if n else None), (t.stride(0) if n > 1 else 16) * 4,
                                                           C.c_void_p(self._stream_handle(stream))))

    def refit_instances_device(self, stream=None):
        """The refit of both TLAS forms after set_instance_transforms_device, enqueued on the stream: boxes bottom-up, topology kept."""
        check(lib.mrt_scene_refit_instances_device(self.handle, C.c_void_p(self._stream_handle(stream))))

    def rebuild_tlas_device(self, stream=None):
        """The topology of both TLAS forms rebuilt on the stream from the poses the device holds, then their boxes refitted: call it INSTEAD of refit_instances_device()
        when instances have migrated.  The rope TLAS gets the nodes a commit would build, bit for bit; the 8-wide TLAS keeps the last commit's collapse and gets fresh
        instance sets under it.  Nothing is allocated, copied from the host or waited for after the first call."""
        check(lib.mrt_scene_rebuild_tlas_device(self.handle, C.c_void_p(self._stream_handle(stream))))

    def update_blas_device(self, mesh_id, positions, normals, stream=None):
        """A mesh deforming inside a two-level scene (option instancing = 1), from the GPU and ordered on a stream: positions and normals are torch.float32 (n, 3)
        tensors on the context's device in OBJECT space, n the vertex count of source mesh mesh_id, rows as update_mesh_device takes them; every instance of the mesh
        shares the result.  Call refit_blas_device() afterwards (several updates may share one).  A NaN or an infinity in the input leaves the scene as it was and is
        counted in device_updates_rejected.  A tensor that is not what the first sentence says raises ValueError; normals of another length than positions raise
        MRTError(MRT_ERR_INVALID_ARGUMENT)."""
        p, ps = self._vertex_rows(positions, "positions"); n, ns = self._vertex_rows(normals, "normals")
        if normals.shape[0] != positions.shape[0]:          # the device reads vertex_count normals: a shorter tensor would be read past its end
            raise MRTError(1, f"update_blas_device: {normals.shape[0]} normals for {positions.shape[0]} positions (one normal per vertex)")
        check(lib.mrt_scene_update_blas_device(self.handle, int(mesh_id), C.c_void_p(p), ps, C.c_void_p(n), ns, positions.shape[0], C.c_void_p(self._stream_handle(stream))))

    def refit_blas_device(self, stream=None):
        """The refit after update_blas_device, enqueued on the stream: the updated meshes' BLASes in place (as a commit after update_mesh computes them), their instances'
        boxes under the poses the device holds, both TLAS forms with the topology kept.  Poses set by set_instance_transforms_device need no refit of their own before it."""
        check(lib.mrt_scene_refit_blas_device(self.handle, C.c_void_p(self._stream_handle(stream))))

    @property
    def device_updates_rejected(self):
        """update_mesh_device / update_blas_device / set_instance_transforms_device calls refused on the device since the scene was created (blocks until the calls enqueued so far have run)."""
        v = C.c_uint64()
        check(lib.mrt_scene_device_updates_rejected(self.handle, C.byref(v)))
        return v.value

    def traversal_stats(self, rays, any_hit=False, alu_dup=0, mem_dup=0):
        """Diagnostics: (n, 8) uint32 {node visits, leaf visits, triangle tests, hit gid, t0, t1, 0, 0} per ray."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((rays.shape[0], 8), np.uint32)
        check(lib.mrt_debug_traversal_stats(self.handle, ptr(rays), rays.shape[0], (1 if any_hit else 0) | (alu_dup << 8) | (mem_dup << 16), ptr(out)))
        return out

    def stream_stats(self, rays, any_hit=False, per_wave=256):
        """Diagnostics: (nwaves, 8) uint32 lane accounting of the wide stream traversal."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        nw = (rays.shape[0] + per_wave - 1) // per_wave
        out = np.zeros((nw, 8), np.uint32)
        check(lib.mrt_debug_stream_stats(self.handle, ptr(rays), rays.shape[0], 1 if any_hit else 0, per_wave, ptr(out), nw))
        return out

    _LAYOUT_PARTS = {"wnodes": 0, "wpackets": 1, "instances": 2, "inst_box": 3, "wtlas_index": 4, "header": 5, "tlas_nodes": 6, "tlas_index": 7,
                     "rope_nodes": 8, "rope_packets": 9}

    def read_layout(self, part):
        """Diagnostics: one array of the committed layouts (mrt_debug_read_layout) as numpy — "wnodes" (n, 20) uint32, "wpackets" (n, 4 x stride)
        uint32, "instances" (n, 20) uint32 (InstanceDev), "inst_box" (n, 16) float32, "wtlas_index" (n,) uint32, "header" (8,) uint32,
        "tlas_nodes" (n, 16) uint32 (the rope TLAS of a two-level scene), "tlas_index" (n,) uint32, "rope_nodes" (n, 16) uint32 (the rope layout of a
        flattened scene, or every BLAS's of a two-level scene; n = 0 when the scene keeps none), "rope_packets" (n, 12) uint32 (its triangle packets)."""
        k = self._LAYOUT_PARTS[part] if isinstance(part, str) else int(part)
        n = C.c_uint64()
        check(lib.mrt_debug_read_layout(self.handle, k, None, 0, C.byref(n)))
        if k == 5:
            out = np.zeros(8, np.uint32)
        elif k in (4, 7):
            out = np.zeros(n.value, np.uint32)
        else:
            words = {0: 20, 2: 20, 3: 16, 6: 16, 8: 16, 9: 12}.get(k)
            if words is None:
                hdr = self.read_layout(5)
                words = 4 * int(hdr[7])
            out = np.zeros((n.value, words), np.float32 if k == 3 else np.uint32)
        check(lib.mrt_debug_read_layout(self.handle, k, ptr(out), out.nbytes, C.byref(n)))
        return out

    def close(self):
        if self.handle:
            lib.mrt_scene_destroy(self.handle)
            self.handle = C.c_void_p()


INTERSECTION_DTYPE = np.dtype([("type", np.int32), ("distance", np.float32), ("instance_id", np.int32), ("geometry_id", np.int32),
                               ("primitive_id", np.int32), ("u", np.float32), ("v", np.float32), ("_pad", np.int32)])


def unpack_intersections(t):
    """Views of the fields of a torch.int32 (n, 8) tensor of MRTIntersection records (DeviceScene.intersect_closest_device): no copy."""
    import torch
    return {"type": t[:, 0], "distance": t[:, 1].view(torch.float32), "instance_id": t[:, 2], "geometry_id": t[:, 3], "primitive_id": t[:, 4],
            "u": t[:, 5].view(torch.float32), "v": t[:, 6].view(torch.float32)}


SURFACE_DTYPE = np.dtype([("position", np.float32, 3), ("distance", np.float32), ("normal", np.float32, 3), ("type", np.int32),
                          ("base_color", np.float32, 3), ("resource_slot", np.int32),
                          ("instance_id", np.int32), ("geometry_id", np.int32), ("primitive_id", np.int32), ("_pad", np.int32)])


def unpack_surfaces(t):
    """The MRTSurface records of DeviceScene.resolve_hits_device as a structured numpy array (SURFACE_DTYPE), one per row of the (n, 16) float32 tensor: a view of a numpy
    array, of a CPU tensor's memory, or of the host copy of a GPU tensor (which waits for the tensor's stream)."""
    if not isinstance(t, np.ndarray):
        t = t.detach().cpu().numpy()
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 16)
    return t.view(SURFACE_DTYPE).reshape(-1)


LOBE_DTYPE = np.dtype([("weight", np.float32, 3), ("lobe", np.int32), ("emission", np.float32, 3), ("_pad", np.int32)])


def unpack_lobes(t):
    """The MRTScatterLobe records of DeviceScene.scatter_materials_device as a structured numpy array (LOBE_DTYPE), one per row of the (n, 8) float32 tensor: a view of a
    numpy array, of a CPU tensor's memory, or of the host copy of a GPU tensor (which waits for the tensor's stream)."""
    if not isinstance(t, np.ndarray):
        t = t.detach().cpu().numpy()
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 8)
    return t.view(LOBE_DTYPE).reshape(-1)


class Renderer:
    """Renderer.swift:12-357.  Draws ignore visibility masks (DeviceScene.set_mesh_masks): every mesh is traced by every ray class; an integrator composed from the query
    and stage methods honours them by passing mask= to its query calls (a renderer option is the follow-up of §11)."""

    @property
    def maxFramesInFlight(self):
        """Renderer.maxFramesInFlight (Renderer.swift:33 keeps 3).  Here: passes in flight on separate HIP streams, each carrying
        `frame_batch` frames (library defaults: 6 passes in flight x 8 frames at 1080p and above, up to 32 frames per pass for smaller images); set with set_option("frames_in_flight", n)."""
        return int(self.get_option("frames_in_flight"))

    def __init__(self, size, scene=None, device=0, seed=1, max_bounces=3, ctx=None, scene_options=None):
        self.size = (int(size[0]), int(size[1]))
        self.scene = scene if scene is not None else DragonScene(self.size)   # Renderer.swift:61
        self._own_ctx = ctx is None
        self.ctx = ctx or Context(device)
        self.device_scene = DeviceScene(self.ctx, self.scene, scene_options)
        self.handle = C.c_void_p()
        check(lib.mrt_renderer_create(self.ctx.handle, self.device_scene.handle, self.size[0], self.size[1], int(seed), int(max_bounces), C.byref(self.handle)))
        self.max_bounces = int(max_bounces)
        self.set_camera(self.scene.camera)

    # -- Renderer.frameIndex (Renderer.swift:41)
    @property
    def frameIndex(self):
        v = C.c_uint32()
        check(lib.mrt_renderer_frame_index(self.handle, C.byref(v)))
        return v.value

    @frameIndex.setter
    def frameIndex(self, v):
        check(lib.mrt_renderer_set_frame_index(self.handle, int(v)))

    def set_camera(self, camera: Camera):
        check(lib.mrt_renderer_set_camera(self.handle, C.byref(camera)))

    def primary_rays_device(self, sample_index=None, out=None, stream=None):
        """Where the rays come from (Raytracing.metal:171-221), on the GPU and ordered on a stream -> (rays (n, 8) float32, halton_index (n,) int32), n = width x height,
        pixel p = y * width + x with row 0 at the bottom as accumulation(): the primary ray draw() traces for that pixel at frame index sample_index (None = the
        renderer's current frameIndex) and the pixel's Halton index, hash(seed, p) + sample_index as int32 — what DeviceScene.scatter_device takes.  The whole image
        whatever the shard; the camera as set_camera left it.  Nothing of the renderer's is written and the frame index does not advance.  out: the tuple (rays,
        halton_index) to write.  Nothing is allocated (but the outputs when out is None), copied or synchronised.  stream: as intersect_closest_device takes it."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        n = self.size[0] * self.size[1]
        if out is None:
            out = (torch.empty((n, 8), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        else:
            out = tuple(out)
            if (len(out) != 2 or any(not isinstance(o, torch.Tensor) or o.device != dev or not o.is_contiguous() for o in out) or out[0].dtype != torch.float32 or tuple(out[0].shape) != (n, 8)
                    or out[1].dtype != torch.int32 or tuple(out[1].shape) != (n,)):
                raise ValueError(f"out must be (rays, halton_index): contiguous tensors on {dev}, torch.float32 {(n, 8)} and torch.int32 {(n,)}")
        si = self.frameIndex if sample_index is None else int(sample_index) & 0xFFFFFFFF
        check(lib.mrt_renderer_primary_rays_device(self.handle, si, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), C.c_void_p(self.device_scene._stream_handle(stream))))
        return out

    # -- Renderer.uniforms / updateUniforms (Renderer.swift:216-229): size, frameIndex, lightCount and camera in one 96-byte block
    @property
    def uniforms(self):
        from ._ffi import Uniforms
        u = Uniforms()
        check(lib.mrt_renderer_get_uniforms(self.handle, C.byref(u)))
        return u

    @uniforms.setter
    def uniforms(self, u):
        check(lib.mrt_renderer_set_uniforms(self.handle, C.byref(u)))
        self.size = (int(u.width), int(u.height))

    @property
    def framesCompleted(self):
        """Frames whose accumulation has finished on the device (never blocks) — the poll form of the completion handler of
        Renderer.swift:285-287."""
        v = C.c_uint64()
        check(lib.mrt_renderer_frames_completed(self.handle, C.byref(v)))
        return v.value

    # the host's knobs (include/mrt_abi.h mrt_renderer_set_option); every other key is one of the library's A/B switches (mrt_debug_renderer_set_option: tests, tools/, bench.py --opt)
    PUBLIC_OPTIONS = ("max_bounces", "frames_in_flight", "sample_offset", "frame_batch", "megakernel", "materials", "guides", "lanes_used", "lane_bytes")

    def set_option(self, key, value):
        fn = lib.mrt_renderer_set_option if key in self.PUBLIC_OPTIONS else lib.mrt_debug_renderer_set_option
        check(fn(self.handle, key.encode(), float(value)))

    def get_option(self, key):
        v = C.c_double(0.0)
        fn = lib.mrt_renderer_get_option if key in self.PUBLIC_OPTIONS else lib.mrt_debug_renderer_get_option
        check(fn(self.handle, key.encode(), C.byref(v)))
        return v.value

    def set_shard(self, rank, world):
        check(lib.mrt_renderer_set_shard(self.handle, int(rank), int(world)))

    def drawableSizeWillChange(self, size):                   # Renderer.swift:353-356
        self.size = (int(size[0]), int(size[1]))
        check(lib.mrt_renderer_resize(self.handle, self.size[0], self.size[1]))
        self.scene.updateUniforms(self.size)
        self.set_camera(self.scene.camera)

    def draw(self, frames=1, wait=False):                     # Renderer.swift:284-351
        check(lib.mrt_renderer_render(self.handle, int(frames)))
        if wait:
            self.wait()

    def wait(self):
        check(lib.mrt_renderer_wait(self.handle))

    def accumulation(self):
        """accumulationTargets[0] (Renderer.swift:332-334): (h, w, 4) float32, row 0 = bottom of the image."""
        out = np.empty((self.size[1], self.size[0], 4), np.float32)
        check(lib.mrt_renderer_read_accum(self.handle, ptr(out), out.nbytes))
        return out

    def tonemapped(self):
        """fragmentShader (Shaders.metal:39-52): (h, w, 4) uint8, top row first."""
        out = np.empty((self.size[1], self.size[0], 4), np.uint8)
        check(lib.mrt_renderer_read_tonemapped_rgba8(self.handle, ptr(out), out.nbytes))
        return out

    def copy_accum_to(self, device_ptr, nbytes):
        check(lib.mrt_renderer_copy_accum_to_device(self.handle, C.c_void_p(device_ptr), nbytes))

    def write_accum_from(self, device_ptr, nbytes):
        check(lib.mrt_renderer_write_accum_from_device(self.handle, C.c_void_p(device_ptr), nbytes))

    # -- first-hit guide buffers and the denoiser (set_option("guides", 1) before drawing; no counterpart in the reference)
    def guides(self):
        """{"normal_depth": (h, w, 4) float32 — shading normal | hit distance of the primary hit, "albedo": (h, w, 4) float32 — baseColor | coverage,
        "ids": (h, w, 4) int32 — type, instance_id, geometry_id, primitive_id of the last frame}; row 0 = bottom, as accumulation()."""
        from ._ffi import GUIDE_ALBEDO, GUIDE_IDS, GUIDE_NORMAL_DEPTH
        out = {}
        for name, which, dt in (("normal_depth", GUIDE_NORMAL_DEPTH, np.float32), ("albedo", GUIDE_ALBEDO, np.float32), ("ids", GUIDE_IDS, np.int32)):
            a = np.empty((self.size[1], self.size[0], 4), dt)
            check(lib.mrt_renderer_read_guide(self.handle, which, ptr(a), a.nbytes))
            out[name] = a
        return out

    def copy_guide_to(self, which, device_ptr, nbytes):
        check(lib.mrt_renderer_copy_guide_to_device(self.handle, int(which), C.c_void_p(device_ptr), nbytes))

    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_depth=None, demodulate=None, read=True):
        """The edge-avoiding a-trous filter of the accumulation buffer (mrt_renderer_denoise) -> (h, w, 4) float32, row 0 = bottom
        (None with read=False: the image stays on the device for denoised_tonemapped() / copy_denoised_to())."""
        from ._ffi import DENOISE_DEFAULTS, DenoiseParams
        given = dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_depth=sigma_depth, demodulate=demodulate)
        v = {k: (DENOISE_DEFAULTS[k] if x is None else x) for k, x in given.items()}
        p = DenoiseParams(int(v["iterations"]), float(v["sigma_color"]), float(v["sigma_normal"]), float(v["sigma_depth"]), int(v["demodulate"]))
        check(lib.mrt_renderer_denoise(self.handle, C.byref(p)))
        return self.denoised() if read else None

    def denoised(self):
        out = np.empty((self.size[1], self.size[0], 4), np.float32)
        check(lib.mrt_renderer_read_denoised(self.handle, ptr(out), out.nbytes))
        return out

    def denoised_tonemapped(self):
        """tonemapped() of the denoised image: (h, w, 4) uint8, top row first."""
        out = np.empty((self.size[1], self.size[0], 4), np.uint8)
        check(lib.mrt_renderer_read_denoised_tonemapped_rgba8(self.handle, ptr(out), out.nbytes))
        return out

    def copy_denoised_to(self, device_ptr, nbytes):
        check(lib.mrt_renderer_copy_denoised_to_device(self.handle, C.c_void_p(device_ptr), nbytes))

    def shard_tiles(self, rank, world):
        """8 x 8 tiles of this image that shard (rank, world) owns (a compact buffer of that shard is tiles x 64 RGBA32F pixels)."""
        n = C.c_uint64()
        check(lib.mrt_renderer_shard_tiles(self.handle, int(rank), int(world), C.byref(n)))
        return n.value

    def pack_owned_tiles(self, device_ptr, nbytes):
        check(lib.mrt_renderer_pack_owned_tiles(self.handle, C.c_void_p(device_ptr), nbytes))

    def unpack_tiles(self, device_ptr, nbytes, rank, world):
        check(lib.mrt_renderer_unpack_tiles(self.handle, C.c_void_p(device_ptr), nbytes, int(rank), int(world)))

    def unpack_tiles_into(self, image_ptr, image_nbytes, device_ptr, nbytes, rank, world):
        """unpack_tiles into a caller's (h, w, 4) float32 device image instead of this renderer's accumulation buffer."""
        check(lib.mrt_renderer_unpack_tiles_into(self.handle, C.c_void_p(image_ptr), image_nbytes, C.c_void_p(device_ptr), nbytes, int(rank), int(world)))

    @property
    def stats(self):
        s = RenderStats()
        check(lib.mrt_renderer_stats(self.handle, C.byref(s)))
        return s

    def reset_stats(self):
        check(lib.mrt_renderer_reset_stats(self.handle))

    @property
    def kernel_times(self):
        """{class: (summed ms, launches)} over the launches of the last draw that carried their own start/stop events."""
        from ._ffi import KERNEL_CLASSES, KernelTimes
        k = KernelTimes()
        check(lib.mrt_renderer_kernel_times(self.handle, C.byref(k)))
        return {name: (float(k.ms[i]), int(k.launches[i])) for i, name in enumerate(KERNEL_CLASSES)}

    def close(self):
        if self.handle:
            lib.mrt_renderer_destroy(self.handle)
            self.handle = C.c_void_p()
        self.device_scene.close()
        if self._own_ctx:
            self.ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _TemplateScene(DeviceScene):
    """A scene that is filled (meshes, lights, options) but not committed: the template a device group replicates."""

    def __init__(self, ctx_handle, scene, options=None):
        self.ctx = None
        self.handle = C.c_void_p()
        check(lib.mrt_scene_create(ctx_handle, C.byref(self.handle)))
        for k, v in (options or {}).items():
            check(lib.mrt_scene_set_option(self.handle, k.encode(), float(v)))
        from .scene import flatten_scene
        for pos, nrm, xf, subs, source in flatten_scene(scene, share=True):
            mid = C.c_int32()
            if source >= 0:
                check(lib.mrt_scene_add_instance(self.handle, source, ptr(xf), C.byref(mid)))
                continue
            pos = np.ascontiguousarray(pos, np.float32)
            nrm = np.ascontiguousarray(nrm, np.float32)
            check(lib.mrt_scene_add_mesh(self.handle, ptr(pos), 12, ptr(nrm), 12, pos.shape[0], ptr(xf), C.byref(mid)))
            for idx, mat in subs:
                idx = np.ascontiguousarray(idx, np.uint32)
                check(lib.mrt_mesh_add_submesh(self.handle, mid.value, ptr(idx), idx.shape[0], C.byref(mat), None))
        self.set_lights(scene.lights)


class GroupRenderer:
    """Renderer over the n GPUs of one node in ONE process (mrt_group_*): the scene is replicated, the image sharded by 8x8 screen tile
    (tile_id % n == rank), `gather()` runs the one reduce(sum) per output image (RCCL over xGMI; peer copies + add when a device is
    named twice).  The reference creates a single MTLDevice (Renderer.swift:46-59); this widens that seam."""

    def __init__(self, size, scene, devices, seed=1, max_bounces=3, scene_options=None):
        self.size = (int(size[0]), int(size[1]))
        self.scene = scene
        ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        self.group = C.c_void_p()
        check(lib.mrt_group_create(ids, len(devices), C.byref(self.group)))
        self.handle = C.c_void_p()
        self._template = None
        try:
            c0 = C.c_void_p()
            check(lib.mrt_group_context(self.group, 0, C.byref(c0)))
            self._template = _TemplateScene(c0, scene, scene_options)
            check(lib.mrt_group_renderer_create(self.group, self._template.handle, self.size[0], self.size[1], int(seed), int(max_bounces), C.byref(self.handle)))
            check(lib.mrt_group_set_camera(self.handle, C.byref(scene.camera)))
        except Exception:
            self.close()
            raise

    @property
    def world(self):
        n = C.c_int32()
        check(lib.mrt_group_size(self.group, C.byref(n)))
        return n.value

    @property
    def reduce_mode(self):
        m = C.c_int32(); buf = C.create_string_buffer(256)
        check(lib.mrt_group_reduce_mode(self.group, C.byref(m), buf, 256))
        return m.value, buf.value.decode()

    def set_reduce_mode(self, mode):
        check(lib.mrt_group_set_reduce_mode(self.group, int(mode)))

    def set_option(self, key, value):
        if key in Renderer.PUBLIC_OPTIONS:
            check(lib.mrt_group_set_option(self.handle, key.encode(), float(value)))
            return
        for rank in range(self.world):                       # an A/B switch: through every device's renderer
            r = C.c_void_p()
            check(lib.mrt_group_renderer_rank(self.handle, rank, C.byref(r)))
            check(lib.mrt_debug_renderer_set_option(r, key.encode(), float(value)))

    def rank_option(self, rank, key):
        r = C.c_void_p(); v = C.c_double()
        check(lib.mrt_group_renderer_rank(self.handle, int(rank), C.byref(r)))
        check(lib.mrt_debug_renderer_get_option(r, key.encode(), C.byref(v)))
        return v.value

    def draw(self, frames=1, wait=False):
        check(lib.mrt_group_render(self.handle, int(frames)))
        if wait:
            self.wait()

    def wait(self):
        check(lib.mrt_group_wait(self.handle))

    def rank_stats(self, rank):
        """One device's own counters and the device time of its last draw (mrt_renderer_stats of that rank's renderer): what a scaling record is diagnosed with."""
        r = C.c_void_p(); s = RenderStats()
        check(lib.mrt_group_renderer_rank(self.handle, int(rank), C.byref(r)))
        check(lib.mrt_renderer_stats(r, C.byref(s)))
        return s

    @property
    def framesCompleted(self):
        v = C.c_uint64()
        check(lib.mrt_group_frames_completed(self.handle, C.byref(v)))
        return v.value

    def gather(self, to_host=True):
        """The assembled image: (h, w, 4) float32, row 0 = bottom (None with to_host=False: it stays on the root device)."""
        if not to_host:
            check(lib.mrt_group_gather(self.handle, None, 0))
            return None
        out = np.empty((self.size[1], self.size[0], 4), np.float32)
        check(lib.mrt_group_gather(self.handle, ptr(out), out.nbytes))
        return out

    @property
    def stats(self):
        s = RenderStats()
        check(lib.mrt_group_stats(self.handle, C.byref(s)))
        return s

    def close(self):
        if self.handle:
            lib.mrt_group_renderer_destroy(self.handle)
            self.handle = C.c_void_p()
        if self._template is not None:
            self._template.close()
            self._template = None
        if self.group:
            lib.mrt_group_destroy(self.group)
            self.group = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def save_png(path, rgba8):
    """The tonemapped image (Renderer.tonemapped(): (h, w, 4) uint8, row 0 = top — the blit's flip, Shaders.metal:35) as an 8-bit RGBA PNG; zlib only."""
    import struct, zlib
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4: raise ValueError("save_png: expected (h, w, 4) uint8")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * 4)], axis=1).tobytes()          # filter byte 0 in front of every row
    def chunk(tag, data): return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def save_pfm(path, accum):
    """The accumulation buffer (Renderer.accumulation(): (h, w, 4) float32 radiance, row 0 = the BOTTOM of the image, SURVEY a-4) as a little-endian colour PFM —
    whose rows are stored bottom to top as well, so the buffer goes out as it lies.  For comparing radiance, not display (no tonemap)."""
    a = np.asarray(accum, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] not in (3, 4): raise ValueError("save_pfm: expected (h, w, 3 or 4) float32")
    h, w = a.shape[:2]
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n-1.0\n".encode()); f.write(np.ascontiguousarray(a[:, :, :3]).astype("<f4").tobytes())
