"""numpy restatement of the masked ray queries (include/mrt_abi.h mrt_scene_intersect_*_masked_device; csrc/masked.hip).

TEST INFRASTRUCTURE.  A wrapper over tests/multihit_reference.py, which it leaves as it is: by the contract the result of a ray with mask r is what the unmasked query returns
on a scene that holds only the meshes visible to r, with the ids of the full scene.  So, per DISTINCT ray mask, the triangles whose mesh — ids[:, 0], the id
MRTIntersection.instance_id reports — is visible are kept, in their order (the tie rule "lowest global id among the visible" is then the reference's own tie rule), and
MultihitReference.intersect_all runs on them: every kept triangle against every ray, no tree, no bound, no filter inside a walk that could be misplaced.
With every mesh visible nothing is filtered and the call IS MultihitReference's."""
import copy

import numpy as np

import multihit_reference as M

ALL = 0xFFFFFFFF


class MaskedReference:
    def __init__(self, entries, mesh_masks=None):
        """entries: flatten_scene(scene) tuples; mesh_masks: one per entry (default: all ones)"""
        self.full = M.MultihitReference(entries)
        self.mesh_masks = np.full(len(entries), ALL, np.uint32)
        if mesh_masks is not None: self.set_mesh_masks(mesh_masks)

    def set_mesh_masks(self, masks, first_mesh_id=0):
        masks = np.asarray(masks, np.uint32)
        self.mesh_masks[first_mesh_id:first_mesh_id + len(masks)] = masks

    def visible(self, ray_mask):
        """per triangle of the full scene: the ray mask sees its mesh"""
        return (self.mesh_masks[self.full.ids[:, 0]] & np.uint32(ray_mask)) != 0

    def _subset(self, keep):
        if keep.all(): return self.full
        sub = copy.copy(self.full)
        sub.v0, sub.e1, sub.e2, sub.ids = self.full.v0[keep], self.full.e1[keep], self.full.e2[keep], self.full.ids[keep]
        return sub

    def intersect_all(self, rays, max_hits, ray_masks=ALL):
        """rays (n, 8) float32; ray_masks: one int for every ray, or (n,) -> (hits (n, max_hits) INTERSECTION_DTYPE, counts (n,) int32)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = rays.shape[0]
        rm = np.broadcast_to(np.asarray(ray_masks, np.int64).astype(np.uint32), (n,))
        hits = np.empty((n, int(max_hits)), M.INTERSECTION_DTYPE); hits[:] = M.miss_record()
        counts = np.zeros(n, np.int32)
        for r in np.unique(rm):
            sel = np.flatnonzero(rm == r)
            h, c = self._subset(self.visible(r)).intersect_all(rays[sel], max_hits)
            hits[sel] = h; counts[sel] = c
        return hits, counts

    def intersect_closest(self, rays, ray_masks=ALL):
        return self.intersect_all(rays, 1, ray_masks)[0][:, 0]

    def intersect_any(self, rays, ray_masks=ALL):
        return (self.intersect_all(rays, 1, ray_masks)[1] > 0).astype(np.int32)


def quad_stack_masks(layers):
    """quad_stack(L): one mesh per quad, quad k with the mask 1 << k (L <= 32)"""
    return (np.uint32(1) << np.arange(layers, dtype=np.uint32)).astype(np.uint32)


def three_models(mrt, visible=(0, 1, 2, 3)):
    """sphere + train + teapot over the plane: four meshes (ids 0 .. 3), the models overlapping around the origin; visible: the ids kept, in order"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            every = [mrt.Model(name="sphere", position=[0.1, -0.2, 0.3], rotation=[0.2, 0.5, -0.1], scale=1.3),
                     mrt.Model(name="train", position=[-0.4, -0.6, 0.2], rotation=[0.0, 0.7, 0.0], scale=1.1),
                     mrt.Model(name="teapot", position=[0.5, 0.0, -0.3], rotation=[-0.1, 0.2, 0.3], scale=0.02),
                     mrt.Model(name="plane", position=[0, -3, 0], scale=50)]
            self.models = [every[k] for k in visible]
    return S((8, 8))
