"""Scenes and Material edits shared by the tests of the materials extension (test_materials.py, test_oracle_kat.py, test_independent_f64.py) — TEST INFRASTRUCTURE."""
import numpy as np


def with_material(mrt, model, **fields):
    """a copy of the model's submeshes with edited Material fields (the cached Submesh objects are shared between models)"""
    for mesh in model.meshes:
        subs = []
        for s in mesh.submeshes:
            m = mrt.Material.from_buffer_copy(bytes(s.material))
            for k, v in fields.items():
                if isinstance(v, (list, tuple)):
                    f = getattr(m, k); f.x, f.y, f.z = v
                else:
                    setattr(m, k, v)
            subs.append(mrt.Submesh(s.name, s.indices, m))
        mesh.submeshes = subs
    return model


def cornell_with_materials(mrt, size, plain=False):
    class S(mrt.CornellScene):
        def __init__(self, size):
            super().__init__(size)
            h = np.pi / 2
            glass = mrt.Model(name="sphere", position=[-0.45, 0.35, 0.35], scale=0.35)
            shiny = mrt.Model(name="sphere", position=[0.45, 0.3, -0.1], scale=0.3)
            lamp = mrt.Model(name="plane", position=[0.99, 1.0, 0.2], rotation=[0, 0, h], scale=0.25)
            if plain:                                             # sphere.mtl carries Ks 0.8 / Ns 32: strip it, so that every lobe choice is the diffuse one
                for mo in (glass, shiny): with_material(mrt, mo, specular=[0.0, 0.0, 0.0])
            else:
                with_material(mrt, glass, dissolve=0.15, refractionIndex=1.5, baseColor=[0.9, 0.9, 0.9])
                with_material(mrt, shiny, specular=[0.8, 0.7, 0.3], specularExponent=96.0, baseColor=[0.2, 0.1, 0.05])
                with_material(mrt, lamp, emission=[2.0, 1.5, 0.5])
            self.models = self.models[:5] + [glass, shiny, lamp]            # the five walls of CornellScene + three objects
    return S(size)


def look_at(mrt, position, target, half_width, half_height, up=(0.0, 1.0, 0.0)):
    """a Camera (ShaderTypes.h:60-65) at `position` looking at `target`: `right` / `up` carry the half extents of the image plane at distance 1"""
    p, t = np.asarray(position, np.float64), np.asarray(target, np.float64)
    f = (t - p) / np.linalg.norm(t - p)
    r = np.cross(f, np.asarray(up, np.float64)); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    cam = mrt.Camera()
    cam.position, cam.right, cam.up, cam.forward = mrt.Float3(*p), mrt.Float3(*(r * half_width)), mrt.Float3(*(u * half_height)), mrt.Float3(*f)
    return cam


def pixel_directions(cam, width, height, x, y):
    """float64 unit directions of the primary rays through the (fractional) pixel coordinates x, y — Raytracing.metal:204-218"""
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)
    ux, uy = np.asarray(x, np.float64) / width * 2.0 - 1.0, np.asarray(y, np.float64) / height * 2.0 - 1.0
    d = ux[..., None] * v(cam.right) + uy[..., None] * v(cam.up) + v(cam.forward)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def quad_scene(mrt, size, quads, lights, camera=None):
    """a scene of plane.obj quads (2 x 2, normal +y before the rotation): quads = [dict(position=, rotation=, scale=, <Material fields>)]"""
    class S(mrt.Scene):
        def __init__(self, size):
            super().__init__(size)
            self.models = []
            for q in quads:
                q = dict(q)
                mo = mrt.Model(name="plane", position=q.pop("position"), rotation=q.pop("rotation", (0.0, 0.0, 0.0)), scale=q.pop("scale", 1.0))
                self.models.append(with_material(mrt, mo, **q))
            self.lights = lights
            if camera is not None:
                self.camera = camera
    return S(size)


# name -> Material fields: between them every boundary of the predicates of docs/HISTORY.md §10 (dissolve at 0, 1, next to either; Ni 1, below 1, 0, high; Ns 0, tiny, huge; ps 0, 1/2, 1)
EDGE_MATERIALS = {
    "glass_thin":     dict(baseColor=[0.9, 0.9, 0.9], specular=[0.0, 0.0, 0.0], specularExponent=30.0, refractionIndex=2.4, dissolve=2.0 ** -20),       # 1 - dissolve rounds next to 1: always the interface
    "glass_tir":      dict(baseColor=[0.7, 0.8, 0.9], specular=[0.0, 0.0, 0.0], specularExponent=30.0, refractionIndex=0.67, dissolve=0.5),             # thinner than vacuum: total internal reflection on the way IN
    "glass_index_1":  dict(baseColor=[0.8, 0.6, 0.4], specular=[0.3, 0.3, 0.3], specularExponent=12.0, refractionIndex=1.0, dissolve=0.3),              # r0 = 0, eta = 1: the ray goes straight on
    "index_0":        dict(baseColor=[0.4, 0.4, 0.4], specular=[0.4, 0.2, 0.1], specularExponent=0.01, refractionIndex=0.0, dissolve=0.5),              # Ni 0 switches the interface off; Ks = Kd (ps = 1/2); a very wide lobe
    "dissolve_0":     dict(baseColor=[0.5, 0.7, 0.5], specular=[0.6, 0.6, 0.6], specularExponent=0.0, refractionIndex=1.5, dissolve=0.0),               # dissolve exactly 0: no interface; Ns 0 with Ks > 0: no lobe either (ps = 0)
    "mirror":         dict(baseColor=[0.0, 0.0, 0.0], specular=[0.9, 0.8, 0.7], specularExponent=1e6, refractionIndex=1.5, dissolve=1.0),               # dissolve exactly 1; Kd 0: ps = 1, 1 / (1 - ps) must never be formed
    "black_emitter":  dict(baseColor=[0.0, 0.0, 0.0], specular=[0.0, 0.0, 0.0], specularExponent=30.0, refractionIndex=1.5, dissolve=1.0 - 2.0 ** -24,  # 1 - dissolve = 2^-24: the interface only at u = 0
                           emission=[1.5, 1.0, 0.25]),
    "emissive_glass": dict(baseColor=[0.6, 0.6, 0.6], specular=[0.5, 0.5, 0.5], specularExponent=50.0, refractionIndex=1.5, dissolve=0.4, emission=[0.25, 0.5, 1.0]),
}


def edge_material_scene(mrt, size):
    """Cornell's five walls + small spheres and upright quads carrying EDGE_MATERIALS, seen from close by: the box nearly fills the frame, a margin of primary rays misses everything.  The second `glass_thin` sphere shares
    the first one's submeshes: with instancing = 1 the two are instances of one mesh (so are walls 1 .. 4 of wall 0)."""
    h = np.pi / 2

    class S(mrt.CornellScene):
        def __init__(self, size):
            super().__init__(size)
            sphere = lambda p, s, name: with_material(mrt, mrt.Model(name="sphere", position=p, scale=s), **EDGE_MATERIALS[name])
            quad = lambda p, s, name: with_material(mrt, mrt.Model(name="plane", position=p, rotation=[h, 0, 0], scale=s), **EDGE_MATERIALS[name])
            objs = [sphere([-0.6, 0.25, 0.3], 0.25, "glass_thin"), sphere([-0.1, 0.2, 0.6], 0.2, "glass_tir"), sphere([0.35, 0.22, 0.25], 0.22, "glass_index_1"),
                    sphere([0.72, 0.2, 0.6], 0.2, "mirror"), quad([-0.55, 1.25, -0.5], 0.22, "index_0"), quad([0.0, 1.4, -0.6], 0.2, "dissolve_0"),
                    quad([0.55, 1.25, -0.5], 0.22, "black_emitter"), quad([0.0, 0.75, -0.2], 0.25, "emissive_glass")]
            twin = mrt.Model(name="sphere", position=[-0.5, 0.85, -0.3], rotation=[0.3, 0.2, 0.1], scale=0.18)
            twin.meshes[0].submeshes = objs[0].meshes[0].submeshes
            self.object_names = ["wall"] * 5 + ["glass_thin", "glass_tir", "glass_index_1", "mirror", "index_0", "dissolve_0", "black_emitter", "emissive_glass", "glass_thin"]
            self.models = self.models[:5] + objs + [twin]
            self.camera = look_at(mrt, [0.0, 1.0, 3.4], [0.0, 0.9, 0.0], 0.5, 0.5 * size[1] / size[0])
    return S(size)
