"""metal-raytracing_amd — MI355X-native path tracer behind the reference's Scene / Model / Mesh /
Submesh / Renderer surface.  The render path is hand-written HIP for gfx950 reached through the C
ABI of include/mrt_abi.h (libmrt_hip.so); importing this package fails if that library is missing.

The directory name carries a hyphen (it follows the reference repository's name); import it as
`metal_raytracing_amd` (the sibling alias package re-exports this one).
"""
from ._ffi import (Camera, Float3, Intersection, Light, LightType, Material, MRTError, Ray, RenderStats, SceneStats, Surface, ScatterLobe, RowColumn, Uniforms, DenoiseParams, DENOISE_DEFAULTS, ReprojectParams, REPROJECT_DEFAULTS, lib, LIB_PATH,
                   GEOMETRY_MASK_TRIANGLE, GEOMETRY_MASK_LIGHT, RAY_MASK_PRIMARY, RAY_MASK_SHADOW, RAY_MASK_SECONDARY)
from .scene import (SCENES, CornellScene, DragonScene, GardenScene, InstancedDragonScene, IrregularDragonScene, HostileDragonScene, dragon_proxy_irregular, dragon_proxy_hostile, Mesh, Model, Scene, Submesh, flatten_scene, make_transform, load_obj, dragon_proxy, bunny_proxy)
from .renderer import Context, DeviceScene, GroupRenderer, Renderer, save_png, save_pfm, unpack_intersections, INTERSECTION_DTYPE, unpack_surfaces, SURFACE_DTYPE, unpack_lobes, LOBE_DTYPE

__all__ = ["Camera", "Float3", "Intersection", "Light", "LightType", "Material", "MRTError", "Ray", "RenderStats", "SceneStats",
           "Uniforms", "DenoiseParams", "DENOISE_DEFAULTS", "ReprojectParams", "REPROJECT_DEFAULTS", "lib", "LIB_PATH", "SCENES", "CornellScene", "DragonScene", "GardenScene", "InstancedDragonScene", "IrregularDragonScene", "HostileDragonScene", "dragon_proxy_irregular", "dragon_proxy_hostile", "Mesh",
           "Model", "Scene", "Submesh", "flatten_scene", "make_transform", "load_obj", "dragon_proxy", "bunny_proxy", "Context",
           "DeviceScene", "GroupRenderer", "Renderer", "save_png", "save_pfm", "unpack_intersections", "INTERSECTION_DTYPE", "unpack_surfaces", "SURFACE_DTYPE", "Surface", "unpack_lobes", "LOBE_DTYPE", "ScatterLobe", "RowColumn",
           "GEOMETRY_MASK_TRIANGLE", "GEOMETRY_MASK_LIGHT", "RAY_MASK_PRIMARY", "RAY_MASK_SHADOW", "RAY_MASK_SECONDARY"]
