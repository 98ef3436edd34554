// abi_check.h — compile-time pin of the data contract of include/mrt_abi.h against the reference's bridging header
// (ShaderTypes.h:60-107; `vector_float3` is 16 bytes, 16-byte aligned).  Included by api.cpp, so a struct edit that moves a
// field breaks the build of libmrt_hip.so; tests/test_abi_and_host.py checks the same offsets through ctypes.
#pragma once
#include <cstddef>
#include "../../include/mrt_abi.h"

#define MRT_AT(T, field, off) static_assert(offsetof(T, field) == (off), #T "." #field " must sit at byte " #off)

static_assert(sizeof(MRTFloat3) == 16, "vector_float3 is 16 bytes");
// Camera, ShaderTypes.h:60-65
static_assert(sizeof(MRTCamera) == 64, "Camera is 64 bytes");
MRT_AT(MRTCamera, position, 0); MRT_AT(MRTCamera, right, 16); MRT_AT(MRTCamera, up, 32); MRT_AT(MRTCamera, forward, 48);
// LightType, ShaderTypes.h:67-74 (the enum quirk of :16-21: 0 is unused)
static_assert(MRTLightTypeUnused == 0 && MRTLightTypeSunlight == 1 && MRTLightTypeSpotlight == 2 && MRTLightTypePointlight == 3 && MRTLightTypeAreaLight == 4, "LightType values");
// Light, ShaderTypes.h:76-87
static_assert(sizeof(MRTLight) == 128, "Light is 128 bytes");
MRT_AT(MRTLight, type, 0); MRT_AT(MRTLight, position, 16); MRT_AT(MRTLight, color, 32); MRT_AT(MRTLight, forward, 48);
MRT_AT(MRTLight, right, 64); MRT_AT(MRTLight, up, 80); MRT_AT(MRTLight, coneAngle, 96); MRT_AT(MRTLight, direction, 112);
// Uniforms, ShaderTypes.h:89-97
static_assert(sizeof(MRTUniforms) == 96, "Uniforms is 96 bytes");
MRT_AT(MRTUniforms, width, 0); MRT_AT(MRTUniforms, height, 4); MRT_AT(MRTUniforms, blocksWide, 8); MRT_AT(MRTUniforms, frameIndex, 12);
MRT_AT(MRTUniforms, lightCount, 16); MRT_AT(MRTUniforms, camera, 32);
// Material, ShaderTypes.h:99-107
static_assert(sizeof(MRTMaterial) == 64, "Material is 64 bytes");
MRT_AT(MRTMaterial, baseColor, 0); MRT_AT(MRTMaterial, specular, 16); MRT_AT(MRTMaterial, emission, 32);
MRT_AT(MRTMaterial, specularExponent, 48); MRT_AT(MRTMaterial, refractionIndex, 52); MRT_AT(MRTMaterial, dissolve, 56);
// query records
static_assert(sizeof(MRTRay) == 32 && sizeof(MRTIntersection) == 32, "ray / intersection records are 32 bytes");
MRT_AT(MRTRay, min_distance, 12); MRT_AT(MRTRay, direction, 16); MRT_AT(MRTRay, max_distance, 28);
// surface records (mrt_scene_resolve_hits_device; no counterpart in ShaderTypes.h): four 16-byte groups
static_assert(sizeof(MRTSurface) == 64, "MRTSurface is 64 bytes");
MRT_AT(MRTSurface, position, 0); MRT_AT(MRTSurface, distance, 12); MRT_AT(MRTSurface, normal, 16); MRT_AT(MRTSurface, type, 28);
MRT_AT(MRTSurface, base_color, 32); MRT_AT(MRTSurface, resource_slot, 44); MRT_AT(MRTSurface, instance_id, 48); MRT_AT(MRTSurface, _pad, 60);
// lobe rows (mrt_scene_scatter_materials_device; no counterpart in ShaderTypes.h): two 16-byte groups
static_assert(sizeof(MRTScatterLobe) == 32, "MRTScatterLobe is 32 bytes");
MRT_AT(MRTScatterLobe, weight, 0); MRT_AT(MRTScatterLobe, lobe, 12); MRT_AT(MRTScatterLobe, emission, 16); MRT_AT(MRTScatterLobe, _pad, 28);
// a column of mrt_context_compact_rows_device (no counterpart in ShaderTypes.h): two pointers, the row's size, padding
static_assert(sizeof(MRTRowColumn) == 24, "MRTRowColumn is 24 bytes");
MRT_AT(MRTRowColumn, src, 0); MRT_AT(MRTRowColumn, dst, 8); MRT_AT(MRTRowColumn, row_bytes, 16); MRT_AT(MRTRowColumn, _pad, 20);
// denoiser parameters (no counterpart in ShaderTypes.h)
static_assert(sizeof(MRTDenoiseParams) == 32, "MRTDenoiseParams is 32 bytes");
MRT_AT(MRTDenoiseParams, iterations, 0); MRT_AT(MRTDenoiseParams, sigma_color, 4); MRT_AT(MRTDenoiseParams, sigma_normal, 8);
MRT_AT(MRTDenoiseParams, sigma_depth, 12); MRT_AT(MRTDenoiseParams, demodulate, 16);
static_assert(sizeof(MRTReprojectParams) == 16, "MRTReprojectParams is 16 bytes");
MRT_AT(MRTReprojectParams, max_history, 0); MRT_AT(MRTReprojectParams, min_cos_normal, 4); MRT_AT(MRTReprojectParams, depth_tolerance, 8);
#undef MRT_AT
