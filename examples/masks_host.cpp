// masks_host.cpp — visibility masks through the C++ host mirror (mrt::Scene::setMeshMasks / intersectClosestMaskedDevice).
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/masks_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o masks_host
//   ./masks_host layers          `layers` (1 .. 31) unit quads at z = 1 .. layers, one mesh each, quad k with the mask 1 << k; layers + 1 rays along +z through (0.75, 0.25),
//                                ray j with the mask ~((1 << j) - 1): it may see the quads j .. layers - 1, so its closest hit is quad j at distance j + 1, and the last ray
//                                sees nothing.  ONE masked closest call with a mask per ray; prints the instance ids and the distances.
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime_api.h>
#include "mrt.hpp"

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: masks_host layers\n"); return 2; }
    const int layers = atoi(argv[1]);
    if (layers < 1 || layers > 31) { fprintf(stderr, "layers must be 1 .. 31\n"); return 2; }
    MRTContext ctx = nullptr; MRTScene scene = nullptr;
    int status = 0;
    try {
        mrt::check(mrt_context_create(0, &ctx));
        mrt::check(mrt_scene_create(ctx, &scene));
        const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const uint32_t indices[6] = {0, 1, 2, 0, 2, 3};
        mrt::Material material{};
        material.baseColor = mrt::f3(0.5f, 0.5f, 0.5f); material.dissolve = 1.0f; material.refractionIndex = 1.0f;
        std::vector<uint32_t> masks;
        for (int k = 0; k < layers; k++) {
            const float z = (float)(k + 1);
            const float positions[12] = {0, 0, z, 1, 0, z, 1, 1, z, 0, 1, z}, normals[12] = {0, 0, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1};
            int32_t id = -1;
            mrt::check(mrt_scene_add_mesh(scene, positions, 12, normals, 12, 4, identity, &id));
            mrt::check(mrt_mesh_add_submesh(scene, id, indices, 2, &material, nullptr));
            masks.push_back(1u << k);
        }
        mrt::Scene::setMeshMasks(scene, 0, masks);          // before the commit; after it works the same and needs no second commit
        mrt::check(mrt_scene_commit(scene));
        if (mrt::Scene::meshMasks(scene, 0, layers) != masks) { fprintf(stderr, "the masks did not survive the commit\n"); status = 1; }
        const size_t n = (size_t)layers + 1;
        std::vector<MRTRay> rays(n);
        std::vector<uint32_t> ray_masks(n);
        for (size_t j = 0; j < n; j++) {
            MRTRay &r = rays[j];
            r.origin[0] = 0.75f; r.origin[1] = 0.25f; r.origin[2] = 0.0f; r.min_distance = 0.0f;
            r.direction[0] = 0.0f; r.direction[1] = 0.0f; r.direction[2] = 1.0f; r.max_distance = INFINITY;
            ray_masks[j] = ~((1u << j) - 1u);
        }
        void *d_rays = nullptr, *d_masks = nullptr, *d_hits = nullptr, *stream = nullptr;
        mrt::check(mrt_context_get_stream(ctx, &stream));
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_masks, n * 4)); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection)));
        HIP_OK(hipMemcpy(d_rays, rays.data(), n * sizeof(MRTRay), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_masks, ray_masks.data(), n * 4, hipMemcpyHostToDevice));
        mrt::Scene::intersectClosestMaskedDevice(scene, d_rays, d_masks, 0u, n, d_hits, stream);
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        std::vector<MRTIntersection> hits(n);
        HIP_OK(hipMemcpy(hits.data(), d_hits, n * sizeof(MRTIntersection), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_rays)); HIP_OK(hipFree(d_masks)); HIP_OK(hipFree(d_hits));
        printf("ids=");
        for (const MRTIntersection &h : hits) printf("%d ", h.instance_id);
        printf("distances=");
        for (const MRTIntersection &h : hits) printf("%g ", h.distance);
        printf("\n");
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        status = 1;
    }
    if (scene) mrt_scene_destroy(scene);
    if (ctx) mrt_context_destroy(ctx);
    return status;
}
