// materials_host.cpp — one bounce of the composed loop with the materials extension on, through the C++ host mirror: generate -> closest -> resolve -> scatter with
// materials -> any, five calls on one stream (mrt::Renderer::primaryRaysDevice / intersectClosestDevice / resolveHitsDevice / scatterMaterialsDevice / intersectAnyDevice).
// At bounce 0 the throughput is 1: the radiance so far is the lobe row's emission plus the light row where the shadow ray got through, and the lobe row's weight is the
// throughput the next bounce starts with.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/materials_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o materials_host
//   ./materials_host width height     the Cornell box's five walls with a glass sphere, a glossy sphere and an emitting quad, seed 1, sample index 0, max_bounces 4; prints
//                                     how many rows took each lobe (0 none, 1 diffuse, 2 / 3 interface reflected / refracted, 4 specular, 5 absorbed), the shadow rays
//                                     wanted, those that got through and a checksum of the light rows, the continuation rays and the lobe rows (four, seven and six floats
//                                     per pixel summed in double in row order; the ray's max_distance, +inf, and the integer words are left out)
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime_api.h>
#include "mrt.hpp"

static void set3(MRTFloat3 &v, float x, float y, float z) { v.x = x; v.y = y; v.z = z; }

struct MaterialsScene : mrt::Scene {          // the Python tests' cornell_with_materials: one area light
    MaterialsScene(int w, int h) : mrt::Scene(w, h) {
        const float pi = 3.14159274f, hp = 1.57079637f;
        models.emplace_back("plane", std::initializer_list<float>{0, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{0, 2, 0}, std::initializer_list<float>{pi, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{0, 1, -1}, std::initializer_list<float>{hp, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{-1, 1, 0}, std::initializer_list<float>{0, 0, -hp}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{1, 1, 0}, std::initializer_list<float>{0, 0, hp}, 1.0f);
        models.emplace_back("sphere", std::initializer_list<float>{-0.45f, 0.35f, 0.35f}, 0.35f);                                       // glass
        models.emplace_back("sphere", std::initializer_list<float>{0.45f, 0.3f, -0.1f}, 0.3f);                                          // glossy
        models.emplace_back("plane", std::initializer_list<float>{0.99f, 1.0f, 0.2f}, std::initializer_list<float>{0, 0, hp}, 0.25f);   // lamp
        for (mrt::Mesh &m : models[5].meshes) for (mrt::Submesh &s : m.submeshes) { s.material.dissolve = 0.15f; s.material.refractionIndex = 1.5f; set3(s.material.baseColor, 0.9f, 0.9f, 0.9f); }
        for (mrt::Mesh &m : models[6].meshes) for (mrt::Submesh &s : m.submeshes) { set3(s.material.specular, 0.8f, 0.7f, 0.3f); s.material.specularExponent = 96.0f; set3(s.material.baseColor, 0.2f, 0.1f, 0.05f); }
        for (mrt::Mesh &m : models[7].meshes) for (mrt::Submesh &s : m.submeshes) set3(s.material.emission, 2.0f, 1.5f, 0.5f);
        lights = {setupLight()};
    }
};

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: materials_host width height\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]);
    if (w < 1 || h < 1 || w > 4096 || h > 4096) { fprintf(stderr, "width and height must be 1 .. 4096\n"); return 2; }
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        const int maxBounces = 4;
        MaterialsScene scene(w, h);
        mrt::Renderer renderer(w, h, scene, 0, 1, maxBounces);
        const size_t n = (size_t)w * h;
        void *d_rays = nullptr, *d_index = nullptr, *d_hits = nullptr, *d_surf = nullptr, *d_shadow = nullptr, *d_light = nullptr, *d_next = nullptr, *d_lobes = nullptr, *d_occ = nullptr;
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_index, n * sizeof(int32_t))); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection)));
        HIP_OK(hipMalloc(&d_surf, n * sizeof(MRTSurface))); HIP_OK(hipMalloc(&d_shadow, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_light, n * 4 * sizeof(float)));
        HIP_OK(hipMalloc(&d_next, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_lobes, n * sizeof(MRTScatterLobe))); HIP_OK(hipMalloc(&d_occ, n * sizeof(int32_t)));
        void *stream = renderer.stream();
        renderer.primaryRaysDevice(0, d_rays, d_index, stream);                 // each call is ordered behind the one before by the stream: no wait in between
        renderer.intersectClosestDevice(d_rays, n, d_hits, stream);
        renderer.resolveHitsDevice(d_rays, d_hits, n, d_surf, stream);
        renderer.scatterMaterialsDevice(d_rays, d_surf, d_index, n, 0, maxBounces, 0, d_shadow, d_light, d_next, d_lobes, stream);
        renderer.intersectAnyDevice(d_shadow, n, d_occ, stream);
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        std::vector<float> light(n * 4); std::vector<MRTRay> next(n); std::vector<MRTScatterLobe> lobes(n); std::vector<int32_t> occ(n);
        HIP_OK(hipMemcpy(light.data(), d_light, n * 4 * sizeof(float), hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(next.data(), d_next, n * sizeof(MRTRay), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(lobes.data(), d_lobes, n * sizeof(MRTScatterLobe), hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(occ.data(), d_occ, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (void *p : {d_rays, d_index, d_hits, d_surf, d_shadow, d_light, d_next, d_lobes, d_occ}) HIP_OK(hipFree(p));
        double sum = 0.0; size_t count[6] = {0, 0, 0, 0, 0, 0}, wanted = 0, lit = 0;
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 4; k++) sum += (double)light[4 * i + k];
            for (int k = 0; k < 3; k++) sum += (double)next[i].origin[k];
            sum += (double)next[i].min_distance;
            for (int k = 0; k < 3; k++) sum += (double)next[i].direction[k];
            for (int k = 0; k < 3; k++) sum += (double)lobes[i].weight[k];
            for (int k = 0; k < 3; k++) sum += (double)lobes[i].emission[k];
            if (lobes[i].lobe < 0 || lobes[i].lobe > 5) { fprintf(stderr, "row %zu: lobe %d\n", i, lobes[i].lobe); return 1; }
            count[lobes[i].lobe]++;
            const bool want = light[4 * i + 3] == 1.0f;          // go by the light row, never by the answer for a zero ray
            wanted += want; lit += want && occ[i] == 0;
        }
        printf("pixels=%zu lobes=%zu,%zu,%zu,%zu,%zu,%zu wanted=%zu lit=%zu checksum=%.17g\n", n, count[0], count[1], count[2], count[3], count[4], count[5], wanted, lit, sum);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
