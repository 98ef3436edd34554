// surface_host.cpp — query -> resolve on device buffers through the C++ host mirror (mrt::Renderer::intersectClosestDevice / resolveHitsDevice).
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/surface_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o surface_host
//   ./surface_host side          the Cornell box (plane.obj x 5 + sphere.obj); side x side rays from (0, 1, 3) through a grid at z = 1; prints hits and a checksum of the
//                                MRTSurface records (the floats summed in double in record order, the ids as integers)
#include <cstdio>
#include <cstdlib>
#include <hip/hip_runtime_api.h>
#include "mrt.hpp"

struct CornellScene : mrt::Scene {          // the plumbing scene of the Python mirror (CornellScene): one area light
    CornellScene(int w, int h) : mrt::Scene(w, h) {
        const float pi = 3.14159274f, hp = 1.57079637f;
        models.emplace_back("plane", std::initializer_list<float>{0, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{0, 2, 0}, std::initializer_list<float>{pi, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{0, 1, -1}, std::initializer_list<float>{hp, 0, 0}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{-1, 1, 0}, std::initializer_list<float>{0, 0, -hp}, 1.0f);
        models.emplace_back("plane", std::initializer_list<float>{1, 1, 0}, std::initializer_list<float>{0, 0, hp}, 1.0f);
        models.emplace_back("sphere", std::initializer_list<float>{0, 0.5f, 0}, 0.5f);
        lights = {setupLight()};
    }
};

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: surface_host side\n"); return 2; }
    const int side = atoi(argv[1]);
    if (side < 1 || side > 4096) { fprintf(stderr, "side must be 1 .. 4096\n"); return 2; }
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        CornellScene scene(64, 64);
        mrt::Renderer renderer(64, 64, scene);
        const size_t n = (size_t)side * side;
        std::vector<MRTRay> rays(n);
        for (int y = 0; y < side; y++)
            for (int x = 0; x < side; x++) {          // every number below is a dyadic rational: the same floats in any language
                MRTRay &r = rays[(size_t)y * side + x];
                r.origin[0] = 0.0f; r.origin[1] = 1.0f; r.origin[2] = 3.0f; r.min_distance = 0.0f;
                r.direction[0] = ((float)(2 * x + 1) / (float)side - 1.0f) * 1.25f; r.direction[1] = ((float)(2 * y + 1) / (float)side - 1.0f) * 1.25f; r.direction[2] = -2.0f;
                r.max_distance = INFINITY;
            }
        void *d_rays = nullptr, *d_hits = nullptr, *d_surf = nullptr;
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection))); HIP_OK(hipMalloc(&d_surf, n * sizeof(MRTSurface)));
        HIP_OK(hipMemcpy(d_rays, rays.data(), n * sizeof(MRTRay), hipMemcpyHostToDevice));
        void *stream = renderer.stream();
        renderer.intersectClosestDevice(d_rays, n, d_hits, stream);
        renderer.resolveHitsDevice(d_rays, d_hits, n, d_surf, stream);          // ordered behind the query by the stream: no wait in between
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        std::vector<MRTSurface> surf(n);
        HIP_OK(hipMemcpy(surf.data(), d_surf, n * sizeof(MRTSurface), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_rays)); HIP_OK(hipFree(d_hits)); HIP_OK(hipFree(d_surf));
        double sum = 0.0; long long ids = 0; size_t hits = 0;
        for (const MRTSurface &s : surf) {
            for (int k = 0; k < 3; k++) sum += (double)s.position[k];
            sum += (double)s.distance;
            for (int k = 0; k < 3; k++) sum += (double)s.normal[k];
            for (int k = 0; k < 3; k++) sum += (double)s.base_color[k];
            ids += (long long)s.type + s.resource_slot + s.instance_id + s.geometry_id + s.primitive_id;
            hits += s.type == 1;
        }
        const std::vector<uint64_t> offs = renderer.vertexOffsets();
        printf("rays=%zu hits=%zu ids=%lld vertices=%llu checksum=%.17g\n", n, hits, ids, (unsigned long long)offs.back(), sum);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
