// integrator_host.cpp — one frame of the composed loop at bounce 0 through the C++ host mirror: generate -> closest -> resolve -> scatter -> any, five calls on one stream
// (mrt::Renderer::primaryRaysDevice / intersectClosestDevice / resolveHitsDevice / scatterDevice / intersectAnyDevice).  Bounce 0 alone needs no element-wise kernel of the
// caller's: the throughput is 1 and the radiance is the light row where the shadow ray got through.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/integrator_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o integrator_host
//   ./integrator_host width height     the Cornell box (plane.obj x 5 + sphere.obj), seed 1, sample index 0; prints the surfaces hit, the shadow rays wanted, those that got
//                                      through and a checksum of the light rows and the bounce rays (four and seven floats per pixel summed in double in row order; the bounce
//                                      ray's max_distance, +inf, is left out)
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
    if (argc < 3) { fprintf(stderr, "usage: integrator_host width height\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]);
    if (w < 1 || h < 1 || w > 4096 || h > 4096) { fprintf(stderr, "width and height must be 1 .. 4096\n"); return 2; }
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        CornellScene scene(w, h);
        mrt::Renderer renderer(w, h, scene, 0, 1);
        const size_t n = (size_t)w * h;
        void *d_rays = nullptr, *d_index = nullptr, *d_hits = nullptr, *d_surf = nullptr, *d_shadow = nullptr, *d_light = nullptr, *d_next = nullptr, *d_occ = nullptr;
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_index, n * sizeof(int32_t))); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection)));
        HIP_OK(hipMalloc(&d_surf, n * sizeof(MRTSurface))); HIP_OK(hipMalloc(&d_shadow, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_light, n * 4 * sizeof(float)));
        HIP_OK(hipMalloc(&d_next, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_occ, n * sizeof(int32_t)));
        void *stream = renderer.stream();
        renderer.primaryRaysDevice(0, d_rays, d_index, stream);                 // each call is ordered behind the one before by the stream: no wait in between
        renderer.intersectClosestDevice(d_rays, n, d_hits, stream);
        renderer.resolveHitsDevice(d_rays, d_hits, n, d_surf, stream);
        renderer.scatterDevice(d_surf, d_index, n, 0, 0, d_shadow, d_light, d_next, stream);
        renderer.intersectAnyDevice(d_shadow, n, d_occ, stream);
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        std::vector<MRTSurface> surf(n); std::vector<float> light(n * 4); std::vector<MRTRay> next(n); std::vector<int32_t> occ(n);
        HIP_OK(hipMemcpy(surf.data(), d_surf, n * sizeof(MRTSurface), hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(light.data(), d_light, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(next.data(), d_next, n * sizeof(MRTRay), hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(occ.data(), d_occ, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (void *p : {d_rays, d_index, d_hits, d_surf, d_shadow, d_light, d_next, d_occ}) HIP_OK(hipFree(p));
        double sum = 0.0; size_t hits = 0, wanted = 0, lit = 0;
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 4; k++) sum += (double)light[4 * i + k];
            for (int k = 0; k < 3; k++) sum += (double)next[i].origin[k];
            sum += (double)next[i].min_distance;
            for (int k = 0; k < 3; k++) sum += (double)next[i].direction[k];
            hits += surf[i].type == 1;
            const bool want = light[4 * i + 3] == 1.0f;          // go by the light row, never by the answer for a zero ray
            wanted += want; lit += want && occ[i] == 0;
        }
        printf("pixels=%zu surfaces=%zu wanted=%zu lit=%zu checksum=%.17g\n", n, hits, wanted, lit, sum);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
