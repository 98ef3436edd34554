// image_stages_host.cpp — guide buffers, denoiser and tonemap as stages on device buffers through the C++ host mirror (mrt::Renderer::foldGuidesDevice / denoiseDevice /
// tonemapDevice): the guides folded frame by frame from the bounce-0 surface rows — generate -> closest -> resolve -> fold, four calls on one stream and no second walk of
// the primary rays — then the filter and the tonemap applied to an image this program holds, here the renderer's accumulation after the same frames.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/image_stages_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o image_stages_host
//   ./image_stages_host width height frames out.bin     the Cornell box, seed 1; out.bin = normal|depth, albedo, ids, denoised (w*h*16 bytes each), RGBA8 (w*h*4)
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
    if (argc < 5) { fprintf(stderr, "usage: image_stages_host width height frames out.bin\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), frames = atoi(argv[3]);
    if (w < 1 || h < 1 || w > 4096 || h > 4096 || frames < 1) { fprintf(stderr, "width and height must be 1 .. 4096, frames at least 1\n"); return 2; }
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        CornellScene scene(w, h);
        mrt::Renderer renderer(w, h, scene, 0, 1);
        const size_t n = (size_t)w * h, image = n * 16, work = renderer.denoiseWorkspaceBytes();
        void *d_rays = nullptr, *d_index = nullptr, *d_hits = nullptr, *d_surf = nullptr, *d_nd = nullptr, *d_alb = nullptr, *d_ids = nullptr, *d_accum = nullptr, *d_work = nullptr,
             *d_den = nullptr, *d_rgba = nullptr;
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_index, n * sizeof(int32_t))); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection)));
        HIP_OK(hipMalloc(&d_surf, n * sizeof(MRTSurface))); HIP_OK(hipMalloc(&d_nd, image)); HIP_OK(hipMalloc(&d_alb, image)); HIP_OK(hipMalloc(&d_ids, image));
        HIP_OK(hipMalloc(&d_accum, image)); HIP_OK(hipMalloc(&d_work, work)); HIP_OK(hipMalloc(&d_den, image)); HIP_OK(hipMalloc(&d_rgba, n * 4));
        void *stream = renderer.stream();
        for (int f = 0; f < frames; f++) {                                      // each call is ordered behind the one before by the stream: no wait in between
            renderer.primaryRaysDevice((uint32_t)f, d_rays, d_index, stream);
            renderer.intersectClosestDevice(d_rays, n, d_hits, stream);
            renderer.resolveHitsDevice(d_rays, d_hits, n, d_surf, stream);
            renderer.foldGuidesDevice(d_surf, d_nd, d_alb, d_ids, (uint32_t)f, stream);          // frame 0 replaces: the buffers need no clearing
        }
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        renderer.draw(frames);
        renderer.wait();
        const std::vector<float> accum = renderer.accumulation();               // any image will do: a composed frame, a gathered one
        HIP_OK(hipMemcpy(d_accum, accum.data(), image, hipMemcpyHostToDevice));
        renderer.denoiseDevice(d_accum, d_nd, d_alb, d_work, work, d_den, nullptr, stream);       // default parameters
        renderer.tonemapDevice(d_den, d_rgba, stream);
        HIP_OK(hipStreamSynchronize((hipStream_t)stream));
        std::vector<float> nd(n * 4), alb(n * 4), den(n * 4); std::vector<int32_t> ids(n * 4); std::vector<uint8_t> rgba(n * 4);
        HIP_OK(hipMemcpy(nd.data(), d_nd, image, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(alb.data(), d_alb, image, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(ids.data(), d_ids, image, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(den.data(), d_den, image, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(rgba.data(), d_rgba, n * 4, hipMemcpyDeviceToHost));
        for (void *p : {d_rays, d_index, d_hits, d_surf, d_nd, d_alb, d_ids, d_accum, d_work, d_den, d_rgba}) HIP_OK(hipFree(p));
        FILE *f = fopen(argv[4], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
        fwrite(nd.data(), 4, nd.size(), f); fwrite(alb.data(), 4, alb.size(), f); fwrite(ids.data(), 4, ids.size(), f);
        fwrite(den.data(), 4, den.size(), f); fwrite(rgba.data(), 1, rgba.size(), f);
        fclose(f);
        printf("guides folded from %d frames of surface rows, denoised and tonemapped %dx%d\n", frames, w, h);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
