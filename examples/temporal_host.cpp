// temporal_host.cpp — temporal reprojection of the accumulated image through the C++ host mirror (mrt::Renderer::reprojectDevice): two frames with a camera move between
// them.  Per frame: generate -> closest -> resolve give the bounce-0 surface rows, reprojectDevice blends the frame's sample with the history fetched where each surface
// point was a frame ago, and foldGuidesDevice(frame 0) leaves the frame's own guide entries for the next one — all on one stream.  The sample is any image this program
// holds, here one frame drawn by the renderer with the frame's camera.
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/temporal_host.cpp -Lmetal-raytracing_amd -lmrt_hip -L/opt/rocm/lib -lamdhip64 -o temporal_host
//   ./temporal_host width height out.bin     the Cornell box, seed 1; out.bin = the history {rgb, length} after frame 0 and after frame 1 (w*h*16 bytes each)
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
    if (argc < 4) { fprintf(stderr, "usage: temporal_host width height out.bin\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]);
    if (w < 1 || h < 1 || w > 4096 || h > 4096) { fprintf(stderr, "width and height must be 1 .. 4096\n"); return 2; }
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        CornellScene scene(w, h);
        mrt::Renderer renderer(w, h, scene, 0, 1);
        const size_t n = (size_t)w * h, image = n * 16;
        void *d_rays = nullptr, *d_index = nullptr, *d_hits = nullptr, *d_surf = nullptr, *d_nd = nullptr, *d_alb = nullptr, *d_ids = nullptr, *d_sample = nullptr, *d_hist[2] = {nullptr, nullptr};
        HIP_OK(hipMalloc(&d_rays, n * sizeof(MRTRay))); HIP_OK(hipMalloc(&d_index, n * sizeof(int32_t))); HIP_OK(hipMalloc(&d_hits, n * sizeof(MRTIntersection)));
        HIP_OK(hipMalloc(&d_surf, n * sizeof(MRTSurface))); HIP_OK(hipMalloc(&d_nd, image)); HIP_OK(hipMalloc(&d_alb, image)); HIP_OK(hipMalloc(&d_ids, image));
        HIP_OK(hipMalloc(&d_sample, image)); HIP_OK(hipMalloc(&d_hist[0], image)); HIP_OK(hipMalloc(&d_hist[1], image));
        HIP_OK(hipMemset(d_hist[0], 0, image));                                 // zeros: no history (length 0 is below 1) ...
        HIP_OK(hipMemset(d_nd, 0, image)); HIP_OK(hipMemset(d_ids, 0, image));  // ... and no previous frame: every entry is off
        void *stream = renderer.stream();
        std::vector<float> out;
        mrt::Camera prev = scene.camera;
        for (int f = 0; f < 2; f++) {
            mrt::Camera cam = scene.camera;
            cam.position.x += 0.05f * (float)f; cam.forward.x -= 0.02f * (float)f;          // the move: a step to the right, turning a little to the left
            MRTUniforms u = renderer.uniforms();
            u.camera = cam; u.frameIndex = 0;
            renderer.setUniforms(u);
            renderer.draw(1);                                                   // this frame's sample: one frame with this camera
            renderer.wait();
            const std::vector<float> sample = renderer.accumulation();
            HIP_OK(hipMemcpy(d_sample, sample.data(), image, hipMemcpyHostToDevice));
            renderer.primaryRaysDevice(0, d_rays, d_index, stream);             // each call is ordered behind the one before by the stream: no wait in between
            renderer.intersectClosestDevice(d_rays, n, d_hits, stream);
            renderer.resolveHitsDevice(d_rays, d_hits, n, d_surf, stream);
            renderer.reprojectDevice(cam, prev, d_surf, nullptr, d_nd, d_ids, d_hist[f & 1], d_sample, d_hist[(f + 1) & 1], nullptr, stream);          // the scene stands still: no previous positions
            renderer.foldGuidesDevice(d_surf, d_nd, d_alb, d_ids, 0, stream);   // frame index 0 every frame: this frame's own entries, not averages
            HIP_OK(hipStreamSynchronize((hipStream_t)stream));
            std::vector<float> hist(n * 4);
            HIP_OK(hipMemcpy(hist.data(), d_hist[(f + 1) & 1], image, hipMemcpyDeviceToHost));
            out.insert(out.end(), hist.begin(), hist.end());
            prev = cam;
        }
        for (void *p : {d_rays, d_index, d_hits, d_surf, d_nd, d_alb, d_ids, d_sample, d_hist[0], d_hist[1]}) HIP_OK(hipFree(p));
        size_t kept = 0;
        for (size_t i = 0; i < n; i++) kept += out[(n + i) * 4 + 3] > 1.0f;
        FILE *fp = fopen(argv[3], "wb");
        if (!fp) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        fwrite(out.data(), 4, out.size(), fp);
        fclose(fp);
        printf("two frames %dx%d with a camera move: %zu of %zu pixels kept their history\n", w, h, kept, n);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
