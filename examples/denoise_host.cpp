// denoise_host.cpp — the guide buffers and the denoiser through the C++ host mirror (mrt::Renderer::guides / denoise / denoisedTonemapped).
//   c++ -std=c++17 -Iinclude examples/denoise_host.cpp -Lmetal-raytracing_amd -lmrt_hip -o denoise_host
//   ./denoise_host width height frames out.bin     DragonScene; out.bin = normal|depth, albedo, ids, denoised (w*h*16 bytes each), tonemapped (w*h*4)
#include <cstdio>
#include <cstdlib>
#include "mrt.hpp"

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: denoise_host width height frames out.bin\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), frames = atoi(argv[3]);
    if (const char *res = getenv("MRT_RESOURCES")) mrt::resourceDirectory() = res;
    try {
        mrt::DragonScene scene(w, h);
        mrt::Renderer renderer(w, h, scene);
        renderer.setOption("guides", 1);
        renderer.draw(frames);
        renderer.wait();
        const mrt::Renderer::Guides g = renderer.guides();
        const std::vector<float> den = renderer.denoise();            // default parameters
        const std::vector<uint8_t> img = renderer.denoisedTonemapped();
        FILE *f = fopen(argv[4], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
        fwrite(g.normalDepth.data(), 4, g.normalDepth.size(), f); fwrite(g.albedo.data(), 4, g.albedo.size(), f); fwrite(g.ids.data(), 4, g.ids.size(), f);
        fwrite(den.data(), 4, den.size(), f); fwrite(img.data(), 1, img.size(), f);
        fclose(f);
        printf("guides + denoised %dx%d after %d frames\n", w, h, frames);
    } catch (const mrt::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
