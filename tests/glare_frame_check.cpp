// A stand-alone host program for tests/test_glare_abi.py: gr_glare_frame, gr_glare_gaussians and gr_glare_exposure (csrc/imageio.cpp,
// compiled into this program) on heap buffers of exactly the frames' sizes, built with -fsanitize=address,undefined - a read or write one
// float past either frame ends the program.  Every case is also compared, bit for bit, with the definition written out again below (per
// output value: the rows pass of the n rows it looks at, then the columns pass, then the combine).  Among the cases: one pixel under 129
// taps, where the clamp binds on both sides of a row and of a column at once, and frames narrower and lower than the PSF.  Then the
// refusals, each of which must leave the destination as it was.  Prints one line per case and "ok".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include "../include/geodesic_hip_internal.h"

static std::string last_error;
extern "C" int gr_internal_fail(int code, const char* msg) {
    last_error = msg ? msg : "";
    return code;
}

static float next_value(unsigned& state) {   // (-2, 2), sixteen bits of mantissa
    state = state * 1664525u + 1013904223u;
    return ((int)(state >> 16) - 32768) / 16384.0f;
}

static int run(int width, int height, const gr_glare& made, const char* name) {
    const size_t floats = (size_t)width * height * 4;
    std::unique_ptr<float[]> src(new float[floats]), dst(new float[floats]);
    std::unique_ptr<gr_glare> g(new gr_glare(made));
    unsigned state = 12345u + 977u * width + 31u * height;
    for (size_t i = 0; i < floats; i++) src[i] = next_value(state);
    std::memset(dst.get(), 0xff, floats * sizeof(float));
    if (gr_glare_frame(src.get(), width, height, g.get(), dst.get()) != GR_OK) {
        std::printf("%s: refused: %s\n", name, last_error.c_str());
        return 1;
    }
    const long long w = width, h = height;
    size_t differing = 0;
    for (long long Y = 0; Y < h; Y++)
        for (long long X = 0; X < w; X++)
            for (int c = 0; c < 4; c++) {
                volatile float out = src[(size_t)((Y * w + X) * 4 + c)];
                if (c < 3) {
                    out = g->core * out;
                    for (int k = 0; k < g->components; k++) {
                        const int n = g->taps[k];
                        const long long radius = (n - 1) / 2;
                        volatile float column = 0;
                        for (int t = 0; t < n; t++) {
                            const long long cy = std::min(std::max(Y - radius + t, 0ll), h - 1);
                            volatile float row = 0;
                            for (int u = 0; u < n; u++) {
                                const long long cx = std::min(std::max(X - radius + u, 0ll), w - 1);
                                volatile float product = g->tap[k][u] * src[(size_t)((cy * w + cx) * 4 + c)];
                                row = u ? row + product : product;
                            }
                            volatile float product = g->tap[k][t] * row;
                            column = t ? column + product : product;
                        }
                        volatile float product = g->weight[k] * column;
                        out = out + product;
                    }
                }
                const float want = out, got = dst[(size_t)((Y * w + X) * 4 + c)];
                if (std::memcmp(&want, &got, sizeof want)) differing++;
            }
    std::printf("%s: %d x %d, %d components: %zu of %zu values differ\n", name, width, height, g->components, differing, floats);
    return differing ? 1 : 0;
}

static gr_glare with_tables(float core, int components, const float* weights, const int* counts, float scale) {
    gr_glare g;
    std::memset(&g, 0, sizeof g);
    g.core = core;
    g.components = components;
    for (int k = 0; k < components; k++) {
        g.weight[k] = weights[k];
        g.taps[k] = counts[k];
        for (int t = 0; t < counts[k]; t++) g.tap[k][t] = scale * (t + 2 + k) * ((t + k) % 4 == 2 ? -1.0f : 1.0f);   // distinct, asymmetric, of both signs
    }
    return g;
}

int main() {
    int failed = 0;
    const int sizes[][2] = {{1, 1}, {1, 3}, {3, 1}, {5, 3}, {67, 9}, {2, 33}};
    const float weights[4] = {0.3f, -0.2f, 0.05f, 1.0f};
    const int one15[1] = {15}, one129[1] = {129}, one3[1] = {3}, four[4] = {7, 129, 1, 15};
    std::unique_ptr<gr_glare> gaussians(new gr_glare);
    const float sigma[2] = {1.5f, 10.0f}, share[2] = {0.06f, 0.03f};
    if (gr_glare_gaussians(sigma, share, 2, gaussians.get()) != GR_OK || gaussians->taps[0] != 11 || gaussians->taps[1] != 61 ||
        gr_glare_exposure(gaussians.get(), 1.0f) != GR_OK || gaussians->weight[0] != 0.12f) {
        std::printf("gr_glare_gaussians / gr_glare_exposure: %s\n", last_error.c_str());
        return 1;
    }
    for (const auto& size : sizes) {
        failed += run(size[0], size[1], with_tables(1.75f, 0, weights, one3, 0.f), "gain");
        failed += run(size[0], size[1], with_tables(0.9f, 1, weights, one3, 0.1f), "three");
        failed += run(size[0], size[1], with_tables(-0.3f, 1, weights, one15, 0.013f), "uneven 15");
        failed += run(size[0], size[1], with_tables(0.0f, 1, weights, one129, 0.002f), "uneven 129");
        failed += run(size[0], size[1], *gaussians, "gaussians");
        failed += run(size[0], size[1], with_tables(0.8f, 4, weights, four, 0.004f), "four");
    }
    // a refusal writes nothing: the frame stays as it was
    {
        std::unique_ptr<float[]> src(new float[16]()), dst(new float[16]);
        std::memset(dst.get(), 0xff, 16 * sizeof(float));
        std::unique_ptr<gr_glare> good(new gr_glare(with_tables(0.9f, 1, weights, one3, 0.1f))), bad(new gr_glare(*good));
        int refused = 0, tried = 0;
        const auto refuses = [&](int rc) { tried++; if (rc != GR_OK && last_error.find("gr_glare_frame") != std::string::npos) refused++; };
        refuses(gr_glare_frame(nullptr, 2, 2, good.get(), dst.get()));
        refuses(gr_glare_frame(src.get(), 2, 2, nullptr, dst.get()));
        refuses(gr_glare_frame(src.get(), 0, 2, good.get(), dst.get()));
        refuses(gr_glare_frame(src.get(), 2, -3, good.get(), dst.get()));
        refuses(gr_glare_frame(dst.get(), 2, 2, good.get(), dst.get()));
        bad->components = 5;
        refuses(gr_glare_frame(src.get(), 2, 2, bad.get(), dst.get()));
        *bad = *good;
        bad->taps[0] = 4;
        refuses(gr_glare_frame(src.get(), 2, 2, bad.get(), dst.get()));
        bad->taps[0] = 131;
        refuses(gr_glare_frame(src.get(), 2, 2, bad.get(), dst.get()));
        *bad = *good;
        bad->tap[0][2] = std::numeric_limits<float>::quiet_NaN();
        refuses(gr_glare_frame(src.get(), 2, 2, bad.get(), dst.get()));
        *bad = *good;
        bad->core = std::numeric_limits<float>::infinity();
        refuses(gr_glare_frame(src.get(), 2, 2, bad.get(), dst.get()));
        int wrote = 0;
        for (int i = 0; i < 16; i++) {
            unsigned bits;
            std::memcpy(&bits, &dst[i], 4);
            if (bits != 0xffffffffu) wrote++;
        }
        std::printf("refusals: %d wrote, %d of %d refused\n", wrote, refused, tried);
        if (wrote || refused != tried) failed++;
    }
    if (failed) {
        std::printf("%d cases failed\n", failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
