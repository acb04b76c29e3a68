// A stand-alone host program for tests/test_filter_abi.py: gr_filter_frame and gr_filter_taps (csrc/imageio.cpp, compiled into this
// program) on heap buffers of exactly the frames' sizes, built with -fsanitize=address,undefined - a read or write one float past either
// frame, or past the table, ends the program.  Every case is also compared, bit for bit, with the definition written out again below
// (per output value: the rows pass of the n traced rows it looks at, then the columns pass).  Among the cases: width 1 at factor 4 with 16
// taps, where W f < n and the clamp binds on both sides of a row at once, and height 1 alike.  Prints one line per case and "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static int run(int width, int height, int factor, const float* table, int count, const char* name) {
    const long long sw = (long long)width * factor, sh = (long long)height * factor;
    const size_t src_floats = (size_t)(sw * sh * 4), dst_floats = (size_t)width * height * 4;
    std::unique_ptr<float[]> src(new float[src_floats]), dst(new float[dst_floats]), taps(new float[count]);
    unsigned state = 12345u + 977u * width + 31u * height + factor;
    for (size_t i = 0; i < src_floats; i++) src[i] = next_value(state);
    std::copy(table, table + count, taps.get());
    std::memset(dst.get(), 0xff, dst_floats * sizeof(float));
    if (gr_filter_frame(src.get(), width, height, factor, taps.get(), count, dst.get()) != GR_OK) {
        std::printf("%s: refused: %s\n", name, last_error.c_str());
        return 1;
    }
    const long long first = (factor - count) / 2;
    size_t differing = 0;
    for (long long Y = 0; Y < height; Y++)
        for (long long X = 0; X < width; X++)
            for (int c = 0; c < 4; c++) {
                volatile float out = 0;
                for (int t = 0; t < count; t++) {
                    const long long cy = std::min(std::max(Y * factor + first + t, 0ll), sh - 1);
                    volatile float h = 0;
                    for (int u = 0; u < count; u++) {
                        const long long cx = std::min(std::max(X * factor + first + u, 0ll), sw - 1);
                        volatile float product = taps[u] * src[(size_t)((cy * sw + cx) * 4 + c)];
                        h = u ? h + product : product;
                    }
                    volatile float product = taps[t] * h;
                    out = t ? out + product : product;
                }
                const float want = out, got = dst[(size_t)((Y * width + X) * 4 + c)];
                if (std::memcmp(&want, &got, sizeof want)) differing++;
            }
    std::printf("%s: %d x %d at factor %d, %d taps: %zu of %zu values differ\n", name, width, height, factor, count, differing, dst_floats);
    return differing ? 1 : 0;
}

int main() {
    int failed = 0;
    const int sizes[][2] = {{1, 1}, {1, 3}, {3, 1}, {5, 3}, {67, 9}, {2, 33}};
    const char* names[] = {"box", "tent", "gaussian", "mitchell"};
    for (int filter = GR_FILTER_TENT; filter <= GR_FILTER_MITCHELL; filter++)
        for (int factor = 1; factor <= 4; factor++) {
            std::unique_ptr<float[]> taps(new float[GR_FILTER_MAX_TAPS]);   // exactly the 16 floats the declaration promises
            int count = 0;
            if (gr_filter_taps(filter, factor, taps.get(), &count) != GR_OK) {
                std::printf("gr_filter_taps(%d, %d): %s\n", filter, factor, last_error.c_str());
                return 1;
            }
            for (const auto& size : sizes) failed += run(size[0], size[1], factor, taps.get(), count, names[filter]);
        }
    float uneven[16];
    for (int t = 0; t < 16; t++) uneven[t] = 0.01f * (t + 1) * (t % 3 == 1 ? -1.0f : 1.0f);
    failed += run(1, 1, 4, uneven, 16, "uneven");   // W f = 4 < n = 16: both ends of a row clamp
    failed += run(3, 2, 4, uneven, 16, "uneven");
    failed += run(2, 3, 3, uneven, 15, "uneven");
    failed += run(4, 4, 2, uneven, 2, "uneven");
    // a refusal writes nothing: the frame stays as it was
    {
        std::unique_ptr<float[]> src(new float[16]()), dst(new float[4]);
        std::memset(dst.get(), 0xff, 4 * sizeof(float));
        const float one = 1.0f;
        if (gr_filter_frame(src.get(), 1, 1, 2, &one, 1, dst.get()) == GR_OK || last_error.find("gr_filter_frame") == std::string::npos) failed++;
        for (int i = 0; i < 4; i++) {
            unsigned bits;
            std::memcpy(&bits, &dst[i], 4);
            if (bits != 0xffffffffu) failed++;
        }
    }
    if (failed) {
        std::printf("%d cases failed\n", failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
