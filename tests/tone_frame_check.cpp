// A stand-alone host program for tests/test_tone_abi.py: gr_meter_histogram_frame, gr_meter_solve_host and gr_tone_frame (csrc/imageio.cpp,
// compiled into this program) on heap buffers of exactly the frames' and the histogram's sizes, built with -fsanitize=address,undefined - a
// read or write one word past a frame or past the 385 counters ends the program.  Every case is also compared with the definition written
// out again below: the counts one by one, the curve bit for bit, out of place and in place.  Then the refusals, each of which must leave
// its destinations as they were.  Prints one line per case and "ok".
#include <cmath>
#include <cstdint>
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

static float next_value(unsigned& state) {   // 2^-30 ... 2^30 of both signs, some zeros, infinities and NaN
    state = state * 1664525u + 1013904223u;
    const unsigned kind = (state >> 8) % 64;
    if (kind == 0) return 0.f;
    if (kind == 1) return -0.f;
    if (kind == 2) return std::numeric_limits<float>::infinity();
    if (kind == 3) return std::numeric_limits<float>::quiet_NaN();
    const float magnitude = std::ldexp(1.f + (float)((state >> 16) & 0xffff) / 65536.f, (int)((state >> 3) % 61) - 30);
    return kind == 4 ? -magnitude : magnitude;
}

static uint32_t bits_of(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static float curve_again(float c, float gain, int curve, float white) {
    volatile float v = gain * c;
    volatile float x = v > 0.f ? (v < 16777216.f ? v : 16777216.f) : 0.f;
    if (curve == GR_TONE_REINHARD) {
        const float iw2 = (float)(1.0 / ((double)white * (double)white));
        volatile float a = x * iw2;
        volatile float one_a = 1.f + a;
        volatile float n = x * one_a;
        volatile float d = 1.f + x;
        volatile float y = n / d;
        return y;
    }
    if (curve == GR_TONE_FILMIC) {
        volatile float n1 = 2.51f * x;
        volatile float n2 = n1 + 0.03f;
        volatile float n = x * n2;
        volatile float d1 = 2.43f * x;
        volatile float d2 = d1 + 0.59f;
        volatile float d3 = x * d2;
        volatile float d = d3 + 0.14f;
        volatile float y = n / d;
        return y < 1.f ? y : 1.f;
    }
    return x;
}

static int run(int width, int height, int curve) {
    const size_t pixels = (size_t)width * height, floats = pixels * 4;
    std::unique_ptr<float[]> src(new float[floats]), dst(new float[floats]);
    std::unique_ptr<unsigned[]> hist(new unsigned[GR_METER_COUNTERS]), again(new unsigned[GR_METER_COUNTERS]());
    std::unique_ptr<gr_tone> tone(new gr_tone);
    unsigned state = 4321u + 977u * width + 31u * height + curve;
    for (size_t i = 0; i < floats; i++) src[i] = next_value(state);
    gr_tone_default(tone.get());
    tone->mode = GR_TONE_AUTO;
    tone->curve = curve;
    tone->white = 2.5f;
    std::memset(hist.get(), 0xff, GR_METER_COUNTERS * sizeof(unsigned));
    if (gr_meter_histogram_frame(src.get(), width, height, hist.get()) != GR_OK) {
        std::printf("refused: %s\n", last_error.c_str());
        return 1;
    }
    size_t differing = 0;
    for (size_t i = 0; i < pixels; i++) {
        volatile float yr = 0.2126f * src[4 * i], yg = 0.7152f * src[4 * i + 1], yb = 0.0722f * src[4 * i + 2];
        volatile float yrg = yr + yg;
        volatile float y = yrg + yb;
        if (!(y > 0.f)) { again[GR_METER_BINS]++; continue; }
        const int e = (int)(bits_of(y) >> 20) - 824;
        again[e < 0 ? 0 : e > GR_METER_BINS - 1 ? GR_METER_BINS - 1 : e]++;
    }
    for (int b = 0; b < GR_METER_COUNTERS; b++) differing += hist[b] != again[b];
    double adapted = 0.0;
    int primed = 0, q = 0;
    float gain = 0.f;
    if (gr_meter_solve_host(hist.get(), tone.get(), &adapted, &primed, &gain, &q) != GR_OK || !(gain > 0.f) || !std::isfinite(gain)) {
        std::printf("solve: %s\n", last_error.c_str());
        return 1;
    }
    std::memset(dst.get(), 0xff, floats * sizeof(float));
    if (gr_tone_frame(src.get(), width, height, tone.get(), gain, dst.get()) != GR_OK) {
        std::printf("refused: %s\n", last_error.c_str());
        return 1;
    }
    for (size_t i = 0; i < floats; i++) {
        const float want = i % 4 == 3 ? src[i] : curve_again(src[i], gain, curve, tone->white);
        if (i % 4 == 3 ? bits_of(src[i]) != bits_of(dst[i]) : bits_of(want) != bits_of(dst[i])) differing++;
    }
    // in place
    std::unique_ptr<float[]> same(new float[floats]);
    std::memcpy(same.get(), src.get(), floats * sizeof(float));
    if (gr_tone_frame(same.get(), width, height, tone.get(), gain, same.get()) != GR_OK || std::memcmp(same.get(), dst.get(), floats * sizeof(float))) differing++;
    std::printf("curve %d: %d x %d, %d sixteenths: %zu differ\n", curve, width, height, q, differing);
    return differing ? 1 : 0;
}

int main() {
    int failed = 0;
    const int sizes[][2] = {{1, 1}, {1, 3}, {3, 1}, {5, 3}, {67, 9}, {2, 33}};
    for (const auto& size : sizes)
        for (int curve : {GR_TONE_LINEAR, GR_TONE_REINHARD, GR_TONE_FILMIC}) failed += run(size[0], size[1], curve);
    // a refusal writes nothing
    {
        std::unique_ptr<float[]> src(new float[16]()), dst(new float[16]);
        std::unique_ptr<unsigned[]> hist(new unsigned[GR_METER_COUNTERS]);
        std::memset(dst.get(), 0xff, 16 * sizeof(float));
        std::memset(hist.get(), 0xff, GR_METER_COUNTERS * sizeof(unsigned));
        std::unique_ptr<gr_tone> good(new gr_tone), bad(new gr_tone);
        gr_tone_default(good.get());
        good->mode = GR_TONE_AUTO;
        double adapted = 1.5;
        int primed = 1, q = 9, refused = 0, tried = 0;
        float gain = 9.f;
        const auto refuses = [&](int rc, const char* who) { tried++; if (rc != GR_OK && last_error.find(who) != std::string::npos) refused++; };
        refuses(gr_tone_frame(nullptr, 2, 2, good.get(), 1.f, dst.get()), "gr_tone_frame");
        refuses(gr_tone_frame(src.get(), 0, 2, good.get(), 1.f, dst.get()), "gr_tone_frame");
        refuses(gr_tone_frame(src.get(), 2, 2, good.get(), std::numeric_limits<float>::quiet_NaN(), dst.get()), "gr_tone_frame");
        *bad = *good;
        bad->curve = 3;
        refuses(gr_tone_frame(src.get(), 2, 2, bad.get(), 1.f, dst.get()), "gr_tone_frame");
        *bad = *good;
        bad->white = 0.f;
        refuses(gr_tone_frame(src.get(), 2, 2, bad.get(), 1.f, dst.get()), "gr_tone_frame");
        refuses(gr_meter_histogram_frame(nullptr, 2, 2, hist.get()), "gr_meter_histogram_frame");
        refuses(gr_meter_histogram_frame(src.get(), 2, -2, hist.get()), "gr_meter_histogram_frame");
        refuses(gr_meter_histogram_frame(src.get(), 65536, 32768, hist.get()), "gr_meter_histogram_frame");
        *bad = *good;
        bad->low = 0.99f;
        refuses(gr_meter_solve_host(hist.get(), bad.get(), &adapted, &primed, &gain, &q), "gr_meter_solve_host");
        *bad = *good;
        bad->rate = 0.f;
        refuses(gr_meter_solve_host(hist.get(), bad.get(), &adapted, &primed, &gain, &q), "gr_meter_solve_host");
        *bad = *good;
        bad->min_stops = 3.f, bad->max_stops = 2.f;
        refuses(gr_meter_solve_host(hist.get(), bad.get(), &adapted, &primed, &gain, &q), "gr_meter_solve_host");
        refuses(gr_meter_solve_host(hist.get(), good.get(), nullptr, &primed, &gain, &q), "gr_meter_solve_host");
        int wrote = 0;
        for (int i = 0; i < 16; i++) wrote += bits_of(dst[i]) != 0xffffffffu;
        for (int b = 0; b < GR_METER_COUNTERS; b++) wrote += hist[b] != 0xffffffffu;
        wrote += adapted != 1.5 || primed != 1 || q != 9 || gain != 9.f;
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
