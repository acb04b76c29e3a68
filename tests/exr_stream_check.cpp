// A stand-alone host program for tests/test_exr_stream.py: the host EXR encoder (csrc/exr_stream.cpp, compiled into this program with
// csrc/png_stream.cpp, whose table builder it calls) on heap buffers of exactly the frame's size and exactly gr_exr_encode_bound bytes,
// built with -fsanitize=address,undefined - a read one byte past the frame or a write one byte past the bound ends the program.  Every
// chunk is walked here: a raw one is compared with the row's halfs, a compressed one is inflated (zlib's uncompress, which checks the
// Adler-32), its predictor and byte split are undone and the result compared with the same halfs, written out again below from the
// definition's words.  Prints one line per case and "ok".
#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../include/geodesic_hip_internal.h"

static std::string last_error;
extern "C" int gr_internal_fail(int code, const char* msg) {
    last_error = msg ? msg : "";
    return code;
}

static unsigned next_value(unsigned& state) {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

static const char* const CONTENTS[] = {"noise", "zero", "smooth", "mixed", "specials"};

static void fill(float* frame, int width, int height, int content) {
    unsigned state = 77u + 131u * width + 7u * height + content;
    static const float SPECIALS[] = {std::numeric_limits<float>::quiet_NaN(), INFINITY, 0.f, 65504.f, 65519.9f, 65520.f, 1e30f, 6.103515625e-05f,
                                     5.9604644775390625e-08f, 2.98023223876953125e-08f, 2.98023223876953125e-08f * (1.f + 0.0009765625f),
                                     1.f + 0.00048828125f, 1.f + 3 * 0.00048828125f};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++)
            for (int c = 0; c < 4; c++) {
                float& v = frame[4 * ((size_t)y * width + x) + c];
                const bool noise = content == 0 || (content == 3 && (y % 3) == 0);
                if (content == 1) v = 0.f;
                else if (content == 4) { const unsigned k = next_value(state) % 26u; v = k < 13u ? SPECIALS[k] : -SPECIALS[k - 13u]; }
                else if (noise) {   // a float that is a random normal half: sixteen bits that do not compress
                    const unsigned r = next_value(state), bits = ((r & 0x8000u) << 16) | ((((r >> 10) & 31u) % 30u + 113u) << 23) | ((r & 1023u) << 13);
                    memcpy(&v, &bits, 4);
                }
                else v = 0.25f + (float)x / (float)(width + 1) * (float)(c + 1) + 0.01f * (float)y;
            }
}

// the definition in words, a second time: NaN +0, clamp, nearest even, subnormals kept - through double arithmetic instead of the bits
static unsigned short half_of(float f) {
    if (std::isnan(f)) return 0;
    const unsigned short sign = std::signbit(f) ? 0x8000 : 0;
    double a = std::fabs((double)f);
    if (a > 65504.0) a = 65504.0;
    if (a < 6.103515625e-05) return (unsigned short)(sign | (unsigned short)std::nearbyint(a * 16777216.0));   // h x 2^-24 (nearbyint: to even)
    int exponent;
    const double mantissa = std::frexp(a, &exponent);   // a = mantissa x 2^exponent, 0.5 <= mantissa < 1
    const unsigned scaled = (unsigned)std::nearbyint(mantissa * 2048.0);   // 1 024 ... 2 048
    return (unsigned short)(sign | (((unsigned)(exponent + 14) << 10) + (scaled - 1024u)));   // (2 048 carries into the exponent)
}

static int run(int width, int height, int content) {
    const size_t pixels = (size_t)width * height, n = 6 * (size_t)width;
    size_t bound = 0;
    if (gr_exr_encode_bound(width, height, &bound) != GR_OK || bound != 313 + 8 * (size_t)height + height * (8 + n)) return 1;
    float* frame = (float*)std::aligned_alloc(16, 16 * pixels);
    std::unique_ptr<unsigned char[]> file(new unsigned char[bound]);
    fill(frame, width, height, content);
    memset(file.get(), 0xee, bound);
    size_t bytes = 0;
    int failed = 0, raw_rows = 0;
    if (gr_exr_encode_f32_host(frame, width, height, file.get(), bound, &bytes) != GR_OK || bytes > bound) {
        std::printf("%d x %d %s: refused: %s\n", width, height, CONTENTS[content], last_error.c_str());
        std::free(frame);
        return 1;
    }
    std::vector<unsigned short> halfs(4 * pixels);
    if (gr_exr_half_bits(frame, 4 * pixels, halfs.data()) != GR_OK) failed++;
    for (size_t i = 0; i < 4 * pixels; i++)
        if (halfs[i] != half_of(frame[i])) { failed++; break; }
    size_t at = 313 + 8 * (size_t)height;
    std::vector<unsigned char> want(n), got(n), reordered(n);
    for (int y = 0; y < height && !failed; y++) {
        unsigned long long offset = 0;
        for (int k = 7; k >= 0; k--) offset = (offset << 8) | file[313 + 8 * (size_t)y + k];
        if (offset != at || at + 8 > bytes) { failed++; break; }
        const unsigned char* chunk = file.get() + at;
        const size_t size = chunk[4] | ((size_t)chunk[5] << 8) | ((size_t)chunk[6] << 16) | ((size_t)chunk[7] << 24);
        if ((chunk[0] | (chunk[1] << 8) | (chunk[2] << 16) | ((unsigned)chunk[3] << 24)) != (unsigned)y || size > n || at + 8 + size > bytes) { failed++; break; }
        for (int plane = 0; plane < 3; plane++)
            for (int x = 0; x < width; x++) {
                const unsigned short h = half_of(frame[4 * ((size_t)y * width + x) + (2 - plane)]);
                want[2 * ((size_t)plane * width + x)] = (unsigned char)h;
                want[2 * ((size_t)plane * width + x) + 1] = (unsigned char)(h >> 8);
            }
        if (size == n) {
            raw_rows++;
            memcpy(got.data(), chunk + 8, n);
        } else {
            uLongf inflated = (uLongf)n;
            if (uncompress(reordered.data(), &inflated, chunk + 8, (uLong)size) != Z_OK || inflated != n) { failed++; break; }
            for (size_t i = 1; i < n; i++) reordered[i] = (unsigned char)(reordered[i] + reordered[i - 1] - 128);
            for (size_t i = 0; i < n; i++) got[i] = reordered[(i & 1 ? n / 2 : 0) + i / 2];
        }
        if (memcmp(got.data(), want.data(), n) != 0) failed++;
        at += 8 + size;
    }
    if (!failed && at != bytes) failed++;
    for (size_t i = bytes; i < bound; i++)
        if (file[i] != 0xee) { failed++; break; }
    std::free(frame);
    if (failed) std::printf("%d x %d %s: the file does not hold the rows' halfs\n", width, height, CONTENTS[content]);
    else std::printf("%d x %d %s: %zu bytes of at most %zu, %d of %d rows raw, decodes to the halfs\n", width, height, CONTENTS[content], bytes, bound, raw_rows, height);
    return failed ? 1 : 0;
}

int main() {
    int failed = 0;
    const int widths[] = {1, 2, 3, 63, 64, 65, 129, 256, 257}, heights[] = {1, 2, 5};
    for (int width : widths)
        for (int height : heights)
            for (int content = 0; content < 5; content++) failed += run(width, height, content);
    // a refusal writes nothing
    {
        float* frame = (float*)std::aligned_alloc(16, 64);
        std::unique_ptr<unsigned char[]> file(new unsigned char[64]);
        memset(frame, 0, 64);
        memset(file.get(), 0xee, 64);
        size_t bytes = 0;
        if (gr_exr_encode_f32_host(frame, 2, 2, file.get(), 64, &bytes) != GR_ERROR_BUFFER_TOO_SMALL || last_error.find("gr_exr_encode_f32_host") == std::string::npos) failed++;
        if (gr_exr_encode_f32_host(frame + 1, 1, 1, file.get(), 64, &bytes) == GR_OK) failed++;
        for (int i = 0; i < 64; i++)
            if (file[i] != 0xee) failed++;
        std::free(frame);
    }
    if (failed) {
        std::printf("%d cases failed\n", failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
