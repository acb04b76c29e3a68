// A stand-alone host program for tests/test_png_runs_stream.py: the host PNG encoder of both stream kinds (csrc/png_stream.cpp, compiled
// into this program) on heap buffers of exactly the frame's size and exactly gr_png_encode_bound bytes, built with
// -fsanitize=address,undefined - a read one byte past the frame or a write one byte past the bound ends the program.  Every file's zlib
// stream is inflated here (zlib's uncompress, which checks the Adler-32) and compared with the filtered rows written out again below; kind 0
// through gr_png_encode_rgba8_host_as is compared with gr_png_encode_rgba8_host byte for byte; the table builder of both kinds runs on
// exact-size arrays.  Prints one line per case and "ok".
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static const char* const CONTENTS[] = {"noise", "zero", "runs", "gradient"};

// the frame from its filtered words for "noise" and "runs" (so that the repeats are where they are meant to be), from its pixels otherwise
static void fill(unsigned char* frame, int width, int height, int content) {
    unsigned state = 99u + 131u * width + 7u * height + content;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            unsigned char* at = frame + 4 * ((size_t)y * width + x);
            if (content == 1) {
                memset(at, 0, 4);
            } else if (content == 3) {
                at[0] = (unsigned char)x, at[1] = (unsigned char)(3 * x), at[2] = (unsigned char)(5 * y), at[3] = 255;
            } else {
                // a filtered word: fresh, or (runs: three times in four) the one of the pixel before - then the filter undone
                unsigned char word[4];
                const bool repeat = content == 2 && x > 0 && next_value(state) % 4 != 0;
                for (int c = 0; c < 4; c++) word[c] = (unsigned char)next_value(state);
                const unsigned char* left = x ? at - 4 : nullptr;
                const unsigned char* up = y ? at - 4 * (size_t)width : nullptr;
                if (repeat) {   // the filtered word of pixel x - 1
                    for (int c = 0; c < 4; c++) {
                        const unsigned char before = y ? (unsigned char)(left[c] - (left - 4 * (size_t)width)[c]) : (unsigned char)(left[c] - (x > 1 ? (left - 4)[c] : 0));
                        word[c] = before;
                    }
                }
                for (int c = 0; c < 4; c++) at[c] = (unsigned char)(word[c] + (y ? up[c] : left ? left[c] : 0));
            }
        }
}

static int run(int kind, int width, int height, int content) {
    const size_t frame_bytes = 4 * (size_t)width * height;
    size_t bound = 0;
    if (gr_png_encode_bound(width, height, &bound) != GR_OK) return 1;
    std::unique_ptr<unsigned char[]> frame(new unsigned char[frame_bytes]), file(new unsigned char[bound]);
    fill(frame.get(), width, height, content);
    memset(file.get(), 0xee, bound);
    size_t bytes = 0;
    if (gr_png_encode_rgba8_host_as(frame.get(), width, height, file.get(), bound, &bytes, kind) != GR_OK || bytes > bound) {
        std::printf("kind %d, %d x %d %s: refused: %s\n", kind, width, height, CONTENTS[content], last_error.c_str());
        return 1;
    }
    if (kind == GR_PNG_STREAM_LITERALS) {
        std::unique_ptr<unsigned char[]> old(new unsigned char[bound]);
        size_t old_bytes = 0;
        if (gr_png_encode_rgba8_host(frame.get(), width, height, old.get(), bound, &old_bytes) != GR_OK || old_bytes != bytes ||
            memcmp(old.get(), file.get(), bytes) != 0) {
            std::printf("kind 0, %d x %d %s: not gr_png_encode_rgba8_host's file\n", width, height, CONTENTS[content]);
            return 1;
        }
    }
    // signature 8, IHDR 25, then the one IDAT: length, tag, data, CRC
    const unsigned char* idat = file.get() + 33;
    const size_t stream_bytes = ((size_t)idat[0] << 24) | ((size_t)idat[1] << 16) | ((size_t)idat[2] << 8) | idat[3];
    if (memcmp(idat + 4, "IDAT", 4) != 0 || 33 + 12 + stream_bytes + 12 != bytes) {
        std::printf("kind %d, %d x %d %s: the file is not signature, IHDR, one IDAT, IEND\n", kind, width, height, CONTENTS[content]);
        return 1;
    }
    const size_t row_bytes = 4 * (size_t)width + 1;
    std::vector<unsigned char> want(row_bytes * height), got(row_bytes * height);
    for (int y = 0; y < height; y++) {
        unsigned char* row = want.data() + row_bytes * y;
        row[0] = y ? 2 : 1;
        for (size_t i = 0; i < 4 * (size_t)width; i++) {
            const unsigned char here = frame[4 * (size_t)width * y + i];
            row[1 + i] = (unsigned char)(here - (y ? frame[4 * (size_t)width * (y - 1) + i] : i >= 4 ? frame[i - 4] : 0));
        }
    }
    uLongf got_bytes = (uLongf)got.size();
    const int rc = uncompress(got.data(), &got_bytes, idat + 8, (uLong)stream_bytes);
    if (rc != Z_OK || got_bytes != want.size() || memcmp(got.data(), want.data(), want.size()) != 0) {
        std::printf("kind %d, %d x %d %s: zlib says %d, %lu of %zu bytes\n", kind, width, height, CONTENTS[content], rc, (unsigned long)got_bytes, want.size());
        return 1;
    }
    std::printf("kind %d, %d x %d %s: %zu bytes of at most %zu, inflates to the filtered rows\n", kind, width, height, CONTENTS[content], bytes, bound);
    return 0;
}

static int tables() {
    int failed = 0;
    for (int kind = 0; kind < 2; kind++) {
        const int symbols = kind ? 285 : 257;
        std::unique_ptr<unsigned long long[]> histogram(new unsigned long long[symbols]);
        std::unique_ptr<unsigned char[]> lengths(new unsigned char[symbols]);
        std::unique_ptr<unsigned short[]> codes(new unsigned short[symbols]);
        std::unique_ptr<unsigned int[]> header(new unsigned int[128]);
        unsigned long long a = 1, b = 1;
        for (int s = 0; s < symbols; s++) {   // Fibonacci weights on every third symbol: a tree far deeper than 15
            histogram[s] = s % 3 ? 0 : a;
            if (s % 3 == 0 && a < (1ull << 60)) { const unsigned long long c = a + b; a = b; b = c; }
        }
        int bits = 0;
        if (gr_png_build_table_as(histogram.get(), kind, lengths.get(), codes.get(), header.get(), &bits) != GR_OK || bits < 74 || bits > 4096) failed++;
        unsigned long long kraft = 0;
        for (int s = 0; s < symbols; s++)
            if (lengths[s]) kraft += 1ull << (15 - lengths[s]);
        if (kraft != 1ull << 15) failed++;
        std::printf("table of kind %d: header of %d bits\n", kind, bits);
    }
    return failed;
}

int main() {
    int failed = 0;
    const int widths[] = {1, 2, 3, 63, 64, 65, 129, 256, 257}, heights[] = {1, 2, 5};
    for (int kind = 0; kind < 2; kind++)
        for (int width : widths)
            for (int height : heights)
                for (int content = 0; content < 4; content++) failed += run(kind, width, height, content);
    failed += tables();
    // a refusal writes nothing
    {
        std::unique_ptr<unsigned char[]> frame(new unsigned char[16]()), file(new unsigned char[64]);
        memset(file.get(), 0xee, 64);
        size_t bytes = 0;
        if (gr_png_encode_rgba8_host_as(frame.get(), 2, 2, file.get(), 64, &bytes, GR_PNG_STREAM_RUNS) != GR_ERROR_BUFFER_TOO_SMALL) failed++;
        if (gr_png_encode_rgba8_host_as(frame.get(), 2, 2, file.get(), 64, &bytes, 2) == GR_OK || last_error.find("gr_png_encode_rgba8_host_as") == std::string::npos) failed++;
        for (int i = 0; i < 64; i++)
            if (file[i] != 0xee) failed++;
    }
    if (failed) {
        std::printf("%d cases failed\n", failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
