// jpeg_stream_check.cpp — csrc/jpeg_stream.cpp and the AVI writer of csrc/imageio.cpp on their own (tests/test_jpeg_stream.py compiles this
// file together with them - host compiler, AddressSanitizer and UBSan, no HIP - and runs it): gr_jpeg_encode_rgba8_host over the size set
// of the tests at four qualities, every frame and every output in a heap block of exactly its size so that a byte past either end is
// caught, then the files of one quality through gr_avi_* with a limit small enough to refuse the last frame.  Prints "<w>x<h>: <bytes at
// quality 90>" per size and "avi: closed".  argv[1]: where the AVI file goes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/geodesic_hip_internal.h"

static std::string last_error;
extern "C" int gr_internal_fail(int code, const char* msg) {   // (capi.cpp's, which is not linked here)
    last_error = msg ? msg : "";
    return code;
}

#define CHECK(what)                                                                  \
    do {                                                                             \
        if (!(what)) {                                                               \
            fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #what, last_error.c_str()); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const int sizes[][2] = {{1, 1}, {7, 5}, {8, 8}, {16, 16}, {17, 16}, {16, 17}, {33, 18}, {16, 160}};
    const int qualities[] = {1, 50, 90, 100};
    std::vector<std::vector<unsigned char>> files;
    for (auto& size : sizes) {
        const int w = size[0], h = size[1];
        unsigned char* pixels = (unsigned char*)malloc((size_t)w * h * 4);   // (tests/test_jpeg_stream.py: images()["gradient"])
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                unsigned char* p = pixels + 4 * ((size_t)y * w + x);
                p[0] = (unsigned char)((x * 3) & 255);
                p[1] = (unsigned char)((y * 5 + x) & 255);
                p[2] = (unsigned char)((255 - x - y) & 255);
                p[3] = 255;
            }
        size_t bound = 0, bytes = 0;
        CHECK(gr_jpeg_encode_bound(w, h, &bound) == GR_OK);
        for (int quality : qualities) {
            unsigned char* out = (unsigned char*)malloc(bound);
            CHECK(gr_jpeg_encode_rgba8_host(pixels, w, h, quality, out, bound, &bytes) == GR_OK);
            CHECK(bytes <= bound && out[0] == 0xff && out[1] == 0xd8 && out[bytes - 2] == 0xff && out[bytes - 1] == 0xd9);
            CHECK(gr_jpeg_encode_rgba8_host(pixels, w, h, quality, out, bound - 1, &bytes) == GR_ERROR_BUFFER_TOO_SMALL);
            if (quality == 90) {
                printf("%dx%d: %zu\n", w, h, bytes);
                files.emplace_back(out, out + bytes);
            }
            free(out);
        }
        short* blocks = (short*)malloc((size_t)((w + 15) / 16) * ((h + 15) / 16) * 6 * 64 * sizeof(short));
        CHECK(gr_jpeg_blocks_host(pixels, w, h, 100, blocks) == GR_OK);
        free(blocks);
        free(pixels);
    }
    gr_avi* avi = nullptr;
    CHECK(gr_avi_open(argv[1], 16, 16, 30000, 1001, &avi) == GR_OK);
    unsigned long long written = 224;
    for (size_t i = 0; i + 1 < files.size(); i++) {
        CHECK(gr_avi_write_frame(avi, files[i].data(), files[i].size()) == GR_OK);
        written += 8 + files[i].size() + (files[i].size() & 1);
    }
    // the finished file with the last frame would be one byte past this limit
    const std::vector<unsigned char>& last = files.back();
    CHECK(gr_avi_set_size_limit(avi, written + 8 + last.size() + (last.size() & 1) + 8 + 16 * files.size() - 1) == GR_OK);
    CHECK(gr_avi_write_frame(avi, last.data(), last.size()) == GR_ERROR_INVALID_ARGUMENT);
    CHECK(last_error.find("past the") != std::string::npos);
    CHECK(gr_avi_close(avi) == GR_OK);
    printf("avi: closed\n");
    return 0;
}
