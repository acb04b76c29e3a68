// frame_format_check.cpp — the table and the refusals of csrc/frame_format.cpp (tests/test_frame_format.py compiles this file together with
// it, with the host compiler and its sanitizers, and compares the lines printed here with the expectations written there).  No HIP, no library.
#include <cstdio>

#include "../geodesic_raytracing_amd/csrc/frame_format.hpp"

using namespace frame_format;

static const int SIZES[][2] = {{1, 1}, {2, 2}, {3, 5}, {7, 8}, {16, 8}, {1920, 1080}, {0, 8}, {8, -1}};
static const int WIDTHS[] = {4, 7, 8};

int main() {
    for (int format = -1; format <= 4; format++) {
        const row* f = find(format);
        if (!f) {
            printf("row %d: none\n", format);
            continue;
        }
        printf("row %d: %s %s layout=%d split=%d\n", format, f->name, f->entry, (int)f->takes_layout, f->split_pixel_bytes);
        printf("bytes %d:", format);
        for (const auto& size : SIZES) printf(" %zu", f->bytes(size[0], size[1]));
        // the alignment at a width: the first of 1, 2, 4, 8, 16 that refusal() lets through as a pointer
        printf("\nalignment %d:", format);
        for (int width : WIDTHS)
            for (uintptr_t out = 1; out <= 16; out *= 2)
                if (refusal(format, false, GR_YUV420_I420, out, &width, 1).empty()) {
                    printf(" %d", (int)out);
                    break;
                }
        printf("\n");
        // the predicate, pointer values 0 ... 15 at widths 7 and 8, as a string of 0 / 1.  The width - a state's, in the frame entries - was
        // read only for a 10-bit pointer aligned to 2 bytes and not to 8: everywhere else there is none to read here, and reading it ends the run
        for (int width : {7, 8}) {
            printf("misaligned %d at %d: ", format, width);
            for (uintptr_t out = 0; out < 16; out++) {
                const bool read = format == GR_FRAME_YUV420P10 && out % 8 != 0 && out % 2 == 0;
                printf("%d", (int)!refusal(format, false, GR_YUV420_I420, out, read ? &width : nullptr, 1).empty());
            }
            printf("\n");
        }
    }
    const int* never = nullptr;   // (no refusal below depends on a width: every pointer is aligned to 8)
    for (int split_only = 0; split_only <= 1; split_only++)
        for (int format = -1; format <= 4; format++)
            printf("format %d split_only=%d: \"%s\"\n", format, split_only, refusal(format, split_only, GR_YUV420_I420, 64, never, 1).c_str());
    for (int format = 0; format <= 3; format++)
        for (int layout : {-1, 0, 1, 2})
            printf("layout %d of %d: \"%s\"\n", layout, format, refusal(format, false, layout, 64, never, 1).c_str());
    for (int format = 0; format <= 3; format++)
        printf("strips of %d: \"%s\"\n", format, refusal(format, false, GR_YUV420_NV12, 64, never, 2).c_str());
    for (int format = 0; format <= 3; format++)
        for (int width : {7, 8})
            printf("pointer 4098 of %d at %d: \"%s\"\n", format, width, refusal(format, false, GR_YUV420_I420, 4098, &width, 1).c_str());
    // the order: format, layout, pointer, strips
    printf("order: \"%s\" | \"%s\" | \"%s\"\n", refusal(7, false, 9, 1, never, 2).c_str(), refusal(GR_FRAME_YUV420, false, 9, 1, never, 2).c_str(),
           refusal(GR_FRAME_YUV420, false, GR_YUV420_I420, 1, never, 2).c_str());
    return 0;
}
