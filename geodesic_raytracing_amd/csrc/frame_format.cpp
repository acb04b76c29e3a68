// frame_format.cpp — the table of frame formats and the refusals that depend on a format (frame_format.hpp).
#include "frame_format.hpp"

namespace frame_format {

static size_t pixels(int width, int height) { return width < 1 || height < 1 ? 0 : (size_t)width * height; }

static const row TABLE[] = {
    {"GR_FRAME_F32", "gr_render_frame", false, 16, [](int w, int h) { return 16 * pixels(w, h); }, 1, 1},
    {"GR_FRAME_RGBA8", "gr_render_frame_rgba8", false, 4, [](int w, int h) { return 4 * pixels(w, h); }, 1, 1},
    {"GR_FRAME_YUV420", "gr_render_frame_yuv420", true, 0, yuv420_bytes, 4, 4},
    {"GR_FRAME_YUV420P10", "gr_render_frame_yuv420p10", true, 0, [](int w, int h) { return 2 * yuv420_bytes(w, h); }, 2, 8},
};
static_assert(GR_FRAME_F32 == 0 && GR_FRAME_RGBA8 == 1 && GR_FRAME_YUV420 == 2 && GR_FRAME_YUV420P10 == 3, "TABLE is indexed by the GR_FRAME_* values");

const row* find(int format) { return format >= 0 && format < (int)(sizeof(TABLE) / sizeof(TABLE[0])) ? &TABLE[format] : nullptr; }

std::string refusal(int format, bool split_only, int layout, uintptr_t out, const int* width, int strip_count) {
    const row* f = find(format);
    if (!f || (split_only && !f->split_pixel_bytes))
        return "unknown frame format " + std::to_string(format) +
               (split_only ? " (GR_FRAME_F32 or GR_FRAME_RGBA8)" : " (GR_FRAME_F32, GR_FRAME_RGBA8, GR_FRAME_YUV420 or GR_FRAME_YUV420P10)");
    if (f->takes_layout && layout != GR_YUV420_I420 && layout != GR_YUV420_NV12)
        return "layout " + std::to_string(layout) + " (GR_YUV420_I420 or GR_YUV420_NV12)";
    if (out % f->alignment_by4 && (out % f->alignment || *width % 4 == 0))
        return "the output must be aligned to " + std::to_string(f->alignment_by4) + " bytes for " + f->name +
               (f->alignment_by4 != f->alignment ? " where the width is a multiple of 4, to " + std::to_string(f->alignment) + " bytes otherwise" : "");
    if (strip_count > 1 && !f->split_pixel_bytes)
        return "whole frames only (strip_count > 1); a split frame travels as float4 or RGBA8: gr_render_frame_tiled_as";
    return "";
}

}  // namespace frame_format
