// frame_format.hpp — the formats a frame leaves the device in: one table, and what an output is refused for on account of its format.
// Host only (no HIP): tests/frame_format_check.cpp compiles frame_format.cpp alone.  frame.cpp, frame_launch.cpp, tiled.cpp and imageio.cpp read it.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/geodesic_hip_internal.h"

namespace frame_format __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

struct row {
    const char *name, *entry;   // the constant's, and the entry point's that renders a frame in it
    bool takes_layout;       // GR_YUV420_I420 or GR_YUV420_NV12; the others ignore theirs
    int split_pixel_bytes;   // of a pixel of a split frame (gr_render_frame_tiled_as); 0: the format travels whole frames only
    size_t (*bytes)(int width, int height);   // of a frame; 0 for a size below 1
    // of the output pointer: at any width, and where the width is a multiple of 4 (the 10-bit kernel's 8-byte stores); the first divides the second
    int alignment, alignment_by4;
};
const row* find(int format);   // NULL: not a GR_FRAME_* value
// gr_yuv420_bytes: the Y plane and two chroma planes of half the size per axis, rounded up (inline: a host check links imageio.cpp alone)
inline size_t yuv420_bytes(int w, int h) { return w < 1 || h < 1 ? 0 : (size_t)w * h + 2 * (((size_t)w + 1) / 2) * (((size_t)h + 1) / 2); }
// What an output is refused for on account of its format, "" for nothing, in this order: a format not in the table (split_only: or one that no split frame
// travels in), with the names accepted; an unknown layout for a format that takes one; a pointer not aligned as the row says (*width is read only where the
// answer depends on it: it may be a state's that no earlier refusal looked at); strip_count > 1 for a format that does not split.  The caller prefixes its name.
std::string refusal(int format, bool split_only, int layout, uintptr_t out, const int* width, int strip_count);

}  // namespace frame_format
