// exr_stream.hpp — the OpenEXR file both EXR encoders write (geodesic_hip_internal.h, "EXR frames"): the half conversion in integers, the
// header, a row's raw bytes and its bytes in zip order, the frame's table (png_stream's construction with BFINAL set), the sizes of the
// rows' zlib streams and the rule that stores a row raw.  Host only (no HIP): exr_stream.cpp compiles without a HIP header - beside
// png_stream.cpp, whose table builder it calls - and holds gr_exr_encode_f32_host, the definition kernels/exr.hip is held to byte for
// byte.  device_encoders.cpp reads it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/geodesic_hip_internal.h"
#include "png_stream.hpp"

namespace exr_stream __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

enum {
    HEADER_BYTES = 313,       // magic, version, the eight attributes, the header's closing 0: the same for every size
    CHUNK_HEADER_BYTES = 8,   // int32 y, int32 size
    END_OF_BLOCK = png_stream::END_OF_BLOCK,
};
const uint64_t MAX_ROW_BYTES = 0x7fffffffull;   // of a row's raw bytes, 6 a pixel

// The half of a float, both as bit patterns: NaN -> +0; otherwise clamped to [-65504, 65504]; round to nearest even, half subnormals kept
// (below 2^-25, and 2^-25 itself - a tie - to a zero of the float's sign).  Integer arithmetic only: kernels/exr.hip states the same lines.
inline uint16_t half_bits(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u;
    uint32_t a = f & 0x7fffffffu;
    if (a > 0x7f800000u) return 0;              // NaN
    if (a > 0x477fe000u) a = 0x477fe000u;       // 65504, the largest half
    if (a >= 0x38800000u) {                     // 2^-14 and above: a normal half - the exponent rebiased by 112, 13 bits rounded away
        const uint32_t r = a - 0x38000000u;
        return (uint16_t)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
    }
    const uint32_t e = a >> 23;
    if (e < 102u) return (uint16_t)sign;        // below 2^-25: nearer 0 than the smallest subnormal
    // a subnormal half is h x 2^-24: the float's 24-bit significand shifted down by 126 - e = 14 ... 24 bits
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;
    uint32_t h = m >> shift;
    const uint32_t rest = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    if (rest > tie || (rest == tie && (h & 1u))) h++;   // (1 024 is the smallest normal half: the carry is right)
    return (uint16_t)(sign | h);
}

inline uint64_t row_bytes(int width) { return 6ull * (uint64_t)width; }
// the 313 bytes in front of the offset table
void write_header(uint8_t* out, int width, int height);
// a row's raw bytes, 6 * width: the planes B, G, R, each `width` little-endian halfs of the float4 frame's b, g, r
void raw_row(const float* frame_rgba_f32, int width, int row, uint8_t* raw);
// ... in OpenEXR's zip order: the even-indexed bytes, then the odd-indexed ones; then every byte but the first minus the one before it
// (of the reordered values) plus 128, mod 256
void predicted_row(const uint8_t* raw, size_t bytes, uint8_t* out);
// the frame's table from histogram[257]: the predicted bytes of all rows and [256] = the rows (one end-of-block each) - png_stream's
// literals table with BFINAL = 1 in the block header
void build_table(const uint64_t* histogram, png_stream::table& out);
// bits of a row's block - header, literals, end-of-block - from the histogram of its predicted bytes (256 words)
uint64_t row_block_bits(const png_stream::table& t, const uint32_t* row_histogram);
// bytes of a row's zlib stream: 78 01, the block and 0 bits up to a byte boundary, the Adler-32
inline uint64_t stream_bytes(uint64_t block_bits) { return 2 + (block_bits + 7) / 8 + 4; }
// THE RULE: a chunk holds the zlib stream where that is shorter than the raw row, otherwise the raw row as it is
inline bool stored_raw(uint64_t stream, int width) { return !(stream < row_bytes(width)); }
// the Adler-32 of a row's n = 6 * width predicted bytes b_i at position i from its sums: sum of b_i and sum of (n - i) b_i, each mod 65521
uint32_t row_adler(int width, uint32_t sum, uint32_t weighted);
// header, offset table, and every row a chunk of its raw bytes: what no file of this size exceeds, exactly; 0 for a bad size
uint64_t file_bound(int width, int height);
// the offset table behind the header from the chunks' offsets in the chunk area (height + 1 of them, the first 0)
void write_offsets(uint8_t* out_file, int height, const uint64_t* chunk_offset);
inline uint64_t chunks_at(int height) { return (uint64_t)HEADER_BYTES + 8ull * (uint64_t)height; }
// what both encoders refuse on account of the frame and the output, "" for nothing; the caller prefixes its name
std::string refusal(const void* frame, int width, int height, const void* out_file, size_t capacity, const void* out_bytes, bool aligned_frame,
                    bool* too_small);

}  // namespace exr_stream
