// jpeg_stream.hpp — the one JPEG stream both JPEG encoders write (geodesic_hip_internal.h, "JPEG frames"): colour conversion, the integer
// DCT, the quantiser, the Annex K Huffman tables, the headers, the sizes.  Host only (no HIP): jpeg_stream.cpp compiles alone and holds
// gr_jpeg_encode_rgba8_host, the definition kernels/jpeg.hip is held to byte for byte.  device_encoders.cpp reads it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/geodesic_hip_internal.h"

namespace jpeg_stream __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

enum {
    MAX_SIZE = 65535,          // of a width or a height: SOF0 holds both in 16 bits
    MCU = 16,                  // pixels a side: 2 x 2 luminance blocks, one Cb block, one Cr block
    BLOCKS_PER_MCU = 6,
    // of one block's code: a DC code of at most 9 bits with 11 value bits, 63 AC codes of at most 16 bits with 10 value bits each
    MAX_BLOCK_BITS = 9 + 11 + 63 * (16 + 10),
    HEADER_BYTES = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14,   // SOI, APP0, two DQT, SOF0, four DHT, DRI, SOS
    // the tables the device reads, as 32-bit words: per component class (0 luminance, 1 chrominance) 16 DC and 256 AC codes
    // (code | length << 16, indexed by the symbol), then per class 64 reciprocals and 64 rounding terms in natural order (quantise())
    TABLE_DC = 0, TABLE_AC = 32, TABLE_RECIPROCAL = 32 + 512, TABLE_HALF = 32 + 512 + 128, TABLE_WORDS = 32 + 512 + 256,
};

extern const uint8_t ZIGZAG[64];         // the natural (row-major) index of zig-zag position k
extern const int32_t DCT[8][8];          // round(2^14 c[u][x]), c the orthonormal DCT-II matrix

inline int mcus_across(int width) { return (width + MCU - 1) / MCU; }
inline int mcu_rows(int height) { return (height + MCU - 1) / MCU; }

// the Annex K tables scaled by the quality (1 ... 100), in natural order
void quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
// Y' - 128, Cb - 128 or Cr - 128 (component 0, 1, 2) of 8-bit R, G, B: JFIF's full-range BT.601 in 16-bit fixed point
int32_t convert(int component, int32_t r, int32_t g, int32_t b);
// the 8 x 8 forward DCT of `samples` (natural order, each -128 ... 127) with 4 fraction bits: out = 16 x the coefficient, natural order
void fdct(const int16_t samples[64], int32_t out[64]);
// a coefficient of fdct() over a step of the quantiser, rounded half away from zero
inline int32_t quantise(int32_t coefficient_x16, int32_t step) {
    const int32_t q = ((coefficient_x16 < 0 ? -coefficient_x16 : coefficient_x16) + 8 * step) / (16 * step);
    return coefficient_x16 < 0 ? -q : q;
}
// the quantised coefficients of a frame: per MCU in scan order six blocks (Y00 Y01 Y10 Y11 Cb Cr) of 64 in zig-zag order
void blocks(const unsigned char* rgba8, int width, int height, int quality, int16_t* out);
// the Huffman codes and the quantiser's tables as the device reads them (TABLE_WORDS words)
void device_tables(int quality, uint32_t* words);
// everything in front of the entropy-coded data (HEADER_BYTES bytes)
void write_headers(uint8_t* out, int width, int height, int quality);
// bytes of an MCU row's entropy-coded segment before byte stuffing, at most; rounded up to 16 for a slot of the device's scratch
inline uint64_t row_bytes_bound(int width) { return ((uint64_t)mcus_across(width) * BLOCKS_PER_MCU * MAX_BLOCK_BITS + 7) / 8; }
inline uint64_t row_slot_bytes(int width) { return (row_bytes_bound(width) + 15) / 16 * 16; }
// what no file of this size exceeds (gr_jpeg_encode_bound): the headers, and per MCU row every byte stuffed and a marker
inline uint64_t file_bound(int width, int height) { return HEADER_BYTES + (uint64_t)mcu_rows(height) * (2 * row_bytes_bound(width) + 2); }
// what both encoders refuse on account of the frame, the quality and the output, "" for nothing; the caller prefixes its name
std::string refusal(const void* rgba8, int width, int height, int quality, const void* out_file, size_t capacity, const void* out_bytes, bool* too_small);
std::string size_refusal(int width, int height);
std::string quality_refusal(int quality);

}  // namespace jpeg_stream
