// png_stream.hpp — the one PNG stream both PNG encoders write (geodesic_hip_internal.h, "PNG frames"): the length-limited Huffman table of
// a frame, its block header as a bit string, the sizes of the row segments, the container.  Host only (no HIP): png_stream.cpp compiles
// alone and holds gr_png_encode_rgba8_host, the definition kernels/png.hip is held to byte for byte.  capi.cpp reads it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/geodesic_hip_internal.h"

namespace png_stream __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

enum {
    SYMBOLS = 257,            // the literals 0 ... 255 and end-of-block; no length symbol is ever used
    END_OF_BLOCK = 256,
    MAX_LENGTH = 15,          // of a literal's code (deflate's limit)
    MAX_LENGTH_OF_LENGTHS = 7,   // of a code-length symbol's code
    // of the block header: 17 bits of counts, 19 x 3 bits, and at most 258 code-length symbols of 7 bits with 7 extra bits = 3 686
    HEADER_MAX_BITS = 4096,
    HEADER_WORDS = HEADER_MAX_BITS / 32,
};
const uint64_t MAX_RAW_BYTES = 0x7fffffffull;   // of a frame, 4 a pixel
const uint64_t MAX_IDAT_BYTES = 0x7fffffffull;  // of one IDAT chunk's data

struct table {
    uint8_t length[SYMBOLS];    // 0: the symbol does not occur
    uint16_t code[SYMBOLS];     // canonical, bit-reversed: written from bit 0 up, as deflate packs Huffman codes
    uint32_t header[HEADER_WORDS];   // BFINAL = 0, BTYPE = 2, the counts, the code lengths: bit k of the stream is bit k % 32 of word k / 32
    int header_bits;
};

// Code lengths of an optimal prefix code over the symbols with count > 0, then limited to max_length with a complete code (Kraft sum
// exactly 1).  Fewer than two symbols with a count: the lowest-numbered others join with count 0 until there are two leaves of one bit.
void limited_lengths(const uint64_t* count, int symbols, int max_length, uint8_t* length);
// deflate's canonical codes of these lengths, each reversed over its own length
void canonical_codes(const uint8_t* length, int symbols, uint16_t* code);
// histogram: of the frame's filtered bytes, filter-type bytes included, and [256] = its rows (one end-of-block each; 0 is taken as 1)
void build_table(const uint64_t histogram[SYMBOLS], table& out);

// the filter type of a row: Sub for row 0, Up for every other
inline int filter_of_row(int row) { return row == 0 ? 1 : 2; }
// bits of a row's block - header, filter byte, literals, end-of-block - from the histogram of its 4 * width filtered pixel bytes
uint64_t row_block_bits(const table& t, int row, const uint32_t row_histogram[256]);
// bytes of a row's segment: the block, the 3 bits of an empty stored block, the padding to a byte, 00 00 FF FF
inline uint64_t row_segment_bytes(uint64_t block_bits) { return (block_bits + 3 + 7) / 8 + 4; }
// the zlib stream around `rows_bytes` of segments: 78 01 in front, 03 00 and the Adler-32 behind
inline uint64_t zlib_bytes(uint64_t rows_bytes) { return 2 + rows_bytes + 2 + 4; }
// the file: signature, IHDR, the IDAT chunks (one below 2^31 - 1 bytes of stream), IEND
uint64_t file_bytes(uint64_t rows_bytes, uint64_t max_idat = MAX_IDAT_BYTES);
// what no frame of this size exceeds (every literal 15 bits, a header of HEADER_MAX_BITS a row): gr_png_encode_bound; 0 for a bad size
uint64_t rows_bound(int width, int height);
// the Adler-32 of a row of n = 4 * width + 1 filtered bytes that starts from 1, from the sums over its pixel bytes b_i at position i
// (0-based; the filter byte is position 0): sum = sum of b_i mod 65521, weighted = sum of (n - i) b_i mod 65521
uint32_t row_adler(int row, int width, uint32_t sum, uint32_t weighted);
// the rows' Adler-32 values joined in order (zlib's adler32_combine)
uint32_t join_adler(const uint32_t* row_adlers, int width, int height);
// writes the file into out (file_bytes(rows_bytes) bytes): `rows` are the segments back to back
void write_container(uint8_t* out, int width, int height, const uint8_t* rows, uint64_t rows_bytes, uint32_t adler, uint64_t max_idat = MAX_IDAT_BYTES);
// what both encoders refuse on account of the frame and the output, "" for nothing; the caller prefixes its name
std::string refusal(const void* rgba8, int width, int height, const void* out_file, size_t capacity, const void* out_bytes, bool* too_small);

}  // namespace png_stream
