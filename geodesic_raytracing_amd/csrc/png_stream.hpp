// png_stream.hpp — the PNG streams both PNG encoders write (geodesic_hip_internal.h, "PNG frames"; two kinds: literals only, and literals
// with previous-pixel run matches): the length-limited Huffman table of a frame, its block header as a bit string, the tokens of a row, the
// sizes of the row segments, the container.  Host only (no HIP): png_stream.cpp compiles alone and holds gr_png_encode_rgba8_host and
// gr_png_encode_rgba8_host_as, the definition kernels/png.hip is held to byte for byte.  device_encoders.cpp reads it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/geodesic_hip_internal.h"

namespace png_stream __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

enum {
    SYMBOLS = 257,            // GR_PNG_STREAM_LITERALS: the literals 0 ... 255 and end-of-block; no length symbol is ever used
    RUNS_SYMBOLS = 285,       // GR_PNG_STREAM_RUNS: those and the length symbols 257 ... 284 (lengths 3 ... 257; the stream uses 4 ... 256)
    MAX_SYMBOLS = RUNS_SYMBOLS,
    END_OF_BLOCK = 256,
    FIRST_LENGTH_SYMBOL = 257,
    GROUP_PIXELS = 64,        // a match of the runs stream stays inside pixels 64 g ... 64 g + 63 of its row
    MAX_LENGTH = 15,          // of a literal's or a length's code (deflate's limit)
    MAX_LENGTH_OF_LENGTHS = 7,   // of a code-length symbol's code
    // of the block header: 17 bits of counts, 19 x 3 bits, and the code-length symbols of the 258 (literals) or 289 (runs) lengths sent: 7
    // bits at most for one that stands for one length, 7 + 7 for one with extra bits, which stands for three lengths or more - 7 bits a
    // length at most, 74 + 289 x 7 = 2 097
    HEADER_MAX_BITS = 4096,
    HEADER_WORDS = HEADER_MAX_BITS / 32,
};
const uint64_t MAX_RAW_BYTES = 0x7fffffffull;   // of a frame, 4 a pixel
const uint64_t MAX_IDAT_BYTES = 0x7fffffffull;  // of one IDAT chunk's data

inline bool known_kind(int stream_kind) { return stream_kind == GR_PNG_STREAM_LITERALS || stream_kind == GR_PNG_STREAM_RUNS; }
// symbols of a kind's literal/length alphabet, and words of a row's histogram as the device stores it (one a literal; one a symbol for the
// runs stream, where [256] stays 0: end-of-block is the host's to count)
inline int symbols_of(int stream_kind) { return stream_kind == GR_PNG_STREAM_RUNS ? RUNS_SYMBOLS : SYMBOLS; }
inline int row_bins_of(int stream_kind) { return stream_kind == GR_PNG_STREAM_RUNS ? RUNS_SYMBOLS : 256; }

struct table {
    int symbols;                    // SYMBOLS or RUNS_SYMBOLS; what lies behind them in the arrays below is 0
    uint8_t length[MAX_SYMBOLS];    // 0: the symbol does not occur
    uint16_t code[MAX_SYMBOLS];     // canonical, bit-reversed: written from bit 0 up, as deflate packs Huffman codes
    uint32_t header[HEADER_WORDS];   // BFINAL = 0, BTYPE = 2, the counts, the code lengths: bit k of the stream is bit k % 32 of word k / 32
    int header_bits;
};

// Code lengths of an optimal prefix code over the symbols with count > 0, then limited to max_length with a complete code (Kraft sum
// exactly 1).  Fewer than two symbols with a count: the lowest-numbered others join with count 0 until there are two leaves of one bit.
void limited_lengths(const uint64_t* count, int symbols, int max_length, uint8_t* length);
// deflate's canonical codes of these lengths, each reversed over its own length
void canonical_codes(const uint8_t* length, int symbols, uint16_t* code);
// histogram[symbols_of(stream_kind)]: of the frame's tokens - literals (filter-type bytes included), [256] = its rows (one end-of-block
// each; 0 is taken as 1) and, for the runs stream, the length symbols of its matches.  The distance lengths sent: literals one, 0; runs
// four, 0 0 0 1 (distance code 3 is distance 4 and has no extra bits)
void build_table(const uint64_t* histogram, int stream_kind, table& out);

// the runs stream's length symbol of a match of `run` pixels (1 ... 64; 4 * run bytes), RFC 1951 3.2.5, and its extra bits
struct length_code { int symbol, extra_bits, extra; };
inline length_code length_code_of(int run) {
    const int m = 4 * run - 3;   // (length - 3)
    int extra_bits = 0;
    while ((m >> extra_bits) >= 8) extra_bits++;
    return {FIRST_LENGTH_SYMBOL + 4 * extra_bits + (m >> extra_bits), extra_bits, m & ((1 << extra_bits) - 1)};
}
inline int extra_bits_of(int length_symbol) { return length_symbol < 265 ? 0 : (length_symbol - 261) / 4; }
// the tokens of a row of the runs stream from its 4 * width filtered pixel bytes: run[x] = 0: pixel x is four literals; r >= 1: pixel x
// heads a match of distance 4 and length 4 r; -1: pixel x lies inside a match.  (Literals stream: all 0.)
void tokenise_row(const uint8_t* filtered, int width, int stream_kind, int* run);

// the filter type of a row: Sub for row 0, Up for every other
inline int filter_of_row(int row) { return row == 0 ? 1 : 2; }
// bits of a row's block - header, filter byte, literals, matches (code, extra bits, the one distance bit), end-of-block - from the
// histogram of its tokens, row_bins_of(kind) words, in which neither the filter byte nor end-of-block is counted
uint64_t row_block_bits(const table& t, int row, const uint32_t* row_histogram);
// bytes of a row's segment: the block, the 3 bits of an empty stored block, the padding to a byte, 00 00 FF FF
inline uint64_t row_segment_bytes(uint64_t block_bits) { return (block_bits + 3 + 7) / 8 + 4; }
// the zlib stream around `rows_bytes` of segments: 78 01 in front, 03 00 and the Adler-32 behind
inline uint64_t zlib_bytes(uint64_t rows_bytes) { return 2 + rows_bytes + 2 + 4; }
// the file: signature, IHDR, the IDAT chunks (one below 2^31 - 1 bytes of stream), IEND
uint64_t file_bytes(uint64_t rows_bytes, uint64_t max_idat = MAX_IDAT_BYTES);
// what no frame of this size exceeds, of either kind (every literal 15 bits, a header of HEADER_MAX_BITS a row; a match stands for 4 bytes
// or more and is 15 + 5 + 1 bits at most, less than its bytes' 60): gr_png_encode_bound; 0 for a bad size
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
