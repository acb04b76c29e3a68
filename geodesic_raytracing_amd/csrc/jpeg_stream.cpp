// jpeg_stream.cpp — the JPEG stream of both JPEG encoders (jpeg_stream.hpp; geodesic_hip_internal.h, "JPEG frames"): colour, DCT,
// quantiser, Huffman tables, headers, and the host encoder that defines the bytes.  No HIP header.
#include "jpeg_stream.hpp"

#include <algorithm>
#include <cstring>

#include "internal.hpp"

namespace jpeg_stream {

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// round(2^14 c[u][x]): c[0][x] = 1 / (2 sqrt 2), c[u][x] = cos((2x + 1) u pi / 16) / 2
const int32_t DCT[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},     {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                           {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568}, {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                           {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793}, {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                           {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135}, {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};

namespace {
// ITU-T T.81 Annex K.1: the luminance and chrominance quantisation tables, natural order
const uint8_t K1_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                             18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t K1_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: codes of each length 1 ... 16, then the symbols in code order - DC then AC, luminance then chrominance
const uint8_t K3_DC_COUNTS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t K3_DC_SYMBOLS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t K3_AC_COUNTS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t K3_AC_SYMBOLS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code | length << 16 of every symbol of a table given as Annex C has it: codes count up within a length and double from one to the next
void codes_of(const uint8_t counts[16], const uint8_t* symbols, uint32_t* by_symbol, int entries) {
    std::fill(by_symbol, by_symbol + entries, 0u);
    uint32_t code = 0;
    int at = 0;
    for (int length = 1; length <= 16; length++, code <<= 1)
        for (int k = 0; k < counts[length - 1]; k++) by_symbol[symbols[at++]] = code++ | ((uint32_t)length << 16);
}

void put_be16(uint8_t*& at, unsigned v) {
    *at++ = (uint8_t)(v >> 8);
    *at++ = (uint8_t)v;
}
void put_marker(uint8_t*& at, unsigned marker, unsigned payload) {
    *at++ = 0xff;
    *at++ = (uint8_t)marker;
    put_be16(at, payload + 2);
}

// the size category of a value: the bits of its magnitude
int category(int32_t v) {
    uint32_t magnitude = (uint32_t)(v < 0 ? -v : v);
    int bits = 0;
    for (; magnitude; magnitude >>= 1) bits++;
    return bits;
}

// an MCU row's entropy-coded bits, most significant bit first
struct bit_string {
    std::vector<uint8_t> bytes;
    uint32_t pending = 0;
    int held = 0;   // bits of `pending`, below 8 between calls
    void put(uint32_t value, int count) {
        for (int b = count - 1; b >= 0; b--) {
            pending = (pending << 1) | ((value >> b) & 1u);
            if (++held == 8) {
                bytes.push_back((uint8_t)pending);
                pending = 0;
                held = 0;
            }
        }
    }
    void put_code(uint32_t entry) { put(entry & 0xffffu, (int)(entry >> 16)); }
    // a value of a category: itself when positive, its low bits minus one when negative (T.81 F.1.2.1)
    void put_value(int32_t v, int bits) { put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << bits) - 1u), bits); }
};
}   // namespace

void quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; i++) {
        luma[i] = (uint8_t)std::min(std::max((K1_LUMA[i] * scale + 50) / 100, 1), 255);
        chroma[i] = (uint8_t)std::min(std::max((K1_CHROMA[i] * scale + 50) / 100, 1), 255);
    }
}

int32_t convert(int component, int32_t r, int32_t g, int32_t b) {
    // 2^16 x (0.299, 0.587, 0.114), (-0.168736, -0.331264, 0.5), (0.5, -0.418688, -0.081312), each row summing to 2^16 or to 0; + 2^15 and an
    // arithmetic shift right by 16: rounded to nearest, halves up
    const int32_t sum = component == 0 ? 19595 * r + 38470 * g + 7471 * b : component == 1 ? -11059 * r - 21709 * g + 32768 * b : 32768 * r - 27439 * g - 5329 * b;
    const int32_t centred = ((sum + 32768) >> 16) - (component == 0 ? 128 : 0);
    return std::min(std::max(centred, -128), 127);   // the sample clamped to 0 ... 255
}

void fdct(const int16_t samples[64], int32_t out[64]) {
    int32_t rows[64];
    for (int y = 0; y < 8; y++)
        for (int u = 0; u < 8; u++) {
            int32_t sum = 0;
            for (int x = 0; x < 8; x++) sum += DCT[u][x] * samples[8 * y + x];
            rows[8 * y + u] = (sum + 128) >> 8;   // 14 fraction bits to 6
        }
    for (int u = 0; u < 8; u++)
        for (int v = 0; v < 8; v++) {
            int32_t sum = 0;
            for (int y = 0; y < 8; y++) sum += DCT[v][y] * rows[8 * y + u];
            out[8 * v + u] = (sum + 32768) >> 16;   // 20 fraction bits to 4
        }
}

namespace {
// one block: its 64 samples gathered by `sample(x, y)`, transformed, quantised, written in zig-zag order
template <class F>
void block_of(F sample, const uint8_t steps[64], int16_t* out) {
    int16_t samples[64];
    int32_t coefficients[64];
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++) samples[8 * y + x] = (int16_t)sample(x, y);
    fdct(samples, coefficients);
    for (int k = 0; k < 64; k++) out[k] = (int16_t)quantise(coefficients[ZIGZAG[k]], steps[ZIGZAG[k]]);
}
}   // namespace

void blocks(const unsigned char* rgba8, int width, int height, int quality, int16_t* out) {
    uint8_t luma[64], chroma[64];
    quant_tables(quality, luma, chroma);
    // a pixel past the right or the bottom edge is the last one of its row or column
    auto pixel = [&](int x, int y) { return rgba8 + 4 * ((size_t)std::min(y, height - 1) * (size_t)width + (size_t)std::min(x, width - 1)); };
    for (int my = 0; my < mcu_rows(height); my++)
        for (int mx = 0; mx < mcus_across(width); mx++) {
            const int x0 = mx * MCU, y0 = my * MCU;
            for (int j = 0; j < 4; j++, out += 64)
                block_of([&](int x, int y) {
                    const unsigned char* p = pixel(x0 + 8 * (j & 1) + x, y0 + 8 * (j >> 1) + y);
                    return convert(0, p[0], p[1], p[2]);
                }, luma, out);
            // chroma: the rounded mean of the 2 x 2 pixels' R, G and B, converted once
            for (int component = 1; component <= 2; component++, out += 64)
                block_of([&](int x, int y) {
                    int32_t sum[3] = {2, 2, 2};
                    for (int j = 0; j < 2; j++)
                        for (int i = 0; i < 2; i++) {
                            const unsigned char* p = pixel(x0 + 2 * x + i, y0 + 2 * y + j);
                            for (int c = 0; c < 3; c++) sum[c] += p[c];
                        }
                    return convert(component, sum[0] >> 2, sum[1] >> 2, sum[2] >> 2);
                }, chroma, out);
        }
}

void device_tables(int quality, uint32_t* words) {
    std::fill(words, words + TABLE_WORDS, 0u);
    uint8_t steps[2][64];
    quant_tables(quality, steps[0], steps[1]);
    for (int cls = 0; cls < 2; cls++) {
        codes_of(K3_DC_COUNTS[cls], K3_DC_SYMBOLS, words + TABLE_DC + 16 * cls, 16);
        codes_of(K3_AC_COUNTS[cls], K3_AC_SYMBOLS[cls], words + TABLE_AC + 256 * cls, 256);
        for (int i = 0; i < 64; i++) {
            // quantise() without a division: with d = 16 step (16 ... 4 080) and M = ceil(2^32 / d), floor(n M / 2^32) = floor(n / d) for every
            // n with n (M d - 2^32) < 2^32, and n = |coefficient| + 8 step stays below 2^15 while M d - 2^32 < d < 2^12
            const uint64_t d = 16ull * steps[cls][i];
            words[TABLE_RECIPROCAL + 64 * cls + i] = (uint32_t)(((1ull << 32) + d - 1) / d);
            words[TABLE_HALF + 64 * cls + i] = 8u * steps[cls][i];
        }
    }
}

void write_headers(uint8_t* out, int width, int height, int quality) {
    uint8_t* at = out;
    *at++ = 0xff;
    *at++ = 0xd8;                     // SOI
    put_marker(at, 0xe0, 14);         // APP0
    memcpy(at, "JFIF", 5);
    at += 5;
    *at++ = 1;                        // version 1.01
    *at++ = 1;
    *at++ = 0;                        // no units: the densities are an aspect ratio, 1:1
    put_be16(at, 1);
    put_be16(at, 1);
    *at++ = 0;                        // no thumbnail
    *at++ = 0;
    uint8_t steps[2][64];
    quant_tables(quality, steps[0], steps[1]);
    for (int cls = 0; cls < 2; cls++) {
        put_marker(at, 0xdb, 65);     // DQT: 8-bit entries, table `cls`, zig-zag order
        *at++ = (uint8_t)cls;
        for (int k = 0; k < 64; k++) *at++ = steps[cls][ZIGZAG[k]];
    }
    put_marker(at, 0xc0, 15);         // SOF0: baseline, 8 bits, three components
    *at++ = 8;
    put_be16(at, (unsigned)height);
    put_be16(at, (unsigned)width);
    *at++ = 3;
    const uint8_t components[3][3] = {{1, 0x22, 0}, {2, 0x11, 1}, {3, 0x11, 1}};   // id, sampling h << 4 | v, quantisation table
    for (auto& c : components)
        for (uint8_t v : c) *at++ = v;
    for (int cls = 0; cls < 2; cls++) {
        put_marker(at, 0xc4, 1 + 16 + 12);    // DHT: DC table `cls`
        *at++ = (uint8_t)cls;
        memcpy(at, K3_DC_COUNTS[cls], 16);
        memcpy(at + 16, K3_DC_SYMBOLS, 12);
        at += 28;
        put_marker(at, 0xc4, 1 + 16 + 162);   // DHT: AC table `cls`
        *at++ = (uint8_t)(0x10 | cls);
        memcpy(at, K3_AC_COUNTS[cls], 16);
        memcpy(at + 16, K3_AC_SYMBOLS[cls], 162);
        at += 178;
    }
    put_marker(at, 0xdd, 2);          // DRI: one MCU row a restart interval
    put_be16(at, (unsigned)mcus_across(width));
    put_marker(at, 0xda, 10);         // SOS: three components, their DC << 4 | AC tables, the whole spectrum, no approximation
    *at++ = 3;
    const uint8_t scan[3][2] = {{1, 0x00}, {2, 0x11}, {3, 0x11}};
    for (auto& c : scan)
        for (uint8_t v : c) *at++ = v;
    *at++ = 0;
    *at++ = 63;
    *at++ = 0;
}

std::string size_refusal(int width, int height) {
    if (width < 1 || height < 1) return "a size below 1";
    if (width > MAX_SIZE || height > MAX_SIZE) return "a size above 65535 (a JPEG frame header holds width and height in 16 bits)";
    return "";
}

std::string quality_refusal(int quality) {
    return quality < 1 || quality > 100 ? "a quality of " + std::to_string(quality) + " (1 to 100)" : "";
}

std::string refusal(const void* rgba8, int width, int height, int quality, const void* out_file, size_t capacity, const void* out_bytes, bool* too_small) {
    *too_small = false;
    if (!rgba8 || !out_file || !out_bytes) return "a required pointer is NULL";
    std::string wrong = size_refusal(width, height);
    if (wrong.empty()) wrong = quality_refusal(quality);
    if (!wrong.empty()) return wrong;
    if ((uintptr_t)rgba8 % 4) return "the frame is not aligned to 4 bytes";
    const uint64_t need = file_bound(width, height);
    if ((uint64_t)capacity < need) {
        *too_small = true;
        return "a capacity of " + std::to_string(capacity) + " bytes, " + std::to_string(need) + " needed (gr_jpeg_encode_bound)";
    }
    return "";
}

}  // namespace jpeg_stream

// ---------------------------------------------------------------------------------------------------------------- exports

namespace js = jpeg_stream;

using gr_internal::refuse;

extern "C" {

int gr_jpeg_encode_bound(int width, int height, size_t* bytes) {
    const char* who = "gr_jpeg_encode_bound";
    if (!bytes) return refuse(who, "a required pointer is NULL");
    const std::string wrong = js::size_refusal(width, height);
    if (!wrong.empty()) return refuse(who, wrong);
    *bytes = (size_t)js::file_bound(width, height);
    return GR_OK;
}

int gr_jpeg_quant_tables(int quality, unsigned char luma[64], unsigned char chroma[64]) {
    const char* who = "gr_jpeg_quant_tables";
    if (!luma || !chroma) return refuse(who, "a required pointer is NULL");
    const std::string wrong = js::quality_refusal(quality);
    if (!wrong.empty()) return refuse(who, wrong);
    js::quant_tables(quality, luma, chroma);
    return GR_OK;
}

int gr_jpeg_fdct_host(const short* samples, int* coefficients_x16) {
    if (!samples || !coefficients_x16) return refuse("gr_jpeg_fdct_host", "a required pointer is NULL");
    for (int i = 0; i < 64; i++)
        if (samples[i] < -128 || samples[i] > 127) return refuse("gr_jpeg_fdct_host", "a sample outside -128 to 127");
    js::fdct(samples, coefficients_x16);
    return GR_OK;
}

int gr_jpeg_blocks_host(const unsigned char* rgba8, int width, int height, int quality, short* out) {
    const char* who = "gr_jpeg_blocks_host";
    if (!rgba8 || !out) return refuse(who, "a required pointer is NULL");
    std::string wrong = js::size_refusal(width, height);
    if (wrong.empty()) wrong = js::quality_refusal(quality);
    if (!wrong.empty()) return refuse(who, wrong);
    js::blocks(rgba8, width, height, quality, out);
    return GR_OK;
}

int gr_jpeg_encode_rgba8_host(const unsigned char* rgba8, int width, int height, int quality, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    const char* who = "gr_jpeg_encode_rgba8_host";
    bool too_small = false;
    const std::string wrong = js::refusal(rgba8, width, height, quality, out_file, capacity, out_bytes, &too_small);
    if (!wrong.empty()) return refuse(who, wrong, too_small);
    const int across = js::mcus_across(width), rows = js::mcu_rows(height);
    std::vector<int16_t> coefficients((size_t)across * rows * js::BLOCKS_PER_MCU * 64);
    js::blocks(rgba8, width, height, quality, coefficients.data());
    std::vector<uint32_t> tables(js::TABLE_WORDS);
    js::device_tables(quality, tables.data());
    js::write_headers(out_file, width, height, quality);
    uint8_t* at = out_file + js::HEADER_BYTES;
    const int16_t* block = coefficients.data();
    for (int row = 0; row < rows; row++) {
        js::bit_string bits;
        int32_t predictor[3] = {0, 0, 0};   // a restart interval starts from 0
        for (int mcu = 0; mcu < across; mcu++)
            for (int b = 0; b < js::BLOCKS_PER_MCU; b++, block += 64) {
                const int component = b < 4 ? 0 : b - 3, cls = b < 4 ? 0 : 1;
                const uint32_t* dc = tables.data() + js::TABLE_DC + 16 * cls;
                const uint32_t* ac = tables.data() + js::TABLE_AC + 256 * cls;
                const int32_t difference = block[0] - predictor[component];
                predictor[component] = block[0];
                int size = js::category(difference);
                bits.put_code(dc[size]);
                bits.put_value(difference, size);
                int run = 0;
                for (int k = 1; k < 64; k++) {
                    if (!block[k]) {
                        run++;
                        continue;
                    }
                    for (; run >= 16; run -= 16) bits.put_code(ac[0xf0]);   // ZRL: sixteen zeros
                    size = js::category(block[k]);
                    bits.put_code(ac[run << 4 | size]);
                    bits.put_value(block[k], size);
                    run = 0;
                }
                if (run) bits.put_code(ac[0x00]);   // EOB
            }
        if (bits.held) bits.put((1u << (8 - bits.held)) - 1u, 8 - bits.held);   // 1-bits up to the byte boundary
        if (bits.bytes.size() > js::row_bytes_bound(width)) return refuse(who, "an MCU row's segment exceeds the bound computed for it");
        for (uint8_t byte : bits.bytes) {
            *at++ = byte;
            if (byte == 0xff) *at++ = 0x00;
        }
        *at++ = 0xff;
        *at++ = row + 1 < rows ? (uint8_t)(0xd0 + row % 8) : (uint8_t)0xd9;   // RSTm, or EOI behind the last row
    }
    *out_bytes = (size_t)(at - out_file);
    return GR_OK;
}

}   // extern "C"
