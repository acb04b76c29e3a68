// exr_stream.cpp — the OpenEXR file of both EXR encoders (exr_stream.hpp; geodesic_hip_internal.h, "EXR frames"): header, rows, table,
// sizes, and the host encoder that defines the bytes.  No HIP header.
#include "exr_stream.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "internal.hpp"

namespace exr_stream {

namespace {
struct writer {
    uint8_t* at;
    void bytes(const void* data, size_t n) { memcpy(at, data, n); at += n; }
    void text(const char* s) { bytes(s, strlen(s) + 1); }   // (with its closing 0)
    void u8(uint8_t v) { *at++ = v; }
    void i32(int32_t v) { const uint32_t u = (uint32_t)v; for (int k = 0; k < 4; k++) u8((uint8_t)(u >> (8 * k))); }
    void f32(float v) { int32_t bits; memcpy(&bits, &v, 4); i32(bits); }
    void attribute(const char* name, const char* type, int32_t size) { text(name); text(type); i32(size); }
};
void put_le32(uint8_t* at, uint32_t v) { for (int k = 0; k < 4; k++) at[k] = (uint8_t)(v >> (8 * k)); }
void put_le64(uint8_t* at, uint64_t v) { for (int k = 0; k < 8; k++) at[k] = (uint8_t)(v >> (8 * k)); }
}   // namespace

void write_header(uint8_t* out, int width, int height) {
    writer w{out};
    static const uint8_t MAGIC_AND_VERSION[8] = {0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0};   // version 2, no flag: one part, scan lines, short names
    w.bytes(MAGIC_AND_VERSION, 8);
    w.attribute("channels", "chlist", 3 * 18 + 1);
    for (const char* name : {"B", "G", "R"}) {   // (a chlist is sorted by name)
        w.text(name);
        w.i32(1);   // HALF
        w.u8(0);    // pLinear
        w.u8(0), w.u8(0), w.u8(0);
        w.i32(1), w.i32(1);   // sampling
    }
    w.u8(0);
    w.attribute("compression", "compression", 1);
    w.u8(2);   // ZIPS: zlib, one scan line a chunk
    for (const char* name : {"dataWindow", "displayWindow"}) {
        w.attribute(name, "box2i", 16);
        w.i32(0), w.i32(0), w.i32(width - 1), w.i32(height - 1);
    }
    w.attribute("lineOrder", "lineOrder", 1);
    w.u8(0);   // increasing y
    w.attribute("pixelAspectRatio", "float", 4);
    w.f32(1.f);
    w.attribute("screenWindowCenter", "v2f", 8);
    w.f32(0.f), w.f32(0.f);
    w.attribute("screenWindowWidth", "float", 4);
    w.f32(1.f);
    w.u8(0);
    static_assert(HEADER_BYTES == 8 + 75 + 29 + 37 + 40 + 25 + 31 + 35 + 32 + 1, "the header's size");
}

void raw_row(const float* frame_rgba_f32, int width, int row, uint8_t* raw) {
    const float* pixels = frame_rgba_f32 + 4 * (size_t)row * (size_t)width;
    for (int plane = 0; plane < 3; plane++)   // B, G, R: components 2, 1, 0
        for (int x = 0; x < width; x++) {
            uint32_t bits;
            memcpy(&bits, pixels + 4 * (size_t)x + (2 - plane), 4);
            const uint16_t h = half_bits(bits);
            uint8_t* at = raw + 2 * ((size_t)plane * (size_t)width + (size_t)x);
            at[0] = (uint8_t)h;
            at[1] = (uint8_t)(h >> 8);
        }
}

void predicted_row(const uint8_t* raw, size_t bytes, uint8_t* out) {
    const size_t half = (bytes + 1) / 2;
    for (size_t i = 0; i < bytes; i++) out[(i & 1 ? half : 0) + i / 2] = raw[i];
    uint8_t before = out[0];
    for (size_t i = 1; i < bytes; i++) {
        const uint8_t here = out[i];
        out[i] = (uint8_t)(here - before + 128);
        before = here;
    }
}

void build_table(const uint64_t* histogram, png_stream::table& out) {
    png_stream::build_table(histogram, GR_PNG_STREAM_LITERALS, out);
    out.header[0] |= 1u;   // BFINAL: a row's stream is this one block
}

uint64_t row_block_bits(const png_stream::table& t, const uint32_t* row_histogram) {
    uint64_t bits = (uint64_t)t.header_bits + t.length[END_OF_BLOCK];
    for (int v = 0; v < 256; v++) bits += (uint64_t)t.length[v] * row_histogram[v];
    return bits;
}

uint32_t row_adler(int width, uint32_t sum, uint32_t weighted) {
    const uint64_t M = 65521, n = row_bytes(width);
    return (uint32_t)((((n % M + weighted) % M) << 16) | ((1 + sum) % M));
}

uint64_t file_bound(int width, int height) {
    if (width < 1 || height < 1 || row_bytes(width) > MAX_ROW_BYTES) return 0;
    return chunks_at(height) + (uint64_t)height * (CHUNK_HEADER_BYTES + row_bytes(width));
}

void write_offsets(uint8_t* out_file, int height, const uint64_t* chunk_offset) {
    for (int r = 0; r < height; r++) put_le64(out_file + HEADER_BYTES + 8 * (size_t)r, chunks_at(height) + chunk_offset[r]);
}

std::string refusal(const void* frame, int width, int height, const void* out_file, size_t capacity, const void* out_bytes, bool aligned_frame,
                    bool* too_small) {
    *too_small = false;
    if (!frame || !out_file || !out_bytes) return "a required pointer is NULL";
    if (width < 1 || height < 1) return "a size below 1 (width " + std::to_string(width) + ", height " + std::to_string(height) + ")";
    if (row_bytes(width) > MAX_ROW_BYTES) return "a row of more than 2^31 - 1 raw bytes (width " + std::to_string(width) + ", 6 bytes a pixel)";
    const uint64_t need = file_bound(width, height);
    if ((uint64_t)capacity < need) {
        *too_small = true;
        return "a capacity of " + std::to_string(capacity) + " bytes, " + std::to_string(need) + " needed (gr_exr_encode_bound)";
    }
    if (aligned_frame && (uintptr_t)frame % 16) return "the frame is not aligned to 16 bytes";
    return "";
}

}  // namespace exr_stream

// ---------------------------------------------------------------------------------------------------------------- exports

namespace es = exr_stream;

using gr_internal::refuse;

namespace {
int encode_host(const char* who, const float* frame, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes, bool aligned_frame) {
    bool too_small = false;
    const std::string wrong = es::refusal(frame, width, height, out_file, capacity, out_bytes, aligned_frame, &too_small);
    if (!wrong.empty()) return refuse(who, wrong, too_small);
    const size_t n = (size_t)es::row_bytes(width);
    std::vector<uint8_t> raw(n), predicted(n);
    // first pass: the rows' histograms - the frame's is their sum, every row counted, plus one end-of-block a row
    std::vector<uint32_t> row_histogram((size_t)height * 256, 0u);
    uint64_t histogram[png_stream::MAX_SYMBOLS] = {};
    for (int r = 0; r < height; r++) {
        es::raw_row(frame, width, r, raw.data());
        es::predicted_row(raw.data(), n, predicted.data());
        uint32_t* mine = &row_histogram[(size_t)r * 256];
        for (size_t i = 0; i < n; i++) mine[predicted[i]]++;
        for (int v = 0; v < 256; v++) histogram[v] += mine[v];
    }
    histogram[es::END_OF_BLOCK] = (uint64_t)height;
    png_stream::table t;
    es::build_table(histogram, t);
    // the sizes, before a bit is packed: which rows are stored raw, where every chunk lies
    std::vector<uint64_t> offset((size_t)height + 1, 0);
    for (int r = 0; r < height; r++) {
        const uint64_t stream = es::stream_bytes(es::row_block_bits(t, &row_histogram[(size_t)r * 256]));
        offset[r + 1] = offset[r] + es::CHUNK_HEADER_BYTES + (es::stored_raw(stream, width) ? n : stream);
    }
    es::write_header(out_file, width, height);
    es::write_offsets(out_file, height, offset.data());
    uint8_t* chunks = out_file + es::chunks_at(height);
    // second pass: the chunks
    for (int r = 0; r < height; r++) {
        uint8_t* chunk = chunks + offset[r];
        const uint64_t size = offset[r + 1] - offset[r] - es::CHUNK_HEADER_BYTES;
        es::put_le32(chunk, (uint32_t)r);
        es::put_le32(chunk + 4, (uint32_t)size);
        uint8_t* data = chunk + es::CHUNK_HEADER_BYTES;
        es::raw_row(frame, width, r, raw.data());
        if (size == n) {
            memcpy(data, raw.data(), n);
            continue;
        }
        es::predicted_row(raw.data(), n, predicted.data());
        memset(data, 0, (size_t)size);
        data[0] = 0x78, data[1] = 0x01;
        uint8_t* block = data + 2;
        uint64_t at = 0;   // in bits
        auto put = [&](uint32_t value, int count) {
            for (int b = 0; b < count; b++, at++)
                if ((value >> b) & 1u) block[at >> 3] |= (uint8_t)(1u << (at & 7));
        };
        for (int b = 0; b < t.header_bits; b += 32) put(t.header[b >> 5], std::min(32, t.header_bits - b));
        for (size_t i = 0; i < n; i++) put(t.code[predicted[i]], t.length[predicted[i]]);
        put(t.code[es::END_OF_BLOCK], t.length[es::END_OF_BLOCK]);
        if (es::stream_bytes(at) != size) return refuse(who, "a row's stream is not the size computed for it", false);
        uLong a = adler32(0, nullptr, 0);
        for (size_t done = 0; done < n;) {
            const size_t piece = std::min<size_t>(n - done, 1u << 30);
            a = adler32(a, predicted.data() + done, (uInt)piece);
            done += piece;
        }
        uint8_t* sum = data + size - 4;
        sum[0] = (uint8_t)(a >> 24), sum[1] = (uint8_t)(a >> 16), sum[2] = (uint8_t)(a >> 8), sum[3] = (uint8_t)a;
    }
    *out_bytes = (size_t)(es::chunks_at(height) + offset[height]);
    return GR_OK;
}
}   // namespace

extern "C" {

int gr_exr_encode_bound(int width, int height, size_t* bytes) {
    const char* who = "gr_exr_encode_bound";
    if (!bytes) return refuse(who, "a required pointer is NULL", false);
    if (width < 1 || height < 1) return refuse(who, "a size below 1 (width " + std::to_string(width) + ", height " + std::to_string(height) + ")", false);
    const uint64_t bound = es::file_bound(width, height);
    if (!bound) return refuse(who, "a row of more than 2^31 - 1 raw bytes (width " + std::to_string(width) + ", 6 bytes a pixel)", false);
    *bytes = (size_t)bound;
    return GR_OK;
}

int gr_exr_half_bits(const float* values, size_t count, unsigned short* out) {
    if (!values || !out) return refuse("gr_exr_half_bits", "a required pointer is NULL", false);
    for (size_t i = 0; i < count; i++) {
        uint32_t bits;
        memcpy(&bits, values + i, 4);
        out[i] = es::half_bits(bits);
    }
    return GR_OK;
}

int gr_exr_encode_f32_host(const float* frame_rgba_f32, int width, int height, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    return encode_host("gr_exr_encode_f32_host", frame_rgba_f32, width, height, out_file, capacity, out_bytes, true);
}

int gr_write_frame_exr(const char* path, const float* frame_rgba_f32, int width, int height) {
    const char* who = "gr_write_frame_exr";
    if (!path) return refuse(who, "a required pointer is NULL", false);
    size_t bound = 0, bytes = 0;
    if (!frame_rgba_f32) return refuse(who, "a required pointer is NULL", false);
    if (width < 1 || height < 1) return refuse(who, "a size below 1 (width " + std::to_string(width) + ", height " + std::to_string(height) + ")", false);
    if (!(bound = (size_t)es::file_bound(width, height))) return refuse(who, "a row of more than 2^31 - 1 raw bytes", false);
    std::vector<unsigned char> file(bound);
    const int rc = encode_host(who, frame_rgba_f32, width, height, file.data(), bound, &bytes, false);   // (the host reads floats: no alignment asked)
    if (rc != GR_OK) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) return refuse(who, std::string("cannot write ") + path, false);
    const bool written = fwrite(file.data(), 1, bytes, f) == bytes;
    if (fclose(f) != 0 || !written) return refuse(who, std::string("cannot write ") + path, false);
    return GR_OK;
}

}   // extern "C"
