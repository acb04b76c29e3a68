// imageio.cpp — PNG in/out for the headless renderer (host side, not on the hot path), and video frames: the host statement of the
// 8-bit Y'CbCr 4:2:0 encode (gr_rgba8_to_yuv420, which kernels/present.hip's gr_present_yuv420 is held to), of the 10-bit one
// (gr_frame_to_rgb10 and gr_rgb10_to_yuv420p10, which gr_present_yuv420p10 is held to) and a YUV4MPEG2 writer for both depths.
//
// Reference counterparts: the screenshot path main.cpp:2762-2808 (read the float4 frame, clamp, linear -> sRGB,
// clamp, 8-bit, PNG through sf::Image) and the background loader graphics_settings.cpp:214-243 (sf::Image from a
// PNG, handed to load_mipped_image).  SFML is not part of the reference checkout; this is a minimal PNG codec on zlib:
// writer = RGBA8, filter 0; reader = 8-bit greyscale / RGB / RGBA / palette, non-interlaced, all five filters.
#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frame_format.hpp"
#include "internal.hpp"

namespace {

void put32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back(x >> 24); v.push_back(x >> 16); v.push_back(x >> 8); v.push_back(x);
}

void chunk(std::vector<uint8_t>& out, const char* type, const std::vector<uint8_t>& data) {
    put32(out, (uint32_t)data.size());
    size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    out.insert(out.end(), data.begin(), data.end());
    put32(out, (uint32_t)crc32(0, out.data() + start, (uInt)(out.size() - start)));
}

// lin_to_srgb_single, cl.cl:326-332 (the host applies the same curve, main.cpp:2797)
float lin_to_srgb(float v) { return v <= 0.0031308f ? v * 12.92f : 1.055f * std::pow(v, 1.0f / 2.4f) - 0.055f; }
float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// The 8-bit encode of one value, stated once (main.cpp:2791-2796): clamp, linear -> sRGB, clamp, * 255 truncated.  gr_frame_to_rgba8
// applies it to a frame; gr_srgb8_thresholds inverts it into the table the device encode (kernels/present.hip) searches.  A NaN passes
// both clamps and its cast is undefined.
unsigned char srgb8(float v) {
    const float c = clamp01(v);
    const float s = clamp01(lin_to_srgb(c));
    return (unsigned char)(s * 255.f);
}

// The 10-bit encode of one value: srgb8's chain with 1 023 for 255 (geodesic_hip_internal.h, "10-bit video frames").  gr_frame_to_rgb10
// applies it; gr_srgb10_thresholds inverts it into the table gr_present_yuv420p10 searches.  A NaN's code is undefined, as its byte is.
int code10(float v) {
    const float c = clamp01(v);
    const float s = clamp01(lin_to_srgb(c));
    return (int)(s * 1023.f);
}

uint32_t get32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

int paeth(int a, int b, int c) {
    int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

}  // namespace

extern "C" {

int gr_write_png_rgba8(const char* path, const unsigned char* rgba, int width, int height) {
    if (!path || !rgba || width <= 0 || height <= 0) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "bad image");
    std::vector<uint8_t> raw((size_t)height * ((size_t)width * 4 + 1));
    for (int y = 0; y < height; y++) {
        raw[(size_t)y * (width * 4 + 1)] = 0;   // filter type 0
        memcpy(&raw[(size_t)y * (width * 4 + 1) + 1], rgba + (size_t)y * width * 4, (size_t)width * 4);
    }
    uLongf bound = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(bound);
    if (compress2(z.data(), &bound, raw.data(), (uLong)raw.size(), 6) != Z_OK) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "deflate failed");
    z.resize(bound);
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<uint8_t> ihdr;
    put32(ihdr, (uint32_t)width);
    put32(ihdr, (uint32_t)height);
    ihdr.insert(ihdr.end(), {8, 6, 0, 0, 0});   // 8 bit, RGBA, deflate, adaptive filtering, no interlace
    chunk(out, "IHDR", ihdr);
    chunk(out, "IDAT", z);
    chunk(out, "IEND", {});
    FILE* f = fopen(path, "wb");
    if (!f) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string("cannot write ") + path).c_str());
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return GR_OK;
}

// the screenshot conversion of main.cpp:2791-2800: clamp, linear -> sRGB (all four channels), clamp, * 255 truncated.  The byte of a
// NaN is undefined here (the device encode, gr_present_rgba8, writes 0 for it).
int gr_frame_to_rgba8(const float* frame_rgba_f32, int width, int height, unsigned char* out_rgba8) {
    if (!frame_rgba_f32 || !out_rgba8) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    size_t n = (size_t)width * height * 4;
    for (size_t i = 0; i < n; i++) out_rgba8[i] = srgb8(frame_rgba_f32[i]);
    return GR_OK;
}

// out[k] = the smallest float of [0, 1] whose byte is >= k (+infinity where none is: 1.055f - 0.055f need not be 1), found by bisection
// over the bit patterns 0 ... 0x3f800000 with srgb8 itself - which is monotone there (tests/test_present_abi.py checks it against
// this library's own powf).  byte(c) is then the largest k with out[k] <= c, whatever libm is underneath.
int gr_srgb8_thresholds(float out[256]) {
    if (!out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    auto of_bits = [](uint32_t bits) { float f; memcpy(&f, &bits, sizeof(f)); return f; };
    const uint32_t one = 0x3f800000u;
    const int top = srgb8(of_bits(one));
    out[0] = 0.f;
    for (int k = 1; k < 256; k++) {
        if (k > top) { out[k] = INFINITY; continue; }
        uint32_t lo = 0, hi = one;   // byte(lo) < k <= byte(hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (srgb8(of_bits(mid)) >= k) hi = mid; else lo = mid;
        }
        out[k] = of_bits(hi);
    }
    return GR_OK;
}

int gr_write_frame_png(const char* path, const float* frame_rgba_f32, int width, int height) {
    std::vector<unsigned char> px((size_t)width * height * 4);
    int rc = gr_frame_to_rgba8(frame_rgba_f32, width, height, px.data());
    if (rc != GR_OK) return rc;
    return gr_write_png_rgba8(path, px.data(), width, height);
}

// Reads a PNG into RGBA8.  Call with out = NULL to get the size.
int gr_read_png_rgba8(const char* path, int* width, int* height, unsigned char* out, size_t capacity) {
    if (!path || !width || !height) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string("cannot read ") + path).c_str());
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + n);
    fclose(f);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (file.size() < 33 || memcmp(file.data(), sig, 8) != 0) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "not a PNG file");
    uint32_t w = 0, h = 0;
    int depth = 0, colour = 0, interlace = 0;
    std::vector<uint8_t> idat, palette, trns;
    for (size_t p = 8; p + 12 <= file.size();) {
        uint32_t len = get32(&file[p]);
        if (p + 12 + len > file.size()) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "truncated PNG");
        const uint8_t* type = &file[p + 4];
        const uint8_t* data = &file[p + 8];
        if (!memcmp(type, "IHDR", 4)) { w = get32(data); h = get32(data + 4); depth = data[8]; colour = data[9]; interlace = data[12]; }
        else if (!memcmp(type, "PLTE", 4)) palette.assign(data, data + len);
        else if (!memcmp(type, "tRNS", 4)) trns.assign(data, data + len);
        else if (!memcmp(type, "IDAT", 4)) idat.insert(idat.end(), data, data + len);
        else if (!memcmp(type, "IEND", 4)) break;
        p += 12 + len;
    }
    if (!w || !h || depth != 8 || interlace != 0) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "unsupported PNG (need 8-bit, non-interlaced)");
    int channels = colour == 0 ? 1 : colour == 2 ? 3 : colour == 3 ? 1 : colour == 4 ? 2 : colour == 6 ? 4 : 0;
    if (!channels) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "unsupported PNG colour type");
    *width = (int)w;
    *height = (int)h;
    if (!out) return GR_OK;
    if (capacity < (size_t)w * h * 4) return gr_internal_fail(GR_ERROR_BUFFER_TOO_SMALL, "buffer too small");
    size_t stride = (size_t)w * channels;
    std::vector<uint8_t> raw((stride + 1) * h);
    uLongf raw_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &raw_len, idat.data(), (uLong)idat.size()) != Z_OK || raw_len != raw.size())
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "PNG inflate failed");
    std::vector<uint8_t> prev(stride, 0), cur(stride);
    for (uint32_t y = 0; y < h; y++) {
        const uint8_t* line = &raw[y * (stride + 1)];
        int filter = line[0];
        for (size_t x = 0; x < stride; x++) {
            int a = x >= (size_t)channels ? cur[x - channels] : 0, b = prev[x], c = x >= (size_t)channels ? prev[x - channels] : 0;
            int v = line[1 + x];
            switch (filter) {
                case 0: break;
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) / 2; break;
                case 4: v += paeth(a, b, c); break;
                default: return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "bad PNG filter");
            }
            cur[x] = (uint8_t)v;
        }
        unsigned char* o = out + (size_t)y * w * 4;
        for (uint32_t x = 0; x < w; x++) {
            const uint8_t* s = &cur[(size_t)x * channels];
            switch (colour) {
                case 0: o[0] = o[1] = o[2] = s[0]; o[3] = 255; break;
                case 2: o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = 255; break;
                case 3: {
                    size_t i = s[0];
                    o[0] = i * 3 + 2 < palette.size() ? palette[i * 3] : 0;
                    o[1] = i * 3 + 2 < palette.size() ? palette[i * 3 + 1] : 0;
                    o[2] = i * 3 + 2 < palette.size() ? palette[i * 3 + 2] : 0;
                    o[3] = i < trns.size() ? trns[i] : 255;
                    break;
                }
                case 4: o[0] = o[1] = o[2] = s[0]; o[3] = s[1]; break;
                case 6: o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; break;
            }
            o += 4;
        }
        prev.swap(cur);
    }
    return GR_OK;
}

// ---- video frames (include/geodesic_hip.h says all of it: formulas, siting, layouts, the stream's format) ----------------------------

size_t gr_yuv420_bytes(int width, int height) { return frame_format::yuv420_bytes(width, height); }

// BT.709, limited range, 16 fractional bits, int32 throughout (the largest intermediate is 28784 * 1020 + 131072 < 2^25); each chroma
// row sums to zero, so a grey block gives 128 exactly.  A missing column or row of the last block is the edge pixel itself.
int gr_rgba8_to_yuv420(const unsigned char* rgba8, int width, int height, int layout, unsigned char* out) {
    if (!rgba8 || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgba8_to_yuv420: null argument");
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgba8_to_yuv420: the frame's size");
    if (layout != GR_YUV420_I420 && layout != GR_YUV420_NV12)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgba8_to_yuv420: layout (GR_YUV420_I420 or GR_YUV420_NV12)");
    const size_t w = (size_t)width, h = (size_t)height, cw = (w + 1) / 2, ch = (h + 1) / 2;
    for (size_t i = 0; i < w * h; i++) {
        const int32_t r = rgba8[4 * i], g = rgba8[4 * i + 1], b = rgba8[4 * i + 2];
        out[i] = (unsigned char)(16 + ((11966 * r + 40254 * g + 4064 * b + 32768) >> 16));
    }
    unsigned char* chroma = out + w * h;
    for (size_t cy = 0; cy < ch; cy++)
        for (size_t cx = 0; cx < cw; cx++) {
            int32_t sr = 0, sg = 0, sb = 0;
            for (size_t j = 0; j < 2; j++)
                for (size_t i = 0; i < 2; i++) {
                    const size_t x = std::min(2 * cx + i, w - 1), y = std::min(2 * cy + j, h - 1);
                    const unsigned char* px = rgba8 + 4 * (y * w + x);
                    sr += px[0]; sg += px[1]; sb += px[2];
                }
            const unsigned char cb = (unsigned char)(128 + ((-6596 * sr - 22188 * sg + 28784 * sb + 131072) >> 18));
            const unsigned char cr = (unsigned char)(128 + ((28784 * sr - 26145 * sg - 2639 * sb + 131072) >> 18));
            if (layout == GR_YUV420_NV12) {
                chroma[2 * (cy * cw + cx)] = cb;
                chroma[2 * (cy * cw + cx) + 1] = cr;
            } else {
                chroma[cy * cw + cx] = cb;
                chroma[cw * ch + cy * cw + cx] = cr;
            }
        }
    return GR_OK;
}

// ---- 10-bit video frames (include/geodesic_hip_internal.h, "10-bit video frames", says all of it) ------------------------------------

size_t gr_yuv420p10_bytes(int width, int height) { return 2 * gr_yuv420_bytes(width, height); }

// gr_srgb8_thresholds with code10 for srgb8: out[k] = the smallest float of [0, 1] whose code is >= k, +infinity above code10(1.0f)
int gr_srgb10_thresholds(float out[1024]) {
    if (!out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_srgb10_thresholds: null argument");
    auto of_bits = [](uint32_t bits) { float f; memcpy(&f, &bits, sizeof(f)); return f; };
    const uint32_t one = 0x3f800000u;
    const int top = code10(of_bits(one));
    out[0] = 0.f;
    for (int k = 1; k < 1024; k++) {
        if (k > top) { out[k] = INFINITY; continue; }
        uint32_t lo = 0, hi = one;   // code(lo) < k <= code(hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (code10(of_bits(mid)) >= k) hi = mid; else lo = mid;
        }
        out[k] = of_bits(hi);
    }
    return GR_OK;
}

// R, G, B of every pixel as 10-bit codes, [height][width][3]; alpha is not encoded
int gr_frame_to_rgb10(const float* frame_rgba_f32, int width, int height, unsigned short* out_rgb) {
    if (!frame_rgba_f32 || !out_rgb) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_frame_to_rgb10: null argument");
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_frame_to_rgb10: the frame's size");
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; i++)
        for (size_t c = 0; c < 3; c++) out_rgb[3 * i + c] = (unsigned short)code10(frame_rgba_f32[4 * i + c]);
    return GR_OK;
}

// BT.709, limited range, 10 bits: gr_rgba8_to_yuv420's arithmetic with the coefficients of 876 / 1023 and 896 / 1023 (the largest
// intermediate is 28700 * 4092 + 131072 < 2^27); each chroma row sums to zero, so a grey block gives 512 exactly.  GR_YUV420_I420 keeps a
// code in the low ten bits of its word (yuv420p10le), GR_YUV420_NV12 in the high ten (P010).
int gr_rgb10_to_yuv420p10(const unsigned short* rgb10, int width, int height, int layout, unsigned short* out) {
    if (!rgb10 || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgb10_to_yuv420p10: null argument");
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgb10_to_yuv420p10: the frame's size");
    if (layout != GR_YUV420_I420 && layout != GR_YUV420_NV12)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgb10_to_yuv420p10: layout (GR_YUV420_I420 or GR_YUV420_NV12)");
    const size_t w = (size_t)width, h = (size_t)height, cw = (w + 1) / 2, ch = (h + 1) / 2;
    for (size_t i = 0; i < 3 * w * h; i++)
        if (rgb10[i] > 1023) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_rgb10_to_yuv420p10: a code above 1023");
    const int shift = layout == GR_YUV420_NV12 ? 6 : 0;
    for (size_t i = 0; i < w * h; i++) {
        const int32_t r = rgb10[3 * i], g = rgb10[3 * i + 1], b = rgb10[3 * i + 2];
        out[i] = (unsigned short)((64 + ((11931 * r + 40136 * g + 4052 * b + 32768) >> 16)) << shift);
    }
    unsigned short* chroma = out + w * h;
    for (size_t cy = 0; cy < ch; cy++)
        for (size_t cx = 0; cx < cw; cx++) {
            int32_t sr = 0, sg = 0, sb = 0;
            for (size_t j = 0; j < 2; j++)
                for (size_t i = 0; i < 2; i++) {
                    const size_t x = std::min(2 * cx + i, w - 1), y = std::min(2 * cy + j, h - 1);
                    const unsigned short* px = rgb10 + 3 * (y * w + x);
                    sr += px[0]; sg += px[1]; sb += px[2];
                }
            const unsigned short cb = (unsigned short)((512 + ((-6576 * sr - 22124 * sg + 28700 * sb + 131072) >> 18)) << shift);
            const unsigned short cr = (unsigned short)((512 + ((28700 * sr - 26068 * sg - 2632 * sb + 131072) >> 18)) << shift);
            if (layout == GR_YUV420_NV12) {
                chroma[2 * (cy * cw + cx)] = cb;
                chroma[2 * (cy * cw + cx) + 1] = cr;
            } else {
                chroma[cy * cw + cx] = cb;
                chroma[cw * ch + cy * cw + cx] = cr;
            }
        }
    return GR_OK;
}

struct gr_y4m {
    FILE* file;          // NULL after a short write: the handle then only waits for gr_y4m_close
    size_t frame_bytes;
    std::string path;
};

// all of `bytes`, flushed; on a short write the file is closed and the handle keeps none
static int y4m_put(gr_y4m* y, const void* data, size_t bytes, const char* what) {
    if (fwrite(data, 1, bytes, y->file) == bytes && fflush(y->file) == 0) return GR_OK;
    fclose(y->file);
    y->file = nullptr;
    return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string("gr_y4m: short write of ") + what + " to " + y->path).c_str());
}

// gr_y4m_open and gr_y4m_open_depth: `who` names the caller in a refusal, `sample_bytes` is 1 (C420jpeg) or 2 (C420p10)
static int y4m_open(const char* who, const char* path, int width, int height, int fps_num, int fps_den, size_t sample_bytes, gr_y4m** out) {
    const std::string name = who;
    if (out) *out = nullptr;
    if (!path || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": null argument").c_str());
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": the frame's size").c_str());
    if (fps_num < 1 || fps_den < 1)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": the frame rate fps_num / fps_den needs both parts >= 1").c_str());
    FILE* f = fopen(path, "wb");
    if (!f) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": cannot write " + path).c_str());
    gr_y4m* y = new gr_y4m{f, sample_bytes * gr_yuv420_bytes(width, height), path};
    const std::string header = "YUV4MPEG2 W" + std::to_string(width) + " H" + std::to_string(height) + " F" + std::to_string(fps_num) + ":" +
                               std::to_string(fps_den) + " Ip A1:1 " + (sample_bytes == 2 ? "C420p10" : "C420jpeg") + " XCOLORRANGE=LIMITED\n";
    const int rc = y4m_put(y, header.data(), header.size(), "the header");
    if (rc != GR_OK) { delete y; return rc; }
    *out = y;
    return GR_OK;
}

int gr_y4m_open(const char* path, int width, int height, int fps_num, int fps_den, gr_y4m** out) {
    return y4m_open("gr_y4m_open", path, width, height, fps_num, fps_den, 1, out);
}

// bit_depth 10: the frames gr_y4m_write_frame takes are gr_yuv420p10_bytes long - GR_YUV420_I420 planes of 16-bit little-endian words, which
// is the order this library's hosts keep an unsigned short in
int gr_y4m_open_depth(const char* path, int width, int height, int fps_num, int fps_den, int bit_depth, gr_y4m** out) {
    if (bit_depth != 8 && bit_depth != 10) {
        if (out) *out = nullptr;
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_y4m_open_depth: bit_depth " + std::to_string(bit_depth) + " (8 or 10)").c_str());
    }
    return y4m_open("gr_y4m_open_depth", path, width, height, fps_num, fps_den, bit_depth == 10 ? 2 : 1, out);
}

int gr_y4m_write_frame(gr_y4m* y, const unsigned char* i420) {
    if (!y || !i420) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_y4m_write_frame: null argument");
    if (!y->file) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_y4m_write_frame: " + y->path + " was closed by a failed write").c_str());
    if (fwrite("FRAME\n", 1, 6, y->file) != 6) {
        fclose(y->file);
        y->file = nullptr;
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_y4m: short write of a frame to " + y->path).c_str());
    }
    return y4m_put(y, i420, y->frame_bytes, "a frame");
}

int gr_y4m_close(gr_y4m* y) {
    if (!y) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_y4m_close: null argument");
    const bool complete = y->file && fclose(y->file) == 0;
    const std::string path = y->path;
    delete y;
    return complete ? GR_OK : gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_y4m_close: " + path + " is incomplete (a write failed)").c_str());
}

// ---- Motion-JPEG in AVI 1.0 (geodesic_hip_internal.h, "JPEG frames"): RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh', 'strf' } },
// LIST 'movi' { '00dc' a frame, padded to even length }, 'idx1' }.  The 224 bytes in front of the first frame are written at open with
// counts of 0 and written again at close with the counts the file ended up with.
struct gr_avi {
    FILE* file;          // NULL after a short write: the handle then only waits for gr_avi_close
    std::string path;
    uint32_t width, height, rate, scale;
    uint64_t bytes;      // of the file so far
    uint64_t limit;      // of the finished file: 2^31 - 1 (AVI 1.0 players read sizes and offsets as signed 32-bit numbers)
    uint32_t largest;    // frame so far
    std::vector<std::pair<uint32_t, uint32_t>> frames;   // offset of the '00dc' chunk from the 'movi' tag, size of its data
};

enum { AVI_HEADER_BYTES = 224, AVI_MOVI_TAG_AT = 220 };

static void avi_header(const gr_avi* a, uint8_t out[AVI_HEADER_BYTES], uint64_t file_bytes, uint64_t movi_bytes) {
    uint8_t* at = out;
    auto tag = [&](const char* t) { memcpy(at, t, 4); at += 4; };
    auto u32 = [&](uint64_t v) { for (int b = 0; b < 4; b++) *at++ = (uint8_t)(v >> (8 * b)); };
    auto u16 = [&](unsigned v) { *at++ = (uint8_t)v; *at++ = (uint8_t)(v >> 8); };
    const uint32_t count = (uint32_t)a->frames.size();
    tag("RIFF"); u32(file_bytes - 8); tag("AVI ");
    tag("LIST"); u32(4 + 64 + 12 + 64 + 48); tag("hdrl");
    tag("avih"); u32(56);
    u32((1000000ull * a->scale + a->rate / 2) / a->rate);            // microseconds a frame
    u32(((uint64_t)a->largest * a->rate + a->scale - 1) / a->scale); // at most, bytes a second
    u32(0); u32(0x10);                                                // no padding granularity; AVIF_HASINDEX
    u32(count); u32(0); u32(1); u32(a->largest);                      // frames, no initial frames, one stream, the largest chunk
    u32(a->width); u32(a->height); u32(0); u32(0); u32(0); u32(0);
    tag("LIST"); u32(4 + 64 + 48); tag("strl");
    tag("strh"); u32(56);
    tag("vids"); tag("MJPG"); u32(0); u16(0); u16(0); u32(0);
    u32(a->scale); u32(a->rate); u32(0); u32(count);                  // rate / scale frames a second, `count` of them from 0
    u32(a->largest); u32(0xffffffffu); u32(0);                        // buffer, default quality, samples of varying size
    u16(0); u16(0); u16(a->width); u16(a->height);
    tag("strf"); u32(40);
    u32(40); u32(a->width); u32(a->height); u16(1); u16(24); tag("MJPG"); u32((uint64_t)a->width * a->height * 3); u32(0); u32(0); u32(0); u32(0);
    tag("LIST"); u32(4 + movi_bytes); tag("movi");
}

static int avi_put(gr_avi* a, const void* data, size_t bytes, const char* what) {
    if (fwrite(data, 1, bytes, a->file) == bytes && fflush(a->file) == 0) return GR_OK;
    fclose(a->file);
    a->file = nullptr;
    return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string("gr_avi: short write of ") + what + " to " + a->path).c_str());
}

int gr_avi_open(const char* path, int width, int height, int fps_num, int fps_den, gr_avi** out) {
    const std::string name = "gr_avi_open";
    if (out) *out = nullptr;
    if (!path || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": null argument").c_str());
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": the frame's size (1 to 65535)").c_str());
    if (fps_num < 1 || fps_den < 1)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": the frame rate fps_num / fps_den needs both parts >= 1").c_str());
    FILE* f = fopen(path, "wb");
    if (!f) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (name + ": cannot write " + path).c_str());
    gr_avi* a = new gr_avi{f, path, (uint32_t)width, (uint32_t)height, (uint32_t)fps_num, (uint32_t)fps_den, AVI_HEADER_BYTES, 0x7fffffffull, 0, {}};
    uint8_t header[AVI_HEADER_BYTES];
    avi_header(a, header, AVI_HEADER_BYTES + 8, 0);
    const int rc = avi_put(a, header, sizeof(header), "the header");
    if (rc != GR_OK) { delete a; return rc; }
    *out = a;
    return GR_OK;
}

int gr_avi_set_size_limit(gr_avi* a, unsigned long long bytes) {
    if (!a || bytes > 0x7fffffffull) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_avi_set_size_limit: a null handle, or a limit above 2^31 - 1");
    a->limit = bytes;
    return GR_OK;
}

int gr_avi_write_frame(gr_avi* a, const unsigned char* jpeg, size_t bytes) {
    if (!a || !jpeg || !bytes) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_avi_write_frame: null argument or an empty frame");
    if (!a->file) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_avi_write_frame: " + a->path + " was closed by a failed write").c_str());
    // the file as it would end up: what is there, this chunk with its padding, and an index of one entry more
    const uint64_t chunk = 8 + (uint64_t)bytes + (bytes & 1), after = a->bytes + chunk + 8 + 16 * ((uint64_t)a->frames.size() + 1);
    if (after > a->limit)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_avi_write_frame: frame " + std::to_string(a->frames.size()) + " of " + std::to_string(bytes) +
                                                            " bytes would take " + a->path + " to " + std::to_string(after) + " bytes, past the " +
                                                            std::to_string(a->limit) + " an AVI 1.0 file holds; close it and start another").c_str());
    uint8_t head[8] = {'0', '0', 'd', 'c'};
    for (int b = 0; b < 4; b++) head[4 + b] = (uint8_t)(bytes >> (8 * b));
    if (fwrite(head, 1, 8, a->file) != 8 || fwrite(jpeg, 1, bytes, a->file) != bytes) {
        fclose(a->file);
        a->file = nullptr;
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_avi: short write of a frame to " + a->path).c_str());
    }
    const uint8_t pad = 0;
    const int rc = avi_put(a, &pad, bytes & 1, "a frame");
    if (rc != GR_OK) return rc;
    a->frames.push_back({(uint32_t)(a->bytes - AVI_MOVI_TAG_AT), (uint32_t)bytes});
    a->largest = std::max(a->largest, (uint32_t)bytes);
    a->bytes += chunk;
    return GR_OK;
}

int gr_avi_close(gr_avi* a) {
    if (!a) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_avi_close: null argument");
    bool complete = a->file != nullptr;
    if (complete) {
        std::vector<uint8_t> index(8 + 16 * a->frames.size());
        uint8_t* at = index.data();
        auto u32 = [&](uint32_t v) { for (int b = 0; b < 4; b++) *at++ = (uint8_t)(v >> (8 * b)); };
        memcpy(at, "idx1", 4);
        at += 4;
        u32((uint32_t)(16 * a->frames.size()));
        for (auto& frame : a->frames) {
            memcpy(at, "00dc", 4);
            at += 4;
            u32(0x10);   // AVIIF_KEYFRAME
            u32(frame.first);
            u32(frame.second);
        }
        uint8_t header[AVI_HEADER_BYTES];
        avi_header(a, header, a->bytes + index.size(), a->bytes - AVI_HEADER_BYTES);
        complete = fwrite(index.data(), 1, index.size(), a->file) == index.size() && fseek(a->file, 0, SEEK_SET) == 0 &&
                   fwrite(header, 1, sizeof(header), a->file) == sizeof(header);
        complete = (fclose(a->file) == 0) && complete;
    }
    const std::string path = a->path;
    delete a;
    return complete ? GR_OK : gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_avi_close: " + path + " is incomplete (a write failed)").c_str());
}

// ---- the shutter of a motion-blurred frame: the host statement of one accumulation step (geodesic_hip_internal.h, "Motion-blurred frames";
// kernels/shutter.hip's gr_shutter_accumulate is held to it at factor 1).  accum = [accum +] weight * frame, one fp32 multiply and one fp32
// add per value, EACH ROUNDED: a fused multiply-add rounds once and gives other bits.  How the compiler is kept from contracting them: the
// function is compiled with fp-contract=off whatever the command line says (the attribute below for GCC, which this library is built
// with; the pragma for a clang build), and the product is a float object of its own.  The library's x86-64 baseline build has no fma
// instruction to contract to either, but -march=native would: tests/test_shutter_abi.py holds it to a triple where the two roundings differ.
#if defined(__clang__)
#define GR_NO_CONTRACTION
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#define GR_NO_CONTRACTION __attribute__((optimize("fp-contract=off")))
#else
#define GR_NO_CONTRACTION
#endif
GR_NO_CONTRACTION int gr_accumulate_frame(float* accum, const float* frame, size_t count_floats, float weight, int first) {
    if (!accum || !frame) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_accumulate_frame: null argument");
    if (!std::isfinite(weight)) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_accumulate_frame: a weight that is not finite");
    if (first) {
        // (not 0 + weight * frame[i]: a weight of 1 hands every value through as it is, the sign of a zero included)
        for (size_t i = 0; i < count_floats; i++) accum[i] = weight * frame[i];
    } else {
        for (size_t i = 0; i < count_floats; i++) {
            const float product = weight * frame[i];
            accum[i] = accum[i] + product;
        }
    }
    return GR_OK;
}

// ---- separable reconstruction filters of a supersampled frame: the host statement (geodesic_hip_internal.h, "Filtered frames";
// kernels/filter.hip's gr_resolve_filtered is held to gr_filter_frame bit for bit).
// The taps of the named filters: k(d) in double from |d|, normalised by their sum in double (ascending t), each rounded to fp32 once; not
// renormalised after rounding.
int gr_filter_taps(int filter, int factor, float taps[GR_FILTER_MAX_TAPS], int* count) {
    if (!taps || !count) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_filter_taps: null argument");
    if (factor < 1 || factor > 4) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_filter_taps: factor " + std::to_string(factor) + " (1 to 4)").c_str());
    if (filter == GR_FILTER_BOX)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_filter_taps: GR_FILTER_BOX has no table: the box average of a pixel's own samples is "
                                                           "gr_resolve_supersampled");
    if (filter != GR_FILTER_TENT && filter != GR_FILTER_GAUSSIAN && filter != GR_FILTER_MITCHELL)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_filter_taps: unknown filter " + std::to_string(filter) +
                                                            " (GR_FILTER_TENT, GR_FILTER_GAUSSIAN or GR_FILTER_MITCHELL)").c_str());
    const int radius = filter == GR_FILTER_TENT ? 1 : 2;
    const int n = 2 * radius * factor - (factor % 2);   // the taps with |d_t| < radius
    double k[GR_FILTER_MAX_TAPS], sum = 0.0;
    for (int t = 0; t < n; t++) {
        const double d = std::fabs((t + 0.5 - n / 2.0) / factor);
        if (filter == GR_FILTER_TENT) {
            k[t] = 1.0 - d;
        } else if (filter == GR_FILTER_GAUSSIAN) {
            k[t] = std::exp(-2.0 * d * d) - std::exp(-8.0);
        } else {
            const double B = 1.0 / 3.0, C = 1.0 / 3.0;
            k[t] = d < 1.0 ? ((12.0 - 9.0 * B - 6.0 * C) * d * d * d + (-18.0 + 12.0 * B + 6.0 * C) * d * d + (6.0 - 2.0 * B)) / 6.0
                           : ((-B - 6.0 * C) * d * d * d + (6.0 * B + 30.0 * C) * d * d + (-12.0 * B - 48.0 * C) * d + (8.0 * B + 24.0 * C)) / 6.0;
        }
        sum += k[t];
    }
    for (int t = 0; t < n; t++) taps[t] = (float)(k[t] / sum);
    *count = n;
    return GR_OK;
}

// what gr_filter_frame and the launcher gr_resolve_filtered (frame_launch.cpp) both refuse about a table; NULL: nothing wrong
extern "C" const char* gr_internal_filter_table_error(int factor, const float* taps, int count) {
    if (factor < 1 || factor > 4) return "a factor outside 1 to 4";
    if (count < 1 || count > GR_FILTER_MAX_TAPS) return "a count of taps outside 1 to 16";
    if ((count - factor) % 2) return "a count of taps of the wrong parity (count = factor mod 2: the table is centred on the pixel)";
    for (int t = 0; t < count; t++)
        if (!std::isfinite(taps[t])) return "a tap that is not finite";
    return nullptr;
}

// The rows pass into an intermediate of width x (height * factor) float4, rounded to fp32, then the columns pass; every product a float
// object of its own and the function compiled without contraction, as gr_accumulate_frame is.
GR_NO_CONTRACTION int gr_filter_frame(const float* src, int width, int height, int factor, const float* taps, int count, float* dst) {
    const std::string who = "gr_filter_frame: ";
    if (!src || !taps || !dst) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "a size below 1").c_str());
    if (const char* wrong = gr_internal_filter_table_error(factor, taps, count)) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + wrong).c_str());
    if (src == dst) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "src and dst are one buffer").c_str());
    const long long sw = (long long)width * factor, sh = (long long)height * factor;
    const long long first = (factor - count) / 2;   // (even: exact)
    std::vector<float> rows;
    try {
        rows.resize((size_t)sh * (size_t)width * 4);
    } catch (const std::exception&) {
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "no memory for the intermediate frame").c_str());
    }
    for (long long y = 0; y < sh; y++) {
        for (long long X = 0; X < width; X++) {
            float* h = &rows[((size_t)y * width + X) * 4];
            for (int t = 0; t < count; t++) {
                const long long cx = std::min(std::max(X * factor + first + t, 0ll), sw - 1);
                const float* s = src + ((size_t)y * sw + cx) * 4;
                for (int c = 0; c < 4; c++) {
                    const float product = taps[t] * s[c];
                    h[c] = t ? h[c] + product : product;
                }
            }
        }
    }
    for (long long Y = 0; Y < height; Y++) {
        for (long long X = 0; X < width; X++) {
            float* o = dst + ((size_t)Y * width + X) * 4;
            for (int t = 0; t < count; t++) {
                const long long cy = std::min(std::max(Y * factor + first + t, 0ll), sh - 1);
                const float* h = &rows[((size_t)cy * width + X) * 4];
                for (int c = 0; c < 4; c++) {
                    const float product = taps[t] * h[c];
                    o[c] = t ? o[c] + product : product;
                }
            }
        }
    }
    return GR_OK;
}

// ---- glare: a PSF and an exposure on the resolved frame - the host statement (geodesic_hip_internal.h, "Glare"; kernels/glare.hip's launches
// behind gr_apply_glare are held to gr_glare_frame bit for bit).
// what gr_glare_frame, gr_apply_glare (frame_launch.cpp) and gr_render_state_set_glare (frame.cpp) refuse about a glare, under the caller's name and by the field's
int gr_internal_check_glare(const char* who, const gr_glare* g) {
    std::string wrong;
    if (!std::isfinite(g->core)) wrong = "core is not finite";
    else if (g->components < 0 || g->components > GR_GLARE_MAX_COMPONENTS) wrong = "components " + std::to_string(g->components) + " (0 to 4)";
    for (int k = 0; wrong.empty() && k < g->components; k++) {
        const std::string at = "[" + std::to_string(k) + "]";
        if (!std::isfinite(g->weight[k])) wrong = "weight" + at + " is not finite";
        else if (g->taps[k] < 1 || g->taps[k] > GR_GLARE_MAX_TAPS || g->taps[k] % 2 == 0) wrong = "taps" + at + " = " + std::to_string(g->taps[k]) + " (odd, 1 to 129)";
        for (int t = 0; wrong.empty() && t < g->taps[k]; t++)
            if (!std::isfinite(g->tap[k][t])) wrong = "tap" + at + "[" + std::to_string(t) + "] is not finite";
    }
    return wrong.empty() ? GR_OK : gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string(who) + ": " + wrong).c_str());
}

int gr_glare_gaussians(const float* sigma, const float* weight, int count, gr_glare* out) {
    const std::string who = "gr_glare_gaussians: ";
    if (!sigma || !weight || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    if (count < 0 || count > GR_GLARE_MAX_COMPONENTS) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "count " + std::to_string(count) + " (0 to 4)").c_str());
    double total = 0.0;
    for (int k = 0; k < count; k++) {
        const std::string at = "[" + std::to_string(k) + "]";
        if (!std::isfinite(sigma[k]) || !(sigma[k] > 0.f) || sigma[k] > 64.f)
            return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "sigma" + at + " is not in (0, 64]").c_str());
        if (!std::isfinite(weight[k]) || weight[k] < 0.f || weight[k] > 1.f)
            return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "weight" + at + " is not in [0, 1]").c_str());
        total += (double)weight[k];
    }
    if (total > 1.0) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "the weights sum to more than 1").c_str());
    gr_glare made;
    std::memset(&made, 0, sizeof made);
    made.core = (float)(1.0 - total);
    made.components = count;
    for (int k = 0; k < count; k++) {
        const double s = (double)sigma[k];
        const int radius = std::min((int)std::ceil(3.0 * s), (GR_GLARE_MAX_TAPS - 1) / 2);
        const int n = 2 * radius + 1;
        double value[GR_GLARE_MAX_TAPS], sum = 0.0;
        for (int t = 0; t < n; t++) {
            const double d = (double)(t - radius);
            value[t] = std::exp(-d * d / (2.0 * s * s));
            sum += value[t];
        }
        for (int t = 0; t < n; t++) made.tap[k][t] = (float)(value[t] / sum);
        made.taps[k] = n;
        made.weight[k] = weight[k];
    }
    *out = made;
    return GR_OK;
}

GR_NO_CONTRACTION int gr_glare_exposure(gr_glare* g, float stops) {
    if (!g) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_glare_exposure: null argument");
    if (!std::isfinite(stops) || stops < -32.f || stops > 32.f)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_glare_exposure: stops is not in -32 to 32");
    const float gain = (float)std::exp2((double)stops);
    g->core = g->core * gain;
    for (int k = 0; k < GR_GLARE_MAX_COMPONENTS; k++) g->weight[k] = g->weight[k] * gain;
    return GR_OK;
}

// Per component: the rows pass into an intermediate of width x height x 3 floats, rounded to fp32, the columns pass, then the component's
// step of the combine into dst; every product a float object of its own and the function compiled without contraction, as gr_filter_frame is.
GR_NO_CONTRACTION int gr_glare_frame(const float* src, int width, int height, const gr_glare* g, float* dst) {
    const std::string who = "gr_glare_frame: ";
    if (!src || !g || !dst) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "a size below 1").c_str());
    if (src == dst) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "src and dst are one buffer").c_str());
    GR_CHECK(gr_internal_check_glare("gr_glare_frame", g));
    const long long w = width, h = height;
    const size_t pixels = (size_t)w * (size_t)h;
    std::vector<float> rows;
    try {
        if (g->components) rows.resize(pixels * 3);
    } catch (const std::exception&) {
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "no memory for the intermediate frame").c_str());
    }
    for (size_t i = 0; i < pixels; i++) {
        for (int c = 0; c < 3; c++) dst[4 * i + c] = g->core * src[4 * i + c];
        dst[4 * i + 3] = src[4 * i + 3];
    }
    for (int k = 0; k < g->components; k++) {
        const int n = g->taps[k];
        const long long radius = (n - 1) / 2;
        const float* tap = g->tap[k];
        for (long long y = 0; y < h; y++)
            for (long long X = 0; X < w; X++) {
                float* o = &rows[((size_t)y * w + X) * 3];
                for (int t = 0; t < n; t++) {
                    const long long cx = std::min(std::max(X - radius + t, 0ll), w - 1);
                    const float* s = src + ((size_t)y * w + cx) * 4;
                    for (int c = 0; c < 3; c++) {
                        const float product = tap[t] * s[c];
                        o[c] = t ? o[c] + product : product;
                    }
                }
            }
        for (long long Y = 0; Y < h; Y++)
            for (long long X = 0; X < w; X++) {
                float column[3];
                for (int t = 0; t < n; t++) {
                    const long long cy = std::min(std::max(Y - radius + t, 0ll), h - 1);
                    const float* r = &rows[((size_t)cy * w + X) * 3];
                    for (int c = 0; c < 3; c++) {
                        const float product = tap[t] * r[c];
                        column[c] = t ? column[c] + product : product;
                    }
                }
                float* o = dst + ((size_t)Y * w + X) * 4;
                for (int c = 0; c < 3; c++) {
                    const float product = g->weight[k] * column[c];
                    o[c] = o[c] + product;
                }
            }
    }
    return GR_OK;
}

// ---- metering and tone curve - the host statements (geodesic_hip_internal.h, "Metering and tone curve"; kernels/tone.hip's launches behind
// gr_meter_frame, gr_meter_solve_device and gr_apply_tone are held to these exactly).
// what every taker of a tone refuses about its fields, under the caller's name and by the field's; all fields in both modes
int gr_internal_check_tone(const char* who, const gr_tone* t) {
    std::string wrong;
    const auto stops = [](float v) { return std::isfinite(v) && v >= -32.f && v <= 32.f; };
    if (t->mode != GR_TONE_MANUAL && t->mode != GR_TONE_AUTO) wrong = "mode " + std::to_string(t->mode) + " (GR_TONE_MANUAL, GR_TONE_AUTO)";
    else if (!stops(t->stops)) wrong = "stops is not in -32 to 32";
    else if (!stops(t->key_stops)) wrong = "key_stops is not in -32 to 32";
    else if (!std::isfinite(t->low) || t->low < 0.f || t->low > 1.f) wrong = "low is not in [0, 1]";
    else if (!std::isfinite(t->high) || t->high < 0.f || t->high > 1.f) wrong = "high is not in [0, 1]";
    else if (!(t->low < t->high)) wrong = "low >= high";
    else if (!stops(t->min_stops)) wrong = "min_stops is not in -32 to 32";
    else if (!stops(t->max_stops)) wrong = "max_stops is not in -32 to 32";
    else if (t->min_stops > t->max_stops) wrong = "min_stops > max_stops";
    else if (!std::isfinite(t->rate) || !(t->rate > 0.f) || t->rate > 1.f) wrong = "rate is not in (0, 1]";
    else if (t->curve != GR_TONE_LINEAR && t->curve != GR_TONE_REINHARD && t->curve != GR_TONE_FILMIC) wrong = "curve " + std::to_string(t->curve) + " (GR_TONE_LINEAR, _REINHARD, _FILMIC)";
    else if (!std::isfinite(t->white) || !(t->white > 0.f) || t->white > 4096.f) wrong = "white is not in (0, 4096]";
    return wrong.empty() ? GR_OK : gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string(who) + ": " + wrong).c_str());
}

int gr_tone_default(gr_tone* out) {
    if (!out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_tone_default: null argument");
    gr_tone made;
    std::memset(&made, 0, sizeof made);
    made.mode = GR_TONE_MANUAL;
    made.stops = 0.f;
    made.key_stops = -0x1.3ca9c6p+1f;   // (float)log2(0.18)
    made.low = 0.5f;
    made.high = 0.98f;
    made.min_stops = -32.f;
    made.max_stops = 32.f;
    made.rate = 1.f;
    made.curve = GR_TONE_LINEAR;
    made.white = 4.f;
    *out = made;
    return GR_OK;
}

GR_NO_CONTRACTION int gr_meter_histogram_frame(const float* src, int width, int height, unsigned* hist) {
    const std::string who = "gr_meter_histogram_frame: ";
    if (!src || !hist) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "a size below 1").c_str());
    if ((long long)width * height > 0x7fffffffll) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "more than 2^31 - 1 pixels").c_str());
    std::memset(hist, 0, GR_METER_COUNTERS * sizeof(unsigned));
    const size_t pixels = (size_t)width * (size_t)height;
    for (size_t i = 0; i < pixels; i++) {
        const float yr = 0.2126f * src[4 * i], yg = 0.7152f * src[4 * i + 1], yb = 0.0722f * src[4 * i + 2];
        const float yrg = yr + yg;
        const float y = yrg + yb;
        if (!(y > 0.f)) {
            hist[GR_METER_BINS]++;
            continue;
        }
        uint32_t bits;
        std::memcpy(&bits, &y, sizeof bits);
        const int e = (int)(bits >> 20) - 824;
        hist[std::min(std::max(e, 0), GR_METER_BINS - 1)]++;
    }
    return GR_OK;
}

namespace {
const float TONE_SIXTEENTHS[16] = GR_TONE_SIXTEENTHS;
inline double tone_lesser(double a, double b) { return a < b ? a : b; }
inline double tone_greater(double a, double b) { return a > b ? a : b; }
}   // namespace

// the gain of `adapted` stops (-32 ... 32), in sixteenths of a stop from the table
GR_NO_CONTRACTION void gr_internal_tone_gain(double adapted, float* gain, int* q_out) {
    const double sixteenths = adapted * 16.0;
    const int q = (int)std::nearbyint(sixteenths);   // (the rounding mode is the default: to nearest, ties to even)
    const int index = ((q % 16) + 16) % 16;
    const int whole = (q - index) / 16;
    *q_out = q;
    *gain = std::ldexp(TONE_SIXTEENTHS[index], whole);
}

// kernels/tone.hip's gr_meter_solve repeats this operation for operation
GR_NO_CONTRACTION int gr_meter_solve_host(const unsigned* hist, const gr_tone* tone, double* adapted_io, int* primed_io, float* gain, int* q_out) {
    const std::string who = "gr_meter_solve_host: ";
    if (!hist || !tone || !adapted_io || !primed_io || !gain || !q_out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    GR_CHECK(gr_internal_check_tone("gr_meter_solve_host", tone));
    double adapted;
    if (tone->mode == GR_TONE_MANUAL) {
        adapted = (double)tone->stops;
    } else {
        if (!std::isfinite(*adapted_io) || *adapted_io < -32.0 || *adapted_io > 32.0)
            return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "adapted is not in -32 to 32").c_str());
        adapted = *adapted_io;
        int primed = *primed_io != 0;
        unsigned long long total = 0;
        for (int b = 0; b < GR_METER_BINS; b++) total += hist[b];
        if (total != 0) {
            const double n = (double)total;
            const double lo = (double)tone->low * n, hi = (double)tone->high * n;
            double sum_w = 0.0, sum_m = 0.0;
            unsigned long long below = 0;
            for (int b = 0; b < GR_METER_BINS; b++) {
                const double c = (double)below;
                below += hist[b];
                const double upper = tone_lesser((double)below, hi), lower = tone_greater(c, lo);
                const double w = tone_greater(0.0, upper - lower);
                const double centre = (double)b + 0.5;
                const double m = w * centre;
                sum_w = sum_w + w;
                sum_m = sum_m + m;
            }
            const double mean = sum_m / sum_w;
            const double octaves = mean / 8.0;
            const double level = octaves - 24.0;
            const double wanted = (double)tone->key_stops - level;
            const double target = tone_lesser(tone_greater(wanted, (double)tone->min_stops), (double)tone->max_stops);
            if (!primed) {
                adapted = target;
                primed = 1;
            } else {
                const double step = target - adapted;
                const double move = (double)tone->rate * step;
                adapted = adapted + move;
            }
        } else if (!primed) {
            adapted = 0.0;
        }
        *adapted_io = adapted;
        *primed_io = primed;
    }
    gr_internal_tone_gain(adapted, gain, q_out);
    return GR_OK;
}

namespace {
GR_NO_CONTRACTION inline float tone_curve(float c, float gain, int curve, float iw2) {
    const float v = gain * c;
    const float x = v > 0.f ? (v < 16777216.f ? v : 16777216.f) : 0.f;
    if (curve == GR_TONE_REINHARD) {
        const float a = x * iw2;
        const float one_a = 1.f + a;
        const float n = x * one_a;
        const float d = 1.f + x;
        return n / d;
    }
    if (curve == GR_TONE_FILMIC) {
        const float n1 = 2.51f * x;
        const float n2 = n1 + 0.03f;
        const float n = x * n2;
        const float d1 = 2.43f * x;
        const float d2 = d1 + 0.59f;
        const float d3 = x * d2;
        const float d = d3 + 0.14f;
        const float y = n / d;
        return y < 1.f ? y : 1.f;
    }
    return x;
}
}   // namespace

float gr_internal_tone_inverse_white_squared(const gr_tone* t) { return (float)(1.0 / ((double)t->white * (double)t->white)); }

GR_NO_CONTRACTION int gr_tone_frame(const float* src, int width, int height, const gr_tone* tone, float gain, float* dst) {
    const std::string who = "gr_tone_frame: ";
    if (!src || !tone || !dst) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "null argument").c_str());
    if (width < 1 || height < 1) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "a size below 1").c_str());
    if ((long long)width * height > 0x7fffffffll) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "more than 2^31 - 1 pixels").c_str());
    GR_CHECK(gr_internal_check_tone("gr_tone_frame", tone));
    if (!std::isfinite(gain) || gain < 0.f) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (who + "gain is not finite or is negative").c_str());
    const float iw2 = gr_internal_tone_inverse_white_squared(tone);
    const size_t pixels = (size_t)width * (size_t)height;
    for (size_t i = 0; i < pixels; i++) {
        const float r = tone_curve(src[4 * i], gain, tone->curve, iw2), g = tone_curve(src[4 * i + 1], gain, tone->curve, iw2),
                    b = tone_curve(src[4 * i + 2], gain, tone->curve, iw2);
        uint32_t alpha;
        std::memcpy(&alpha, &src[4 * i + 3], sizeof alpha);   // (as an integer: a NaN's payload passes whatever the machine does to float moves)
        dst[4 * i] = r;
        dst[4 * i + 1] = g;
        dst[4 * i + 2] = b;
        std::memcpy(&dst[4 * i + 3], &alpha, sizeof alpha);
    }
    return GR_OK;
}

}  // extern "C"
