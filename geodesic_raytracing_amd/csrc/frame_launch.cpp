// frame_launch.cpp — the launchers of the stages between a traced frame and its sink: the box resolve and the three encodes that hold
// one, the shutter's accumulation, the separable filters, the glare, the meter, its solve and the tone curve.  Which of them a delivery
// calls, in what order and on which buffers, is decided in delivery_plan.cpp (no HIP, host-tested) and carried out in frame.cpp; here
// are each launcher's refusals - all before its first device call - its grid and its argument array in the kernel's order.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "frame_format.hpp"
#include "internal.hpp"
#include "trace_plan.hpp"

using gr_internal::blocks, gr_internal::launch, gr_internal::refuse;

namespace {

bool overlaps(const void* a, size_t na, const void* b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }
// more source pixels than a 31-bit index counts
bool too_many_pixels(int width, int height, int factor) { return (long long)width * factor * height * factor > 0x7fffffffll; }
// a one-dimensional grid whose workgroups walk `tiles` tiles with the grid's stride: a workgroup a tile, at most `cap`
unsigned strided_grid(unsigned long long tiles, unsigned long long cap) { return (unsigned)std::min(tiles, cap); }

// What the glare, the meter, the solve and the tone refuse first and alike: a NULL among their pointers (`missing`), a NULL program ...
int refuse_nulls(const char* who, bool missing, const gr_program* p) {
    if (missing) return refuse(who, "null argument");
    return p ? GR_OK : refuse(who, "null program");
}
// ... and then, those with a frame: a size below 1, more pixels than 2^31 - 1
int refuse_size(const char* who, int width, int height) {
    if (width < 1 || height < 1) return refuse(who, "a size below 1");
    return too_many_pixels(width, height, 1) ? refuse(who, "more than 2^31 - 1 pixels") : GR_OK;
}

// What the resolve, present and accumulate launchers below refuse alike, before any device call: a NULL buffer; a NULL program where the
// launcher answers for it under its own name (launch() refuses it for the others); a factor outside 1 ... 4; a size below 1 or with more
// than 2^31 - 1 source pixels; then grid_rows workgroup rows that the grid does not hold (0: no such check; a caller's blocks() of a bad size is 0 too).
int refuse_frame_launch(const char* who, const gr_program* p, bool needs_program, const void* src, const void* dst, int width, int height,
                        int factor, unsigned grid_rows) {
    GR_NEED(who, src, dst);
    if (needs_program && !p) return refuse(who, "null program");
    if (factor < 1 || factor > 4) return refuse(who, "factor " + std::to_string(factor) + " (1 to 4)");
    if (width <= 0 || height <= 0 || too_many_pixels(width, height, factor)) return refuse(who, "the frame's size");
    if (grid_rows > 65535u) return refuse(who, "a frame of " + std::to_string(height) + " rows does not fit the grid");
    return GR_OK;
}

// one work item per output pixel of this device's rows, a wave on 64 consecutive pixels of one row, four rows to a workgroup: the grid
// and the row dealing of kernels/resolve.hip and of gr_present_rgba8
int launch_dealt_rows(int k, const char* who, gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor,
                      int block_rows, int strip_rank, int strip_count, int compact_out) {
    GR_CHECK(refuse_frame_launch(who, p, false, src, dst, width, height, factor, 0));
    const trace_plan::strip_share share = trace_plan::strips(height, block_rows, strip_rank, strip_count, trace_plan::THE_HEIGHT);
    if (share.bad) return refuse(who, "bad strip parameters");
    block_rows = share.block_rows; strip_rank = share.strip_rank; strip_count = share.strip_count;
    int local_rows = gr_strip_local_blocks(height, block_rows, strip_rank, strip_count) * block_rows;
    void* args[] = {&src, &dst, &width, &height, &factor, &block_rows, &strip_rank, &strip_count, &compact_out, &local_rows};
    return launch(p, k, stream, blocks(width, 64), blocks(local_rows, 4), 64, 4, args);
}

// gr_present_rgba8's resolve and encode, then BT.709 Y'CbCr 4:2:0 (kernels/present.hip: gr_present_yuv420, and gr_present_yuv420p10 with ten
// bits a sample in 16-bit words): a lane per 2 rows x 4 columns, a workgroup of 64 x 4 lanes on 256 columns x 8 rows.  Whole frames only.
// The two differ in the kernel and in dst's alignment, which is the format's (frame_format.cpp).
int launch_video(int k, const char* who, int format, gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor,
                 int layout) {
    const unsigned gx = blocks(((long long)width + 3) / 4, 64), gy = blocks(((long long)height + 1) / 2, 4);
    GR_CHECK(refuse_frame_launch(who, p, true, src, dst, width, height, factor, gy));
    const std::string wrong = frame_format::refusal(format, false, layout, (uintptr_t)dst, &width, 1);
    if (!wrong.empty()) return refuse(who, wrong);
    void* args[] = {&src, &dst, &width, &height, &factor, &layout};
    return launch(p, k, stream, gx, gy, 64, 4, args);
}

}   // namespace

extern "C" {

// the box filter of a supersampled frame (kernels/resolve.hip)
int gr_resolve_supersampled(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int block_rows,
                            int strip_rank, int strip_count, int compact_out) {
    return launch_dealt_rows(K_RESOLVE_SUPERSAMPLED, "gr_resolve_supersampled", p, stream, src, dst, width, height, factor, block_rows, strip_rank,
                             strip_count, compact_out);
}

// gr_resolve_supersampled fused with the 8-bit sRGB encode (kernels/present.hip): the same grid, the same row dealing, one uint32 a pixel
int gr_present_rgba8(gr_program* p, void* stream, const void* src, void* dst_rgba8, int width, int height, int factor, int block_rows,
                     int strip_rank, int strip_count, int compact_out) {
    return launch_dealt_rows(K_PRESENT_RGBA8, "gr_present_rgba8", p, stream, src, dst_rgba8, width, height, factor, block_rows, strip_rank, strip_count,
                             compact_out);
}

int gr_present_yuv420(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int layout) {
    return launch_video(K_PRESENT_YUV420, "gr_present_yuv420", GR_FRAME_YUV420, p, stream, src, dst, width, height, factor, layout);
}
int gr_present_yuv420p10(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, int layout) {
    return launch_video(K_PRESENT_YUV420P10, "gr_present_yuv420p10", GR_FRAME_YUV420P10, p, stream, src, dst, width, height, factor, layout);
}

// one sub-frame of a shutter into the accumulation frame (kernels/shutter.hip): gr_resolve_supersampled's grid over the whole frame; with
// `first` the accumulation frame is written without being read
int gr_shutter_accumulate(gr_program* p, void* stream, const void* src, void* accum, int width, int height, int factor, float weight, int first) {
    const char* who = "gr_shutter_accumulate";
    const unsigned gy = blocks(height, 4);
    GR_CHECK(refuse_frame_launch(who, p, true, src, accum, width, height, factor, gy));
    if (src == accum) return refuse(who, "the sub-frame and the accumulation frame are one buffer");
    if (!std::isfinite(weight)) return refuse(who, "a weight that is not finite");
    first = first ? 1 : 0;
    void* args[] = {&src, &accum, &width, &height, &factor, &weight, &first};
    return launch(p, K_SHUTTER_ACCUMULATE, stream, blocks(width, 64), gy, 64, 4, args);
}

// a filtered frame (kernels/filter.hip; geodesic_hip_internal.h, "Filtered frames"): one workgroup of 256 lanes per tile of 32 x 8 output
// pixels (the kernel's GR_FILTER_TX x GR_FILTER_TY), the taps - host memory - copied into the argument block.  gr_filter_frame's refusals
// (imageio.cpp) and the grid's.
int gr_resolve_filtered(gr_program* p, void* stream, const void* src, void* dst, int width, int height, int factor, const float* taps, int count) {
    const char* who = "gr_resolve_filtered";
    GR_NEED(who, src, dst, taps);
    if (!p) return refuse(who, "null program");
    if (width < 1 || height < 1) return refuse(who, "a size below 1");
    if (const char* wrong = gr_internal_filter_table_error(factor, taps, count)) return refuse(who, wrong);
    if (src == dst) return refuse(who, "src and dst are one buffer");
    if (too_many_pixels(width, height, factor)) return refuse(who, "more than 2^31 - 1 source pixels");
    const unsigned gy = blocks(height, 8);
    if (gy > 65535u) return refuse(who, "a frame of " + std::to_string(height) + " rows does not fit the grid");
    struct { float tap[GR_FILTER_MAX_TAPS]; } table = {};
    std::copy(taps, taps + count, table.tap);
    void* args[] = {&src, &dst, &width, &height, &factor, &count, &table};
    return launch(p, K_RESOLVE_FILTERED, stream, blocks(width, 32), gy, 256, 1, args);
}

// ---- glare (kernels/glare.hip; geodesic_hip_internal.h, "Glare") -----------------------------------------------------------------------

int gr_glare_scratch_bytes(int width, int height, size_t* bytes) {
    const char* who = "gr_glare_scratch_bytes";
    if (!bytes) return refuse(who, "null argument");
    GR_CHECK(refuse_size(who, width, height));
    *bytes = (size_t)width * (size_t)height * 4 * sizeof(float);   // h_k of the one component in flight
    return GR_OK;
}

// No component: one elementwise launch.  Otherwise, per component, gr_glare_rows (256 pixels of a row a workgroup) from src into scratch
// and gr_glare_columns (16 x 64 pixels a workgroup) from scratch into dst, which adds the component to core * src (the first) or to what
// dst holds (the others); the component's taps - host memory - are copied into the argument block.  The grids are strided and at most
// 2^20 workgroups.  gr_glare_frame's refusals (imageio.cpp) and the buffers'.
int gr_apply_glare(gr_program* p, void* stream, const void* src, void* dst, void* scratch, size_t scratch_bytes, int width, int height,
                   const gr_glare* g) {
    const char* who = "gr_apply_glare";
    GR_CHECK(refuse_nulls(who, !src || !dst || !scratch || !g, p));
    GR_CHECK(refuse_size(who, width, height));
    if (src == dst) return refuse(who, "src and dst are one buffer");
    GR_CHECK(gr_internal_check_glare(who, g));
    const size_t frame_bytes = (size_t)width * (size_t)height * 4 * sizeof(float);
    if (scratch_bytes < frame_bytes)
        return refuse(who, "scratch of " + std::to_string(scratch_bytes) + " bytes is too short (gr_glare_scratch_bytes: " + std::to_string(frame_bytes) + ")");
    if ((uintptr_t)scratch % 16) return refuse(who, "scratch is not aligned to 16 bytes");
    if (overlaps(src, frame_bytes, dst, frame_bytes) || overlaps(src, frame_bytes, scratch, scratch_bytes) || overlaps(dst, frame_bytes, scratch, scratch_bytes))
        return refuse(who, "src, dst and scratch overlap");
    const unsigned long long pixels = (unsigned long long)width * (unsigned long long)height, cap = 1ull << 20;
    if (g->components == 0) {
        float scale = g->core;
        unsigned long long count = pixels;
        void* args[] = {&src, &dst, &count, &scale};
        return launch(p, K_GLARE_SCALE, stream, strided_grid((pixels + 255) / 256, cap), 1, 256, 1, args);
    }
    const unsigned long long row_tiles = (((unsigned long long)width + 255) / 256) * (unsigned long long)height;
    const unsigned long long column_tiles = (((unsigned long long)width + 15) / 16) * (((unsigned long long)height + 63) / 64);
    for (int k = 0; k < g->components; k++) {
        struct { float tap[GR_GLARE_MAX_TAPS]; } table = {};
        std::copy(g->tap[k], g->tap[k] + g->taps[k], table.tap);
        int count = g->taps[k], first = k == 0 ? 1 : 0;
        float scale = g->core, weight = g->weight[k];
        const void* rows = scratch;
        const void* previous = first ? src : dst;
        void* row_args[] = {&src, &scratch, &width, &height, &count, &table};
        GR_CHECK(launch(p, K_GLARE_ROWS, stream, strided_grid(row_tiles, cap), 1, 256, 1, row_args));
        void* column_args[] = {&rows, &previous, &dst, &width, &height, &count, &scale, &weight, &first, &table};
        GR_CHECK(launch(p, K_GLARE_COLUMNS, stream, strided_grid(column_tiles, cap), 1, 256, 1, column_args));
    }
    return GR_OK;
}

// ---- metering and tone curve (kernels/tone.hip; geodesic_hip_internal.h, "Metering and tone curve") ----------------------------------

// The 385 counters are zeroed on the stream, then one launch: a strided grid of at most METER_MAX_WORKGROUPS workgroups of METER_LANES
// lanes on tiles of METER_TILE pixels.  METER_TILE and METER_LANES are tone.hip's GR_METER_TILE and GR_METER_LANES (tests/test_tone_abi.py
// holds the two files to one value).
static const unsigned long long METER_TILE = 1024, METER_MAX_WORKGROUPS = 1024;
static const unsigned METER_LANES = 256;
int gr_meter_frame(gr_program* p, void* stream, const void* src, int width, int height, void* device_hist) {
    const char* who = "gr_meter_frame";
    GR_CHECK(refuse_nulls(who, !src || !device_hist, p));
    GR_CHECK(refuse_size(who, width, height));
    if ((uintptr_t)src % 16) return refuse(who, "src is not aligned to 16 bytes");
    if ((uintptr_t)device_hist % 4) return refuse(who, "device_hist is not aligned to 4 bytes");
    HIP_CHECK(hipMemsetAsync(device_hist, 0, GR_METER_COUNTERS * sizeof(unsigned), (hipStream_t)stream));
    unsigned long long pixels = (unsigned long long)width * (unsigned long long)height;
    const unsigned grid = strided_grid((pixels + METER_TILE - 1) / METER_TILE, METER_MAX_WORKGROUPS);
    void* args[] = {&src, &pixels, &device_hist};
    return launch(p, K_METER_HISTOGRAM, stream, grid, 1, METER_LANES, 1, args);
}

int gr_meter_solve_device(gr_program* p, void* stream, const void* device_hist, const gr_tone* tone, void* device_state) {
    const char* who = "gr_meter_solve_device";
    GR_CHECK(refuse_nulls(who, !device_hist || !tone || !device_state, p));
    GR_CHECK(gr_internal_check_tone(who, tone));
    if (tone->mode != GR_TONE_AUTO) return refuse(who, "mode is not GR_TONE_AUTO (a manual gain is gr_meter_solve_host's)");
    if ((uintptr_t)device_hist % 4) return refuse(who, "device_hist is not aligned to 4 bytes");
    if ((uintptr_t)device_state % 8) return refuse(who, "device_state is not aligned to 8 bytes");
    float key = tone->key_stops, low = tone->low, high = tone->high, lowest = tone->min_stops, highest = tone->max_stops, rate = tone->rate;
    void* args[] = {&device_hist, &device_state, &key, &low, &high, &lowest, &highest, &rate};
    return launch(p, K_METER_SOLVE, stream, 1, 1, 64, 1, args);
}

int gr_apply_tone(gr_program* p, void* stream, const void* src, void* dst, int width, int height, const gr_tone* tone, const void* device_gain,
                  float host_gain) {
    const char* who = "gr_apply_tone";
    GR_CHECK(refuse_nulls(who, !src || !dst || !tone, p));
    GR_CHECK(refuse_size(who, width, height));
    GR_CHECK(gr_internal_check_tone(who, tone));
    if (!device_gain && (!std::isfinite(host_gain) || host_gain < 0.f)) return refuse(who, "host_gain is not finite or is negative");
    if ((uintptr_t)src % 16 || (uintptr_t)dst % 16) return refuse(who, "src or dst is not aligned to 16 bytes");
    if ((uintptr_t)device_gain % 4) return refuse(who, "device_gain is not aligned to 4 bytes");
    const size_t frame_bytes = (size_t)width * (size_t)height * 4 * sizeof(float);
    if (src != dst && overlaps(src, frame_bytes, dst, frame_bytes)) return refuse(who, "src and dst overlap and are not one buffer");
    unsigned long long pixels = (unsigned long long)width * (unsigned long long)height;
    int curve = tone->curve;
    float iw2 = gr_internal_tone_inverse_white_squared(tone);
    void* args[] = {&src, &dst, &pixels, &curve, &iw2, &device_gain, &host_gain};
    return launch(p, K_TONE_APPLY, stream, strided_grid((pixels + 255) / 256, 1ull << 20), 1, 256, 1, args);
}

}   // extern "C"
