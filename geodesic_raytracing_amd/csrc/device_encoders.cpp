// device_encoders.cpp — the three file encoders that run on the device, gr_png_encoder (kernels/png.hip; its stream and host encoder:
// png_stream.cpp), gr_exr_encoder (kernels/exr.hip; exr_stream.cpp) and gr_jpeg_encoder (kernels/jpeg.hip; jpeg_stream.cpp), on one core: a borrowed program, a fenced scratch
// (guarded_scratch.hpp), a pinned staging buffer and a launch timer.  An encoder adds its region sizes, its own buffers and its encode.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "exr_stream.hpp"
#include "guarded_scratch.hpp"
#include "internal.hpp"
#include "jpeg_stream.hpp"
#include "png_stream.hpp"

using gr_internal::blocks, gr_internal::launch, gr_internal::refuse;

namespace {

int fail(int code, const std::string& msg) { return gr_internal_fail(code, msg.c_str()); }

struct encoder_core {
    gr_program* program = nullptr;
    int device = 0, width = 0, height = 0;
    // device: one allocation of 32-bit words, all filled with GUARD_PATTERN at creation; used[r]: the most words of region r any encode
    // so far may have written (scratch_intact looks at everything else)
    guarded_scratch::layout regions;
    size_t used[guarded_scratch::MAX_REGIONS] = {};
    unsigned int* scratch = nullptr;
    unsigned char* staging = nullptr;   // pinned
    std::vector<void*> on_device, pinned;   // everything allocated, the two above included: the destructor's
    bool time_launches = false, timed = false;
    hipEvent_t events[4] = {};   // made when time_launches is first switched on

    ~encoder_core() {
        if (program) (void)hipSetDevice(device);
        for (void* memory : on_device) (void)hipFree(memory);
        for (void* memory : pinned) (void)hipHostFree(memory);
        for (hipEvent_t e : events)
            if (e) (void)hipEventDestroy(e);
    }
    int borrow(gr_program* p, int w, int h) {
        program = p, device = gr_internal::device_of(p), width = w, height = h;
        HIP_CHECK(hipSetDevice(device));
        return GR_OK;
    }
    template <class T> int allocate(T** out, size_t bytes, bool pin = false) {
        if (pin) HIP_CHECK(hipHostMalloc((void**)out, bytes, hipHostMallocDefault));
        else HIP_CHECK(hipMalloc((void**)out, bytes));
        (pin ? pinned : on_device).push_back(*out);
        return GR_OK;
    }
    int fill_scratch() { HIP_CHECK(hipMemsetD32((hipDeviceptr_t)scratch, (int)guarded_scratch::GUARD_PATTERN, regions.total)); return GR_OK; }
    unsigned int* region(int r) const { return scratch + regions.at[r]; }
    // the launch timer: an event behind what the stream holds, where timing is on; the milliseconds between two of them
    int mark(int i, hipStream_t on) { if (time_launches) HIP_CHECK(hipEventRecord(events[i], on)); return GR_OK; }
    int elapsed(float* ms, int from, int to) { HIP_CHECK(hipEventElapsedTime(ms, events[from], events[to])); return GR_OK; }
};

// the three calls every kind of encoder answers alike; `kind` is "gr_png_encoder", "gr_exr_encoder" or "gr_jpeg_encoder"
int set_time_launches(const std::string& kind, encoder_core* e, int on) {
    if (!e) return fail(GR_ERROR_INVALID_ARGUMENT, kind + "_time_launches: a required pointer is NULL");
    HIP_CHECK(hipSetDevice(e->device));
    if (on)
        for (hipEvent_t& event : e->events)
            if (!event) HIP_CHECK(hipEventCreate(&event));
    e->time_launches = on != 0;
    e->timed = false;
    return GR_OK;
}

// ms[k]: from event k * stride to the event behind it
int launch_ms(const std::string& kind, encoder_core* e, float* ms, int count, int stride) {
    if (!e || !ms) return fail(GR_ERROR_INVALID_ARGUMENT, kind + "_launch_ms: a required pointer is NULL");
    if (!e->timed) return fail(GR_ERROR_INVALID_ARGUMENT, kind + "_launch_ms: no encode was timed (" + kind + "_time_launches)");
    for (int k = 0; k < count; k++) GR_CHECK(e->elapsed(&ms[k], k * stride, k * stride + 1));
    return GR_OK;
}

int scratch_intact(const std::string& kind, encoder_core* e, int* intact) {
    if (!e || !intact) return fail(GR_ERROR_INVALID_ARGUMENT, kind + "_scratch_intact: a required pointer is NULL");
    HIP_CHECK(hipSetDevice(e->device));
    guarded_scratch::span spans[guarded_scratch::MAX_REGIONS + 1];
    const int count = guarded_scratch::unwritten_spans(e->regions, e->used, spans);
    *intact = 1;
    for (int s = 0; s < count; s++) {
        std::vector<unsigned int> host(spans[s].to - spans[s].from);
        HIP_CHECK(hipMemcpy(host.data(), e->scratch + spans[s].from, host.size() * 4, hipMemcpyDeviceToHost));
        if (!guarded_scratch::holds_pattern(host.data(), host.size())) *intact = 0;
    }
    return GR_OK;
}

}   // namespace

// ---- PNG frames --------------------------------------------------------------------------------------------------------------------

struct gr_png_encoder : encoder_core {
    // the stream kind, and with it the bins of a histogram as the kernels store it (256, runs: 285) and the table's symbols (257, 285)
    int stream_kind = GR_PNG_STREAM_LITERALS, bins = 256, symbols = png_stream::SYMBOLS;
    // device: [frame histogram bins | rows' histograms height x bins | rows' sums height x 2] words, downloaded in one copy ...
    unsigned int* statistics = nullptr;
    size_t statistics_words = 0;
    // ... [rows' offsets height + 1, 64 bit | table symbols | header png_stream::HEADER_WORDS] uploaded in one copy ...
    unsigned char* placement = nullptr;
    unsigned char* placement_host = nullptr;   // (pinned)
    size_t placement_bytes = 0;
    // ... and the stream, the scratch's one region: an encode zeroes the words its stream takes and nothing else (used[0]: the longest
    // stream of any encode so far).  The staging buffer takes the statistics, then the stream.
    size_t stream_capacity_words = 0;
};

static int png_encoder_create(const std::string& who, gr_program* p, int width, int height, int stream_kind, gr_png_encoder** out) {
    if (!p || !out) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    if (width < 1 || height < 1) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a size below 1");
    const uint64_t rows_bound = png_stream::rows_bound(width, height);
    if (!rows_bound) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a frame of more than 2^31 - 1 raw bytes");
    if (!png_stream::known_kind(stream_kind)) return fail(GR_ERROR_INVALID_ARGUMENT, who + "an unknown stream kind " + std::to_string(stream_kind));
    auto e = std::make_unique<gr_png_encoder>();
    GR_CHECK(e->borrow(p, width, height));
    e->stream_kind = stream_kind;
    e->bins = png_stream::row_bins_of(stream_kind);
    e->symbols = png_stream::symbols_of(stream_kind);
    e->statistics_words = (size_t)e->bins + (size_t)height * ((size_t)e->bins + 2);
    e->placement_bytes = ((size_t)height + 1) * 8 + ((size_t)e->symbols + png_stream::HEADER_WORDS) * 4;
    e->stream_capacity_words = (size_t)((rows_bound + 3) / 4);
    e->regions = guarded_scratch::lay_out(&e->stream_capacity_words, 1, 1);
    GR_CHECK(e->allocate(&e->statistics, e->statistics_words * 4));
    GR_CHECK(e->allocate(&e->placement, e->placement_bytes));
    GR_CHECK(e->allocate(&e->scratch, e->regions.total * 4));
    GR_CHECK(e->allocate(&e->placement_host, e->placement_bytes, true));
    GR_CHECK(e->allocate(&e->staging, std::max(e->statistics_words * 4, e->stream_capacity_words * 4), true));
    GR_CHECK(e->fill_scratch());
    HIP_CHECK(hipDeviceSynchronize());
    *out = e.release();
    return GR_OK;
}

int gr_png_encoder_create(gr_program* p, int width, int height, gr_png_encoder** out) {
    return png_encoder_create("gr_png_encoder_create: ", p, width, height, GR_PNG_STREAM_LITERALS, out);
}
int gr_png_encoder_create_as(gr_program* p, int width, int height, int stream_kind, gr_png_encoder** out) {
    return png_encoder_create("gr_png_encoder_create_as: ", p, width, height, stream_kind, out);
}
void gr_png_encoder_destroy(gr_png_encoder* e) { delete e; }
int gr_png_encoder_time_launches(gr_png_encoder* e, int on) { return set_time_launches("gr_png_encoder", e, on); }
int gr_png_encoder_launch_ms(gr_png_encoder* e, float ms[2]) { return launch_ms("gr_png_encoder", e, ms, 2, 2); }   // (events 0 - 1, 2 - 3)
int gr_png_encoder_scratch_intact(gr_png_encoder* e, int* intact) { return scratch_intact("gr_png_encoder", e, intact); }

int gr_png_encode_rgba8(gr_png_encoder* e, void* stream, const void* device_rgba8, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    const std::string who = "gr_png_encode_rgba8: ";
    if (!e) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    bool too_small = false;
    const std::string wrong = png_stream::refusal(device_rgba8, e->width, e->height, out_file, capacity, out_bytes, &too_small);
    if (!wrong.empty()) return refuse("gr_png_encode_rgba8", wrong, too_small);
    int width = e->width, height = e->height;
    const bool runs = e->stream_kind == GR_PNG_STREAM_RUNS;
    const size_t bins = (size_t)e->bins;
    hipStream_t on = (hipStream_t)stream;
    HIP_CHECK(hipSetDevice(e->device));
    // the first round trip: the frame's and the rows' histograms, the rows' Adler sums
    unsigned int* frame_histogram = e->statistics;
    unsigned int* row_histogram = e->statistics + bins;
    unsigned int* row_sums = row_histogram + (size_t)height * bins;
    HIP_CHECK(hipMemsetAsync(frame_histogram, 0, bins * 4, on));
    GR_CHECK(e->mark(0, on));
    void* histogram_args[] = {&device_rgba8, &width, &height, &frame_histogram, &row_histogram, &row_sums};
    GR_CHECK(launch(e->program, runs ? K_PNG_HISTOGRAM_RUNS : K_PNG_HISTOGRAM, stream, (unsigned)height, 1, 64, 4, histogram_args));
    GR_CHECK(e->mark(1, on));
    HIP_CHECK(hipMemcpyAsync(e->staging, e->statistics, e->statistics_words * 4, hipMemcpyDeviceToHost, on));
    HIP_CHECK(hipStreamSynchronize(on));
    // the table from the frame's histogram - with what the device does not count: a filter-type byte and an end-of-block a row -, the rows'
    // offsets from their own histograms, the Adler-32 from their sums
    const unsigned int* got = (const unsigned int*)e->staging;
    uint64_t histogram[png_stream::MAX_SYMBOLS] = {};
    for (size_t v = 0; v < bins; v++) histogram[v] = got[v];
    histogram[1] += 1;
    histogram[2] += (uint64_t)height - 1;
    histogram[png_stream::END_OF_BLOCK] = (uint64_t)height;
    png_stream::table t;
    png_stream::build_table(histogram, e->stream_kind, t);
    uint64_t* offset = (uint64_t*)e->placement_host;
    unsigned int* table_words = (unsigned int*)(e->placement_host + ((size_t)height + 1) * 8);
    unsigned int* header_words = table_words + e->symbols;
    std::vector<uint32_t> adlers(height);
    offset[0] = 0;
    for (int r = 0; r < height; r++) {
        offset[r + 1] = offset[r] + png_stream::row_segment_bytes(png_stream::row_block_bits(t, r, got + bins + (size_t)r * bins));
        const unsigned int* sums = got + bins + (size_t)height * bins + 2 * (size_t)r;
        adlers[r] = png_stream::row_adler(r, width, sums[0], sums[1]);
    }
    const uint64_t rows_bytes = offset[height], stream_words = (rows_bytes + 3) / 4;
    if (stream_words > e->stream_capacity_words) return fail(GR_ERROR_DEVICE, who + "the rows' sizes exceed the bound (the device's histograms are not a frame's)");
    for (int s = 0; s < e->symbols; s++) table_words[s] = (unsigned int)t.code[s] | ((unsigned int)t.length[s] << 16);
    std::copy(t.header, t.header + png_stream::HEADER_WORDS, header_words);
    // the second: placement up, the stream zeroed (the pack ORs the words segments share), the pack, the stream down
    unsigned int* stream_at = e->region(0);
    HIP_CHECK(hipMemcpyAsync(e->placement, e->placement_host, e->placement_bytes, hipMemcpyHostToDevice, on));
    HIP_CHECK(hipMemsetAsync(stream_at, 0, (size_t)stream_words * 4, on));
    e->used[0] = std::max(e->used[0], (size_t)stream_words);
    GR_CHECK(e->mark(2, on));
    int header_bits = t.header_bits;
    const unsigned long long* offsets_on_device = (const unsigned long long*)e->placement;
    const unsigned int* table_on_device = (const unsigned int*)(e->placement + ((size_t)height + 1) * 8);
    const unsigned int* header_on_device = table_on_device + e->symbols;
    unsigned long long word_count = stream_words;
    void* pack_args[] = {&device_rgba8, &width, &height, &table_on_device, &header_on_device, &header_bits, &offsets_on_device, &stream_at, &word_count};
    GR_CHECK(launch(e->program, runs ? K_PNG_PACK_RUNS : K_PNG_PACK, stream, (unsigned)height, 1, 64, 4, pack_args));
    GR_CHECK(e->mark(3, on));
    HIP_CHECK(hipMemcpyAsync(e->staging, stream_at, (size_t)stream_words * 4, hipMemcpyDeviceToHost, on));
    HIP_CHECK(hipStreamSynchronize(on));
    e->timed = e->time_launches;
    png_stream::write_container(out_file, width, height, e->staging, rows_bytes, png_stream::join_adler(adlers.data(), width, height));
    *out_bytes = (size_t)png_stream::file_bytes(rows_bytes);
    return GR_OK;
}

// ---- EXR frames --------------------------------------------------------------------------------------------------------------------

struct gr_exr_encoder : encoder_core {
    // device: [frame histogram 256 | rows' histograms height x 256 | rows' sums height x 2] words, downloaded in one copy ...
    unsigned int* statistics = nullptr;
    size_t statistics_words = 0;
    // ... [chunks' offsets height + 1, 64 bit | rows' words height x 2: Adler-32, raw | table 257 | header png_stream::HEADER_WORDS] uploaded in one ...
    unsigned char* placement = nullptr;
    unsigned char* placement_host = nullptr;   // (pinned)
    size_t placement_bytes = 0;
    // ... and the chunk area, the scratch's one region: what follows the offset table in the file, chunk headers included.  An encode zeroes
    // the words its chunks take and nothing else (used[0]: the longest of any encode so far).  The staging buffer takes the statistics, then
    // the chunks; header and offset table are the host's, written into out_file in front of them.
    size_t stream_capacity_words = 0;
};

int gr_exr_encoder_create(gr_program* p, int width, int height, gr_exr_encoder** out) {
    const std::string who = "gr_exr_encoder_create: ";
    if (!p || !out) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    if (width < 1 || height < 1) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a size below 1 (width " + std::to_string(width) + ", height " + std::to_string(height) + ")");
    const uint64_t bound = exr_stream::file_bound(width, height);
    if (!bound) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a row of more than 2^31 - 1 raw bytes (width " + std::to_string(width) + ", 6 bytes a pixel)");
    auto e = std::make_unique<gr_exr_encoder>();
    GR_CHECK(e->borrow(p, width, height));
    e->statistics_words = 256 + (size_t)height * (256 + 2);
    e->placement_bytes = ((size_t)height + 1) * 8 + ((size_t)height * 2 + png_stream::SYMBOLS + png_stream::HEADER_WORDS) * 4;
    e->stream_capacity_words = (size_t)((bound - exr_stream::chunks_at(height) + 3) / 4);
    e->regions = guarded_scratch::lay_out(&e->stream_capacity_words, 1, 1);
    GR_CHECK(e->allocate(&e->statistics, e->statistics_words * 4));
    GR_CHECK(e->allocate(&e->placement, e->placement_bytes));
    GR_CHECK(e->allocate(&e->scratch, e->regions.total * 4));
    GR_CHECK(e->allocate(&e->placement_host, e->placement_bytes, true));
    GR_CHECK(e->allocate(&e->staging, std::max(e->statistics_words * 4, e->stream_capacity_words * 4), true));
    GR_CHECK(e->fill_scratch());
    HIP_CHECK(hipDeviceSynchronize());
    *out = e.release();
    return GR_OK;
}

void gr_exr_encoder_destroy(gr_exr_encoder* e) { delete e; }
int gr_exr_encoder_time_launches(gr_exr_encoder* e, int on) { return set_time_launches("gr_exr_encoder", e, on); }
int gr_exr_encoder_launch_ms(gr_exr_encoder* e, float ms[2]) { return launch_ms("gr_exr_encoder", e, ms, 2, 2); }   // (events 0 - 1, 2 - 3)
int gr_exr_encoder_scratch_intact(gr_exr_encoder* e, int* intact) { return scratch_intact("gr_exr_encoder", e, intact); }

int gr_exr_encode_f32(gr_exr_encoder* e, void* stream, const void* device_rgba_f32, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    const std::string who = "gr_exr_encode_f32: ";
    if (!e) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    bool too_small = false;
    const std::string wrong = exr_stream::refusal(device_rgba_f32, e->width, e->height, out_file, capacity, out_bytes, true, &too_small);
    if (!wrong.empty()) return refuse("gr_exr_encode_f32", wrong, too_small);
    int width = e->width, height = e->height;
    hipStream_t on = (hipStream_t)stream;
    HIP_CHECK(hipSetDevice(e->device));
    // the first round trip: the frame's and the rows' histograms of predicted bytes, the rows' Adler sums
    unsigned int* frame_histogram = e->statistics;
    unsigned int* row_histogram = e->statistics + 256;
    unsigned int* row_sums = row_histogram + (size_t)height * 256;
    HIP_CHECK(hipMemsetAsync(frame_histogram, 0, 256 * 4, on));
    GR_CHECK(e->mark(0, on));
    void* histogram_args[] = {&device_rgba_f32, &width, &height, &frame_histogram, &row_histogram, &row_sums};
    GR_CHECK(launch(e->program, K_EXR_HISTOGRAM, stream, (unsigned)height, 1, 64, 4, histogram_args));
    GR_CHECK(e->mark(1, on));
    HIP_CHECK(hipMemcpyAsync(e->staging, e->statistics, e->statistics_words * 4, hipMemcpyDeviceToHost, on));
    HIP_CHECK(hipStreamSynchronize(on));
    // the table from the frame's histogram and one end-of-block a row; from every row's own histogram the size of its zlib stream, and
    // with it whether the row is stored raw and where its chunk lies; the Adler-32 from its sums
    const unsigned int* got = (const unsigned int*)e->staging;
    uint64_t histogram[png_stream::MAX_SYMBOLS] = {};
    for (int v = 0; v < 256; v++) histogram[v] = got[v];
    histogram[exr_stream::END_OF_BLOCK] = (uint64_t)height;
    png_stream::table t;
    exr_stream::build_table(histogram, t);
    uint64_t* offset = (uint64_t*)e->placement_host;
    unsigned int* row_words = (unsigned int*)(e->placement_host + ((size_t)height + 1) * 8);
    unsigned int* table_words = row_words + 2 * (size_t)height;
    unsigned int* header_words = table_words + png_stream::SYMBOLS;
    const uint64_t raw_bytes = exr_stream::row_bytes(width);
    offset[0] = 0;
    for (int r = 0; r < height; r++) {
        const uint64_t zipped = exr_stream::stream_bytes(exr_stream::row_block_bits(t, got + 256 + (size_t)r * 256));
        const bool raw = exr_stream::stored_raw(zipped, width);
        const unsigned int* sums = got + 256 + (size_t)height * 256 + 2 * (size_t)r;
        offset[r + 1] = offset[r] + exr_stream::CHUNK_HEADER_BYTES + (raw ? raw_bytes : zipped);
        row_words[2 * (size_t)r] = exr_stream::row_adler(width, sums[0], sums[1]);
        row_words[2 * (size_t)r + 1] = raw ? 1u : 0u;
    }
    const uint64_t chunks_bytes = offset[height], stream_words = (chunks_bytes + 3) / 4;
    if (stream_words > e->stream_capacity_words) return fail(GR_ERROR_DEVICE, who + "the chunks' sizes exceed the bound");   // (the raw fallback rules it out)
    for (int s = 0; s < png_stream::SYMBOLS; s++) table_words[s] = (unsigned int)t.code[s] | ((unsigned int)t.length[s] << 16);
    std::copy(t.header, t.header + png_stream::HEADER_WORDS, header_words);
    // the second: placement up, the chunk area zeroed (the pack ORs the words chunks share), the pack, the chunks down
    unsigned int* stream_at = e->region(0);
    HIP_CHECK(hipMemcpyAsync(e->placement, e->placement_host, e->placement_bytes, hipMemcpyHostToDevice, on));
    HIP_CHECK(hipMemsetAsync(stream_at, 0, (size_t)stream_words * 4, on));
    e->used[0] = std::max(e->used[0], (size_t)stream_words);
    GR_CHECK(e->mark(2, on));
    int header_bits = t.header_bits;
    const unsigned long long* offsets_on_device = (const unsigned long long*)e->placement;
    const unsigned int* row_words_on_device = (const unsigned int*)(e->placement + ((size_t)height + 1) * 8);
    const unsigned int* table_on_device = row_words_on_device + 2 * (size_t)height;
    const unsigned int* header_on_device = table_on_device + png_stream::SYMBOLS;
    unsigned long long word_count = stream_words;
    void* pack_args[] = {&device_rgba_f32, &width, &height, &table_on_device, &header_on_device, &header_bits, &offsets_on_device, &row_words_on_device,
                         &stream_at, &word_count};
    GR_CHECK(launch(e->program, K_EXR_PACK, stream, (unsigned)height, 1, 64, 4, pack_args));
    GR_CHECK(e->mark(3, on));
    HIP_CHECK(hipMemcpyAsync(e->staging, stream_at, (size_t)stream_words * 4, hipMemcpyDeviceToHost, on));
    // (the header and the offset table while the chunks travel: the offsets are final)
    exr_stream::write_header(out_file, width, height);
    exr_stream::write_offsets(out_file, height, offset);
    HIP_CHECK(hipStreamSynchronize(on));
    e->timed = e->time_launches;
    memcpy(out_file + exr_stream::chunks_at(height), e->staging, (size_t)chunks_bytes);
    *out_bytes = (size_t)(exr_stream::chunks_at(height) + chunks_bytes);
    return GR_OK;
}

// ---- JPEG frames -------------------------------------------------------------------------------------------------------------------

struct gr_jpeg_encoder : encoder_core {
    int quality = 0;
    // the scratch's four regions, each a multiple of 16 bytes: [coefficients | rows' slots | rows' byte counts, rows' FF counts, the file's
    // size (64 bit) | file]; the file region starts with the headers, uploaded at creation and never written again (used[3]: the longest
    // file of any encode so far; the other three count as written whole).  The staging buffer takes the file's size, then the file.
    unsigned int* tables = nullptr;    // jpeg_stream::device_tables
    uint64_t file_capacity = 0;
};

int gr_jpeg_encoder_create(gr_program* p, int width, int height, int quality, gr_jpeg_encoder** out) {
    const std::string who = "gr_jpeg_encoder_create: ";
    if (!p || !out) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    std::string wrong = jpeg_stream::size_refusal(width, height);
    if (wrong.empty()) wrong = jpeg_stream::quality_refusal(quality);
    if (!wrong.empty()) return fail(GR_ERROR_INVALID_ARGUMENT, who + wrong);
    auto e = std::make_unique<gr_jpeg_encoder>();
    GR_CHECK(e->borrow(p, width, height));
    e->quality = quality;
    const size_t rows = (size_t)jpeg_stream::mcu_rows(height), across = (size_t)jpeg_stream::mcus_across(width);
    e->file_capacity = jpeg_stream::file_bound(width, height);
    const size_t words[4] = {rows * across * jpeg_stream::BLOCKS_PER_MCU * 32, rows * (size_t)(jpeg_stream::row_slot_bytes(width) / 4), 2 * rows + 2,
                             (size_t)((e->file_capacity + 3) / 4)};
    e->regions = guarded_scratch::lay_out(words, 4, 4);
    std::copy(e->regions.words, e->regions.words + 3, e->used);
    e->used[3] = (jpeg_stream::HEADER_BYTES + 3) / 4;
    GR_CHECK(e->allocate(&e->scratch, e->regions.total * 4));
    GR_CHECK(e->allocate(&e->tables, jpeg_stream::TABLE_WORDS * 4));
    GR_CHECK(e->allocate(&e->staging, 8 + e->regions.words[3] * 4, true));
    GR_CHECK(e->fill_scratch());
    uint32_t tables[jpeg_stream::TABLE_WORDS];
    uint8_t headers[jpeg_stream::HEADER_BYTES];
    jpeg_stream::device_tables(quality, tables);
    jpeg_stream::write_headers(headers, width, height, quality);
    HIP_CHECK(hipMemcpy(e->tables, tables, sizeof(tables), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(e->region(3), headers, sizeof(headers), hipMemcpyHostToDevice));
    HIP_CHECK(hipDeviceSynchronize());
    *out = e.release();
    return GR_OK;
}

void gr_jpeg_encoder_destroy(gr_jpeg_encoder* e) { delete e; }
int gr_jpeg_encoder_time_launches(gr_jpeg_encoder* e, int on) { return set_time_launches("gr_jpeg_encoder", e, on); }
int gr_jpeg_encoder_launch_ms(gr_jpeg_encoder* e, float ms[3]) { return launch_ms("gr_jpeg_encoder", e, ms, 3, 1); }   // (events 0 - 1, 1 - 2, 2 - 3)
int gr_jpeg_encoder_scratch_intact(gr_jpeg_encoder* e, int* intact) { return scratch_intact("gr_jpeg_encoder", e, intact); }

int gr_jpeg_encode_rgba8(gr_jpeg_encoder* e, void* stream, const void* device_rgba8, unsigned char* out_file, size_t capacity, size_t* out_bytes) {
    const std::string who = "gr_jpeg_encode_rgba8: ";
    if (!e) return fail(GR_ERROR_INVALID_ARGUMENT, who + "a required pointer is NULL");
    bool too_small = false;
    const std::string wrong = jpeg_stream::refusal(device_rgba8, e->width, e->height, e->quality, out_file, capacity, out_bytes, &too_small);
    if (!wrong.empty()) return refuse("gr_jpeg_encode_rgba8", wrong, too_small);
    hipStream_t on = (hipStream_t)stream;
    HIP_CHECK(hipSetDevice(e->device));
    int width = e->width, height = e->height, rows = jpeg_stream::mcu_rows(height);
    unsigned int* coefficients = e->region(0);
    unsigned int* slots = e->region(1);
    unsigned int* row_bytes = e->region(2);
    unsigned int* row_ff = row_bytes + rows;
    unsigned long long* file_bytes = (unsigned long long*)(e->region(2) + e->regions.words[2] - 2);   // the region's last two words: 8-byte aligned
    unsigned char* file = (unsigned char*)e->region(3);
    unsigned int slot_words = (unsigned int)(jpeg_stream::row_slot_bytes(width) / 4), header_bytes = jpeg_stream::HEADER_BYTES;
    unsigned long long file_capacity = e->file_capacity;
    const unsigned int* tables = e->tables;
    GR_CHECK(e->mark(0, on));
    void* blocks_args[] = {&device_rgba8, &width, &height, &tables, &coefficients};
    GR_CHECK(launch(e->program, K_JPEG_BLOCKS, stream, blocks(jpeg_stream::mcus_across(width), 4), (unsigned)rows, 64, 4, blocks_args));
    GR_CHECK(e->mark(1, on));
    void* pack_args[] = {&coefficients, &width, &height, &tables, &slots, &slot_words, &row_bytes, &row_ff};
    GR_CHECK(launch(e->program, K_JPEG_PACK, stream, (unsigned)rows, 1, 64, 6, pack_args));
    GR_CHECK(e->mark(2, on));
    void* gather_args[] = {&slots, &slot_words, &row_bytes, &row_ff, &rows, &file, &header_bytes, &file_capacity, &file_bytes};
    GR_CHECK(launch(e->program, K_JPEG_GATHER, stream, (unsigned)rows, 1, 64, 4, gather_args));
    GR_CHECK(e->mark(3, on));
    // the first synchronisation: the file's size; the second: that many bytes
    HIP_CHECK(hipMemcpyAsync(e->staging, file_bytes, 8, hipMemcpyDeviceToHost, on));
    HIP_CHECK(hipStreamSynchronize(on));
    e->timed = e->time_launches;
    unsigned long long bytes = 0;
    memcpy(&bytes, e->staging, 8);
    if (bytes <= header_bytes || bytes > file_capacity) return fail(GR_ERROR_DEVICE, who + "the device's file size is not a file's of this frame size");
    e->used[3] = std::max(e->used[3], ((size_t)bytes + 3) / 4);
    HIP_CHECK(hipMemcpyAsync(e->staging + 8, file, (size_t)bytes, hipMemcpyDeviceToHost, on));
    HIP_CHECK(hipStreamSynchronize(on));
    memcpy(out_file, e->staging + 8, (size_t)bytes);
    *out_bytes = (size_t)bytes;
    return GR_OK;
}
