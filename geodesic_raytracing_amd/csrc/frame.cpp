// frame.cpp — per-frame device buffers and the frame enqueue sequence.
//
// Reference counterparts: render_state.hpp:97-197 (buffers), main.cpp:2244-2526 (the sequence of
// launches on one in-order queue), execute_kernel main.cpp:139-205.  Everything is asynchronous on
// the caller's stream; the only host->device traffic per frame is camera (48 B), cfg and features.
// What a frame decides is in frame_plan.cpp, what its delivery decides - the stages behind the trace, their order and their buffers -
// in delivery_plan.cpp; both are host-tested, and this file gathers their inputs and carries their plans out.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <mutex>

#include "delivery_plan.hpp"
#include "frame_format.hpp"
#include "frame_plan.hpp"
#include "internal.hpp"

using frame_plan::origin_on_screen;
using frame_plan::picture_motion;
namespace switches = frame_plan::switches;

// Small host -> device uploads (camera, $cfg values, features) go through PINNED memory of the library's own: hipMemcpyAsync from
// pageable memory may read its source when the stream gets there, not when it is called - and the sources here are locals of
// gr_render_frame and the caller's structs.  With the device to itself a frame's uploads ran at once and nothing showed; eight
// processes sharing one GPU (the inter-process rehearsal of a split frame, tests/test_gpu_two_ranks.py) delayed the streams, and
// a state's first frame read its features off a dead stack frame - one share of one frame rendered with garbage parameters.
// A ring of 256-byte chunks; a chunk is reused 64 uploads later at the earliest, after the event recorded behind ITS copy on the stream
// that copy went to (round 5: one event per 16 uploads, recorded on whichever stream issued the 16th, did not cover the copies the
// caller's stream and the look-ahead slots' streams had queued in between - the host never blocks in the pipelined path and can run
// 64 uploads ahead of a delayed stream).  One lock: two threads may drive one state's look-ahead.
struct upload_ring {
    static const int CHUNK = 256, CHUNKS = 64;
    char* base = nullptr;
    hipEvent_t used[CHUNKS] = {};
    bool recorded[CHUNKS] = {};
    unsigned long long next = 0;
    std::mutex lock;
    int copy(void* dst, const void* src, size_t bytes, hipStream_t stream) {
        if (bytes > (size_t)CHUNK) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "upload_ring: too large");
        std::lock_guard<std::mutex> guard(lock);
        if (!base) {
            HIP_CHECK(hipHostMalloc((void**)&base, (size_t)CHUNK * CHUNKS, hipHostMallocDefault));
            for (auto& e : used) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        const int chunk = (int)(next % CHUNKS);
        if (recorded[chunk]) HIP_CHECK(hipEventSynchronize(used[chunk]));   // (64 uploads ago: long done, whichever stream it was on)
        memcpy(base + (size_t)chunk * CHUNK, src, bytes);
        HIP_CHECK(hipMemcpyAsync(dst, base + (size_t)chunk * CHUNK, bytes, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipEventRecord(used[chunk], stream));
        recorded[chunk] = true;
        next++;
        return GR_OK;
    }
    void release() {
        if (base) (void)hipHostFree(base);
        for (auto& e : used) if (e) (void)hipEventDestroy(e);
        base = nullptr;
    }
};

struct gr_render_state {
    int device = 0;
    int width = 0, height = 0;      // what every frame of the state is traced and shaded at
    // gr_render_state_create_supersampled: width x height above are supersample x the caller's frame per axis; a frame is shaded into
    // traced_frame (float4[width * height], NULL for factor 1) and box-averaged from there into the caller's out (gr_resolve_supersampled).
    // gr_render_frame_rgba8 shades into it at every factor: a factor-1 state gets one, and the events, with its first 8-bit frame.
    int supersample = 1;
    int out_width = 0, out_height = 0;
    void* traced_frame = nullptr;
    // gr_render_subframe: the sum of the shutter's sub-frames so far, float4[out_width * out_height], allocated with the state's first
    // sub-frame; accumulated: sub-frames in it since the last one with `first` (0: nothing to add to, nothing to deliver)
    void* accumulation = nullptr;
    unsigned long long accumulated = 0;
    // What gr_render_state_set_filter, _set_glare and _set_tone set, and the buffers their stages work in (delivery_plan.hpp tells the
    // chain and names the buffers: filtered_frame is its RESOLVED).  Each is float4[out_width * out_height] - but tone_words: a
    // gr_tone_state, then the 385 counters - and is allocated with the first call whose plan needs it and that is not refused.
    int filter = GR_FILTER_BOX;
    void* filtered_frame = nullptr;
    bool glare_set = false;
    gr_glare glare{};
    void* glare_frame = nullptr;
    void* glare_scratch = nullptr;
    bool tone_set = false;
    gr_tone tone{};
    void* tone_frame = nullptr;
    void* tone_words = nullptr;
    bool tone_reset = false;   // the adaptation state is zeroed on the stream of the next delivery
    // gr_render_state_set_sky: with a sky every frame of the state is shaded by gr_render_analytic and reads no background; without
    // one (the default) by gr_render / gr_render_strips, launch for launch as before.  Shading only: the records do not depend on it.
    bool sky_set = false;
    gr_analytic_sky sky{};
    // gr_render_state_set_stars: likewise shaded by gr_render_stars, from catalogues the caller keeps alive; never both (the setters refuse)
    bool stars_set = false;
    gr_star_sky star_sky{};
    const gr_star_catalogue* near_stars = nullptr;
    const gr_star_catalogue* far_stars = nullptr;
    hipEvent_t ev_resolve[2] = {};   // time_kernels = 1: around the resolve launch (gr_render_state_resolve_ms)
    bool resolve_timed = false;
    upload_ring uploads;
    // small buffers (render_state.hpp:150-170)
    void* camera_pos_cart = nullptr;
    void* camera_quat = nullptr;
    void* camera_pos_generic = nullptr;
    void* tetrad[4] = {};
    void* rays_count_in = nullptr;
    void* rays_adaptive_count = nullptr;
    void* render_data_count = nullptr;
    void* cfg = nullptr;            // struct dynamic_config (floats in declaration order)
    void* dfg = nullptr;            // struct dynamic_feature_config
    void* attempts = nullptr;       // uint64[GR_COUNTER_WORDS]: attempts, shader cycles, 100 MHz ticks, waves (the last three: fused trace only); [8..255] probe builds; [256..511] the fused trace's attempts, spread
    // per-pixel buffers (render_state.hpp:172-196); ray records are allocated on first use
    void* rays_in = nullptr;
    void* rays_adaptive = nullptr;
    void* render_data = nullptr;
    void* termination_buffer = nullptr;
    void* tile_order = nullptr;      // the order the persistent trace hands its tiles out in (gr_order_tiles)
    size_t tile_order_bytes = 0;
    // what each tile of the last fused frame cost (gr_trace_fused_args.tile_cost) and the frame shape that goes with it: the next
    // frame's tiles are handed out dearest first by it (gr_frame_options.tile_history)
    void* lattice_rays = nullptr;   // adaptive sampling on the fused path: gr_lattice_rays_bytes (allocated on first use)
    // the pixels of the second launch traced ahead by the lattice launch (gr_apply_guessed): [0] what this frame's lattice launch traces,
    // [1] what this frame's second launch leaves for the next; swapped every frame that keeps them
    void* guessed[2] = {nullptr, nullptr};
    bool guessed_valid = false;
    void* parking_records = nullptr;   // gr_trace_fused_parking's lot (gr_parking_lot_bytes; allocated the first time a frame parks)
    void* parking_words = nullptr;
    int parking_slots = 0;
    void* pending_list = nullptr;   // ... the pixels of its second launch, dearest first: gr_pending_list_bytes
    // ... and what the rays of each 2x2 block cost in this frame / in the frame before (the two alternate): the order of the next
    // frame's list while the picture moves little
    void* block_cost = nullptr;
    void* block_cost_before = nullptr;
    bool block_cost_valid = false;
    unsigned long long block_cost_program = 0;
    gr_camera block_cost_camera{};
    void* tile_cost = nullptr;
    int tile_cost_shape[3] = {0, 0, 0};   // block_rows, strip_rank, strip_count
    bool tile_cost_valid = false;
    float tile_cost_anchor[2] = {0, 0};   // the pixel that frame's camera saw the coordinate origin at (origin_on_screen)
    bool tile_cost_anchored = false;
    gr_camera tile_cost_camera{};
    unsigned long long tile_cost_program = 0;
    // reference-shaped sequence, rays in tile slot order: what every tile cost in this state's last such frame ([1]: the one before),
    // and the tiles sorted by it (gr_do_generic_rays_scheduled, gr_sort_tiles_by_cost)
    void* ref_cost[2] = {nullptr, nullptr};
    void* ref_order = nullptr;
    void* ref_sort_work = nullptr;
    int ref_cost_tiles = 0;
    bool ref_cost_valid = false;
    gr_camera ref_cost_camera{};
    unsigned long long ref_cost_program = 0;
    unsigned long long history_recorded = 0, history_followed = 0;   // frames (gr_render_state_tile_history)
    unsigned long long prepass_reused = 0;   // frames that took the previous frame's set-up and prepass (gr_render_state_prepass_reused)
    int history_last_shift[2] = {0, 0};
    size_t ray_capacity = 0;
    hipEvent_t ev_start[GR_STAGE_COUNT] = {};
    hipEvent_t ev_stop[GR_STAGE_COUNT] = {};
    bool stage_timed[GR_STAGE_COUNT] = {};
    std::vector<float> host_cfg;
    gr_features host_features{};
    bool features_valid = false;
    // Look-ahead (gr_frame_options.next_camera / next_camera2): the camera set-up and the prepass of the next one or two
    // frames - latency-bound launches of only W/16 x H/16 rays - run on high-priority side streams into buffer sets of
    // their own while this frame traces.  A frame that finds its own request in a slot swaps that set in and skips both.
    struct camera_set {
        void* camera_pos_cart = nullptr;
        void* camera_quat = nullptr;
        void* camera_pos_generic = nullptr;
        void* tetrad[4] = {};
        void* termination_buffer = nullptr;
        void* tile_order = nullptr;   // gr_order_tiles' list for the frame's trace (the cost estimates sit behind the prepass flags)
    };
    struct prefetch_key {
        gr_camera camera{};
        std::vector<float> cfg;
        gr_features features{};
        unsigned long long program = 0;   // gr_program_serial: an address could be reused by a later program
        const void* geodesic = nullptr;
        float geodesic_time = 0;
        int transport = 0;
        int strip[3] = {0, 0, 0};   // block_rows, strip_rank, strip_count: the prepass only covers the cells these rows look at
        bool operator==(const prefetch_key& o) const {
            return memcmp(&camera, &o.camera, sizeof(camera)) == 0 && cfg == o.cfg && memcmp(&features, &o.features, sizeof(features)) == 0 &&
                   program == o.program && geodesic == o.geodesic && (!geodesic || (geodesic_time == o.geodesic_time && transport == o.transport)) &&
                   memcmp(strip, o.strip, sizeof(strip)) == 0;
        }
    };
    struct prefetch_slot {
        camera_set set;
        void* velocity = nullptr;   // interpolated 4-velocity written by handle_interpolating_geodesic (unused here)
        hipStream_t stream = nullptr;
        hipEvent_t ready = nullptr;
        bool valid = false;
        unsigned long long age = 0;
        prefetch_key key;
    };
    static const int LOOKAHEAD = 2;
    prefetch_slot pre[LOOKAHEAD];
    prefetch_key previous_key;          // of the last whole fused frame with a prepass, whose camera set-up and prepass verdicts are still
    bool previous_key_valid = false;    // in the current buffer set (gr_frame_tuning.reuse_still_camera); false once anybody was handed a buffer
    hipStream_t previous_stream = nullptr;
    // Prepass policy (use_prepass = -2, whole frames on the fused path; opt-in: see the last sentence).  The prepass pays for itself through the pixels it lets the
    // trace skip; where it skips next to nothing (Kerr with a = 0.9 in the script's units: a naked singularity, no shadow - 8.4 ms of
    // single-ray latency in front of every 4K frame, for nothing) it is left out: its flags are copied to the host after a frame
    // that ran it, read a frame or two later without waiting, and when fewer than PREPASS_MIN_SKIP of the cells have their whole
    // 5-point stencil marked (the share of the pixels the trace may skip) the next PREPASS_HOLIDAY frames go without one; then it
    // is tried again.  Not the default, because it is not quite neutral: a pixel the prepass skips is black by decree (its five cells'
    // rays were lost), and traced on its own its ray may still find a way out in a chaotic region - measured on the a = 0.9 frame:
    // the pixels that differ are among the < 2 % the prepass would have skipped (tests/test_gpu_schedule.py).
    struct prepass_policy {
        int* host_flags = nullptr;   // pinned
        size_t capacity = 0, cells = 0;
        int grid_width = 0;
        hipEvent_t copied = nullptr;
        bool in_flight = false;
        int holiday = 0;
        float last_fraction = -1.f;
        unsigned long long with_prepass = 0, without_prepass = 0;
    } policy;
    static constexpr float PREPASS_MIN_SKIP = 0.02f;
    static const int PREPASS_HOLIDAY = 30;
    hipEvent_t main_mark = nullptr;
    unsigned long long frame_counter = 0;
    unsigned long long policy_program = 0;
    // time_kernels == 2: one event pair per trace launch, kept until gr_render_state_trace_log collects them (frames of
    // several states overlap on the GPU in pipelined rendering, so "the last frame" is not a representative sample)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> trace_log;
    size_t trace_log_used = 0;

    void swap_in(camera_set& o) {
        std::swap(camera_pos_cart, o.camera_pos_cart);
        std::swap(camera_quat, o.camera_quat);
        std::swap(camera_pos_generic, o.camera_pos_generic);
        for (int i = 0; i < 4; i++) std::swap(tetrad[i], o.tetrad[i]);
        std::swap(termination_buffer, o.termination_buffer);
        std::swap(tile_order, o.tile_order);
    }
};

static const int CFG_MAX = 64;

// A snapshot of the camera's own timelike geodesic (main.cpp:1232-1242 buffers, :2675-2760 snapshot): path, velocity and
// proper-time step per sample, the four tetrad legs parallel transported along it, all resident on the device.
struct gr_geodesic_camera {
    int device = 0;
    upload_ring uploads;
    int max_path_length = 0;
    void* path = nullptr;        // float4[max]
    void* velocity = nullptr;    // float4[max]
    void* ds = nullptr;          // float[max]
    void* count = nullptr;       // int
    void* transported[4] = {};   // float4[max] each
    void* ray = nullptr;         // lightray
    void* ray_count = nullptr;   // int
    void* basis_speed = nullptr; // float4
    void* camera_generic = nullptr;
    void* tetrad[4] = {};
    void* interpolated_velocity = nullptr;
    void* cfg = nullptr;
    void* dfg = nullptr;
    int steps = 0;
    float proper_time = 0;
};

// features and $cfg values as a frame or a snapshot gets them: the caller's, else the metric's defaults
static int resolve_parameters(const gr_metric* m, const gr_features* features_in, const float* cfg_values, int num_cfg_values, gr_metric_info& info,
                              gr_features& features, std::vector<float>& cfg) {
    GR_CHECK(gr_metric_get_info(m, &info));
    gr_features_default(&features);
    if (features_in) features = *features_in;
    else features.max_acceleration_change = info.max_acceleration_change;   // metric_manager.hpp:50
    // dynamic_config: $cfg values in declaration order (metric_manager.hpp:60-66)
    cfg.assign(info.num_dynamic_vars > 0 ? info.num_dynamic_vars : 1, 0.f);
    for (int i = 0; i < info.num_dynamic_vars; i++)
        cfg[i] = (cfg_values && i < num_cfg_values) ? cfg_values[i] : gr_metric_dynamic_var_default(m, i);
    if ((int)cfg.size() > CFG_MAX) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "too many dynamic variables");
    return GR_OK;
}

extern "C" {

int gr_render_state_tile_history(gr_render_state* s, unsigned long long* frames_recorded, unsigned long long* frames_followed, int last_shift[2]) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    if (frames_recorded) *frames_recorded = s->history_recorded;
    if (frames_followed) *frames_followed = s->history_followed;
    if (last_shift) { last_shift[0] = s->history_last_shift[0]; last_shift[1] = s->history_last_shift[1]; }
    return GR_OK;
}

int gr_render_state_prepass_reused(gr_render_state* s, unsigned long long* frames) {
    if (!s || !frames) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    *frames = s->prepass_reused;
    return GR_OK;
}

int gr_camera_origin_on_screen(const gr_camera* camera, float field_of_view, int width, int height, float pixel_out[2]) {
    if (!camera || !pixel_out || width <= 0 || height <= 0) return 0;
    return origin_on_screen(*camera, field_of_view, width, height, pixel_out) ? 1 : 0;
}

float gr_picture_motion(const gr_camera* from, const gr_camera* to, float field_of_view, int width) {
    if (!from || !to || width <= 0) return 1e9f;
    return picture_motion(*from, *to, field_of_view, width);
}

// Is an earlier fused frame still on this device when the next one is submitted?  (What tile_history's default asks: a frame that
// has the device to itself ends when its last tile ends, and the order of its tiles decides when that is; frames that overlap fill
// each other's tails, and there the order measured 3-4 % slower than image order.)  The end of every fused frame is marked with an
// event; the question is whether the latest such mark has been reached.
namespace {
struct device_activity {
    std::mutex lock;
    struct mark { hipEvent_t reached = nullptr; hipStream_t stream = nullptr; bool set = false; } marks[4];
    unsigned int used = 0;
};
device_activity g_activity[64];

// Frames on the caller's own stream do not count: they run one after the other whatever the host does, so a host that submits
// its next frame while the last one is still running - on the same stream - has the device to itself per frame all the same.
bool earlier_frame_still_running(int device, hipStream_t stream) {
    if (device < 0 || device >= 64) return false;
    auto& a = g_activity[device];
    std::lock_guard<std::mutex> hold(a.lock);
    for (auto& m : a.marks) {
        if (!m.set || m.stream == stream) continue;
        const hipError_t e = hipEventQuery(m.reached);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return true; }
        m.set = false;   // reached (or unusable): nothing to ask again
    }
    return false;
}

void mark_frame_end(int device, hipStream_t stream) {
    if (device < 0 || device >= 64) return;
    auto& a = g_activity[device];
    std::lock_guard<std::mutex> hold(a.lock);
    // the stream's own slot if it has one (one mark per stream is enough: its latest), else the oldest
    auto* slot = &a.marks[a.used % 4];
    for (auto& m : a.marks)
        if (m.set && m.stream == stream) { slot = &m; break; }
    if (!slot->reached && hipEventCreateWithFlags(&slot->reached, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        slot->reached = nullptr;
        return;
    }
    if (hipEventRecord(slot->reached, stream) == hipSuccess) {
        if (slot == &a.marks[a.used % 4]) a.used++;
        slot->stream = stream;
        slot->set = true;
    } else {
        (void)hipGetLastError();
    }
}
}   // namespace

void gr_camera_default(gr_camera* c) {
    if (!c) return;
    // camera::camera(), main.cpp:669-673: rot.load_from_axis_angle({1, 0, 0, -pi/2})
    c->position[0] = 0; c->position[1] = 0; c->position[2] = -4; c->position[3] = 0;
    float half = (float)(-M_PI / 2) / 2;
    c->quat[0] = std::sin(half); c->quat[1] = 0; c->quat[2] = 0; c->quat[3] = std::cos(half);
    c->basis_speed[0] = c->basis_speed[1] = c->basis_speed[2] = 0;
    c->flip = 0;
}

int gr_render_state_prepass_policy(gr_render_state* s, unsigned long long* frames_with_prepass, unsigned long long* frames_without,
                                   float* last_marked_fraction) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    if (frames_with_prepass) *frames_with_prepass = s->policy.with_prepass;
    if (frames_without) *frames_without = s->policy.without_prepass;
    if (last_marked_fraction) *last_marked_fraction = s->policy.last_fraction;
    return GR_OK;
}

void gr_frame_options_default(gr_frame_options* o) {
    if (!o) return;
    o->mode = GR_MODE_FUSED;
    o->tiled = 1;
    o->use_prepass = -1;
    o->max_probes = 8;
    o->strip_rank = 0;
    o->strip_count = 1;
    o->block_rows = 16;
    o->compact_out = 0;
    o->time_kernels = 0;
    o->next_camera = nullptr;
    o->next_camera2 = nullptr;
    o->geodesic = nullptr;
    o->geodesic_time = 0;
    o->parallel_transport_observer = 1;   // main.cpp:1259
    o->tuning = nullptr;
}

void gr_frame_tuning_default(gr_frame_tuning* t) {
    if (!t) return;
    t->ray_compaction = -1;
    t->rays_per_lane = 0;
    t->fused_shading = -1;
    t->inline_prepass = -1;
    t->trace_waves_per_simd = 0;
    t->tile_history = -1;
    t->park_lanes = -1;
    t->park_trips = 0;
    t->next_strip_rank = -1;
    t->next_strip_rank2 = -1;
    t->next_geodesic_time = 0;
    t->next_geodesic_time2 = 0;
    t->count_attempts = 0;
    t->guess_still_camera = -1;
    t->reuse_still_camera = -1;
    t->speculative_classes = -1;
}

int gr_device_count(int* count) {
    if (!count) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipGetDeviceCount(count));
    return GR_OK;
}
int gr_device_alloc(int device, size_t bytes, void** out) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMalloc(out, bytes ? bytes : 1));
    return GR_OK;
}
int gr_device_free(int device, void* ptr) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipFree(ptr));
    return GR_OK;
}
int gr_device_download(int device, void* dst, const void* src, size_t bytes) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return GR_OK;
}
int gr_device_upload(int device, void* dst, const void* src, size_t bytes) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return GR_OK;
}
int gr_stream_create(int device, int high_priority, void** out) {
    if (!out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipSetDevice(device));
    hipStream_t s = nullptr;
    if (high_priority) {
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
    } else {
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    *out = (void*)s;
    return GR_OK;
}
int gr_stream_synchronize(void* stream) {
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return GR_OK;
}
int gr_stream_destroy(void* stream) {
    if (stream) HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return GR_OK;
}
int gr_device_synchronize(int device) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipDeviceSynchronize());
    return GR_OK;
}
int gr_host_alloc(size_t bytes, void** out) {
    if (!out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return GR_OK;
}
int gr_host_free(void* ptr) {
    if (ptr) HIP_CHECK(hipHostFree(ptr));
    return GR_OK;
}
int gr_device_download_async(void* stream, void* host_dst, const void* device_src, size_t bytes) {
    if (!host_dst || !device_src) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return GR_OK;
}

// The states that exist (create_render_state adds one, gr_render_state_destroy takes it off).  Why a list: gr_render_frame and
// gr_render_subframe promise to refuse a NULL background with an error code BEFORE they look inside any object they were handed - a
// caller's mistake must not become a crash, and tests/test_shutter_abi.py holds them to it with pointers that are no states at all.
// Whether a NULL background is a mistake now depends on the state (one with a sky reads none), so that one question is asked only of a
// pointer found here.  It is asked only when a background is missing: a frame that brings its textures never takes the lock.
static std::mutex live_states_lock;
static std::vector<const gr_render_state*> live_states;
static bool state_has_sky(const gr_render_state* s) {
    std::lock_guard<std::mutex> guard(live_states_lock);
    return std::find(live_states.begin(), live_states.end(), s) != live_states.end() && (s->sky_set || s->stars_set);
}

// a state whose frames are out_width x out_height and are traced at factor x that per axis (1: gr_render_state_create)
static int create_render_state(int device, int out_width, int out_height, int factor, gr_render_state** out) {
    if (!out || out_width <= 0 || out_height <= 0) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "bad render state size");
    if (factor < 1 || factor > 4)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("supersampling factor " + std::to_string(factor) + ": 1, 2, 3 or 4 per axis").c_str());
    if (factor > 1 && (long long)out_width * factor * out_height * factor > 0x7fffffffll)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("supersampling factor " + std::to_string(factor) + ": " + std::to_string(out_width) + " x " +
                                                            std::to_string(out_height) + " traced at that factor has more pixels than an int counts").c_str());
    const int width = out_width * factor, height = out_height * factor;
    HIP_CHECK(hipSetDevice(device));
    gr_render_state* s = new gr_render_state();
    s->device = device;
    s->width = width;
    s->height = height;
    s->supersample = factor;
    s->out_width = out_width;
    s->out_height = out_height;
    auto alloc = [&](void** p, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
        return e;
    };
    hipError_t e = hipSuccess;
    auto A = [&](void** p, size_t bytes) { if (e == hipSuccess) e = alloc(p, bytes); };
    A(&s->camera_pos_cart, 16);
    A(&s->camera_quat, 16);
    A(&s->camera_pos_generic, 16);
    for (auto& t : s->tetrad) A(&t, 16);
    A(&s->rays_count_in, 4);
    A(&s->rays_adaptive_count, 4);
    A(&s->render_data_count, 4);
    A(&s->cfg, CFG_MAX * sizeof(float));
    A(&s->dfg, sizeof(gr_features));
    A(&s->attempts, GR_COUNTER_WORDS * 8);
    size_t px = (size_t)width * height;
    A(&s->render_data, px * sizeof(gr_render_data));
    A(&s->termination_buffer, px * sizeof(int));
    // two words per tile: 8x8 tiles of the whole image or, split over devices, of at most all its blocks + their halo pieces
    const size_t order_bytes = (px / 16 + 2 * (size_t)width + 8192) * sizeof(unsigned int);
    A(&s->tile_order, order_bytes);
    s->tile_order_bytes = order_bytes;
    A(&s->tile_cost, order_bytes / 2);
    for (auto& slot : s->pre) {
        A(&slot.set.camera_pos_cart, 16);
        A(&slot.set.camera_quat, 16);
        A(&slot.set.camera_pos_generic, 16);
        for (auto& t : slot.set.tetrad) A(&t, 16);
        A(&slot.set.termination_buffer, px * sizeof(int));
        A(&slot.set.tile_order, order_bytes);
        A(&slot.velocity, 16);
    }
    if (factor > 1) {
        A(&s->traced_frame, px * 4 * sizeof(float));
        for (auto& ev : s->ev_resolve)
            if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (e == hipSuccess) {
        // High priority: the look-ahead prepass is a latency-bound launch of a few hundred waves that must make progress
        // while the trace kernel occupies every CU, and priority streams get hardware queues of their own (with the
        // default priority the stream can share a queue with the caller's stream once a framework - torch + RCCL - has
        // created a few streams of its own, which serialises the overlap: measured 6.66 -> 7.98 ms per 4K frame).
        int least = 0, greatest = 0;
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        for (auto& slot : s->pre) {
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&slot.stream, hipStreamNonBlocking, greatest);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&slot.ready, hipEventDisableTiming);
        }
    }
    // hipMemset returns before the device has done it, and the null stream it is ordered on does not hold back the non-blocking
    // streams frames are submitted on: a state's first frame could be overtaken by its own zeroing (seen with eight processes
    // sharing one GPU: a share of a state's first frame rendered from a zeroed camera and features)
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->main_mark, hipEventDisableTiming);
    for (int i = 0; i < GR_STAGE_COUNT && e == hipSuccess; i++) {
        e = hipEventCreate(&s->ev_start[i]);
        if (e == hipSuccess) e = hipEventCreate(&s->ev_stop[i]);
    }
    if (e != hipSuccess) {
        gr_render_state_destroy(s);
        return gr_internal_fail(GR_ERROR_DEVICE, (std::string("render state allocation: ") + hipGetErrorString(e)).c_str());
    }
    {
        std::lock_guard<std::mutex> guard(live_states_lock);
        live_states.push_back(s);
    }
    *out = s;
    return GR_OK;
}

int gr_render_state_create(int device, int width, int height, gr_render_state** out) { return create_render_state(device, width, height, 1, out); }

int gr_render_state_create_supersampled(int device, int width, int height, int factor, gr_render_state** out) {
    return create_render_state(device, width, height, factor, out);
}

int gr_render_state_supersample(const gr_render_state* s, int* factor, int* traced_width, int* traced_height) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null render state");
    if (factor) *factor = s->supersample;
    if (traced_width) *traced_width = s->width;
    if (traced_height) *traced_height = s->height;
    return GR_OK;
}

int gr_render_state_set_filter(gr_render_state* s, int filter) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_filter: null render state");
    if (filter != GR_FILTER_BOX && filter != GR_FILTER_TENT && filter != GR_FILTER_GAUSSIAN && filter != GR_FILTER_MITCHELL)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("gr_render_state_set_filter: unknown filter " + std::to_string(filter) +
                                                            " (GR_FILTER_BOX, GR_FILTER_TENT, GR_FILTER_GAUSSIAN or GR_FILTER_MITCHELL)").c_str());
    s->filter = filter;
    return GR_OK;
}

int gr_render_state_filter(const gr_render_state* s, int* filter) {
    if (!s || !filter) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_filter: null argument");
    *filter = s->filter;
    return GR_OK;
}

int gr_render_state_set_glare(gr_render_state* s, const gr_glare* glare) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_glare: null render state");
    if (glare) {
        GR_CHECK(gr_internal_check_glare("gr_render_state_set_glare", glare));
        s->glare = *glare;
    }
    s->glare_set = glare != nullptr;
    return GR_OK;
}

int gr_render_state_glare(const gr_render_state* s, gr_glare* out, int* is_set) {
    if (!s || !out || !is_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_glare: null argument");
    *is_set = s->glare_set ? 1 : 0;
    if (s->glare_set) *out = s->glare;
    return GR_OK;
}

int gr_render_state_set_tone(gr_render_state* s, const gr_tone* tone) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_tone: null render state");
    if (tone) {
        GR_CHECK(gr_internal_check_tone("gr_render_state_set_tone", tone));
        s->tone = *tone;
    }
    s->tone_set = tone != nullptr;
    s->tone_reset = true;   // (the adaptation starts again; zeroed on the stream of the next delivery: nothing here touches the device)
    return GR_OK;
}

int gr_render_state_tone(const gr_render_state* s, gr_tone* out, int* is_set) {
    if (!s || !out || !is_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_tone: null argument");
    *is_set = s->tone_set ? 1 : 0;
    if (s->tone_set) *out = s->tone;
    return GR_OK;
}

// the last delivered frame's exposure: the only call here that waits for the device (tests, the CLI's printout)
int gr_render_state_exposure(gr_render_state* s, void* stream, float* stops, float* gain) {
    if (!s || !stops || !gain) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_exposure: null argument");
    if (!s->tone_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_exposure: the state has no tone (gr_render_state_set_tone)");
    gr_tone_state words{};
    words.gain = 1.f;
    if (s->tone.mode == GR_TONE_MANUAL) {
        gr_internal_tone_gain((double)s->tone.stops, &words.gain, &words.q);
    } else if (s->tone_words && !s->tone_reset) {
        HIP_CHECK(hipSetDevice(s->device));
        HIP_CHECK(hipMemcpyAsync(&words, s->tone_words, sizeof words, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        if (!words.primed && words.gain == 0.f) words.gain = 1.f;   // (no frame delivered yet: the words are still zero)
    }
    *stops = (float)words.q / 16.f;
    *gain = words.gain;
    return GR_OK;
}

int gr_render_state_set_sky(gr_render_state* s, const gr_analytic_sky* sky) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_sky: null render state");
    if (sky) {
        GR_CHECK(gr_internal_check_analytic_sky("gr_render_state_set_sky", sky));   // (the sky is looked at before the state)
        if (s->stars_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_sky: the state has stars (gr_render_state_set_stars); the two are not composed");
        s->sky = *sky;
    }
    s->sky_set = sky != nullptr;
    return GR_OK;
}

int gr_render_state_sky(const gr_render_state* s, gr_analytic_sky* out, int* is_set) {
    if (!s || !out || !is_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_sky: null argument");
    *is_set = s->sky_set ? 1 : 0;
    if (s->sky_set) *out = s->sky;
    return GR_OK;
}

int gr_render_state_set_stars(gr_render_state* s, const gr_star_sky* sky, const gr_star_catalogue* near, const gr_star_catalogue* far) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_stars: null render state");
    if (sky) {
        GR_CHECK(gr_internal_check_star_sky("gr_render_state_set_stars", sky, near, far, nullptr));   // (likewise)
        if (s->sky_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_set_stars: the state has an analytic sky (gr_render_state_set_sky); the two are not composed");
        s->star_sky = *sky;
    }
    s->stars_set = sky != nullptr;
    s->near_stars = sky ? near : nullptr;
    s->far_stars = sky ? far : nullptr;
    return GR_OK;
}

int gr_render_state_stars(const gr_render_state* s, gr_star_sky* out, const gr_star_catalogue** near, const gr_star_catalogue** far, int* is_set) {
    if (!s || !out || !near || !far || !is_set) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_state_stars: null argument");
    *is_set = s->stars_set ? 1 : 0;
    if (s->stars_set) *out = s->star_sky, *near = s->near_stars, *far = s->far_stars;
    return GR_OK;
}

int gr_render_state_resolve_ms(gr_render_state* s, float* ms) {
    if (!s || !ms) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    *ms = 0;
    if (!s->resolve_timed) return GR_OK;
    HIP_CHECK(hipEventSynchronize(s->ev_resolve[1]));
    HIP_CHECK(hipEventElapsedTime(ms, s->ev_resolve[0], s->ev_resolve[1]));
    return GR_OK;
}

void gr_render_state_destroy(gr_render_state* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();   // (uploads from the pinned ring may still be queued)
    s->uploads.release();
    std::vector<void*> ptrs = {s->camera_pos_cart, s->camera_quat, s->camera_pos_generic, s->tetrad[0], s->tetrad[1], s->tetrad[2],
                               s->tetrad[3], s->rays_count_in, s->rays_adaptive_count, s->render_data_count, s->cfg, s->dfg,
                               s->attempts, s->rays_in, s->rays_adaptive, s->render_data, s->termination_buffer, s->tile_order,
                               s->tile_cost, s->lattice_rays, s->guessed[0], s->guessed[1], s->pending_list, s->block_cost, s->block_cost_before, s->ref_cost[0], s->ref_cost[1], s->ref_order, s->ref_sort_work, s->parking_records, s->parking_words,
                               s->traced_frame, s->accumulation, s->filtered_frame, s->glare_frame, s->glare_scratch, s->tone_frame, s->tone_words};
    for (auto& slot : s->pre) {
        if (slot.stream) { (void)hipStreamSynchronize(slot.stream); (void)hipStreamDestroy(slot.stream); }
        if (slot.ready) (void)hipEventDestroy(slot.ready);
        ptrs.insert(ptrs.end(), {slot.set.camera_pos_cart, slot.set.camera_quat, slot.set.camera_pos_generic, slot.set.tetrad[0],
                                 slot.set.tetrad[1], slot.set.tetrad[2], slot.set.tetrad[3], slot.set.termination_buffer, slot.set.tile_order,
                                 slot.velocity});
    }
    if (s->main_mark) (void)hipEventDestroy(s->main_mark);
    for (auto& ev : s->ev_resolve) if (ev) (void)hipEventDestroy(ev);
    if (s->policy.copied) (void)hipEventDestroy(s->policy.copied);
    if (s->policy.host_flags) (void)hipHostFree(s->policy.host_flags);
    for (auto& pr : s->trace_log) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (int i = 0; i < GR_STAGE_COUNT; i++) {
        if (s->ev_start[i]) (void)hipEventDestroy(s->ev_start[i]);
        if (s->ev_stop[i]) (void)hipEventDestroy(s->ev_stop[i]);
    }
    {
        std::lock_guard<std::mutex> guard(live_states_lock);
        live_states.erase(std::remove(live_states.begin(), live_states.end(), s), live_states.end());
    }
    delete s;
}

// (for csrc/tiled.cpp: a participant checks that the state it is handed is of its frame's size)
extern "C" int gr_internal_render_state_size(const gr_render_state* s, int* width, int* height) {
    if (!s) return 0;
    if (width) *width = s->width;
    if (height) *height = s->height;
    return 1;
}

void* gr_render_state_buffer(gr_render_state* s, int which) {
    if (!s) return nullptr;
    // whoever holds a pointer to the camera set, the prepass verdicts or the parameters may write through it: the next frame does its
    // own set-up and prepass (reuse_still_camera); ray and render-data records are outputs of every frame
    if (which != GR_BUF_RAYS_IN && which != GR_BUF_RAYS_COUNT && which != GR_BUF_RENDER_DATA && which != GR_BUF_RAYS_ADAPTIVE &&
        which != GR_BUF_RAYS_ADAPTIVE_COUNT)
        s->previous_key_valid = false;
    switch (which) {
        case GR_BUF_RAYS_IN: return s->rays_in;
        case GR_BUF_RAYS_COUNT: return s->rays_count_in;
        case GR_BUF_RENDER_DATA: return s->render_data;
        case GR_BUF_TERMINATION: return s->termination_buffer;
        case GR_BUF_CAMERA_GENERIC: return s->camera_pos_generic;
        case GR_BUF_TETRAD0: return s->tetrad[0];
        case GR_BUF_TETRAD1: return s->tetrad[1];
        case GR_BUF_TETRAD2: return s->tetrad[2];
        case GR_BUF_TETRAD3: return s->tetrad[3];
        case GR_BUF_RAYS_ADAPTIVE: return s->rays_adaptive;
        case GR_BUF_RAYS_ADAPTIVE_COUNT: return s->rays_adaptive_count;
        case GR_BUF_CFG: return s->cfg;
        case GR_BUF_DFG: return s->dfg;
        case GR_BUF_CAMERA_QUAT: return s->camera_quat;
    }
    return nullptr;
}

int gr_render_state_stage_ms(gr_render_state* s, int stage, float* ms) {
    if (!s || !ms || stage < 0 || stage >= GR_STAGE_COUNT) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "bad stage");
    *ms = 0;
    if (!s->stage_timed[stage]) return GR_OK;
    HIP_CHECK(hipEventSynchronize(s->ev_stop[stage]));
    HIP_CHECK(hipEventElapsedTime(ms, s->ev_start[stage], s->ev_stop[stage]));
    return GR_OK;
}

int gr_render_state_trace_log(gr_render_state* s, float* total_ms, int* launches, int reset) {
    if (!s) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipSetDevice(s->device));
    double sum = 0;
    for (size_t i = 0; i < s->trace_log_used; i++) {
        float ms = 0;
        HIP_CHECK(hipEventSynchronize(s->trace_log[i].second));
        HIP_CHECK(hipEventElapsedTime(&ms, s->trace_log[i].first, s->trace_log[i].second));
        sum += ms;
    }
    if (total_ms) *total_ms = (float)sum;
    if (launches) *launches = (int)s->trace_log_used;
    if (reset) s->trace_log_used = 0;
    return GR_OK;
}

int gr_render_state_shader_clock(gr_render_state* s, double* mhz) {
    if (!s || !mhz) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipSetDevice(s->device));
    unsigned long long v[4] = {};
    HIP_CHECK(hipMemcpy(v, s->attempts, 32, hipMemcpyDeviceToHost));
    *mhz = v[2] ? 100.0 * (double)v[1] / (double)v[2] : 0.0;   // cycles per tick of the 100 MHz reference clock
    return GR_OK;
}

int gr_render_state_wave_time(gr_render_state* s, double* wave_ms, unsigned long long* waves) {
    if (!s || !wave_ms || !waves) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipSetDevice(s->device));
    unsigned long long v[4] = {};
    HIP_CHECK(hipMemcpy(v, s->attempts, 32, hipMemcpyDeviceToHost));
    *wave_ms = (double)v[2] * 1e-5;   // ticks of 10 ns
    *waves = v[3];
    return GR_OK;
}

int gr_render_state_counters(gr_render_state* s, unsigned long long* words, int count) {
    if (!s || !words || count < 0 || count > 256) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "counters: up to 256 words");
    HIP_CHECK(hipSetDevice(s->device));
    HIP_CHECK(hipMemcpy(words, s->attempts, (size_t)count * 8, hipMemcpyDeviceToHost));
    return GR_OK;
}

int gr_render_state_attempts(gr_render_state* s, unsigned long long* attempts) {
    if (!s || !attempts) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    HIP_CHECK(hipSetDevice(s->device));
    std::vector<unsigned long long> words(GR_COUNTER_WORDS);
    HIP_CHECK(hipMemcpy(words.data(), s->attempts, words.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long sum = words[0];   // the reference-shaped, pair and compaction kernels count here
    for (int i = 256; i < GR_COUNTER_WORDS; i++) sum += words[i];   // gr_trace_fused: spread over 256 words (kernels/program.hip)
    *attempts = sum;
    return GR_OK;
}

static int ensure_rays(gr_render_state* s, size_t slots, bool adaptive) {
    if (s->ray_capacity < slots) {
        if (s->rays_in) (void)hipFree(s->rays_in);
        if (s->rays_adaptive) (void)hipFree(s->rays_adaptive);
        s->rays_in = s->rays_adaptive = nullptr;
        s->ray_capacity = 0;
        HIP_CHECK(hipMalloc(&s->rays_in, slots * sizeof(gr_lightray)));
        s->ray_capacity = slots;
    }
    if (adaptive && !s->rays_adaptive) HIP_CHECK(hipMalloc(&s->rays_adaptive, s->ray_capacity * sizeof(gr_lightray)));
    return GR_OK;
}

// ---- camera on a timelike geodesic ------------------------------------------------------------------
int gr_geodesic_camera_create(int device, int max_path_length, gr_geodesic_camera** out) {
    if (!out || max_path_length < 2) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "bad geodesic camera size");
    HIP_CHECK(hipSetDevice(device));
    gr_geodesic_camera* g = new gr_geodesic_camera();
    g->device = device;
    g->max_path_length = max_path_length;
    hipError_t e = hipSuccess;
    auto A = [&](void** p, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(p, bytes);
        if (e == hipSuccess) e = hipMemset(*p, 0, bytes);
    };
    size_t n = (size_t)max_path_length;
    A(&g->path, n * 16); A(&g->velocity, n * 16); A(&g->ds, n * 4); A(&g->count, 4);
    for (auto& t : g->transported) A(&t, n * 16);
    A(&g->ray, sizeof(gr_lightray)); A(&g->ray_count, 4); A(&g->basis_speed, 16); A(&g->camera_generic, 16);
    for (auto& t : g->tetrad) A(&t, 16);
    A(&g->interpolated_velocity, 16);
    A(&g->cfg, CFG_MAX * sizeof(float)); A(&g->dfg, sizeof(gr_features));
    if (e == hipSuccess) e = hipDeviceSynchronize();   // (the zeroing above must not overtake the first snapshot: see gr_render_state_create)
    if (e != hipSuccess) {
        gr_geodesic_camera_destroy(g);
        return gr_internal_fail(GR_ERROR_DEVICE, (std::string("geodesic camera allocation: ") + hipGetErrorString(e)).c_str());
    }
    *out = g;
    return GR_OK;
}

void gr_geodesic_camera_destroy(gr_geodesic_camera* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    g->uploads.release();
    void* ptrs[] = {g->path, g->velocity, g->ds, g->count, g->transported[0], g->transported[1], g->transported[2], g->transported[3],
                    g->ray, g->ray_count, g->basis_speed, g->camera_generic, g->tetrad[0], g->tetrad[1], g->tetrad[2], g->tetrad[3],
                    g->interpolated_velocity, g->cfg, g->dfg};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete g;
}

int gr_geodesic_camera_snapshot(gr_geodesic_camera* g, gr_program* p, const gr_metric* m, void* stream_v, const gr_camera* camera,
                                const float geodesic_basis_speed[3], const gr_features* features_in, const float* cfg_values,
                                int num_cfg_values, int* steps_out, float* proper_time_out) {
    if (!g || !p || !m || !camera || !geodesic_basis_speed) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_CHECK(hipSetDevice(g->device));
    gr_metric_info info;
    gr_features features;
    std::vector<float> cfg;
    GR_CHECK(resolve_parameters(m, features_in, cfg_values, num_cfg_values, info, features, cfg));
    float speed4[4] = {geodesic_basis_speed[0], geodesic_basis_speed[1], geodesic_basis_speed[2], 0.f};
    if (speed4[0] * speed4[0] + speed4[1] * speed4[1] + speed4[2] * speed4[2] >= 1.f)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "geodesic basis speed must be below c");
    void* cart = g->interpolated_velocity;   // scratch until the first interpolation
    GR_CHECK(g->uploads.copy(g->cfg, cfg.data(), cfg.size() * sizeof(float), stream));
    GR_CHECK(g->uploads.copy(g->dfg, &features, sizeof(features), stream));
    GR_CHECK(g->uploads.copy(g->basis_speed, speed4, 16, stream));
    GR_CHECK(g->uploads.copy(cart, camera->position, 16, stream));
    HIP_CHECK(hipMemsetAsync(g->count, 0, 4, stream));
    HIP_CHECK(hipMemsetAsync(g->ray_count, 0, 4, stream));
    // main.cpp:2311-2329 (this frame's camera), then :2689-2758
    GR_CHECK(gr_cart_to_generic(p, stream, cart, g->camera_generic, 1, camera->flip, g->cfg));
    GR_CHECK(gr_init_basis_vectors(p, stream, g->camera_generic, 1, camera->basis_speed, g->tetrad[0], g->tetrad[1], g->tetrad[2],
                                   g->tetrad[3], g->cfg));
    GR_CHECK(gr_boost_tetrad(p, stream, g->camera_generic, 1, g->basis_speed, g->tetrad[0], g->tetrad[1], g->tetrad[2], g->tetrad[3],
                             g->cfg));
    GR_CHECK(gr_init_inertial_ray(p, stream, g->camera_generic, 1, g->ray, g->ray_count, g->tetrad[0], g->tetrad[1], g->tetrad[2],
                                  g->tetrad[3], g->basis_speed, g->cfg));
    GR_CHECK(gr_get_geodesic_path(p, stream, g->ray, 1, g->path, g->velocity, g->ds, g->ray_count, g->max_path_length, g->cfg, g->dfg,
                                  g->count));
    for (int i = 0; i < 4; i++)
        GR_CHECK(gr_parallel_transport_quantity(p, stream, g->path, g->velocity, g->ds, g->tetrad[i], g->count, 1, g->transported[i],
                                                g->cfg));
    HIP_CHECK(hipMemcpyAsync(&g->steps, g->count, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    std::vector<float> ds((size_t)std::max(g->steps, 1));
    if (g->steps > 0) HIP_CHECK(hipMemcpy(ds.data(), g->ds, (size_t)g->steps * 4, hipMemcpyDeviceToHost));
    double total = 0;
    for (int i = 0; i + 1 < g->steps; i++) total += ds[i];   // the last sample has no successor (cl.cl:2808-2845)
    g->proper_time = (float)total;
    if (steps_out) *steps_out = g->steps;
    if (proper_time_out) *proper_time_out = g->proper_time;
    return GR_OK;
}

int gr_geodesic_camera_interpolate(gr_geodesic_camera* g, gr_program* p, void* stream_v, float proper_time,
                                   int parallel_transport_observer, float camera_generic_out[4], float tetrad_out[16],
                                   float velocity_out[4]) {
    if (!g || !p) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_CHECK(hipSetDevice(g->device));
    GR_CHECK(gr_handle_interpolating_geodesic(p, stream, g->path, g->velocity, g->ds, g->camera_generic, g->transported[0],
                                              g->transported[1], g->transported[2], g->transported[3], g->tetrad[0], g->tetrad[1],
                                              g->tetrad[2], g->tetrad[3], proper_time, g->count, parallel_transport_observer,
                                              g->basis_speed, g->interpolated_velocity, g->cfg));
    if (camera_generic_out) HIP_CHECK(hipMemcpyAsync(camera_generic_out, g->camera_generic, 16, hipMemcpyDeviceToHost, stream));
    if (velocity_out) HIP_CHECK(hipMemcpyAsync(velocity_out, g->interpolated_velocity, 16, hipMemcpyDeviceToHost, stream));
    if (tetrad_out)
        for (int i = 0; i < 4; i++) HIP_CHECK(hipMemcpyAsync(tetrad_out + 4 * i, g->tetrad[i], 16, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    return GR_OK;
}

void* gr_geodesic_camera_buffer(gr_geodesic_camera* g, int which) {
    if (!g) return nullptr;
    switch (which) {
        case GR_GEOBUF_PATH: return g->path;
        case GR_GEOBUF_VELOCITY: return g->velocity;
        case GR_GEOBUF_DS: return g->ds;
        case GR_GEOBUF_COUNT: return g->count;
        case GR_GEOBUF_TRANSPORTED0: return g->transported[0];
        case GR_GEOBUF_TRANSPORTED1: return g->transported[1];
        case GR_GEOBUF_TRANSPORTED2: return g->transported[2];
        case GR_GEOBUF_TRANSPORTED3: return g->transported[3];
    }
    return nullptr;
}

// What a frame refuses before any HIP call (render_traced_frame, and deliver_frame before it allocates for a factor-1 state).
static int check_frame_arguments(const gr_render_state* s, const gr_program* p, const gr_metric* m, const gr_camera* camera, const float* cfg_values,
                                 int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height, int bg_levels, const void* out) {
    if (!s || !p || !m || !camera) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    // a frame that is to be shaded needs both skies and their shape (the texture pass reads them unchecked: a NULL sky is a device fault,
    // not an error code - tests/test_gpu_lifecycle.py found it); out == NULL stops after the render-data
    if (out && (!bg1 || !bg2 || bg_width <= 0 || bg_height <= 0 || bg_levels <= 0) && !state_has_sky(s))   // (a state with a sky reads no background)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_frame: an output frame needs both background textures and their width, height and levels");
    if (num_cfg_values < 0 || (num_cfg_values > 0 && !cfg_values)) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_frame: cfg_values");
    return GR_OK;
}

// ---- one frame at the state's traced size: render_traced_frame, a sequence of the stages below ---------------------------------
// What the stages share.  Decisions that need no device live in frame_plan.cpp (the fused path's: frame_plan::plan_fused); the stages
// gather their inputs, carry them out, and keep the order of the HIP calls on every stream.
struct frame_context {
    gr_render_state* s; gr_program* p; hipStream_t stream; const gr_camera* camera;
    const void *bg1, *bg2; int bg_width, bg_height, bg_levels;
    void* out;   // float4[s->width * s->height], or NULL: stop after the render-data
    gr_frame_options opt;
    gr_frame_tuning tune;   // which fused kernel, schedule and launch size (geodesic_hip_internal.h; NULL = the defaults)
    gr_features features;
    std::vector<float> cfg;
    int width, height, prepass_width, prepass_height;
    bool use_prepass, adaptive, cfg_changed, cfg_jumped, features_changed, prepass_by_policy;
    bool prefetched = false, repeats_previous_frame = false, reuse_on = false, one_launch_setup = false, log_trace = false;
    const gr_geodesic_camera* gc = nullptr;
    void* attempts = nullptr;
    // fused mode
    frame_plan::fused_plan plan;
    struct request { const gr_camera* camera; float time; int strip_rank; };   // strip_rank < 0: this frame's
    std::vector<request> todo;   // look-ahead requests that are not already sitting in a slot
    bool claimed[gr_render_state::LOOKAHEAD] = {};   // a slot serves one request (two frames may share one camera)

    int begin(int st) {
        if (log_trace) { if (st == GR_STAGE_TRACE) HIP_CHECK(hipEventRecord(s->trace_log[s->trace_log_used].first, stream)); }
        else if (opt.time_kernels) { HIP_CHECK(hipEventRecord(s->ev_start[st], stream)); }
        return GR_OK;
    }
    int end(int st) {
        if (log_trace) { if (st == GR_STAGE_TRACE) { HIP_CHECK(hipEventRecord(s->trace_log[s->trace_log_used].second, stream)); s->trace_log_used++; } }
        else if (opt.time_kernels) { HIP_CHECK(hipEventRecord(s->ev_stop[st], stream)); s->stage_timed[st] = true; }
        return GR_OK;
    }
    gr_render_state::prefetch_key make_key(const gr_camera* c, float time, int frame_strip_rank) const {
        gr_render_state::prefetch_key k;
        k.camera = *c;
        k.cfg = cfg;
        k.features = features;
        k.program = gr_program_serial(p);
        k.geodesic = (const void*)opt.geodesic;
        k.geodesic_time = time;
        k.transport = opt.parallel_transport_observer;
        k.strip[2] = opt.strip_count > 1 ? opt.strip_count : 1;
        k.strip[1] = k.strip[2] > 1 ? frame_strip_rank : 0;
        k.strip[0] = k.strip[2] > 1 ? opt.block_rows : 0;
        return k;
    }
    gr_render_state::prefetch_key own_key() const { return make_key(camera, opt.geodesic_time, opt.strip_rank); }
    // camera position and tetrad: from the cartesian camera (main.cpp:2311, 2329), or - camera on a geodesic - interpolated
    // from the snapshot at the requested proper time (main.cpp:2264-2293)
    int camera_setup(hipStream_t st, void* cart, void* generic, void* const* tetrad, const gr_camera* cam, float time, void* velocity_out) const {
        if (gc)
            return gr_handle_interpolating_geodesic(p, st, gc->path, gc->velocity, gc->ds, generic, gc->transported[0], gc->transported[1],
                                                    gc->transported[2], gc->transported[3], tetrad[0], tetrad[1], tetrad[2], tetrad[3],
                                                    time, gc->count, opt.parallel_transport_observer, gc->basis_speed, velocity_out,
                                                    s->cfg);
        GR_CHECK(gr_cart_to_generic(p, st, cart, generic, 1, cam->flip, s->cfg));
        return gr_init_basis_vectors(p, st, generic, 1, cam->basis_speed, tetrad[0], tetrad[1], tetrad[2], tetrad[3], s->cfg);
    }
    // the prepass verdicts a trace or ray set-up reads, and their grid (without a prepass: none, and the image's own size)
    const void* verdicts() const { return use_prepass ? s->termination_buffer : nullptr; }
    int grid_width() const { return use_prepass ? prepass_width : width; }
    int grid_height() const { return use_prepass ? prepass_height : height; }
    // The prepass rays' costs are kept behind the prepass flags in the termination buffer, which is allocated per pixel
    void* cost_plane(void* termination_buffer) const { return plan.order_capable ? (void*)((unsigned int*)termination_buffer + plan.cells) : nullptr; }
    // are costs left by an earlier frame (same program, parameters within a step of a slider) still those of this picture, give or take max_motion px?
    bool picture_kept(unsigned long long program_then, const gr_camera& camera_then, float max_motion) const {
        return !cfg_jumped && !features_changed && program_then == gr_program_serial(p) &&
               picture_motion(camera_then, *camera, features.field_of_view, width) <= max_motion;
    }
};

// options, tuning, features and $cfg values of this frame
static int resolve_inputs(frame_context& f, const gr_metric* m, const gr_features* features_in, const float* cfg_values, int num_cfg_values,
                          const gr_frame_options* opt_in) {
    gr_frame_options_default(&f.opt);
    if (opt_in) f.opt = *opt_in;
    gr_frame_tuning_default(&f.tune);
    if (f.opt.tuning) f.tune = *f.opt.tuning;
    f.width = f.s->width; f.height = f.s->height;
    gr_metric_info info;
    GR_CHECK(resolve_parameters(m, features_in, cfg_values, num_cfg_values, info, f.features, f.cfg));
    // The defaults of gr_features (adaptive_sampling on, as the reference's GUI) and of gr_frame_options (fused mode) work
    // together: a frame is sampled adaptively on the fused path (half-resolution lattice, gr_adaptive_refine, second fused
    // launch over the marked pixels; cl.cl:3234-3250, 5223-5345) - a device's share of a split frame too: it traces the lattice
    // rows its blocks' decisions read (two rows of halo either side) and its rows come out as those of the whole frame.
    f.use_prepass = f.opt.use_prepass < 0 ? info.use_prepass != 0 : f.opt.use_prepass != 0;
    f.adaptive = f.features.adaptive_sampling != 0 && !f.features.use_triangle_rendering;
    // The 2x2 blocks of handle_adaptive_sampling cover 2 (W/2) x 2 (H/2) pixels (cl.cl:5228-5236): with an odd width or height the
    // last column or row belongs to no block and would keep whatever its record held.  The fused path then traces every pixel.
    if (f.opt.mode == GR_MODE_FUSED && ((f.width | f.height) & 1)) f.adaptive = false;
    return GR_OK;
}

// what changed since the state's last frame, and what that invalidates
static void note_parameter_changes(frame_context& f) {
    gr_render_state* s = f.s;
    f.cfg_changed = f.cfg != s->host_cfg;
    // ... by a step of a slider (every parameter within a tenth of itself): the picture is nearly the one before, and what its tiles cost is
    // still the best estimate there is of what they cost now - orders are only orders, a wrong one costs time, never a record.  A frame of a
    // slider being dragged (the dynamic program, new parameters every frame: metric_manager.hpp:60-66) would otherwise start from image
    // order every time (4K Kerr: 6.0 ms against 5.1).
    f.cfg_jumped = f.cfg_changed && [&] {
        if (f.cfg.size() != s->host_cfg.size()) return true;
        for (size_t i = 0; i < f.cfg.size(); i++) {
            const float a = f.cfg[i], b = s->host_cfg[i];
            if (!(std::fabs(a - b) <= 0.1f * std::max(std::max(std::fabs(a), std::fabs(b)), 0.05f))) return true;
        }
        return false;
    }();
    f.features_changed = !s->features_valid || memcmp(&f.features, &s->host_features, sizeof(f.features)) != 0;
    // another metric, parameter set or field of view: what the last frame's tiles cost says nothing about this one's (tile_history)
    if (f.cfg_jumped || f.features_changed || gr_program_serial(f.p) != s->tile_cost_program) {
        s->tile_cost_valid = false;
        s->tile_cost_program = gr_program_serial(f.p);
    }
}

// use_prepass = -2: does this frame run its prepass (gr_render_state::prepass_policy)?
static int apply_prepass_policy(frame_context& f) {
    gr_render_state* s = f.s;
    f.prepass_by_policy = f.opt.use_prepass == -2 && f.use_prepass && f.opt.mode == GR_MODE_FUSED && f.opt.strip_count <= 1;
    if (!f.prepass_by_policy) return GR_OK;
    auto& pol = s->policy;
    const unsigned long long serial = gr_program_serial(f.p);
    if (f.cfg_changed || f.features_changed || serial != s->policy_program) {   // another metric or parameter set: start over
        pol.holiday = 0;
        pol.last_fraction = -1.f;
        if (pol.in_flight) { HIP_CHECK(hipEventSynchronize(pol.copied)); pol.in_flight = false; }
        s->policy_program = serial;
    }
    if (pol.in_flight && hipEventQuery(pol.copied) == hipSuccess) {
        // the share of the grid whose 5-point stencil is marked throughout: what init_rays_generic's test lets the trace skip
        // (a pixel is skipped when the cell it rounds to and that cell's four neighbours are all marked, cl.cl:3213-3232)
        size_t skippable = 0;
        const int pw = pol.grid_width, ph = pol.cells && pw ? (int)(pol.cells / pw) : 0;
        for (int y = 1; y + 1 < ph; y++)
            for (int x = 1; x + 1 < pw; x++) {
                const int* c = pol.host_flags + (size_t)y * pw + x;
                skippable += c[0] == 1 && c[-1] == 1 && c[1] == 1 && c[-pw] == 1 && c[pw] == 1;
            }
        pol.last_fraction = pol.cells ? (float)skippable / (float)pol.cells : 0.f;
        pol.in_flight = false;
        if (pol.last_fraction < gr_render_state::PREPASS_MIN_SKIP) pol.holiday = gr_render_state::PREPASS_HOLIDAY;
    } else if (pol.in_flight) {
        (void)hipGetLastError();   // hipErrorNotReady is not an error
    }
    if (pol.holiday > 0) { pol.holiday--; pol.without_prepass++; f.use_prepass = false; }
    else pol.with_prepass++;
    return GR_OK;
}

// ... its flags -> host, behind the prepass on the frame's stream; read when a later frame finds them there
static int inspect_prepass(frame_context& f) {
    gr_render_state* s = f.s;
    auto& pol = s->policy;
    const size_t cells = f.plan.cells;
    if (!(f.prepass_by_policy && f.use_prepass && !pol.in_flight)) return GR_OK;
    if (pol.capacity < cells) {
        if (pol.host_flags) (void)hipHostFree(pol.host_flags);
        pol.host_flags = nullptr;
        HIP_CHECK(hipHostMalloc((void**)&pol.host_flags, cells * sizeof(int), hipHostMallocDefault));
        pol.capacity = cells;
    }
    if (!pol.copied) HIP_CHECK(hipEventCreateWithFlags(&pol.copied, hipEventDisableTiming));
    HIP_CHECK(hipMemcpyAsync(pol.host_flags, s->termination_buffer, cells * sizeof(int), hipMemcpyDeviceToHost, f.stream));
    HIP_CHECK(hipEventRecord(pol.copied, f.stream));
    pol.cells = cells;
    pol.grid_width = f.prepass_width;
    pol.in_flight = true;
    return GR_OK;
}

// new parameters go to the device, behind the look-ahead prepasses that still read the old ones
static int upload_parameters(frame_context& f) {
    gr_render_state* s = f.s;
    if (f.cfg_changed || f.features_changed) {
        // Look-ahead prepasses read s->cfg / s->dfg on their side streams: the upload below must not overtake one that is still
        // running (it would read a mix of old and new parameters), and what the slots hold was computed for the old parameters.
        for (auto& slot : s->pre) {
            if (!slot.valid) continue;
            HIP_CHECK(hipStreamWaitEvent(f.stream, slot.ready, 0));
            slot.valid = false;
        }
    }
    if (f.cfg_changed) {
        GR_CHECK(s->uploads.copy(s->cfg, f.cfg.data(), f.cfg.size() * sizeof(float), f.stream));
        s->host_cfg = f.cfg;
    }
    if (f.features_changed) {
        GR_CHECK(s->uploads.copy(s->dfg, &f.features, sizeof(f.features), f.stream));
        s->host_features = f.features;
        s->features_valid = true;
    }
    return GR_OK;
}

// Was this frame's camera set-up + prepass already done - on a side stream during an earlier frame, or by the previous frame?
static int take_prepared_setup(frame_context& f) {
    gr_render_state* s = f.s;
    const gr_frame_options& opt = f.opt;
    f.prepass_width = f.width / 16; f.prepass_height = f.height / 16;   // main.cpp:2380-2381
    if (f.prepass_width < 1 || f.prepass_height < 1) f.use_prepass = false;
    s->frame_counter++;
    if (opt.mode == GR_MODE_FUSED && f.use_prepass) {
        const auto want = f.own_key();
        gr_render_state::prefetch_slot* hit = nullptr;   // the oldest matching prefetch: it has had the most time to finish
        for (auto& slot : s->pre)
            if (slot.valid && slot.key == want && (!hit || slot.age < hit->age)) hit = &slot;
        if (hit) {
            s->swap_in(hit->set);
            HIP_CHECK(hipStreamWaitEvent(f.stream, hit->ready, 0));
            hit->valid = false;
            f.prefetched = true;
        }
    }
    // ... or is it the previous frame of this state over again - camera, parameters, features, program, bit for bit, on the same stream
    // (gr_frame_tuning.reuse_still_camera)?  Camera position, tetrad and the prepass verdicts are functions of exactly those, and they are
    // where that frame left them: a viewer whose user has stopped moving pays neither again (the reference does, every frame:
    // main.cpp:2311-2437).  Whole frames with a Cartesian camera whose tiles are not ordered by the prepass rays' costs.
    const int tile_order_mode = switches::tile_order();
    const bool reuse_default = switches::reuse_still_camera();
    f.repeats_previous_frame = opt.mode == GR_MODE_FUSED && f.use_prepass && !opt.geodesic && opt.strip_count <= 1 && s->previous_key_valid &&
                               s->previous_key == f.own_key();
    f.reuse_on = (f.tune.reuse_still_camera < 0 ? reuse_default : f.tune.reuse_still_camera != 0) && tile_order_mode != 1;
    if (!f.prefetched && f.repeats_previous_frame && f.reuse_on && s->previous_stream == f.stream) {
        f.prefetched = true;
        s->prepass_reused++;
    }
    s->previous_key_valid = false;   // until this frame has left its own set-up and prepass behind
    if (!f.prefetched) {
        GR_CHECK(s->uploads.copy(s->camera_pos_cart, f.camera->position, 16, f.stream));
        GR_CHECK(s->uploads.copy(s->camera_quat, f.camera->quat, 16, f.stream));
    }
    return GR_OK;
}

// timers and counters of this frame, and the camera set-up where it is a launch of its own
static int begin_frame(frame_context& f) {
    gr_render_state* s = f.s;
    for (int i = 0; i < GR_STAGE_COUNT; i++) s->stage_timed[i] = false;
    f.log_trace = f.opt.time_kernels == 2;
    if (f.log_trace && s->trace_log_used == s->trace_log.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        s->trace_log.emplace_back(a, b);
    }
    if (f.tune.count_attempts) {
        HIP_CHECK(hipMemsetAsync(s->attempts, 0, GR_COUNTER_WORDS * 8, f.stream));
        f.attempts = s->attempts;
    }
    f.gc = f.opt.geodesic;
    if (f.gc && f.gc->device != s->device) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "geodesic camera lives on another device");
    // fused mode with a Cartesian camera: camera set-up and prepass are one call (gr_camera_prepass), issued by fused_setup_and_prepass
    f.one_launch_setup = f.opt.mode == GR_MODE_FUSED && !f.gc;
    if (!f.prefetched && !f.one_launch_setup) {
        GR_CHECK(f.begin(GR_STAGE_CAMERA));
        GR_CHECK(f.camera_setup(f.stream, s->camera_pos_cart, s->camera_pos_generic, s->tetrad, f.camera, f.opt.geodesic_time,
                                f.gc ? f.gc->interpolated_velocity : nullptr));
        GR_CHECK(f.end(GR_STAGE_CAMERA));
    }
    return GR_OK;
}

// ---- the fused path ------------------------------------------------------------------------------------------------------------
// frame_plan::plan_fused's inputs from the frame, the program and the state; its refusal, and the one write it asks for
static int fused_plan_frame(frame_context& f) {
    gr_render_state* s = f.s;
    frame_plan::fused_input in;
    in.width = f.width; in.height = f.height;
    in.strip_count = f.opt.strip_count; in.strip_rank = f.opt.strip_rank; in.block_rows = f.opt.block_rows;
    in.adaptive = f.adaptive; in.use_prepass = f.use_prepass; in.prefetched = f.prefetched; in.geodesic = f.gc != nullptr; in.out = f.out != nullptr;
    in.tune = f.tune;
    in.has_pair = gr_program_has_trace_pair(f.p) != 0; in.has_parking = gr_program_has_parking(f.p) != 0;
    in.has_tile_shading = gr_program_has_tile_shading(f.p) != 0;
    in.wave_slots = [&] { return gr_trace_fused_wave_slots(f.p); };
    in.tile_order_bytes = gr_tile_order_bytes;
    in.earlier_frame_still_running = [&] { return earlier_frame_still_running(s->device, f.stream); };
    in.tile_order_bytes_held = s->tile_order_bytes;
    in.tile_cost_valid = s->tile_cost_valid; in.tile_cost_anchored = s->tile_cost_anchored;
    memcpy(in.tile_cost_shape, s->tile_cost_shape, sizeof(in.tile_cost_shape));
    in.tile_cost_camera = s->tile_cost_camera; in.camera = *f.camera;
    in.field_of_view = f.features.field_of_view;
    f.plan = frame_plan::plan_fused(in);
    if (f.plan.refused.code != GR_OK) return gr_internal_fail(f.plan.refused.code, f.plan.refused.message);
    if (f.plan.invalidate_tile_cost) s->tile_cost_valid = false;
    // a frame with an analytic sky is shaded by fused_shade's one launch: the trace has no textures to shade tiles from
    if (s->sky_set || s->stars_set) f.plan.shade_in_trace = false;
    return GR_OK;
}

// camera set-up and prepass of one frame on one stream into one buffer set (this frame's, or a look-ahead slot's), and the order its costs give
static int fused_setup_and_prepass(frame_context& f, hipStream_t stream, const gr_render_state::camera_set& set, const gr_camera* cam, float time,
                                   int strip_rank, void* velocity, bool prepass_in_front, bool order_tiles) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    void* const costs = f.cost_plane(set.termination_buffer);
    if (f.one_launch_setup) {
        GR_CHECK(gr_camera_prepass(f.p, stream, set.camera_pos_cart, cam->flip, cam->basis_speed, set.camera_pos_generic, set.tetrad[0], set.tetrad[1],
                                   set.tetrad[2], set.tetrad[3], set.camera_quat, set.termination_buffer, prepass_in_front ? f.prepass_width : 0,
                                   prepass_in_front ? f.prepass_height : 0, s->cfg, s->dfg, f.height, q.block_rows, strip_rank, q.strip_count, costs,
                                   q.prepass_margin));
    } else {
        if (velocity) GR_CHECK(f.camera_setup(stream, set.camera_pos_cart, set.camera_pos_generic, set.tetrad, cam, time, velocity));
        GR_CHECK(gr_prepass_fused_strips(f.p, stream, set.camera_pos_generic, set.camera_quat, set.termination_buffer, f.prepass_width, f.prepass_height,
                                         set.tetrad[0], set.tetrad[1], set.tetrad[2], set.tetrad[3], s->cfg, s->dfg, f.height, q.block_rows, strip_rank,
                                         q.strip_count, costs, q.prepass_margin));
    }
    if (order_tiles)
        GR_CHECK(gr_order_tiles(f.p, stream, set.termination_buffer, costs, f.prepass_width, f.prepass_height, f.width, f.height, q.block_rows,
                                strip_rank, q.strip_count, set.tile_order));
    return GR_OK;
}

// this frame's own, unless it was prepared (take_prepared_setup); a camera on a geodesic was set up by begin_frame
static int fused_own_setup(frame_context& f) {
    gr_render_state* s = f.s;
    if (f.prefetched || !(f.one_launch_setup || f.use_prepass)) return GR_OK;
    gr_render_state::camera_set own;
    own.camera_pos_cart = s->camera_pos_cart; own.camera_quat = s->camera_quat; own.camera_pos_generic = s->camera_pos_generic;
    for (int i = 0; i < 4; i++) own.tetrad[i] = s->tetrad[i];
    own.termination_buffer = s->termination_buffer; own.tile_order = s->tile_order;
    GR_CHECK(f.begin(GR_STAGE_PREPASS));
    GR_CHECK(fused_setup_and_prepass(f, f.stream, own, f.camera, f.opt.geodesic_time, f.plan.strip_rank, nullptr, f.use_prepass && !f.plan.inline_prepass,
                                     f.plan.order_tiles));
    return f.end(GR_STAGE_PREPASS);
}

// the look-ahead requests (gr_frame_options.next_camera / next_camera2) that are not already sitting in a slot
static int fused_collect_look_ahead(frame_context& f) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    if (f.use_prepass) {
        frame_context::request asked[2] = {{f.opt.next_camera, f.tune.next_geodesic_time, f.tune.next_strip_rank},
                                           {f.opt.next_camera2, f.tune.next_geodesic_time2, f.tune.next_strip_rank2}};
        // nobody announced the next camera, and this frame is the previous one over again: the guess "the same once more"
        // (gr_frame_tuning.guess_still_camera, off by default since reuse_still_camera does without the prepass altogether) - used
        // by the next frame only if its key matches bit for bit
        const bool guess_default = switches::guess_still_camera();
        if (!f.opt.next_camera && !f.opt.next_camera2 && !f.gc && q.strip_count == 1 && (f.tune.guess_still_camera < 0 ? guess_default : f.tune.guess_still_camera != 0) &&
            f.repeats_previous_frame && !f.reuse_on)
            asked[0] = {f.camera, f.opt.geodesic_time, -1};
        for (auto& r : asked) {
            if (!r.camera) continue;
            if (r.strip_rank < 0 || r.strip_rank >= q.strip_count) r.strip_rank = q.strip_rank;
            const auto k = f.make_key(r.camera, r.time, r.strip_rank);
            bool have = false;
            for (int i = 0; i < gr_render_state::LOOKAHEAD && !have; i++)
                if (!f.claimed[i] && s->pre[i].valid && s->pre[i].key == k) f.claimed[i] = have = true;
            if (!have) f.todo.push_back(r);
        }
    }
    if (!f.todo.empty()) HIP_CHECK(hipEventRecord(s->main_mark, f.stream));   // everything up to here is older than the prefetches
    return GR_OK;
}

// ... each on a side stream, into a slot's buffer set, while this frame traces
static int fused_submit_look_ahead(frame_context& f) {
    gr_render_state* s = f.s;
    for (const auto& r : f.todo) {
        // a free slot, else the stalest one no current request claims (a camera that was announced but never came)
        int chosen = -1;
        for (int i = 0; i < gr_render_state::LOOKAHEAD; i++)
            if (!f.claimed[i] && (chosen < 0 || (!s->pre[i].valid && s->pre[chosen].valid) ||
                                  (s->pre[i].valid == s->pre[chosen].valid && s->pre[i].age < s->pre[chosen].age)))
                chosen = i;
        if (chosen < 0) break;
        gr_render_state::prefetch_slot* slot = &s->pre[chosen];
        f.claimed[chosen] = true;
        // camera set-up and prepass on the slot's stream, into the slot's buffer set, while the trace runs.  The set may
        // have belonged to the previous frame (swapped out above): the stream first waits for everything the caller's
        // stream had queued before this frame's trace.
        HIP_CHECK(hipStreamWaitEvent(slot->stream, s->main_mark, 0));
        GR_CHECK(s->uploads.copy(slot->set.camera_pos_cart, r.camera->position, 16, slot->stream));
        GR_CHECK(s->uploads.copy(slot->set.camera_quat, r.camera->quat, 16, slot->stream));
        // (the look-ahead frame's order too: off the frame's critical path like its prepass)
        GR_CHECK(fused_setup_and_prepass(f, slot->stream, slot->set, r.camera, r.time, r.strip_rank, slot->velocity, true, f.plan.order_capable));
        HIP_CHECK(hipEventRecord(slot->ready, slot->stream));
        slot->valid = true;
        slot->age = s->frame_counter;
        slot->key = f.make_key(r.camera, r.time, r.strip_rank);
    }
    return GR_OK;
}

// what every launch of gr_trace_fused of this frame is given
static gr_trace_fused_args fused_trace_args(const frame_context& f) {
    const gr_render_state* s = f.s;
    gr_trace_fused_args a{};
    a.camera_generic = s->camera_pos_generic; a.camera_quat = s->camera_quat; a.render_data = s->render_data;
    a.width = f.width; a.height = f.height; a.block_rows = f.plan.block_rows; a.strip_rank = f.plan.strip_rank; a.strip_count = f.plan.strip_count;
    a.termination_buffer = f.verdicts(); a.prepass_width = f.grid_width(); a.prepass_height = f.grid_height();
    a.e0 = s->tetrad[0]; a.e1 = s->tetrad[1]; a.e2 = s->tetrad[2]; a.e3 = s->tetrad[3]; a.cfg = s->cfg; a.dfg = s->dfg;
    a.attempt_counter = f.attempts;
    a.waves_per_simd = f.tune.trace_waves_per_simd;
    a.inline_prepass = f.plan.inline_prepass ? 1 : 0;
    return a;
}

// the order of the frame before's costs and the record of this frame's, for the launch that traces the frame's tiles
// (gr_trace_fused on every pixel, or the lattice launch of adaptive sampling: tiles of 8 x 8 lattice pixels = 16 x 16 pixels)
static int follow_and_record_history(frame_context& f, gr_trace_fused_args& a) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    float anchor[2] = {0, 0};
    const bool anchored = q.record_history && !f.gc && origin_on_screen(*f.camera, f.features.field_of_view, f.width, f.height, anchor);
    if (q.history_order) {
        // how far the picture has moved since the costs were recorded, in tiles
        int shift[2] = {0, 0};
        if (switches::tile_history_follow() && anchored && s->tile_cost_anchored)
            for (int i = 0; i < 2; i++)
                shift[i] = (int)std::lround(std::max(-4096.f, std::min(4096.f, (anchor[i] - s->tile_cost_anchor[i]) / (f.adaptive ? 16.f : 8.f))));
        GR_CHECK(gr_order_tiles_by_history(f.p, f.stream, s->tile_cost, q.hist_width, q.hist_height, q.hist_block_rows, q.strip_rank, q.strip_count,
                                           s->tile_order, shift[0], shift[1]));
        s->history_followed++;
        s->history_last_shift[0] = shift[0]; s->history_last_shift[1] = shift[1];
        a.tile_order = s->tile_order;
        a.tile_order_by_history = 1;
        a.speculative_classes = f.tune.speculative_classes < 0 ? 0 : f.tune.speculative_classes == 0 ? -1 : f.tune.speculative_classes;
    }
    if (q.record_history) {
        a.tile_cost = s->tile_cost;
        s->history_recorded++;
        memcpy(s->tile_cost_shape, q.shape, sizeof(q.shape));
        s->tile_cost_valid = true;
        s->tile_cost_anchored = anchored;
        s->tile_cost_anchor[0] = anchor[0]; s->tile_cost_anchor[1] = anchor[1];
        s->tile_cost_camera = *f.camera;
    }
    return GR_OK;
}

// every pixel, one ray per lane: gr_trace_fused, with parking and in-tile shading where the plan has them
static int fused_trace_full(frame_context& f) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    gr_trace_fused_args a = fused_trace_args(f);
    a.tile_order = q.order_tiles ? s->tile_order : nullptr;
    GR_CHECK(follow_and_record_history(f, a));
    if (q.refused_at_trace.code != GR_OK) return gr_internal_fail(q.refused_at_trace.code, q.refused_at_trace.message);
    // parking (gr_trace_fused_parking): the lot is the state's, allocated the first time a frame asks for it - room for an
    // eighth of the frame's rays (a = 0.9 at 4K parks 4 % of them, re-parked ones counted again; a full lot is not an error)
    if (q.parking) {
        const int slots = (int)std::min<long long>(1 << 24, std::max<long long>(65536, (long long)f.width * f.height / 8));
        if (!s->parking_records || s->parking_slots != slots) {
            if (s->parking_records) (void)hipFree(s->parking_records);
            if (s->parking_words) (void)hipFree(s->parking_words);
            s->parking_records = s->parking_words = nullptr;
            size_t words_bytes = 0;
            const size_t bytes = gr_parking_lot_bytes(slots, slots, &words_bytes);
            HIP_CHECK(hipMalloc(&s->parking_records, bytes));
            HIP_CHECK(hipMalloc(&s->parking_words, words_bytes));
            s->parking_slots = slots;
        }
        a.parking.records = s->parking_records; a.parking.words = s->parking_words;
        a.parking.lanes = std::min(q.park_lanes, 64); a.parking.trips = q.park_trips;
        a.parking.slots = slots; a.parking.groups = slots;
    }
    // the trace shades the pixels whose filter neighbours are in their own tile; gr_render_seams (fused_shade) does the rest
    if (q.shade_in_trace) {
        a.shading.out = f.out; a.shading.background1 = f.bg1; a.shading.background2 = f.bg2; a.shading.bg_width = f.bg_width;
        a.shading.bg_height = f.bg_height; a.shading.bg_levels = f.bg_levels; a.shading.max_probes = f.opt.max_probes;
        a.shading.compact_out = q.strip_count > 1 ? f.opt.compact_out : 0;
    }
    return gr_trace_fused_launch(f.p, f.stream, &a);
}

// adaptive sampling: a quarter of the primary rays (the pixels (2x, 2y)), then the blocks that need it refined by a second launch
static int fused_trace_adaptive(frame_context& f) {
    gr_render_state* s = f.s;
    gr_program* p = f.p;
    hipStream_t stream = f.stream;
    const auto& q = f.plan;
    const int width = f.width, height = f.height;
    gr_trace_fused_args a = fused_trace_args(f);
    a.lattice = 2;
    if (!s->lattice_rays) HIP_CHECK(hipMalloc(&s->lattice_rays, gr_lattice_rays_bytes(width, height)));
    if (!s->pending_list) HIP_CHECK(hipMalloc(&s->pending_list, gr_pending_list_bytes(width, height)));
    a.lattice_rays = s->lattice_rays;
    GR_CHECK(follow_and_record_history(f, a));
    // Tracing ahead what the second launch will ask for (gr_apply_guessed): where the frame before's second launch found pixels of
    // 4 096 attempts and more (program.hip GR_GUESSED_ATTEMPTS), this frame's lattice launch traces the same pixels beside its
    // tiles.  Whole frames that find the device idle (GR_ADAPTIVE_GUESS=0: never).
    const float guess_max_motion = switches::adaptive_guess_max_motion();
    const bool keep_guesses = q.guesses_wanted && !q.device_busy;
    if (keep_guesses && !s->guessed[0])
        for (void*& g : s->guessed) { HIP_CHECK(hipMalloc(&g, gr_guessed_bytes())); HIP_CHECK(hipMemsetAsync(g, 0, 32, stream)); }
    const bool use_guesses = keep_guesses && s->guessed_valid && s->block_cost_valid && f.picture_kept(s->block_cost_program, s->block_cost_camera, guess_max_motion);
    if (keep_guesses && !use_guesses) HIP_CHECK(hipMemsetAsync(s->guessed[0], 0, 4, stream));   // (whatever is there is not for this picture)
    a.guessed = keep_guesses ? s->guessed[0] : nullptr;
    GR_CHECK(gr_trace_fused_launch(p, stream, &a));
    a.tile_order = nullptr; a.tile_order_by_history = 0; a.tile_cost = nullptr;   // (the second launch below is not the lattice's)
    GR_CHECK(f.end(GR_STAGE_TRACE));
    GR_CHECK(f.begin(GR_STAGE_ADAPTIVE));
    HIP_CHECK(hipMemsetAsync(s->rays_adaptive_count, 0, 4, stream));
    // the decisions, the marked pixels as a list ordered dearest first, and the second launch over that list: every lane
    // of every wave has a ray (GR_ADAPTIVE_PENDING_LIST=0: the marked pixels found by walking the image's tiles again)
    if (switches::adaptive_pending_list()) {
        // the list's order: what the lattice rays around a block cost, and - while the picture has moved little since - what
        // the block's own rays cost in this state's frame before (the long rays are filaments a pixel or two wide)
        const float history_max_motion = switches::adaptive_history_max_motion();
        const size_t image_blocks = (size_t)(width / 2) * (height / 2);
        std::swap(s->block_cost, s->block_cost_before);
        if (!s->block_cost) HIP_CHECK(hipMalloc(&s->block_cost, image_blocks * sizeof(unsigned int)));
        const bool by_history = q.strip_count == 1 && s->block_cost_valid && s->block_cost_before && !f.gc &&
                                f.picture_kept(s->block_cost_program, s->block_cost_camera, history_max_motion);
        HIP_CHECK(hipMemsetAsync(s->block_cost, 0, image_blocks * sizeof(unsigned int), stream));
        GR_CHECK(gr_adaptive_refine_list(p, stream, s->render_data, s->rays_adaptive_count, width, height, s->dfg, q.block_rows, q.strip_rank,
                                         q.strip_count, s->lattice_rays, s->cfg, s->pending_list, by_history ? s->block_cost_before : nullptr));
        if (keep_guesses) {
            HIP_CHECK(hipMemsetAsync(s->guessed[1], 0, 4, stream));
            GR_CHECK(gr_apply_guessed(p, stream, s->render_data, width, s->guessed[0], s->guessed[1], s->block_cost, f.attempts));
        }
        GR_CHECK(gr_trace_pending(p, stream, s->camera_pos_generic, s->camera_quat, s->render_data, width, height, s->tetrad[0],
                                  s->tetrad[1], s->tetrad[2], s->tetrad[3], s->cfg, s->dfg, f.attempts, s->pending_list,
                                  f.tune.trace_waves_per_simd, s->block_cost, keep_guesses ? s->guessed[1] : nullptr));
        if (keep_guesses) std::swap(s->guessed[0], s->guessed[1]);
        s->guessed_valid = keep_guesses;
        s->block_cost_valid = q.strip_count == 1;
        s->block_cost_program = gr_program_serial(p);
        s->block_cost_camera = *f.camera;
    } else {
        s->block_cost_valid = false;
        s->guessed_valid = false;
        GR_CHECK(gr_adaptive_refine_strips(p, stream, s->render_data, s->rays_adaptive_count, width, height, s->dfg, q.block_rows,
                                           q.strip_rank, q.strip_count, s->lattice_rays, s->cfg));
        a.lattice = 1;
        a.pending_only = 1;
        a.inline_prepass = 0;
        GR_CHECK(gr_trace_fused_launch(p, stream, &a));
    }
    return f.end(GR_STAGE_ADAPTIVE);
}

// every device runs the (tiny) prepass itself; its own row blocks (+ one halo row each) are traced here, by the kernel the plan names
static int fused_trace(frame_context& f) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    GR_CHECK(f.begin(GR_STAGE_TRACE));
    if (q.keep_lanes > 0)
        GR_CHECK(gr_trace_compact(f.p, f.stream, s->camera_pos_generic, s->camera_quat, s->render_data, f.width, f.height, q.block_rows, q.strip_rank,
                                  q.strip_count, f.verdicts(), f.grid_width(), f.grid_height(), s->tetrad[0], s->tetrad[1], s->tetrad[2], s->tetrad[3],
                                  s->cfg, s->dfg, f.attempts, q.keep_lanes));
    else if (f.adaptive)
        return fused_trace_adaptive(f);   // (ends GR_STAGE_TRACE behind its lattice launch)
    else if (q.rays_per_lane == 2)
        GR_CHECK(gr_trace_pair(f.p, f.stream, s->camera_pos_generic, s->camera_quat, s->render_data, f.width, f.height, q.block_rows, q.strip_rank,
                               q.strip_count, f.verdicts(), f.grid_width(), f.grid_height(), s->tetrad[0], s->tetrad[1], s->tetrad[2], s->tetrad[3],
                               s->cfg, s->dfg, f.attempts));
    else
        GR_CHECK(fused_trace_full(f));
    return f.end(GR_STAGE_TRACE);
}

// f.out shaded from the state's records by the sky the state carries - stars, the analytic sky, else the texture (the setters refuse
// two at once): the whole frame off the counted records (the reference-shaped sequence), or this device's strips of a fused frame
static int shade_frame(frame_context& f, bool whole_frame) {
    gr_render_state* s = f.s;
    const auto& q = f.plan;
    const int count = f.width * f.height, block_rows = q.strip_count > 1 ? q.block_rows : f.height;
    const int compact_out = q.strip_count > 1 ? f.opt.compact_out : 0;
    if (s->stars_set)
        return whole_frame ? gr_render_stars(f.p, f.stream, s->render_data, s->render_data_count, count, f.out, &s->star_sky, s->near_stars, s->far_stars,
                                             f.width, f.height, s->cfg, s->dfg)
                           : gr_render_stars_strips(f.p, f.stream, s->render_data, f.out, &s->star_sky, s->near_stars, s->far_stars, f.width, f.height,
                                                    block_rows, q.strip_rank, q.strip_count, compact_out, s->cfg, s->dfg);
    if (s->sky_set)
        return whole_frame ? gr_render_analytic(f.p, f.stream, s->render_data, s->render_data_count, count, f.out, &s->sky, f.width, f.height, s->cfg, s->dfg)
                           : gr_render_analytic_strips(f.p, f.stream, s->render_data, f.out, &s->sky, f.width, f.height, block_rows, q.strip_rank,
                                                       q.strip_count, compact_out, s->cfg, s->dfg);
    if (whole_frame)
        return gr_render(f.p, f.stream, s->render_data, s->render_data_count, count, f.out, f.bg1, f.bg2, f.bg_width, f.bg_height, f.bg_levels, f.width,
                         f.height, f.opt.max_probes, s->cfg, s->dfg);
    if (q.shade_in_trace)
        return gr_render_seams(f.p, f.stream, s->render_data, f.out, f.bg1, f.bg2, f.bg_width, f.bg_height, f.bg_levels, f.width, f.height, q.block_rows,
                               q.strip_rank, q.strip_count, compact_out, f.opt.max_probes, s->cfg, s->dfg);
    return gr_render_strips(f.p, f.stream, s->render_data, f.out, f.bg1, f.bg2, f.bg_width, f.bg_height, f.bg_levels, f.width, f.height, block_rows,
                            q.strip_rank, q.strip_count, compact_out, f.opt.max_probes, s->cfg, s->dfg);
}

static int fused_shade(frame_context& f) {
    if (!f.out) return GR_OK;
    GR_CHECK(f.begin(GR_STAGE_RENDER));
    GR_CHECK(shade_frame(f, false));
    return f.end(GR_STAGE_RENDER);
}

static int render_fused(frame_context& f) {
    gr_render_state* s = f.s;
    GR_CHECK(fused_plan_frame(f));
    GR_CHECK(fused_own_setup(f));
    GR_CHECK(fused_collect_look_ahead(f));
    if (!f.plan.inline_prepass) GR_CHECK(inspect_prepass(f));   // (with the prepass inside the trace launch: after it)
    GR_CHECK(fused_trace(f));
    if (f.plan.inline_prepass) GR_CHECK(inspect_prepass(f));
    GR_CHECK(fused_submit_look_ahead(f));
    s->previous_key_valid = f.use_prepass && f.plan.strip_count == 1 && !f.gc;
    if (s->previous_key_valid) { s->previous_key = f.own_key(); s->previous_stream = f.stream; }
    GR_CHECK(fused_shade(f));
    if (f.plan.history_wanted || f.plan.guesses_wanted) mark_frame_end(s->device, f.stream);
    return GR_OK;
}

// ---- the reference-shaped sequence ---------------------------------------------------------------------------------------------
// Rays in tile slot order are traced the way the fused kernel's tiles are: the device filled once, tiles by ticket, dearest first by
// what they cost in this state's frame before while the picture has moved little since (GR_REFERENCE_SCHEDULED=0: the reference's own
// launch shape, one work item per record).  The records are the same either way.
static int reference_trace_scheduled(frame_context& f) {
    gr_render_state* s = f.s;
    const int tiles_x = (f.width + 7) / 8, tiles_y = (f.height + 7) / 8, tile_count = tiles_x * tiles_y;
    if (s->ref_cost_tiles != tile_count) {
        for (void*& b : s->ref_cost) { if (b) (void)hipFree(b); b = nullptr; }
        if (s->ref_order) (void)hipFree(s->ref_order);
        if (s->ref_sort_work) (void)hipFree(s->ref_sort_work);
        s->ref_order = s->ref_sort_work = nullptr;
        for (void*& b : s->ref_cost) HIP_CHECK(hipMalloc(&b, (size_t)tile_count * sizeof(unsigned int)));
        HIP_CHECK(hipMalloc(&s->ref_order, (size_t)tile_count * sizeof(unsigned int)));
        HIP_CHECK(hipMalloc(&s->ref_sort_work, ((size_t)tile_count + 128) * sizeof(unsigned int)));
        s->ref_cost_tiles = tile_count;
        s->ref_cost_valid = false;
    }
    const float max_motion = switches::tile_history_max_motion();
    const bool follow = s->ref_cost_valid && !f.gc && f.picture_kept(s->ref_cost_program, s->ref_cost_camera, max_motion);
    std::swap(s->ref_cost[0], s->ref_cost[1]);
    if (follow) {
        GR_CHECK(gr_sort_tiles_by_cost(f.p, f.stream, s->ref_cost[1], tiles_x, tiles_y, s->ref_order, s->ref_sort_work));
        s->history_followed++;
    }
    s->history_recorded++;
    GR_CHECK(gr_do_generic_rays_scheduled(f.p, f.stream, s->rays_in, s->rays_count_in, tile_count, s->cfg, s->dfg, f.attempts,
                                          follow ? s->ref_order : nullptr, s->ref_cost[0]));
    s->ref_cost_valid = true;
    s->ref_cost_camera = *f.camera;
    s->ref_cost_program = gr_program_serial(f.p);
    return GR_OK;
}

static int render_reference_shaped(frame_context& f) {
    gr_render_state* s = f.s;
    gr_program* p = f.p;
    hipStream_t stream = f.stream;
    const int width = f.width, height = f.height, prepass_width = f.prepass_width, prepass_height = f.prepass_height;
    const int tiled = (f.opt.tiled && !f.adaptive) ? 1 : 0;
    const size_t slots = tiled ? (size_t)gr_tiled_slot_count(width, height) : (size_t)width * height;
    GR_CHECK(ensure_rays(s, slots, f.adaptive));

    if (f.use_prepass) {
        GR_CHECK(f.begin(GR_STAGE_PREPASS));
        GR_CHECK(gr_clear_termination_buffer(p, stream, s->termination_buffer, prepass_width, prepass_height));
        HIP_CHECK(hipMemsetAsync(s->rays_count_in, 0, 4, stream));
        GR_CHECK(gr_init_rays_generic(p, stream, s->camera_pos_generic, s->camera_quat, s->rays_in, s->rays_count_in,
                                      prepass_width, prepass_height, s->termination_buffer, prepass_width, prepass_height, 0,
                                      s->tetrad[0], s->tetrad[1], s->tetrad[2], s->tetrad[3], s->cfg, s->dfg, 1, 0));
        GR_CHECK(gr_do_generic_rays(p, stream, s->rays_in, s->rays_count_in, prepass_width * prepass_height, nullptr, nullptr,
                                    s->cfg, s->dfg, width, height, 0, 0, nullptr, nullptr, 0, nullptr));
        GR_CHECK(gr_calculate_singularities(p, stream, s->rays_in, s->rays_count_in, prepass_width * prepass_height,
                                            s->termination_buffer, prepass_width, prepass_height));
        GR_CHECK(f.end(GR_STAGE_PREPASS));
    }

    GR_CHECK(f.begin(GR_STAGE_INIT));
    GR_CHECK(gr_init_rays_generic(p, stream, s->camera_pos_generic, s->camera_quat, s->rays_in, s->rays_count_in, width, height,
                                  s->termination_buffer, f.grid_width(), f.grid_height(), 0, s->tetrad[0], s->tetrad[1], s->tetrad[2], s->tetrad[3],
                                  s->cfg, s->dfg, 0, tiled));
    GR_CHECK(f.end(GR_STAGE_INIT));

    GR_CHECK(f.begin(GR_STAGE_TRACE));
    const bool scheduled_default = switches::reference_scheduled();
    if (tiled && scheduled_default)
        GR_CHECK(reference_trace_scheduled(f));
    else
        GR_CHECK(gr_do_generic_rays(p, stream, s->rays_in, s->rays_count_in, (int)slots, nullptr, nullptr, s->cfg, s->dfg, width,
                                    height, 0, 0, nullptr, nullptr, 0, f.attempts));
    GR_CHECK(f.end(GR_STAGE_TRACE));

    HIP_CHECK(hipMemsetAsync(s->render_data_count, 0, 4, stream));
    GR_CHECK(f.begin(GR_STAGE_RENDER_DATA));
    GR_CHECK(gr_calculate_render_data(p, stream, s->rays_in, s->rays_count_in, (int)slots, s->render_data, s->render_data_count,
                                      width, height, s->cfg, s->dfg));
    GR_CHECK(f.end(GR_STAGE_RENDER_DATA));

    if (f.adaptive) {
        GR_CHECK(f.begin(GR_STAGE_ADAPTIVE));
        HIP_CHECK(hipMemsetAsync(s->rays_adaptive_count, 0, 4, stream));
        GR_CHECK(gr_handle_adaptive_sampling(p, stream, s->rays_in, s->rays_count_in, s->render_data, s->render_data_count,
                                             s->rays_adaptive, s->rays_adaptive_count, s->camera_pos_generic, s->camera_quat,
                                             s->tetrad[0], s->tetrad[1], s->tetrad[2], s->tetrad[3], width, height, s->cfg,
                                             s->dfg));
        GR_CHECK(gr_do_generic_rays(p, stream, s->rays_adaptive, s->rays_adaptive_count, width * height, nullptr, nullptr, s->cfg,
                                    s->dfg, width, height, 0, 0, nullptr, nullptr, 0, f.attempts));
        GR_CHECK(gr_calculate_render_data(p, stream, s->rays_adaptive, s->rays_adaptive_count, width * height, s->render_data,
                                          s->render_data_count, width, height, s->cfg, s->dfg));
        GR_CHECK(f.end(GR_STAGE_ADAPTIVE));
    }

    if (f.out) {
        GR_CHECK(f.begin(GR_STAGE_RENDER));
        GR_CHECK(shade_frame(f, true));
        GR_CHECK(f.end(GR_STAGE_RENDER));
    }
    return GR_OK;
}

// one frame at the state's traced size: out is float4[s->width * s->height] (gr_render_frame below for a state of factor 1, and what a
// supersampled state shades into its own traced frame)
static int render_traced_frame(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream_v, const gr_camera* camera,
                               const gr_features* features_in, const float* cfg_values, int num_cfg_values, const void* bg1,
                               const void* bg2, int bg_width, int bg_height, int bg_levels, void* out, const gr_frame_options* opt_in) {
    GR_CHECK(check_frame_arguments(s, p, m, camera, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels, out));
    HIP_CHECK(hipSetDevice(s->device));
    frame_context f{s, p, (hipStream_t)stream_v, camera, bg1, bg2, bg_width, bg_height, bg_levels, out};
    GR_CHECK(resolve_inputs(f, m, features_in, cfg_values, num_cfg_values, opt_in));
    note_parameter_changes(f);
    GR_CHECK(apply_prepass_policy(f));
    GR_CHECK(upload_parameters(f));
    GR_CHECK(take_prepared_setup(f));
    GR_CHECK(begin_frame(f));
    return f.opt.mode == GR_MODE_FUSED ? render_fused(f) : render_reference_shaped(f);
}

// ---- frame delivery: a frame, then a sink ---------------------------------------------------------------------------------------
// What the entry points below deliver: the frame as render_traced_frame renders it, at the traced size, into the state's own traced frame (at factor 1
// too: the encoders read float4 and the caller has only bytes), and from there into a sink - the caller's memory in one of the formats of frame_format.cpp,
// or the state's accumulation frame.  A device's share of a split frame is traced in blocks of factor x as many rows: the rows its output blocks average.
// Which stages lie between the traced frame and the sink, and in which of the state's buffers, is delivery_plan.cpp's answer (the chain is
// told there, once); this file gathers the facts, allocates what the plan needs and calls the stages' launchers (frame_launch.cpp).
namespace dp = delivery_plan;

// The one launch that makes `out` from a float4 frame of width*factor x height*factor: the format's existing launcher - the box average
// as float4, or resolve and encode in one pass as 8-bit sRGB or as BT.709 Y'CbCr 4:2:0 planes of 8-bit or 10-bit samples (whole frames only).
// strips: the options of a share of a split frame with block_rows in output rows, NULL for a whole frame.
static int encode_frame(gr_program* p, void* stream, int format, int layout, const void* src, int width, int height, int factor,
                        const gr_frame_options* strips, void* out) {
    const int rows = strips ? strips->block_rows : 0, rank = strips ? strips->strip_rank : 0, count = strips ? strips->strip_count : 1,
              compact_out = strips ? strips->compact_out : 0;   // (strip_count 1: every row, whatever the rest says)
    switch (format) {
    case GR_FRAME_F32: return gr_resolve_supersampled(p, stream, src, out, width, height, factor, rows, rank, count, compact_out);
    case GR_FRAME_RGBA8: return gr_present_rgba8(p, stream, src, out, width, height, factor, rows, rank, count, compact_out);
    case GR_FRAME_YUV420: return gr_present_yuv420(p, stream, src, out, width, height, factor, layout);
    case GR_FRAME_YUV420P10: return gr_present_yuv420p10(p, stream, src, out, width, height, factor, layout);
    }
    return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, ("unknown frame format " + std::to_string(format)).c_str());
}

// frame_format::refusal of an output under the entry point's name.  The state is read only where the answer depends on its width.
static int refuse_output(const char* name, int format, int layout, const void* out, const gr_render_state* s, int strip_count) {
    const std::string wrong = frame_format::refusal(format, false, layout, (uintptr_t)out, s ? &s->out_width : nullptr, strip_count);
    return wrong.empty() ? GR_OK : gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string(name) + ": " + wrong).c_str());
}

// where a delivered frame goes: encoded as (format, layout) into out, or - accumulate - weight x the frame into the accumulation frame
struct sink { int format, layout; void* out; bool accumulate; float weight; int first; };

// the facts of a call on this state, and what delivery_plan.cpp makes of them (options NULL: a whole frame)
static dp::plan plan_delivery(const gr_render_state* s, dp::call_kind call, int format, const void* out, const gr_frame_options* options) {
    dp::facts f;
    f.factor = s->supersample;
    f.filtered = s->filter != GR_FILTER_BOX;
    f.glare_set = s->glare_set;
    f.tone = !s->tone_set ? dp::TONE_NONE : s->tone.mode == GR_TONE_AUTO ? dp::TONE_AUTO : dp::TONE_MANUAL;
    f.tone_reset = s->tone_reset || !s->tone_words;   // (words allocated by this call start zeroed too)
    f.format = format;
    f.call = call;
    f.out_is_null = !out;
    if (options) {
        f.strip_count = options->strip_count;
        f.mode_is_fused = options->mode == GR_MODE_FUSED;   // (as the fused path reads strips; the reference-shaped sequence renders whole frames)
        f.block_rows = options->block_rows;
    }
    return dp::plan_delivery(f);
}

// the state's buffer of that name (dp::buffer's first seven)
static void** state_buffer(gr_render_state* s, int name) {
    void** const buffers[dp::STATE_BUFFERS] = {&s->traced_frame, &s->accumulation, &s->filtered_frame, &s->glare_frame, &s->glare_scratch, &s->tone_frame, &s->tone_words};
    return buffers[name];
}

// tone_words: a gr_tone_state at 0, the 385 counters at 32
static const size_t TONE_WORDS_BYTES = 32 + GR_METER_COUNTERS * sizeof(unsigned);

// What the plan needs of the state's buffers and is not there yet, on the state's device - which is set here only if something is
// missing (render_traced_frame sets it for everything else).  The traced frame of a factor-1 state comes with the resolve's events,
// the tone's words with a reset.
static int allocate_missing(gr_render_state* s, unsigned needs, bool device_is_set) {
    for (int name = 0; name < dp::STATE_BUFFERS; name++) {
        void** buffer = state_buffer(s, name);
        if (!(needs >> name & 1) || *buffer) continue;
        if (!device_is_set) HIP_CHECK(hipSetDevice(s->device));
        device_is_set = true;
        const size_t pixels = name == dp::TRACED ? (size_t)s->width * s->height : (size_t)s->out_width * s->out_height;
        HIP_CHECK(hipMalloc(buffer, name == dp::TONE_WORDS ? TONE_WORDS_BYTES : pixels * 4 * sizeof(float)));
        if (name == dp::TRACED)
            for (auto& ev : s->ev_resolve)
                if (!ev) HIP_CHECK(hipEventCreate(&ev));
        if (name == dp::TONE_WORDS) s->tone_reset = true;
    }
    return GR_OK;
}

// The plan's stages, one launcher each, in order.  strips: the call's options where a stage may take a share's description from them.
// No call here waits for the device.
static int run_stages(const dp::plan& plan, gr_render_state* s, gr_program* p, void* stream, const sink& to, const gr_frame_options* strips,
                      const float* taps, int tap_count) {
    const int w = s->out_width, h = s->out_height;
    const auto at = [&](dp::buffer name) -> void* { return name == dp::NONE ? nullptr : name == dp::OUT ? to.out : *state_buffer(s, name); };
    for (int i = 0; i < plan.count; i++) {
        const dp::stage& stage = plan.stages[i];
        const void* src = at(stage.source);
        void* dst = at(stage.destination);
        switch (stage.kind) {
        case dp::FILTER: GR_CHECK(gr_resolve_filtered(p, stream, src, dst, w, h, stage.factor, taps, tap_count)); break;
        case dp::BOX: GR_CHECK(gr_resolve_supersampled(p, stream, src, dst, w, h, stage.factor, 0, 0, 1, 0)); break;
        case dp::GLARE: GR_CHECK(gr_apply_glare(p, stream, src, dst, s->glare_scratch, (size_t)w * h * 4 * sizeof(float), w, h, &s->glare)); break;
        case dp::ZERO_TONE_STATE:
            HIP_CHECK(hipMemsetAsync(s->tone_words, 0, 32, (hipStream_t)stream));
            s->tone_reset = false;
            break;
        case dp::METER: GR_CHECK(gr_meter_frame(p, stream, src, w, h, (char*)s->tone_words + 32)); break;
        case dp::SOLVE: GR_CHECK(gr_meter_solve_device(p, stream, (char*)s->tone_words + 32, &s->tone, s->tone_words)); break;
        case dp::TONE: {   // auto: the word the solve wrote; manual: the host's gain in the argument block
            const void* device_gain = s->tone.mode == GR_TONE_AUTO ? &((gr_tone_state*)s->tone_words)->gain : nullptr;
            float host_gain = 1.f;
            int q = 0;
            if (!device_gain) gr_internal_tone_gain((double)s->tone.stops, &host_gain, &q);
            GR_CHECK(gr_apply_tone(p, stream, src, dst, w, h, &s->tone, device_gain, host_gain));
            break;
        }
        case dp::ACCUMULATE: GR_CHECK(gr_shutter_accumulate(p, stream, src, dst, w, h, stage.factor, to.weight, to.first)); break;
        case dp::ENCODE: GR_CHECK(encode_frame(p, stream, to.format, to.layout, src, w, h, stage.factor, stage.with_strips ? strips : nullptr, dst)); break;
        }
    }
    return GR_OK;
}

// The delivery core of a frame and of a sub-frame (`name`: the entry point's, for its refusals): facts, plan, refuse, allocate, render,
// stages.  What needs no device is refused first; nothing is allocated for a call that is refused.
static int deliver_frame(const char* name, const sink& to, gr_render_state* s, gr_program* p, const gr_metric* m, void* stream,
                         const gr_camera* camera, const gr_features* features, const float* cfg_values, int num_cfg_values, const void* bg1,
                         const void* bg2, int bg_width, int bg_height, int bg_levels, const gr_frame_options* options) {
    gr_frame_options opt;
    gr_frame_options_default(&opt);
    if (options) opt = *options;
    const dp::plan plan = plan_delivery(s, to.accumulate ? dp::ACCUMULATE_SUBFRAME : dp::DELIVER, to.format, to.out, &opt);
    if (plan.direct)
        return render_traced_frame(s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels, to.out, options);
    if (plan.refused) return gr_internal::refuse(name, plan.refused);
    GR_CHECK(check_frame_arguments(s, p, m, camera, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels, to.accumulate ? s : to.out));   // (s: any non-NULL out)
    float taps[GR_FILTER_MAX_TAPS];
    int tap_count = 0;
    if (s->filter != GR_FILTER_BOX) GR_CHECK(gr_filter_taps(s->filter, s->supersample, taps, &tap_count));   // (geodesic_hip_internal.h, "Filtered frames")
    GR_CHECK(allocate_missing(s, plan.needs, false));
    if (to.accumulate && to.first) s->accumulated = 0;   // (a sub-frame that fails below leaves nothing to deliver)
    gr_frame_options traced = opt;   // the frame behind it: blocks of factor x as many rows
    traced.block_rows *= s->supersample;
    GR_CHECK(render_traced_frame(s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels,
                                 s->traced_frame, &traced));
    const bool timed = opt.time_kernels == 1;
    if (timed) HIP_CHECK(hipEventRecord(s->ev_resolve[0], (hipStream_t)stream));
    GR_CHECK(run_stages(plan, s, p, stream, to, &opt, taps, tap_count));
    if (timed) {
        HIP_CHECK(hipEventRecord(s->ev_resolve[1], (hipStream_t)stream));
        s->resolve_timed = true;
    }
    if (to.accumulate) s->accumulated++;
    return GR_OK;
}

// gr_render_frame and its three encoded kin by format. All but float4 refuse a NULL and what their launch would of `out` before anything is rendered or allocated.
int gr_internal_render_frame_as(int format, int layout, gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera,
                                const gr_features* features, const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2,
                                int bg_width, int bg_height, int bg_levels, void* out, const gr_frame_options* options) {
    if (!frame_format::find(format)) return refuse_output("gr_internal_render_frame_as", format, layout, out, s, 1);
    const frame_format::row& f = *frame_format::find(format);
    if (format != GR_FRAME_F32) {
        if (!s || !p || !m || !camera || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string(f.entry) + ": null argument").c_str());
        GR_CHECK(refuse_output(f.entry, format, layout, out, s, options ? options->strip_count : 1));
    }
    if (!s) return render_traced_frame(s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels, out, options);   // (float4: refused there)
    s->resolve_timed = false;
    return deliver_frame(f.entry, sink{format, layout, out, false, 0.f, 0}, s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2,
                         bg_width, bg_height, bg_levels, options);
}

int gr_render_frame(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera, const gr_features* features,
                    const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height,
                    int bg_levels, void* out, const gr_frame_options* options) {
    return gr_internal_render_frame_as(GR_FRAME_F32, 0, s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height,
                                       bg_levels, out, options);
}

int gr_render_frame_rgba8(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera, const gr_features* features,
                          const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height,
                          int bg_levels, void* out_rgba8, const gr_frame_options* options) {
    return gr_internal_render_frame_as(GR_FRAME_RGBA8, 0, s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width, bg_height,
                                       bg_levels, out_rgba8, options);
}

int gr_render_frame_yuv420(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera, const gr_features* features,
                           const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height,
                           int bg_levels, void* out_yuv420, int layout, const gr_frame_options* options) {
    return gr_internal_render_frame_as(GR_FRAME_YUV420, layout, s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width,
                                       bg_height, bg_levels, out_yuv420, options);
}

int gr_render_frame_yuv420p10(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera,
                              const gr_features* features, const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2,
                              int bg_width, int bg_height, int bg_levels, void* out_yuv420p10, int layout, const gr_frame_options* options) {
    return gr_internal_render_frame_as(GR_FRAME_YUV420P10, layout, s, p, m, stream, camera, features, cfg_values, num_cfg_values, bg1, bg2, bg_width,
                                       bg_height, bg_levels, out_yuv420p10, options);
}

// ---- motion-blurred frames (geodesic_hip_internal.h, "Motion-blurred frames") -------------------------------------------------------
// One sub-frame of a shutter: a delivery whose sink is the state's accumulation frame, by ONE launch of gr_shutter_accumulate.  A
// sub-frame is a frame: nothing in frame_plan.cpp knows of it, and consecutive sub-frames are consecutive frames of the state (tile
// history, look-ahead, still-camera reuse).
int gr_render_subframe(gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera, const gr_features* features,
                       const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2, int bg_width, int bg_height, int bg_levels,
                       float weight, int first, const gr_frame_options* options) {
    if (!s || !p || !m || !camera || ((!bg1 || !bg2) && !state_has_sky(s))) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_subframe: null argument");
    if (!std::isfinite(weight)) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_subframe: a weight that is not finite");
    if (options && options->strip_count > 1)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_subframe: whole frames only (strip_count > 1); a share of a split frame is not accumulated");
    // (the three refusals above need no device and look at no object; without a device the answer from here on is GR_ERROR_DEVICE, as
    // the creation of every object this call takes would have been)
    int devices = 0;
    HIP_CHECK(hipGetDeviceCount(&devices));
    if (!first && !s->accumulated)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_render_subframe: first = 0 on a state that holds no accumulation (a shutter's first sub-frame has first = 1)");
    s->resolve_timed = false;
    return deliver_frame("gr_render_subframe", sink{GR_FRAME_F32, 0, nullptr, true, weight, first}, s, p, m, stream, camera, features, cfg_values,
                         num_cfg_values, bg1, bg2, bg_width, bg_height, bg_levels, options);
}

// The accumulation frame through the format's launch at factor 1 - the launch gr_render_frame* ends with, from another source.
int gr_deliver_accumulated(gr_render_state* s, gr_program* p, void* stream, int format, int layout, void* out) {
    if (!s || !p || !out) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_deliver_accumulated: null argument");
    GR_CHECK(refuse_output("gr_deliver_accumulated", format, layout, out, s, 1));
    if (!s->accumulated || !s->accumulation)
        return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, "gr_deliver_accumulated: the state holds no accumulation (gr_render_subframe first)");
    const dp::plan plan = plan_delivery(s, dp::DELIVER_ACCUMULATED, format, out, nullptr);
    if (plan.refused) return gr_internal::refuse("gr_deliver_accumulated", plan.refused);
    HIP_CHECK(hipSetDevice(s->device));   // (nothing is rendered here that would set it)
    GR_CHECK(allocate_missing(s, plan.needs, true));
    return run_stages(plan, s, p, stream, sink{format, layout, out, false, 0.f, 0}, nullptr, nullptr, 0);
}

}  // extern "C"
