// frame_plan.hpp — what a frame DECIDES, apart from what it launches: the environment switches of frame.cpp, how far the picture moves
// between two cameras, and the plan of a fused frame (which kernel, which schedule, what is refused).  Plain C++, no HIP header: every
// decision here can be checked without a GPU (tests/frame_plan_check.cpp).  frame.cpp gathers the inputs and carries the plan out.
#pragma once
#include <functional>

#include "../../include/geodesic_hip_internal.h"

namespace frame_plan {

// Every environment switch of frame.cpp: name, default, meaning (frame_plan.cpp has the measurements behind the defaults).  Each is read
// once, the first time it is asked for.
namespace switches {
int tile_order();                    // GR_TILE_ORDER            unset (-1): order a share's tiles by the prepass rays' costs; 0 never, else always
bool reuse_still_camera();           // GR_REUSE_STILL_CAMERA    1: default of gr_frame_tuning.reuse_still_camera
bool tile_history();                 // GR_TILE_HISTORY          1: default of gr_frame_tuning.tile_history (within its conditions)
bool lattice_history();              // GR_LATTICE_HISTORY       1: the lattice launch of an adaptive whole frame records and follows a history too
bool adaptive_guess();               // GR_ADAPTIVE_GUESS        1: the lattice launch traces ahead the dear pixels of the second launch
int trace_compact();                 // GR_TRACE_COMPACT         0: keep_lanes (1..64) of gr_trace_compact for every frame
int trace_rays_per_lane();           // GR_TRACE_RAYS_PER_LANE   2: rays per lane where the program has gr_trace_pair (1 or 2)
bool inline_prepass();               // GR_INLINE_PREPASS        1: default of gr_frame_tuning.inline_prepass (within its conditions)
float tile_history_max_motion();     // GR_TILE_HISTORY_MAX_MOTION  48: pixels of picture motion up to which a tile history is followed
float tile_history_max_turn();       // GR_TILE_HISTORY_MAX_TURN    64: ... of camera turn, with both frames seeing the origin
bool tile_history_follow();          // GR_TILE_HISTORY_FOLLOW   1: shift the history by how far the origin's picture has moved
bool guess_still_camera();           // GR_GUESS_STILL_CAMERA    0: default of gr_frame_tuning.guess_still_camera
float adaptive_guess_max_motion();   // GR_ADAPTIVE_GUESS_MAX_MOTION  0.5: pixels of motion up to which traced-ahead pixels are used
bool adaptive_pending_list();        // GR_ADAPTIVE_PENDING_LIST 1: the second launch of adaptive sampling works off a list, dearest first
float adaptive_history_max_motion(); // GR_ADAPTIVE_HISTORY_MAX_MOTION  48: pixels up to which that list is ordered by the frame before's costs
int park_lanes();                    // GR_PARK="lanes,trips"    0: default of gr_frame_tuning.park_lanes ...
int park_trips();                    //                          0: ... and of park_trips (<= 0: 512)
bool reference_scheduled();          // GR_REFERENCE_SCHEDULED   1: reference-shaped frames in tile slot order are traced by ticket, dearest first
}   // namespace switches

// Where a camera sees the coordinate origin, in pixels, as if space were flat (= gr_camera_origin_on_screen); false: not on screen.
bool origin_on_screen(const gr_camera& c, float fov_degrees, int width, int height, float out[2]);
// An upper estimate of how many pixels the picture moves between two cameras (= gr_picture_motion; 1e9 where there is none) ...
float picture_motion(const gr_camera& a, const gr_camera& b, float fov_degrees, int width);
// ... and its two parts on their own: the turn of the camera and the parallax of the origin
bool picture_motion_parts(const gr_camera& a, const gr_camera& b, float fov_degrees, int width, float& turn_px, float& parallax_px);

struct fused_input {
    int width = 0, height = 0;                            // traced size
    int strip_count = 1, strip_rank = 0, block_rows = 16; // as in gr_frame_options
    bool adaptive = false, use_prepass = false;           // as resolved (features, metric, policy, a grid of at least 1 x 1)
    bool prefetched = false, geodesic = false, out = false;
    gr_frame_tuning tune{};
    bool has_pair = false, has_parking = false, has_tile_shading = false;   // the program's kernels
    std::function<long long()> wave_slots;                // gr_trace_fused_wave_slots (asks the runtime the first time: only where needed)
    long long (*tile_order_bytes)(int width, int height, int block_rows, int strip_rank, int strip_count) = nullptr;   // gr_tile_order_bytes
    std::function<bool()> earlier_frame_still_running;    // asked at most once, and only by a frame that would record or guess by default
    size_t tile_order_bytes_held = 0;                     // the state's tile_order_bytes
    bool tile_cost_valid = false, tile_cost_anchored = false;
    int tile_cost_shape[3] = {0, 0, 0};
    gr_camera tile_cost_camera{}, camera{};
    float field_of_view = 0;
};

struct refusal { int code = GR_OK; const char* message = nullptr; };

struct fused_plan {
    refusal refused;                  // before any launch of the frame
    refusal refused_at_trace;         // by the launch of gr_trace_fused on every pixel, where that is the frame's trace
    int strip_count = 1, strip_rank = 0, block_rows = 0;
    int prepass_margin = 0;
    size_t cells = 0;
    int hist_width = 0, hist_height = 0, hist_block_rows = 0, shape[3] = {0, 0, 0};
    bool history_wanted = false, guesses_wanted = false, device_busy = false, order_capable = false;
    bool inline_prepass = false, order_tiles = false, record_history = false, history_order = false;
    bool invalidate_tile_cost = false;   // the state's tile_cost_valid is to be cleared
    int keep_lanes = 0, rays_per_lane = 1;
    int park_lanes = 0, park_trips = 512;
    bool parking = false, shade_in_trace = false;
};

fused_plan plan_fused(const fused_input& in);

}   // namespace frame_plan
