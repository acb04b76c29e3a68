// trace_plan.hpp — what a launch of the trace stage DECIDES, apart from what it enqueues: the environment switches of the launchers, the
// one rule for a strip description, a device's tile count, and the plan of gr_trace_fused and its kin (which kernel, how many
// workgroups, by ticket or not, what is reset, what is refused).  Plain C++, no HIP header: every decision here can be checked without
// a GPU (tests/trace_plan_check.cpp).  trace_launch.cpp gathers the inputs and carries the plan out.
#pragma once
#include <cstddef>
#include <functional>

#include "internal.hpp"

namespace trace_plan __attribute__((visibility("hidden"))) {   // (not among the library's exported names)

// Every environment switch of the trace launchers: name, value when unset, the values accepted, value for anything else.  All are
// experiment hooks.  Six are read once per process, the first time they are asked for; GR_TICKET_TILES is read at EVERY launch that
// draws a ticket (a probe can change it between two launches of one process).
namespace switches {
int trace_block();                // GR_TRACE_BLOCK               256; 64 or 128 (kernel built with the same -DGR_TRACE_BLOCK); else 256
bool trace_persistent();          // GR_TRACE_PERSISTENT          on; off where the text begins with '0': one wave per tile whatever the size
int trace_waves_per_simd();       // GR_TRACE_WAVES_PER_SIMD      0 (what fits); 1..8: that many persistent waves per SIMD whatever fits; else 0
int ticket_tiles();               // GR_TICKET_TILES              0 (the plan's own count); 1..64: tiles per ticket; else 0.  Every launch.
int speculative_classes();        // GR_SPECULATIVE_CLASSES       5; 0..14; else 0 (sic: not the default)
int tile_history_reach();         // GR_TILE_HISTORY_REACH        2; 0..8: tiles a tile looks around itself in the history; else 2
int scheduled_waves_per_simd();   // GR_SCHEDULED_WAVES_PER_SIMD  0 (what fits); 1..8: gr_do_generic_rays_scheduled's waves per SIMD; else 0
int parse(const char* name, const char* text);   // what `text` (NULL: unset) means for the switch of that name, by the table above
}   // namespace switches

// ---- the strip description ----------------------------------------------------------------------------------------------------------
// strip_count <= 1 means the whole frame: one strip, rank 0, and ONE block whose rows are the caller's convention -
enum whole_frame_block {
    HEIGHT_ROUNDED_UP_TO_8,   // the trace, its tile order and the refine launches: the block is the image in whole tiles
    EIGHT_ROWS,               // the prepass launches: they only compare image rows with block_rows, and no row is another device's
    THE_HEIGHT                // the row-dealing launches (resolve, present): exactly the image's rows
};
struct strip_share {
    bool bad;   // block_rows <= 0, or not 0 <= strip_rank < strip_count.  Each caller adds its own conditions and words its own refusal.
    int block_rows, strip_rank, strip_count;
};
strip_share strips(int height, int block_rows, int strip_rank, int strip_count, whole_frame_block whole);
// (how many blocks of the image's rows the share's rank holds: gr_strip_local_blocks of the public header, defined in trace_plan.cpp)
// Tiles (one wave each) a device traces: its row blocks cut into 8 x 8 tiles and, on a split frame, per block the halo row in 64-pixel
// pieces.  block_rows is a multiple of 8 here; 0 for an image without pixels.
long long device_tiles(int width, int height, const strip_share& s);

// ---- gr_trace_fused, gr_trace_pair, gr_trace_fused_adaptive, gr_trace_fused_launch -------------------------------------------------
struct trace_input {
    gr_trace_fused_args args{};   // as gr_trace_fused_launch normalises them (lattice 1 or 2, flags 0 or 1)
    int rays_per_lane = 1;        // 2: gr_trace_pair
    gr_internal::program_facts program;
    // Workgroups of `wg` lanes of `kernel` that one compute unit holds at once; GR_OK or the status to return (its text is set).
    // Asked at most once, and only when nothing is left to refuse: it is the plan's one question to the device.
    std::function<int(int kernel, int wg, int* per_cu)> resident_per_cu;
};

struct refusal { int code = GR_OK; const char* message = nullptr; };   // (no message: resident_per_cu's status)

// the kernels' trace_shading and parking_lot, by value and field for field (kernels/trace.hip)
struct kernel_shading { void* out; const void* bg1; const void* bg2; int bg_width, bg_height, bg_levels, most_probes, compact_out; };
struct kernel_lot { void* records; void* words; int lanes, trips, slots, groups; };

struct trace_plan {
    refusal refused;
    bool nothing = false;          // an empty share: GR_OK and no device call
    int kernel = K_TRACE_FUSED, wg = 256;
    unsigned grid = 0;             // workgroups
    bool ticket = false;           // the launch draws its tiles from a counter (internal.hpp: draw_ticket)
    int ticket_tiles = 1, prepass_tickets = 0, total_waves = 0;
    int block_rows = 0, strip_rank = 0, strip_count = 1;
    int last_class_is_skipped = 0; // bits 8 and up: the speculative classes
    size_t termination_bytes = 0, tile_cost_bytes = 0, lot_words_bytes = 0;   // what is reset before the launch: to 0xff, to 0, to 0
    kernel_shading shading{};
    kernel_lot lot{};
};

trace_plan plan_trace(const trace_input& in);

// ---- the other persistent launches: how many workgroups --------------------------------------------------------------------------
// `per_cu`: resident workgroups of the kernel per compute unit (256 lanes; gr_do_generic_rays_scheduled: 64)
long long pending_groups(int compute_units, int per_cu, int waves_per_simd, int width, int height);   // gr_trace_pending
long long scheduled_groups(int compute_units, int per_cu, int tile_count);                            // gr_do_generic_rays_scheduled
long long compact_groups(int compute_units, long long tiles);                                         // gr_trace_compact

}   // namespace trace_plan
