// trace_plan.cpp — the decisions of a trace launch (trace_plan.hpp).  No HIP call, no state written: inputs in, plan out.
#include "trace_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#ifndef GR_DEFAULT_SPECULATIVE_CLASSES
#define GR_DEFAULT_SPECULATIVE_CLASSES 5   // gr_trace_fused: the list's first classes do not wait for the prepass cells of their own launch
#endif

// block-cyclic dealing: of the image's blocks of block_rows rows, rank r holds r, r + strip_count, ...
extern "C" int gr_strip_local_blocks(int height, int block_rows, int strip_rank, int strip_count) {
    if (block_rows <= 0 || strip_count <= 0) return 0;
    int total = (height + block_rows - 1) / block_rows;
    return strip_rank < total ? (total - strip_rank + strip_count - 1) / strip_count : 0;
}

namespace trace_plan {

namespace switches {
namespace {
// accepted: low, low + step, ... up to high.  on_unless_0 looks at the text's first character only.
struct spec { const char* name; int unset, low, high, step, otherwise; bool on_unless_0; };
const spec TABLE[] = {
    {"GR_TRACE_BLOCK", 256, 64, 128, 64, 256, false},
    {"GR_TRACE_PERSISTENT", 1, 0, 0, 1, 1, true},
    {"GR_TRACE_WAVES_PER_SIMD", 0, 1, 8, 1, 0, false},
    {"GR_TICKET_TILES", 0, 1, 64, 1, 0, false},
    {"GR_SPECULATIVE_CLASSES", GR_DEFAULT_SPECULATIVE_CLASSES, 0, 14, 1, 0, false},
    {"GR_TILE_HISTORY_REACH", 2, 0, 8, 1, 2, false},
    {"GR_SCHEDULED_WAVES_PER_SIMD", 0, 1, 8, 1, 0, false},
};
int read(const char* name) { return parse(name, getenv(name)); }
}   // namespace

int parse(const char* name, const char* text) {
    for (const spec& s : TABLE) {
        if (strcmp(s.name, name) != 0) continue;
        if (s.on_unless_0) return !(text && text[0] == '0');
        const int v = text ? atoi(text) : s.unset;
        return (v >= s.low && v <= s.high && (v - s.low) % s.step == 0) ? v : s.otherwise;
    }
    return 0;
}

// four tile-waves per workgroup (measured on MI355X, 4K Kerr: 64 -> 7.59 ms, 128 -> 7.43, 256 -> 7.24; one wave per SIMD still leaves
// the full 512-VGPR budget to the heaviest metrics)
int trace_block() { static const int v = read("GR_TRACE_BLOCK"); return v; }
bool trace_persistent() { static const bool v = read("GR_TRACE_PERSISTENT") != 0; return v; }
int trace_waves_per_simd() { static const int v = read("GR_TRACE_WAVES_PER_SIMD"); return v; }   // (occupancy studies)
int ticket_tiles() { return read("GR_TICKET_TILES"); }
// Classes are octaves of a tile's longest ray in the frame before, 16 384 attempts = class 0: the default, 5, are the tiles that had a
// ray of 1 024 attempts or more.
int speculative_classes() { static const int v = read("GR_SPECULATIVE_CLASSES"); return v; }
int tile_history_reach() { static const int v = read("GR_TILE_HISTORY_REACH"); return v; }   // the image may have moved by that much since
int scheduled_waves_per_simd() { static const int v = read("GR_SCHEDULED_WAVES_PER_SIMD"); return v; }   // (occupancy studies)
}   // namespace switches

strip_share strips(int height, int block_rows, int strip_rank, int strip_count, whole_frame_block whole) {
    if (strip_count <= 1) {
        strip_count = 1;
        strip_rank = 0;
        block_rows = whole == HEIGHT_ROUNDED_UP_TO_8 ? ((height + 7) / 8) * 8 : whole == EIGHT_ROWS ? 8 : height;
    }
    return {block_rows <= 0 || strip_rank < 0 || strip_rank >= strip_count, block_rows, strip_rank, strip_count};
}

long long device_tiles(int width, int height, const strip_share& s) {
    if (width <= 0 || height <= 0) return 0;
    const long long per_block = (long long)((width + 7) / 8) * (s.block_rows / 8) + (s.strip_count > 1 ? (width + 63) / 64 : 0);
    return per_block * gr_strip_local_blocks(height, s.block_rows, s.strip_rank, s.strip_count);
}

static trace_plan refuse(const char* message) {
    trace_plan plan;
    plan.refused = {GR_ERROR_INVALID_ARGUMENT, message};
    return plan;
}

// k persistent waves per SIMD as workgroups of wg lanes on the whole device
static long long groups_of_waves_per_simd(int compute_units, int k, int wg) { return (long long)compute_units * 4 * k * 64 / wg; }

trace_plan plan_trace(const trace_input& in) {
    const gr_trace_fused_args& a = in.args;
    const int rays_per_lane = in.rays_per_lane, width = a.width, height = a.height, lattice = a.lattice;
    trace_plan plan;
    // the prepass inside the launch: its cell waves are the first tickets (gr_trace_fused's prepass_tickets)
    if (a.inline_prepass) {
        if (rays_per_lane != 1 || a.pending_only || (a.tile_order && !a.tile_order_by_history) || !a.termination_buffer || a.prepass_width <= 0 ||
            a.prepass_height <= 0 || a.prepass_width == width || a.prepass_height == height)
            return refuse("inline_prepass: gr_trace_fused on every pixel of its rows (or the lattice launch of adaptive sampling), in image order or the order of "
                          "gr_order_tiles_by_history (gr_order_tiles' needs the prepass first), with a prepass grid");
        // a cell wave is 8 x 8 cells (trace.hip: GR_CELL_BLOCK; a program built with -DGR_CELL_BLOCK=0 takes 64 cells of a row)
        plan.prepass_tickets = in.program.cell_rows ? (int)(((long long)a.prepass_width * a.prepass_height + 63) / 64)
                                                    : ((a.prepass_width + 7) / 8) * ((a.prepass_height + 7) / 8);
    }
    if ((lattice != 1 && lattice != 2) || ((lattice == 2 || a.pending_only) && rays_per_lane != 1))
        return refuse("lattice / pending_only: gr_trace_fused only");
    const gr_parking_lot& lot = a.parking;
    const bool parks = lot.lanes > 0;
    if (parks) {
        if (!in.program.has_parking)
            return refuse("parking: the program was built without -DGR_PARKING in its argument string (gr_program_has_parking)");
        if (rays_per_lane != 1 || lattice != 1 || a.pending_only || a.shading.out)
            return refuse("parking: gr_trace_fused on every pixel of its rows, one ray per lane, no in-tile shading");
        if (!lot.records || !lot.words || lot.lanes > 64 || lot.trips < 1 || lot.slots < 64 || lot.slots > (1 << 24) || lot.groups < 1)
            return refuse("parking: records and words (gr_parking_lot_bytes), 1 <= lanes <= 64, trips >= 1, 64 <= slots <= 2^24, groups >= 1");
    }
    if (rays_per_lane == 2 && !in.program.has_pair)
        return refuse("this program has no gr_trace_pair kernel (its expressions do not instantiate on pairs)");
    const strip_share share = strips(height, a.block_rows, a.strip_rank, a.strip_count, HEIGHT_ROUNDED_UP_TO_8);
    if (share.bad || share.block_rows % 8 != 0) return refuse("block_rows must be a positive multiple of 8 and 0 <= strip_rank < strip_count");
    if (share.strip_count > 1 && height > 1 && (height - 1) % share.block_rows == 0)
        return refuse("the last image row must not start a block (its filter reads the row above)");
    plan.block_rows = share.block_rows; plan.strip_rank = share.strip_rank; plan.strip_count = share.strip_count;
    // lattice 2: tiles of the whole half-resolution grid, whoever owns the rows (the kernel leaves the rows of others alone)
    const long long waves = lattice == 2 ? (long long)((width / 2 + 7) / 8) * ((height / 2 + 7) / 8) : device_tiles(width, height, share);
    if (waves <= 0) { plan.nothing = true; return plan; }
    if (waves > 0x7fffffff) return refuse("too many tiles");
    plan.total_waves = (int)waves;
    if (a.shading.out) {
        if (!in.program.tile_shading) return refuse("in-tile shading: the program was built without -DGR_TILE_SHADING in its argument string");
        if (rays_per_lane != 1 || lattice != 1 || a.pending_only || width % 8 != 0 || height % 8 != 0)
            return refuse("in-tile shading: gr_trace_fused on every pixel of an image whose sides are multiples of 8");
        plan.shading = {a.shading.out, a.shading.background1, a.shading.background2, a.shading.bg_width, a.shading.bg_height, a.shading.bg_levels,
                        a.shading.max_probes, share.strip_count > 1 ? a.shading.compact_out : 0};
    }
    if (a.tile_cost && (rays_per_lane != 1 || a.pending_only || (lattice == 2 && share.strip_count > 1)))
        return refuse("tile_cost: gr_trace_fused on every pixel of its rows, or the lattice launch of a whole frame");
    // (every argument has been checked by now: nothing below fails for a reason of the caller's, and nothing above has asked the device)
    // (the lattice launch of adaptive sampling that leaves its rays behind is a kernel of its own: gr_trace_fused is not touched by it)
    const int wg = plan.wg = switches::trace_block();
    plan.kernel = parks ? K_TRACE_FUSED_PARKING : rays_per_lane == 2 ? K_TRACE_PAIR : (lattice == 2 && a.lattice_rays) ? K_TRACE_FUSED_LATTICE : K_TRACE_FUSED;
    int per_cu = 0;
    if (int rc = in.resident_per_cu(plan.kernel, wg, &per_cu)) { plan.refused = {rc, nullptr}; return plan; }
    // Persistent mode only pays when there are more tiles than wave slots.  The launch is exactly as many workgroups as the kernel's
    // register and scratch footprint lets the device hold: a larger one leaves workgroups queued behind the resident ones which start
    // only when the tickets are gone, and which the dispatcher then has to retire before the next launch's workgroups get the freed slots.
    long long resident = (long long)in.program.compute_units * per_cu;
    // A caller that keeps several frames in flight may take fewer slots per launch: two smaller launches then share the device and the
    // one drains while the other is in full swing (gr_frame_options.trace_waves_per_simd).
    if (const int forced = switches::trace_waves_per_simd()) resident = groups_of_waves_per_simd(in.program.compute_units, forced, wg);
    else if (a.waves_per_simd >= 1 && a.waves_per_simd <= 8) resident = std::min(resident, groups_of_waves_per_simd(in.program.compute_units, a.waves_per_simd, wg));
    long long groups = (((waves + rays_per_lane - 1) / rays_per_lane + plan.prepass_tickets) * 64 + wg - 1) / wg;
    // prepass tickets need the ticket order whatever the size, and so do a lot and the pixels traced ahead
    plan.ticket = (switches::trace_persistent() && groups > resident) || plan.prepass_tickets || parks || a.guessed;
    if (plan.ticket) {
        groups = std::min(groups, resident);
        // tiles per ticket: one, unless a wave would draw more than 32 tickets (then as many as keep it at 32, at most 8)
        const long long launched_waves = groups * (wg / 64);
        const long long per_wave = (waves + plan.prepass_tickets + launched_waves - 1) / launched_waves;
        plan.ticket_tiles = (int)std::min<long long>(8, std::max<long long>(1, (per_wave + 31) / 32));
        if (const int v = switches::ticket_tiles()) plan.ticket_tiles = v;
    }
    plan.grid = (unsigned)groups;
    if (plan.prepass_tickets) plan.termination_bytes = (size_t)a.prepass_width * a.prepass_height * sizeof(int);   // every cell unknown (GR_CELL_UNKNOWN = -1) until its ray has been traced
    if (a.tile_cost) plan.tile_cost_bytes = (size_t)plan.total_waves * sizeof(unsigned int);
    // Whether the list's last class is a promise (gr_order_tiles: nothing to trace, nothing to look up) or a guess
    // (gr_order_tiles_by_history) is written into the list by the launch that made it, and the kernel reads it there; the caller's
    // flag only says which he thinks it is, for the checks above.  The word's low bits stay 0 (kept in the kernel's parameter list: 1
    // would force the promise, nothing passes it).  Its upper bits: how many of the list's classes, dearest first, do not wait for the
    // prepass cells they look at when those are traced by this launch (trace_fused_body: speculative tiles).
    const int speculative = a.speculative_classes < 0 ? 0 : a.speculative_classes == 0 ? switches::speculative_classes() : std::min(a.speculative_classes, 14);
    if (plan.prepass_tickets && a.tile_order && a.tile_order_by_history && !parks) plan.last_class_is_skipped |= speculative << 8;
    if (parks) {   // an empty lot before every launch
        plan.lot = {lot.records, lot.words, lot.lanes, lot.trips, lot.slots, lot.groups};
        plan.lot_words_bytes = (16 + (size_t)lot.groups) * sizeof(unsigned int);
    }
    return plan;
}

// (How many entries the list holds is only known on the device: the launch fills the machine and its waves draw tickets until the list
// is used up - no more workgroups than the worst case needs, though.)
long long pending_groups(int compute_units, int per_cu, int waves_per_simd, int width, int height) {
    const int wg = 256;
    long long groups = (long long)compute_units * per_cu;
    if (waves_per_simd >= 1 && waves_per_simd <= 8) groups = std::min(groups, groups_of_waves_per_simd(compute_units, waves_per_simd, wg));
    const long long worst = (3LL * (width / 2) * (height / 2) + wg - 1) / wg;
    return std::max(1LL, std::min(groups, worst));
}

long long scheduled_groups(int compute_units, int per_cu, int tile_count) {
    long long groups = (long long)compute_units * per_cu;
    if (const int forced = switches::scheduled_waves_per_simd()) groups = groups_of_waves_per_simd(compute_units, forced, 64);
    return std::max(1LL, std::min(groups, (long long)tile_count));
}

long long compact_groups(int compute_units, long long tiles) {
    const int wg = 256;
    return std::min<long long>((tiles * 64 + wg - 1) / wg, (long long)compute_units * 32 * 64 / wg);
}

}   // namespace trace_plan
