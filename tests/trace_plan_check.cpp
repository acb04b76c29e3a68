// trace_plan_check.cpp — the decision table of csrc/trace_plan.cpp (tests/test_trace_plan.py compiles this file together with it, with the
// host compiler and its sanitizers, and compares the lines printed here with the expectations written there).  No HIP, no library.
#include <cstdio>
#include <cstdlib>

#include "../geodesic_raytracing_amd/csrc/trace_plan.hpp"

using namespace trace_plan;

static int g_asked = 0, g_per_cu = 8, g_status = GR_OK;
static int g_cells[1], g_order[1], g_cost[1], g_rays[1], g_guessed[1], g_records[1], g_words[1], g_pixels[1];   // stand for device buffers: never read

// a whole frame traced by gr_trace_fused on a device of 256 compute units that holds 8 workgroups of the kernel per unit; every kernel there is
static trace_input frame(int width, int height) {
    trace_input in;
    in.args.width = width; in.args.height = height; in.args.strip_count = 1; in.args.lattice = 1;
    in.program.compute_units = 256;
    in.program.has_pair = in.program.has_parking = in.program.tile_shading = true;
    in.resident_per_cu = [](int, int, int* per_cu) { g_asked++; *per_cu = g_per_cu; return g_status; };
    return in;
}

static trace_input split(int width, int height, int block_rows, int rank, int count) {
    trace_input in = frame(width, height);
    in.args.block_rows = block_rows; in.args.strip_rank = rank; in.args.strip_count = count;
    return in;
}

static trace_input with_prepass(trace_input in, int prepass_width, int prepass_height) {
    in.args.inline_prepass = 1;
    in.args.termination_buffer = g_cells;
    in.args.prepass_width = prepass_width; in.args.prepass_height = prepass_height;
    return in;
}

static trace_input by_history(trace_input in) { in.args.tile_order = g_order; in.args.tile_order_by_history = 1; return in; }
static trace_input parked(trace_input in) { in.args.parking = {g_records, g_words, 16, 512, 4096, 100}; return in; }
static trace_input shaded(trace_input in) { in.args.shading.out = g_pixels; in.args.shading.compact_out = 1; in.args.shading.max_probes = 7; return in; }

static void row(const char* name, const trace_input& in) {
    g_asked = 0;
    const auto q = plan_trace(in);
    if (q.refused.code != GR_OK) {
        if (q.refused.message) printf("%s: refused asked=%d code=%d \"%s\"\n", name, g_asked, q.refused.code, q.refused.message);
        else printf("%s: refused asked=%d code=%d no text\n", name, g_asked, q.refused.code);
        return;
    }
    if (q.nothing) { printf("%s: nothing asked=%d\n", name, g_asked); return; }
    const char* kernel = q.kernel == K_TRACE_FUSED ? "fused" : q.kernel == K_TRACE_PAIR ? "pair" : q.kernel == K_TRACE_FUSED_LATTICE ? "lattice"
                       : q.kernel == K_TRACE_FUSED_PARKING ? "parking" : "?";
    printf("%s: %s wg=%d grid=%u tiles=%d ticket=%d ticket_tiles=%d prepass_tickets=%d strips=%d/%d/%d word=%d resets=%zu/%zu/%zu asked=%d\n", name, kernel, q.wg,
           q.grid, q.total_waves, q.ticket, q.ticket_tiles, q.prepass_tickets, q.block_rows, q.strip_rank, q.strip_count, q.last_class_is_skipped,
           q.termination_bytes, q.tile_cost_bytes, q.lot_words_bytes, g_asked);
    if (q.shading.out || q.lot.records)
        printf("%s: shading out=%d probes=%d compact=%d lot=%d/%d/%d/%d/%d/%d\n", name, q.shading.out == g_pixels, q.shading.most_probes, q.shading.compact_out,
               q.lot.records == g_records, q.lot.words == g_words, q.lot.lanes, q.lot.trips, q.lot.slots, q.lot.groups);
}

static void strip_row(const char* name, int height, int block_rows, int rank, int count) {
    printf("%s:", name);
    for (whole_frame_block whole : {HEIGHT_ROUNDED_UP_TO_8, EIGHT_ROWS, THE_HEIGHT}) {
        const strip_share s = strips(height, block_rows, rank, count, whole);
        if (s.bad) printf(" bad");
        else printf(" %d/%d/%d", s.block_rows, s.strip_rank, s.strip_count);
    }
    printf("\n");
}

static void parse_row(const char* name, std::initializer_list<const char*> texts) {
    printf("%s:", name);
    for (const char* text : texts) printf(" %d", switches::parse(name, text));
    printf("\n");
}

int main() {
    trace_input in;
    // ---------------------------------------------------------------- whole frames
    row("64 x 64", frame(64, 64));
    in = frame(64, 64); in.rays_per_lane = 2;
    row("64 x 64, two rays per lane", in);
    in = frame(64, 64); in.args.lattice = 2;
    row("64 x 64, lattice 2", in);
    row("60 x 60", frame(60, 60));
    row("3840 x 2160", frame(3840, 2160));
    in = frame(3840, 2160); in.args.waves_per_simd = 1;
    row("3840 x 2160, waves_per_simd 1", in);
    in.args.waves_per_simd = 9;
    row("3840 x 2160, waves_per_simd 9", in);
    in.args.waves_per_simd = 1; in.program.compute_units = 64;
    row("3840 x 2160, 64 compute units, waves_per_simd 1", in);
    in = frame(64, 64); in.args.tile_cost = g_cost;
    row("64 x 64, tile_cost", in);
    in = frame(64, 64); in.args.lattice = 2; in.args.guessed = g_guessed;
    row("64 x 64, lattice 2, guessed", in);
    // ---------------------------------------------------------------- split frames
    row("split, rank 0", split(64, 64, 16, 0, 2));
    row("split, rank 1", split(64, 64, 16, 1, 2));
    row("split, height 65", split(64, 65, 16, 0, 2));
    row("split, a rank without blocks", split(64, 16, 16, 1, 2));
    row("no width", frame(0, 64));
    // ---------------------------------------------------------------- the prepass inside the launch
    row("prepass 20 x 12", with_prepass(frame(64, 64), 20, 12));
    in = with_prepass(frame(64, 64), 20, 12); in.program.cell_rows = true;
    row("prepass 20 x 12, cell_rows", in);
    row("prepass, history order", by_history(with_prepass(frame(64, 64), 20, 12)));
    row("prepass, history order, parking", parked(by_history(with_prepass(frame(64, 64), 20, 12))));
    row("history order, no prepass", by_history(frame(64, 64)));
    in = by_history(with_prepass(frame(64, 64), 20, 12));
    in.args.speculative_classes = -1; row("prepass, history order, speculative_classes -1", in);
    in.args.speculative_classes = 3; row("prepass, history order, speculative_classes 3", in);
    in.args.speculative_classes = 20; row("prepass, history order, speculative_classes 20", in);
    // ---------------------------------------------------------------- which kernel
    row("kernel parking", parked(frame(64, 64)));
    in = frame(64, 64); in.args.lattice = 2; in.args.lattice_rays = g_rays;
    row("kernel lattice with rays", in);
    row("kernel fused, shading", shaded(frame(64, 64)));
    row("kernel fused, shading, split", shaded(split(64, 64, 16, 1, 2)));
    // ---------------------------------------------------------------- refusals, in the launcher's order
    in = with_prepass(frame(64, 64), 20, 12); in.args.tile_order = g_order;
    row("refused 1, prepass with gr_order_tiles' list", in);
    row("refused 1, prepass grid as wide as the image", with_prepass(frame(64, 64), 64, 12));
    in = frame(64, 64); in.args.lattice = 0;
    row("refused 2, lattice 0", in);
    in = frame(64, 64); in.args.pending_only = 1; in.rays_per_lane = 2;
    row("refused 2, pending_only, two rays per lane", in);
    in = parked(frame(64, 64)); in.program.has_parking = false;
    row("refused 3, parking without the kernel", in);
    row("refused 4, parking with shading", shaded(parked(frame(64, 64))));
    in = parked(frame(64, 64)); in.args.parking.slots = 63;
    row("refused 5, a lot of 63 slots", in);
    in = frame(64, 64); in.rays_per_lane = 2; in.program.has_pair = false;
    row("refused 6, no pair kernel", in);
    row("refused 7, block_rows 12", split(64, 64, 12, 0, 2));
    row("refused 7, rank 2 of 2", split(64, 64, 16, 2, 2));
    row("refused 7, no height", frame(64, 0));
    row("refused 8, the last row starts a block", split(64, 33, 16, 0, 2));
    row("refused 9, too many tiles", frame(1 << 20, 1 << 20));
    in = shaded(frame(64, 64)); in.program.tile_shading = false;
    row("refused 10, shading without the build option", in);
    row("refused 11, shading, 60 x 64", shaded(frame(60, 64)));
    in = frame(64, 64); in.args.tile_cost = g_cost; in.args.pending_only = 1;
    row("refused 12, tile_cost, pending_only", in);
    in = split(64, 64, 16, 0, 2); in.args.tile_cost = g_cost; in.args.lattice = 2;
    row("refused 12, tile_cost, lattice 2 of a split frame", in);
    g_status = GR_ERROR_DEVICE;
    row("refused 13, the device does not answer", frame(64, 64));
    g_status = GR_OK;
    // ---------------------------------------------------------------- two faults: the earlier one
    in = with_prepass(frame(64, 64), 20, 12); in.rays_per_lane = 2; in.program.has_pair = false;
    row("two faults, 1 and 6", in);
    in = shaded(split(64, 64, 12, 0, 2)); in.program.tile_shading = false;
    row("two faults, 7 and 10", in);
    in = shaded(frame(64, 64)); in.program.tile_shading = false; in.args.tile_cost = g_cost; in.args.pending_only = 1;
    row("two faults, 10 and 12", in);
    in = shaded(split(64, 16, 16, 1, 2)); in.program.tile_shading = false;
    row("an empty share with fault 10", in);
    // ---------------------------------------------------------------- the strip rule, under the three conventions
    strip_row("strips whole frame of 60 rows", 60, 0, 5, 1);
    strip_row("strips count 0", 60, 16, 0, 0);
    strip_row("strips 12 rows, rank 1 of 2", 60, 12, 1, 2);
    strip_row("strips no rows to a block", 60, 0, 0, 2);
    strip_row("strips rank 2 of 2", 60, 16, 2, 2);
    strip_row("strips rank -1", 60, 16, -1, 2);
    strip_row("strips whole frame without rows", 0, 16, 0, 1);
    printf("device tiles: %lld %lld %lld %lld %lld\n", device_tiles(64, 64, strips(64, 0, 0, 1, HEIGHT_ROUNDED_UP_TO_8)),
           device_tiles(60, 60, strips(60, 0, 0, 1, HEIGHT_ROUNDED_UP_TO_8)), device_tiles(64, 64, strips(64, 16, 1, 2, HEIGHT_ROUNDED_UP_TO_8)),
           device_tiles(100, 40, strips(40, 8, 2, 3, HEIGHT_ROUNDED_UP_TO_8)), device_tiles(0, 64, strips(64, 0, 0, 1, HEIGHT_ROUNDED_UP_TO_8)));
    // ---------------------------------------------------------------- the other persistent launches: 2 x 2, 64 x 64, 3840 x 2160
    printf("pending groups: %lld %lld %lld %lld\n", pending_groups(256, 8, 0, 2, 2), pending_groups(256, 8, 0, 64, 64), pending_groups(256, 8, 0, 3840, 2160),
           pending_groups(256, 8, 1, 3840, 2160));
    printf("scheduled groups: %lld %lld %lld\n", scheduled_groups(256, 32, 1), scheduled_groups(256, 32, 64), scheduled_groups(256, 32, 129600));
    printf("compact groups: %lld %lld %lld\n", compact_groups(256, 1), compact_groups(256, 64), compact_groups(256, 129600));
    // ---------------------------------------------------------------- switches
    printf("switches unset: %d %d %d %d %d %d %d\n", switches::trace_block(), switches::trace_persistent(), switches::trace_waves_per_simd(), switches::ticket_tiles(),
           switches::speculative_classes(), switches::tile_history_reach(), switches::scheduled_waves_per_simd());
    parse_row("GR_TRACE_BLOCK", {nullptr, "64", "128", "256", "96", "512", "0"});
    parse_row("GR_TRACE_PERSISTENT", {nullptr, "0", "1", "", "00", "no"});
    parse_row("GR_TRACE_WAVES_PER_SIMD", {nullptr, "1", "8", "0", "9"});
    parse_row("GR_TICKET_TILES", {nullptr, "1", "64", "0", "65"});
    parse_row("GR_SPECULATIVE_CLASSES", {nullptr, "0", "14", "15", "-1"});
    parse_row("GR_TILE_HISTORY_REACH", {nullptr, "0", "8", "9", "-1"});
    parse_row("GR_SCHEDULED_WAVES_PER_SIMD", {nullptr, "1", "8", "0", "9"});
    // six are read once: set now, they stay as they were first read; GR_TICKET_TILES is read by every plan that draws a ticket
    setenv("GR_TRACE_BLOCK", "64", 1); setenv("GR_TRACE_PERSISTENT", "0", 1); setenv("GR_TRACE_WAVES_PER_SIMD", "2", 1); setenv("GR_SPECULATIVE_CLASSES", "9", 1);
    setenv("GR_TILE_HISTORY_REACH", "4", 1); setenv("GR_SCHEDULED_WAVES_PER_SIMD", "3", 1); setenv("GR_TICKET_TILES", "16", 1);
    printf("switches set after their first reading: %d %d %d %d %d %d %d\n", switches::trace_block(), switches::trace_persistent(), switches::trace_waves_per_simd(),
           switches::ticket_tiles(), switches::speculative_classes(), switches::tile_history_reach(), switches::scheduled_waves_per_simd());
    row("3840 x 2160, GR_TICKET_TILES=16", frame(3840, 2160));
    row("64 x 64, GR_TICKET_TILES=16", frame(64, 64));
    setenv("GR_TICKET_TILES", "65", 1);
    row("3840 x 2160, GR_TICKET_TILES=65", frame(3840, 2160));
    return 0;
}
