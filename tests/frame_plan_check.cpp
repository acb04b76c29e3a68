// frame_plan_check.cpp — the decision table of csrc/frame_plan.cpp (tests/test_frame_plan.py compiles this file together with it, with the
// host compiler and its sanitizers, and compares the lines printed here with the expectations written there).  No HIP, no library.
#include <cstdio>
#include <cstring>

#include "../geodesic_raytracing_amd/csrc/frame_plan.hpp"

using namespace frame_plan;

// gr_tile_order_bytes (csrc/trace_launch.cpp) restated: 32 header words, one id and one class per tile of the device's row blocks
static long long order_bytes(int width, int height, int block_rows, int strip_rank, int strip_count) {
    if (strip_count <= 1) { strip_count = 1; strip_rank = 0; block_rows = ((height + 7) / 8) * 8; }
    long long blocks = 0;
    for (int b = 0; b * block_rows < height; b++) blocks += b % strip_count == strip_rank;
    const long long per_block = (long long)((width + 7) / 8) * (block_rows / 8) + (strip_count > 1 ? (width + 63) / 64 : 0);
    return (32 + 2 * per_block * blocks) * 4;
}

static bool g_busy = false, g_asked = false;

static gr_frame_tuning default_tuning() {   // gr_frame_tuning_default (csrc/frame.cpp, which needs HIP)
    gr_frame_tuning t{};
    t.ray_compaction = t.fused_shading = t.inline_prepass = t.tile_history = t.park_lanes = t.next_strip_rank = t.next_strip_rank2 = -1;
    t.guess_still_camera = t.reuse_still_camera = t.speculative_classes = -1;
    return t;
}

static void turn(gr_camera& c, float x, float y, float z, float w) { c.quat[0] = x; c.quat[1] = y; c.quat[2] = z; c.quat[3] = w; }

// 256 x 256 (prepass grid 16 x 16), fused, prepass on, Cartesian camera, not prefetched, default tuning, device idle, enough wave slots,
// the tile order buffer of gr_render_state_create
static fused_input base(bool has_pair) {
    fused_input in;
    in.width = in.height = 256;
    in.use_prepass = true;
    in.out = true;
    in.tune = default_tuning();
    in.has_pair = has_pair;
    in.wave_slots = [] { return 4096LL; };
    in.tile_order_bytes = order_bytes;
    in.earlier_frame_still_running = [] { g_asked = true; return g_busy; };
    in.tile_order_bytes_held = ((size_t)256 * 256 / 16 + 2 * 256 + 8192) * sizeof(unsigned int);
    in.camera.position[2] = -4.f;   // gr_camera_default
    turn(in.camera, -0.70710677f, 0, 0, 0.70710677f);
    in.tile_cost_camera = in.camera;
    in.field_of_view = 90.f;
    return in;
}

static void history_of(fused_input& in, int block_rows) {   // a whole frame's, recorded by the same camera with the origin on screen
    in.tile_cost_valid = in.tile_cost_anchored = true;
    in.tile_cost_shape[0] = block_rows; in.tile_cost_shape[1] = 0; in.tile_cost_shape[2] = 1;
}

static void row(const char* name, const fused_input& in, bool busy = false) {
    g_busy = busy; g_asked = false;
    const fused_plan q = plan_fused(in);
    if (q.refused.code != GR_OK) {
        printf("%s: refused=%s asked=%d \"%s\"\n", name, q.refused.code == GR_ERROR_INVALID_ARGUMENT ? "INVALID_ARGUMENT" : "?", g_asked, q.refused.message);
        return;
    }
    printf("%s: rays_per_lane=%d keep_lanes=%d history_wanted=%d guesses_wanted=%d asked=%d record_history=%d invalidate=%d order_capable=%d "
           "inline_prepass=%d order_tiles=%d history_order=%d shape={%d,%d,%d} history=%dx%d margin=%d\n",
           name, q.rays_per_lane, q.keep_lanes, q.history_wanted, q.guesses_wanted, g_asked, q.record_history, q.invalidate_tile_cost, q.order_capable,
           q.inline_prepass, q.order_tiles, q.history_order, q.shape[0], q.shape[1], q.shape[2], q.hist_width, q.hist_height, q.prepass_margin);
}

int main() {
    { fused_input in = base(true); history_of(in, 256); row("1 pair", in); }
    { fused_input in = base(false); row("2 no pair, no history yet", in); history_of(in, 256); row("2 no pair, history", in); }
    { fused_input in = base(false); history_of(in, 256); row("3 busy", in, true); }
    { fused_input in = base(false); in.strip_count = 2; in.strip_rank = 1; in.block_rows = 16; row("4 share", in); }
    { fused_input in = base(true); in.adaptive = true; row("5 pair, adaptive", in); }
    { fused_input in = base(false); in.adaptive = true; row("6 no pair, adaptive", in); }
    { fused_input in = base(false); history_of(in, 256); in.tune.tile_history = 0; row("7 tile_history=0", in); }
    // the camera turned about z by 0.38 and by 0.51: gr_picture_motion of the commit before gives 48.6399994 and 65.2799988 px at 90 degrees, 256 wide
    { fused_input in = base(false); history_of(in, 256);
      turn(in.camera, -0.694381833f, -0.133543402f, 0.133543402f, 0.694381833f);
      printf("8 motion: %.9g\n", picture_motion(in.tile_cost_camera, in.camera, 90.f, 256)); row("8 turned 48.64 px", in);
      turn(in.camera, -0.684241295f, -0.178364441f, 0.178364441f, 0.684241295f);
      printf("8 motion: %.9g\n", picture_motion(in.tile_cost_camera, in.camera, 90.f, 256)); row("8 turned 65.28 px", in); }
    { fused_input in = base(false); in.adaptive = true; in.tune.ray_compaction = 8; row("9 adaptive, ray_compaction", in); }
    { fused_input in = base(true); in.adaptive = true; in.tune.rays_per_lane = 2; row("9 adaptive, rays_per_lane=2", in); }
    { fused_input in = base(false); in.adaptive = true; in.tune.fused_shading = 1; row("9 adaptive, fused_shading", in); }
    { fused_input in = base(false); in.tune.rays_per_lane = 2; row("9 rays_per_lane=2, no pair", in); }
    { fused_input in = base(false); in.prefetched = true; row("10 prefetched", in); }
    { fused_input in = base(false); in.use_prepass = false; row("11 no prepass", in); }
    { fused_input in = base(false); in.width = 8; in.use_prepass = false; row("12 width 8", in); }
    { fused_input in = base(false); in.tile_order_bytes_held = 1024; row("13 small order buffer", in); }
    return 0;
}
