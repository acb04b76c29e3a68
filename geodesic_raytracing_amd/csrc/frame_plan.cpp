// frame_plan.cpp — the decisions of a frame (frame_plan.hpp).  No HIP call, no state written: inputs in, plan out.
#include "frame_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// library defaults of gr_frame_tuning.tile_history = -1 and of gr_frame_options.rays_per_lane = 0 (see include/geodesic_hip.h)
#ifndef GR_DEFAULT_TILE_HISTORY
#define GR_DEFAULT_TILE_HISTORY 1
#endif
#ifndef GR_DEFAULT_RAYS_PER_LANE
#define GR_DEFAULT_RAYS_PER_LANE 2   /* where the program has gr_trace_pair (program_build.cpp: pair_kernel_applies) */
#endif

namespace frame_plan {

namespace switches {
namespace {
const char* env(const char* name) { return getenv(name); }
bool on_unless_0(const char* name) { const char* e = env(name); return !(e && e[0] == '0'); }      // default on
bool flag(const char* name, bool unset) { const char* e = env(name); return !e ? unset : e[0] != '0'; }
float number(const char* name, float unset) { const char* e = env(name); return e ? (float)atof(e) : unset; }
}   // namespace

// The prepass rays' costs order the tiles of the trace, longest first (gr_order_tiles).  Default: on a device's share of a split frame
// (+8 % with three frames in flight, +35 % one frame at a time, one of 8 devices), not on a whole frame (there image order measured
// 2 % faster); GR_TILE_ORDER=0 never, =1 always.
int tile_order() { static const int v = [] { const char* e = env("GR_TILE_ORDER"); return !e ? -1 : e[0] == '0' ? 0 : 1; }(); return v; }
bool reuse_still_camera() { static const bool v = flag("GR_REUSE_STILL_CAMERA", true); return v; }
// Default: whole frames that find the device idle when they are submitted (they record their costs, and follow those of the frame
// before if that one did too).  Not frames of more than 32 tiles per wave slot (8K Alcubierre: 72 short tiles of much the same cost;
// recording and sorting them measured +3 % on the frame, with nothing to gain).
bool tile_history() { static const bool v = flag("GR_TILE_HISTORY", GR_DEFAULT_TILE_HISTORY != 0); return v; }
// An adaptively sampled whole frame: the same for its lattice launch - the tiles of the half-resolution grid, their costs left by the
// lattice launch of the frame before (GR_LATTICE_HISTORY=0: image order as before round 6's fifth session).  Only for the metrics with a
// prepass - the ones with a shadow and long rays along its edge: there the launch gains by its speculative tiles when it traces
// its own cells, and by the order alone where it is long (4K Kerr a = 0.9, prepass reused: 12.2 -> 9.1 ms); recording + sorting cost
// the 0.4 ms frames of the metrics without a prepass 5-10 %.
bool lattice_history() { static const bool v = on_unless_0("GR_LATTICE_HISTORY"); return v; }
bool adaptive_guess() { static const bool v = on_unless_0("GR_ADAPTIVE_GUESS"); return v; }
// library default: no compaction (the benchmark workloads keep > 95 % of their lanes busy without it); experiments can switch it on
// for every frame with GR_TRACE_COMPACT=<keep_lanes>
int trace_compact() { static const int v = [] { const char* e = env("GR_TRACE_COMPACT"); int k = e ? atoi(e) : 0; return (k >= 1 && k <= 64) ? k : 0; }(); return v; }
int trace_rays_per_lane() {
    static const int v = [] { const char* e = env("GR_TRACE_RAYS_PER_LANE"); int k = e ? atoi(e) : 0; return (k == 1 || k == 2) ? k : GR_DEFAULT_RAYS_PER_LANE; }();
    return v;
}
// By default on whole frames that do not order their tiles (the order needs the prepass rays' costs first).  A device's share of a
// split frame can do it too (inline_prepass = 1: it traces the cells its rows look at), but does not by default, on measurement - one
// rank of 8 / of 4, one frame at a time, 2 wave slots per SIMD: 2.41 / 3.42 ms against 2.20 / 2.80 with the prepass in front and the
// tiles ordered by its costs (tools/strip_probe.py, STRIP_PROBE_DEPTH=0): a share is few tiles, and which of them start first matters
// more than the prepass's latency.
bool inline_prepass() { static const bool v = flag("GR_INLINE_PREPASS", true); return v; }
// A history the picture has moved more than 48 px away from is not followed: a wrong order is worse than none (a camera rolling 5
// degrees a frame, 170 px at the edge: 4K Kerr 7.8 -> 13.4 ms, a = 0.9 27 -> 85 ms following it blindly; up to 43 px - 0.08 units
// sideways or 1 degree of roll a frame - it measured a gain or nothing).
float tile_history_max_motion() { static const float v = number("GR_TILE_HISTORY_MAX_MOTION", 48.f); return v; }
// ... or, when the camera mostly TURNED (mouse look: the picture shifts rigidly and the order shifts with it as long as both frames see
// the coordinate origin), up to this many px of turn with at most the 48 px of parallax: 1.5 degrees a frame at 4K (50 px) rendered in
// 6.23 ms with the history dropped and in 5.24 with it (a = 0.9: 24.0 and 21.9), 2.2 degrees (73 px) in 6.36 and 5.50 (24.4 and 23.3);
// at 3 degrees (100 px) the a = 0.9 frame loses badly (23.9 -> 33.8 ms: the shift is the picture centre's, a perspective picture moves by
// 1 / cos^2 more towards its edges, and beyond the guard ring of 48 px tiles guessed empty are dear): 64 px.
float tile_history_max_turn() { static const float v = number("GR_TILE_HISTORY_MAX_TURN", 64.f); return v; }
bool tile_history_follow() { static const bool v = on_unless_0("GR_TILE_HISTORY_FOLLOW"); return v; }
bool guess_still_camera() { static const bool v = flag("GR_GUESS_STILL_CAMERA", false); return v; }
// (a guess is a PIXEL: it is right when the picture has not moved - a viewer whose user is looking, or dragging a slider - and a ray
// traced for nothing otherwise: used up to half a pixel of motion)
float adaptive_guess_max_motion() { static const float v = number("GR_ADAPTIVE_GUESS_MAX_MOTION", 0.5f); return v; }
bool adaptive_pending_list() { static const bool v = on_unless_0("GR_ADAPTIVE_PENDING_LIST"); return v; }
float adaptive_history_max_motion() { static const float v = number("GR_ADAPTIVE_HISTORY_MAX_MOTION", 48.f); return v; }
int park_lanes() { static const int v = [] { const char* e = env("GR_PARK"); return e ? atoi(e) : 0; }(); return v; }
int park_trips() { static const int v = [] { const char* e = env("GR_PARK"); const char* c = e ? strchr(e, ',') : nullptr; return c ? atoi(c + 1) : 0; }(); return v; }
// Rays in tile slot order are traced the way the fused kernel's tiles are (round 5: in slot order, a workgroup to a tile, the 4K Kerr
// launch took 6.1 ms against the fused trace's 4.8 - the difference was the tail).  =0: the reference's own launch shape.
bool reference_scheduled() { static const bool v = on_unless_0("GR_REFERENCE_SCHEDULED"); return v; }
}   // namespace switches

static double focal_length(float fov_degrees, int width) { return (width / 2.0) / std::tan(fov_degrees / 360.0 * M_PI); }

// Between two frames of a moving or turning camera the picture of whatever sits at the origin - the hole, the bubble, the throat, which
// is where the dear tiles are - moves by about as much as this point does (the inverse of the kernels' pixel_direction); false if the
// origin is behind the camera or the camera sits on it.
bool origin_on_screen(const gr_camera& c, float fov_degrees, int width, int height, float out[2]) {
    const double px = c.position[1], py = c.position[2], pz = c.position[3];
    const double r = std::sqrt(px * px + py * py + pz * pz);
    double qx = c.quat[0], qy = c.quat[1], qz = c.quat[2], qw = c.quat[3];
    const double qn = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    if (!(r > 1e-6) || !(qn > 1e-6)) return false;
    qx = -qx / qn; qy = -qy / qn; qz = -qz / qn; qw /= qn;   // the inverse rotation: world -> camera
    const double d[3] = {-px / r, -py / r, -pz / r};
    const double t[3] = {2 * (qy * d[2] - qz * d[1]), 2 * (qz * d[0] - qx * d[2]), 2 * (qx * d[1] - qy * d[0])};
    const double v[3] = {d[0] + qw * t[0] + (qy * t[2] - qz * t[1]), d[1] + qw * t[1] + (qz * t[0] - qx * t[2]),
                         d[2] + qw * t[2] + (qx * t[1] - qy * t[0])};
    if (!(v[2] > 0.05)) return false;
    const double f_stop = focal_length(fov_degrees, width);
    out[0] = (float)(width / 2.0 + f_stop * v[0] / v[2]);
    out[1] = (float)(height / 2.0 + f_stop * v[1] / v[2]);
    return std::isfinite(out[0]) && std::isfinite(out[1]);
}

// What both estimates are made of: the angle between the two orientations, the parallax of the origin as a ratio, the focal length.
// A turn of the camera moves the picture rigidly (the history's shift follows it), a step moves it by parallax.
namespace {
struct motion_terms { double angle, parallax_ratio, f_stop; };
bool motion_between(const gr_camera& a, const gr_camera& b, float fov_degrees, int width, motion_terms& m) {
    double dot = 0, na = 0, nb = 0, dp = 0, r = 0;
    for (int i = 0; i < 4; i++) { dot += (double)a.quat[i] * b.quat[i]; na += (double)a.quat[i] * a.quat[i]; nb += (double)b.quat[i] * b.quat[i]; }
    for (int i = 1; i < 4; i++) { dp += ((double)a.position[i] - b.position[i]) * ((double)a.position[i] - b.position[i]); r += (double)b.position[i] * b.position[i]; }
    if (!(na > 0) || !(nb > 0)) return false;
    if (a.flip != b.flip || memcmp(a.basis_speed, b.basis_speed, sizeof(a.basis_speed)) != 0) return false;
    m.angle = 2 * std::acos(std::min(1.0, std::fabs(dot) / std::sqrt(na * nb)));
    m.parallax_ratio = std::sqrt(dp) / std::max(std::sqrt(r), 1e-3);
    m.f_stop = focal_length(fov_degrees, width);
    return true;
}
}   // namespace

bool picture_motion_parts(const gr_camera& a, const gr_camera& b, float fov_degrees, int width, float& turn_px, float& parallax_px) {
    turn_px = parallax_px = 1e9f;
    motion_terms m;
    if (!motion_between(a, b, fov_degrees, width, m)) return false;
    const double turn = m.angle * m.f_stop, parallax = m.parallax_ratio * m.f_stop;
    if (!std::isfinite(turn) || !std::isfinite(parallax)) return false;
    turn_px = (float)turn; parallax_px = (float)parallax;
    return true;
}

float picture_motion(const gr_camera& a, const gr_camera& b, float fov_degrees, int width) {
    motion_terms m;
    if (!motion_between(a, b, fov_degrees, width, m)) return 1e9f;
    const double motion = (m.angle + m.parallax_ratio) * m.f_stop;
    return std::isfinite(motion) ? (float)motion : 1e9f;
}

// A frame on the fused path.  In the order gr_render_frame has always decided, refusals included: the first that applies is reported.
fused_plan plan_fused(const fused_input& in) {
    fused_plan q;
    const gr_frame_tuning& tune = in.tune;
    const int width = in.width, height = in.height, prepass_width = width / 16, prepass_height = height / 16;   // main.cpp:2380-2381
    const bool adaptive = in.adaptive, use_prepass = in.use_prepass;
    const int strip_count = q.strip_count = in.strip_count > 1 ? in.strip_count : 1;
    const int strip_rank = q.strip_rank = strip_count > 1 ? in.strip_rank : 0;
    const int block_rows = q.block_rows = strip_count > 1 ? in.block_rows : ((height + 7) / 8) * 8;
    // fused mode with a Cartesian camera: camera set-up and prepass are one call (gr_camera_prepass)
    const bool one_launch_setup = !in.geodesic;
    const int tile_order_mode = switches::tile_order();
    const bool history_default = switches::tile_history(), lattice_history = switches::lattice_history();
    // the other source of an order: what the tiles of this state's previous frame cost (gr_order_tiles_by_history); an adaptive frame's
    // history is that of its lattice launch, over the half-resolution grid
    q.hist_width = adaptive ? width / 2 : width; q.hist_height = adaptive ? height / 2 : height;
    q.hist_block_rows = adaptive ? ((q.hist_height + 7) / 8) * 8 : block_rows;
    const long long hist_bytes = in.tile_order_bytes(q.hist_width, q.hist_height, q.hist_block_rows, strip_rank, strip_count);
    q.history_wanted = (tune.tile_history < 0 ? history_default && strip_count == 1 && hist_bytes / 8 <= 32 * in.wave_slots() : tune.tile_history != 0) &&
                       (!adaptive || (lattice_history && strip_count == 1 && use_prepass)) && (size_t)hist_bytes <= in.tile_order_bytes_held;
    // (the pixels traced ahead for the second launch of adaptive sampling are for such lone frames too, prepass or not)
    q.guesses_wanted = switches::adaptive_guess() && adaptive && strip_count == 1 && !in.geodesic && tune.tile_history != 0 && history_default;
    q.device_busy = (q.history_wanted || q.guesses_wanted) && tune.tile_history < 0 && in.earlier_frame_still_running();
    const bool tile_order_enabled = !q.history_wanted && (tile_order_mode == 1 || (tile_order_mode == -1 && strip_count > 1));
    q.cells = use_prepass ? (size_t)prepass_width * prepass_height : 0;
    // (a frame whose prepass rides in its trace launch has no costs to order by; the frames it announces still do)
    q.order_capable = tile_order_enabled && use_prepass && !adaptive && 2 * q.cells <= (size_t)width * height &&
                      (size_t)in.tile_order_bytes(width, height, block_rows, strip_rank, strip_count) <= in.tile_order_bytes_held;
    q.prepass_margin = adaptive ? 2 : 0;   // the lattice rows beyond a block that its 2x2 decisions read
    // which trace kernel this frame takes (needed here already: the prepass may ride in the trace launch)
    const int default_compaction = switches::trace_compact();
    q.keep_lanes = tune.ray_compaction < 0 ? default_compaction : tune.ray_compaction;
    // What does not combine is refused, not silently dropped: ray compaction and the two-rays-per-lane kernel trace every
    // pixel (no lattice / pending-only form), in-tile shading needs every pixel's record in its own tile's wave.
    auto refuse = [&](const char* message) { q.refused = {GR_ERROR_INVALID_ARGUMENT, message}; return q; };
    if (adaptive && tune.ray_compaction > 0)
        return refuse("ray_compaction > 0 with adaptive sampling: gr_trace_compact traces every pixel (switch one of them off)");
    if (adaptive && tune.rays_per_lane == 2)
        return refuse("rays_per_lane = 2 with adaptive sampling: gr_trace_pair traces every pixel (switch one of them off)");
    if (tune.fused_shading == 1 && (adaptive || q.keep_lanes > 0 || tune.rays_per_lane == 2))
        return refuse("fused_shading = 1 needs one ray per lane, no compaction and no adaptive sampling");
    if (adaptive) q.keep_lanes = 0;   // GR_TRACE_COMPACT (an experiment switch for every frame) does not apply to adaptive frames
    // two rays per lane (gr_trace_pair) where the program has that kernel, unless told otherwise - on an adaptive frame too, whose
    // launches never are that kernel's ("How a frame is sequenced")
    const int default_rays_per_lane = switches::trace_rays_per_lane();
    q.rays_per_lane = tune.rays_per_lane == 1 || tune.rays_per_lane == 2 ? tune.rays_per_lane : default_rays_per_lane;
    if (q.rays_per_lane == 2 && !in.has_pair) {
        if (tune.rays_per_lane == 2) return refuse("rays_per_lane = 2: this program has no gr_trace_pair kernel");
        q.rays_per_lane = 1;
    }
    // The prepass inside the trace launch (gr_trace_fused_args.inline_prepass): for a frame whose prepass was not computed
    // ahead of time - an interactive caller does not know the next camera - the prepass's single-ray latency (1.1 ms at 4K
    // Kerr, 8 ms with a = 0.9) then runs alongside the first tiles instead of in front of the whole trace.
    const bool inline_default = switches::inline_prepass();
    const bool inline_wanted = tune.inline_prepass < 0 ? (inline_default && strip_count == 1 && !q.order_capable) : tune.inline_prepass != 0;
    // (an adaptively sampled whole frame: the cells ride in front of the lattice launch's tiles)
    q.inline_prepass = inline_wanted && !in.prefetched && one_launch_setup && use_prepass && (!adaptive || strip_count == 1) && q.keep_lanes == 0 &&
                       q.rays_per_lane == 1 && prepass_width != width && prepass_height != height;
    q.order_tiles = q.order_capable && !q.inline_prepass;
    // (the kernels that record and follow the history are gr_trace_fused's: one ray per lane, no compaction)
    q.record_history = q.history_wanted && !q.device_busy && q.keep_lanes == 0 && q.rays_per_lane == 1;
    q.invalidate_tile_cost = q.history_wanted && !q.record_history;   // (what is there would be older than the last frame)
    const int shape[3] = {adaptive ? -q.hist_block_rows : block_rows, strip_rank, strip_count};   // (negative: the tiles of a lattice launch)
    memcpy(q.shape, shape, sizeof(shape));
    const float max_motion = switches::tile_history_max_motion(), max_turn = switches::tile_history_max_turn();
    q.history_order = q.record_history && in.tile_cost_valid && memcmp(shape, in.tile_cost_shape, sizeof(shape)) == 0 && !in.geodesic && [&] {
        if (picture_motion(in.tile_cost_camera, in.camera, in.field_of_view, width) <= max_motion) return true;
        float turn = 0, parallax = 0, anchor[2];
        return picture_motion_parts(in.tile_cost_camera, in.camera, in.field_of_view, width, turn, parallax) && parallax <= max_motion &&
               turn <= max_turn && in.tile_cost_anchored && origin_on_screen(in.camera, in.field_of_view, width, height, anchor);
    }();
    // gr_trace_fused on every pixel: parking (gr_trace_fused_parking) and in-tile shading; what these refuse, the launch refuses
    if (q.keep_lanes > 0 || adaptive || q.rays_per_lane != 1) return q;
    q.park_lanes = tune.park_lanes < 0 ? switches::park_lanes() : tune.park_lanes;
    q.park_trips = tune.park_trips > 0 ? tune.park_trips : switches::park_trips() > 0 ? switches::park_trips() : 512;
    q.parking = q.park_lanes > 1 && tune.fused_shading != 1 && in.has_parking;
    // the trace shades the pixels whose filter neighbours are in their own tile; gr_render_seams does the rest (default: off, on measurement)
    q.shade_in_trace = in.out && tune.fused_shading == 1 && width % 8 == 0 && height % 8 == 0 && in.has_tile_shading;
    if (tune.park_lanes > 1 && !in.has_parking)
        q.refused_at_trace = {GR_ERROR_INVALID_ARGUMENT, "park_lanes: needs a program built with -DGR_PARKING appended to its argument string"};
    else if (tune.fused_shading == 1 && !q.shade_in_trace && in.out)
        q.refused_at_trace = {GR_ERROR_INVALID_ARGUMENT, "fused_shading = 1: needs a program built with -DGR_TILE_SHADING and width, height multiples of 8"};
    return q;
}

}   // namespace frame_plan
