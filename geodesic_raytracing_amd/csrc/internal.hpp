// internal.hpp — what the library's translation units share and no caller sees: the gr_internal_* calls between them, one HIP_CHECK and
// one GR_CHECK, and the little of a program (capi.cpp) that a file outside capi.cpp needs to launch its kernels.  No HIP header: the host-only
// files (png_stream.cpp, exr_stream.cpp, jpeg_stream.cpp, imageio.cpp) include it and compile alone; the macros name HIP only where they are expanded.
#pragma once

#include <initializer_list>
#include <string>

#include "../../include/geodesic_hip_internal.h"

extern "C" {
int gr_internal_fail(int code, const char* msg);   // capi.cpp: the text behind gr_last_error; returns code
int gr_internal_check_analytic_sky(const char* who, const gr_analytic_sky* sky);   // shading.cpp: what every taker of a sky refuses
int gr_internal_check_star_sky(const char* who, const gr_star_sky* sky, const gr_star_catalogue* near, const gr_star_catalogue* far, const gr_program* p);   // star_catalogue.cpp
int gr_internal_render_state_size(const gr_render_state* s, int* width, int* height);   // frame.cpp
const char* gr_internal_filter_table_error(int factor, const float* taps, int count);   // imageio.cpp: NULL for nothing wrong
int gr_internal_check_tone(const char* who, const gr_tone* t);   // imageio.cpp: what every taker of a tone refuses about its fields
void gr_internal_tone_gain(double adapted_stops, float* gain, int* q);   // imageio.cpp: section 2's gain, for a manual tone too
float gr_internal_tone_inverse_white_squared(const gr_tone* t);   // imageio.cpp: iw2 of the Reinhard curve, as gr_tone_frame takes it
int gr_internal_check_glare(const char* who, const gr_glare* g);   // imageio.cpp: what every taker of a glare refuses about its fields
// frame.cpp: gr_render_frame and its three encoded kin by the format's value (tiled.cpp renders a share through it)
int gr_internal_render_frame_as(int format, int layout, gr_render_state* s, gr_program* p, const gr_metric* m, void* stream, const gr_camera* camera,
                                const gr_features* features, const float* cfg_values, int num_cfg_values, const void* bg1, const void* bg2,
                                int bg_width, int bg_height, int bg_levels, void* out, const gr_frame_options* options);
}

#define HIP_CHECK(expr)                                                                                            \
    do {                                                                                                           \
        hipError_t _e = (expr);                                                                                    \
        if (_e != hipSuccess)                                                                                      \
            return gr_internal_fail(GR_ERROR_DEVICE, (std::string(#expr) + ": " + hipGetErrorString(_e)).c_str()); \
    } while (0)
#define GR_CHECK(expr)                \
    do {                              \
        int _rc = (expr);             \
        if (_rc != GR_OK) return _rc; \
    } while (0)
#define GR_NEED(who, ...) GR_CHECK(gr_internal::need(who, {__VA_ARGS__}))

// a program's kernels, in the order of capi.cpp's KERNEL_NAMES
enum KernelId {
    K_CART_TO_GENERIC, K_INIT_BASIS, K_CLEAR_TERM, K_INIT_RAYS, K_DO_RAYS, K_CALC_SING, K_CALC_RDATA,
    K_ADAPTIVE, K_RENDER, K_TRACE_FUSED, K_TRACE_FUSED_LATTICE, K_TRACE_PAIR, K_TRACE_COMPACT, K_PREPASS_FUSED, K_CAMERA_SETUP, K_ORDER_TILES, K_ADAPTIVE_REFINE, K_TRACE_PENDING, K_APPLY_GUESSED, K_DO_RAYS_SCHEDULED, K_SORT_TILES_COUNT, K_SORT_TILES_PLACE, K_TRACE_FUSED_PARKING, K_BOOST_TETRAD, K_INIT_INERTIAL, K_GEODESIC_PATH, K_PARALLEL_TRANSPORT,
    K_INTERPOLATE_GEODESIC, K_RESOLVE_SUPERSAMPLED, K_PRESENT_RGBA8, K_BACKGROUND_REDUCE, K_BACKGROUND_SLICES, K_PRESENT_YUV420, K_PRESENT_YUV420P10, K_SHUTTER_ACCUMULATE, K_RESOLVE_FILTERED, K_PNG_HISTOGRAM, K_PNG_PACK, K_JPEG_BLOCKS, K_JPEG_PACK, K_JPEG_GATHER, K_PNG_HISTOGRAM_RUNS, K_PNG_PACK_RUNS, K_RENDER_ANALYTIC,
    K_RENDER_STARS, K_STARS_COUNT, K_STARS_SCAN, K_STARS_SCATTER, K_STARS_ORDER, K_STARS_GATHER, K_STARS_SUMS, K_STARS_PREFIX,
    K_GLARE_ROWS, K_GLARE_COLUMNS, K_GLARE_SCALE, K_EXR_HISTOGRAM, K_EXR_PACK,
    K_METER_HISTOGRAM, K_METER_SOLVE, K_TONE_APPLY, K_COUNT
};

namespace gr_internal __attribute__((visibility("hidden"))) {   // (not among the library's exported names)
// what a refusal() of png_stream, exr_stream, jpeg_stream said - or any refusal in words - as a status, the caller's name in front
inline int refuse(const std::string& who, const std::string& wrong, bool too_small = false) {
    return gr_internal_fail(too_small ? GR_ERROR_BUFFER_TOO_SMALL : GR_ERROR_INVALID_ARGUMENT, (who + ": " + wrong).c_str());
}
// capi.cpp: kernel k of the program on `stream` (a hipStream_t), an empty grid launches nothing; the program's device
int launch(gr_program* p, int k, void* stream, unsigned gx, unsigned gy, unsigned bx, unsigned by, void** args);
int device_of(const gr_program* p);
const void* no_count_of(const gr_program* p);   // the device int INT_MAX that a range launch hands its kernel as the records' count
inline unsigned blocks(long long n, int b) { return n <= 0 ? 0u : (unsigned)((n + b - 1) / b); }
// capi.cpp, for the trace launchers (trace_launch.cpp, which decides by trace_plan.hpp): what a plan needs to know of a program ...
struct program_facts {
    int compute_units = 0;
    bool cell_rows = false, tile_shading = false;    // built with -DGR_CELL_BLOCK=0, with -DGR_TILE_SHADING
    bool has_pair = false, has_parking = false;      // gr_trace_pair, gr_trace_fused_parking
};
program_facts facts_of(const gr_program* p);
// ... the workgroups of `wg` lanes of kernel k that one compute unit holds at once (asked of the runtime once per kernel; where it
// does not say, 4 SIMDs x 8 waves: 4 * 8 * 64 / wg); GR_OK or the status, its text set ...
int resident_groups_per_cu(gr_program* p, int k, int wg, int* per_cu);
// ... and the counter of a launch by ticket: the next one of the program's ring, zeroed on `stream` (the device set)
int draw_ticket(gr_program* p, void* stream, unsigned int** ticket);
// A launcher refuses a NULL where its kernel dereferences unconditionally: the reference's clSetKernelArg returns CL_INVALID_MEM_OBJECT
// for a null buffer, a HIP launch takes it and the device faults (and a device fault ends the process).  cfg / dfg are not checked:
// a substituted program reads neither.
inline int need(const char* who, std::initializer_list<const void*> buffers) {
    for (const void* b : buffers)
        if (!b) return gr_internal_fail(GR_ERROR_INVALID_ARGUMENT, (std::string(who) + ": a required buffer is NULL").c_str());
    return GR_OK;
}
// what gr_render_stars takes of a catalogue, by value (star_catalogue_view of kernels/shading.hip, field for field)
struct catalogue_view {
    const int* cell_start;
    const void* stars;
    const double* table;
    int n, cells_u, cells_v;
};
catalogue_view view_of(const gr_star_catalogue* c);   // star_catalogue.cpp; a NULL catalogue: n = 0 and no pointers
}  // namespace gr_internal
