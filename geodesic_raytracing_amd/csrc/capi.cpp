// capi.cpp — the C ABI of libgeodesic_hip.so (include/geodesic_hip.h): metric -> macro string on the
// host, macro string -> gfx950 code object through hiprtc, and one launcher per reference kernel.
//
// Reference counterparts: metric_manager.hpp:19-219 (program build + cache), main.cpp:139-205 and
// 2244-2526 (the launches).  HIP is used directly (module API); there is no fallback of any kind:
// without libamdhip64/hiprtc or without a device the calls fail with GR_ERROR_DEVICE/COMPILE.
#include "../../include/geodesic_hip_internal.h"

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <hip/hiprtc.h>
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "builtin_metrics.hpp"
#include "codeobject.hpp"
#include "internal.hpp"
#include "jsfront.hpp"
#include "metric_codegen.hpp"
#include "program_build.hpp"

namespace {

thread_local std::string g_error;

int fail(gr_status code, const std::string& msg) {
    g_error = msg;
    return (int)code;
}

#define GR_TRY_BEGIN try {
#define GR_TRY_END                                                                 \
    }                                                                              \
    catch (const std::exception& e) { return fail(GR_ERROR_SCRIPT, e.what()); }    \
    catch (...) { return fail(GR_ERROR_SCRIPT, "unknown exception"); }

std::string library_dir() {
    Dl_info info;
    if (dladdr((void*)&gr_last_error, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.rfind('/');
        if (s != std::string::npos) return p.substr(0, s);
    }
    return ".";
}

const char* const KERNEL_NAMES[] = {
    "gr_cart_to_generic", "gr_init_basis_vectors", "gr_clear_termination_buffer", "gr_init_rays_generic",
    "gr_do_generic_rays", "gr_calculate_singularities", "gr_calculate_render_data",
    "gr_handle_adaptive_sampling", "gr_render", "gr_trace_fused", "gr_trace_fused_lattice", "gr_trace_pair", "gr_trace_compact", "gr_prepass_fused", "gr_camera_setup", "gr_order_tiles", "gr_adaptive_refine", "gr_trace_pending", "gr_apply_guessed", "gr_do_generic_rays_scheduled", "gr_sort_tiles_count", "gr_sort_tiles_place", "gr_trace_fused_parking", "gr_boost_tetrad", "gr_init_inertial_ray",
    "gr_get_geodesic_path", "gr_parallel_transport_quantity", "gr_handle_interpolating_geodesic", "gr_resolve_supersampled", "gr_present_rgba8",
    "gr_background_reduce", "gr_background_slices", "gr_present_yuv420", "gr_present_yuv420p10", "gr_shutter_accumulate", "gr_resolve_filtered", "gr_png_histogram", "gr_png_pack",
    "gr_jpeg_blocks", "gr_jpeg_pack", "gr_jpeg_gather", "gr_png_histogram_runs", "gr_png_pack_runs", "gr_render_analytic",
    "gr_render_stars", "gr_stars_count", "gr_stars_scan", "gr_stars_scatter", "gr_stars_order", "gr_stars_gather", "gr_stars_sums", "gr_stars_prefix",
    "gr_glare_rows", "gr_glare_columns", "gr_glare_scale", "gr_exr_histogram", "gr_exr_pack",
    "gr_meter_histogram", "gr_meter_solve", "gr_tone_apply"};

// the kernels of the set-up module (kernels/camera.hip, geodesic_camera.hip): once per frame, one lane, IEEE arithmetic - and the box
// filter of a supersampled frame (kernels/resolve.hip), its 8-bit sRGB and 8- and 10-bit Y'CbCr 4:2:0 encodes (kernels/present.hip) and the sky's mip slices
// (kernels/background.hip), which want the same arithmetic and no part in the ray kernels' compilation - and the two integer kernels of the
// PNG encoder (kernels/png.hip; each in two instances, one a stream kind) and the three of the JPEG encoder (kernels/jpeg.hip), which want
// no part in it either - and the seven that build a star catalogue (kernels/stars.hip), whose sums are taken in the order they are written -
// and the three of the glare (kernels/glare.hip), which are held to a host definition bit for bit - and the two integer kernels of the
// EXR encoder (kernels/exr.hip), which use the PNG encoder's bit-packer - and the three of the meter and the tone curve (kernels/tone.hip),
// held to host statements exactly
bool is_setup_kernel(int k) {
    return k == K_CART_TO_GENERIC || k == K_INIT_BASIS || k == K_CAMERA_SETUP || k == K_BOOST_TETRAD || k == K_INIT_INERTIAL ||
           k == K_GEODESIC_PATH || k == K_PARALLEL_TRANSPORT || k == K_INTERPOLATE_GEODESIC || k == K_RESOLVE_SUPERSAMPLED || k == K_PRESENT_RGBA8 ||
           k == K_BACKGROUND_REDUCE || k == K_BACKGROUND_SLICES || k == K_PRESENT_YUV420 || k == K_PRESENT_YUV420P10 || k == K_SHUTTER_ACCUMULATE || k == K_RESOLVE_FILTERED ||
           k == K_PNG_HISTOGRAM || k == K_PNG_PACK || k == K_JPEG_BLOCKS || k == K_JPEG_PACK || k == K_JPEG_GATHER || k == K_PNG_HISTOGRAM_RUNS ||
           k == K_PNG_PACK_RUNS || (k >= K_STARS_COUNT && k <= K_STARS_PREFIX) || k == K_GLARE_ROWS || k == K_GLARE_COLUMNS || k == K_GLARE_SCALE || k == K_EXR_HISTOGRAM ||
           k == K_EXR_PACK || k == K_METER_HISTOGRAM || k == K_METER_SOLVE || k == K_TONE_APPLY;
}

namespace pb = program_build;   // what a build decides: switches, options, source lists, keys, the occupancy rule, the cache files
using pb::PART_FRAME;
using pb::PART_REST;

// hiprtc's version (part of every cache key), asked once per process: the first call into hiprtc initialises the HIP runtime behind it,
// and two threads doing that at the same moment (the two builds of build_frame_path) left one of them without a device on the GPU box
// ("hipSetDevice: no ROCm-capable device is detected" in the first program a process created)
void rtc_version(int& major, int& minor) {
    static int v[2] = {0, 0};
    static std::once_flag once;
    std::call_once(once, [] { hiprtcVersion(&v[0], &v[1]); });
    major = v[0];
    minor = v[1];
}

// the fallback of both modules' builds: hiprtc itself (no pass over the code; a source error shows up here with its diagnostics)
int build_through_hiprtc(const std::string& source, const char* name, const std::vector<std::string>& options, std::string& out) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, source.c_str(), name, 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail(GR_ERROR_COMPILE, "hiprtcCreateProgram failed");
    std::vector<const char*> copts;
    for (auto& o : options) copts.push_back(o.c_str());
    hiprtcResult r = hiprtcCompileProgram(prog, (int)copts.size(), copts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        return fail(GR_ERROR_COMPILE, std::string("hiprtc: ") + hiprtcGetErrorString(r) + "\n" + log);
    }
    size_t n = 0;
    hiprtcGetCodeSize(prog, &n);
    out.assign(n, '\0');
    hiprtcGetCode(prog, &out[0]);
    hiprtcDestroyProgram(&prog);
    return GR_OK;
}

// One build of the ray kernels' source with `options`: through the assembly pass when it is on and the code-object manager is
// there, else through hiprtc (a source error shows up there with its diagnostics).  pass_not_applied is set where the build goes out
// as compiled although the pass is on.
int build_ray_kernels(const std::string& source, const std::vector<std::string>& options, int run_limit, std::string& out, bool& pass_not_applied) {
    const bool verbose = pb::switches::verbose_build();
    // (GR_VECTOR_RUN_LIMIT=0 goes the same way without the pass: which code-object manager hiprtc would find depends on
    // what else the process has loaded, and the copy bundled with PyTorch aborts on these kernels)
    std::string assembly, log;
    if (gr::compile_to_assembly(source, options, assembly, log)) {
        if (run_limit <= 0 && gr::assemble_code_object(assembly, out, log)) return GR_OK;
        // the kernels that hold a Verlet loop; the others (set-up, shading, tile order ...) are left as compiled
        static const std::vector<std::string> integrators = {"gr_trace_fused", "gr_trace_fused_lattice", "gr_trace_pair", "gr_trace_compact", "gr_prepass_fused",
                                                             "gr_do_generic_rays", "gr_do_generic_rays_scheduled", "gr_trace_fused_parking"};
        std::string patched = assembly;
        const gr::vector_run_stats st = gr::break_vector_runs(patched, run_limit, integrators);
        if (gr::assemble_code_object(patched, out, log)) {
            if (verbose)
                fprintf(stderr, "[gr] vector runs: %d longer than %d (longest %d) cut by %d s_nop, longest now %d\n", st.runs_broken,
                        run_limit, st.longest_before, st.inserted, st.longest_after);
            return GR_OK;
        }
        // The compiler sized its branches for the code it emitted; in a very large function the added instructions can push
        // one past the 16-bit branch offset ("branch size exceeds simm16").  Then the code as compiled.
        if (verbose) fprintf(stderr, "[gr] assembly pass not applied (%s)\n", log.c_str());
        pass_not_applied = true;
        if (gr::assemble_code_object(assembly, out, log)) return GR_OK;
    }
    if (run_limit > 0) pass_not_applied = true;
    if (verbose) fprintf(stderr, "[gr] building through hiprtc (%s)\n", log.c_str());
    return build_through_hiprtc(source, "geodesic_kernels_all_parts.hip", options, out);
}

// Compiles (or fetches from the on-disk cache) one code object of the ray kernels for one macro string (program_build.hpp: the two
// parts).  cache_only: an empty `code` and GR_OK when the part is not in the cache (the caller builds it later, or on another thread).
int compile_code_object(const std::string& argument_string, std::string& code, std::string* key_out = nullptr, pb::build_part part = PART_FRAME,
                        bool cache_only = false) {
    std::string source;
    const std::string unreadable = pb::read_source(pb::RAY_KERNELS, library_dir() + "/csrc/kernels", source);
    if (!unreadable.empty()) return fail(GR_ERROR_COMPILE, unreadable);
    const pb::option_list made = pb::options(argument_string, pb::RAY_KERNELS, part);
    if (!made.refusal.empty()) return fail(GR_ERROR_INVALID_ARGUMENT, made.refusal);
    const std::vector<std::string>& opts = made.options;
    int rtc_major = 0, rtc_minor = 0;
    rtc_version(rtc_major, rtc_minor);
    const int run_limit = pb::switches::vector_run_limit();
    const bool tuning = pb::switches::occupancy_tuning();
    const std::string name = pb::code_object_name(source, opts, rtc_major, rtc_minor, run_limit, tuning);
    if (key_out) key_out->assign(name, 0, 16);
    const std::string cache_dir = pb::cache_dir(library_dir()), cache_path = cache_dir + "/" + name;
    if (pb::fetch(cache_path, code) || cache_only) return GR_OK;

    bool pass_not_applied = false;   // some build of this call went out as compiled although the pass is on
    auto build = [&](const std::vector<std::string>& options, std::string& out) { return build_ray_kernels(source, options, run_limit, out, pass_not_applied); };
    // free, or held to fewer registers by the occupancy rule - whose decision is remembered per shape of program, next to the code objects
    const bool rule_applies = pb::occupancy_rule_applies(opts, part, tuning);
    const std::string shape_path = cache_dir + "/" + pb::shape_name(source, opts, rtc_major, rtc_minor, run_limit);
    std::string note;
    const bool remembered = rule_applies && pb::fetch(shape_path, note);
    const pb::occupancy_outcome built = pb::build_by_occupancy_rule(opts, rule_applies, remembered ? &note : nullptr, build, [&] { return pass_not_applied; }, code);
    if (pb::switches::verbose_build())
        for (auto& line : built.lines) fprintf(stderr, "%s\n", line.c_str());
    if (built.rc != GR_OK) return built.rc;
    if (!built.note.empty()) pb::publish(shape_path, built.note);

    if (pass_not_applied) {
        // The cache key says "vector runs <= N"; this code object does not have them cut (a branch pushed past its 16-bit offset, or
        // the code-object manager could not be loaded and hiprtc built it).  It is used but not cached under that key: a later
        // process in which the pass can run builds it properly instead of being served this one for good.
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "[gr] warning: the pass over the compiled code (vector runs <= %d) could not be applied to a program; it runs as "
                            "compiled (~20 %% slower Verlet loop) and is not cached.  GR_VERBOSE_BUILD=1 says why.\n", run_limit);
        return GR_OK;
    }
    pb::publish(cache_path, code);
    return GR_OK;
}

// The set-up module of a program: the kernels that run once per frame on one lane - camera coordinates, tetrad, the camera's own
// geodesic - from program + probes + metric + setup + camera + geodesic_camera, built with IEEE arithmetic (kernels/camera.hip says
// why).  Same macro string, a cache file of its own; no pass over the code, no occupancy rule: nothing here is issue-bound.
// The table kernels/present.hip searches, as source text: gr_srgb8_thresholds' T[1 ... 255] (imageio.cpp - the host encode inverted with
// the host's own powf) as bit patterns, in the breadth-first order of the perfect search tree over them (node i: children 2i and 2i + 1;
// entry 0 unused).  Part of the set-up module's source, so of its cache key: a host whose libm rounds differently builds its own.
const std::string& srgb8_tree_source() {
    static const std::string text = [] {
        float sorted[256];
        uint32_t tree[256] = {};
        (void)gr_srgb8_thresholds(sorted);
        for (int level = 0; level < 8; level++)   // entry j of level l is the (2 j + 1) 2^(7 - l)-th threshold in sorted order
            for (int j = 0; j < (1 << level); j++) memcpy(&tree[(1 << level) + j], &sorted[(2 * j + 1) << (7 - level)], sizeof(uint32_t));
        std::string t = "__device__ const unsigned int GR_SRGB8_TREE_BITS[256] = {";
        char word[32];
        for (int i = 0; i < 256; i++) {
            snprintf(word, sizeof(word), "%s0x%08xu", i ? (i % 8 ? ", " : ",\n    ") : "\n    ", tree[i]);
            t += word;
        }
        return t + "};\n";
    }();
    return text;
}

// The same for gr_present_yuv420p10: gr_srgb10_thresholds' T[1 ... 1023], ten levels
const std::string& srgb10_tree_source() {
    static const std::string text = [] {
        static float sorted[1024];
        static uint32_t tree[1024] = {};
        (void)gr_srgb10_thresholds(sorted);
        for (int level = 0; level < 10; level++)   // entry j of level l is the (2 j + 1) 2^(9 - l)-th threshold in sorted order
            for (int j = 0; j < (1 << level); j++) memcpy(&tree[(1 << level) + j], &sorted[(2 * j + 1) << (9 - level)], sizeof(uint32_t));
        std::string t = "__device__ const unsigned int GR_SRGB10_TREE_BITS[1024] = {";
        char word[32];
        for (int i = 0; i < 1024; i++) {
            snprintf(word, sizeof(word), "%s0x%08xu", i ? (i % 8 ? ", " : ",\n    ") : "\n    ", tree[i]);
            t += word;
        }
        return t + "};\n";
    }();
    return text;
}

int compile_setup_module(const std::string& argument_string, std::string& code, bool cache_only = false) {
    std::string source;
    const std::string unreadable = pb::read_source(pb::SETUP_MODULE, library_dir() + "/csrc/kernels", source);
    if (!unreadable.empty()) return fail(GR_ERROR_COMPILE, unreadable);
    if (!pb::switches::setup_kernel_source() && pb::switches::kernel_source()) {
        // (so that nobody takes a patched metric.hip to reach the camera kernels)
        static std::atomic<bool> said{false};
        if (!said.exchange(true))
            fprintf(stderr, "[gr] note: GR_KERNEL_SOURCE replaces the ray kernels' source only; the set-up module (camera, tetrad, geodesic camera) is built "
                            "from the library's csrc/kernels - GR_SETUP_KERNEL_SOURCE replaces that\n");
    }
    source = srgb8_tree_source() + srgb10_tree_source() + source;
    const pb::option_list made = pb::options(argument_string, pb::SETUP_MODULE, PART_FRAME);
    if (!made.refusal.empty()) return fail(GR_ERROR_INVALID_ARGUMENT, made.refusal);
    const std::vector<std::string>& opts = made.options;
    int rtc_major = 0, rtc_minor = 0;
    rtc_version(rtc_major, rtc_minor);
    const std::string cache_path = pb::cache_dir(library_dir()) + "/" + pb::setup_module_name(source, opts, rtc_major, rtc_minor);
    if (pb::fetch(cache_path, code) || cache_only) return GR_OK;
    std::string assembly, log;
    if (!gr::compile_to_assembly(source, opts, assembly, log) || !gr::assemble_code_object(assembly, code, log)) {
        // the code-object manager could not be loaded (or is the copy bundled with another library): hiprtc, as for the ray kernels'
        // module - this module needs no pass over its code, so the result is the same program and is cached like any other
        if (pb::switches::verbose_build()) fprintf(stderr, "[gr] set-up module: building through hiprtc (%s)\n", log.c_str());
        const int rc = build_through_hiprtc(source, "geodesic_setup_kernels.hip", opts, code);
        if (rc != GR_OK) return rc;
    }
    pb::publish(cache_path, code);
    return GR_OK;
}

}  // namespace

struct gr_metric {
    gr::MetricConfig cfg;
    gr::MetricFunctions functions;
    gr::DynamicVars vars;
    gr::MetricDescriptor desc;
    std::shared_ptr<void> keepalive;   // script interpreter state owning the closures
    bool settings_only = false;        // gr_metric_from_info: no symbolic content, only what the frame driver reads
    gr_metric_info stored_info = {};
};

struct gr_program {
    int device = 0;
    hipModule_t module = nullptr;
    hipModule_t setup_module = nullptr;   // camera / tetrad / geodesic-camera kernels, IEEE arithmetic (compile_setup_module)
    hipFunction_t fn[K_COUNT] = {};
    void* huge_count = nullptr;   // device int = INT_MAX: "no device-side count" for range launches
    // tile tickets of the persistent fused trace: one counter per launch, taken round robin from a small ring so that
    // launches in flight on different streams never share one
    static const int TICKET_RING = 64;
    unsigned int* tickets = nullptr;
    std::atomic<unsigned> next_ticket{0};
    int compute_units = 256;
    bool tile_shading = false;   // built with -DGR_TILE_SHADING: gr_trace_fused can shade the inner pixels of its tiles
    bool cell_rows = false;      // built with -DGR_CELL_BLOCK=0: a cell wave of an in-launch prepass is 64 cells of a row, not 8 x 8 cells
    int resident_groups_per_cu[K_COUNT] = {};   // of the trace kernels at the launch's workgroup size: 0 = not asked yet
    // The kernels a fused frame does not launch (PART_REST) are a code object of their own, loaded when first asked for: from the
    // cache when gr_program_create found it there, else from a build that started on a worker thread when the program was created.
    // Whoever asks first (launch of such a kernel, gr_program_kernel_info, gr_program_complete) waits for that build.
    struct rest_build {
        std::mutex mu;
        std::condition_variable cv;
        bool done = false;
        int rc = GR_OK;
        std::string code, error;
    };
    std::shared_ptr<rest_build> rest;     // shared with the worker, which may outlive the program
    std::thread rest_worker;
    std::mutex rest_mu;                   // serialises the load
    bool rest_loaded = false;
    int rest_rc = GR_OK;
    std::string rest_error;
    hipModule_t module_rest = nullptr;
    bool in_rest[K_COUNT] = {};           // kernels expected in the other code object
    std::string arguments;
    std::string key;   // what the code object was built from: kernel source, every compile option, hiprtc version (16 hex digits)
    // identity for caches keyed by program (frame.cpp prefetch slots): an address can be reused by a later program, this cannot
    unsigned long long serial = 0;
    ~gr_program() {
        if (module || tickets || huge_count) (void)hipSetDevice(device);
        if (tickets) (void)hipFree(tickets);
        if (huge_count) (void)hipFree(huge_count);
        if (module) (void)hipModuleUnload(module);
        if (module_rest) (void)hipModuleUnload(module_rest);
        if (setup_module) (void)hipModuleUnload(setup_module);
        // a build still inside the compiler cannot be interrupted; it holds its own state (rest_build) and is left to finish
        if (rest_worker.joinable()) {
            bool done;
            { std::lock_guard<std::mutex> lock(rest->mu); done = rest->done; }
            if (done) rest_worker.join(); else rest_worker.detach();
        }
    }
};

extern "C" {

const char* gr_last_error(void) { return g_error.c_str(); }

void gr_features_default(gr_features* f) {
    if (!f) return;
    // main.cpp:1123-1158
    f->adaptive_sampling_threshold = 64.f;
    f->field_of_view = 90.f;
    f->max_acceleration_change = 0.01f;
    f->max_precision_radius = 10.f;
    f->min_step = 0.000001f;
    f->ray_skip = 4.f;
    f->universe_size = 20.f;
    f->adaptive_sampling = 1;
    f->redshift = 0;
    f->reparameterisation = 0;
    f->use_old_redshift = 0;
    f->use_triangle_rendering = 0;
}

static gr::FeatureConfig to_feature_config(const gr_features* f) {
    gr_features d;
    gr_features_default(&d);
    if (f) d = *f;
    gr::FeatureConfig c;
    c.set("adaptive_sampling_threshold", d.adaptive_sampling_threshold);
    c.set("field_of_view", d.field_of_view);
    c.set("max_acceleration_change", d.max_acceleration_change);
    c.set("max_precision_radius", d.max_precision_radius);
    c.set("min_step", d.min_step);
    c.set("ray_skip", d.ray_skip);
    c.set("universe_size", d.universe_size);
    c.set("adaptive_sampling", d.adaptive_sampling != 0);
    c.set("redshift", d.redshift != 0);
    c.set("reparameterisation", d.reparameterisation != 0);
    c.set("use_old_redshift", d.use_old_redshift != 0);
    c.set("use_triangle_rendering", d.use_triangle_rendering != 0);
    return c;
}

int gr_metric_builtin(const char* name, gr_metric** out) {
    if (!name || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    GR_TRY_BEGIN
    auto m = std::make_unique<gr_metric>();
    if (!gr::builtin_metric(name, m->cfg, m->functions, m->vars))
        return fail(GR_ERROR_INVALID_ARGUMENT, std::string("unknown built-in metric ") + name);
    m->desc.load(m->functions, m->cfg);
    *out = m.release();
    return GR_OK;
    GR_TRY_END
}

int gr_metric_load_script(const char* scripts_dir, const char* name, gr_metric** out) {
    if (!scripts_dir || !name || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    GR_TRY_BEGIN
    auto m = std::make_unique<gr_metric>();
    m->keepalive = gr::load_metric_from_scripts(scripts_dir, name, m->cfg, m->functions, m->vars);
    m->desc.load(m->functions, m->cfg);
    *out = m.release();
    return GR_OK;
    GR_TRY_END
}

int gr_metric_from_info(const gr_metric_info* info, const char* const* var_names, const float* var_defaults, gr_metric** out) {
    if (!info || !out || info->num_dynamic_vars < 0 || (info->num_dynamic_vars > 0 && !var_defaults))
        return fail(GR_ERROR_INVALID_ARGUMENT, "gr_metric_from_info: null argument");
    GR_TRY_BEGIN
    auto m = std::make_unique<gr_metric>();
    m->settings_only = true;
    m->stored_info = *info;
    for (int i = 0; i < info->num_dynamic_vars; i++) {
        m->vars.names.push_back(var_names && var_names[i] ? var_names[i] : "v" + std::to_string(i));
        m->vars.defaults.push_back(var_defaults[i]);
    }
    *out = m.release();
    return GR_OK;
    GR_TRY_END
}

void gr_metric_destroy(gr_metric* m) { delete m; }

int gr_metric_get_info(const gr_metric* m, gr_metric_info* out) {
    if (!m || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    if (m->settings_only) { *out = m->stored_info; return GR_OK; }
    out->is_big = m->desc.is_big;
    out->is_constant_theta = m->desc.is_spherical && m->cfg.system == gr::CoordinateSystem::X_Y_THETA_PHI;
    out->use_prepass = m->cfg.use_prepass;
    out->adaptive_precision = m->cfg.adaptive_precision;
    out->max_acceleration_change = m->cfg.max_acceleration_change;
    out->num_dynamic_vars = (int)m->vars.names.size();
    out->accel_ops = m->desc.accel_ops.ops;
    out->accel_transcendentals = m->desc.accel_ops.transcendental;
    out->coord_ops = m->desc.coord_ops.ops;
    return GR_OK;
}

const char* gr_metric_dynamic_var_name(const gr_metric* m, int i) {
    if (!m || i < 0 || i >= (int)m->vars.names.size()) return nullptr;
    return m->vars.names[i].c_str();
}

float gr_metric_dynamic_var_default(const gr_metric* m, int i) {
    if (!m || i < 0 || i >= (int)m->vars.defaults.size()) return 0.f;
    return m->vars.defaults[i];
}

int gr_metric_argument_string(const gr_metric* m, const gr_features* features, int is_static, const float* cfg_values,
                              int num_cfg_values, char* buffer, size_t capacity, size_t* needed) {
    if (!m) return fail(GR_ERROR_INVALID_ARGUMENT, "null metric");
    if (m->settings_only) return fail(GR_ERROR_INVALID_ARGUMENT, "a metric made by gr_metric_from_info has no expressions to generate from");
    GR_TRY_BEGIN
    gr::FeatureConfig fc = to_feature_config(features);
    std::string s;
    if (is_static) {
        std::vector<float> vals(cfg_values, cfg_values + (cfg_values ? num_cfg_values : 0));
        gr::MetricImpl concrete = m->desc.concrete(m->vars.substitution(vals));
        s = gr::build_argument_string(m->desc, concrete, m->cfg, m->vars, true, fc);
    } else {
        s = gr::build_argument_string(m->desc, m->desc.raw, m->cfg, m->vars, false, fc);
    }
    if (needed) *needed = s.size() + 1;
    if (!buffer && capacity == 0 && needed) return GR_OK;   // size query
    if (!buffer || capacity < s.size() + 1) return fail(GR_ERROR_BUFFER_TOO_SMALL, "buffer too small");
    memcpy(buffer, s.c_str(), s.size() + 1);
    return GR_OK;
    GR_TRY_END
}

int gr_metric_evaluate_count(int what) {
    switch (what) {
        case GR_EVAL_METRIC_TENSOR: return 16;
        case GR_EVAL_METRIC_DERIVATIVES: return 64;
        case GR_EVAL_ACCELERATION: case GR_EVAL_TO_POLAR: case GR_EVAL_FROM_POLAR: return 4;
        case GR_EVAL_ORIGIN_DISTANCE: return 1;
        default: return 0;
    }
}

// The host-side evaluator of the generated expressions: sym::eval over the metric's DAGs (the same graphs build_argument_string prints),
// position / velocity / $cfg bound by name.  One point per call; a graph node is visited once per call (memoised).
int gr_metric_evaluate(const gr_metric* m, int what, const double position[4], const double velocity[4], const float* cfg_values,
                       int num_cfg_values, double* out, int out_count) {
    if (!m || !position || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "gr_metric_evaluate: null argument");
    if (m->settings_only) return fail(GR_ERROR_INVALID_ARGUMENT, "a metric made by gr_metric_from_info has no expressions to evaluate");
    const int count = gr_metric_evaluate_count(what);
    if (count == 0) return fail(GR_ERROR_INVALID_ARGUMENT, "gr_metric_evaluate: unknown kind");
    if (out_count < count) return fail(GR_ERROR_BUFFER_TOO_SMALL, "gr_metric_evaluate: out_count too small");
    if (what == GR_EVAL_ACCELERATION && !velocity) return fail(GR_ERROR_INVALID_ARGUMENT, "gr_metric_evaluate: the acceleration needs a velocity");
    if (cfg_values && num_cfg_values != (int)m->vars.names.size())
        return fail(GR_ERROR_INVALID_ARGUMENT, "gr_metric_evaluate: num_cfg_values is not the metric's number of $cfg parameters");
    GR_TRY_BEGIN
    std::map<std::string, double> env;
    static const char* const pos_names[4] = {"v1", "v2", "v3", "v4"};
    static const char* const vel_names[4] = {"iv1", "iv2", "iv3", "iv4"};
    for (int i = 0; i < 4; i++) {
        env[pos_names[i]] = position[i];
        env[vel_names[i]] = velocity ? velocity[i] : 0.0;
    }
    for (size_t i = 0; i < m->vars.names.size(); i++)
        env["cfg->" + m->vars.names[i]] = cfg_values ? (double)cfg_values[i] : (double)m->vars.defaults[i];
    env["always_lightlike"] = 0.0;
    const gr::MetricImpl& impl = m->desc.raw;
    auto eval_all = [&](const std::vector<sym::E>& v, double* dst) { for (size_t i = 0; i < v.size(); i++) dst[i] = sym::eval(v[i], env); };
    switch (what) {
        case GR_EVAL_METRIC_TENSOR:
            for (int i = 0; i < 16; i++) out[i] = 0.0;
            if (impl.real_eq.size() == 4) { for (int i = 0; i < 4; i++) out[i * 4 + i] = sym::eval(impl.real_eq[(size_t)i], env); }
            else eval_all(impl.real_eq, out);
            break;
        case GR_EVAL_METRIC_DERIVATIVES:
            for (int i = 0; i < 64; i++) out[i] = 0.0;
            if (impl.derivatives.size() == 16) { for (int k = 0; k < 4; k++) for (int i = 0; i < 4; i++) out[k * 16 + i * 4 + i] = sym::eval(impl.derivatives[(size_t)(k * 4 + i)], env); }
            else eval_all(impl.derivatives, out);
            break;
        case GR_EVAL_ACCELERATION: eval_all(impl.accel, out); break;
        case GR_EVAL_TO_POLAR: eval_all(impl.to_polar, out); break;
        case GR_EVAL_FROM_POLAR: eval_all(impl.from_polar, out); break;
        case GR_EVAL_ORIGIN_DISTANCE: {   // DISTANCE_FUNC is a function of the POLAR point (kernels/metric.hip distance_to_object): composed with TO_COORDn here
            double polar[4];
            eval_all(impl.to_polar, polar);
            for (int i = 0; i < 4; i++) env[pos_names[i]] = polar[i];
            out[0] = sym::eval(impl.distance_function, env);
            break;
        }
    }
    return GR_OK;
    GR_TRY_END
}

int gr_metric_substituted_op_counts(const gr_metric* m, const float* cfg_values, int num_cfg_values, int* accel_ops,
                                    int* accel_transcendentals, int* coord_ops) {
    if (!m) return fail(GR_ERROR_INVALID_ARGUMENT, "null metric");
    if (m->settings_only) return fail(GR_ERROR_INVALID_ARGUMENT, "a metric made by gr_metric_from_info has no expressions to count");
    GR_TRY_BEGIN
    std::vector<float> vals(cfg_values, cfg_values + (cfg_values ? num_cfg_values : 0));
    const gr::MetricImpl concrete = m->desc.concrete(m->vars.substitution(vals));
    const sym::OpCount accel = sym::count_ops(concrete.accel);
    std::vector<sym::E> coord = concrete.to_polar;
    coord.push_back(concrete.distance_function);
    if (accel_ops) *accel_ops = accel.ops;
    if (accel_transcendentals) *accel_transcendentals = accel.transcendental;
    if (coord_ops) *coord_ops = sym::count_ops(coord).ops;
    return GR_OK;
    GR_TRY_END
}

int gr_argument_string_accelerations_call_trig(const char* argument_string) {
    if (!argument_string) return -1;
    return pb::accelerations_without_trig(pb::defines_of(argument_string)) ? 0 : 1;
}

int gr_argument_string_radius_exits_ordered(const char* argument_string) {
    if (!argument_string) return -1;
    return pb::radius_exits_ordered(pb::defines_of(argument_string)) ? 1 : 0;
}

int gr_program_precompile(const char* argument_string) {
    if (!argument_string) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument string");
    std::string code, rest, setup;
    int rc = compile_code_object(argument_string, code);
    if (rc != GR_OK) return rc;
    rc = compile_code_object(argument_string, rest, nullptr, PART_REST);
    if (rc != GR_OK) return rc;
    return compile_setup_module(argument_string, setup);
}

// Builds that outlive their program (a program destroyed while its second code object is still inside the compiler detaches the
// worker): the process must not run its exit handlers - which tear down the compiler's own static state - under such a thread.  They
// are counted, and an atexit handler waits for the count to reach zero (a build is seconds; bounded at two minutes).
static std::mutex g_background_mu;
static std::condition_variable g_background_cv;
static int g_background_builds = 0;
static void background_builds_wait() {
    std::unique_lock<std::mutex> lock(g_background_mu);
    g_background_cv.wait_for(lock, std::chrono::seconds(120), [] { return g_background_builds == 0; });
}
static void background_builds_begin() {
    static std::once_flag once;
    std::call_once(once, [] { atexit(background_builds_wait); });
    std::lock_guard<std::mutex> lock(g_background_mu);
    g_background_builds++;
}
static void background_builds_end() {
    std::lock_guard<std::mutex> lock(g_background_mu);
    g_background_builds--;
    g_background_cv.notify_all();
}

// the frame path of a program: its PART_FRAME code object and the set-up module, each from the cache or built - the two builds side by
// side on two threads when both are missing (the compiler runs are independent; ~1.3 s and ~2.5 s of one core each for Kerr)
static int build_frame_path(const std::string& arguments, std::string& code, std::string& setup_code, std::string* key) {
    std::string setup_error;
    int setup_rc = GR_OK;
    { int a, b; rtc_version(a, b); }   // (before the second thread exists)
    // (both in the cache - every program after its first use: no thread at all)
    int rc = compile_setup_module(arguments, setup_code, /*cache_only=*/true);
    if (rc != GR_OK) return rc;
    if (!setup_code.empty()) return compile_code_object(arguments, code, key);
    std::thread side([&]() {
        setup_rc = compile_setup_module(arguments, setup_code);
        if (setup_rc != GR_OK) setup_error = g_error;
    });
    rc = compile_code_object(arguments, code, key);
    side.join();
    if (rc != GR_OK) return rc;
    if (setup_rc != GR_OK) return fail((gr_status)setup_rc, setup_error);
    return GR_OK;
}

// the function of kernel k, loading the program's other code object when the kernel lives there (blocks while that is still being
// built); nullptr with the error set when it cannot be had
static hipFunction_t function_of(gr_program* p, int k) {
    if (p->fn[k] || !p->in_rest[k]) return p->fn[k];
    std::lock_guard<std::mutex> lock(p->rest_mu);
    if (!p->rest_loaded) {
        auto& b = *p->rest;
        {
            std::unique_lock<std::mutex> wait(b.mu);
            b.cv.wait(wait, [&] { return b.done; });
        }
        if (p->rest_worker.joinable()) p->rest_worker.join();
        p->rest_rc = b.rc;
        p->rest_error = b.error;
        if (p->rest_rc == GR_OK) {
            hipError_t e = hipSetDevice(p->device);
            if (e == hipSuccess) e = hipModuleLoadData(&p->module_rest, b.code.data());
            for (int i = 0; i < K_COUNT && e == hipSuccess; i++)
                if (p->in_rest[i] && !p->fn[i]) e = hipModuleGetFunction(&p->fn[i], p->module_rest, KERNEL_NAMES[i]);
            if (e != hipSuccess) { p->rest_rc = GR_ERROR_DEVICE; p->rest_error = std::string("loading the program's second code object: ") + hipGetErrorString(e); }
        }
        b.code.clear();
        p->rest_loaded = true;
    }
    if (p->rest_rc != GR_OK) { (void)fail((gr_status)p->rest_rc, p->rest_error); return nullptr; }
    return p->fn[k];
}

int gr_program_precompile_frame_path(const char* argument_string) {
    if (!argument_string) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument string");
    std::string code, setup;
    return build_frame_path(argument_string, code, setup, nullptr);
}

int gr_program_complete(gr_program* p) {
    if (!p) return fail(GR_ERROR_INVALID_ARGUMENT, "null program");
    for (int k = 0; k < K_COUNT; k++)
        if (p->in_rest[k] && !function_of(p, k)) return p->rest_rc != GR_OK ? p->rest_rc : fail(GR_ERROR_DEVICE, std::string("kernel missing: ") + KERNEL_NAMES[k]);
    return GR_OK;
}

int gr_program_create(const char* argument_string, int device, gr_program** out) {
    if (!argument_string || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    std::string code, key, setup_code;
    int rc = build_frame_path(argument_string, code, setup_code, &key);
    if (rc != GR_OK) return rc;
    HIP_CHECK(hipSetDevice(device));
    auto p = std::make_unique<gr_program>();
    p->key = key;
    {
        // What was built for this key is not a function of the key alone: the occupancy rule of compile_code_object depends on a
        // spill size that varies from one compiler run to the next, and a cache directory may hold either outcome.  The key a
        // caller sees (and the committed hardware counters carry) therefore names the outcome too: registers and scratch of the
        // fused trace kernel as loaded.
        int vgprs = 0, scratch = 0;
        if (pb::kernel_resources(code, "gr_trace_fused", vgprs, scratch)) p->key += "-v" + std::to_string(vgprs) + "s" + std::to_string(scratch);
    }
    p->device = device;
    p->arguments = argument_string;
    {
        const char* extra = pb::switches::extra_flags();
        p->tile_shading = p->arguments.find("-DGR_TILE_SHADING") != std::string::npos || (extra && strstr(extra, "-DGR_TILE_SHADING"));
        p->cell_rows = p->arguments.find("-DGR_CELL_BLOCK=0") != std::string::npos || (extra && strstr(extra, "-DGR_CELL_BLOCK=0"));
    }
    static std::atomic<unsigned long long> next_serial{1};
    p->serial = next_serial.fetch_add(1);
    HIP_CHECK(hipModuleLoadData(&p->module, code.data()));
    HIP_CHECK(hipModuleLoadData(&p->setup_module, setup_code.data()));
    for (int k = 0; k < K_COUNT; k++) {
        if (is_setup_kernel(k)) {
            HIP_CHECK(hipModuleGetFunction(&p->fn[k], p->setup_module, KERNEL_NAMES[k]));
            continue;
        }
        // what the frame-path code object does not hold is in the other one - but for the two kernels that are built for some programs
        // only (gr_trace_pair: pair_kernel_applies; gr_trace_fused_parking: -DGR_PARKING) and belong to the frame path when they exist
        if (hipModuleGetFunction(&p->fn[k], p->module, KERNEL_NAMES[k]) != hipSuccess) {
            p->fn[k] = nullptr;
            (void)hipGetLastError();
            p->in_rest[k] = !(k == K_TRACE_PAIR || k == K_TRACE_FUSED_PARKING || k == K_RENDER_ANALYTIC || k == K_RENDER_STARS);   // (gr_render_analytic, gr_render_stars: shading.hip puts them beside gr_render)
        }
    }
    if (!p->fn[K_TRACE_FUSED] || !p->fn[K_RENDER] || !p->fn[K_PREPASS_FUSED] || !p->fn[K_ORDER_TILES])
        return fail(GR_ERROR_COMPILE, "the frame-path code object lacks one of gr_trace_fused / gr_render / gr_prepass_fused / gr_order_tiles");
    // the other kernels: from the cache now, or from a build that starts here and is waited for by whoever first needs one of them
    p->rest = std::make_shared<gr_program::rest_build>();
    rc = compile_code_object(argument_string, p->rest->code, nullptr, PART_REST, /*cache_only=*/true);
    if (rc != GR_OK) return rc;
    if (!p->rest->code.empty()) p->rest->done = true;
    else {
        auto state = p->rest;
        const std::string arguments = argument_string;
        background_builds_begin();
        try {
        p->rest_worker = std::thread([state, arguments]() {
            std::string built;
            const int build_rc = compile_code_object(arguments, built, nullptr, PART_REST);   // compiler only: no device work on this thread
            {
                std::lock_guard<std::mutex> lock(state->mu);
                state->rc = build_rc;
                if (build_rc != GR_OK) state->error = g_error;
                state->code.swap(built);
                state->done = true;
                state->cv.notify_all();
            }
            background_builds_end();
        });
        } catch (const std::system_error& e) {   // no thread to be had: built here and now, on the caller's thread
            background_builds_end();
            const int build_rc = compile_code_object(arguments, state->code, nullptr, PART_REST);
            state->rc = build_rc;
            if (build_rc != GR_OK) state->error = g_error;
            state->done = true;
        }
    }
    const int huge = 0x7fffffff;
    HIP_CHECK(hipMalloc((void**)&p->tickets, gr_program::TICKET_RING * sizeof(unsigned int)));
    HIP_CHECK(hipDeviceGetAttribute(&p->compute_units, hipDeviceAttributeMultiprocessorCount, p->device));
    HIP_CHECK(hipMalloc(&p->huge_count, sizeof(int)));
    HIP_CHECK(hipMemcpy(p->huge_count, &huge, sizeof(int), hipMemcpyHostToDevice));
    *out = p.release();
    return GR_OK;
}

// ---- background build of the substituted program (metric_manager.hpp:153-219) ---------------------------------

struct gr_program_future {
    std::string arguments;
    int device = 0;
    std::thread worker;
    std::mutex mu;
    bool done = false;
    int rc = GR_OK;
    std::string error;
    std::string code;
    std::atomic<bool> cancelled{false};   // nobody wants the result any more: the worker stops at its next stage boundary
};

int gr_program_create_async(const char* argument_string, int device, gr_program_future** out) {
    if (!argument_string || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    auto* f = new gr_program_future();
    f->arguments = argument_string;
    f->device = device;
    f->worker = std::thread([f]() {
        // the program's frame path (compiler only: no device work on this thread); its other kernels are built behind the swap, by the
        // program itself (gr_program_create)
        std::string code, setup;
        int rc = build_frame_path(f->arguments, code, setup, nullptr);
        std::lock_guard<std::mutex> lock(f->mu);
        f->rc = rc;
        if (rc != GR_OK) f->error = g_error;
        f->code.swap(code);
        f->done = true;
    });
    *out = f;
    return GR_OK;
}

int gr_program_future_poll(gr_program_future* f, gr_program** out) {
    if (!f || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    {
        std::lock_guard<std::mutex> lock(f->mu);
        if (!f->done) return 0;
        if (f->rc != GR_OK) return fail((gr_status)f->rc, f->error);
    }
    int rc = gr_program_create(f->arguments.c_str(), f->device, out);   // code object now comes from the cache
    return rc == GR_OK ? 1 : rc;
}

void gr_program_future_destroy(gr_program_future* f) {
    if (!f) return;
    if (f->worker.joinable()) f->worker.join();
    delete f;
}

// ---- metric_manager (metric_manager.hpp:19-219): which program to launch this frame -----------------------------------------
// The dynamic program (parameters read from memory) is built first and is usable whatever the parameters; the substituted one
// (parameters and features folded into the code) builds on a worker thread and is swapped in by the first gr_program_manager_current
// call that finds it finished (check_substitution, :172-219).  Changing a parameter puts the dynamic program back at once
// (check_recompile's soft recompile, :129-166) and starts a new substituted build; the finished one is retired, not destroyed,
// because frames launched with it may still be in flight on the caller's streams.
struct gr_program_manager {
    const gr_metric* metric = nullptr;
    int device = 0;
    gr_program* dynamic = nullptr;
    gr_program* substituted = nullptr;       // swapped in (using_swapped)
    gr_program_future* pending = nullptr;    // substituted_program_opt
    bool pending_is_stale = false;           // the parameters changed while it was building: its result is discarded, the next build follows it
    std::vector<gr_program*> retired;
    gr_features features{};
    std::vector<float> cfg;
    unsigned long long swaps = 0, updates = 0, builds_started = 0;
};

static int manager_start_build(gr_program_manager* pm) {
    size_t need = 0;
    int rc = gr_metric_argument_string(pm->metric, &pm->features, 1, pm->cfg.data(), (int)pm->cfg.size(), nullptr, 0, &need);
    if (rc != GR_OK) return rc;
    std::string arguments(need, '\0');
    rc = gr_metric_argument_string(pm->metric, &pm->features, 1, pm->cfg.data(), (int)pm->cfg.size(), &arguments[0], need, &need);
    if (rc != GR_OK) return rc;
    pm->pending_is_stale = false;
    pm->builds_started++;
    return gr_program_create_async(arguments.c_str(), pm->device, &pm->pending);
}

// AT MOST ONE BUILD IN FLIGHT (round 5).  A build that a parameter change has overtaken is not waited for - its worker cannot be
// interrupted inside the compiler, and joining it would stall the caller's frame loop for the rest of the compile every time a slider
// moves - but neither is a second one started next to it: a slider dragged for ten seconds changes the parameters every frame, and a
// build per change (round 4) meant hundreds of compiler threads and code-object-manager contexts alive at once.  The overtaken build is
// marked stale and told to stop at its next stage; the manager only remembers the latest parameters; whoever next finds the worker
// finished (update or current) discards its result and starts the build of the latest parameters.  The reference cancels the pending
// build the same way (metric_manager.hpp:129-166).  Returns < 0 on an error of the build that was started.
static int manager_follow_stale_build(gr_program_manager* pm) {
    if (!pm->pending || !pm->pending_is_stale) return GR_OK;
    bool done;
    {
        std::lock_guard<std::mutex> lock(pm->pending->mu);
        done = pm->pending->done;
    }
    if (!done) return GR_OK;
    gr_program_future_destroy(pm->pending);   // joins a worker that has left its last statement
    pm->pending = nullptr;
    return manager_start_build(pm);
}

static void manager_retire(gr_program_manager* pm, gr_program* p) {
    if (!p) return;
    pm->retired.push_back(p);
    while (pm->retired.size() > 2) {   // the oldest is two parameter changes old: nothing launched with it can still be queued
        (void)hipSetDevice(pm->device);
        (void)hipDeviceSynchronize();
        gr_program_destroy(pm->retired.front());
        pm->retired.erase(pm->retired.begin());
    }
}

int gr_program_manager_create(const gr_metric* m, int device, const gr_features* features, const float* cfg_values, int num_cfg_values,
                              gr_program_manager** out) {
    if (!m || !out) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    auto pm = std::make_unique<gr_program_manager>();
    pm->metric = m;
    pm->device = device;
    gr_features_default(&pm->features);
    pm->features.max_acceleration_change = m->cfg.max_acceleration_change;   // metric_manager.hpp:50
    if (features) pm->features = *features;
    const int n = (int)m->vars.names.size();
    for (int i = 0; i < n; i++) pm->cfg.push_back(cfg_values && i < num_cfg_values ? cfg_values[i] : m->vars.defaults[i]);
    size_t need = 0;
    int rc = gr_metric_argument_string(m, nullptr, 0, nullptr, 0, nullptr, 0, &need);
    if (rc != GR_OK) return rc;
    std::string arguments(need, '\0');
    rc = gr_metric_argument_string(m, nullptr, 0, nullptr, 0, &arguments[0], need, &need);
    if (rc != GR_OK) return rc;
    rc = gr_program_create(arguments.c_str(), device, &pm->dynamic);   // the first program of a metric is waited for (should_block)
    if (rc != GR_OK) return rc;
    rc = manager_start_build(pm.get());
    if (rc != GR_OK) { gr_program_destroy(pm->dynamic); return rc; }
    *out = pm.release();
    return GR_OK;
}

int gr_program_manager_update(gr_program_manager* pm, const gr_features* features, const float* cfg_values, int num_cfg_values) {
    if (!pm) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    gr_features f = pm->features;
    if (features) f = *features;
    std::vector<float> cfg = pm->cfg;
    for (size_t i = 0; i < cfg.size(); i++)
        if (cfg_values && (int)i < num_cfg_values) cfg[i] = cfg_values[i];
    if (memcmp(&f, &pm->features, sizeof(f)) == 0 && cfg == pm->cfg) return GR_OK;   // nothing changed: keep what is running or building
    pm->features = f;
    pm->cfg = cfg;
    pm->updates++;
    manager_retire(pm, pm->substituted);   // the substituted program is invalid for the new values: the dynamic one again
    pm->substituted = nullptr;
    if (pm->pending) {   // one build in flight: it is overtaken, the next one starts when its worker has finished
        pm->pending_is_stale = true;
        pm->pending->cancelled.store(true);
        return manager_follow_stale_build(pm);
    }
    return manager_start_build(pm);
}

int gr_program_manager_current(gr_program_manager* pm, int wait, gr_program** program, int* is_substituted) {
    if (!pm || !program) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    while (pm->pending) {
        if (pm->pending_is_stale) {   // an overtaken build: nothing of it is wanted; the build of the latest parameters follows it
            const int rc = manager_follow_stale_build(pm);
            if (rc != GR_OK) return rc;
            if (pm->pending && pm->pending_is_stale) {   // its worker is still inside the compiler
                if (!wait) break;
                std::this_thread::sleep_for(std::chrono::milliseconds(5));
            }
            continue;
        }
        gr_program* ready = nullptr;
        const int rc = gr_program_future_poll(pm->pending, &ready);
        if (rc < 0) {   // the substituted build failed: the dynamic program goes on serving, the error is reported once
            gr_program_future_destroy(pm->pending);
            pm->pending = nullptr;
            return rc;
        }
        if (rc == 1) {
            gr_program_future_destroy(pm->pending);
            pm->pending = nullptr;
            pm->substituted = ready;
            pm->swaps++;
            break;
        }
        if (!wait) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
    *program = pm->substituted ? pm->substituted : pm->dynamic;
    if (is_substituted) *is_substituted = pm->substituted ? 1 : 0;
    return GR_OK;
}

gr_program* gr_program_manager_dynamic(gr_program_manager* pm) { return pm ? pm->dynamic : nullptr; }

void gr_program_manager_counters(const gr_program_manager* pm, unsigned long long out[4]) {
    if (!pm || !out) return;
    out[0] = pm->updates; out[1] = pm->swaps; out[2] = pm->builds_started; out[3] = pm->pending && pm->pending_is_stale ? 1 : 0;
}

void gr_program_manager_destroy(gr_program_manager* pm) {
    if (!pm) return;
    if (pm->pending) { pm->pending->cancelled.store(true); gr_program_future_destroy(pm->pending); }
    for (gr_program* p : pm->retired) gr_program_destroy(p);
    gr_program_destroy(pm->substituted);
    gr_program_destroy(pm->dynamic);
    delete pm;
}

void gr_program_destroy(gr_program* p) {
    delete p;   // ~gr_program releases the module and its device buffers (also on gr_program_create's error paths)
}

unsigned long long gr_program_serial(const gr_program* p) { return p ? p->serial : 0; }

const char* gr_program_build_key(const gr_program* p) { return p ? p->key.c_str() : ""; }

int gr_program_kernel_info(const gr_program* p, const char* kernel_name, int* vgprs, int* sgprs, int* scratch_bytes) {
    if (!p || !kernel_name) return fail(GR_ERROR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < K_COUNT; k++) {
        if (strcmp(kernel_name, KERNEL_NAMES[k]) != 0) continue;
        int v = 0, l = 0;
        hipFunction_t f = function_of(const_cast<gr_program*>(p), k);
        if (!f) return p->in_rest[k] ? p->rest_rc : fail(GR_ERROR_INVALID_ARGUMENT, std::string("this program has no ") + kernel_name);
        HIP_CHECK(hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_NUM_REGS, f));
        HIP_CHECK(hipFuncGetAttribute(&l, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f));
        if (vgprs) *vgprs = v;
        if (sgprs) *sgprs = 0;
        if (scratch_bytes) *scratch_bytes = l;
        return GR_OK;
    }
    return fail(GR_ERROR_INVALID_ARGUMENT, "unknown kernel");
}

// ---- launch helpers ---------------------------------------------------------------------------

extern "C++" {   // (internal.hpp: device_encoders.cpp launches through these too)
int gr_internal::launch(gr_program* p, int k, void* stream, unsigned gx, unsigned gy, unsigned bx, unsigned by, void** args) {
    if (!p) return fail(GR_ERROR_INVALID_ARGUMENT, "null program");
    if (gx == 0 || gy == 0) return GR_OK;
    hipFunction_t f = function_of(p, k);
    if (!f) return p->in_rest[k] && p->rest_rc != GR_OK ? p->rest_rc : fail(GR_ERROR_INVALID_ARGUMENT, std::string("this program has no ") + KERNEL_NAMES[k]);
    HIP_CHECK(hipModuleLaunchKernel(f, gx, gy, 1, bx, by, 1, 0, (hipStream_t)stream, args, nullptr));
    return GR_OK;
}
int gr_internal::device_of(const gr_program* p) { return p->device; }
const void* gr_internal::no_count_of(const gr_program* p) { return p->huge_count; }
gr_internal::program_facts gr_internal::facts_of(const gr_program* p) {
    program_facts f;
    if (!p) return f;
    f.compute_units = p->compute_units; f.cell_rows = p->cell_rows; f.tile_shading = p->tile_shading;
    f.has_pair = p->fn[K_TRACE_PAIR] != nullptr; f.has_parking = p->fn[K_TRACE_FUSED_PARKING] != nullptr;
    return f;
}
int gr_internal::resident_groups_per_cu(gr_program* p, int k, int wg, int* per_cu) {
    if (!p->resident_groups_per_cu[k]) {
        int n = 0;
        if (hipSetDevice(p->device) != hipSuccess) return fail(GR_ERROR_DEVICE, "hipSetDevice");
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, function_of(p, k), wg, 0) != hipSuccess || n < 1) {
            (void)hipGetLastError();
            n = 4 * 8 * 64 / wg;
        }
        p->resident_groups_per_cu[k] = n;
    }
    *per_cu = p->resident_groups_per_cu[k];
    return GR_OK;
}
int gr_internal::draw_ticket(gr_program* p, void* stream, unsigned int** ticket) {
    if (!p) return fail(GR_ERROR_INVALID_ARGUMENT, "null program");
    *ticket = p->tickets + (p->next_ticket.fetch_add(1) % gr_program::TICKET_RING);
    HIP_CHECK(hipSetDevice(p->device));
    HIP_CHECK(hipMemsetAsync(*ticket, 0, sizeof(unsigned int), (hipStream_t)stream));
    return GR_OK;
}
}
using gr_internal::blocks, gr_internal::launch;

int gr_cart_to_generic(gr_program* p, void* stream, const void* in, void* out, int count, float flip, const void* cfg) {
    GR_NEED("gr_cart_to_generic", in, out);
    void* args[] = {&in, &out, &count, &flip, &cfg};
    return launch(p, K_CART_TO_GENERIC, stream, blocks(count, 64), 1, 64, 1, args);
}

int gr_init_basis_vectors(gr_program* p, void* stream, const void* generic_in, int count, const float speed[3],
                          void* e0, void* e1, void* e2, void* e3, const void* cfg) {
    GR_NEED("gr_init_basis_vectors", generic_in, e0, e1, e2, e3);
    float sx = speed ? speed[0] : 0.f, sy = speed ? speed[1] : 0.f, sz = speed ? speed[2] : 0.f;
    void* args[] = {&generic_in, &count, &sx, &sy, &sz, &e0, &e1, &e2, &e3, &cfg};
    return launch(p, K_INIT_BASIS, stream, blocks(count, 64), 1, 64, 1, args);
}

int gr_clear_termination_buffer(gr_program* p, void* stream, void* buf, int width, int height) {
    GR_NEED("gr_clear_termination_buffer", buf);
    void* args[] = {&buf, &width, &height};
    return launch(p, K_CLEAR_TERM, stream, blocks((long long)width * height, 256), 1, 256, 1, args);
}

int gr_tiled_slot_count(int width, int height) {
    const int T = 8;
    return ((width + T - 1) / T) * ((height + T - 1) / T) * T * T;
}

int gr_init_rays_generic(gr_program* p, void* stream, const void* camera_generic, const void* camera_quat, void* rays,
                         void* ray_count, int width, int height, const void* termination_buffer, int prepass_width,
                         int prepass_height, int flip, const void* e0, const void* e1, const void* e2, const void* e3,
                         const void* cfg, const void* dfg, int i_am_prepass, int tiled) {
    GR_NEED("gr_init_rays_generic", camera_generic, camera_quat, rays, ray_count, e0, e1, e2, e3);
    if (!termination_buffer && prepass_width != width && prepass_height != height) return fail(GR_ERROR_INVALID_ARGUMENT, "gr_init_rays_generic: a prepass grid without its termination buffer");
    long long slots = tiled ? gr_tiled_slot_count(width, height) : (long long)width * height;
    void* args[] = {&camera_generic, &camera_quat, &rays, &ray_count, &width, &height, &termination_buffer,
                    &prepass_width, &prepass_height, &flip, &e0, &e1, &e2, &e3, &cfg, &dfg, &i_am_prepass, &tiled};
    return launch(p, K_INIT_RAYS, stream, blocks(slots, 256), 1, 256, 1, args);
}

int gr_do_generic_rays(gr_program* p, void* stream, void* rays, const void* ray_count, int num_rays, void* tmin, void* tmax,
                       const void* cfg, const void* dfg, int width, int height, int mouse_x, int mouse_y, void* ray_write,
                       void* ray_write_counts, int max_write, void* attempt_counter) {
    GR_NEED("gr_do_generic_rays", rays, ray_count);
    void* args[] = {&rays, &ray_count, &tmin, &tmax, &cfg, &dfg, &width, &height, &mouse_x, &mouse_y,
                    &ray_write, &ray_write_counts, &max_write, &attempt_counter};
    return launch(p, K_DO_RAYS, stream, blocks(num_rays, 64), 1, 64, 1, args);
}

int gr_calculate_singularities(gr_program* p, void* stream, const void* rays, const void* count, int num_rays, void* term,
                               int width, int height) {
    GR_NEED("gr_calculate_singularities", rays, count, term);
    void* args[] = {&rays, &count, &term, &width, &height};
    return launch(p, K_CALC_SING, stream, blocks(num_rays, 256), 1, 256, 1, args);
}

int gr_calculate_render_data(gr_program* p, void* stream, const void* rays, const void* ray_count, int num_rays, void* rdata,
                             void* rdata_count, int width, int height, const void* cfg, const void* dfg) {
    GR_NEED("gr_calculate_render_data", rays, ray_count, rdata, rdata_count);
    void* args[] = {&rays, &ray_count, &rdata, &rdata_count, &width, &height, &cfg, &dfg};
    return launch(p, K_CALC_RDATA, stream, blocks(num_rays, 256), 1, 256, 1, args);
}

int gr_handle_adaptive_sampling(gr_program* p, void* stream, const void* rays, const void* ray_count, void* rdata,
                                void* rdata_count, void* new_rays, void* new_ray_count, const void* camera_generic,
                                const void* camera_quat, const void* e0, const void* e1, const void* e2, const void* e3,
                                int width, int height, const void* cfg, const void* dfg) {
    GR_NEED("gr_handle_adaptive_sampling", rays, ray_count, rdata, rdata_count, new_rays, new_ray_count, camera_generic, camera_quat, e0, e1, e2, e3);
    void* args[] = {&rays, &ray_count, &rdata, &rdata_count, &new_rays, &new_ray_count, &camera_generic, &camera_quat,
                    &e0, &e1, &e2, &e3, &width, &height, &cfg, &dfg};
    return launch(p, K_ADAPTIVE, stream, blocks(width / 2, 8), blocks(height / 2, 8), 8, 8, args);
}

// (the shading pass's launchers - gr_render and its kin, the analytic sky - are in shading.cpp; gr_strip_local_blocks is in trace_plan.cpp)

// (the launchers of the stages behind the trace - resolve, present, shutter, filter, glare, meter, solve, tone - are in frame_launch.cpp,
// the order a delivery calls them in is delivery_plan.cpp's)

// ---- the sky's mip slices on the device (kernels/background.hip) ------------------------------------

// gr_pack_mipped_background's level count (graphics_settings.cpp:164-168), in integers
static int background_levels(int width, int height) {
    int levels = 0;
    for (int m = std::min(width, height); m > 0 && levels < 10; m >>= 1) levels++;
    return levels;
}

// the float4 pyramid of levels 1 ... levels - 1, back to back
static size_t background_scratch_bytes(int width, int height, int levels) {
    size_t texels = 0;
    for (int l = 1; l < levels; l++) texels += (size_t)(width >> l) * (size_t)(height >> l);
    return texels * 4 * sizeof(float);
}

// the sizes both entry points refuse: none, or more texels than a slice may index with 31 bits / the slice writer's grid may cover
static int background_size_check(const char* who, int width, int height) {
    if (width <= 0 || height <= 0 || (long long)width * height > 0x7fffffffll || (long long)width * height * 10 / 4 > 0xffffff00ll)
        return fail(GR_ERROR_INVALID_ARGUMENT, std::string(who) + ": the image's size " + std::to_string(width) + " x " + std::to_string(height));
    return GR_OK;
}

int gr_mipped_background_scratch_bytes(int width, int height, size_t* bytes) {
    if (!bytes) return fail(GR_ERROR_INVALID_ARGUMENT, "gr_mipped_background_scratch_bytes: null argument");
    int rc = background_size_check("gr_mipped_background_scratch_bytes", width, height);
    if (rc != GR_OK) return rc;
    *bytes = background_scratch_bytes(width, height, background_levels(width, height));
    return GR_OK;
}

// Everything is refused before the first HIP call.  Then: the float levels in one launch per five levels (gr_background_reduce), the
// slices in one launch over all of them (gr_background_slices), on `stream` in that order.
int gr_build_mipped_background(gr_program* p, void* stream, const void* rgba8, int width, int height, void* packed_out, void* scratch,
                               size_t scratch_bytes) {
    const char* who = "gr_build_mipped_background";
    int rc = background_size_check(who, width, height);
    if (rc != GR_OK) return rc;
    const int levels = background_levels(width, height);
    const size_t image_bytes = (size_t)width * height * 4, packed_bytes = image_bytes * levels, need_bytes = background_scratch_bytes(width, height, levels);
    if (need_bytes) GR_NEED(who, rgba8, packed_out, scratch);
    else GR_NEED(who, rgba8, packed_out);
    if (scratch_bytes < need_bytes)
        return fail(GR_ERROR_INVALID_ARGUMENT, std::string(who) + ": scratch of " + std::to_string(scratch_bytes) + " bytes, " + std::to_string(need_bytes) + " needed (gr_mipped_background_scratch_bytes)");
    const uintptr_t image_at = (uintptr_t)rgba8, packed_at = (uintptr_t)packed_out, scratch_at = (uintptr_t)scratch;
    if (image_at % 4 || packed_at % 16 || (need_bytes && scratch_at % 16))
        return fail(GR_ERROR_INVALID_ARGUMENT, std::string(who) + ": rgba8 must be aligned to 4 bytes, packed_out and scratch to 16");
    auto overlap = [](uintptr_t a, size_t an, uintptr_t b, size_t bn) { return an && bn && a < b + bn && b < a + an; };
    const bool in_place = image_at == packed_at;
    if ((!in_place && overlap(image_at, image_bytes, packed_at, packed_bytes)) || overlap(scratch_at, need_bytes, packed_at, packed_bytes) ||
        overlap(scratch_at, need_bytes, image_at, image_bytes))
        return fail(GR_ERROR_INVALID_ARGUMENT, std::string(who) + ": rgba8, packed_out and scratch overlap (rgba8 == packed_out is the one overlap allowed)");
    if (!p) return fail(GR_ERROR_INVALID_ARGUMENT, std::string(who) + ": null program");
    for (int source_level = 0; source_level < levels - 1; source_level += 5) {
        int count = std::min(5, levels - 1 - source_level);
        void* args[] = {&rgba8, &scratch, &width, &height, &source_level, &count};
        rc = launch(p, K_BACKGROUND_REDUCE, stream, blocks((width >> source_level) >> 1, 16), blocks((height >> source_level) >> 1, 16), 16, 16, args);
        if (rc != GR_OK) return rc;
    }
    if (in_place && levels == 1) return levels;   // slice 0 is the image and is where it should be
    int levels_arg = levels, in_place_arg = in_place ? 1 : 0;
    void* args[] = {&rgba8, &scratch, &packed_out, &width, &height, &levels_arg, &in_place_arg};
    rc = launch(p, K_BACKGROUND_SLICES, stream, blocks(((long long)width * height * levels + 3) / 4, 256), 1, 256, 1, args);
    return rc != GR_OK ? rc : levels;
}

int gr_internal_fail(int code, const char* msg) { return fail((gr_status)code, msg ? msg : ""); }

// (the trace stage's launchers - prepass, tile order, gr_trace_fused and its kin, refine, pending, scheduled, compact - are in
// trace_launch.cpp, their decisions in trace_plan.cpp)
int gr_program_has_trace_pair(const gr_program* p) { return p && p->fn[K_TRACE_PAIR] ? 1 : 0; }
int gr_program_has_tile_shading(const gr_program* p) { return p && p->tile_shading ? 1 : 0; }
int gr_program_has_parking(const gr_program* p) { return p && p->fn[K_TRACE_FUSED_PARKING] ? 1 : 0; }

// ---- camera on a timelike geodesic (cl.cl:2441-2481, 3117-3141, 4735-4940, 2569-2620, 2738-2872) --------------------

int gr_boost_tetrad(gr_program* p, void* stream, const void* generic_in, int count, const void* basis_speed, void* e0, void* e1,
                    void* e2, void* e3, const void* cfg) {
    void* args[] = {&generic_in, &count, &basis_speed, &e0, &e1, &e2, &e3, &cfg};
    return launch(p, K_BOOST_TETRAD, stream, blocks(count, 64), 1, 64, 1, args);
}

int gr_init_inertial_ray(gr_program* p, void* stream, const void* generic_position_in, int ray_count, void* rays, void* ray_count_out,
                         const void* e0, const void* e1, const void* e2, const void* e3, const void* basis_speed, const void* cfg) {
    void* args[] = {&generic_position_in, &ray_count, &rays, &ray_count_out, &e0, &e1, &e2, &e3, &basis_speed, &cfg};
    return launch(p, K_INIT_INERTIAL, stream, blocks(ray_count, 64), 1, 64, 1, args);
}

int gr_get_geodesic_path(gr_program* p, void* stream, const void* rays, int num_rays, void* positions_out, void* velocities_out,
                         void* ds_out, const void* ray_count, int max_path_length, const void* cfg, const void* dfg, void* count_out) {
    void* args[] = {&rays, &positions_out, &velocities_out, &ds_out, &ray_count, &max_path_length, &cfg, &dfg, &count_out};
    return launch(p, K_GEODESIC_PATH, stream, blocks(num_rays, 64), 1, 64, 1, args);
}

int gr_parallel_transport_quantity(gr_program* p, void* stream, const void* geodesic_path, const void* geodesic_velocity,
                                   const void* ds_in, const void* quantity, const void* count_in, int count, void* quantity_out,
                                   const void* cfg) {
    void* args[] = {&geodesic_path, &geodesic_velocity, &ds_in, &quantity, &count_in, &count, &quantity_out, &cfg};
    return launch(p, K_PARALLEL_TRANSPORT, stream, blocks(count, 64), 1, 64, 1, args);
}

int gr_handle_interpolating_geodesic(gr_program* p, void* stream, const void* geodesic_path, const void* geodesic_velocity,
                                     const void* ds_in, void* camera_generic_out, const void* t_e0, const void* t_e1,
                                     const void* t_e2, const void* t_e3, void* e0_out, void* e1_out, void* e2_out, void* e3_out,
                                     float target_time, const void* count_in, int parallel_transport_observer,
                                     const void* basis_speed, void* interpolated_velocity, const void* cfg) {
    void* args[] = {&geodesic_path, &geodesic_velocity, &ds_in, &camera_generic_out, &t_e0, &t_e1, &t_e2, &t_e3, &e0_out, &e1_out,
                    &e2_out, &e3_out, &target_time, &count_in, &parallel_transport_observer, &basis_speed, &interpolated_velocity,
                    &cfg};
    return launch(p, K_INTERPOLATE_GEODESIC, stream, 1, 1, 64, 1, args);
}

int gr_pack_mipped_background(const unsigned char* rgba, int width, int height, unsigned char* out) {
    if (width <= 0 || height <= 0) return fail(GR_ERROR_INVALID_ARGUMENT, "bad size");
    // graphics_settings.cpp:164-168
    int levels = (int)std::floor(std::log2((double)std::min(width, height))) + 1;
    if (levels > 10) levels = 10;
    if (!out) return levels;
    if (!rgba) return fail(GR_ERROR_INVALID_ARGUMENT, "null image");
    std::vector<float> cur((size_t)width * height * 4);
    for (size_t i = 0; i < cur.size(); i++) cur[i] = rgba[i] / 255.f;
    int cw = width, ch = height;
    for (int l = 0; l < levels; l++) {
        if (l > 0) {
            // 2x2 box filter (the reference takes the GL driver's mip chain)
            int nw = std::max(cw / 2, 1), nh = std::max(ch / 2, 1);
            std::vector<float> next((size_t)nw * nh * 4);
            for (int y = 0; y < nh; y++)
                for (int x = 0; x < nw; x++)
                    for (int c = 0; c < 4; c++) {
                        int x0 = std::min(2 * x, cw - 1), x1 = std::min(2 * x + 1, cw - 1);
                        int y0 = std::min(2 * y, ch - 1), y1 = std::min(2 * y + 1, ch - 1);
                        next[((size_t)y * nw + x) * 4 + c] =
                            0.25f * (cur[((size_t)y0 * cw + x0) * 4 + c] + cur[((size_t)y0 * cw + x1) * 4 + c] +
                                     cur[((size_t)y1 * cw + x0) * 4 + c] + cur[((size_t)y1 * cw + x1) * 4 + c]);
                    }
            cur.swap(next);
            cw = nw;
            ch = nh;
        }
        unsigned char* slice = out + (size_t)l * width * height * 4;
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                int lx = std::min(x, cw - 1), ly = std::min(y, ch - 1);   // edge replicate
                for (int c = 0; c < 4; c++) {
                    float v = cur[((size_t)ly * cw + lx) * 4 + c];
                    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
                    slice[((size_t)y * width + x) * 4 + c] = (unsigned char)(v * 255);
                }
            }
    }
    return levels;
}

}  // extern "C"
