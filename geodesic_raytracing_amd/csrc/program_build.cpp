// program_build.cpp — the decisions of a program's build (program_build.hpp): switches, options, source lists, keys, the metadata note,
// the occupancy rule, the cache files.  Reference counterpart: metric_manager.hpp:19-219 (program build + cache).  No HIP header.
#include "program_build.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace program_build {

#ifndef GR_DEFAULT_VECTOR_RUN_LIMIT
#define GR_DEFAULT_VECTOR_RUN_LIMIT 8
#endif

namespace switches {
namespace {
bool on_unless_0(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
}   // namespace
const char* kernel_source() { return getenv("GR_KERNEL_SOURCE"); }
const char* setup_kernel_source() { return getenv("GR_SETUP_KERNEL_SOURCE"); }
const char* extra_flags() { return getenv("GR_EXTRA_FLAGS"); }
const char* setup_extra_flags() { return getenv("GR_SETUP_EXTRA_FLAGS"); }
const char* cache_dir() { return getenv("GR_CACHE_DIR"); }
// Pass over the compiled code (codeobject.hpp): no more than this many vector instructions in a row without a scalar one.
// GR_VECTOR_RUN_LIMIT=0: no pass (the build still goes through the code-object manager, capi.cpp build_ray_kernels).
int vector_run_limit() { const char* e = getenv("GR_VECTOR_RUN_LIMIT"); return e ? atoi(e) : GR_DEFAULT_VECTOR_RUN_LIMIT; }
bool occupancy_tuning() { return on_unless_0("GR_OCCUPANCY_TUNING"); }
int trace_pair_build() { const char* e = getenv("GR_TRACE_PAIR_BUILD"); return !e ? -1 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : -1; }
bool verbose_build() { return getenv("GR_VERBOSE_BUILD") != nullptr; }
}   // namespace switches

// ---------------------------------------------------------------------------------------------------------------- macro string -> options

std::vector<std::string> split_arguments(const std::string& s) {
    std::vector<std::string> out;
    for (size_t i = 0; i < s.size();) {
        while (i < s.size() && isspace((unsigned char)s[i])) i++;
        size_t j = i;
        while (j < s.size() && !isspace((unsigned char)s[j])) j++;
        if (j > i) out.push_back(s.substr(i, j - i));
        i = j;
    }
    return out;
}

token_kind classify_token(const std::string& tok) {
    if (tok.rfind("-D", 0) == 0) return TOKEN_DEFINE;
    if (tok == "-cl-fp32-correctly-rounded-divide-sqrt") return TOKEN_ROUNDED_DIVIDE_SQRT;
    if (tok.rfind("-cl-", 0) == 0 || tok == "-I" || tok == "./") return TOKEN_IGNORED;   // OpenCL-only prefix flags
    return TOKEN_REFUSED;
}

std::vector<std::string> defines_of(const std::string& argument_string) {
    std::vector<std::string> opts;
    for (auto& tok : split_arguments(argument_string))
        if (classify_token(tok) == TOKEN_DEFINE) opts.push_back(tok);
    return opts;
}

// gr_trace_pair (two rays per lane, packed fp32) is built when
//  * the expressions evaluated inside the Verlet loop can be instantiated on pairs of floats - no `?:` (the comparison /
//    select forms of CMath.lt, CMath.select, csqrt) - and are small enough that two rays' temporaries fit the register
//    file (the complex-valued double-Kerr family already needs 170-260 VGPRs for one ray), and
//  * the program steps with the fixed heuristic step (no ADAPTIVE_PRECISION).  Measured on MI355X, 4K frames, substituted
//    programs: Schwarzschild 1.96 -> 1.38 ms, Minkowski 1.80 -> 1.16, wormhole 1.83 -> 1.42; with the adaptive controller
//    Kerr 7.9 -> 9.3 ms, Alcubierre 3.0 -> 3.3: the controller (sqrt, rsq, clamps, compares, the per-ray commit) has no
//    packed form, costs twice per lane what it costs the one-ray kernel per lane, and at 133 instead of 92 VGPRs only three
//    waves per SIMD are left to hide its serial tail - that outweighs what the packed multiplies save (EXPERIMENTS.md C.2).
// GR_TRACE_PAIR_BUILD=0 never builds it, =1 builds it for adaptive programs too (it is correct there, only slower).
bool pair_kernel_applies(const std::vector<std::string>& opts) {
    const int mode = switches::trace_pair_build();
    if (mode == 0) return false;
    static const char* const LOOP_MACROS[] = {"-DGEO_ACCEL", "-DTEMPORARIES0=", "-DTO_COORD", "-DDISTANCE_FUNC="};
    size_t total = 0;
    for (auto& o : opts) {
        if (mode != 1 && o == "-DADAPTIVE_PRECISION") return false;
        for (const char* m : LOOP_MACROS)
            if (o.rfind(m, 0) == 0) {
                if (o.find('?') != std::string::npos) return false;
                total += o.size();
            }
    }
    return total > 0 && total < 16384;
}

// Do the expressions the Verlet loop evaluates call the range-limited sin / cos (kernels/metric.hip GR_ACCEL_TRIG: the bare polynomials,
// which answer an argument of 8 192 or more with a NaN so that the ray leaves the fast loop for the one that calls libm)?  A program whose
// accelerations hold none - every Cartesian chart: Kerr-Schild, Alcubierre, Krasnikov ... - can never see such a NaN: its loop then treats
// a non-finite rejected attempt the reference's way (retried with the smaller step in the same loop: -DGR_ACCEL_WITHOUT_TRIG,
// integrator.hip) instead of leaving for the slow loop at the first overshoot into a singularity.
bool accelerations_without_trig(const std::vector<std::string>& opts) {
    static const char* const CALLS[] = {"sin(", "cos(", "gr_sin2(", "gr_cos2(", "gr_sincos("};
    bool any = false;
    for (auto& o : opts) {
        const size_t eq = o.find('=');
        if (o.rfind("-D", 0) != 0 || eq == std::string::npos) continue;
        const std::string name = o.substr(2, eq - 2);
        if (name.find("ACCEL") == std::string::npos && name.find("TEMPORARIES") == std::string::npos) continue;
        any = true;
        for (const char* call : CALLS)
            for (size_t at = o.find(call, eq); at != std::string::npos; at = o.find(call, at + 1)) {
                const char before = o[at - 1];
                if (!(isalnum((unsigned char)before) || before == '_')) return false;   // ("asin(", "gm_cos(" ... are other functions)
            }
    }
    return any;
}

// May a wave whose live rays are all inside the precision radius skip the outer boundary test (-DGR_RADIUS_EXITS_ORDERED, kernels/integrator.hip)?
// Only when both hold for the program as it is built:
//   * the distance the precision radius is compared with IS the polar radius the boundary tests compare, one float: DISTANCE_FUNC is the
//     variable v2 itself and, where the generator's composed form stands in for it (GR_DISTANCE_OF_GENERIC), that and TO_COORD2 are both
//     the bare variable v2 - the chart's own radius (Boyer-Lindquist, Schwarzschild ...), so nothing rests on the compiler evaluating two
//     copies of one expression to the same bits.  Decided on the expressions, never by sampling.  Macro strings are compared: a string
//     that writes the same thing another way, or does not say it, merely loses the shortcut.  Two holes' distance is not the chart radius;
//   * SINGULAR_TERMINATOR < max_precision_radius < universe_size, as the floats the kernel compares with - which a substituted program
//     (-DKERNEL_IS_STATIC, -DFEATURE_*) knows and a program whose features arrive at run time does not.
// Then "inside the radius" excludes "at the outer boundary".  (The lower bound is the issue's condition for the pair of shortcuts; the
// terminator-side one - no terminator test in a wave with nobody inside - is not built, the kernel tests the terminator in every wave, so
// here the lower bound only withholds the shortcut.)  Anything else: the outer boundary is tested in every wave.
bool radius_exits_ordered(const std::vector<std::string>& opts) {
    bool is_static = false, singular = false;
    std::string radius, universe, terminator, distance, composed, polar_radius;
    for (auto& o : opts) {
        if (o == "-DKERNEL_IS_STATIC") is_static = true;
        else if (o.rfind("-DDISTANCE_FUNC=", 0) == 0) distance = o.substr(o.find('=') + 1);
        else if (o.rfind("-DGR_DISTANCE_OF_GENERIC=", 0) == 0) composed = o.substr(o.find('=') + 1);
        else if (o.rfind("-DTO_COORD2=", 0) == 0) polar_radius = o.substr(o.find('=') + 1);
        else if (o == "-DSINGULAR") singular = true;
        else if (o.rfind("-DFEATURE_max_precision_radius=", 0) == 0) radius = o.substr(o.find('=') + 1);
        else if (o.rfind("-DFEATURE_universe_size=", 0) == 0) universe = o.substr(o.find('=') + 1);
        else if (o.rfind("-DSINGULAR_TERMINATOR=", 0) == 0) terminator = o.substr(o.find('=') + 1);
    }
    // a float literal as the generator writes it (float_literal: "10.0f"); anything else - an expression, a hex float - is not understood
    auto literal = [](const std::string& text, float& value) {
        if (text.empty()) return false;
        char* end = nullptr;
        value = strtof(text.c_str(), &end);
        if (end == text.c_str()) return false;
        if (*end == 'f' || *end == 'F') end++;
        return *end == '\0' && std::isfinite(value);
    };
    const bool distance_is_radius = distance == "v2" && !polar_radius.empty() && (composed.empty() || (composed == "v2" && polar_radius == "v2"));
    float r = 0, u = 0, t = 0;
    if (!is_static || !distance_is_radius || !literal(radius, r) || !literal(universe, u)) return false;
    if (singular && !literal(terminator, t)) return false;
    return (!singular || t < r) && r < u;
}

option_list options(const std::string& argument_string, module_kind kind, build_part part) {
    option_list out;
    std::vector<std::string>& opts = out.options;
    if (kind == SETUP_MODULE)   // IEEE arithmetic (kernels/camera.hip says why)
        opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-math-errno", "-fno-slp-vectorize",
                "-fhip-fp32-correctly-rounded-divide-sqrt", "-DGR_SETUP_MODULE", "-DGR_LIBM_TRIG", "-DGR_LIBM_TANH"};
    else
        opts = {"--offload-arch=gfx950", "-O3", "-std=c++17",
                // the reference builds with -cl-unsafe-math-optimizations (metric_manager.hpp:70): reassociation,
                // reciprocal division, contraction - but NaN/Inf stay meaningful (IS_DEGENERATE, cl.cl:68)
                "-ffp-contract=fast", "-fno-math-errno", "-freciprocal-math", "-fassociative-math",
                "-fno-signed-zeros", "-fno-trapping-math",
                // OpenCL's default 2.5-ulp fp32 divide/sqrt (the reference does not pass -cl-fp32-correctly-rounded-divide-sqrt):
                // v_rcp_f32 / v_sqrt_f32 instead of the ~10-instruction correctly rounded sequences
                "-fno-hip-fp32-correctly-rounded-divide-sqrt",
                // ... and its "unsafe math": approximate-function semantics for divide/sqrt/libm (a/b = a * v_rcp_f32(b) with no
                // denormal rescaling) and flushed fp32 denormals.  Measured -18 % on the Kerr Verlet kernel, parity unchanged.
                "-fapprox-func", "-fgpu-flush-denormals-to-zero",
                // no SLP vectorisation: packed fp32 (v_pk_mul/fma_f32) is at best ~1.2x the plain rate on gfx950 and needs operand
                // pairs in adjacent registers - the straight-line metric code paid ~55 v_mov per Verlet step for it.
                // Measured on the Kerr kernel: 102 -> 80 VGPRs, 12.7 -> 10.1 ms.
                "-fno-slp-vectorize"};
    for (auto& tok : split_arguments(argument_string)) {
        const token_kind what = classify_token(tok);
        if (what == TOKEN_DEFINE) opts.push_back(tok);
        else if (what == TOKEN_ROUNDED_DIVIDE_SQRT && kind == RAY_KERNELS) {
            // OpenCL's own switch for IEEE divide and square root (the reference does not pass it, metric_manager.hpp:70; a caller who
            // appends it to the argument string gets what it means): the ray kernels without v_rcp_f32 / v_sqrt_f32 arithmetic.
            // Measured on the frame that shows the difference most (near-extreme double Kerr, tests/golden/soak/): masked pixel RMSE
            // 1.30e-4 -> 6.4e-5, pixels off 93 -> 9 of 9 216 - the reference's own distance from itself under a one-ulp change of the
            // camera position; the Verlet loop pays ~10 instructions per division.  (The set-up module has that arithmetic anyway.)
            for (const char* drop : {"-freciprocal-math", "-fapprox-func", "-fno-hip-fp32-correctly-rounded-divide-sqrt"})
                opts.erase(std::remove(opts.begin(), opts.end(), std::string(drop)), opts.end());
            opts.push_back("-fhip-fp32-correctly-rounded-divide-sqrt");
        }
        else if (what == TOKEN_REFUSED) return {{}, "unsupported token in argument string: " + tok};
    }
    if (kind == RAY_KERNELS) {
        if (pair_kernel_applies(opts)) opts.push_back("-DGR_TWO_RAYS_PER_LANE");
        if (accelerations_without_trig(opts)) opts.push_back("-DGR_ACCEL_WITHOUT_TRIG");
        if (radius_exits_ordered(opts)) opts.push_back("-DGR_RADIUS_EXITS_ORDERED");
    }
    if (const char* extra = kind == RAY_KERNELS ? switches::extra_flags() : switches::setup_extra_flags())
        for (auto& tok : split_arguments(extra)) opts.push_back(tok);
    if (kind == RAY_KERNELS) opts.push_back(part == PART_FRAME ? "-DGR_BUILD_FRAME_PATH" : "-DGR_BUILD_REST");
    return out;
}

// ---------------------------------------------------------------------------------------------------------------- source

namespace {
// the ray kernels' source: the parts under csrc/kernels/ in this order, as one translation unit (GR_KERNEL_SOURCE: one file instead)
const char* const KERNEL_PARTS[] = {"program.hip",       // structs of the boundary, build switches
                                    "probes.inc",        // measurement hooks (all off by default)
                                    "metric.hip",        // hosts of the generated expressions
                                    "setup.hip",         // tetrads, ray set-up
                                    "integrator.hip",    // the Verlet loop, one and two rays per lane
                                    "trace.hip",         // render-data, the reference-shaped and the fused kernels, prepass, tile order, adaptive sampling
                                    "shading.hip"};      // texture sampling, gr_render
// ... and the set-up module's: what runs once per frame on one lane (camera.hip, geodesic_camera.hip), the box filter of a supersampled
// frame, the separable filters that replace it (filter.hip), the shutter's accumulation (which uses the box), the encodes, the sky's
// mip slices, the PNG encoder's two kernels, the EXR encoder's two (behind png.hip: they use its bit-packer), the JPEG encoder's three, the seven that build a star catalogue, the three of the meter and the tone curve (tone.hip) and the three of the glare
const char* const PARTS[] = {"program.hip", "probes.inc", "metric.hip", "setup.hip", "camera.hip", "geodesic_camera.hip", "resolve.hip",
                             "filter.hip", "shutter.hip", "present.hip", "background.hip", "png.hip", "exr.hip", "jpeg.hip", "stars.hip", "tone.hip", "glare.hip"};
}   // namespace

bool read_file(const std::string& path, std::string& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    char buffer[65536];
    size_t n;
    while ((n = fread(buffer, 1, sizeof(buffer), f)) > 0) out.append(buffer, n);
    fclose(f);
    return true;
}

std::string read_source(module_kind kind, const std::string& kernels_dir, std::string& source) {
    source.clear();
    // GR_SETUP_KERNEL_SOURCE: one file instead of the parts, as GR_KERNEL_SOURCE is for the ray kernels' module.  (GR_KERNEL_SOURCE
    // alone replaces the ray kernels only - the tools that use it patch the trace kernel - and the set-up module is then built from the
    // library's own parts.)
    if (const char* file = kind == RAY_KERNELS ? switches::kernel_source() : switches::setup_kernel_source()) {
        if (!read_file(file, source)) return std::string(kind == RAY_KERNELS ? "cannot read kernel source " : "cannot read set-up kernel source ") + file;
        return "";
    }
    const char* const* parts = kind == RAY_KERNELS ? KERNEL_PARTS : PARTS;
    const size_t count = kind == RAY_KERNELS ? sizeof(KERNEL_PARTS) / sizeof(*KERNEL_PARTS) : sizeof(PARTS) / sizeof(*PARTS);
    for (size_t i = 0; i < count; i++) {
        std::string text;
        const std::string path = kernels_dir + "/" + parts[i];
        if (!read_file(path, text)) return "cannot read kernel source " + path;
        source += text;
        if (!text.empty() && text.back() != '\n') source += '\n';
    }
    return "";
}

// ---------------------------------------------------------------------------------------------------------------- keys

uint64_t fnv1a(const std::string& s, uint64_t h) {
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ull;
    }
    return h;
}

namespace {
std::string file_name(uint64_t h, const char* suffix) {
    char name[64];
    snprintf(name, sizeof(name), "%016llx%s", (unsigned long long)h, suffix);
    return name;
}
std::string rtc(int major, int minor) { return "hiprtc " + std::to_string(major) + "." + std::to_string(minor); }
}   // namespace

std::string code_object_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor, int run_limit,
                             bool occupancy_tuning) {
    uint64_t h = fnv1a(source);
    for (auto& o : opts) h = fnv1a(o + "\n", h);
    h = fnv1a(rtc(rtc_major, rtc_minor), h);
    if (!occupancy_tuning) h = fnv1a("no occupancy tuning", h);   // changes what is built for the same options
    if (run_limit > 0) h = fnv1a("vector runs <= " + std::to_string(run_limit) + " in the integrator kernels, list of round 5", h);   // (the list of integrator kernels is part of what is built)
    return file_name(h, ".hsaco");
}

std::string setup_module_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor) {
    uint64_t h = fnv1a(source);
    for (auto& o : opts) h = fnv1a(o + "\n", h);
    return file_name(fnv1a("set-up module, " + rtc(rtc_major, rtc_minor), h), ".setup.hsaco");
}

std::vector<std::string> blank_literals(const std::vector<std::string>& opts) {
    std::vector<std::string> out;
    for (auto& o : opts) {
        // (round 6: the device's own rendering of the accelerations - GR_DEVICE_ACCEL*, GR_DEVICE_TEMPORARIES - shares other
        // sub-expressions from one parameter set to the next, so its text has another length and another set of temporaries; with it
        // in the key no two parameter sets of round 5 ever had the same shape and every slider move paid the rule's three builds)
        if (o.rfind("-DGR_DEVICE_", 0) == 0) continue;
        std::string blank;
        for (size_t i = 0; i < o.size();) {
            const bool starts_number = isdigit((unsigned char)o[i]) && (i == 0 || !(isalnum((unsigned char)o[i - 1]) || o[i - 1] == '_'));
            if (!starts_number) { blank += o[i++]; continue; }
            size_t j = i;
            while (j < o.size() && (isdigit((unsigned char)o[j]) || o[j] == '.' || ((o[j] == 'e' || o[j] == 'E') && j + 1 < o.size() && (isdigit((unsigned char)o[j + 1]) || o[j + 1] == '-' || o[j + 1] == '+')) ||
                                    ((o[j] == '-' || o[j] == '+') && j > i && (o[j - 1] == 'e' || o[j - 1] == 'E')))) j++;
            const bool is_float = j < o.size() && o[j] == 'f' && o.substr(i, j - i).find_first_of(".e") != std::string::npos;
            if (is_float) { blank += '#'; i = j + 1; } else { blank.append(o, i, j - i); i = j; }
        }
        // (the generator orders the operands of sums and products by a hash that takes the literals in, and numbers its temporaries as
        // it meets them: two parameter sets give the same expressions in another order.  What is left after blanking the literals
        // is therefore taken as a bag of characters, every digit the same - a hint's key may collide, the rule's conditions decide.)
        for (char& ch : blank) if (isdigit((unsigned char)ch)) ch = '9';
        const size_t eq = blank.find('=');
        if (eq != std::string::npos) std::sort(blank.begin() + (long)eq + 1, blank.end());
        out.push_back(blank);
    }
    return out;
}

std::string shape_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor, int run_limit) {
    uint64_t sh = fnv1a(source);
    for (auto& blank : blank_literals(opts)) sh = fnv1a(blank + "\n", sh);
    return file_name(fnv1a("shape, " + rtc(rtc_major, rtc_minor) + ", runs " + std::to_string(run_limit), sh), ".occupancy");
}

// ---------------------------------------------------------------------------------------------------------------- metadata note

// VGPRs and scratch bytes per lane of one kernel, read from the code object's metadata note (msgpack: the kernel's map holds
// ".name", later ".private_segment_fixed_size" and ".vgpr_count" - keys are sorted).  false when the note is not understood.
bool kernel_resources(const std::string& code, const char* kernel, int& vgprs, int& scratch_bytes, int* sgprs) {
    auto msgpack_uint = [&](size_t at, long& value) -> bool {
        if (at >= code.size()) return false;
        const unsigned char c = (unsigned char)code[at];
        if (c < 0x80) { value = c; return true; }
        if (c == 0xcc && at + 1 < code.size()) { value = (unsigned char)code[at + 1]; return true; }
        if (c == 0xcd && at + 2 < code.size()) { value = ((unsigned char)code[at + 1] << 8) | (unsigned char)code[at + 2]; return true; }
        if (c == 0xce && at + 4 < code.size()) {
            value = ((long)(unsigned char)code[at + 1] << 24) | ((unsigned char)code[at + 2] << 16) | ((unsigned char)code[at + 3] << 8) | (unsigned char)code[at + 4];
            return true;
        }
        return false;
    };
    const std::string name_key = std::string(".name") + (char)(0xa0 + strlen(kernel)) + kernel;   // fixstr key, fixstr value (< 32 chars)
    if (strlen(kernel) >= 32) return false;
    size_t at = code.find(name_key);
    if (at == std::string::npos) return false;
    const std::string scratch_key = ".private_segment_fixed_size", vgpr_key = ".vgpr_count";
    size_t s = code.find(scratch_key, at), v = code.find(vgpr_key, at);
    if (s == std::string::npos || v == std::string::npos) return false;
    long sv = 0, vv = 0;
    if (!msgpack_uint(s + scratch_key.size(), sv) || !msgpack_uint(v + vgpr_key.size(), vv)) return false;
    vgprs = (int)vv;
    scratch_bytes = (int)sv;
    if (sgprs) {
        const std::string sgpr_key = ".sgpr_count";
        const size_t g = code.find(sgpr_key, at);
        long gv = 0;
        *sgprs = (g != std::string::npos && g < v && msgpack_uint(g + sgpr_key.size(), gv)) ? (int)gv : 0;
    }
    return vgprs > 0 && vgprs <= 512;
}

// Waves per SIMD a kernel of 256-thread workgroups is resident with on gfx950, by registers.  Vector registers: 512 per lane in
// granules of 8.  Scalar registers: 800 per SIMD, a wave takes its count + 6 (VCC, flat scratch, XNACK) rounded up to 16, plus 16 -
// measured with a timeline of tile begin / end stamps (tools/timeline_probe.py): the Kerr kernel at 72 VGPRs and 94 SGPRs holds 6
// waves per SIMD, not the 7 its vector registers allow; capped to 90 or 78 SGPRs it holds 7; at 64 VGPRs and <= 74 SGPRs 8.
// (sgprs 0: by the vector registers alone.)
int resident_waves_per_simd(int vgprs, int sgprs) {
    int by_vgprs = 512 / (((vgprs + 7) / 8) * 8);
    int by_sgprs = sgprs > 0 ? 800 / ((((sgprs + 6) + 15) / 16) * 16 + 16) : 8;
    int w = by_vgprs < by_sgprs ? by_vgprs : by_sgprs;
    return w > 8 ? 8 : w;
}

// ---------------------------------------------------------------------------------------------------------------- the occupancy rule

// (the rule is about gr_trace_fused: the other part is built as the compiler allocates it)
bool occupancy_rule_applies(const std::vector<std::string>& opts, build_part part, bool occupancy_tuning) {
    bool tuned_by_caller = false;
    for (auto& o : opts) tuned_by_caller |= o.rfind("-DGR_FUSED_WAVES", 0) == 0 || o.rfind("-DGR_TRACE_WAVES", 0) == 0;
    return part == PART_FRAME && !tuned_by_caller && occupancy_tuning;
}

namespace {
std::string line(const char* format, ...) __attribute__((format(printf, 1, 2)));
std::string line(const char* format, ...) {
    char text[512];
    va_list args;
    va_start(args, format);
    vsnprintf(text, sizeof(text), format, args);
    va_end(args);
    return text;
}

// One build held to `waves` waves per SIMD, and the rule's judgement of it: kept unless it spills more than 96 bytes per lane over
// `spill_base`, or its waves would not be resident anyway.
struct held_build {
    std::string code;
    int vgprs = 0, scratch = 0, sgprs = 0;
    bool resident = false, keep = false;
};
held_build build_held(const std::vector<std::string>& opts, int waves, int spill_base, const build_fn& build) {
    held_build h;
    std::vector<std::string> capped = opts;
    capped.push_back("-DGR_FUSED_WAVES=" + std::to_string(waves));
    const bool built = build(capped, h.code) == GR_OK && kernel_resources(h.code, "gr_trace_fused", h.vgprs, h.scratch, &h.sgprs);
    h.resident = built && resident_waves_per_simd(h.vgprs, h.sgprs) >= waves;
    h.keep = built && h.scratch <= spill_base + 96 && h.resident;
    return h;
}
}   // namespace

// The rule costs up to three more compiler runs.  Its outcome depends on the program's SHAPE - kernel source, options, the metric's
// expressions - far more than on the literals a substituted program carries, and a slider move changes only those: the decision is
// remembered per shape (shape_name: the options with every float literal blanked) next to the code objects, and a program of a known
// shape is built held to the remembered wave count straight away - one compiler run, the swap of the substituted program after a
// parameter change ~20 s -> ~8 s - as long as that build still meets the rule's own conditions.
//
// Occupancy of the fused trace kernel.  Left alone, the register allocator takes what the kernel could use at its widest
// point (Kerr, substituted: 97 VGPRs, 5 waves per SIMD), part of which is cold inside the Verlet loop (set-up and epilogue
// values).  Measured on MI355X, 4K Kerr, three frames in flight / one launch on its own, with the loop that still kept a
// finished ray's state in twelve registers of its own (108 VGPRs free): free build 1 400 Mrays/s / 6.7 ms; held to 96 VGPRs (5
// waves, nothing spilled) 1 492 / 6.5; to 80 (6 waves, 60 bytes per lane spilled, none of it inside the loop's attempts)
// 1 535 / 6.2; to 72 (7 waves, 84 bytes) 1 530 / 6.2.  With today's loop: 6 waves spill 24 bytes; 7 and 8 waves measure the same.
// Rule: rebuild with the register budget of five sixths of what the free build took, rounded down to an occupancy step,
// and keep that build unless it spills more than 96 bytes per lane (the same source compiles to a spill that differs by 20 B
// from one hiprtc run to the next, and a limit next to the expected number flipped the decision with it) - or unless its waves
// would not be resident anyway (round 4): the kernel's ~94 scalar registers admit 6 waves per SIMD, so the "7 waves" build of
// rounds 2 and 3 (72 VGPRs, 48 B spilled) ran 6 like the 80-register build that spills 16 B; that one is 3 % faster one frame at
// a time (5.46 against 5.65 ms, 4K Kerr) and the same with frames in flight.
occupancy_outcome build_by_occupancy_rule(const std::vector<std::string>& opts, bool rule_applies, const std::string* remembered,
                                          const build_fn& build, const std::function<bool()>& pass_not_applied, std::string& code) {
    occupancy_outcome out;
    int waves = 0, free_vgprs = 0, free_scratch = 0;
    if (rule_applies && remembered && sscanf(remembered->c_str(), "waves=%d free_vgprs=%d free_scratch=%d", &waves, &free_vgprs, &free_scratch) == 3 &&
        waves >= 1 && waves <= 8) {
        held_build h = build_held(opts, waves, free_scratch, build);
        if (h.keep) {
            code.swap(h.code);
            out.lines.push_back(line("[gr] gr_trace_fused: held to %d waves as remembered for programs of this shape: %d VGPRs / %d SGPRs / %d B scratch (kept, one compiler run)", waves, h.vgprs, h.sgprs, h.scratch));
            return out;
        }
    }
    out.rc = build(opts, code);
    int vgprs = 0, scratch = 0;
    if (out.rc != GR_OK || !rule_applies || !kernel_resources(code, "gr_trace_fused", vgprs, scratch) || vgprs <= 64) return out;
    const int free_waves = resident_waves_per_simd(vgprs, 0);
    int target_waves = resident_waves_per_simd(vgprs * 5 / 6, 0);
    while (target_waves > 1 && (512 / target_waves) / 8 * 8 > vgprs * 5 / 6) target_waves++;   // budget of w waves <= 5/6 of the free build
    if (target_waves > 8) target_waves = 8;
    if (target_waves <= free_waves) out.lines.push_back(line("[gr] gr_trace_fused: free build %d VGPRs / %d B scratch, left alone", vgprs, scratch));
    // from the rule's target down to one wave more than the free build holds: the first budget that does not spill too much
    // (double Kerr: 172 VGPRs = 2 waves; held to 4 waves it spills 148 B, held to 3 - 168 VGPRs - nothing)
    for (waves = target_waves; waves > free_waves; waves--) {
        held_build h = build_held(opts, waves, scratch, build);
        out.lines.push_back(line("[gr] gr_trace_fused: free build %d VGPRs / %d B scratch; held to %d waves: %d VGPRs / %d SGPRs / %d B scratch%s", vgprs, scratch,
                                 waves, h.vgprs, h.sgprs, h.scratch, h.keep ? " (kept)" : h.resident ? " (dropped)" : " (dropped: its scalar registers admit fewer waves)"));
        if (!h.keep) continue;
        code.swap(h.code);
        if (!pass_not_applied())   // remembered for the next program of this shape
            out.note = "waves=" + std::to_string(waves) + " free_vgprs=" + std::to_string(vgprs) + " free_scratch=" + std::to_string(scratch) + "\n";
        break;
    }
    return out;
}

// ---------------------------------------------------------------------------------------------------------------- cache files

std::string cache_dir(const std::string& library_dir) {
    const char* env = switches::cache_dir();
    return env ? env : library_dir + "/_cache";
}

bool fetch(const std::string& path, std::string& bytes) {
    if (read_file(path, bytes) && !bytes.empty()) return true;
    bytes.clear();
    return false;
}

void publish(const std::string& path, const std::string& bytes) {
    const size_t slash = path.rfind('/');
    if (slash != std::string::npos) mkdir(path.substr(0, slash).c_str(), 0755);
    // unique per writer: a background build (gr_program_create_async) and a foreground build of the same key may run in one
    // process, and several processes share the cache directory; rename() publishes a complete file atomically
    static std::atomic<unsigned long> writer{0};
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid()) + "." + std::to_string(writer.fetch_add(1));
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    const bool written = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    // (a failed write - disk full, read-only - or a failed rename: the build still succeeded)
    if (fclose(f) != 0 || !written || rename(tmp.c_str(), path.c_str()) != 0) remove(tmp.c_str());
}

}   // namespace program_build
