// program_build.hpp — what the build of a program DECIDES, apart from the compiler runs: its environment switches, macro string ->
// compile options, the source lists, the cache keys, the code object's metadata note, the occupancy rule and the cache files.  Plain
// C++, no HIP or hiprtc header: all of it can be checked without a GPU or a compiler run (tests/program_build_check.cpp).  capi.cpp
// finds the library's directory and hiprtc's version, runs the compiler and carries the decisions out.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/geodesic_hip_internal.h"

namespace program_build {

// Every environment switch of the build.  Each is read whenever it is asked for - a process may change them between two builds.
namespace switches {
const char* kernel_source();         // GR_KERNEL_SOURCE         unset: the ray kernels' module from KERNEL_PARTS; else this one file
const char* setup_kernel_source();   // GR_SETUP_KERNEL_SOURCE   unset: the set-up module from PARTS; else this one file
const char* extra_flags();           // GR_EXTRA_FLAGS           unset: options appended to the ray kernels' (after the derived defines)
const char* setup_extra_flags();     // GR_SETUP_EXTRA_FLAGS     unset: ... to the set-up module's
const char* cache_dir();             // GR_CACHE_DIR             unset: <library directory>/_cache
int vector_run_limit();              // GR_VECTOR_RUN_LIMIT      8: vector instructions in a row in the integrator kernels; <= 0: no pass
bool occupancy_tuning();             // GR_OCCUPANCY_TUNING      1: the occupancy rule below; 0: as the compiler allocates (another key)
int trace_pair_build();              // GR_TRACE_PAIR_BUILD      unset (-1): gr_trace_pair where pair_kernel_applies; 0 never, 1 for adaptive programs too
bool verbose_build();                // GR_VERBOSE_BUILD         unset: quiet; set: the [gr] lines of a build on stderr
}   // namespace switches

// A program is the ray kernels' module - two code objects (kernels/program.hip): PART_FRAME, what a fused frame launches, and PART_REST,
// the reference-shaped sequence and ray compaction - and the set-up module (kernels/camera.hip says why it is one of its own).
enum module_kind { RAY_KERNELS, SETUP_MODULE };
enum build_part { PART_FRAME = 0, PART_REST = 1 };

// ---- macro string -> options
std::vector<std::string> split_arguments(const std::string& s);
enum token_kind { TOKEN_DEFINE, TOKEN_ROUNDED_DIVIDE_SQRT, TOKEN_IGNORED, TOKEN_REFUSED };
token_kind classify_token(const std::string& token);               // -D... / -cl-fp32-correctly-rounded-divide-sqrt / -cl-*, -I, ./ / anything else
std::vector<std::string> defines_of(const std::string& argument_string);   // its -D tokens, in order
struct option_list {
    std::vector<std::string> options;
    std::string refusal;   // not empty: GR_ERROR_INVALID_ARGUMENT with this text, no options
};
option_list options(const std::string& argument_string, module_kind kind, build_part part);   // (part: of RAY_KERNELS only)
bool pair_kernel_applies(const std::vector<std::string>& opts);
bool accelerations_without_trig(const std::vector<std::string>& opts);
bool radius_exits_ordered(const std::vector<std::string>& opts);

// ---- source (the lists KERNEL_PARTS and PARTS: program_build.cpp)
bool read_file(const std::string& path, std::string& out);
// the module's source: the switch's file, else the parts under kernels_dir as one translation unit.  Returns the error's text, empty when read.
std::string read_source(module_kind kind, const std::string& kernels_dir, std::string& source);

// ---- keys (file names in the cache directory)
uint64_t fnv1a(const std::string& s, uint64_t h = 1469598103934665603ull);
std::string code_object_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor, int run_limit,
                             bool occupancy_tuning);                                                                   // <16 hex>.hsaco
std::string setup_module_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor);   // <16 hex>.setup.hsaco
std::vector<std::string> blank_literals(const std::vector<std::string>& opts);   // the options as the shape key takes them
std::string shape_name(const std::string& source, const std::vector<std::string>& opts, int rtc_major, int rtc_minor, int run_limit);   // <16 hex>.occupancy

// ---- the code object's metadata note
bool kernel_resources(const std::string& code, const char* kernel, int& vgprs, int& scratch_bytes, int* sgprs = nullptr);
int resident_waves_per_simd(int vgprs, int sgprs);

// ---- the occupancy rule of gr_trace_fused (program_build.cpp has the measurements)
using build_fn = std::function<int(const std::vector<std::string>& options, std::string& code)>;   // one compiler run: GR_OK or a status
bool occupancy_rule_applies(const std::vector<std::string>& opts, build_part part, bool occupancy_tuning);
struct occupancy_outcome {
    int rc = GR_OK;                   // of the free build, where it failed (the error is the callable's)
    std::string note;                 // not empty: to be written as the shape's note
    std::vector<std::string> lines;   // what GR_VERBOSE_BUILD prints, without the newline
};
// Builds `code` through `build` alone: held to the remembered wave count (`remembered`: the shape's note, nullptr where there is none),
// else free and then by the rule.  pass_not_applied: has some build so far gone out without the assembly pass although it is on?
occupancy_outcome build_by_occupancy_rule(const std::vector<std::string>& opts, bool rule_applies, const std::string* remembered,
                                          const build_fn& build, const std::function<bool()>& pass_not_applied, std::string& code);

// ---- cache files
std::string cache_dir(const std::string& library_dir);
bool fetch(const std::string& path, std::string& bytes);            // false, and `bytes` empty, where the file is absent or empty
void publish(const std::string& path, const std::string& bytes);   // complete or not at all (temporary + rename); a failed write is no error

}   // namespace program_build
