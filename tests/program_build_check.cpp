// program_build_check.cpp — the decision table of csrc/program_build.cpp (tests/test_program_build.py compiles this file together with
// it, with the host compiler and its sanitizers, and compares the lines printed here with the expectations written there).  No HIP, no
// hiprtc, no library.  argv[1]: an empty directory for the cache-file rows.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../geodesic_raytracing_amd/csrc/program_build.hpp"

using namespace program_build;
typedef std::vector<std::string> strings;

static std::string joined(const strings& v, const char* with = " ") {
    std::string s;
    for (auto& x : v) s += (s.empty() ? "" : with) + x;
    return s;
}

// ---- a metadata note: msgpack keys and unsigned values as the reader meets them
enum form { FIXINT, U8 = 0xcc, U16 = 0xcd, U32 = 0xce };
static std::string uint_as(form f, unsigned long v) {
    std::string s;
    if (f != FIXINT) s += (char)f;
    for (int byte = f == U32 ? 3 : f == U16 ? 1 : 0; byte >= 0; byte--) s += (char)((v >> (8 * byte)) & 0xff);
    return s;
}
static std::string name_entry(const std::string& kernel) { return std::string(".name") + (char)(0xa0 + kernel.size()) + kernel; }
static std::string note_of(const std::string& kernel, form f, unsigned long scratch, unsigned long sgprs, unsigned long vgprs) {
    return std::string("\x82\xa5") + name_entry(kernel) + ".private_segment_fixed_size" + uint_as(f, scratch) + ".sgpr_count" + uint_as(f, sgprs) +
           ".vgpr_count" + uint_as(f, vgprs) + ".wavefront_size\x40";
}
static void resources_row(const char* name, const std::string& note, const char* kernel = "gr_trace_fused") {
    int vgprs = -1, scratch = -1, sgprs = -1;
    if (kernel_resources(note, kernel, vgprs, scratch, &sgprs)) printf("%s: true vgprs=%d scratch=%d sgprs=%d\n", name, vgprs, scratch, sgprs);
    else printf("%s: false\n", name);
}

// ---- the occupancy rule with a compiler that answers from a table: wave budget (0: the free build) -> what it "compiles"
struct answer { int rc, vgprs, sgprs, scratch; };
static void rule_row(const char* name, std::map<int, answer> table, const char* remembered = nullptr, bool pass_not_applied = false,
                     strings opts = {"-O3", "-DA=1"}, build_part part = PART_FRAME) {
    strings asked;
    auto build = [&](const strings& options, std::string& code) {
        int budget = 0;
        if (options.size() == opts.size() + 1 && sscanf(options.back().c_str(), "-DGR_FUSED_WAVES=%d", &budget) != 1) budget = -1;
        asked.push_back(budget == 0 ? "free" : std::to_string(budget));
        const answer a = table.count(budget) ? table[budget] : answer{GR_ERROR_COMPILE, 0, 0, 0};
        if (a.rc == GR_OK) code = note_of("gr_trace_fused", U16, a.scratch, a.sgprs, a.vgprs) + "#" + asked.back();
        return a.rc;
    };
    const std::string text = remembered ? remembered : "";
    std::string code;
    const occupancy_outcome o = build_by_occupancy_rule(opts, occupancy_rule_applies(opts, part, switches::occupancy_tuning()), remembered ? &text : nullptr,
                                                        build, [&] { return pass_not_applied; }, code);
    std::string note = o.note;
    if (!note.empty() && note.back() == '\n') note.back() = '$';   // (the note ends its line)
    printf("%s: builds=%s rc=%d kept=%s note=\"%s\"\n", name, joined(asked, ",").c_str(), o.rc, code.empty() ? "none" : code.substr(code.rfind('#') + 1).c_str(), note.c_str());
    for (auto& l : o.lines) printf("%s: %s\n", name, l.c_str());
}

static void options_row(const char* name, const std::string& arguments, module_kind kind, build_part part) {
    const option_list o = options(arguments, kind, part);
    if (!o.refusal.empty()) printf("%s: refused \"%s\" options=%zu\n", name, o.refusal.c_str(), o.options.size());
    else printf("%s: %s\n", name, joined(o.options).c_str());
}

static std::string listing(const std::string& dir) {
    strings names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d))
            if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) names.push_back(e->d_name);
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    return joined(names, ",");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    // ---------------------------------------------------------------- the metadata reader
    resources_row("meta fixint", note_of("gr_trace_fused", FIXINT, 24, 94, 80));
    resources_row("meta 0xcc", note_of("gr_trace_fused", U8, 148, 102, 168));
    resources_row("meta 0xcd", note_of("gr_trace_fused", U16, 1000, 94, 256));
    resources_row("meta 0xce", note_of("gr_trace_fused", U32, 70000, 94, 97));
    {
        const std::string whole = note_of("gr_trace_fused", U16, 24, 94, 80);
        const size_t value = whole.find(".vgpr_count") + strlen(".vgpr_count");
        resources_row("meta ends inside a value", whole.substr(0, value + 2));   // 0xcd and one of its two bytes
        resources_row("meta ends after a key", whole.substr(0, value));
    }
    resources_row("meta no scratch key", std::string("\x82\xa5") + name_entry("gr_trace_fused") + ".sgpr_count\x5e.vgpr_count\x50");
    resources_row("meta no vgpr key", std::string("\x82\xa5") + name_entry("gr_trace_fused") + ".private_segment_fixed_size\x18.sgpr_count\x5e");
    resources_row("meta name of 32 characters", note_of("gr_kernel_name_of_32_characters_", FIXINT, 24, 94, 80), "gr_kernel_name_of_32_characters_");
    resources_row("meta name of 31 characters", note_of("gr_kernel_name_of_31_characters", FIXINT, 24, 94, 80), "gr_kernel_name_of_31_characters");
    resources_row("meta vgpr_count 0", note_of("gr_trace_fused", FIXINT, 24, 94, 0));
    resources_row("meta vgpr_count 513", note_of("gr_trace_fused", U16, 24, 94, 513));
    resources_row("meta vgpr_count 512", note_of("gr_trace_fused", U16, 24, 94, 512));
    resources_row("meta sgpr_count after vgpr_count", std::string("\x82\xa5") + name_entry("gr_trace_fused") + ".private_segment_fixed_size\x18.vgpr_count\x50.sgpr_count\x5e");
    resources_row("meta only the lattice kernel", note_of("gr_trace_fused_lattice", FIXINT, 24, 94, 80));
    resources_row("meta second kernel of two", note_of("gr_trace_fused_lattice", FIXINT, 8, 60, 40) + note_of("gr_trace_fused", U8, 24, 94, 80));
    {
        const int at[][2] = {{72, 94}, {72, 78}, {64, 74}, {97, 0}, {172, 0}};
        for (auto& p : at) printf("resident waves: (%d, %d) -> %d\n", p[0], p[1], resident_waves_per_simd(p[0], p[1]));
    }

    // ---------------------------------------------------------------- the occupancy rule
    const char* const note6 = "waves=6 free_vgprs=97 free_scratch=0\n";
    rule_row("rule a", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}, {5, {GR_OK, 96, 94, 0}}});
    rule_row("rule b", {{0, {GR_OK, 172, 100, 0}}, {4, {GR_OK, 128, 100, 148}}, {3, {GR_OK, 168, 100, 0}}});
    rule_row("rule c", {{0, {GR_OK, 87, 94, 0}}, {7, {GR_OK, 72, 94, 48}}, {6, {GR_OK, 80, 94, 16}}});
    rule_row("rule d", {{0, {GR_OK, 64, 74, 0}}, {8, {GR_OK, 56, 74, 0}}});
    rule_row("rule d, 65", {{0, {GR_OK, 65, 74, 0}}, {8, {GR_OK, 64, 74, 0}}});   // 5/6 of it is 54 registers: 8 waves, and the free build holds 7
    rule_row("rule d, 400", {{0, {GR_OK, 400, 100, 0}}});   // 5/6 of it is 333 registers: one wave, as the free build holds
    rule_row("rule e", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, note6);
    rule_row("rule f", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 97}}, {5, {GR_OK, 96, 94, 0}}}, note6);
    rule_row("rule f, 96 B more", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 136}}}, "waves=6 free_vgprs=97 free_scratch=40\n");
    rule_row("rule g, malformed", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, "waves=six free_vgprs=97 free_scratch=0\n");
    rule_row("rule g, waves=9", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}, {9, {GR_OK, 56, 94, 0}}}, "waves=9 free_vgprs=97 free_scratch=0\n");
    rule_row("rule h", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, nullptr, /*pass_not_applied=*/true);
    rule_row("rule i, PART_REST", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, note6, false, {"-O3", "-DA=1"}, PART_REST);
    rule_row("rule i, GR_FUSED_WAVES", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, note6, false, {"-O3", "-DGR_FUSED_WAVES=5"});
    rule_row("rule i, GR_TRACE_WAVES", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, note6, false, {"-DGR_TRACE_WAVES=4", "-O3"});
    setenv("GR_OCCUPANCY_TUNING", "0", 1);
    rule_row("rule i, GR_OCCUPANCY_TUNING=0", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 24}}}, note6);
    unsetenv("GR_OCCUPANCY_TUNING");
    rule_row("rule j", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_ERROR_COMPILE, 0, 0, 0}}, {5, {GR_OK, 96, 94, 0}}});
    rule_row("rule k, free build fails", {{0, {GR_ERROR_COMPILE, 0, 0, 0}}}, note6);
    rule_row("rule l, nothing kept", {{0, {GR_OK, 97, 94, 0}}, {6, {GR_OK, 80, 94, 100}}, {5, {GR_OK, 96, 94, 120}}});

    // ---------------------------------------------------------------- the shape key
    const std::string source = "__global__ void gr_trace_fused() {}\n";
    const strings shape1 = {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=12"};
    auto shape_row = [&](const char* name, const strings& other, int major = 6, int minor = 4, int runs = 8, const std::string& text = "") {
        printf("shape %s: %s\n", name, shape_name(text.empty() ? source : text, other, major, minor, runs) == shape_name(source, shape1, 6, 4, 8) ? "same" : "different");
    };
    printf("shape blanked: %s\n", joined(blank_literals(shape1), " | ").c_str());
    printf("shape name: %s\n", shape_name(source, shape1, 6, 4, 8).c_str());
    shape_row("other float literals", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.6f", "-DACCEL=(v1*0.6f+2.5e+03f)*10.0f", "-DN=12"});
    shape_row("other identifier", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(w1*0.45f+1e-05f)*10.0f", "-DN=12"});
    shape_row("other number in an identifier", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v2*0.45f+1e-05f)*10.0f", "-DN=12"});
    shape_row("other integer, as many digits", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=34"});
    shape_row("other integer, more digits", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=123"});
    shape_row("float literal for an integer", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=12.0f"});
    shape_row("GR_DEVICE_ options", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DGR_DEVICE_ACCEL0=t3*t4", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=12"});
    shape_row("operands in another order", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=10.0f*(1e-05f+0.45f*v1)", "-DN=12"});
    shape_row("name before = in another order", {"--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCLE=(v1*0.45f+1e-05f)*10.0f", "-DN=12"});
    shape_row("options in another order", {"--offload-arch=gfx950", "-O3", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DFEATURE_x=0.45f", "-DN=12"});
    shape_row("run limit 0", shape1, 6, 4, 0);
    shape_row("hiprtc 6.5", shape1, 6, 5, 8);
    shape_row("hiprtc 7.4", shape1, 7, 4, 8);
    shape_row("other source", shape1, 6, 4, 8, source + "\n");
    printf("key code object: %s\n", code_object_name(source, shape1, 6, 4, 8, true).c_str());
    printf("key code object, no tuning: %s\n", code_object_name(source, shape1, 6, 4, 8, false).c_str());
    printf("key code object, no pass: %s\n", code_object_name(source, shape1, 6, 4, 0, true).c_str());
    printf("key set-up module: %s\n", setup_module_name(source, shape1, 6, 4).c_str());

    // ---------------------------------------------------------------- options and switches
    const std::string arguments = "-DA=1  -cl-std=CL2.0 -I ./\t-DGEO_ACCEL0=v1*v1\n";
    printf("split: %s\n", joined(split_arguments(arguments), "|").c_str());
    printf("defines: %s\n", joined(defines_of(arguments + " --not-a-define -cl-fp32-correctly-rounded-divide-sqrt"), "|").c_str());
    options_row("options frame", arguments, RAY_KERNELS, PART_FRAME);
    options_row("options set-up", arguments, SETUP_MODULE, PART_FRAME);
    setenv("GR_EXTRA_FLAGS", "-DX=2 -g", 1);
    setenv("GR_SETUP_EXTRA_FLAGS", "-DY", 1);
    options_row("options rest, extra flags", arguments, RAY_KERNELS, PART_REST);
    options_row("options set-up, extra flags", arguments, SETUP_MODULE, PART_FRAME);
    unsetenv("GR_EXTRA_FLAGS");
    unsetenv("GR_SETUP_EXTRA_FLAGS");
    options_row("options rounded", "-DA=1 -cl-fp32-correctly-rounded-divide-sqrt -DB", RAY_KERNELS, PART_FRAME);
    options_row("options set-up, rounded", "-DA=1 -cl-fp32-correctly-rounded-divide-sqrt -DB", SETUP_MODULE, PART_FRAME);
    options_row("options refused", "-DA=1 --not-a-define -DB", RAY_KERNELS, PART_FRAME);
    options_row("options set-up, refused", "-DA=1 --not-a-define -DB", SETUP_MODULE, PART_FRAME);
    options_row("options adaptive", "-DGEO_ACCEL0=v1 -DADAPTIVE_PRECISION", RAY_KERNELS, PART_FRAME);
    setenv("GR_TRACE_PAIR_BUILD", "1", 1);
    options_row("options adaptive, GR_TRACE_PAIR_BUILD=1", "-DGEO_ACCEL0=v1 -DADAPTIVE_PRECISION", RAY_KERNELS, PART_FRAME);
    setenv("GR_TRACE_PAIR_BUILD", "0", 1);
    options_row("options GR_TRACE_PAIR_BUILD=0", "-DGEO_ACCEL0=v1", RAY_KERNELS, PART_FRAME);
    unsetenv("GR_TRACE_PAIR_BUILD");
    options_row("options trig, ordered radii", "-DGEO_ACCEL0=sin(v1) -DKERNEL_IS_STATIC -DDISTANCE_FUNC=v2 -DTO_COORD2=v2 -DFEATURE_max_precision_radius=10.0f "
                "-DFEATURE_universe_size=20.0f", RAY_KERNELS, PART_FRAME);
    printf("trig: %d %d %d\n", accelerations_without_trig({"-DGEO_ACCEL0=sin(v1)"}), accelerations_without_trig({"-DGEO_ACCEL0=asin(v1)*gm_cos(v2)"}),
           accelerations_without_trig({"-DTO_COORD0=sin(v1)"}));
    printf("switches unset: %d %d %d %d %d\n", switches::vector_run_limit(), switches::occupancy_tuning(), switches::trace_pair_build(), switches::verbose_build(),
           !switches::kernel_source() && !switches::setup_kernel_source() && !switches::extra_flags() && !switches::setup_extra_flags() && !switches::cache_dir());
    setenv("GR_VECTOR_RUN_LIMIT", "0", 1); setenv("GR_OCCUPANCY_TUNING", "0", 1); setenv("GR_TRACE_PAIR_BUILD", "2", 1); setenv("GR_VERBOSE_BUILD", "", 1);
    printf("switches set: %d %d %d %d\n", switches::vector_run_limit(), switches::occupancy_tuning(), switches::trace_pair_build(), switches::verbose_build());
    printf("cache dir: %s\n", cache_dir("/lib").c_str());
    setenv("GR_CACHE_DIR", "/elsewhere", 1);
    printf("cache dir: %s\n", cache_dir("/lib").c_str());

    // ---------------------------------------------------------------- cache files
    const std::string dir = std::string(argv[1]) + "/cache";   // (not there yet: publish makes it)
    const std::string bytes = std::string("\x7f" "ELF\0\0code", 10);
    std::string back = "stale";
    bool there = fetch(dir + "/a.hsaco", back);
    printf("cache fetch, nothing there: %d %zu\n", there, back.size());
    publish(dir + "/a.hsaco", bytes);
    there = fetch(dir + "/a.hsaco", back);
    printf("cache round trip: %d %d [%s]\n", there, back == bytes, listing(dir).c_str());
    publish(dir + "/a.hsaco", "second");
    there = fetch(dir + "/a.hsaco", back);
    printf("cache published again: %d %s [%s]\n", there, back.c_str(), listing(dir).c_str());
    publish(dir + "/a.hsaco/b.hsaco", bytes);   // a directory that cannot be made or written to (whoever runs this): its parent is a file
    printf("cache unwritable: %d [%s]\n", fetch(dir + "/a.hsaco/b.hsaco", back), listing(dir).c_str());
    publish(dir + "/empty.occupancy", "");
    printf("cache empty file: %d [%s]\n", fetch(dir + "/empty.occupancy", back), listing(dir).c_str());
    return 0;
}
