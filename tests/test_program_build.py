"""What the build of a program decides (csrc/program_build.cpp), checked without a GPU and without a compiler run:
tests/program_build_check.cpp is compiled together with program_build.cpp - host compiler, AddressSanitizer and UBSan, no HIP, no
hiprtc - and run as a program of its own with no GR_* variable set; it prints one or more lines per row of the table below.  The
expectations were derived by reading the build as it stood before it moved out of csrc/capi.cpp (compile_code_object,
compile_setup_module, kernel_resources, resident_waves_per_simd), not from what the new code prints; the file names are computed here,
by this file's own FNV-1a, from the strings that code hashed.  What looked odd while deriving them is kept and listed in DESIGN.md."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "program_build_check.cpp"), os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "program_build.cpp")]


def fnv1a(*texts):
    h = 1469598103934665603
    for text in texts:
        for c in text.encode():
            h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return "%016x" % h


def rule(builds, kept, note="", rc=0):
    return f'builds={builds} rc={rc} kept={kept} note="{note}"'


def held(free, waves, got, verdict):   # the line of one capped build: (VGPRs, scratch) of the free build, (VGPRs, SGPRs, scratch) of the capped one
    return (f"[gr] gr_trace_fused: free build {free[0]} VGPRs / {free[1]} B scratch; held to {waves} waves: "
            f"{got[0]} VGPRs / {got[1]} SGPRs / {got[2]} B scratch ({verdict})")


def remembered(waves, got):
    return (f"[gr] gr_trace_fused: held to {waves} waves as remembered for programs of this shape: "
            f"{got[0]} VGPRs / {got[1]} SGPRs / {got[2]} B scratch (kept, one compiler run)")


FEWER = "dropped: its scalar registers admit fewer waves"
SOURCE = "__global__ void gr_trace_fused() {}\n"
SHAPE1 = ["--offload-arch=gfx950", "-O3", "-DFEATURE_x=0.45f", "-DACCEL=(v1*0.45f+1e-05f)*10.0f", "-DN=12"]
# every float literal a '#', every other digit a 9, what follows the first '=' sorted as characters
BLANKED = ["--offload-arch=999fgx", "-O9", "-DFEATURE_x=#", "-DACCEL=###()**+9v", "-DN=99"]
HASHED = [SOURCE] + [o + "\n" for o in SHAPE1]
RAY = ("--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-math-errno -freciprocal-math -fassociative-math -fno-signed-zeros "
       "-fno-trapping-math -fno-hip-fp32-correctly-rounded-divide-sqrt -fapprox-func -fgpu-flush-denormals-to-zero -fno-slp-vectorize ")
RAY_ROUNDED = ("--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -fno-math-errno -fassociative-math -fno-signed-zeros "
               "-fno-trapping-math -fgpu-flush-denormals-to-zero -fno-slp-vectorize ")
SETUP = ("--offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-math-errno -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt "
         "-DGR_SETUP_MODULE -DGR_LIBM_TRIG -DGR_LIBM_TANH ")
DEFINES = "-DA=1 -DGEO_ACCEL0=v1*v1"   # of "-DA=1  -cl-std=CL2.0 -I ./\t-DGEO_ACCEL0=v1*v1\n": no `?:`, no sin / cos, fixed step
REFUSED = 'refused "unsupported token in argument string: --not-a-define" options=0'
NOTE6_OF_97 = "waves=6 free_vgprs=97 free_scratch=0$"   # ($: the note's newline)
A = [rule("free,6", 6, NOTE6_OF_97), held((97, 0), 6, (80, 94, 24), "kept")]   # 5/6 of 97 is 80 registers: 6 waves; the free build holds 4

EXPECTED = {
    # ---- kernel_resources: the four encodings, what is missing or cut short, the bounds on the name's length and on the VGPR count
    "meta fixint": "true vgprs=80 scratch=24 sgprs=94",
    "meta 0xcc": "true vgprs=168 scratch=148 sgprs=102",
    "meta 0xcd": "true vgprs=256 scratch=1000 sgprs=94",
    "meta 0xce": "true vgprs=97 scratch=70000 sgprs=94",
    "meta ends inside a value": "false",
    "meta ends after a key": "false",
    "meta no scratch key": "false",
    "meta no vgpr key": "false",
    "meta name of 32 characters": "false",   # (the note holds that very name: only the length refuses)
    "meta name of 31 characters": "true vgprs=80 scratch=24 sgprs=94",
    "meta vgpr_count 0": "false",
    "meta vgpr_count 513": "false",
    "meta vgpr_count 512": "true vgprs=512 scratch=24 sgprs=94",
    "meta sgpr_count after vgpr_count": "true vgprs=80 scratch=24 sgprs=0",   # only an .sgpr_count in front of .vgpr_count is the kernel's own
    "meta only the lattice kernel": "false",   # the name's length byte differs
    "meta second kernel of two": "true vgprs=80 scratch=24 sgprs=94",
    # ---- the three measured points of its comment, and by vector registers alone (104 and 176 registers in granules of 8)
    "resident waves": ["(72, 94) -> 6", "(72, 78) -> 7", "(64, 74) -> 8", "(97, 0) -> 4", "(172, 0) -> 2"],
    # ---- the occupancy rule: the budgets asked of the compiler in order, the build kept, the note to write, the verbose lines
    "rule a": A,
    # 5/6 of 172 is 143 registers: 3 waves' budget (168) is more, 4 waves' (128) is not; the free build holds 2
    "rule b": [rule("free,4,3", 3, "waves=3 free_vgprs=172 free_scratch=0$"), held((172, 0), 4, (128, 100, 148), "dropped"),
               held((172, 0), 3, (168, 100, 0), "kept")],
    # 5/6 of 87 is 72 registers: 7 waves; the free build holds 5; 94 scalar registers admit 6
    "rule c": [rule("free,7,6", 6, "waves=6 free_vgprs=87 free_scratch=0$"), held((87, 0), 7, (72, 94, 48), FEWER), held((87, 0), 6, (80, 94, 16), "kept")],
    "rule d": rule("free", "free"),
    "rule d, 65": [rule("free,8", 8, "waves=8 free_vgprs=65 free_scratch=0$"), held((65, 0), 8, (64, 74, 0), "kept")],
    "rule d, 400": [rule("free", "free"), "[gr] gr_trace_fused: free build 400 VGPRs / 0 B scratch, left alone"],
    "rule e": [rule("6", 6), remembered(6, (80, 94, 24))],
    # 97 B is more than the note's free_scratch + 96; the free build's scratch is 0 too, so 6 waves are dropped again and 5 are tried
    "rule f": [rule("6,free,6,5", 5, "waves=5 free_vgprs=97 free_scratch=0$"), held((97, 0), 6, (80, 94, 97), "dropped"), held((97, 0), 5, (96, 94, 0), "kept")],
    "rule f, 96 B more": [rule("6", 6), remembered(6, (80, 94, 136))],
    "rule g, malformed": A,
    "rule g, waves=9": A,
    "rule h": [rule("free,6", 6), A[1]],   # the build went out without the assembly pass: kept for this program, not remembered
    "rule i, PART_REST": rule("free", "free"),
    "rule i, GR_FUSED_WAVES": rule("free", "free"),
    "rule i, GR_TRACE_WAVES": rule("free", "free"),
    "rule i, GR_OCCUPANCY_TUNING=0": rule("free", "free"),
    # a capped build that fails is a dropped one (its line shows no registers and blames the scalar ones)
    "rule j": [rule("free,6,5", 5, "waves=5 free_vgprs=97 free_scratch=0$"), held((97, 0), 6, (0, 0, 0), FEWER), held((97, 0), 5, (96, 94, 0), "kept")],
    "rule k, free build fails": rule("6,free", "none", rc=-3),   # GR_ERROR_COMPILE, after the remembered budget failed too
    "rule l, nothing kept": [rule("free,6,5", "free"), held((97, 0), 6, (80, 94, 100), "dropped"), held((97, 0), 5, (96, 94, 120), "dropped")],
    # ---- the shape key against the one of SHAPE1, hiprtc 6.4, run limit 8
    "shape blanked": " | ".join(BLANKED),
    "shape name": fnv1a(SOURCE, *[b + "\n" for b in BLANKED], "shape, hiprtc 6.4, runs 8") + ".occupancy",
    "shape other float literals": "same",           # 0.6f, 2.5e+03f, 10.0f
    "shape other identifier": "different",          # w1 for v1
    "shape other number in an identifier": "same",  # v2 for v1: the generator numbers its temporaries as it meets them
    "shape other integer, as many digits": "same",  # 34 for 12: every digit counts as a 9 (as found)
    "shape other integer, more digits": "different",
    "shape float literal for an integer": "different",
    "shape GR_DEVICE_ options": "same",
    "shape operands in another order": "same",
    "shape name before = in another order": "different",
    "shape options in another order": "different",
    "shape run limit 0": "different",
    "shape hiprtc 6.5": "different",
    "shape hiprtc 7.4": "different",
    "shape other source": "different",
    "key code object": fnv1a(*HASHED, "hiprtc 6.4", "vector runs <= 8 in the integrator kernels, list of round 5") + ".hsaco",
    "key code object, no tuning": fnv1a(*HASHED, "hiprtc 6.4", "no occupancy tuning", "vector runs <= 8 in the integrator kernels, list of round 5") + ".hsaco",
    "key code object, no pass": fnv1a(*HASHED, "hiprtc 6.4") + ".hsaco",
    "key set-up module": fnv1a(*HASHED, "set-up module, hiprtc 6.4") + ".setup.hsaco",
    # ---- macro string -> options: the defines in order, then the derived defines, the extra flags, the part
    "split": "-DA=1|-cl-std=CL2.0|-I|./|-DGEO_ACCEL0=v1*v1",
    "defines": "-DA=1|-DGEO_ACCEL0=v1*v1",
    "options frame": RAY + DEFINES + " -DGR_TWO_RAYS_PER_LANE -DGR_ACCEL_WITHOUT_TRIG -DGR_BUILD_FRAME_PATH",
    "options set-up": SETUP + DEFINES,
    "options rest, extra flags": RAY + DEFINES + " -DGR_TWO_RAYS_PER_LANE -DGR_ACCEL_WITHOUT_TRIG -DX=2 -g -DGR_BUILD_REST",
    "options set-up, extra flags": SETUP + DEFINES + " -DY",
    "options rounded": RAY_ROUNDED + "-DA=1 -fhip-fp32-correctly-rounded-divide-sqrt -DB -DGR_BUILD_FRAME_PATH",
    "options set-up, rounded": SETUP + "-DA=1 -DB",
    "options refused": REFUSED,
    "options set-up, refused": REFUSED,
    "options adaptive": RAY + "-DGEO_ACCEL0=v1 -DADAPTIVE_PRECISION -DGR_ACCEL_WITHOUT_TRIG -DGR_BUILD_FRAME_PATH",
    "options adaptive, GR_TRACE_PAIR_BUILD=1": RAY + "-DGEO_ACCEL0=v1 -DADAPTIVE_PRECISION -DGR_TWO_RAYS_PER_LANE -DGR_ACCEL_WITHOUT_TRIG -DGR_BUILD_FRAME_PATH",
    "options GR_TRACE_PAIR_BUILD=0": RAY + "-DGEO_ACCEL0=v1 -DGR_ACCEL_WITHOUT_TRIG -DGR_BUILD_FRAME_PATH",
    "options trig, ordered radii": RAY + "-DGEO_ACCEL0=sin(v1) -DKERNEL_IS_STATIC -DDISTANCE_FUNC=v2 -DTO_COORD2=v2 -DFEATURE_max_precision_radius=10.0f "
                                   "-DFEATURE_universe_size=20.0f -DGR_TWO_RAYS_PER_LANE -DGR_RADIUS_EXITS_ORDERED -DGR_BUILD_FRAME_PATH",
    "trig": "0 1 0",   # sin( called; asin( and gm_cos( are other functions; TO_COORD0 is not evaluated by the loop's accelerations: nothing to go by
    "switches unset": "8 1 -1 0 1",   # run limit, occupancy tuning, pair build, verbose, the five strings unset
    "switches set": "0 0 -1 1",       # GR_VECTOR_RUN_LIMIT=0 GR_OCCUPANCY_TUNING=0 GR_TRACE_PAIR_BUILD=2 (neither 0 nor 1) GR_VERBOSE_BUILD= (set)
    "cache dir": ["/lib/_cache", "/elsewhere"],
    # ---- cache files
    "cache fetch, nothing there": "0 0",
    "cache round trip": "1 1 [a.hsaco]",
    "cache published again": "1 second [a.hsaco]",
    "cache unwritable": "0 [a.hsaco]",            # no error, and no temporary left behind
    "cache empty file": "0 [a.hsaco,empty.occupancy]",   # there, and counts as absent
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    work = tmp_path_factory.mktemp("program_build")
    out = str(work / "program_build_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer"] + SOURCES + ["-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GR_")}   # no switches set
    r = subprocess.run([out, str(work)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(": ")
        rows.setdefault(name, []).append(rest)
    return rows


def test_the_table_has_every_row_and_no_other(printed):
    assert sorted(printed) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_decision(printed, name):
    want = EXPECTED[name]
    print(name, printed[name])
    assert printed[name] == (want if isinstance(want, list) else [want])
