"""CPU test of the fenced scratch both device encoders allocate (csrc/guarded_scratch.hpp): tests/guarded_scratch_check.cpp - the header alone
with a main of its own, host compiler, address and undefined-behaviour sanitizers, no HIP - holds the layouts to what gr_png_encoder_create
and gr_jpeg_encoder_create computed before the header existed, and the verdicts to theirs.  Nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")


def test_the_layouts_and_verdicts_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "guarded_scratch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "guarded_scratch_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert [line.split(":")[0] for line in lines[:-1]] == ["png 1 words", "png 3 words", "png 4 words", "jpeg 1x1", "jpeg 16x16", "jpeg 17x33", "jpeg 1025x31"]
    assert "jpeg 1x1: regions at 64 320 696 764, 1608 words in all" in lines


def test_the_header_has_no_hip_and_the_encoders_use_it():
    header = open(os.path.join(CSRC, "guarded_scratch.hpp")).read()
    assert "#include <hip" not in header and "#include \"" not in header
    assert "#include <hip" not in open(os.path.join(CSRC, "internal.hpp")).read()
    encoders = open(os.path.join(CSRC, "device_encoders.cpp")).read()
    assert "guarded_scratch::lay_out(" in encoders and "guarded_scratch::unwritten_spans(" in encoders
    assert "GUARD_PATTERN = " not in encoders and "GUARD_WORDS = " not in encoders
