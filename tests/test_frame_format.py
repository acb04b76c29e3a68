"""The table of frame formats and the refusals that depend on a format (csrc/frame_format.cpp), checked without a GPU:
tests/frame_format_check.cpp is compiled together with frame_format.cpp - host compiler, AddressSanitizer and UBSan, no HIP - and run as a
program of its own; it prints the lines compared below.  The expectations are the headers' formulas (include/geodesic_hip.h, "video
frames"; geodesic_hip_internal.h) and the rules as csrc/frame.cpp, capi.cpp and tiled.cpp stated them before they moved, not what the
new code prints.  The 10-bit alignment rule was spelled in two ways there; that the two and the table's are one predicate is checked
here, for every pointer value 0 ... 15 at widths 7 and 8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "frame_format_check.cpp"), os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "frame_format.cpp")]

F32, RGBA8, YUV420, YUV420P10 = range(4)
NAMES = ["GR_FRAME_F32", "GR_FRAME_RGBA8", "GR_FRAME_YUV420", "GR_FRAME_YUV420P10"]
ENTRIES = ["gr_render_frame", "gr_render_frame_rgba8", "gr_render_frame_yuv420", "gr_render_frame_yuv420p10"]   # the headers' declarations
SIZES = [(1, 1), (2, 2), (3, 5), (7, 8), (16, 8), (1920, 1080), (0, 8), (8, -1)]   # the last two: a size below 1


def yuv420(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


BYTES = [lambda w, h: 16 * w * h, lambda w, h: 4 * w * h, yuv420, lambda w, h: 2 * yuv420(w, h)]
assert [yuv420(*s) for s in ((3, 5), (7, 8), (1920, 1080))] == [27, 88, 3110400] and 2 * yuv420(1920, 1080) == 6220800
ALIGNMENT = [(1, 1, 1), (1, 1, 1), (4, 4, 4), (8, 2, 8)]   # at widths 4, 7, 8


def refused_by_the_frame_entries(fmt, p, w):   # gr_render_frame_yuv420 / _yuv420p10 and gr_deliver_accumulated, as they spelled it
    return bool(p % 4) if fmt == YUV420 else bool(p % 8 and (p % 2 or w % 4 == 0)) if fmt == YUV420P10 else False


def refused_by_the_launchers(fmt, p, w):   # gr_present_yuv420 / _yuv420p10, as they spelled it
    return bool(p % 4) if fmt == YUV420 else bool(p % (8 if w % 4 == 0 else 2)) if fmt == YUV420P10 else False


ALL = "(GR_FRAME_F32, GR_FRAME_RGBA8, GR_FRAME_YUV420 or GR_FRAME_YUV420P10)"   # gr_deliver_accumulated's list
SPLIT = "(GR_FRAME_F32 or GR_FRAME_RGBA8)"                                      # gr_render_frame_tiled_as' and gr_tiled_exchange_as'
WHOLE = "whole frames only (strip_count > 1); a split frame travels as float4 or RGBA8: gr_render_frame_tiled_as"
BY4 = "the output must be aligned to 4 bytes for GR_FRAME_YUV420"
BY8 = "the output must be aligned to 8 bytes for GR_FRAME_YUV420P10 where the width is a multiple of 4, to 2 bytes otherwise"


def expected():
    rows = {}
    for fmt in (-1, 4):
        rows[f"row {fmt}"] = "none"
    for fmt in range(4):
        rows[f"row {fmt}"] = f"{NAMES[fmt]} {ENTRIES[fmt]} layout={int(fmt >= YUV420)} split={(16, 4, 0, 0)[fmt]}"
        rows[f"bytes {fmt}"] = " ".join(str(BYTES[fmt](w, h) if w >= 1 and h >= 1 else 0) for w, h in SIZES)
        rows[f"alignment {fmt}"] = " ".join(str(a) for a in ALIGNMENT[fmt])
        for w in (7, 8):
            one, other = ([int(spelling(fmt, p, w)) for p in range(16)] for spelling in (refused_by_the_frame_entries, refused_by_the_launchers))
            assert one == other, (fmt, w)   # the two spellings are one predicate
            rows[f"misaligned {fmt} at {w}"] = "".join(map(str, one))   # (the check hands in a width only where the frame entries read their state's)
    for split_only in (0, 1):
        for fmt in range(-1, 5):
            known = 0 <= fmt < (2 if split_only else 4)
            rows[f"format {fmt} split_only={split_only}"] = '""' if known else f'"unknown frame format {fmt} {SPLIT if split_only else ALL}"'
    for fmt in range(4):
        for layout in (-1, 0, 1, 2):
            refused = fmt >= YUV420 and layout not in (0, 1)
            rows[f"layout {layout} of {fmt}"] = f'"layout {layout} (GR_YUV420_I420 or GR_YUV420_NV12)"' if refused else '""'
        rows[f"strips of {fmt}"] = f'"{WHOLE}"' if fmt >= YUV420 else '""'
        for w in (7, 8):   # 4098 is aligned to 2 bytes and to no more
            rows[f"pointer 4098 of {fmt} at {w}"] = f'"{BY4}"' if fmt == YUV420 else f'"{BY8}"' if fmt == YUV420P10 and w == 8 else '""'
    rows["order"] = f'"unknown frame format 7 {ALL}" | "layout 9 (GR_YUV420_I420 or GR_YUV420_NV12)" | "{BY4}"'
    return rows


EXPECTED = expected()


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frame_format") / "frame_format_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer"] + SOURCES + ["-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(": ")
        assert name not in rows, name
        rows[name] = rest
    return rows


def test_the_check_prints_every_row_and_no_other(printed):
    assert sorted(printed) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_row(printed, name):
    print(name, printed[name])
    assert printed[name] == EXPECTED[name]
