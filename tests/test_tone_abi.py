"""CPU tests of the meter and the tone curve (include/geodesic_hip_internal.h, "Metering and tone curve"): the names; the host histogram
against an integer numpy model, exactly; the solve against the definition in Python floats bit for bit and against an exact rational
evaluation of the level; the table and the gains; every curve against numpy float32 bit for bit and against float64 within its counted
bound; monotony, zeros, alpha, NaN and infinity, in place; every refusal that needs no device; the stand-alone sanitizer program
(tests/tone_frame_check.cpp); the kernels' place in the set-up module and the frame path's source lists; the CLI's parsing and refusals."""
import ctypes
import glob
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import meter_histogram, meter_solve, tone_frame
import tone_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(gra.__file__), "csrc")
NAMES = ["gr_tone_default", "gr_meter_histogram_frame", "gr_meter_solve_host", "gr_tone_frame", "gr_meter_frame", "gr_meter_solve_device", "gr_apply_tone",
         "gr_render_state_set_tone", "gr_render_state_tone", "gr_render_state_exposure"]
INVALID = -1   # GR_ERROR_INVALID_ARGUMENT


def last_error_names(*names):
    text = gra.lib.gr_last_error() or b""
    return all(name.encode() in text for name in names)


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def test_the_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in NAMES:
        assert name in internal and name not in contract, name
        assert hasattr(gra.lib, name) and name in gra.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    assert header.index("---- Glare") < header.index("---- Metering and tone curve") < header.index("gr_tone_default(") < header.index("---- PNG frames")
    assert "NEVER fused" in header[header.index("---- Metering and tone curve"):]
    public = open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()
    assert len(public.splitlines()) == 350 and len(contract) <= 80 and "tone" not in public.lower() and "gr_meter" not in public
    assert ctypes.sizeof(gra.ToneStruct) == 40 and ctypes.sizeof(gra.ToneStateStruct) == 24
    t = gra.tone()
    assert (t.mode, t.stops, t.low, t.high, t.min_stops, t.max_stops, t.rate, t.curve, t.white) == (gra.TONE_MANUAL, 0.0, 0.5, np.float32(0.98), -32.0, 32.0, 1.0, gra.TONE_LINEAR, 4.0)
    assert tm.bits(np.float32(t.key_stops)) == tm.bits(np.float32(math.log2(0.18)))


def test_the_histogram_of_the_edge_values_is_the_integer_models():
    frame = tm.edge_frame()
    y = tm.luminance(frame).ravel()
    words = tm.bits(y)
    for k in range(823, 1209):   # both sides of every edge are among the luminances, not only among the colours
        assert ((words == (k << 20)) | (words == (k << 20) + 1)).any() and ((words == (k << 20) - 1) | (words == (k << 20) - 2)).any(), k
    got, want = meter_histogram(frame), tm.histogram(frame)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert int(got.sum()) == frame.shape[0] * frame.shape[1] and (got[:384] > 0).all() and got[384] > 0
    # by value: one grey pixel each (the weights sum to 1 within an ulp or two, so these stay on their side of an edge)
    for value, where in ((0.0, 384), (-0.0, 384), (-1.0, 384), (np.nan, 384), (-np.inf, 384), (np.inf, 383), (1e-42, 0), (2.0 ** -27, 0), (1.5 * 2.0 ** -24, 4),
                         (2.0 ** 25, 383), (1.5 * 2.0 ** 23, 380), (1.05, 192), (1.15, 193), (1.95, 199), (float(np.finfo(np.float32).max), 383)):
        pixel = np.array([[[value, value, value, 1.0]]], dtype=np.float32)
        hist = meter_histogram(pixel)
        assert hist.sum() == 1 and hist[where] == 1 and np.array_equal(hist, tm.histogram(pixel)), (value, int(hist.argmax()))


@pytest.mark.parametrize("w,h", tm.SIZES)
def test_the_histogram_of_random_frames_is_the_integer_models(w, h):
    frame = tm.random_frame(w, h, 17 * w + h)
    assert np.array_equal(meter_histogram(frame), tm.histogram(frame))
    big = tm.random_frame(211, 97, w)
    got = meter_histogram(big)
    assert np.array_equal(got, tm.histogram(big)) and (got > 0).sum() > 300


def check_solve(name, hist, tone, adapted, primed):
    got, want = meter_solve(hist, tone, adapted, primed), tm.solve(hist, tone, adapted, primed)
    assert got[0] == want[0] and math.copysign(1, got[0]) == math.copysign(1, want[0]), (name, got, want)
    assert got[1] == want[1] and got[3] == want[3] and tm.bits(got[2]) == tm.bits(want[2]), (name, got, want)
    return got


def test_the_solve_is_the_definition_bit_for_bit():
    for name, (hist, tone, adapted, primed) in tm.solve_cases().items():
        got = check_solve(name, hist, tone, adapted, primed)
        if "empty" in name:
            assert got[:2] == (adapted, primed) and got[3] == round(adapted * 16) and (primed or got[2] == 1.0)
        else:
            assert got[1] is True
    # a single occupied bin: the level is the bin's centre
    hist, tone, _, _ = tm.solve_cases()["one bin"]
    assert meter_solve(hist, tone)[0] == float(np.float32(tone.key_stops)) - ((200 + 0.5) / 8 - 24)
    # the clamps hold at both ends
    cases = tm.solve_cases()
    assert meter_solve(*cases["clamped above"][:2])[0] == 6.5 and meter_solve(*cases["clamped below"][:2])[0] == -4.25
    assert meter_solve(*cases["both clamps at one value"][:2])[0] == float(np.float32(1.3))
    # manual mode: the stops, and the state as it was
    manual = gra.tone(stops=-2.53)
    got = check_solve("manual", cases["one bin"][0], manual, 1.25, True)
    assert got[:2] == (1.25, True) and got[3] == round(float(np.float32(-2.53)) * 16)


@pytest.mark.parametrize("rate", [1.0, 0.5, 2.0 ** -6])
def test_adaptation_over_twenty_frames(rate):
    tone = gra.tone(auto=True, rate=rate)
    state, model = (0.0, False), (0.0, False)
    seen = []
    for k, hist in enumerate(tm.sequence(20)):
        got, want = meter_solve(hist, tone, *state), tm.solve(hist, tone, *model)
        assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and tm.bits(got[2]) == tm.bits(want[2]), (k, got, want)
        if k == 7:
            assert got[0] == state[0]   # the empty frame changes nothing
        state, model = got[:2], want[:2]
        seen.append(got[0])
    assert len(set(seen)) >= 15 and (rate < 1 or seen[3] == tm.solve(tm.sequence(20)[3], tone)[0])   # rate 1 has no memory


def test_the_level_against_exact_rationals():
    for name, (hist, tone, _, _) in tm.solve_cases().items():
        if "empty" in name or "clamp" in name:
            continue
        level = float(np.float32(tone.key_stops)) - meter_solve(hist, tone)[0]   # (not primed, not clamped: adapted = key - level; one more rounding)
        exact = tm.exact_level(hist, tone)
        assert abs(float(exact)) > 0.1   # (no case sits where the 24 taken away cancels the level: the bound is relative to the level itself)
        units = abs(Fraction(level) - exact) / abs(exact) / Fraction(2) ** -52
        print(f"{name}: level {float(exact):+.6f}, {float(units):.2f} x 2^-52 relative")
        assert units <= 385, (name, level, float(exact))


def test_the_table_and_the_gains():
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    literals = re.search(r"#define GR_TONE_SIXTEENTHS \{(.*?)\}", header, flags=re.S).group(1).replace("\\", "")
    table = [float.fromhex(x.strip().rstrip("f")) for x in literals.split(",")]
    assert len(table) == 16
    for i, value in enumerate(table):
        assert value == float(np.float32(value)) and np.float32(value) == np.float32(np.exp2(np.float64(i) / 16.0)), i
    kernel = open(os.path.join(CSRC, "kernels", "tone.hip")).read()
    in_kernel = re.search(r"gr_tone_sixteenths\[16\] = \{(.*?)\}", kernel, flags=re.S).group(1)
    assert [x.strip() for x in in_kernel.split(",")] == [x.strip() for x in literals.split(",")]   # host and kernel share the one table
    assert "exp2" not in re.sub(r"//[^\n]*", "", kernel)   # (neither evaluates it: the comments may name it)
    hist = np.zeros(385, dtype=np.uint32)
    for q in range(-512, 513):
        _, _, gain, got_q = meter_solve(hist, gra.tone(stops=q / 16.0))
        want = np.float32(2.0 ** (q / 16.0))
        assert got_q == q and abs(int(tm.bits(gain).item()) - int(tm.bits(want).item())) <= 1, q
        if q % 16 == 0:
            assert gain == want and gain == np.float32(2.0) ** np.float32(q // 16)
    # ties go to even sixteenths
    assert meter_solve(hist, gra.tone(stops=1.5 / 16))[3] == 2 and meter_solve(hist, gra.tone(stops=2.5 / 16))[3] == 2 and meter_solve(hist, gra.tone(stops=-0.5 / 16))[3] == 0


@pytest.mark.parametrize("name", list(tm.CURVES))
def test_every_curve_against_float32_and_float64(name):
    """Bit for bit against numpy float32, and within a counted bound of the float64 evaluation (tone_model.curve_bound).  LINEAR within 4 and
    FILMIC within 6 units of 2^-24 relative, as first stated.  REINHARD's first count of 4 was derived wrongly - it counted n, 1 + x, the
    quotient and v, and left out that v's error passes through a, that a and 1 + a are rounded too, and that iw2 is a rounded float: the
    worst case over these inputs is 4.29 units (white 0.37).  Re-derived, with u = 2^-24, A = a / (1 + a), X = x / (1 + x) and every |d_i| <= u:
        x^ = x (1 + d1)                 iw2 = (1 / white^2) (1 + d0)          a^ = a (1 + d0 + d1 + d2)
        (1 + a)^ = (1 + a) (1 + A (d0 + d1 + d2) + d3)                        n^ = x^ (1 + a)^ (1 + d4)
        (1 + x)^ = (1 + x) (1 + X d1 + d5)                                    y^ = n^ / (1 + x)^ (1 + d6)
        y^ / y - 1 = d1 (1 + A - X) + (d0 + d2) A + d3 + d4 + d5 + d6   to first order
    so |y^ - y| <= (|1 + A - X| + 2 A + 4) u y, at most 7 u for white >= 1 and below 8 u for any white; the test holds every value to
    its own bound (with 2^-20 of it for the second-order terms)."""
    curve = tm.CURVES[name]
    worst = worst_of_bound = 0.0
    for white in (4.0, 1.0, 0.37, 4096.0) if curve == gra.TONE_REINHARD else (4.0,):
        for gain in (np.float32(1.0), np.float32(2.0 ** (-37 / 16.0)), np.float32(2.0 ** (75 / 16.0))):
            tone = gra.tone(curve=curve, white=white)
            for w, h in tm.SIZES + [(97, 41)]:
                frame = tm.colours(w, h, 3 * w + h)
                got = tone_frame(frame, tone, gain)
                assert tm.same_frame(got, tm.toned(frame, gain, curve, white)), (name, white, gain, w, h)
                assert not np.isnan(got[..., :3]).any() and not np.signbit(got[..., :3]).any()
                want = tm.curve64(frame[..., :3], gain, curve, white)
                error = np.abs(got[..., :3].astype(np.float64) - want)
                assert (error[want == 0] == 0).all()
                lit = want > 0
                units = error[lit] / want[lit] / 2.0 ** -24
                bound = tm.curve_bound(frame[..., :3], gain, curve, white)[lit]
                worst, worst_of_bound = max(worst, float(units.max())), max(worst_of_bound, float((units / bound).max()))
                assert (units <= bound * (1 + 2.0 ** -20)).all(), (name, white, gain, float(units.max()))
    print(f"{name}: worst relative error against float64 {worst:.3f} x 2^-24; {worst_of_bound:.3f} of its bound")


def test_curves_monotone_zero_alpha_and_in_place():
    ascending = np.exp2(np.linspace(-30, 26, 4096)).astype(np.float32)
    frame = np.zeros((1, 4096, 4), dtype=np.float32)
    frame[0, :, 0], frame[0, :, 1], frame[0, :, 2] = ascending, ascending, ascending
    for name, curve in tm.CURVES.items():
        for gain in (1.0, 0.013, 77.0):
            y = tone_frame(frame, gra.tone(curve=curve), gain)[0, :, 0]
            assert (np.diff(y) >= 0).all() and y[0] > 0 and y[-1] > y[0], name
        assert y[-1] == (1.0 if name == "filmic" else 16777216.0 if name == "linear" else np.float32(16777216.0) * np.float32(1048577.0) / np.float32(16777216.0))
        # y(0) = +0, for -0, negatives and NaN too; infinity is 2^24
        pixel = np.array([[[0.0, -0.0, -7.0, np.nan], [np.nan, -np.inf, np.inf, -0.0]]], dtype=np.float32)
        got = tone_frame(pixel, gra.tone(curve=curve), 2.0)
        assert tm.bits(got)[0, 0, :3].tolist() == [0, 0, 0] and tm.bits(got)[0, 1, :2].tolist() == [0, 0]
        assert tm.bits(got)[0, 0, 3] == tm.bits(pixel)[0, 0, 3] and tm.bits(got)[0, 1, 3] == 0x80000000
        assert got[0, 1, 2] == tm.curve32(np.float32(16777216.0), 1.0, curve, 4.0)
        # in place
        frame2 = tm.colours(33, 21, 5)
        want = tone_frame(frame2, gra.tone(curve=curve, white=2.5), 0.7)
        same = frame2.copy()
        assert tone_frame(same, gra.tone(curve=curve, white=2.5), 0.7, out=same) is same and tm.same_frame(same, want)
        assert np.array_equal(tm.bits(want[..., 3]), tm.bits(frame2[..., 3]))


def test_refusals():
    lib = gra.lib
    src = np.ones((4, 4, 4), dtype=np.float32)
    dst = np.full((4, 4, 4), np.float32(5.5), dtype=np.float32)
    hist = np.full(385, 7, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    good = gra.tone(auto=True)

    def bad(**fields):
        t = gra.tone(auto=True)
        for k, v in fields.items():
            setattr(t, k, v)
        return t
    wrong = [("mode", bad(mode=2)), ("mode", bad(mode=-1)), ("stops", bad(stops=32.5)), ("stops", bad(stops=np.nan)), ("key_stops", bad(key_stops=-33.0)),
             ("key_stops", bad(key_stops=np.inf)), ("low", bad(low=-0.1)), ("low", bad(low=np.nan)), ("high", bad(high=1.5)), ("high", bad(high=np.nan)),
             ("low >= high", bad(low=0.5, high=0.5)), ("low >= high", bad(low=0.9, high=0.2)), ("min_stops", bad(min_stops=-40.0)), ("max_stops", bad(max_stops=np.inf)),
             ("min_stops > max_stops", bad(min_stops=2.0, max_stops=1.0)), ("rate", bad(rate=0.0)), ("rate", bad(rate=1.5)), ("rate", bad(rate=np.nan)),
             ("curve", bad(curve=3)), ("curve", bad(curve=-1)), ("white", bad(white=0.0)), ("white", bad(white=5000.0)), ("white", bad(white=np.inf)), ("white", bad(white=np.nan))]
    a_, p_, g_, q_ = ctypes.c_double(1.5), ctypes.c_int(1), ctypes.c_float(9.0), ctypes.c_int(9)
    refs = (ctypes.byref(a_), ctypes.byref(p_), ctypes.byref(g_), ctypes.byref(q_))
    for field, t in wrong:
        assert lib.gr_tone_frame(p(src), 4, 4, ctypes.byref(t), 1.0, p(dst)) == INVALID and last_error_names("gr_tone_frame", field), (field, lib.gr_last_error())
        assert lib.gr_meter_solve_host(p(hist), ctypes.byref(t), *refs) == INVALID and last_error_names("gr_meter_solve_host", field), field
        assert lib.gr_render_state_set_tone(None, ctypes.byref(t)) == INVALID
    g = ctypes.byref(good)
    for args, word in (((None, 4, 4, g, 1.0, p(dst)), "null"), ((p(src), 4, 4, None, 1.0, p(dst)), "null"), ((p(src), 4, 4, g, 1.0, None), "null"),
                       ((p(src), 0, 4, g, 1.0, p(dst)), "size"), ((p(src), 4, -1, g, 1.0, p(dst)), "size"), ((p(src), 65536, 32768, g, 1.0, p(dst)), "2^31 - 1 pixels"),
                       ((p(src), 4, 4, g, np.nan, p(dst)), "gain"), ((p(src), 4, 4, g, np.inf, p(dst)), "gain"), ((p(src), 4, 4, g, -1.0, p(dst)), "gain")):
        assert lib.gr_tone_frame(*args) == INVALID and last_error_names("gr_tone_frame", word), (word, lib.gr_last_error())
    for args, word in (((None, 4, 4, p(hist)), "null"), ((p(src), 4, 4, None), "null"), ((p(src), 0, 4, p(hist)), "size"), ((p(src), 4, 0, p(hist)), "size"),
                       ((p(src), 65536, 32768, p(hist)), "2^31 - 1 pixels")):
        assert lib.gr_meter_histogram_frame(*args) == INVALID and last_error_names("gr_meter_histogram_frame", word), word
    for k in range(6):
        args = [p(hist), g, *refs]
        args[k] = None
        assert lib.gr_meter_solve_host(*args) == INVALID and last_error_names("gr_meter_solve_host", "null"), k
    for value in (np.nan, 40.0):
        assert lib.gr_meter_solve_host(p(hist), g, ctypes.byref(ctypes.c_double(value)), *refs[1:]) == INVALID and last_error_names("gr_meter_solve_host", "adapted")
    # nothing was written
    assert (dst == np.float32(5.5)).all() and (hist == 7).all() and (a_.value, p_.value, g_.value, q_.value) == (1.5, 1, 9.0, 9)
    assert lib.gr_tone_default(None) == INVALID and last_error_names("gr_tone_default")
    # the launchers: all before any device call (the device pointers are made up and never dereferenced)
    a, b, c = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)
    for args, word in (((None, None, a, 4, 4, b), "null program"), ((a, None, None, 4, 4, b), "null"), ((a, None, a, 4, 4, None), "null"), ((a, None, a, 0, 4, b), "size"),
                       ((a, None, a, 65536, 32768, b), "2^31 - 1 pixels"), ((a, None, ctypes.c_void_p(4100), 4, 4, b), "aligned"), ((a, None, a, 4, 4, ctypes.c_void_p(8194)), "aligned")):
        assert lib.gr_meter_frame(*args) == INVALID and last_error_names("gr_meter_frame", word), (word, lib.gr_last_error())
    manual = gra.tone()
    for args, word in (((None, None, b, g, c), "null program"), ((a, None, None, g, c), "null"), ((a, None, b, None, c), "null"), ((a, None, b, g, None), "null"),
                       ((a, None, b, ctypes.byref(manual), c), "mode"), ((a, None, ctypes.c_void_p(8194), g, c), "aligned"), ((a, None, b, g, ctypes.c_void_p(16388)), "aligned")):
        assert lib.gr_meter_solve_device(*args) == INVALID and last_error_names("gr_meter_solve_device", word), (word, lib.gr_last_error())
    for args, word in (((None, None, a, b, 4, 4, g, None, 1.0), "null program"), ((a, None, None, b, 4, 4, g, None, 1.0), "null"), ((a, None, a, None, 4, 4, g, None, 1.0), "null"),
                       ((a, None, a, b, 4, 4, None, None, 1.0), "null"), ((a, None, a, b, 4, 0, g, None, 1.0), "size"), ((a, None, a, b, 65536, 32768, g, None, 1.0), "2^31 - 1 pixels"),
                       ((a, None, a, b, 4, 4, g, None, np.nan), "host_gain"), ((a, None, a, b, 4, 4, g, None, -2.0), "host_gain"),
                       ((a, None, ctypes.c_void_p(4104), b, 4, 4, g, None, 1.0), "aligned"), ((a, None, a, ctypes.c_void_p(8200), 4, 4, g, None, 1.0), "aligned"),
                       ((a, None, a, b, 4, 4, g, ctypes.c_void_p(16386), 1.0), "aligned"), ((a, None, a, ctypes.c_void_p(4096 + 128), 4, 4, g, None, 1.0), "overlap")):
        assert lib.gr_apply_tone(*args) == INVALID and last_error_names("gr_apply_tone", word), (word, lib.gr_last_error())
    for field, t in wrong:
        assert lib.gr_apply_tone(a, None, a, b, 4, 4, ctypes.byref(t), None, 1.0) == INVALID and last_error_names("gr_apply_tone", field), field
        assert lib.gr_meter_solve_device(a, None, b, ctypes.byref(t), c) == INVALID and last_error_names("gr_meter_solve_device", field), field
    # the state's
    out, is_set, f1, f2 = gra.ToneStruct(), ctypes.c_int(0), ctypes.c_float(), ctypes.c_float()
    assert lib.gr_render_state_set_tone(None, g) == INVALID and last_error_names("gr_render_state_set_tone")
    assert lib.gr_render_state_tone(None, ctypes.byref(out), ctypes.byref(is_set)) == INVALID and last_error_names("gr_render_state_tone")
    assert lib.gr_render_state_exposure(None, None, ctypes.byref(f1), ctypes.byref(f2)) == INVALID and last_error_names("gr_render_state_exposure")
    with pytest.raises(ValueError):
        gra.tone(curve="aces")
    with pytest.raises(ValueError):
        tone_frame(np.zeros((5, 4, 3), np.float32), good, 1.0)
    with pytest.raises(ValueError):
        meter_solve(np.zeros(384, np.uint32), good)


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """the three host statements on heap buffers of exactly their sizes, address and undefined-behaviour sanitizers on: the host code alone
    with a main of its own (tests/tone_frame_check.cpp) - nothing is loaded into this process"""
    exe = str(tmp_path / "tone_frame_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "tone_frame_check.cpp"), os.path.join(CSRC, "imageio.cpp"), "-lz", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert len([line for line in lines if line.endswith("differ")]) == 6 * 3 and "refusals: 0 wrote, 12 of 12 refused" in lines


def test_the_kernels_are_in_the_setup_module_only_and_the_frame_paths_sources_are_as_they_were():
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    program_build = open(os.path.join(CSRC, "program_build.cpp")).read()
    lists = {name: re.findall(r'"([a-z_]+\.(?:hip|inc))"', body) for name, body in re.findall(r"const (\w*PARTS)\[\] = \{(.*?)\};", program_build, flags=re.S)}
    parts = lists["PARTS"]
    assert "tone.hip" in parts and parts.index("tone.hip") < parts.index("glare.hip") and parts[-1] == "glare.hip" and parts.count("tone.hip") == 1
    # the frame path's build key hashes these files and nothing of the set-up module's: the list is what it was
    assert lists["KERNEL_PARTS"] == ["program.hip", "probes.inc", "metric.hip", "setup.hip", "integrator.hip", "trace.hip", "shading.hip"]
    for other in lists["KERNEL_PARTS"]:
        text = open(os.path.join(CSRC, "kernels", other)).read()
        assert "gr_meter" not in text and "gr_tone" not in text, other
    for name in ("K_METER_HISTOGRAM", "K_METER_SOLVE", "K_TONE_APPLY"):
        assert re.search(r"is_setup_kernel\(int k\) \{[^}]*" + name, capi), name
    kernel = open(os.path.join(CSRC, "kernels", "tone.hip")).read()
    assert "fma" not in kernel
    for name in ("gr_meter_histogram(", "gr_meter_solve(", "gr_tone_apply(", "__syncthreads()", "atomicAdd(&hist["):
        assert name in kernel, name
    waves, counters, lanes, per_lane, tile = (int(re.search(r"#define GR_METER_" + n + r" (\d+)", kernel).group(1)) for n in ("WAVES", "COUNTERS", "LANES", "PER_LANE", "TILE"))
    assert (waves, counters) == (4, 385) and waves * counters * 4 <= 64 * 1024   # static LDS a workgroup
    assert lanes == 64 * waves and tile == lanes * per_lane
    # the launcher's tile and workgroup are the kernel's: a grid sized by another tile would leave pixels uncounted
    launchers = open(os.path.join(CSRC, "frame_launch.cpp")).read()   # (gr_meter_frame's file)
    launcher = re.search(r"static const unsigned long long METER_TILE = (\d+), METER_MAX_WORKGROUPS = (\d+);\s*static const unsigned METER_LANES = (\d+);", launchers)
    assert launcher and (int(launcher.group(1)), int(launcher.group(3))) == (tile, lanes) and int(launcher.group(2)) >= 1
    assert "(pixels + METER_TILE - 1) / METER_TILE" in launchers and "K_METER_HISTOGRAM, stream, grid, 1, METER_LANES, 1" in launchers


def test_the_setup_module_cross_compiles_with_the_three_kernels(tmp_path, monkeypatch):
    """the set-up module as the library builds it - program_build.cpp's PARTS as one translation unit, Minkowski's macros, the module's own
    options - cross-compiled for gfx950 into an empty cache (no GPU needed): the module's code object holds the three kernels and the
    frame path's do not; gr_meter_histogram's static LDS is the four sub-histograms, and it holds LDS and global atomic adds"""
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.Program.precompile(gra.Metric("minkowski").argument_string())
    files = glob.glob(os.path.join(str(tmp_path), "*.hsaco"))
    (setup,) = [f for f in files if f.endswith(".setup.hsaco")]
    assert len(files) > 1
    for f in files:
        blob = open(f, "rb").read()
        for name in (b"gr_meter_histogram", b"gr_meter_solve", b"gr_tone_apply"):
            assert (name in blob) == (f == setup), (name, f)
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-readelf")) or not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-readelf / llvm-objdump in this image: the names were checked, the LDS size and the atomics were not")
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", setup], capture_output=True, text=True, check=True).stdout
    # (a kernel's map in the metadata note: its keys sorted, at one indent - the arguments' own .name keys sit deeper)
    lds = {name: int(size) for size, name in re.findall(r"^    \.group_segment_fixed_size:\s*(\d+)\n(?:^ .*\n)*?^    \.name:\s+(\w+)", notes, flags=re.M)}
    assert lds["gr_meter_histogram"] == 4 * 385 * 4 and lds["gr_meter_solve"] == 0 and lds["gr_tone_apply"] == 0 and max(lds.values()) <= 64 * 1024, lds
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", setup], capture_output=True, text=True, check=True).stdout
    ops, inside = [], False
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            inside = m.group(1) == "gr_meter_histogram"
        elif inside and line.startswith("\t"):
            ops.append(line.strip().split(" ")[0])
    assert "ds_add_u32" in ops and "global_atomic_add" in ops and "s_barrier" in ops, sorted(set(ops))


def test_the_cli_parses_and_refuses(capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert render.parse_tone_curve("linear") == (gra.TONE_LINEAR, None) and render.parse_tone_curve("reinhard") == (gra.TONE_REINHARD, None)
    assert render.parse_tone_curve("reinhard:2.5") == (gra.TONE_REINHARD, 2.5) and render.parse_tone_curve("filmic") == (gra.TONE_FILMIC, None)
    assert render.parse_meter("0.25:0.9") == (0.25, 0.9)
    for text in ("aces", "filmic:2", "reinhard:", "reinhard:x", "linear:1"):
        with pytest.raises(ValueError):
            render.parse_tone_curve(text)
    for text in ("0.5", "0.1:0.2:0.3", "a:b"):
        with pytest.raises(ValueError):
            render.parse_meter(text)
    assert render.tone_of() is None
    t = render.tone_of(True, (0.25, 0.9), 0.5, (gra.TONE_REINHARD, 2.5))
    assert bytes(t) == bytes(gra.tone(auto=True, low=0.25, high=0.9, rate=0.5, curve="reinhard", white=2.5)) and t.mode == gra.TONE_AUTO
    t = render.tone_of(-1.5)
    assert t.mode == gra.TONE_AUTO and t.key_stops == -1.5 and t.curve == gra.TONE_LINEAR
    t = render.tone_of(curve=(gra.TONE_FILMIC, None))
    assert t.mode == gra.TONE_MANUAL and t.stops == 0.0 and t.curve == gra.TONE_FILMIC
    base = ["--metric", "kerr_boyer", "--out", "x.png"]
    for argv, words in ((["--auto-exposure", "--devices", "0,1"], ("--auto-exposure", "--devices")), (["--tone", "filmic", "--devices", "0"], ("--tone", "--devices")),
                        (["--auto-exposure", "--exposure", "1"], ("--auto-exposure", "--exposure")), (["--auto-exposure", "-2", "--exposure", "1"], ("--auto-exposure", "--exposure")),
                        (["--meter", "0.5:0.9"], ("--meter", "without --auto-exposure")), (["--adapt", "0.5"], ("--adapt", "without --auto-exposure")),
                        (["--auto-exposure", "--meter", "0.9:0.5"], ("--meter", "low >= high")), (["--auto-exposure", "--meter", "0.5"], ("--meter", "LOW:HIGH")),
                        (["--auto-exposure", "--adapt", "0"], ("--adapt", "rate")), (["--auto-exposure", "--adapt", "2"], ("--adapt", "rate")),
                        (["--auto-exposure", "40"], ("--auto-exposure", "key_stops")), (["--auto-exposure", "bright"], ("--auto-exposure",)),
                        (["--tone", "aces"], ("--tone", "reinhard")), (["--tone", "reinhard:0"], ("--tone", "white")), (["--tone", "reinhard:5000"], ("--tone", "white")),
                        (["--adapt", "fast", "--auto-exposure"], ("--adapt",))):
        with pytest.raises(SystemExit) as e:
            render.main(base + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(word in err for word in words), (argv, err[-300:])
    assert os.listdir(tmp_path) == []
    # --exposure and --glare parse as they did
    g = render.glare_of(render.parse_glare("0.06:1.5,0.03:10"), 1.0)
    assert [g.taps[0], g.taps[1]] == [11, 61] and render.glare_of(None, -2.0).core == 0.25
