"""CPU tests of filtered frames (include/geodesic_hip_internal.h, "Filtered frames"): the five names; gr_filter_taps against the formulas
restated in numpy float64; gr_filter_frame against the definition restated in numpy float32 - whose `*` and `+` are single IEEE
operations - bit for bit, with tables that tell a reversed tap order and swapped passes apart; a triple on which a fused multiply-add
gives another float; the identity; a constant frame; every refusal that needs no device; the stand-alone sanitizer program
(tests/filter_frame_check.cpp); the kernel's place in the set-up module; the CLI's refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import filter_frame, filter_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_filter_taps", "gr_filter_frame", "gr_resolve_filtered", "gr_render_state_set_filter", "gr_render_state_filter"]
INVALID = -1   # GR_ERROR_INVALID_ARGUMENT
FILTERS = {"tent": (gra.FILTER_TENT, 1), "gaussian": (gra.FILTER_GAUSSIAN, 2), "mitchell": (gra.FILTER_MITCHELL, 2)}   # name: (value, radius)
SIZES = [(1, 1), (5, 3), (67, 9), (130, 2), (2, 33)]
# distinct, asymmetric, of both signs: a reversed order or a pass with the other axis' role gives other floats
UNEVEN16 = np.array([0.01 * (t + 1) * (-1 if t % 3 == 1 else 1) for t in range(16)], dtype=np.float32)
UNEVEN15 = np.array([0.013 * (t + 2) * (-1 if t % 4 == 2 else 1) for t in range(15)], dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def last_error_names(name):
    return name.encode() in (gra.lib.gr_last_error() or b"")


def kernel_values(filter_value, factor, radius):
    """k(d_t) of the header's formulas in float64, t ascending"""
    n = 2 * radius * factor - factor % 2
    d = np.abs((np.arange(n) + 0.5 - n / 2.0) / factor)
    if filter_value == gra.FILTER_TENT:
        k = 1.0 - d
    elif filter_value == gra.FILTER_GAUSSIAN:
        k = np.exp(-2.0 * d * d) - np.exp(-8.0)
    else:
        B = C = 1.0 / 3.0
        k = np.where(d < 1.0, ((12 - 9 * B - 6 * C) * d ** 3 + (-18 + 12 * B + 6 * C) * d ** 2 + (6 - 2 * B)) / 6,
                     ((-B - 6 * C) * d ** 3 + (6 * B + 30 * C) * d ** 2 + (-12 * B - 48 * C) * d + (8 * B + 24 * C)) / 6)
    assert (d < radius).all() and n <= 16
    return k


def restated(src, factor, taps):
    """the definition in numpy float32: the rows pass, then the columns pass; one rounded multiply and one rounded add a tap"""
    src = np.asarray(src, dtype=np.float32)
    taps = np.asarray(taps, dtype=np.float32)
    sh, sw = src.shape[:2]
    h, w, n = sh // factor, sw // factor, len(taps)
    first = (factor - n) // 2   # (even: exact)
    with np.errstate(all="ignore"):
        rows = None
        for t in range(n):
            cx = np.clip(np.arange(w) * factor + first + t, 0, sw - 1)
            product = taps[t] * src[:, cx, :]
            rows = product if t == 0 else rows + product
        out = None
        for t in range(n):
            cy = np.clip(np.arange(h) * factor + first + t, 0, sh - 1)
            product = taps[t] * rows[cy, :, :]
            out = product if t == 0 else out + product
    assert rows.dtype == np.float32 and out.dtype == np.float32 and out.shape == (h, w, 4)
    return out


def same_bits(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def source(w, h, f, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((h * f, w * f, 4)) * np.exp(rs.uniform(-6, 6, (h * f, w * f, 4)))).astype(np.float32)


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
    assert header.index("Motion-blurred frames") < header.index("Filtered frames") < header.index("gr_filter_taps(")
    assert "does NOT renormalise" in header and "NEVER a fused multiply-add" in header
    assert re.search(r"enum \{ GR_FILTER_BOX = 0, GR_FILTER_TENT = 1, GR_FILTER_GAUSSIAN = 2, GR_FILTER_MITCHELL = 3 \};", header)
    assert (gra.FILTER_BOX, gra.FILTER_TENT, gra.FILTER_GAUSSIAN, gra.FILTER_MITCHELL) == (0, 1, 2, 3)
    assert len(contract) <= 80 and len(open(os.path.join(ROOT, "include", "geodesic_hip.h")).read().splitlines()) <= 350


@pytest.mark.parametrize("name", sorted(FILTERS))
@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_taps(name, factor):
    value, radius = FILTERS[name]
    taps = filter_taps(value, factor)
    n = 2 * radius * factor - factor % 2
    assert taps.dtype == np.float32 and len(taps) == n and (n - factor) % 2 == 0
    assert np.array_equal(bits(taps), bits(taps[::-1]))                       # symmetric, bit for bit
    assert abs(float(taps.astype(np.float64).sum()) - 1.0) <= n * 2.0 ** -24
    k = kernel_values(value, factor, radius)
    total = 0.0
    for v in k:   # ascending t, in double
        total += float(v)
    want = (k / total).astype(np.float32)
    ulps = np.abs(bits(taps).astype(np.int64) - bits(want).astype(np.int64))   # (same sign everywhere: checked next)
    assert np.array_equal(np.signbit(taps), np.signbit(want)) and ulps.max() <= 1, (taps, want)
    assert np.array_equal(filter_taps(name, factor), taps)                      # by name
    if name == "mitchell" and factor >= 2:
        assert taps[0] < 0 and taps[-1] < 0
    if name != "mitchell":
        assert (taps > 0).all()


def test_the_known_tables():
    assert bits(filter_taps(gra.FILTER_TENT, 1)).tolist() == bits(np.array([1.0], dtype=np.float32)).tolist()
    assert bits(filter_taps(gra.FILTER_TENT, 2)).tolist() == bits(np.array([0.125, 0.375, 0.375, 0.125], dtype=np.float32)).tolist()
    assert (len(filter_taps("gaussian", 4)), len(filter_taps("mitchell", 4)), len(filter_taps("mitchell", 3)), len(filter_taps("tent", 3))) == (16, 16, 11, 5)


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_frame_is_the_definition(w, h):
    for factor in (1, 2, 3, 4):
        src = source(w, h, factor, 1000 * factor + w + h)
        tables = [filter_taps(value, factor) for value, _ in FILTERS.values()]
        if factor == 4:
            tables.append(UNEVEN16)
        if factor == 3:
            tables.append(UNEVEN15)
        for taps in tables:
            want = restated(src, factor, taps)
            got = filter_frame(src, factor, taps)
            assert same_bits(got, want), (factor, len(taps))
    # the uneven tables tell the orders apart: reversed taps and the transposed problem give other frames
    src = source(w, h, 4, 77 + w)
    want = restated(src, 4, UNEVEN16)
    assert not np.array_equal(bits(want), bits(restated(src, 4, UNEVEN16[::-1])))
    assert same_bits(filter_frame(src.transpose(1, 0, 2), 4, UNEVEN16), restated(src.transpose(1, 0, 2), 4, UNEVEN16))


def test_the_passes_are_rows_first():
    """columns first rounds another intermediate: on a random frame with an uneven table the two orders differ in some last bits, and the
    library is with rows first"""
    src = source(9, 7, 3, 5)
    rows_first = restated(src, 3, UNEVEN15)
    columns_first = restated(src.transpose(1, 0, 2), 3, UNEVEN15).transpose(1, 0, 2)
    assert (bits(rows_first) != bits(columns_first)).sum() > 10
    assert same_bits(filter_frame(src, 3, UNEVEN15), rows_first)


def test_a_fused_multiply_add_would_differ():
    """acc + w * r with w * r inexact (tests/test_shutter_abi.py's triple): two roundings give 0, an fma 2^-24.  Factor 2, two taps
    {1, w}, a 2 x 2 traced frame whose rows are (a, r): h = 1 * a + w * r is 0 in both rows by the definition, and out = 1 * 0 + w * 0 = 0;
    with a fused rows pass h = 2^-24 and out is not 0."""
    a, w, r = np.float32(-(1.0 + 2.0 ** -11)), np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)
    exact_product = np.float64(w) * np.float64(r)
    assert exact_product == 1.0 + 2.0 ** -11 + 2.0 ** -24 and np.float32(np.float64(a) + exact_product) == np.float32(2.0 ** -24)
    assert np.float32(a + np.float32(exact_product)) == 0
    src = np.empty((2, 2, 4), dtype=np.float32)
    src[:, 0, :], src[:, 1, :] = a, r
    taps = np.array([1.0, w], dtype=np.float32)
    want = restated(src, 2, taps)
    assert (bits(want) == 0).all()
    got = filter_frame(src, 2, taps)
    assert (bits(got) == 0).all(), got
    # ... and over many values some of which differ under an fma
    rs = np.random.RandomState(11)
    src = rs.uniform(0.5, 2.0, (64, 96, 4)).astype(np.float32)
    taps = filter_taps("mitchell", 2)
    fused = np.zeros((64, 48, 4))
    for t in range(8):
        cx = np.clip(np.arange(48) * 2 - 3 + t, 0, 95)
        product = np.float64(taps[t]) * src[:, cx, :].astype(np.float64)
        fused = product.astype(np.float32).astype(np.float64) if t == 0 else (fused + product).astype(np.float32).astype(np.float64)
    got = filter_frame(src, 2, taps)
    assert same_bits(got, restated(src, 2, taps))
    rows_only = None
    for t in range(8):
        cx = np.clip(np.arange(48) * 2 - 3 + t, 0, 95)
        product = taps[t] * src[:, cx, :]
        rows_only = product if t == 0 else rows_only + product
    assert (bits(rows_only) != bits(fused.astype(np.float32))).sum() > 100   # an fma in the rows pass is visible in hundreds of values


def test_a_single_tap_of_one_is_the_identity():
    rs = np.random.RandomState(6)
    src = rs.randint(0, 2 ** 32, size=(33, 21, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)   # every kind of float, NaNs included
    src[0, 0] = [0.0, -0.0, np.inf, -np.inf]
    got = filter_frame(src, 1, np.array([1.0], dtype=np.float32))
    number = ~np.isnan(src)
    assert np.array_equal(bits(got)[number], bits(src)[number]) and np.isnan(got[~number]).all()
    assert bits(got)[0, 0, 1] == 0x80000000   # -0.0 stays -0.0
    # tent at factor 1 is that table
    assert same_bits(filter_frame(src, 1, filter_taps("tent", 1)), got)


def test_a_constant_frame_comes_back():
    for name, (value, _) in FILTERS.items():
        for factor in (1, 2, 3, 4):
            taps = filter_taps(value, factor)
            n = len(taps)
            for constant in (np.float32(0.7231), np.float32(-183.25), np.float32(1.0)):
                src = np.full((7 * factor, 9 * factor, 4), constant, dtype=np.float32)
                got = filter_frame(src, factor, taps)
                assert np.abs(got.astype(np.float64) / float(constant) - 1.0).max() <= 2 * n * 2.0 ** -24, (name, factor, constant)


def test_nan_and_infinity_propagate():
    src = np.ones((8, 8, 4), dtype=np.float32)
    src[3, 3, 0], src[6, 1, 1], src[0, 7, 2] = np.nan, np.inf, -np.inf
    for taps in (filter_taps("tent", 2), filter_taps("mitchell", 2)):
        got = filter_frame(src, 2, taps)
        assert same_bits(got, restated(src, 2, taps))
        assert np.isnan(got[..., 0]).any() and not np.isfinite(got[..., 1]).all() and np.isfinite(got[..., 3]).all()
    zero = np.zeros(4, dtype=np.float32)   # taps of weight 0 are not skipped: 0 * inf is a NaN
    assert np.isnan(filter_frame(src, 2, zero)[..., 1]).any()


def test_refusals():
    lib = gra.lib
    src = np.zeros((8, 8, 4), dtype=np.float32)
    dst = np.full((4, 4, 4), np.float32(5.5), dtype=np.float32)
    taps = np.array([0.125, 0.375, 0.375, 0.125], dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    bad_taps = [np.array([0.5, np.nan, 0.25, 0.25], dtype=np.float32), np.array([0.5, 0.25, np.inf, 0.25], dtype=np.float32),
                np.array([-np.inf, 0.25, 0.5, 0.25], dtype=np.float32)]
    frame_cases = [(None, 4, 4, 2, p(taps), 4, p(dst)), (p(src), 4, 4, 2, None, 4, p(dst)), (p(src), 4, 4, 2, p(taps), 4, None),
                   (p(src), 0, 4, 2, p(taps), 4, p(dst)), (p(src), 4, -1, 2, p(taps), 4, p(dst)),
                   (p(src), 4, 4, 0, p(taps), 4, p(dst)), (p(src), 4, 4, 5, p(taps), 4, p(dst)), (p(src), 4, 4, -2, p(taps), 4, p(dst)),
                   (p(src), 4, 4, 2, p(taps), 0, p(dst)), (p(src), 4, 4, 2, p(taps), 17, p(dst)), (p(src), 4, 4, 2, p(taps), -1, p(dst)),
                   (p(src), 4, 4, 2, p(taps), 3, p(dst)), (p(src), 2, 2, 3, p(taps), 4, p(dst)), (p(src), 4, 4, 1, p(taps), 2, p(dst)),
                   (p(src), 4, 4, 2, p(taps), 4, p(src))]
    frame_cases += [(p(src), 4, 4, 2, p(t), 4, p(dst)) for t in bad_taps]
    for args in frame_cases:
        assert lib.gr_filter_frame(*args) == INVALID, args
        assert last_error_names("gr_filter_frame")
        assert (dst == np.float32(5.5)).all() and (src == 0).all()   # nothing was written
    assert lib.gr_filter_frame(p(src), 4, 4, 2, p(taps), 4, p(dst)) == 0 and (dst == 0).all()
    # the launcher: the same, a NULL program, too many source pixels - all before any device call (the device pointers are made up and
    # never dereferenced; the taps are host memory and are read)
    a, b = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    launcher_cases = [(a, None, None, b, 4, 4, 2, p(taps), 4), (a, None, a, None, 4, 4, 2, p(taps), 4), (a, None, a, b, 4, 4, 2, None, 4),
                      (None, None, a, b, 4, 4, 2, p(taps), 4), (a, None, a, b, 0, 4, 2, p(taps), 4), (a, None, a, b, 4, 0, 2, p(taps), 4),
                      (a, None, a, b, 4, 4, 0, p(taps), 4), (a, None, a, b, 4, 4, 5, p(taps), 4), (a, None, a, b, 4, 4, 2, p(taps), 0),
                      (a, None, a, b, 4, 4, 2, p(taps), 17), (a, None, a, b, 4, 4, 2, p(taps), 3), (a, None, a, b, 4, 4, 3, p(taps), 4),
                      (a, None, a, a, 4, 4, 2, p(taps), 4), (a, None, a, b, 30000, 20000, 2, p(taps), 4), (a, None, a, b, 2, 600000, 2, p(taps), 4)]
    launcher_cases += [(a, None, a, b, 4, 4, 2, p(t), 4) for t in bad_taps]
    for args in launcher_cases:
        assert lib.gr_resolve_filtered(*args) == INVALID, args
        assert last_error_names("gr_resolve_filtered")
    assert lib.gr_resolve_filtered(None, None, a, b, 4, 4, 2, p(taps), 4) == INVALID and b"null program" in lib.gr_last_error()
    # the tables
    out, count = (ctypes.c_float * 16)(), ctypes.c_int(-7)
    assert lib.gr_filter_taps(gra.FILTER_BOX, 2, out, ctypes.byref(count)) == INVALID
    assert last_error_names("gr_filter_taps") and last_error_names("gr_resolve_supersampled")
    for args in ((gra.FILTER_TENT, 2, None, ctypes.byref(count)), (gra.FILTER_TENT, 2, out, None), (gra.FILTER_TENT, 0, out, ctypes.byref(count)),
                 (gra.FILTER_MITCHELL, 5, out, ctypes.byref(count)), (4, 2, out, ctypes.byref(count)), (-1, 2, out, ctypes.byref(count))):
        assert lib.gr_filter_taps(*args) == INVALID, args
        assert last_error_names("gr_filter_taps")
    assert count.value == -7 and all(v == 0 for v in out)
    # the state's filter
    value = ctypes.c_int(0)
    assert lib.gr_render_state_set_filter(None, gra.FILTER_TENT) == INVALID and last_error_names("gr_render_state_set_filter")
    assert lib.gr_render_state_filter(None, ctypes.byref(value)) == INVALID and last_error_names("gr_render_state_filter")
    with pytest.raises(gra.GeodesicError, match="gr_filter_taps"):
        filter_taps("box", 2)
    with pytest.raises(ValueError):
        filter_taps("lanczos", 2)
    with pytest.raises(ValueError):
        filter_frame(np.zeros((5, 4, 4), np.float32), 2, taps)
    with pytest.raises(gra.GeodesicError, match="gr_filter_frame.*parity"):
        filter_frame(np.zeros((4, 4, 4), np.float32), 2, taps[:3])


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """gr_filter_frame on heap buffers of exactly the frames' sizes, address and undefined-behaviour sanitizers on: the host code alone
    with a main of its own (tests/filter_frame_check.cpp) - nothing is loaded into this process"""
    csrc = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")
    exe = str(tmp_path / "filter_frame_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "filter_frame_check.cpp"), os.path.join(csrc, "imageio.cpp"), "-lz", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "uneven: 1 x 1 at factor 4, 16 taps: 0 of 4 values differ" in lines
    assert len([line for line in lines if line.endswith("values differ")]) == 3 * 4 * 6 + 4 and "AddressSanitizer" not in r.stderr


def test_the_kernel_is_part_of_the_setup_module_only():
    here = os.path.join(os.path.dirname(gra.__file__), "csrc")
    capi = open(os.path.join(here, "capi.cpp")).read()
    program_build = open(os.path.join(here, "program_build.cpp")).read()
    lists = {name: re.findall(r'"([a-z_]+\.(?:hip|inc))"', body) for name, body in re.findall(r"const (\w*PARTS)\[\] = \{(.*?)\};", program_build, flags=re.S)}
    frame_files, setup_files = lists["KERNEL_PARTS"], lists["PARTS"]
    assert "filter.hip" in setup_files and "filter.hip" not in frame_files
    assert setup_files.index("resolve.hip") + 1 == setup_files.index("filter.hip")
    assert re.search(r"is_setup_kernel\(int k\) \{[^}]*K_RESOLVE_FILTERED", capi)
    kernel = open(os.path.join(here, "kernels", "filter.hip")).read()
    assert "gr_resolve_filtered(" in kernel and "__syncthreads()" in kernel
    for other in frame_files:
        assert "gr_resolve_filtered" not in open(os.path.join(here, "kernels", other)).read(), other


def test_the_cli_refuses_a_filter_it_cannot_render(capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for argv, names in ((["--filter", "mitchell", "--devices", "0,1"], "--devices"), (["--filter", "tent", "--supersample", "2", "--devices", "0"], "--devices")):
        for out in ("x.png", "x.y4m"):
            with pytest.raises(SystemExit) as e:
                render.main(["--metric", "kerr_boyer", "--out", out] + argv)
            err = capsys.readouterr().err
            assert e.value.code == 2 and "--filter" in err and names in err, (argv, err[-300:])
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--out", "x.png", "--filter", "lanczos"])
    assert e.value.code == 2 and "--filter" in capsys.readouterr().err
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="filter"):
        render.render("kerr_boyer", 8, 8, filter="lanczos")
