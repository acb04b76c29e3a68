"""CPU tests of the PNG runs stream (GR_PNG_STREAM_RUNS: include/geodesic_hip_internal.h, "PNG frames"; csrc/png_stream.cpp): the host
encoder gr_png_encode_rgba8_host_as against an independent writer of the stream (tests/png_runs_model.py) byte for byte, against zlib and
PIL as decoders, against gr_png_encode_bound; kind 0 through the new entry points against the old ones; the contents the tokeniser can
go wrong on; the refusals; the exports, the kernels' place and the CLI's refusal; the host encoder of both kinds under the sanitizers in a
stand-alone program (tests/png_runs_check.cpp)."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
import png_runs_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS, HEIGHTS = (1, 2, 63, 64, 65, 129), (1, 2, 5)


def check_file(pixels, what):
    """the runs file of the host encoder: the independent writer's, decodes to the pixels, within the bound"""
    png = gra.png_encode_host(pixels, gra.PNG_STREAM_RUNS)
    assert png == model.encode_runs(pixels), what
    assert np.array_equal(model.decoded(png), pixels), what
    assert len(png) <= gra.png_encode_bound(pixels.shape[1], pixels.shape[0]), what
    try:
        from PIL import Image
    except ImportError:
        return png
    assert np.array_equal(np.array(Image.open(io.BytesIO(png)).convert("RGBA")), pixels), what
    return png


@pytest.mark.parametrize("width", WIDTHS)
def test_the_host_file_is_the_independent_writers_and_decodes(width):
    for height in HEIGHTS:
        for name, pixels in model.contents(width, height).items():
            check_file(pixels, (width, height, name))


@pytest.mark.parametrize("width", WIDTHS)
def test_kind_0_through_the_new_entry_point_is_the_old_file(width):
    for height in HEIGHTS:
        for name, pixels in model.contents(width, height).items():
            assert gra.png_encode_host(pixels, gra.PNG_STREAM_LITERALS) == gra.png_encode_host(pixels), (width, height, name)
            assert gra.png_encode_host(pixels, "literals") == gra.png_encode_host(pixels)


def test_kind_0_of_the_table_builder_is_the_old_table():
    rng = np.random.default_rng(3)
    histogram = rng.integers(0, 50, 257).astype(np.uint64)
    old = (np.zeros(257, np.uint8), np.zeros(257, np.uint16), np.zeros(128, np.uint32), ctypes.c_int())
    gra.check(gra.lib.gr_png_build_table(histogram.ctypes.data, old[0].ctypes.data, old[1].ctypes.data, old[2].ctypes.data, ctypes.byref(old[3])))
    new = model.build_table(histogram, model.LITERALS)
    assert all(np.array_equal(a, b) for a, b in zip(old[:3], new[:3])) and old[3].value == new[3]


def test_a_constant_frame_is_runs_of_64_pixels_and_63_in_the_first_group():
    pixels = np.zeros((3, 200, 4), np.uint8)
    for row in model.filtered_words(pixels):
        run = model.tokens_of_row(row)
        assert [int(r) for r in run[run >= 0]] == [0, 63, 64, 64, 8]      # pixel 0, then one match a group
    png = check_file(pixels, "zero")
    # 3 rows of 4 literals and 4 matches against 3 x 800 literals: the file is a fraction of the literal stream's
    assert len(png) < len(gra.png_encode_host(pixels)) / 2


def test_every_run_length_at_every_phase():
    pixels = model.every_run_at_every_phase()
    seen = set()
    for p, row in enumerate(model.filtered_words(pixels)):
        run = model.tokens_of_row(row)
        for x in np.flatnonzero(run > 0):
            seen.add((int(x) % 64, int(run[x])))
        # what the row was made to hold: L repeats from phase p on are one match, or two where they pass the end of the group
        for L in range(1, 65):
            assert (p, min(L, 64 - p)) in seen, (p, L)
            if L > 64 - p:
                assert (0, L - (64 - p)) in seen, (p, L)
    assert {(p, r) for p in range(64) for r in range(1, 65 - p)} <= seen
    check_file(pixels, "every run at every phase")


def test_runs_at_a_group_boundary():
    frames = model.contents(129, 2)
    run = model.tokens_of_row(model.filtered_words(frames["ends_on_boundary"])[1])
    assert run[60] == 4 and run[64] == 0 and run[124] == 4 and run[128] == 0
    run = model.tokens_of_row(model.filtered_words(frames["straddles_boundary"])[1])
    assert run[60] == 4 and run[64] == 4 and run[68] == 0                  # repeats 60 ... 67: two matches
    run = model.tokens_of_row(model.filtered_words(frames["at_boundary_only"])[1])
    assert [int(x) for x in np.flatnonzero(run)] == [64, 128] and run[64] == 1 and run[128] == 1


def test_white_noise_has_no_match_and_still_four_distance_lengths():
    pixels = model.contents(129, 5)["noise"]
    assert all((model.tokens_of_row(row) == 0).all() for row in model.filtered_words(pixels))
    png = check_file(pixels, "noise")
    hlit, hdist, sent = model.first_block_header(png)
    assert (hlit, hdist) == (285, 4) and sent[285:] == [0, 0, 0, 1] and not any(sent[257:285])
    # the literal stream of the same pixels sends 257 + 1
    hlit, hdist, sent = model.first_block_header(gra.png_encode_host(pixels))
    assert (hlit, hdist) == (257, 1) and sent[257:] == [0]


def test_a_frame_of_one_literal_and_one_length():
    pixels = model.one_literal_one_length()
    run = model.tokens_of_row(model.filtered_words(pixels)[0])
    assert run[0] == 0 and run[1] == 63 and (run[2:] == -1).all()
    png = check_file(pixels, "one literal, one length")
    _, _, sent = model.first_block_header(png)
    assert [s for s, length in enumerate(sent[:285]) if length] == [1, 256, 284]
    assert model.length_symbol(252) == (284, 5, 25)


def test_the_length_symbols_are_rfc_1951s():
    """the encoder computes them; here they are looked up in the RFC's table: every length the stream can hold, through a frame that holds it"""
    assert model.length_symbol(4) == (258, 0, 0) and model.length_symbol(12) == (265, 1, 1) and model.length_symbol(256) == (284, 5, 29)
    for run in range(1, 65):
        q = np.arange(1, 130, dtype=np.uint32)[None, :].copy()
        q[0, 65:65 + run] = q[0, 64]                      # `run` repeats from pixel 65 on: one match (run <= 63) ...
        if run == 64:
            q = np.full((1, 129), 7, np.uint32)           # ... and the one of 64 pixels is a whole group of repeats
        check_file(model.pixels_of(q), run)


def test_refusals_name_the_entry_point():
    lib = gra.lib
    pixels = np.zeros((4, 4, 4), np.uint8)
    bound = gra.png_encode_bound(4, 4)
    out = np.zeros(bound + 8, np.uint8)
    size = ctypes.c_size_t()

    def host(frame=pixels.ctypes.data, width=4, height=4, to=out.ctypes.data, capacity=bound, got=ctypes.byref(size), kind=1):
        return lib.gr_png_encode_rgba8_host_as(frame, width, height, to, capacity, got, kind), lib.gr_last_error().decode()

    for kind in (0, 1):
        for call, what in ((dict(frame=None), "NULL"), (dict(to=None), "NULL"), (dict(got=None), "NULL"), (dict(width=0), "size below 1"),
                           (dict(height=-3), "size below 1"), (dict(frame=pixels.ctypes.data + 1), "aligned to 4 bytes"),
                           (dict(width=32768, height=16384), "2^31 - 1 raw bytes")):
            rc, message = host(kind=kind, **call)
            assert rc == -1 and message.startswith("gr_png_encode_rgba8_host_as: ") and what in message, (call, message)
        rc, message = host(kind=kind, capacity=bound - 1)
        assert rc == -5 and message.startswith("gr_png_encode_rgba8_host_as: ") and "capacity" in message and str(bound) in message
        assert host(kind=kind, to=out.ctypes.data + 1)[0] == 0          # the output needs no alignment
    for kind in (2, -1, 256):
        before = out.copy()
        rc, message = host(kind=kind)
        assert rc == -1 and message.startswith("gr_png_encode_rgba8_host_as: ") and "unknown stream kind" in message and str(kind) in message
        assert np.array_equal(out, before)                              # nothing written
    # the table builder's
    histogram, lengths, codes, header, bits = np.ones(285, np.uint64), np.zeros(285, np.uint8), np.zeros(285, np.uint16), np.zeros(128, np.uint32), ctypes.c_int()
    good = [histogram.ctypes.data, 1, lengths.ctypes.data, codes.ctypes.data, header.ctypes.data, ctypes.byref(bits)]
    assert lib.gr_png_build_table_as(*good) == 0
    for i in (0, 2, 3, 4, 5):
        assert lib.gr_png_build_table_as(*[None if k == i else v for k, v in enumerate(good)]) == -1
        assert lib.gr_last_error().decode().startswith("gr_png_build_table_as: ") and "NULL" in lib.gr_last_error().decode()
    assert lib.gr_png_build_table_as(*[7 if k == 1 else v for k, v in enumerate(good)]) == -1
    assert lib.gr_last_error().decode().startswith("gr_png_build_table_as: ") and "unknown stream kind 7" in lib.gr_last_error().decode()
    # the device encoder's, before any device call: refused where no device exists
    handle = ctypes.c_void_p()
    for args, what in (((None, 4, 4, 1, ctypes.byref(handle)), "NULL"), ((ctypes.c_void_p(8), 4, 4, 1, None), "NULL"),
                       ((ctypes.c_void_p(8), 0, 4, 1, ctypes.byref(handle)), "size below 1"),
                       ((ctypes.c_void_p(8), 32768, 16384, 1, ctypes.byref(handle)), "2^31 - 1 raw bytes"),
                       ((ctypes.c_void_p(8), 4, 4, 2, ctypes.byref(handle)), "unknown stream kind 2"),
                       ((ctypes.c_void_p(8), 4, 4, -1, ctypes.byref(handle)), "unknown stream kind -1")):
        assert lib.gr_png_encoder_create_as(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_png_encoder_create_as: ") and what in message, message
    assert not handle.value
    # and Python's names of the kinds
    with pytest.raises(ValueError, match="stream kind"):
        gra.png_encode_host(pixels, "matches")


def test_the_table_of_285_symbols():
    rng = np.random.default_rng(11)
    histogram = np.zeros(285, np.uint64)
    histogram[rng.choice(285, 90, replace=False)] = rng.integers(1, 10000, 90).astype(np.uint64)
    histogram[256] = 5
    lengths, codes, header, header_bits = model.build_table(histogram)
    used = np.flatnonzero(histogram)
    assert (lengths[used] > 0).all() and (lengths[histogram == 0] == 0).all() and lengths.max() <= 15
    assert sum(2 ** (15 - int(n)) for n in lengths if n) == 2 ** 15              # Kraft's sum is exactly 1
    assert len({(int(lengths[s]), int(codes[s])) for s in used}) == len(used)
    assert header_bits <= 74 + 289 * 7                                           # the bound's argument (the header)
    # the deepest tree the limit of 15 has to cut, over all 285 symbols
    a, b = 1, 1
    fibonacci = np.zeros(285, np.uint64)
    for s in range(0, 285, 7):
        fibonacci[s] = a
        a, b = b, a + b
    fibonacci[256] = 1
    lengths = model.build_table(fibonacci)[0]
    assert lengths.max() == 15 and sum(2 ** (15 - int(n)) for n in lengths if n) == 2 ** 15


def test_exports_kernels_and_bindings():
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    for name in ("gr_png_encode_rgba8_host_as", "gr_png_encoder_create_as", "gr_png_build_table_as"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in gra.EXPORTED_SYMBOLS and hasattr(gra.lib, name)
    assert re.search(r"enum \{ GR_PNG_STREAM_LITERALS = 0, GR_PNG_STREAM_RUNS = 1 \};", header)
    assert (gra.PNG_STREAM_LITERALS, gra.PNG_STREAM_RUNS) == (0, 1) and gra.PNG_STREAM_NAMES == {"literals": 0, "runs": 1}
    here = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")
    source, capi = open(os.path.join(here, "kernels", "png.hip")).read(), open(os.path.join(here, "capi.cpp")).read()
    for kernel in ("gr_png_histogram_runs", "gr_png_pack_runs"):
        assert f'extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) {kernel}(' in source
        assert f'"{kernel}"' in capi and re.search(rf"is_setup_kernel\(int k\) \{{[^}}]*K_{kernel[3:].upper()}\b", capi)
    assert "png_histogram_row<1>" in source and "png_pack_row<1>" in source and "png_histogram_row<0>" in source and "png_pack_row<0>" in source


def test_the_setup_module_holds_the_runs_kernels_and_the_frame_path_does_not(tmp_path, monkeypatch):
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("minkowski").argument_string().encode()))
    (setup,) = list(tmp_path.glob("*.setup.hsaco"))
    blob = setup.read_bytes()
    assert b"gr_png_histogram_runs" in blob and b"gr_png_pack_runs" in blob and b"gr_png_pack" in blob
    for other in tmp_path.glob("*.hsaco"):
        if other != setup:
            assert b"gr_png_pack_runs" not in other.read_bytes()


def test_cli_refuses_a_stream_kind_without_png_device(capsys):
    from geodesic_raytracing_amd.render import main, render
    for extra in ([], ["--png", "host"]):
        with pytest.raises(SystemExit):
            main(["--metric", "minkowski", "--png-stream", "runs", "--out", "frame.png"] + extra)
        err = capsys.readouterr().err
        assert "--png-stream runs" in err and "--png device" in err
    with pytest.raises(SystemExit):
        main(["--metric", "minkowski", "--png", "device", "--png-stream", "lz77", "--out", "frame.png"])
    assert "--png-stream" in capsys.readouterr().err
    with pytest.raises(ValueError, match="png_stream"):
        render("minkowski", 8, 8, png="host", png_stream="runs")
    with pytest.raises(ValueError, match="png_stream"):
        render("minkowski", 8, 8, png="device", rgba8=True, png_stream="lz77")


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """the host encoder of both kinds on heap buffers of exactly the frame's size and exactly gr_png_encode_bound bytes, address and
    undefined-behaviour sanitizers on: the host code alone with a main of its own (tests/png_runs_check.cpp) - nothing is loaded into
    this process"""
    csrc = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")
    exe = str(tmp_path / "png_runs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "png_runs_check.cpp"), os.path.join(csrc, "png_stream.cpp"), "-lz", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert len([line for line in lines if line.endswith("inflates to the filtered rows")]) == 2 * 9 * 3 * 4
