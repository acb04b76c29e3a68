"""GPU tests (-m gpu) of the PNG runs stream made on the device (gr_png_histogram_runs and gr_png_pack_runs of kernels/png.hip behind an
encoder of gr_png_encoder_create_as): the device's file equals the host encoder's of that kind (gr_png_encode_rgba8_host_as, the
definition) byte for byte and decodes to the input - widths either side of a group of 64 pixels, of a wave and of a pass of 256 lanes, one
to three rows, the contents the tokeniser can go wrong on (tests/png_runs_model.py), every run length at every phase of a group; segment
ends at every byte phase of a word, an output at an odd host address, the stream scratch between its guard words after every encode; one
encoder for several frames, and a literals and a runs encoder in turn on one stream; a rendered frame; the CLI."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
import png_runs_model as model  # noqa: E402
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

WIDTHS = (1, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
HEIGHTS = (1, 2, 3)
_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file (the PNG kernels are in every program's set-up module)"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def encode_into(encoder, pixels, offset=0):
    """gr_png_encode_rgba8 of host pixels uploaded to the device, into a host array `offset` bytes past its start; the encoder's stream
    scratch is checked against its guard words afterwards"""
    height, width = pixels.shape[:2]
    frame = DeviceBuffer.from_numpy(0, pixels)
    bound = gra.png_encode_bound(width, height)
    out = np.full(bound + offset + 16, 0xEE, np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_png_encode_rgba8(encoder.handle, None, frame.ptr, ctypes.c_void_p(out.ctypes.data + offset), bound, ctypes.byref(size)))
    assert encoder.scratch_intact(), "the pack kernel wrote outside its stream"
    assert (out[:offset] == 0xEE).all() and (out[offset + size.value:] == 0xEE).all()
    return out[offset:offset + size.value].tobytes()


@pytest.mark.parametrize("width", WIDTHS)
def test_the_device_file_is_the_host_file(width):
    _, prog, _ = kerr()
    for height in HEIGHTS:
        encoder = gra.PngEncoder(prog, width, height, gra.PNG_STREAM_RUNS)
        for name, pixels in model.contents(width, height).items():
            want = gra.png_encode_host(pixels, gra.PNG_STREAM_RUNS)
            got = encode_into(encoder, pixels)
            assert got == want, (width, height, name)
            assert np.array_equal(model.decoded(got), pixels), (width, height, name)
        encoder.close()


def test_every_run_length_at_every_phase_and_the_two_symbol_frame():
    _, prog, _ = kerr()
    for pixels in (model.every_run_at_every_phase(), model.one_literal_one_length()):
        encoder = gra.PngEncoder(prog, pixels.shape[1], pixels.shape[0], "runs")
        got = encode_into(encoder, pixels)
        assert got == gra.png_encode_host(pixels, "runs")
        assert np.array_equal(model.decoded(got), pixels)
        encoder.close()


def test_every_byte_phase_of_a_segment_end_occurs():
    """(over the frames above the rows' segments end at every residue of a byte offset mod 4, in the runs stream as in the literal one)"""
    phases = set()
    for width in WIDTHS:
        for name, pixels in model.contents(width, 3).items():
            stream = model.zlib_stream_of(gra.png_encode_host(pixels, "runs"))[2]
            at = 0
            while True:
                at = stream.find(b"\x00\x00\xff\xff", at)
                if at < 0:
                    break
                at += 4
                phases.add((at - 2) % 4)       # (the stream's first two bytes are the zlib header, not a segment's)
    assert phases == {0, 1, 2, 3}


def test_an_output_at_an_odd_host_address():
    _, prog, _ = kerr()
    pixels = model.contents(65, 3)["random_runs"]
    encoder = gra.PngEncoder(prog, 65, 3, "runs")
    for offset in (1, 3):
        assert encode_into(encoder, pixels, offset=offset) == gra.png_encode_host(pixels, "runs")
    encoder.close()


def test_an_encoder_serves_frame_after_frame_and_the_two_kinds_take_turns():
    """one runs encoder and one literals encoder of one size, in turn on one stream over frames whose streams differ in length: each file
    is its own kind's host file, and what a longer stream left in a scratch does not show in a shorter one"""
    _, prog, _ = kerr()
    width, height = 130, 3
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    runs, literals = gra.PngEncoder(prog, width, height, "runs"), gra.PngEncoder(prog, width, height)
    assert (runs.stream_kind, literals.stream_kind) == (gra.PNG_STREAM_RUNS, gra.PNG_STREAM_LITERALS)
    frames = model.contents(width, height)
    for name in ("noise", "zero", "random_runs", "gradient", "noise"):
        pixels = frames[name]
        frame = DeviceBuffer.from_numpy(0, pixels)
        want_runs, want_literals = gra.png_encode_host(pixels, "runs"), gra.png_encode_host(pixels)
        assert runs.encode(frame.ptr, stream) == want_runs, name
        assert literals.encode(frame.ptr, stream) == want_literals, name
        assert runs.encode(frame.ptr, stream) == want_runs, name
        assert runs.scratch_intact() and literals.scratch_intact()
        if name in ("zero", "random_runs", "gradient"):
            assert len(want_runs) < len(want_literals), name
    runs.time_launches()
    assert runs.encode(frame.ptr, stream) == want_runs
    histogram_ms, pack_ms = runs.launch_ms()
    assert histogram_ms > 0 and pack_ms > 0
    runs.close()
    literals.close()
    check(lib.gr_stream_destroy(stream))


def test_a_rendered_frame_decodes_to_its_bytes():
    metric, prog, cfgv = kerr()
    width, height = 96, 64
    state = gra.RenderState(width, height, 0)
    dbg, levels = background()
    out = DeviceBuffer(0, width * height * 4)
    state.render_rgba8(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                       gra.frame_options(mode=gra.MODE_FUSED))
    encoder = gra.PngEncoder(prog, width, height, "runs")
    png = encoder.encode(out.ptr)       # (on the frame's stream: it queues behind the frame)
    assert encoder.scratch_intact()
    pixels = out.to_numpy(np.uint8, (height, width, 4))
    assert len(np.unique(pixels)) > 16                        # a picture, not a blank frame
    assert png == gra.png_encode_host(pixels, "runs")
    assert np.array_equal(model.decoded(png), pixels)
    encoder.close()


def test_the_cli_writes_a_runs_png_made_on_the_device(tmp_path):
    from geodesic_raytracing_amd import render
    paths = {"host": str(tmp_path / "host.png"), "runs": str(tmp_path / "runs.png")}
    common = ["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "96x54", "--encode", "device"]
    assert render.main(common + ["--png", "host", "--out", paths["host"]]) == 0
    assert render.main(common + ["--png", "device", "--png-stream", "runs", "--out", paths["runs"]]) == 0
    pixels = render.read_png(paths["host"])
    assert np.array_equal(render.read_png(paths["runs"]), pixels)
    data = open(paths["runs"], "rb").read()
    assert data == gra.png_encode_host(pixels, "runs") and np.array_equal(model.decoded(data), pixels)
