"""GPU tests (-m gpu) of PNG frames encoded on the device (kernels/png.hip behind gr_png_encode_rgba8): the device's file equals the host
encoder's (gr_png_encode_rgba8_host, the definition) byte for byte and decodes to the input - rows shorter than a wave, rows around one and
two passes of 256 lanes, segment ends at every byte phase of a word, one, two and five rows, contents that use every literal, the two-leaf
table and a smooth gradient; an output at an odd host address; the encoder's stream scratch between its guard words; a rendered frame."""
import ctypes
import io
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file (the PNG kernels are in every program's set-up module)"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def contents(width, height):
    rng = np.random.default_rng(7 * width + height)
    gradient = np.zeros((height, width, 4), np.uint8)
    gradient[..., 0] = np.arange(width)[None, :] & 255
    gradient[..., 1] = (np.arange(width)[None, :] * 3) & 255
    gradient[..., 2] = (np.arange(height)[:, None] * 5) & 255
    gradient[..., 3] = 255
    return {"random": rng.integers(0, 256, (height, width, 4), dtype=np.uint8), "zero": np.zeros((height, width, 4), np.uint8), "gradient": gradient}


def decoded(png):
    """the pixels of a file of this stream, with zlib alone: chunk CRCs, the Adler-32, Sub on row 0 and Up on the others undone"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, stream, size = 8, b"", None
    while at < len(png):
        (n,) = struct.unpack(">I", png[at:at + 4])
        tag, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        if tag == b"IHDR":
            size = struct.unpack(">II", data[:8])
        if tag == b"IDAT":
            stream += data
        at += 12 + n
    width, height = size
    rows = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(height, 4 * width + 1)
    assert rows[0, 0] == 1 and (rows[1:, 0] == 2).all()
    first = rows[0, 1:].reshape(width, 4).astype(np.uint32).cumsum(axis=0)
    body = np.concatenate([first.reshape(1, -1), rows[1:, 1:].astype(np.uint32)]).cumsum(axis=0)
    return (body & 255).astype(np.uint8).reshape(height, width, 4)


def device_png(pixels, offset=0):
    """gr_png_encode_rgba8 of host pixels uploaded to the device, into a host array `offset` bytes past its start; the encoder's stream
    scratch is checked against its guard words afterwards"""
    _, prog, _ = kerr()
    height, width = pixels.shape[:2]
    frame = DeviceBuffer.from_numpy(0, pixels)
    encoder = gra.PngEncoder(prog, width, height)
    bound = gra.png_encode_bound(width, height)
    out = np.full(bound + offset + 16, 0xEE, np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_png_encode_rgba8(encoder.handle, None, frame.ptr, ctypes.c_void_p(out.ctypes.data + offset), bound, ctypes.byref(size)))
    assert encoder.scratch_intact(), "the pack kernel wrote outside its stream"
    assert (out[:offset] == 0xEE).all() and (out[offset + size.value:] == 0xEE).all()
    encoder.close()
    return out[offset:offset + size.value].tobytes()


@pytest.mark.parametrize("width", [1, 3, 63, 64, 65, 255, 256, 257, 513])
def test_the_device_file_is_the_host_file(width):
    for height in (1, 2, 5):
        for name, pixels in contents(width, height).items():
            want = gra.png_encode_host(pixels)
            got = device_png(pixels)
            assert got == want, (width, height, name)
            assert np.array_equal(decoded(got), pixels), (width, height, name)


def test_every_byte_phase_of_a_segment_end_occurs():
    """(what the widths above are chosen for: over those frames the rows' segments end at every residue of a byte offset mod 4)"""
    phases = set()
    for width in (1, 3, 63, 64, 65, 255, 256, 257, 513):
        pixels = contents(width, 5)["random"]
        stream = b"".join(gra.png_encode_host(pixels).split(b"IDAT")[1:])
        at = 0
        while True:
            at = stream.find(b"\x00\x00\xff\xff", at)
            if at < 0:
                break
            at += 4
            phases.add((at - 2) % 4)       # (the stream's first two bytes are the zlib header, not a segment's)
    assert phases == {0, 1, 2, 3}


def test_an_output_at_an_odd_host_address():
    pixels = contents(65, 5)["random"]
    assert device_png(pixels, offset=3) == gra.png_encode_host(pixels)


def test_an_encoder_serves_frame_after_frame():
    """one encoder, three frames of one size whose streams differ in length: each file is the host's, and what a longer stream left in the
    scratch does not show in a shorter one"""
    _, prog, _ = kerr()
    width, height = 130, 6
    encoder = gra.PngEncoder(prog, width, height)
    for name in ("random", "zero", "gradient", "random"):
        pixels = contents(width, height)[name]
        frame = DeviceBuffer.from_numpy(0, pixels)
        assert encoder.encode(frame.ptr) == gra.png_encode_host(pixels), name
        assert encoder.scratch_intact()
    encoder.time_launches()
    assert encoder.encode(frame.ptr) == gra.png_encode_host(pixels)
    histogram_ms, pack_ms = encoder.launch_ms()
    assert histogram_ms > 0 and pack_ms > 0


def test_a_rendered_frame_decodes_to_its_bytes(tmp_path):
    metric, prog, cfgv = kerr()
    width, height = 64, 48
    state = gra.RenderState(width, height, 0)
    dbg, levels = background()
    out = DeviceBuffer(0, width * height * 4)
    state.render_rgba8(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                       gra.frame_options(mode=gra.MODE_FUSED))
    encoder = gra.PngEncoder(prog, width, height)
    png = encoder.encode(out.ptr)       # (on the frame's stream: it queues behind the frame)
    pixels = out.to_numpy(np.uint8, (height, width, 4))
    assert len(np.unique(pixels)) > 16                        # a picture, not a blank frame
    assert png == gra.png_encode_host(pixels)
    assert np.array_equal(decoded(png), pixels)
    path = tmp_path / "frame.png"
    assert encoder.write(str(path), out.ptr) == len(png)
    from geodesic_raytracing_amd.render import read_png
    assert np.array_equal(read_png(str(path)), pixels)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(io.BytesIO(png)).convert("RGBA")), pixels)


def test_the_cli_writes_a_png_made_on_the_device(tmp_path):
    from geodesic_raytracing_amd import render
    paths = {}
    for where in ("host", "device"):
        paths[where] = str(tmp_path / f"{where}.png")
        assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "96x54", "--encode", "device", "--png", where, "--out", paths[where]]) == 0
    assert np.array_equal(render.read_png(paths["device"]), render.read_png(paths["host"]))
    assert open(paths["device"], "rb").read() == gra.png_encode_host(render.read_png(paths["host"]))
