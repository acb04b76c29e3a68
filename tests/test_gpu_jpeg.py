"""GPU tests (-m gpu) of JPEG frames encoded on the device (kernels/jpeg.hip behind gr_jpeg_encode_rgba8): the device's file equals the host
encoder's (gr_jpeg_encode_rgba8_host, the definition) byte for byte - the sizes of tests/test_jpeg_stream.py, widths around what one pass of
a gr_jpeg_pack workgroup covers, a flat MCU row between two busy ones, four contents at three qualities; an output at an odd host address;
the encoder's scratch between its guard words after every encode; one encoder for frame after frame; the launch times; a rendered frame."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from test_gpu_fullsize import SCRIPTS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 16), (16, 17), (33, 18), (16, 160)]
QUALITIES = [1, 90, 100]
# the MCUs one pass of a gr_jpeg_pack workgroup covers (a lane a block, six blocks an MCU), read from the kernel's source
GR_JPEG_PACK_MCUS = int(re.search(r"#define GR_JPEG_PACK_MCUS (\d+)", open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "kernels", "jpeg.hip")).read()).group(1))
_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file (the JPEG kernels are in every program's set-up module)"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def contents(width, height):
    rng = np.random.default_rng(7 * width + height)
    y, x = np.mgrid[0:height, 0:width]
    gradient = np.stack([(x * 3) & 255, (y * 5 + x) & 255, (255 - x - y) & 255, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    checkerboard = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1)
    return {"random": rng.integers(0, 256, (height, width, 4), dtype=np.uint8), "flat": np.full((height, width, 4), (10, 200, 30, 255), np.uint8),
            "gradient": gradient, "checkerboard": checkerboard}


def device_jpeg(pixels, quality, offset=0):
    """gr_jpeg_encode_rgba8 of host pixels uploaded to the device, into a host array `offset` bytes past its start and guarded on both sides;
    the encoder's scratch is checked against its guard words afterwards"""
    _, prog, _ = kerr()
    height, width = pixels.shape[:2]
    frame = DeviceBuffer.from_numpy(0, np.ascontiguousarray(pixels))
    encoder = gra.JpegEncoder(prog, width, height, quality)
    bound = gra.jpeg_encode_bound(width, height)
    out = np.full(bound + offset + 16, 0xEE, np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_jpeg_encode_rgba8(encoder.handle, None, frame.ptr, ctypes.c_void_p(out.ctypes.data + offset), bound, ctypes.byref(size)))
    assert encoder.scratch_intact(), "a kernel wrote outside its region of the scratch"
    assert (out[:offset] == 0xEE).all() and (out[offset + size.value:] == 0xEE).all()
    encoder.close()
    return out[offset:offset + size.value].tobytes()


@pytest.mark.parametrize("width,height", SIZES)
def test_the_device_file_is_the_host_file(width, height):
    for name, pixels in contents(width, height).items():
        for quality in QUALITIES:
            assert device_jpeg(pixels, quality) == gra.jpeg_encode_host(pixels, quality), (width, height, name, quality)


@pytest.mark.parametrize("mcus", [GR_JPEG_PACK_MCUS - 1, GR_JPEG_PACK_MCUS, GR_JPEG_PACK_MCUS + 1])
def test_widths_around_one_pass_of_the_pack_workgroup(mcus):
    """one MCU fewer than, exactly, and one more than GR_JPEG_PACK_MCUS; random pixels at quality 100 also fill more than one LDS window a pass"""
    assert GR_JPEG_PACK_MCUS == 64
    width, height = 16 * mcus, 17
    for name, quality in (("random", 100), ("random", 1), ("gradient", 90), ("checkerboard", 100), ("flat", 90)):
        pixels = contents(width, height)[name]
        assert device_jpeg(pixels, quality) == gra.jpeg_encode_host(pixels, quality), (mcus, name, quality)


def test_a_flat_row_between_two_busy_ones():
    """three MCU rows, the middle one flat: the shortest and the longest segments are neighbours"""
    pixels = contents(200, 48)["random"]
    pixels[16:32] = (40, 40, 40, 255)
    for quality in QUALITIES:
        assert device_jpeg(pixels, quality) == gra.jpeg_encode_host(pixels, quality), quality


def test_an_output_at_an_odd_host_address():
    pixels = contents(65, 35)["random"]
    assert device_jpeg(pixels, 90, offset=3) == gra.jpeg_encode_host(pixels, 90)


def test_an_encoder_serves_frame_after_frame():
    """one encoder, frames of one size whose files differ in length: each file is the host's, and what a longer one left in the scratch does
    not show in a shorter one; with time_launches on, launch_ms gives three positive times"""
    _, prog, _ = kerr()
    width, height = 130, 40
    encoder = gra.JpegEncoder(prog, width, height, 100)
    for name in ("random", "flat", "gradient", "random", "checkerboard"):
        pixels = contents(width, height)[name]
        frame = DeviceBuffer.from_numpy(0, pixels)
        assert encoder.encode(frame.ptr) == gra.jpeg_encode_host(pixels, 100), name
        assert encoder.scratch_intact()
    encoder.time_launches()
    assert encoder.encode(frame.ptr) == gra.jpeg_encode_host(pixels, 100)
    times = encoder.launch_ms()
    assert len(times) == 3 and all(ms > 0 for ms in times)


def test_a_rendered_frame_through_render():
    from geodesic_raytracing_amd.render import render
    files = {where: render("kerr_boyer", 64, 48, SCRIPTS, {"a": 0.45}, rgba8=True, jpeg=where, quality=90) for where in ("device", "host")}
    assert files["device"] == files["host"] and files["host"][:2] == b"\xff\xd8"
    pixels = render("kerr_boyer", 64, 48, SCRIPTS, {"a": 0.45}, rgba8=True)
    assert len(np.unique(pixels)) > 16                        # a picture, not a flat frame
    assert files["host"] == gra.jpeg_encode_host(pixels, 90)
