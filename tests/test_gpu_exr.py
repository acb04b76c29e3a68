"""GPU tests (-m gpu) of OpenEXR frames encoded on the device (kernels/exr.hip behind gr_exr_encode_f32): the device's file equals the host
encoder's (gr_exr_encode_f32_host, the definition) byte for byte and decodes, through the independent reader of tests/exr_model.py, to
numpy's halfs of the input - rows shorter than a wave, rows around one and two passes of the pack kernel a plane, chunk ends at every byte
phase of a word, one, two and five rows, zeros, a gradient, random half bit patterns, the specials, raw rows between compressed ones and
the reverse; an output at an odd host address; the encoder's chunk scratch between its guard words; one encoder for several frames; a
rendered star-sky frame with values above 1; the CLI's two ways to the same file."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import exr_model as model  # noqa: E402
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from test_gpu_fullsize import SCRIPTS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SOURCE = open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "kernels", "exr.hip")).read()
# bytes of the reordered row a pass of gr_exr_pack covers - and so pixels of a plane's low or high bytes
PASS = int(re.search(r"#define GR_EXR_LANES (\d+)", _SOURCE).group(1)) * int(re.search(r"#define GR_EXR_ITEM_BYTES (\d+)", _SOURCE).group(1))
WIDTHS = [1, 3, 63, 64, 65, 255, 256, 257, PASS - 1, PASS, PASS + 1, 2 * PASS - 1, 2 * PASS, 2 * PASS + 1]
HEIGHTS = (1, 2, 5)

_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file (the EXR kernels are in every program's set-up module)"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def frames(width, height):
    """the contents of a size, and for five rows the frames whose rows alternate between raw and compressed"""
    found = dict(model.contents(width, height))
    if height == 5:
        found["mixed"] = model.rows_of("nssns", width)
        found["alternating"] = model.rows_of("snsns", width)
    return found


def device_exr(encoder, frame, offset=0):
    """gr_exr_encode_f32 of a host frame uploaded to the device, into a host array `offset` bytes past its start; the encoder's chunk
    scratch is checked against its guard words afterwards"""
    height, width = frame.shape[:2]
    on_device = DeviceBuffer.from_numpy(0, frame)
    bound = gra.exr_encode_bound(width, height)
    out = np.full(bound + offset + 16, 0xEE, np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_exr_encode_f32(encoder.handle, None, on_device.ptr, ctypes.c_void_p(out.ctypes.data + offset), bound, ctypes.byref(size)))
    assert encoder.scratch_intact(), "the pack kernel wrote outside its chunks"
    assert (out[:offset] == 0xEE).all() and (out[offset + size.value:] == 0xEE).all()
    return out[offset:offset + size.value].tobytes()


@pytest.mark.parametrize("width", WIDTHS)
def test_the_device_file_is_the_host_file(width):
    _, prog, _ = kerr()
    for height in HEIGHTS:
        encoder = gra.ExrEncoder(prog, width, height)
        for name, frame in frames(width, height).items():
            want = gra.exr_encode_host(frame)
            got = device_exr(encoder, frame)
            assert got == want, (width, height, name)
            halfs, _kinds, _ends = model.read_exr(got, width, height)
            assert np.array_equal(halfs, model.expected_halfs(frame)), (width, height, name)
        encoder.close()


def test_every_byte_phase_and_both_kinds_of_neighbour_occur():
    """(what the frames above are chosen for, on the host file: over them the chunks end at every residue of a file offset mod 4 - the chunk
    area starts at 313 + 8 height, so the device's own offsets see every phase too -, a raw row lies between two compressed ones and a
    compressed row between two raw ones)"""
    phases, in_stream = set(), set()
    for width in WIDTHS:
        for height in HEIGHTS:
            for frame in frames(width, height).values():
                ends = model.read_exr(gra.exr_encode_host(frame), width, height)[2]
                phases.update(end % 4 for end in ends)
                in_stream.update((end - 313 - 8 * height) % 4 for end in ends)
    assert phases == {0, 1, 2, 3} and in_stream == {0, 1, 2, 3}
    for width in (65, 257, PASS + 1):
        assert model.read_exr(gra.exr_encode_host(model.rows_of("nssns", width)), width, 5)[1] == ["raw", "zip", "zip", "raw", "zip"], width
        assert model.read_exr(gra.exr_encode_host(model.rows_of("snsns", width)), width, 5)[1] == ["zip", "raw", "zip", "raw", "zip"], width


def test_an_output_at_an_odd_host_address():
    _, prog, _ = kerr()
    frame = model.mixed(65)
    encoder = gra.ExrEncoder(prog, 65, 5)
    assert device_exr(encoder, frame, offset=3) == gra.exr_encode_host(frame)


def test_an_encoder_serves_frame_after_frame():
    """one encoder, frames of one size whose chunks differ in kind and length: each file is the host's, and what a longer chunk area left
    in the scratch does not show in a shorter one"""
    _, prog, _ = kerr()
    width, height = 130, 5
    encoder = gra.ExrEncoder(prog, width, height)
    for name in ("noise", "zero", "mixed", "smooth", "specials", "alternating", "noise"):
        frame = frames(width, height)[name]
        on_device = DeviceBuffer.from_numpy(0, frame)
        assert encoder.encode(on_device.ptr) == gra.exr_encode_host(frame), name
        assert encoder.scratch_intact()
    encoder.time_launches()
    assert encoder.encode(on_device.ptr) == gra.exr_encode_host(frame)
    histogram_ms, pack_ms = encoder.launch_ms()
    assert histogram_ms > 0 and pack_ms > 0


def test_a_rendered_star_sky_frame_decodes_to_its_halfs(tmp_path):
    from geodesic_raytracing_amd.render import StarField, glare_of
    metric, prog, cfgv = kerr()
    width, height = 96, 64
    state = gra.RenderState(width, height, 0, stars=StarField(20000, 7).on(prog), glare=glare_of(None, 16.0))      # (sixteen stops up: pixels this large make stars faint)
    out = DeviceBuffer(0, width * height * 16)
    state.render(prog, metric, gra.default_camera(), out.ptr, None, metric.features(adaptive_sampling=0), cfgv, gra.frame_options(mode=gra.MODE_FUSED))
    encoder = gra.ExrEncoder(prog, width, height)
    data = encoder.encode(out.ptr)       # (on the frame's stream: it queues behind the frame)
    frame = out.to_numpy(np.float32, (height, width, 4))
    assert frame[..., :3].max() > 1.0 and len(np.unique(frame[..., :3])) > 16          # a picture no 8-bit file holds
    assert data == gra.exr_encode_host(frame)
    halfs, kinds, _ends = model.read_exr(data, width, height)
    assert np.array_equal(halfs, model.expected_halfs(frame))
    assert halfs.view(np.float16).max() > 1.0
    assert encoder.scratch_intact()
    path = tmp_path / "frame.exr"
    assert encoder.write(str(path), out.ptr) == len(data) and path.read_bytes() == data


def test_the_cli_writes_the_same_file_either_way(tmp_path):
    from geodesic_raytracing_amd import render
    paths = {}
    for where in ("host", "device"):
        paths[where] = tmp_path / f"{where}.exr"
        assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "96x54", "--sky", "stars:20000:7", "--exposure", "16", "--exr", where,
                            "--out", str(paths[where])]) == 0
    assert paths["device"].read_bytes() == paths["host"].read_bytes()
    halfs = model.read_exr(paths["device"].read_bytes(), 96, 54)[0]
    assert halfs.view(np.float16).max() > 1.0
