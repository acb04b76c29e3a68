"""CPU tests of the OpenEXR file both EXR encoders write (csrc/exr_stream.cpp; include/geodesic_hip_internal.h, "EXR frames"): the host
encoder read back by an independent reader (tests/exr_model.py: struct, zlib and numpy alone) and held, bit for bit, to numpy's own
float32 -> float16 conversion; the half conversion on its own; rows stored raw beside rows that compress; width 1; the bound; every
refusal; where the kernels' source is built; the exports; the CLI's refusals; the host encoder under the sanitizers in a stand-alone
program (tests/exr_stream_check.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import exr_model as model
import geodesic_raytracing_amd as gra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")


def test_the_half_conversion_is_numpys():
    values = model.specials()
    with np.errstate(all="ignore"):
        want = np.clip(np.nan_to_num(values, nan=0), -65504, 65504).astype(np.float16).view(np.uint16)
    assert np.array_equal(gra.exr_half_bits(values), want)

    def half(value):
        return int(gra.exr_half_bits(np.array([value], np.float32))[0])

    assert half(np.nan) == 0 and half(-np.nan) == 0                                                       # NaN of either sign: +0
    assert half(np.inf) == 0x7BFF and half(-np.inf) == 0xFBFF and half(65520.0) == 0x7BFF and half(65519.9) == 0x7BFF and half(1e30) == 0x7BFF
    assert half(0.0) == 0 and half(-0.0) == 0x8000
    assert half(2.0 ** -14) == 0x0400 and half(2.0 ** -24) == 0x0001 and half(2.0 ** -25) == 0 and half(-2.0 ** -25) == 0x8000
    assert half(2.0 ** -25 * (1 + 2.0 ** -10)) == 0x0001                                                  # just above the tie: up
    assert half(1 + 2.0 ** -11) == 0x3C00 and half(1 + 3 * 2.0 ** -11) == 0x3C02                          # ties go to even
    # every float32 exponent, a million random bit patterns
    bits = np.random.default_rng(3).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    floats = bits.view(np.float32)
    with np.errstate(all="ignore"):
        want = np.clip(np.nan_to_num(floats, nan=0), -65504, 65504).astype(np.float16).view(np.uint16)
    assert np.array_equal(gra.exr_half_bits(floats), want)


@pytest.mark.parametrize("width,height", [(1, 1), (1, 5), (2, 2), (3, 1), (5, 7), (64, 3), (257, 4)])
def test_the_host_file_decodes_to_numpys_halfs(width, height):
    for name, frame in model.contents(width, height).items():
        data = gra.exr_encode_host(frame)
        halfs, kinds, _ends = model.read_exr(data, width, height)
        assert np.array_equal(halfs, model.expected_halfs(frame)), name
        assert len(data) <= gra.exr_encode_bound(width, height)
        if width == 1:
            assert kinds == ["raw"] * height       # a zlib stream is longer than 6 bytes


def test_raw_rows_beside_compressed_rows():
    frame = model.mixed()
    data = gra.exr_encode_host(frame)
    halfs, kinds, _ends = model.read_exr(data, 257, 5)
    assert np.array_equal(halfs, model.expected_halfs(frame))
    assert kinds == ["raw", "zip", "zip", "raw", "zip"]
    # every row raw: the bound is the file's size exactly
    noise = model.rows_of("nnn", 64)
    data = gra.exr_encode_host(noise)
    assert model.read_exr(data, 64, 3)[1] == ["raw"] * 3 and len(data) == gra.exr_encode_bound(64, 3) == 313 + 8 * 3 + 3 * (8 + 6 * 64)
    # the table counts the rows that end up raw: the compressed rows of the mixed frame are not the rows of a frame without the noise
    smooth_only = gra.exr_encode_host(frame[[1, 2, 4]])
    zipped = [len(c) for c in (data_of_rows(gra.exr_encode_host(frame), 257, 5)[r] for r in (1, 2, 4))]
    assert zipped != [len(c) for c in data_of_rows(smooth_only, 257, 3)]


def data_of_rows(data, width, height):
    ends = model.read_exr(data, width, height)[2]
    starts = [313 + 8 * height] + ends[:-1]
    return [data[a + 8:b] for a, b in zip(starts, ends)]


def test_the_written_file_is_the_encoded_file(tmp_path):
    from geodesic_raytracing_amd.render import write_frame_exr
    frame = model.mixed(33)
    path = tmp_path / "frame.exr"
    write_frame_exr(str(path), frame)
    assert path.read_bytes() == gra.exr_encode_host(frame)
    unaligned = np.zeros(4 * 33 * 5 + 1, np.float32)[1:].reshape(5, 33, 4)      # gr_write_frame_exr asks for no alignment
    unaligned[...] = frame
    write_frame_exr(str(path), unaligned)
    assert path.read_bytes() == gra.exr_encode_host(frame)
    assert gra.lib.gr_write_frame_exr(str(tmp_path / "no" / "such" / "folder.exr").encode(), frame.ctypes.data, 33, 5) == -1
    assert gra.lib.gr_last_error().decode().startswith("gr_write_frame_exr: ")


def test_refusals_name_the_entry_point_and_the_field():
    lib = gra.lib
    frame = np.zeros(4 * 4 * 4 + 8, np.float32)
    frame = frame[(-frame.ctypes.data % 16) // 4:][:64]
    assert frame.ctypes.data % 16 == 0
    bound = gra.exr_encode_bound(4, 4)
    assert bound == 313 + 8 * 4 + 4 * (8 + 24)
    out = np.zeros(bound + 8, np.uint8)
    size = ctypes.c_size_t()

    def host(pixels=frame.ctypes.data, width=4, height=4, to=out.ctypes.data, capacity=bound, got=ctypes.byref(size)):
        return lib.gr_exr_encode_f32_host(pixels, width, height, to, capacity, got), lib.gr_last_error().decode()

    for call, what in ((dict(pixels=None), "NULL"), (dict(to=None), "NULL"), (dict(got=None), "NULL"), (dict(width=0), "size below 1 (width 0"),
                       (dict(height=-3), "height -3"), (dict(pixels=frame.ctypes.data + 4), "frame is not aligned to 16 bytes"),
                       (dict(width=357913942, capacity=1 << 62), "row of more than 2^31 - 1 raw bytes (width 357913942")):
        rc, message = host(**call)
        assert rc == -1 and message.startswith("gr_exr_encode_f32_host: ") and what in message, (call, message)
    rc, message = host(capacity=bound - 1)
    assert rc == -5 and message.startswith("gr_exr_encode_f32_host: ") and "capacity" in message and str(bound) in message
    assert (out == 0).all()                                # a refusal writes nothing
    assert host(to=out.ctypes.data + 1)[0] == 0            # the output needs no alignment
    # the bound's own
    need = ctypes.c_size_t()
    for args, what in (((4, 4, None), "NULL"), ((0, 4, ctypes.byref(need)), "size below 1"), ((4, 0, ctypes.byref(need)), "size below 1"),
                       ((357913942, 1, ctypes.byref(need)), "2^31 - 1 raw bytes")):
        assert lib.gr_exr_encode_bound(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_exr_encode_bound: ") and what in message
    assert lib.gr_exr_encode_bound(357913941, 3, ctypes.byref(need)) == 0 and need.value == 313 + 24 + 3 * (8 + 6 * 357913941)
    # the device encoder's, before any device call: refused where no device exists
    handle = ctypes.c_void_p()
    for args, what in (((None, 4, 4, ctypes.byref(handle)), "NULL"), ((ctypes.c_void_p(8), 4, 4, None), "NULL"),
                       ((ctypes.c_void_p(8), 0, 4, ctypes.byref(handle)), "size below 1"),
                       ((ctypes.c_void_p(8), 357913942, 1, ctypes.byref(handle)), "2^31 - 1 raw bytes")):
        assert lib.gr_exr_encoder_create(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_exr_encoder_create: ") and what in message
    assert lib.gr_exr_encode_f32(None, None, ctypes.c_void_p(16), out.ctypes.data, bound, ctypes.byref(size)) == -1
    assert lib.gr_last_error().decode().startswith("gr_exr_encode_f32: ") and "NULL" in lib.gr_last_error().decode()
    for name, argument in (("time_launches", 1), ("launch_ms", None), ("scratch_intact", None)):
        assert getattr(lib, "gr_exr_encoder_" + name)(None, argument) == -1 and lib.gr_last_error().decode().startswith("gr_exr_encoder_" + name)
    lib.gr_exr_encoder_destroy(None)


def test_exr_kernels_are_built_into_the_setup_module_behind_the_png_kernels():
    text = open(os.path.join(CSRC, "program_build.cpp")).read()
    parts = re.search(r"const char\* const PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    kernel_parts = re.search(r"const char\* const KERNEL_PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert '"png.hip", "exr.hip"' in parts and "exr.hip" not in kernel_parts       # exr.hip uses png.hip's bit-packer
    source = open(os.path.join(CSRC, "kernels", "exr.hip")).read()
    for kernel in ("gr_exr_histogram", "gr_exr_pack"):
        assert f'extern "C" __global__ void __launch_bounds__(GR_EXR_LANES) {kernel}(' in source
        assert f'"{kernel}"' in open(os.path.join(CSRC, "capi.cpp")).read()
    assert not re.search(r"\b(float|double|half|_Float16)\b\s+\w+\s*[=;,)]", re.sub(r"//.*", "", source))      # integers only: no float variable
    for host_only in ("exr_stream.cpp", "exr_stream.hpp"):
        assert "#include <hip" not in open(os.path.join(CSRC, host_only)).read()
    assert "_Float16" not in open(os.path.join(CSRC, "exr_stream.hpp")).read().replace("no compiler's _Float16", "")


def test_the_setup_module_holds_the_exr_kernels(tmp_path, monkeypatch):
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("minkowski").argument_string().encode()))
    (setup,) = list(tmp_path.glob("*.setup.hsaco"))
    blob = setup.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and b"gr_exr_histogram" in blob and b"gr_exr_pack" in blob
    for other in tmp_path.glob("*.hsaco"):
        if other != setup:
            assert b"gr_exr_pack" not in other.read_bytes()


def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    assert "---- EXR frames ----" in header
    for name in ("gr_exr_encode_bound", "gr_exr_half_bits", "gr_exr_encode_f32_host", "gr_write_frame_exr", "gr_exr_encoder_create", "gr_exr_encoder_destroy",
                 "gr_exr_encode_f32", "gr_exr_encoder_time_launches", "gr_exr_encoder_launch_ms", "gr_exr_encoder_scratch_intact"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in gra.EXPORTED_SYMBOLS and hasattr(gra.lib, name)
    assert "gr_exr_" not in open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()
    assert gra.ExrEncoder._prefix == "gr_exr_" and gra.PngEncoder._encode == "encode_rgba8"


def test_cli_refusals(capsys):
    from geodesic_raytracing_amd.render import main, render
    for argv, what in ((["--exr", "device", "--devices", "0,1", "--out", "frame.exr"], "--exr device with --devices"),
                       (["--exr", "host", "--out", "frame.png"], "--exr host with --out frame.png"),
                       (["--exr", "device", "--out", "clip.y4m"], "--exr device with --out clip.y4m"),
                       (["--exr", "device", "--out", "clip.avi"], "--exr device with --out clip.avi"),
                       (["--encode", "device", "--out", "frame.exr"], "--encode device with --out NAME.exr"),
                       (["--png", "host", "--out", "frame.exr"], "--png with --out NAME.exr"),
                       (["--png", "device", "--out", "frame.exr"], "--png with --out NAME.exr"),
                       (["--jpeg", "host", "--out", "frame.exr"], "--jpeg with --out NAME.exr"),
                       (["--quality", "80", "--out", "frame.exr"], "--quality with --out NAME.exr"),
                       (["--bit-depth", "8", "--out", "frame.exr"], "--bit-depth with --out NAME.exr")):
        with pytest.raises(SystemExit):
            main(["--metric", "minkowski"] + argv)
        assert what in capsys.readouterr().err, argv
    for arguments in (dict(exr="gpu"), dict(exr="device", rgba8=True), dict(exr="host", yuv420=True), dict(exr="host", rgba8=True, jpeg="host")):
        with pytest.raises(ValueError, match="exr"):
            render("minkowski", 8, 8, **arguments)


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    """the host encoder on heap buffers of exactly the frame's size and exactly gr_exr_encode_bound bytes, address and undefined-behaviour
    sanitizers on: the host code alone with a main of its own (tests/exr_stream_check.cpp) - nothing is loaded into this process"""
    exe = str(tmp_path / "exr_stream_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "exr_stream_check.cpp"), os.path.join(CSRC, "exr_stream.cpp"), os.path.join(CSRC, "png_stream.cpp"),
                           "-lz", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    decoded = [line for line in lines if line.endswith("decodes to the halfs")]
    assert len(decoded) == 9 * 3 * 5
    assert any(" 0 of " not in line for line in decoded) and any(" 0 of " in line for line in decoded)      # raw rows and compressed rows both occur
