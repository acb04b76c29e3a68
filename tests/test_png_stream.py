"""CPU tests of the PNG stream both PNG encoders write (csrc/png_stream.cpp; include/geodesic_hip_internal.h, "PNG frames"): the host encoder
against zlib, a numpy restatement of the Sub / Up filters, the project's own reader and PIL; the length-limited table builder; the sizes
computed before a bit is packed; the refusals; where the kernels' source is built; the exports."""
import ctypes
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd.render import read_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def images(width, height):
    rng = np.random.default_rng(width * 1000 + height)
    gradient = np.zeros((height, width, 4), np.uint8)
    gradient[..., 0] = np.arange(width)[None, :] & 255
    gradient[..., 1] = (np.arange(width)[None, :] * 3) & 255
    gradient[..., 2] = 40
    gradient[..., 3] = 255
    return {"random": rng.integers(0, 256, (height, width, 4), dtype=np.uint8), "zero": np.zeros((height, width, 4), np.uint8),
            "colour": np.full((height, width, 4), (10, 200, 30, 255), np.uint8), "gradient": gradient}


def filtered_bytes(pixels):
    """the bytes the zlib stream holds: per row the filter type (1 = Sub with bpp 4 for row 0, 2 = Up for the others) and 4 * width differences mod 256"""
    height, width = pixels.shape[:2]
    flat = pixels.reshape(height, width * 4).astype(np.int32)
    out = np.zeros((height, width * 4 + 1), np.uint8)
    out[0, 0], out[1:, 0] = 1, 2
    left = np.zeros_like(flat[0])
    left[4:] = flat[0, :-4]
    out[0, 1:] = (flat[0] - left) & 255
    out[1:, 1:] = (flat[1:] - flat[:-1]) & 255
    return out


def chunks_of(png):
    """[(tag, data)] with every chunk's CRC checked"""
    assert png[:8] == SIGNATURE
    at, found = 8, []
    while at < len(png):
        (size,) = struct.unpack(">I", png[at:at + 4])
        tag, data = png[at + 4:at + 8], png[at + 8:at + 8 + size]
        assert struct.unpack(">I", png[at + 8 + size:at + 12 + size])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        found.append((tag, data))
        at += 12 + size
    assert at == len(png)
    return found


def build_table(histogram):
    histogram = np.ascontiguousarray(histogram, dtype=np.uint64)
    assert histogram.shape == (257,)
    lengths, codes, header, bits = np.zeros(257, np.uint8), np.zeros(257, np.uint16), np.zeros(128, np.uint32), ctypes.c_int()
    gra.check(gra.lib.gr_png_build_table(histogram.ctypes.data, lengths.ctypes.data, codes.ctypes.data, header.ctypes.data, ctypes.byref(bits)))
    return lengths, codes, header, bits.value


class Bits:
    """deflate's bit order: from bit 0 of byte 0 up"""

    def __init__(self):
        self.value, self.count = 0, 0

    def put(self, value, count):
        self.value |= int(value) << self.count
        self.count += int(count)

    def align(self):
        self.count = (self.count + 7) // 8 * 8

    def bytes(self):
        assert self.count % 8 == 0
        return self.value.to_bytes(self.count // 8, "little")


@pytest.mark.parametrize("width,height", [(1, 1), (1, 2), (3, 1), (5, 7), (64, 3), (257, 4)])
def test_host_encoder_round_trip_and_checksums(width, height, tmp_path):
    for name, pixels in images(width, height).items():
        png = gra.png_encode_host(pixels)
        chunks = chunks_of(png)
        assert [tag for tag, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], name
        assert chunks[0][1] == struct.pack(">IIBBBBB", width, height, 8, 6, 0, 0, 0)
        stream = chunks[1][1]
        assert stream[:2] == b"\x78\x01" and stream[-6:-4] == b"\x03\x00"
        assert zlib.decompress(stream) == filtered_bytes(pixels).tobytes(), name      # (zlib checks the Adler-32)
        path = tmp_path / f"{name}.png"
        path.write_bytes(png)
        assert np.array_equal(read_png(str(path)), pixels), name
        try:
            from PIL import Image
        except ImportError:
            continue
        assert np.array_equal(np.array(Image.open(io.BytesIO(png)).convert("RGBA")), pixels), name


def fibonacci_histogram():
    h = np.zeros(257, np.uint64)
    a, b = 1, 1
    for s in range(40):     # 40 Fibonacci weights: Huffman's tree is a chain 39 deep
        h[s * 5] = a
        a, b = b, a + b
    h[256] = 1
    return h


def one_literal_histogram():
    h = np.zeros(257, np.uint64)
    h[0], h[256] = 5000, 3
    return h


@pytest.mark.parametrize("histogram", [fibonacci_histogram(), one_literal_histogram(), np.full(257, 7, np.uint64)], ids=["fibonacci", "one_literal", "uniform"])
def test_table_builder(histogram):
    lengths, codes, header, header_bits = build_table(histogram)
    used = np.flatnonzero(histogram)
    assert (lengths[used] > 0).all() and (lengths[histogram == 0] == 0).all()
    assert lengths.max() <= 15
    assert sum(2 ** (15 - int(l)) for l in lengths if l) == 2 ** 15          # Kraft's sum is exactly 1
    if len(used) == 2:
        assert sorted(lengths[used]) == [1, 1]                                # the two-leaf tree
    assert len({(int(lengths[s]), int(codes[s])) for s in used}) == len(used)
    # a block packed here with the returned header and codes, then an empty stored block and the final fixed block, as the stream has them
    rng = np.random.default_rng(4)
    literals = rng.choice(used[used < 256], size=300)
    bits = Bits()
    for word in range((header_bits + 31) // 32):
        bits.put(int(header[word]), min(32, header_bits - 32 * word))
    for s in list(literals) + [256]:
        bits.put(codes[s], lengths[s])
    bits.put(0, 3)
    bits.align()
    bits.put(0xFFFF0000, 32)
    bits.put(0x0003, 16)
    assert zlib.decompressobj(-15).decompress(bits.bytes()) == bytes(int(s) for s in literals)


def test_a_deeper_tree_than_15_is_what_the_fibonacci_histogram_asks_for():
    """(the case above limits something: the unrestricted code of that histogram is deeper than 15)"""
    import heapq
    heap = [(int(v), i, 0) for i, v in enumerate(fibonacci_histogram()) if v]      # (weight, tie-break, depth of the subtree)
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), max(a[2], b[2]) + 1))
    assert heap[0][2] > 15
    lengths = build_table(fibonacci_histogram())[0]
    assert lengths.max() == 15 and lengths[195] < lengths[0]      # the heaviest literal has the shorter code


@pytest.mark.parametrize("width,height", [(1, 1), (5, 7), (64, 3), (257, 4)])
def test_exact_size(width, height):
    for name, pixels in images(width, height).items():
        filtered = filtered_bytes(pixels)
        histogram = np.zeros(257, np.uint64)
        histogram[:256] = np.bincount(filtered.ravel(), minlength=256)
        histogram[256] = height
        lengths, _codes, _header, header_bits = build_table(histogram)
        stream = 2 + 2 + 4
        for row in filtered:
            block = header_bits + int(lengths[row].astype(np.int64).sum()) + int(lengths[256])
            stream += (block + 3 + 7) // 8 + 4
        want = 8 + 25 + 12 + stream + 12
        png = gra.png_encode_host(pixels)
        assert len(png) == want, name
        assert len(png) <= gra.png_encode_bound(width, height)


def test_refusals_name_the_entry_point():
    lib = gra.lib
    pixels = np.zeros((4, 4, 4), np.uint8)
    bound = gra.png_encode_bound(4, 4)
    out = np.zeros(bound + 8, np.uint8)
    size = ctypes.c_size_t()

    def host(frame=pixels.ctypes.data, width=4, height=4, to=out.ctypes.data, capacity=bound, got=ctypes.byref(size)):
        return lib.gr_png_encode_rgba8_host(frame, width, height, to, capacity, got), lib.gr_last_error().decode()

    for call, what in ((dict(frame=None), "NULL"), (dict(to=None), "NULL"), (dict(got=None), "NULL"), (dict(width=0), "size below 1"),
                       (dict(height=-3), "size below 1"), (dict(frame=pixels.ctypes.data + 1), "aligned to 4 bytes"),
                       (dict(width=32768, height=16384), "2^31 - 1 raw bytes")):
        rc, message = host(**call)
        assert rc == -1 and message.startswith("gr_png_encode_rgba8_host: ") and what in message, (call, message)
    rc, message = host(capacity=bound - 1)
    assert rc == -5 and message.startswith("gr_png_encode_rgba8_host: ") and "capacity" in message and str(bound) in message
    assert host(to=out.ctypes.data + 1)[0] == 0          # the output needs no alignment
    # the bound's own
    need = ctypes.c_size_t()
    for args, what in (((4, 4, None), "NULL"), ((0, 4, ctypes.byref(need)), "size below 1"), ((32768, 16384, ctypes.byref(need)), "2^31 - 1 raw bytes")):
        assert lib.gr_png_encode_bound(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_png_encode_bound: ") and what in message
    assert lib.gr_png_encode_bound(23170, 23170, ctypes.byref(need)) == 0 and need.value > 4 * 23170 * 23170
    # the device encoder's, before any device call: a NULL program and a bad size are refused where no device exists, and so is a NULL encoder
    handle = ctypes.c_void_p()
    for args, what in (((None, 4, 4, ctypes.byref(handle)), "NULL"), ((ctypes.c_void_p(8), 4, 4, None), "NULL"),
                       ((ctypes.c_void_p(8), 0, 4, ctypes.byref(handle)), "size below 1"),
                       ((ctypes.c_void_p(8), 32768, 16384, ctypes.byref(handle)), "2^31 - 1 raw bytes")):
        assert lib.gr_png_encoder_create(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_png_encoder_create: ") and what in message
    assert lib.gr_png_encode_rgba8(None, None, ctypes.c_void_p(16), out.ctypes.data, bound, ctypes.byref(size)) == -1
    assert lib.gr_last_error().decode().startswith("gr_png_encode_rgba8: ") and "NULL" in lib.gr_last_error().decode()
    lib.gr_png_encoder_destroy(None)


def test_png_kernels_are_built_into_the_setup_module_only():
    text = open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "program_build.cpp")).read()
    parts = re.search(r"const char\* const PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    kernel_parts = re.search(r"const char\* const KERNEL_PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert '"png.hip"' in parts and "png.hip" not in kernel_parts
    source = open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "kernels", "png.hip")).read()
    for kernel in ("gr_png_histogram", "gr_png_pack"):
        assert f'extern "C" __global__ void __launch_bounds__(GR_PNG_LANES) {kernel}(' in source
        assert f'"{kernel}"' in open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "capi.cpp")).read()
    assert "#include <hip" not in open(os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "png_stream.cpp")).read()


def test_the_setup_module_holds_the_png_kernels(tmp_path, monkeypatch):
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("minkowski").argument_string().encode()))
    (setup,) = list(tmp_path.glob("*.setup.hsaco"))
    blob = setup.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and b"gr_png_histogram" in blob and b"gr_png_pack" in blob
    for other in tmp_path.glob("*.hsaco"):
        if other != setup:
            assert b"gr_png_pack" not in other.read_bytes()


def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    for name in ("gr_png_encoder_create", "gr_png_encoder_destroy", "gr_png_encode_bound", "gr_png_encode_rgba8", "gr_png_encode_rgba8_host",
                 "gr_png_build_table"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in gra.EXPORTED_SYMBOLS and hasattr(gra.lib, name)
    assert "gr_png_" not in open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()


def test_cli_refuses_png_device_with_video(capsys):
    from geodesic_raytracing_amd.render import main
    with pytest.raises(SystemExit):
        main(["--metric", "minkowski", "--png", "device", "--out", "clip.y4m"])
    assert "--png device" in capsys.readouterr().err
