"""CPU tests of the JPEG stream both JPEG encoders write (csrc/jpeg_stream.cpp; include/geodesic_hip_internal.h, "JPEG frames"): the host
encoder's files against PIL (libjpeg) as decoder and as reference encoder, a walk over the markers, the restart segments and their byte
stuffing, the quantised coefficients against a float64 model (the colour conversion restated in integers, scipy's DCT, the same quantiser),
the DCT's derived error bound, the bound on a file's size, the refusals, where the kernels' source is built, the exports.

Restated from the header: chroma is the rounded mean ((sum + 2) >> 2) of the 2 x 2 pixels' R, of their G and of their B, converted once;
a pixel past the right or bottom edge is the last of its row or column."""
import ctypes
import io
import os
import re
import struct
import subprocess
import warnings

import numpy as np
import pytest
from PIL import Image
from scipy.fft import dctn

import geodesic_raytracing_amd as gra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geodesic_raytracing_amd", "csrc")
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 16), (16, 17), (33, 18), (16, 160)]   # (width, height); 16 x 160: ten MCU rows, RST7 then RST0
QUALITIES = [1, 50, 90, 100]
DCT_BOUND = 0.19   # of an unquantised coefficient against the exact DCT: derived in the header, restated in test_the_dct_error_bound...

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# ITU-T T.81 Annex K.3: (table class << 4 | destination) -> (codes of each length 1 ... 16, symbols in code order)
_AC_TAIL = [0x10 * r + s for r in range(0x10) for s in range(1, 11)]   # every run/size the tables hold, for the sets below
ANNEX_K = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
           [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
            0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
            0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
            0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
            0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
            0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
}
assert all(sum(counts) == len(symbols) for counts, symbols in ANNEX_K.values())
assert all(set(ANNEX_K[t][1]) == set(_AC_TAIL) | {0x00, 0xf0} for t in (0x10, 0x11))


def code_lengths(table):
    counts, symbols = ANNEX_K[table]
    lengths = [length for length, n in enumerate(counts, 1) for _ in range(n)]
    return dict(zip(symbols, lengths))


def images(width, height):
    rng = np.random.default_rng(width * 1000 + height)
    y, x = np.mgrid[0:height, 0:width]
    gradient = np.stack([(x * 3) & 255, (y * 5 + x) & 255, (255 - x - y) & 255, np.full_like(x, 255)], axis=-1).astype(np.uint8)
    checkerboard = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1)
    return {"random": rng.integers(0, 256, (height, width, 4), dtype=np.uint8), "flat": np.full((height, width, 4), (10, 200, 30, 255), np.uint8),
            "gradient": gradient, "checkerboard": checkerboard}


def saturated_checkerboards():
    """32 x 16: an MCU of the 1-pixel checkerboard (the largest AC values) and an MCU whose 8 x 8 blocks are black, white, white, black (the
    largest DC differences)"""
    y, x = np.mgrid[0:16, 0:32]
    grey = np.where(x < 16, ((x + y) & 1) * 255, (((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)
    return np.repeat(grey[..., None], 4, axis=-1)


def last_coefficient_only():
    """16 x 16 grey: every 8 x 8 block is 128 + 300 x the (7, 7) basis function, so at quality 50 (step 99 there, 10 or more elsewhere, and a
    pixel's rounding moves a coefficient by less than 4) the only non-zero AC value of a luminance block is the last in zig-zag order"""
    c7 = 0.5 * np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    block = np.rint(128 + 300 * np.outer(c7, c7)).astype(np.uint8)
    return np.repeat(np.tile(block, (2, 2))[..., None], 4, axis=-1)


def segments_of(jpeg):
    """([(marker, payload)] up to and including SOS, the entropy-coded data without the EOI)"""
    assert jpeg[:2] == b"\xff\xd8" and jpeg[-2:] == b"\xff\xd9"
    at, found = 2, [(0xd8, b"")]
    while True:
        assert jpeg[at] == 0xff
        marker, (size,) = jpeg[at + 1], struct.unpack(">H", jpeg[at + 2:at + 4])
        found.append((marker, jpeg[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xda:
            return found, jpeg[at:-2]


def rows_of(data):
    """the entropy-coded data split at its RSTm markers: ([unstuffed bytes of each segment], [m of each marker]); every FF inside is followed by
    00 or is an RSTm"""
    rows, markers, current, at = [], [], bytearray(), 0
    while at < len(data):
        if data[at] != 0xff:
            current.append(data[at])
            at += 1
            continue
        follower = data[at + 1]
        assert follower == 0 or 0xd0 <= follower <= 0xd7, hex(follower)
        if follower == 0:
            current.append(0xff)
        else:
            rows.append(bytes(current))
            markers.append(follower - 0xd0)
            current = bytearray()
        at += 2
    rows.append(bytes(current))
    return rows, markers


def decode(jpeg):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(jpeg))
        image.load()
    return image


def blocks_host(pixels, quality):
    height, width = pixels.shape[:2]
    out = np.zeros((((height + 15) // 16) * ((width + 15) // 16) * 6, 64), np.int16)
    pixels = np.ascontiguousarray(pixels)
    gra.check(gra.lib.gr_jpeg_blocks_host(pixels.ctypes.data, width, height, quality, out.ctypes.data))
    return out


def model_quotients(pixels, quality):
    """per block in scan order, natural order: the float64 DCT of the integer colour conversion over the quantiser's step"""
    height, width = pixels.shape[:2]
    padded = np.pad(pixels[..., :3].astype(np.int64), ((0, -height % 16), (0, -width % 16), (0, 0)), mode="edge")
    r, g, b = padded[..., 0], padded[..., 1], padded[..., 2]
    luma = np.clip((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0, 255)
    mean = (padded[0::2, 0::2] + padded[0::2, 1::2] + padded[1::2, 0::2] + padded[1::2, 1::2] + 2) >> 2
    r, g, b = mean[..., 0], mean[..., 1], mean[..., 2]
    cb = np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255)
    cr = np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)
    steps = [t.astype(np.float64) for t in gra.jpeg_quant_tables(quality)]
    out = []
    for my in range(padded.shape[0] // 16):
        for mx in range(padded.shape[1] // 16):
            for j in range(4):
                y0, x0 = 16 * my + 8 * (j >> 1), 16 * mx + 8 * (j & 1)
                out.append(dctn(luma[y0:y0 + 8, x0:x0 + 8] - 128.0, norm="ortho") / steps[0])
            for plane in (cb, cr):
                out.append(dctn(plane[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] - 128.0, norm="ortho") / steps[1])
    return np.array(out).reshape(-1, 64), np.concatenate([steps[0].reshape(1, 64)] * 4 + [steps[1].reshape(1, 64)] * 2)


def rounded_half_away(q):
    return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(np.int64)


def symbols_of(blocks, across):
    """per MCU row, per block: (component class, DC size, [AC run << 4 | size symbols]) as the entropy coder forms them from quantised blocks
    in zig-zag order; DC predictors start from 0 in every MCU row"""
    size = lambda v: int(abs(int(v))).bit_length()
    rows = []
    for first in range(0, len(blocks), 6 * across):
        predictor, row = [0, 0, 0], []
        for b in range(first, first + 6 * across):
            component = max(b % 6 - 3, 0)
            dc = size(int(blocks[b][0]) - predictor[component])
            predictor[component] = int(blocks[b][0])
            ac, run = [], 0
            for v in blocks[b][1:]:
                if v == 0:
                    run += 1
                    continue
                ac += [0xf0] * (run // 16) + [(run % 16) << 4 | size(v)]
                run = 0
            if run:
                ac.append(0x00)
            row.append((min(component, 1), dc, ac))
        rows.append(row)
    return rows


def bits_of(row):
    dc, ac = [code_lengths(0x00), code_lengths(0x01)], [code_lengths(0x10), code_lengths(0x11)]
    return sum(dc[cls][size] + size + sum(ac[cls][s] + (s & 15) for s in symbols) for cls, size, symbols in row)


CASES = [(w, h, name, q) for w, h in SIZES for name in ("random", "flat", "gradient", "checkerboard") for q in QUALITIES]


@pytest.fixture(scope="module")
def files():
    return {(w, h, name, q): gra.jpeg_encode_host(images(w, h)[name], q) for w, h, name, q in CASES}


def test_every_file_decodes_with_pil_and_keeps_to_the_bound(files):
    for (w, h, name, q), jpeg in files.items():
        image = decode(jpeg)
        assert image.size == (w, h) and image.mode == "RGB", (w, h, name, q)
        assert len(jpeg) <= gra.jpeg_encode_bound(w, h), (w, h, name, q)
    # a flat frame comes back flat, within the quantiser's reach
    back = np.asarray(decode(files[(33, 18, "flat", 90)])).astype(int)
    assert np.abs(back - (10, 200, 30)).max() <= 3


def test_headers_in_order_with_the_tables_they_promise(files):
    for (w, h, name, q), jpeg in files.items():
        found, _ = segments_of(jpeg)
        assert [m for m, _ in found] == [0xd8, 0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
        payload = [p for _, p in found]
        assert payload[1] == b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
        luma, chroma = gra.jpeg_quant_tables(q)
        assert payload[2] == bytes([0]) + bytes(int(luma.ravel()[z]) for z in ZIGZAG)
        assert payload[3] == bytes([1]) + bytes(int(chroma.ravel()[z]) for z in ZIGZAG)
        assert payload[4] == struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
        for at, table in zip((5, 6, 7, 8), (0x00, 0x10, 0x01, 0x11)):
            counts, symbols = ANNEX_K[table]
            assert payload[at] == bytes([table] + counts + symbols), hex(table)
        assert payload[9] == struct.pack(">H", (w + 15) // 16)
        assert payload[10] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(jpeg) - len(segments_of(jpeg)[1]) - 2 == 629   # the headers' size the header file states


def test_the_quality_rule():
    k1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
    for q in (1, 10, 49, 50, 51, 90, 100):
        scale = 5000 // q if q < 50 else 200 - 2 * q
        luma, chroma = gra.jpeg_quant_tables(q)
        assert np.array_equal(luma.ravel(), np.clip((k1 * scale + 50) // 100, 1, 255))
        assert chroma[7, 7] == np.clip((99 * scale + 50) // 100, 1, 255) and chroma[0, 0] == np.clip((17 * scale + 50) // 100, 1, 255)
    assert (gra.jpeg_quant_tables(100)[0] == 1).all() and (gra.jpeg_quant_tables(50)[0].ravel() == k1).all()


def test_restart_segments_stuffing_and_bit_counts(files):
    residues = set()
    for (w, h, name, q), jpeg in files.items():
        rows, markers = rows_of(segments_of(jpeg)[1])
        mcu_rows, across = (h + 15) // 16, (w + 15) // 16
        assert len(rows) == mcu_rows and markers == [r % 8 for r in range(mcu_rows - 1)], (w, h, name, q)
        # the segments' sizes follow from the quantised blocks and the tables' code lengths: the last byte is padded with 1-bits
        for row, symbols in zip(rows, symbols_of(blocks_host(images(w, h)[name], q), across)):
            bits = bits_of(symbols)
            assert len(row) == (bits + 7) // 8, (w, h, name, q)
            if bits % 8:
                assert row[-1] & ((1 << (8 - bits % 8)) - 1) == (1 << (8 - bits % 8)) - 1
            residues.add(bits % 8)
    assert residues == set(range(8))   # (the set needs no further widths for this)
    assert b"\xff\x00" in segments_of(files[(33, 18, "random", 100)])[1]   # the stuffing path is exercised
    assert rows_of(segments_of(files[(16, 160, "random", 90)])[1])[1] == [0, 1, 2, 3, 4, 5, 6, 7, 0]


def test_the_dct_error_bound_is_derived_and_holds():
    """the header's derivation restated: K = round(2^14 c); e = the largest row sum of |K / 2^14 - c|, A = that of |c|; a row value carries
    128 e + 2^-7 (6 fraction bits), a coefficient A e1 + e (128 A + e1) + 2^-5 (4 fraction bits)"""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    c[0, :] = 1 / (2 * np.sqrt(2))
    k = np.rint(c * 16384)
    source = open(os.path.join(CSRC, "jpeg_stream.cpp")).read()
    typed = re.search(r"const int32_t DCT\[8\]\[8\] = \{(.*?)\};", source, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"-?\d+", typed)] == k.astype(int).ravel().tolist()
    e, a = np.abs(k / 16384 - c).sum(axis=1).max(), np.abs(c).sum(axis=1).max()
    e1 = 128 * e + 2.0 ** -7
    derived = a * e1 + e * (128 * a + e1) + 2.0 ** -5
    assert derived <= DCT_BOUND < 0.5
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:8, 0:8]
    blocks = [rng.integers(-128, 128, (8, 8)) for _ in range(200)] + [np.full((8, 8), -128), np.full((8, 8), 127),
              np.where((xx + yy) & 1, 127, -128), np.where((xx + yy) & 1, -128, 127), np.where(xx & 1, 127, -128), np.where(yy & 1, -128, 127)]
    worst = 0.0
    for block in blocks:
        samples, got = np.ascontiguousarray(block, np.int16), np.zeros((8, 8), np.int32)
        gra.check(gra.lib.gr_jpeg_fdct_host(samples.ctypes.data, got.ctypes.data))
        worst = max(worst, np.abs(got / 16.0 - dctn(block.astype(np.float64), norm="ortho")).max())
    print(f"largest error of an unquantised coefficient: {worst:.4f} (bound {DCT_BOUND})")
    assert worst <= DCT_BOUND
    bad = np.full(64, 128, np.int16)
    assert gra.lib.gr_jpeg_fdct_host(bad.ctypes.data, got.ctypes.data) == -1


def test_coefficients_against_the_float64_model():
    """a quantised value may differ from the model's, by 1 only, and only where the model's quotient lies within DCT_BOUND / step of a
    rounding boundary.  Of the 111 744 values compared here, 633 differ (printed), most of them where the exact quotient is a half itself."""
    compared = differing = 0
    cases = [(images(w, h)[name], q) for w, h in SIZES for name in ("random", "gradient", "checkerboard") for q in QUALITIES]
    cases += [(saturated_checkerboards(), 100), (last_coefficient_only(), 50)]
    for pixels, q in cases:
        got = blocks_host(pixels, q).astype(np.int64)
        quotient, steps = model_quotients(pixels, q)
        quotient = quotient[:, ZIGZAG]
        steps = np.tile(steps, (len(got) // 6, 1))[:, ZIGZAG]
        want = rounded_half_away(quotient)
        off = got != want
        assert (np.abs(got - want)[off] == 1).all()
        to_boundary = np.abs(np.abs(quotient) - (np.floor(np.abs(quotient)) + 0.5))
        assert (to_boundary[off] <= DCT_BOUND / steps[off] + 1e-9).all()
        compared += got.size
        differing += int(off.sum())
    print(f"{differing} of {compared} quantised values differ from the float64 model's")


def test_zrl_and_the_largest_sizes_occur():
    pixels = last_coefficient_only()
    quotient, _ = model_quotients(pixels, 50)
    model = rounded_half_away(quotient[:, ZIGZAG])
    assert (model[:4, 1:63] == 0).all() and (model[:4, 63] != 0).all() and (model[4:] == 0).all()
    assert np.array_equal(blocks_host(pixels, 50), model)
    (row,) = symbols_of(model, 1)
    assert row[0][2] == [0xf0, 0xf0, 0xf0, 0xe0 | int(abs(model[0, 63])).bit_length()]
    decode(gra.jpeg_encode_host(pixels, 50))
    pixels = saturated_checkerboards()
    quotient, _ = model_quotients(pixels, 100)
    (row,) = symbols_of(rounded_half_away(quotient[:, ZIGZAG]), 2)
    assert max(dc for _, dc, _ in row) == 11 and max(s & 15 for _, _, ac in row for s in ac) == 10
    assert np.abs(np.asarray(decode(gra.jpeg_encode_host(pixels, 100))).astype(int) - pixels[..., :3]).max() <= 2


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_against_libjpeg():
    """PIL's decode of our file against PIL's decode of PIL's own encode (libjpeg, the reference) of the same pixels with our tables and 4:2:0:
    ours may lie at most 0.5 dB below"""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:48, 0:64]
    noisy = np.clip(np.stack([2 * x + y, 255 - 3 * y, x + 3 * y, np.full_like(x, 255)], axis=-1) + rng.integers(-12, 13, (48, 64, 4)), 0, 255).astype(np.uint8)
    for label, pixels in (("33x18 random", images(33, 18)["random"]), ("64x48 gradient + noise", noisy)):
        rgb = np.ascontiguousarray(pixels[..., :3])
        for q in (50, 90):
            ours = psnr(np.asarray(decode(gra.jpeg_encode_host(pixels, q))), rgb)
            tables = [t.ravel().tolist() for t in gra.jpeg_quant_tables(q)]
            file = io.BytesIO()
            Image.fromarray(rgb).save(file, "JPEG", qtables=tables, subsampling=2)
            found, _ = segments_of(file.getvalue())
            assert [p[1:] for m, p in found if m == 0xdb] == [bytes(t[z] for z in ZIGZAG) for t in tables]   # (libjpeg did use our tables)
            theirs = psnr(np.asarray(decode(file.getvalue())), rgb)
            print(f"{label} quality {q}: ours {ours:.3f} dB, libjpeg {theirs:.3f} dB, gap {theirs - ours:+.3f} dB")
            assert ours >= theirs - 0.5


def test_refusals_name_the_entry_point():
    lib = gra.lib
    pixels = np.zeros((4, 4, 4), np.uint8)
    bound = gra.jpeg_encode_bound(4, 4)
    out = np.zeros(bound + 8, np.uint8)
    size = ctypes.c_size_t()

    def host(frame=pixels.ctypes.data, width=4, height=4, quality=90, to=out.ctypes.data, capacity=bound, got=ctypes.byref(size)):
        return lib.gr_jpeg_encode_rgba8_host(frame, width, height, quality, to, capacity, got), lib.gr_last_error().decode()

    for call, what in ((dict(frame=None), "NULL"), (dict(to=None), "NULL"), (dict(got=None), "NULL"), (dict(width=0), "size below 1"),
                       (dict(height=-3), "size below 1"), (dict(width=65536), "size above 65535"), (dict(quality=0), "quality of 0"),
                       (dict(quality=101), "quality of 101"), (dict(frame=pixels.ctypes.data + 1), "aligned to 4 bytes")):
        rc, message = host(**call)
        assert rc == -1 and message.startswith("gr_jpeg_encode_rgba8_host: ") and what in message, (call, message)
    rc, message = host(capacity=bound - 1)
    assert rc == -5 and message.startswith("gr_jpeg_encode_rgba8_host: ") and "capacity" in message and str(bound) in message
    # an output at an odd host address
    assert host(to=out.ctypes.data + 1)[0] == 0 and bytes(out[1:1 + size.value]) == gra.jpeg_encode_host(pixels, 90)
    need = ctypes.c_size_t()
    for args, what in (((4, 4, None), "NULL"), ((0, 4, ctypes.byref(need)), "size below 1"), ((4, 65536, ctypes.byref(need)), "size above 65535")):
        assert lib.gr_jpeg_encode_bound(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_jpeg_encode_bound: ") and what in message
    assert lib.gr_jpeg_encode_bound(65535, 65535, ctypes.byref(need)) == 0 and need.value > 65535 * 65535
    table = np.zeros(64, np.uint8)
    for args, what in (((90, None, table.ctypes.data), "NULL"), ((0, table.ctypes.data, table.ctypes.data), "quality of 0")):
        assert lib.gr_jpeg_quant_tables(*args) == -1 and lib.gr_last_error().decode().startswith("gr_jpeg_quant_tables: ") and what in lib.gr_last_error().decode()
    assert lib.gr_jpeg_blocks_host(None, 4, 4, 90, out.ctypes.data) == -1 and "gr_jpeg_blocks_host: " in lib.gr_last_error().decode()
    assert lib.gr_jpeg_blocks_host(pixels.ctypes.data, 4, 4, 0, out.ctypes.data) == -1 and "quality of 0" in lib.gr_last_error().decode()
    # the device encoder's, before any device call: refused where no device exists
    handle = ctypes.c_void_p()
    for args, what in (((None, 4, 4, 90, ctypes.byref(handle)), "NULL"), ((ctypes.c_void_p(8), 4, 4, 90, None), "NULL"),
                       ((ctypes.c_void_p(8), 0, 4, 90, ctypes.byref(handle)), "size below 1"),
                       ((ctypes.c_void_p(8), 4, 65536, 90, ctypes.byref(handle)), "size above 65535"),
                       ((ctypes.c_void_p(8), 4, 4, 0, ctypes.byref(handle)), "quality of 0")):
        assert lib.gr_jpeg_encoder_create(*args) == -1
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_jpeg_encoder_create: ") and what in message
    assert lib.gr_jpeg_encode_rgba8(None, None, ctypes.c_void_p(16), out.ctypes.data, bound, ctypes.byref(size)) == -1
    assert lib.gr_last_error().decode().startswith("gr_jpeg_encode_rgba8: ") and "NULL" in lib.gr_last_error().decode()
    for call in (lib.gr_jpeg_encoder_time_launches(None, 1), lib.gr_jpeg_encoder_launch_ms(None, None), lib.gr_jpeg_encoder_scratch_intact(None, None)):
        assert call == -1
    lib.gr_jpeg_encoder_destroy(None)


def test_jpeg_kernels_are_built_into_the_setup_module_only():
    text = open(os.path.join(CSRC, "program_build.cpp")).read()
    parts = re.search(r"const char\* const PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    kernel_parts = re.search(r"const char\* const KERNEL_PARTS\[\] = \{(.*?)\};", text, flags=re.S).group(1)
    assert '"jpeg.hip"' in parts and "jpeg.hip" not in kernel_parts
    source = open(os.path.join(CSRC, "kernels", "jpeg.hip")).read()
    for kernel in ("gr_jpeg_blocks", "gr_jpeg_pack", "gr_jpeg_gather"):
        assert re.search(rf'extern "C" __global__ void __launch_bounds__\(\w+\) {kernel}\(', source)
        assert f'"{kernel}"' in open(os.path.join(CSRC, "capi.cpp")).read()
    assert "asm" not in re.sub(r"//.*", "", source)
    assert "#include <hip" not in open(os.path.join(CSRC, "jpeg_stream.cpp")).read() + open(os.path.join(CSRC, "jpeg_stream.hpp")).read()


def test_the_setup_module_holds_the_jpeg_kernels(tmp_path, monkeypatch):
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("minkowski").argument_string().encode()))
    (setup,) = list(tmp_path.glob("*.setup.hsaco"))
    blob = setup.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"gfx950" in blob and all(k in blob for k in (b"gr_jpeg_blocks", b"gr_jpeg_pack", b"gr_jpeg_gather"))
    for other in tmp_path.glob("*.hsaco"):
        if other != setup:
            assert b"gr_jpeg_pack" not in other.read_bytes()


def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    assert "/* ---- JPEG frames" in header
    for name in ("gr_jpeg_encode_bound", "gr_jpeg_quant_tables", "gr_jpeg_encode_rgba8_host", "gr_jpeg_blocks_host", "gr_jpeg_fdct_host",
                 "gr_jpeg_encoder_create", "gr_jpeg_encoder_destroy", "gr_jpeg_encode_rgba8", "gr_jpeg_encoder_time_launches",
                 "gr_jpeg_encoder_launch_ms", "gr_jpeg_encoder_scratch_intact", "gr_avi_open", "gr_avi_write_frame", "gr_avi_close",
                 "gr_avi_set_size_limit"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in gra.EXPORTED_SYMBOLS and hasattr(gra.lib, name)
    public = open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()
    assert "gr_jpeg_" not in public and "gr_avi_" not in public


@pytest.fixture(scope="module")
def stream_check(tmp_path_factory):
    """tests/jpeg_stream_check.cpp with jpeg_stream.cpp and imageio.cpp and nothing else of the library: host compiler, AddressSanitizer and
    UBSan, no HIP - the host encoder and the AVI writer over the size set, every output in a buffer of exactly the bound"""
    out = str(tmp_path_factory.mktemp("jpeg_stream") / "jpeg_stream_check")
    sources = [os.path.join(ROOT, "tests", "jpeg_stream_check.cpp"), os.path.join(CSRC, "jpeg_stream.cpp"), os.path.join(CSRC, "imageio.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer"] + sources + ["-lz", "-o", out])
    return out


def test_the_stream_compiles_alone_and_runs_clean_under_sanitizers(stream_check, tmp_path):
    r = subprocess.run([stream_check, str(tmp_path / "check.avi")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.splitlines())
    for w, h in SIZES:
        pixels = images(w, h)["gradient"]   # (the check makes the same gradient)
        assert int(lines[f"{w}x{h}"]) == len(gra.jpeg_encode_host(pixels, 90)), (w, h)
    assert lines["avi"] == "closed"


def cli_error(argv, capsys):
    from geodesic_raytracing_amd.render import main
    with pytest.raises(SystemExit):
        main(argv)
    return capsys.readouterr().err


def test_cli_refusals(capsys):
    base = ["--metric", "minkowski"]
    assert "--bit-depth 10" in cli_error(base + ["--bit-depth", "10", "--out", "x.jpg"], capsys)
    assert "--bit-depth 10" in cli_error(base + ["--bit-depth", "10", "--out", "x.avi"], capsys)
    assert "--png device" in cli_error(base + ["--png", "device", "--out", "x.jpg"], capsys)
    assert "--png device" in cli_error(base + ["--png", "device", "--out", "x.avi"], capsys)
    assert "--jpeg" in cli_error(base + ["--jpeg", "device", "--out", "x.png"], capsys)
    assert "--jpeg" in cli_error(base + ["--jpeg", "host", "--out", "x.y4m"], capsys)
    assert "--jpeg" in cli_error(base + ["--quality", "80", "--out", "x.png"], capsys)
    assert "--quality 0" in cli_error(base + ["--quality", "0", "--out", "x.jpg"], capsys)
    assert "--quality 101" in cli_error(base + ["--quality", "101", "--out", "x.avi"], capsys)


def test_cli_writes_jpg_and_avi(tmp_path, monkeypatch):
    """--out x.jpg and --out x.avi parse: the arguments reach render() as jpeg / quality (stubbed here: no device), and the files it returns
    are written as they are, into one Motion-JPEG file at --fps for an .avi"""
    from geodesic_raytracing_amd import render
    seen = []

    def fake_render(*args, **kwargs):
        seen.append(kwargs)
        frame = gra.jpeg_encode_host(images(16, 16)["gradient"], kwargs["quality"])
        return [frame, frame, frame] if kwargs["cameras"] is not None else frame

    monkeypatch.setattr(render, "render", fake_render)
    jpg, avi = str(tmp_path / "x.jpg"), str(tmp_path / "x.avi")
    assert render.main(["--metric", "minkowski", "--size", "16x16", "--out", jpg]) == 0
    assert seen[-1]["jpeg"] == "host" and seen[-1]["quality"] == 90 and seen[-1]["rgba8"] is True and seen[-1]["png"] == "host"
    assert decode(open(jpg, "rb").read()).size == (16, 16)
    assert render.main(["--metric", "minkowski", "--size", "16x16", "--jpeg", "device", "--quality", "75", "--camera-to", "0,0,-5,0", "--frames", "3",
                        "--fps", "30000/1001", "--shutter", "0.5", "--supersample", "2", "--filter", "tent", "--out", avi]) == 0
    assert seen[-1]["jpeg"] == "device" and seen[-1]["quality"] == 75 and seen[-1]["rgba8"] is True and seen[-1]["shutter_samples"] == 8
    data = open(avi, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and data.count(b"00dc") == 6 and struct.unpack("<II", data[128:136]) == (1001, 30000)
