"""CPU tests of 10-bit video frames (include/geodesic_hip_internal.h, "10-bit video frames"): the seven names, the thresholds of the 10-bit
sRGB code against the library's own encode, gr_rgb10_to_yuv420p10 against a numpy restatement of its integer formulas in both layouts,
the properties the definition promises (grey neutrality, ranges, distance from the real-valued BT.709 formula), the C420p10 file, every
refusal on the host side - the launcher's and the frame entry's come before any device call - and the CLI's."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import (Y4MWriter, frame_to_rgb10, rgb10_to_yuv420p10, rgba8_to_yuv420, srgb10_thresholds, yuv420_bytes,
                                              yuv420p10_bytes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_srgb10_thresholds", "gr_frame_to_rgb10", "gr_rgb10_to_yuv420p10", "gr_yuv420p10_bytes", "gr_y4m_open_depth", "gr_present_yuv420p10",
         "gr_render_frame_yuv420p10"]
CONTRACT_SHA256 = "8d085403df7f900e515ee2740ba562a30fdaee115bae2c6b4c608a80dad10245"   # include/geodesic_hip.h of the parent commit
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 7), (8, 2), (65, 9)]   # width, height
GUARD, GUARD_BYTE = 64, 0xA5
ONE = 0x3f800000


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def code10(values):
    """the library's 10-bit code of float32 values of any shape, taken from gr_frame_to_rgb10 (values ride in the R channel)"""
    values = np.asarray(values, dtype=np.float32)
    frame = np.zeros((1, max(values.size, 1), 4), dtype=np.float32)
    frame[0, :values.size, 0] = values.reshape(-1)
    return frame_to_rgb10(frame)[0, :values.size, 0].astype(np.int64).reshape(values.shape)


def test_the_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in NAMES:
        assert name in internal and name not in contract, name
        assert hasattr(gra.lib, name) and name in gra.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    assert "10-bit video frames" in header and header.index("10-bit video frames") < header.index("gr_srgb10_thresholds")
    assert yuv420p10_bytes(1920, 1080) == 1920 * 1080 * 3 and yuv420p10_bytes(3, 3) == 2 * (9 + 8)
    assert yuv420p10_bytes(0, 4) == 0 and yuv420p10_bytes(4, -1) == 0
    for w, h in SIZES:
        assert yuv420p10_bytes(w, h) == 2 * yuv420_bytes(w, h)


def test_the_contract_header_is_the_parent_commits():
    blob = open(os.path.join(ROOT, "include", "geodesic_hip.h"), "rb").read()
    assert hashlib.sha256(blob).hexdigest() == CONTRACT_SHA256


def test_the_encode_of_single_values():
    """clamped at both ends, -0 and negatives 0, +inf the code of 1; the chain restated in float32 with numpy's pow agrees to one code
    (the definition is the library's own powf, which the thresholds invert exactly - next test)"""
    top = int(code10(np.float32(1.0)))
    assert top in (1022, 1023)
    special = np.array([0.0, -0.0, -1.0, -np.inf, 1.0, 1.5, np.inf, 0.0031308, 0.5], dtype=np.float32)
    got = code10(special)
    assert list(got[:4]) == [0, 0, 0, 0] and list(got[4:7]) == [top, top, top]
    v = np.random.RandomState(3).uniform(0, 1, size=20000).astype(np.float32)
    s = np.where(v <= np.float32(0.0031308), v * np.float32(12.92), np.float32(1.055) * np.power(v, np.float32(1.0 / 2.4)) - np.float32(0.055))
    want = (np.clip(s.astype(np.float32), 0, 1) * np.float32(1023.0)).astype(np.int64)
    assert np.abs(code10(v) - want).max() <= 1


def test_the_thresholds_invert_the_encode():
    t = srgb10_thresholds()
    assert t.shape == (1024,) and t.dtype == np.float32 and t[0] == 0
    top = int(code10(np.float32(1.0)))
    finite = t[:top + 1]
    assert np.isfinite(finite).all() and (finite <= 1).all() and np.isposinf(t[top + 1:]).all()
    assert (t[1:] >= t[:-1]).all()   # non-decreasing
    k = np.arange(1, top + 1)
    assert (code10(t[1:top + 1]) >= k).all()
    assert (code10(np.nextafter(t[1:top + 1], np.float32(0))) < k).all()
    # 2^20 random bit patterns of [0, 1]: the count of T[k] <= c is the library's code
    bits = np.random.RandomState(20).randint(0, ONE + 1, size=1 << 20).astype(np.uint32)
    bits[:4] = [0, 1, ONE - 1, ONE]
    c = bits.view(np.float32)
    counted = np.searchsorted(t[1:], c, side="right")   # (+inf entries are never <= c)
    assert (counted == code10(c)).all()


def planes_by_formula(codes):
    """the definition's integer formulas in numpy (int32, arithmetic shifts): (Y [h, w], Cb [ch, cw], Cr [ch, cw]) of uint16 [h, w, 3]"""
    h, w = codes.shape[:2]
    v = codes.astype(np.int32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    y = 64 + ((11931 * r + 40136 * g + 4052 * b + 32768) >> 16)
    rows = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1)   # the missing row / column is the edge pixel itself
    cols = np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    padded = v[rows][:, cols]
    s = padded.reshape(len(rows) // 2, 2, len(cols) // 2, 2, 3).sum(axis=(1, 3), dtype=np.int32)
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    cb = 512 + ((-6576 * sr - 22124 * sg + 28700 * sb + 131072) >> 18)
    cr = 512 + ((28700 * sr - 26068 * sg - 2632 * sb + 131072) >> 18)
    for plane in (y, cb, cr):
        assert plane.dtype == np.int32 and plane.min() >= 0 and plane.max() <= 1023
    return y.astype(np.uint16), cb.astype(np.uint16), cr.astype(np.uint16)


def packed(planes, layout):
    y, cb, cr = planes
    if layout == I420:
        return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    return np.concatenate([y.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)]) << 6


def library_encode(codes, layout):
    """gr_rgb10_to_yuv420p10 into a buffer between guard bytes, which must survive; uint16 words"""
    h, w = codes.shape[:2]
    n = yuv420p10_bytes(w, h)
    assert n == 2 * (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2))
    buf = np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    assert gra.lib.gr_rgb10_to_yuv420p10(codes.ctypes.data_as(ctypes.c_void_p), w, h, layout, ctypes.c_void_p(buf.ctypes.data + GUARD)) == 0
    assert (buf[:GUARD] == GUARD_BYTE).all() and (buf[GUARD + n:] == GUARD_BYTE).all(), "guard bytes were written"
    return buf[GUARD:GUARD + n].copy().view("<u2")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", [I420, NV12])
def test_the_definition_is_the_integer_formulas(w, h, layout):
    rs = np.random.RandomState(1000 * w + h)
    for _ in range(3):
        codes = rs.randint(0, 1024, size=(h, w, 3)).astype(np.uint16)
        want = packed(planes_by_formula(codes), layout)
        got = library_encode(codes, layout)
        assert got.tobytes() == want.astype("<u2").tobytes()
        assert rgb10_to_yuv420p10(codes, layout).tobytes() == got.tobytes()
        if layout == NV12:
            assert (got & 63 == 0).all()      # P010: the code sits in the high ten bits
        else:
            assert (got <= 1023).all()        # yuv420p10le: in the low ten


@pytest.mark.parametrize("w,h", SIZES)
def test_p010_is_yuv420p10le_rearranged_and_shifted(w, h):
    codes = np.random.RandomState(w + 100 * h).randint(0, 1024, size=(h, w, 3)).astype(np.uint16)
    planar, p010 = library_encode(codes, I420), library_encode(codes, NV12)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert len(planar) == len(p010) == w * h + 2 * cw * ch
    assert (p010[:w * h] == planar[:w * h] << 6).all()
    pairs = p010[w * h:].reshape(ch, cw, 2)
    assert (pairs[..., 0].reshape(-1) == planar[w * h:w * h + cw * ch] << 6).all() and (pairs[..., 1].reshape(-1) == planar[w * h + cw * ch:] << 6).all()


def uniform_blocks(colours):
    """colours [n, 3] as n 2 x 2 blocks of one colour each, side by side: (Y, Cb, Cr) per colour through the library"""
    n = len(colours)
    codes = np.zeros((2, 2 * n, 3), dtype=np.uint16)
    codes[:, :, :] = np.repeat(colours, 2, axis=0)[None]
    out = library_encode(codes, I420)
    y = out[:4 * n].reshape(2, 2 * n)
    assert (y == y[0, ::2].repeat(2)[None]).all()   # the four pixels of a block have one luma
    return y[0, ::2].astype(np.int32), out[4 * n:5 * n].astype(np.int32), out[5 * n:].astype(np.int32)


def bt709(rgb_over_1023):
    """the real-valued BT.709 limited-range 10-bit Y'CbCr of R'G'B' in [0, 1], float64"""
    r, g, b = rgb_over_1023[..., 0], rgb_over_1023[..., 1], rgb_over_1023[..., 2]
    ey = 0.2126 * r + 0.7152 * g + 0.0722 * b
    return 64 + 876 * ey, 512 + 896 * (b - ey) / 1.8556, 512 + 896 * (r - ey) / 1.5748


CORNERS = np.array([[r, g, b] for r in (0, 1023) for g in (0, 1023) for b in (0, 1023)], dtype=np.uint16)


def test_greys_are_neutral_and_white_and_black_are_where_video_puts_them():
    v = np.arange(1024)
    y, cb, cr = uniform_blocks(np.stack([v, v, v], axis=1).astype(np.uint16))
    assert (cb == 512).all() and (cr == 512).all()
    assert np.abs(y - (64 + 876 * v / 1023)).max() <= 0.51
    assert (y[1023], cb[1023], cr[1023]) == (940, 512, 512) and (y[0], cb[0], cr[0]) == (64, 512, 512)
    assert 11931 + 40136 + 4052 == 56119 == round(876 / 1023 * 65536) and -6576 - 22124 + 28700 == 0 and 28700 - 26068 - 2632 == 0


def test_ranges_and_the_distance_from_the_real_valued_formula():
    """the cube's corners and 10^6 random colours as uniform 2 x 2 blocks, then 10^6 random blocks of four different colours (2 * 10^6
    triples in all): Y in [64, 940], Cb and Cr in [64, 960], each within 0.51 of a code of float64 BT.709 (0.5 is the rounding, the rest
    the 16-bit coefficients)"""
    rs = np.random.RandomState(7)
    n = 1000000
    colours = np.concatenate([CORNERS, rs.randint(0, 1024, size=(n, 3)).astype(np.uint16)])
    got = uniform_blocks(colours)
    want = bt709(colours.astype(np.float64) / 1023)
    worst = np.array([np.abs(got[k] - want[k]).max() for k in range(3)])
    assert (got[0].min(), got[0].max()) == (64, 940)
    assert (got[1].min(), got[1].max()) == (64, 960) and (got[2].min(), got[2].max()) == (64, 960)   # the corners reach every end
    codes = rs.randint(0, 1024, size=(2, 2 * n, 3)).astype(np.uint16)
    out = library_encode(codes, I420).astype(np.int32)
    y, cb, cr = out[:4 * n].reshape(2, 2 * n), out[4 * n:5 * n], out[5 * n:]
    real = codes.astype(np.float64) / 1023
    worst[0] = max(worst[0], np.abs(y - bt709(real)[0]).max())
    mean = real.reshape(2, n, 2, 3).mean(axis=(0, 2))   # the chroma of a block is that of the mean of its four encoded pixels
    _, want_cb, want_cr = bt709(mean)
    worst[1], worst[2] = max(worst[1], np.abs(cb - want_cb).max()), max(worst[2], np.abs(cr - want_cr).max())
    assert y.min() >= 64 and y.max() <= 940 and min(cb.min(), cr.min()) >= 64 and max(cb.max(), cr.max()) <= 960
    print("largest distance from float64 BT.709 (Y, Cb, Cr):", worst)
    assert (worst <= 0.51).all(), worst


@pytest.mark.parametrize("w,h", [(3, 3), (5, 7), (65, 9), (1, 1), (2, 5), (7, 4)])
def test_an_odd_edge_is_the_edge_pixel_counted_twice(w, h):
    codes = np.random.RandomState(w * 31 + h).randint(0, 1024, size=(h, w, 3)).astype(np.uint16)
    rows, cols = np.minimum(np.arange(h + h % 2), h - 1), np.minimum(np.arange(w + w % 2), w - 1)
    even = codes[rows][:, cols]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    odd_out, even_out = library_encode(codes, I420), library_encode(even, I420)
    assert odd_out[w * h:].tobytes() == even_out[4 * cw * ch:].tobytes()                              # both chroma planes
    assert odd_out[:w * h].reshape(h, w).tobytes() == even_out[:4 * cw * ch].reshape(2 * ch, 2 * cw)[:h, :w].tobytes()


def test_a_frame_becomes_codes_of_its_three_colour_channels():
    rs = np.random.RandomState(4)
    frame = rs.uniform(-0.1, 1.2, size=(5, 7, 4)).astype(np.float32)
    codes = frame_to_rgb10(frame)
    assert codes.shape == (5, 7, 3) and codes.dtype == np.uint16 and codes.max() <= 1023
    for c in range(3):
        assert (codes[..., c] == code10(frame[..., c])).all()
    other = frame.copy()
    other[..., 3] = rs.uniform(size=(5, 7))   # alpha is not encoded
    assert frame_to_rgb10(other).tobytes() == codes.tobytes()
    buf = np.full(5 * 7 * 3 * 2 + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
    assert gra.lib.gr_frame_to_rgb10(frame.ctypes.data_as(ctypes.c_void_p), 7, 5, ctypes.c_void_p(buf.ctypes.data + GUARD)) == 0
    assert (buf[:GUARD] == GUARD_BYTE).all() and (buf[-GUARD:] == GUARD_BYTE).all()
    assert buf[GUARD:-GUARD].tobytes() == codes.tobytes()


def test_a_10_bit_y4m_file_of_three_frames(tmp_path):
    w, h, fps = 7, 5, (30000, 1001)
    rs = np.random.RandomState(w)
    frames = [rgb10_to_yuv420p10(rs.randint(0, 1024, size=(h, w, 3)).astype(np.uint16)) for _ in range(3)]
    path = tmp_path / "three.y4m"
    with Y4MWriter(str(path), w, h, fps, bit_depth=10) as stream:
        for frame in frames:
            stream.write(frame)
        with pytest.raises(ValueError):
            stream.write(frame[:-1])
    header = b"YUV4MPEG2 W7 H5 F30000:1001 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n"
    blob = path.read_bytes()
    n = yuv420p10_bytes(w, h)
    assert n == 2 * (35 + 2 * 12)
    assert blob.startswith(header) and len(blob) == len(header) + 3 * (6 + n)
    for k, frame in enumerate(frames):
        at = len(header) + k * (6 + n)
        assert blob[at:at + 6] == b"FRAME\n"
        body = blob[at + 6:at + 6 + n]
        # little-endian: the low byte of every sample first
        assert [body[2 * i] | (body[2 * i + 1] << 8) for i in range(n // 2)] == [int(v) for v in frame]


def test_open_depth_8_writes_the_file_gr_y4m_open_writes(tmp_path):
    w, h = 6, 4
    frame = rgba8_to_yuv420(np.random.RandomState(1).randint(0, 256, size=(h, w, 4)).astype(np.uint8))
    paths = [str(tmp_path / "a.y4m").encode(), str(tmp_path / "b.y4m").encode()]
    for path, depth in zip(paths, (None, 8)):
        handle = ctypes.c_void_p()
        if depth is None:
            assert gra.lib.gr_y4m_open(path, w, h, 25, 1, ctypes.byref(handle)) == 0
        else:
            assert gra.lib.gr_y4m_open_depth(path, w, h, 25, 1, depth, ctypes.byref(handle)) == 0
        for _ in range(2):
            assert gra.lib.gr_y4m_write_frame(handle, frame.ctypes.data_as(ctypes.c_void_p)) == 0
        assert gra.lib.gr_y4m_close(handle) == 0
    a, b = open(paths[0], "rb").read(), open(paths[1], "rb").read()
    assert a == b and a.startswith(b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n") and len(a) == 59 + 2 * (6 + 36)


def last_error_names(name):
    return name.encode() in gra.lib.gr_last_error()


def test_the_host_functions_refuse_bad_arguments(tmp_path):
    codes, out = np.zeros((2, 2, 3), dtype=np.uint16), np.full(6, 0xA5A5, dtype=np.uint16)
    src, dst = codes.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    over = codes.copy()
    over[1, 1, 2] = 1024
    for args in ((None, 2, 2, I420, dst), (src, 2, 2, I420, None), (src, 0, 2, I420, dst), (src, 2, -1, I420, dst), (src, 2, 2, 2, dst),
                 (src, 2, 2, -1, dst), (over.ctypes.data_as(ctypes.c_void_p), 2, 2, NV12, dst)):
        assert gra.lib.gr_rgb10_to_yuv420p10(*args) == -1, args
        assert last_error_names("gr_rgb10_to_yuv420p10")
        assert (out == 0xA5A5).all()   # refused before any write
    frame, rgb = np.zeros((2, 2, 4), dtype=np.float32), np.full(12, 0xA5A5, dtype=np.uint16)
    fsrc, fdst = frame.ctypes.data_as(ctypes.c_void_p), rgb.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 2, 2, fdst), (fsrc, 2, 2, None), (fsrc, 0, 2, fdst), (fsrc, 2, -3, fdst)):
        assert gra.lib.gr_frame_to_rgb10(*args) == -1, args
        assert last_error_names("gr_frame_to_rgb10") and (rgb == 0xA5A5).all()
    assert gra.lib.gr_srgb10_thresholds(None) == -1 and last_error_names("gr_srgb10_thresholds")
    with pytest.raises(ValueError):
        rgb10_to_yuv420p10(np.zeros((4, 4, 4), dtype=np.uint16))
    with pytest.raises(ValueError):
        frame_to_rgb10(np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(gra.GeodesicError):
        rgb10_to_yuv420p10(np.full((2, 2, 3), 1024, dtype=np.uint16))
    # the writer
    good = str(tmp_path / "x.y4m").encode()
    missing = str(tmp_path / "no_such_directory" / "x.y4m").encode()
    for args in ((None, 16, 8, 24, 1, 10), (good, 0, 8, 24, 1, 10), (good, 16, -2, 24, 1, 10), (good, 16, 8, 0, 1, 10), (good, 16, 8, 24, 0, 8),
                 (good, 16, 8, 24, 1, 9), (good, 16, 8, 24, 1, 12), (good, 16, 8, 24, 1, 0), (missing, 16, 8, 24, 1, 10)):
        handle = ctypes.c_void_p(1)
        assert gra.lib.gr_y4m_open_depth(*args, ctypes.byref(handle)) == -1 and not handle.value, args
        assert last_error_names("gr_y4m_open_depth")
    assert gra.lib.gr_y4m_open_depth(good, 16, 8, 24, 1, 10, None) == -1 and last_error_names("gr_y4m_open_depth")
    assert not os.path.exists(good)   # every refusal came before the file was created
    with pytest.raises(gra.GeodesicError):
        Y4MWriter(good.decode(), 16, 8, bit_depth=12)
    assert not os.path.exists(good)
    if os.path.exists("/dev/full"):   # the short-write rule: the header fails, no handle stays
        handle = ctypes.c_void_p(1)
        assert gra.lib.gr_y4m_open_depth(b"/dev/full", 16, 8, 24, 1, 10, ctypes.byref(handle)) == -1 and not handle.value
        assert b"short write" in gra.lib.gr_last_error()


def test_the_launcher_and_the_frame_entry_check_their_arguments_before_any_device_call():
    """(this box has no GPU, and no answer is GR_ERROR_DEVICE: the checks precede every HIP call)"""
    invalid = -1   # GR_ERROR_INVALID_ARGUMENT
    src = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    by2, by4, odd = ctypes.c_void_p(4098), ctypes.c_void_p(4100), ctypes.c_void_p(4097)
    for program in (None, src):
        for args in ((None, src, 8, 8, 2, I420), (src, None, 8, 8, 2, I420), (src, src, 8, 8, 0, I420), (src, src, 8, 8, 5, I420),
                     (src, src, 0, 8, 2, I420), (src, src, 8, -1, 2, I420), (src, src, 30000, 20000, 2, I420), (src, src, 2, 600000, 1, NV12),
                     (src, src, 8, 8, 2, 2), (src, src, 8, 8, 2, -1),
                     (src, by2, 8, 8, 2, NV12), (src, by4, 8, 8, 1, I420), (src, odd, 8, 8, 1, I420),      # 8-byte stores: aligned to 8
                     (src, odd, 7, 8, 1, I420), (src, odd, 10, 3, 2, NV12)):                                # stores of a word: aligned to 2
            assert gra.lib.gr_present_yuv420p10(program, None, *args) == invalid, args
            assert last_error_names("gr_present_yuv420p10")
    assert gra.lib.gr_present_yuv420p10(None, None, src, src, 8, 8, 2, I420) == invalid   # nothing wrong but the program
    assert last_error_names("gr_present_yuv420p10")
    assert gra.lib.gr_present_yuv420p10(None, None, src, by2, 7, 8, 2, I420) == invalid and b"null program" in gra.lib.gr_last_error()
    cam, feats, opts = gra.default_camera(), gra.default_features(), gra.frame_options()
    strips = gra.frame_options(mode=gra.MODE_FUSED, strip_count=2, strip_rank=0, block_rows=8)

    def entry(state, program, metric, camera, out, layout, options):
        return gra.lib.gr_render_frame_yuv420p10(state, program, metric, None, camera, ctypes.byref(feats), None, 0, src, src, 64, 32, 1, out, layout,
                                                 ctypes.byref(options))

    for args in ((None, src, src, ctypes.byref(cam), src, I420, opts), (src, None, src, ctypes.byref(cam), src, I420, opts),
                 (src, src, None, ctypes.byref(cam), src, NV12, opts), (src, src, src, None, src, I420, opts),
                 (src, src, src, ctypes.byref(cam), None, I420, opts), (src, src, src, ctypes.byref(cam), src, 2, opts),
                 (src, src, src, ctypes.byref(cam), src, -1, opts), (src, src, src, ctypes.byref(cam), odd, I420, opts),
                 (src, src, src, ctypes.byref(cam), src, I420, strips), (src, src, src, ctypes.byref(cam), src, NV12, strips)):
        assert entry(*args) == invalid, args
        assert last_error_names("gr_render_frame_yuv420p10")
    assert entry(src, src, src, ctypes.byref(cam), src, I420, strips) == invalid and b"gr_render_frame_tiled_as" in gra.lib.gr_last_error()


def test_the_kernel_and_its_table_are_part_of_the_setup_module():
    here = os.path.join(os.path.dirname(gra.__file__), "csrc")
    capi = open(os.path.join(here, "capi.cpp")).read()
    present = open(os.path.join(here, "kernels", "present.hip")).read()
    assert "gr_present_yuv420p10(" in present and "GR_SRGB10_TREE_BITS" in present and "__shared__ float tree[1024]" in present
    assert re.search(r"is_setup_kernel\(int k\) \{[^}]*K_PRESENT_YUV420P10", capi)
    assert "srgb8_tree_source() + srgb10_tree_source() + source" in capi
    for other in ("trace.hip", "integrator.hip", "shading.hip"):
        assert "yuv420p10" not in open(os.path.join(here, "kernels", other)).read()


def test_the_cli_refuses_ten_bits_for_a_png(capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for argv in (["--bit-depth", "10", "--out", "x.png"], ["--bit-depth", "10", "--encode", "device", "--out", "x.png"],
                 ["--bit-depth", "12", "--out", "x.y4m"]):
        with pytest.raises(SystemExit) as e:
            render.main(["--metric", "kerr_boyer"] + argv)
        assert e.value.code == 2 and "--bit-depth" in capsys.readouterr().err, argv
    assert not os.path.exists("x.png") and not os.path.exists("x.y4m") and os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="bit_depth"):
        render.render("kerr_boyer", 8, 8, bit_depth=10)   # 10 bits are a depth of video frames (refused before anything is loaded)
