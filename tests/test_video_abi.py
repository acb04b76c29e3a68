"""CPU tests of video frames (gr_rgba8_to_yuv420, gr_yuv420_bytes, the gr_y4m_* writer, gr_present_yuv420's and gr_render_frame_yuv420's
argument checks): the host definition of the 8-bit BT.709 Y'CbCr 4:2:0 encode against a numpy restatement of its integer formulas, the
properties the definition promises (grey neutrality, ranges, distance from the real-valued BT.709 formula), edge replication, the two
layouts, the YUV4MPEG2 file read back by a parser written here, which code the kernel is part of, the CLI's argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import Y4MWriter, rgba8_to_yuv420, yuv420_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["gr_render_frame_yuv420", "gr_rgba8_to_yuv420", "gr_y4m_open", "gr_y4m_write_frame", "gr_y4m_close"]
INTERNAL = ["gr_present_yuv420", "gr_yuv420_bytes"]   # (gr_yuv420_bytes: the contract header states the formula and keeps to its 80 names)
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 7), (8, 2), (65, 9)]   # width, height
GUARD, GUARD_BYTE = 64, 0xA5


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def planes_by_formula(rgba):
    """the issue's integer formulas in numpy (int32, arithmetic shifts): (Y [h, w], Cb [ch, cw], Cr [ch, cw]) of uint8 [h, w, 4]"""
    h, w = rgba.shape[:2]
    v = rgba.astype(np.int32)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    y = 16 + ((11966 * r + 40254 * g + 4064 * b + 32768) >> 16)
    rows = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1)   # the missing row / column is the edge pixel itself
    cols = np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    padded = v[rows][:, cols]
    s = padded.reshape(len(rows) // 2, 2, len(cols) // 2, 2, 4).sum(axis=(1, 3), dtype=np.int32)
    sr, sg, sb = s[..., 0], s[..., 1], s[..., 2]
    cb = 128 + ((-6596 * sr - 22188 * sg + 28784 * sb + 131072) >> 18)
    cr = 128 + ((28784 * sr - 26145 * sg - 2639 * sb + 131072) >> 18)
    for plane in (y, cb, cr):
        assert plane.dtype == np.int32 and plane.min() >= 0 and plane.max() <= 255
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def packed(planes, layout):
    y, cb, cr = planes
    if layout == I420:
        return np.concatenate([y.reshape(-1), cb.reshape(-1), cr.reshape(-1)])
    return np.concatenate([y.reshape(-1), np.stack([cb, cr], axis=-1).reshape(-1)])


def library_encode(rgba, layout):
    """gr_rgba8_to_yuv420 into a buffer between guard bytes, which must survive"""
    h, w = rgba.shape[:2]
    n = yuv420_bytes(w, h)
    assert n == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    buf = np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
    rgba = np.ascontiguousarray(rgba)
    assert gra.lib.gr_rgba8_to_yuv420(rgba.ctypes.data_as(ctypes.c_void_p), w, h, layout, ctypes.c_void_p(buf.ctypes.data + GUARD)) == 0
    assert (buf[:GUARD] == GUARD_BYTE).all() and (buf[GUARD + n:] == GUARD_BYTE).all(), "guard bytes were written"
    return buf[GUARD:GUARD + n].copy()


def test_the_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in PUBLIC:
        assert name in contract and name not in internal, name
    for name in INTERNAL:
        assert name in internal and name not in contract, name
    for name in PUBLIC + INTERNAL:
        assert hasattr(gra.lib, name), name
        assert name in gra.EXPORTED_SYMBOLS, name
    assert yuv420_bytes(1920, 1080) == 1920 * 1080 * 3 // 2 and yuv420_bytes(3, 3) == 9 + 8 and yuv420_bytes(0, 4) == 0 and yuv420_bytes(4, -1) == 0


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("layout", [I420, NV12])
def test_the_definition_is_the_integer_formulas(w, h, layout):
    rs = np.random.RandomState(1000 * w + h)
    for _ in range(3):
        rgba = rs.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
        want = packed(planes_by_formula(rgba), layout)
        assert library_encode(rgba, layout).tobytes() == want.tobytes()
        assert rgba8_to_yuv420(rgba, layout).tobytes() == want.tobytes()
        other = rgba.copy()
        other[..., 3] = rs.randint(0, 256, size=(h, w))   # alpha is dropped
        assert library_encode(other, layout).tobytes() == want.tobytes()


def uniform_blocks(colours):
    """colours [n, 3] as n 2 x 2 blocks of one colour each, side by side: (Y, Cb, Cr) per colour through the library"""
    n = len(colours)
    rgba = np.zeros((2, 2 * n, 4), dtype=np.uint8)
    rgba[:, :, :3] = np.repeat(colours, 2, axis=0)[None]
    out = library_encode(rgba, I420)
    y = out[:4 * n].reshape(2, 2 * n)
    assert (y == y[0, ::2].repeat(2)[None]).all()   # the four pixels of a block have one luma
    return y[0, ::2].astype(np.int32), out[4 * n:5 * n].astype(np.int32), out[5 * n:].astype(np.int32)


def bt709(rgb_over_255):
    """the real-valued BT.709 limited-range Y'CbCr of R'G'B' in [0, 1], float64"""
    r, g, b = rgb_over_255[..., 0], rgb_over_255[..., 1], rgb_over_255[..., 2]
    ey = 0.2126 * r + 0.7152 * g + 0.0722 * b
    return 16 + 219 * ey, 128 + 224 * (b - ey) / 1.8556, 128 + 224 * (r - ey) / 1.5748


def test_greys_are_neutral_and_white_and_black_are_where_video_puts_them():
    v = np.arange(256)
    y, cb, cr = uniform_blocks(np.stack([v, v, v], axis=1).astype(np.uint8))
    assert (cb == 128).all() and (cr == 128).all()
    assert (y == np.floor(219 * v / 255 + 0.5).astype(np.int32)+ 16).all()
    assert (y[255], cb[255], cr[255]) == (235, 128, 128) and (y[0], cb[0], cr[0]) == (16, 128, 128)


def test_ranges_and_the_distance_from_the_real_valued_formula():
    """all 2^24 colours as uniform 2 x 2 blocks, in 64 slices of 2^18, and 10^6 random blocks of four different colours: Y in [16, 235],
    Cb and Cr in [16, 240], each within 0.51 of a code of float64 BT.709 (0.5 is the rounding, the rest the 16-bit coefficients)"""
    worst = np.zeros(3)
    low, high = np.full(3, 255), np.zeros(3, dtype=np.int64)
    gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2)
    for r0 in range(0, 256, 4):
        colours = np.concatenate([np.concatenate([np.full((65536, 1), r), gb], axis=1) for r in range(r0, r0 + 4)]).astype(np.uint8)
        got = uniform_blocks(colours)
        want = bt709(colours.astype(np.float64) / 255)
        for k in range(3):
            worst[k] = max(worst[k], np.abs(got[k] - want[k]).max())
            low[k], high[k] = min(low[k], got[k].min()), max(high[k], got[k].max())
    assert (low[0], high[0]) == (16, 235) and (low[1], high[1]) == (16, 240) and (low[2], high[2]) == (16, 240)
    rs = np.random.RandomState(7)
    n = 1000000
    rgba = rs.randint(0, 256, size=(2, 2 * n, 4)).astype(np.uint8)
    out = library_encode(rgba, I420).astype(np.int32)
    y, cb, cr = out[:4 * n].reshape(2, 2 * n), out[4 * n:5 * n], out[5 * n:]
    real = rgba[..., :3].astype(np.float64) / 255
    worst[0] = max(worst[0], np.abs(y - bt709(real)[0]).max())
    mean = real.reshape(2, n, 2, 3).mean(axis=(0, 2))   # the chroma of a block is that of the mean of its four encoded pixels
    _, want_cb, want_cr = bt709(mean)
    worst[1], worst[2] = max(worst[1], np.abs(cb - want_cb).max()), max(worst[2], np.abs(cr - want_cr).max())
    assert y.min() >= 16 and y.max() <= 235 and min(cb.min(), cr.min()) >= 16 and max(cb.max(), cr.max()) <= 240
    print("largest distance from float64 BT.709 (Y, Cb, Cr):", worst)
    assert (worst <= 0.51).all(), worst


@pytest.mark.parametrize("w,h", [(3, 3), (5, 7), (65, 9), (1, 1), (2, 5), (7, 4)])
def test_an_odd_edge_is_the_edge_pixel_counted_twice(w, h):
    rgba = np.random.RandomState(w * 31 + h).randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    rows, cols = np.minimum(np.arange(h + h % 2), h - 1), np.minimum(np.arange(w + w % 2), w - 1)
    even = rgba[rows][:, cols]
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert even.shape[:2] == (2 * ch, 2 * cw)
    odd_out, even_out = library_encode(rgba, I420), library_encode(even, I420)
    assert odd_out[w * h:].tobytes() == even_out[4 * cw * ch:].tobytes()                              # both chroma planes
    assert odd_out[:w * h].reshape(h, w).tobytes() == even_out[:4 * cw * ch].reshape(2 * ch, 2 * cw)[:h, :w].tobytes()


@pytest.mark.parametrize("w,h", SIZES)
def test_nv12_is_i420_rearranged(w, h):
    rgba = np.random.RandomState(w + 100 * h).randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    i420, nv12 = library_encode(rgba, I420), library_encode(rgba, NV12)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert len(i420) == len(nv12) == w * h + 2 * cw * ch
    assert i420[:w * h].tobytes() == nv12[:w * h].tobytes()
    pairs = nv12[w * h:].reshape(ch, cw, 2)
    assert pairs[..., 0].tobytes() == i420[w * h:w * h + cw * ch].tobytes() and pairs[..., 1].tobytes() == i420[w * h + cw * ch:].tobytes()


def parse_y4m(path):
    """(width, height, (fps_num, fps_den), [frame bytes]) of a YUV4MPEG2 file as this library writes it; everything else is an error"""
    blob = open(path, "rb").read()
    end = blob.index(b"\n")
    m = re.fullmatch(rb"YUV4MPEG2 W(\d+) H(\d+) F(\d+):(\d+) Ip A1:1 C420jpeg XCOLORRANGE=LIMITED", blob[:end])
    assert m, blob[:end]
    w, h, num, den = (int(v) for v in m.groups())
    n = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    body = blob[end + 1:]
    assert len(body) % (6 + n) == 0, (len(body), n)
    frames = []
    for at in range(0, len(body), 6 + n):
        assert body[at:at + 6] == b"FRAME\n"
        frames.append(body[at + 6:at + 6 + n])
    return w, h, (num, den), frames


@pytest.mark.parametrize("w,h,fps", [(16, 8, (24, 1)), (7, 5, (30000, 1001))])
def test_a_y4m_file_reads_back(tmp_path, w, h, fps):
    rs = np.random.RandomState(w)
    frames = [rgba8_to_yuv420(rs.randint(0, 256, size=(h, w, 4)).astype(np.uint8)) for _ in range(3)]
    path = tmp_path / "three.y4m"
    with Y4MWriter(str(path), w, h, fps) as stream:
        for frame in frames:
            stream.write(frame)
        with pytest.raises(ValueError):
            stream.write(frame[:-1])
    header = b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (w, h, fps[0], fps[1])
    blob = path.read_bytes()
    assert blob.startswith(header) and len(blob) == len(header) + 3 * (6 + yuv420_bytes(w, h))
    got = parse_y4m(path)
    assert got[:3] == (w, h, fps) and [bytes(f) for f in got[3]] == [f.tobytes() for f in frames]


def test_the_y4m_writer_refuses_what_it_cannot_write(tmp_path):
    handle = ctypes.c_void_p(1)
    missing = str(tmp_path / "no_such_directory" / "x.y4m").encode()
    assert gra.lib.gr_y4m_open(missing, 16, 8, 24, 1, ctypes.byref(handle)) == -1 and not handle.value
    message = gra.lib.gr_last_error()
    assert b"gr_y4m_open" in message and b"no_such_directory" in message
    with pytest.raises(gra.GeodesicError):
        Y4MWriter(missing.decode(), 16, 8)
    good = str(tmp_path / "x.y4m").encode()
    for args in ((None, 16, 8, 24, 1), (good, 0, 8, 24, 1), (good, 16, -2, 24, 1), (good, 16, 8, 0, 1), (good, 16, 8, 24, 0), (good, 16, 8, -24, 1)):
        handle = ctypes.c_void_p(1)
        assert gra.lib.gr_y4m_open(*args, ctypes.byref(handle)) == -1 and not handle.value, args
        assert b"gr_y4m_open" in gra.lib.gr_last_error()
    assert gra.lib.gr_y4m_open(good, 16, 8, 24, 1, None) == -1
    assert not os.path.exists(good)   # every refusal came before the file was created
    assert gra.lib.gr_y4m_write_frame(None, good) == -1 and gra.lib.gr_y4m_close(None) == -1
    assert gra.lib.gr_y4m_open(good, 16, 8, 24, 1, ctypes.byref(handle)) == 0 and handle.value
    assert gra.lib.gr_y4m_write_frame(handle, None) == -1
    assert gra.lib.gr_y4m_close(handle) == 0
    assert parse_y4m(good.decode()) == (16, 8, (24, 1), [])


def test_a_short_write_is_an_error_and_closes_the_file():
    """/dev/full takes an open and refuses every byte: the header (small sizes) or the frame fails, and close reports the file incomplete"""
    if not os.path.exists("/dev/full"):
        return
    handle = ctypes.c_void_p(1)
    assert gra.lib.gr_y4m_open(b"/dev/full", 16, 8, 24, 1, ctypes.byref(handle)) == -1 and not handle.value
    assert b"short write" in gra.lib.gr_last_error()


def test_the_encode_refuses_bad_arguments():
    rgba, out = np.zeros((2, 2, 4), dtype=np.uint8), np.zeros(6, dtype=np.uint8)
    src, dst = rgba.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 2, 2, I420, dst), (src, 2, 2, I420, None), (src, 0, 2, I420, dst), (src, 2, -1, I420, dst), (src, 2, 2, 2, dst), (src, 2, 2, -1, dst)):
        assert gra.lib.gr_rgba8_to_yuv420(*args) == -1, args
        assert b"gr_rgba8_to_yuv420" in gra.lib.gr_last_error()
    with pytest.raises(ValueError):
        rgba8_to_yuv420(np.zeros((4, 4, 3), dtype=np.uint8))


def test_the_launcher_and_the_frame_entry_check_their_arguments_before_any_device_call():
    """(this box has no GPU, and the answer is not GR_ERROR_DEVICE: the checks precede every HIP call)"""
    src, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)   # never dereferenced: every call below is refused on the host
    for program in (None, src):
        for args in ((None, src, 8, 8, 2, I420), (src, None, 8, 8, 2, I420), (src, src, 8, 8, 0, I420), (src, src, 8, 8, 5, I420),
                     (src, src, 0, 8, 2, I420), (src, src, 8, -1, 2, I420), (src, src, 30000, 20000, 2, I420), (src, src, 2, 600000, 1, NV12),
                     (src, src, 8, 8, 2, 2), (src, src, 8, 8, 2, -1), (src, odd, 8, 8, 2, NV12), (src, ctypes.c_void_p(4097), 8, 8, 1, I420)):
            assert gra.lib.gr_present_yuv420(program, None, *args) == -1, args
            assert b"gr_present_yuv420" in gra.lib.gr_last_error()
    assert gra.lib.gr_present_yuv420(None, None, src, src, 8, 8, 2, I420) == -1   # nothing wrong but the program
    assert b"gr_present_yuv420" in gra.lib.gr_last_error()
    cam, feats, opts = gra.default_camera(), gra.default_features(), gra.frame_options()
    strips = gra.frame_options(mode=gra.MODE_FUSED, strip_count=2, strip_rank=0, block_rows=8)

    def entry(state, program, metric, camera, out, layout, options):
        return gra.lib.gr_render_frame_yuv420(state, program, metric, None, camera, ctypes.byref(feats), None, 0, src, src, 64, 32, 1, out, layout,
                                              ctypes.byref(options))

    for args in ((None, src, src, ctypes.byref(cam), src, I420, opts), (src, None, src, ctypes.byref(cam), src, I420, opts),
                 (src, src, None, ctypes.byref(cam), src, NV12, opts), (src, src, src, None, src, I420, opts),
                 (src, src, src, ctypes.byref(cam), None, I420, opts), (src, src, src, ctypes.byref(cam), src, 2, opts),
                 (src, src, src, ctypes.byref(cam), src, -1, opts), (src, src, src, ctypes.byref(cam), odd, I420, opts),
                 (src, src, src, ctypes.byref(cam), src, I420, strips), (src, src, src, ctypes.byref(cam), src, NV12, strips)):
        assert entry(*args) == -1, args
        assert b"gr_render_frame_yuv420" in gra.lib.gr_last_error()
    assert entry(src, src, src, ctypes.byref(cam), src, I420, strips) == -1 and b"gr_render_frame_tiled_as" in gra.lib.gr_last_error()


def test_the_kernel_is_part_of_the_setup_modules_source_only():
    """the two lists of source files the library assembles its two modules from (csrc/program_build.cpp): the kernel is in a file of the
    set-up module's list and in no file of the frame path's - and the library looks it up in the set-up module (csrc/capi.cpp)"""
    kernels = os.path.join(os.path.dirname(gra.__file__), "csrc", "kernels")
    capi = open(os.path.join(os.path.dirname(gra.__file__), "csrc", "capi.cpp")).read()
    program_build = open(os.path.join(os.path.dirname(gra.__file__), "csrc", "program_build.cpp")).read()
    lists = {name: re.findall(r'"([a-z_]+\.(?:hip|inc))"', body) for name, body in re.findall(r"const (\w*PARTS)\[\] = \{(.*?)\};", program_build, flags=re.S)}
    assert sorted(lists) == ["KERNEL_PARTS", "PARTS"]
    frame_files, setup_files = lists["KERNEL_PARTS"], lists["PARTS"]
    assert "present.hip" in setup_files and "resolve.hip" in setup_files and "present.hip" not in frame_files
    assert "trace.hip" in frame_files and "integrator.hip" in frame_files and "shading.hip" in frame_files

    def source(files):
        return "".join(open(os.path.join(kernels, f)).read() for f in files)

    assert "gr_present_yuv420" in source(setup_files) and "gr_present_rgba8" in source(setup_files)
    assert "gr_trace_fused" in source(frame_files) and "gr_present_yuv420" not in source(frame_files)
    assert re.search(r"is_setup_kernel\(int k\) \{[^}]*K_PRESENT_YUV420", capi)


def test_the_cli_refuses_what_a_video_cannot_be(capsys):
    for argv, word in ((["--devices", "0,1", "--out", "x.y4m"], "--devices"), (["--fps", "0", "--out", "x.y4m"], "--fps"),
                       (["--fps", "24/0", "--out", "x.y4m"], "--fps"), (["--fps", "ntsc", "--out", "x.y4m"], "--fps"),
                       (["--fps", "1/2/3", "--out", "x.png"], "--fps"),
                       (["--camera-to", "0,1,2,3", "--geodesic-speed", "0,0.3,0", "--out", "x.y4m"], "--camera-to")):
        with pytest.raises(SystemExit) as e:
            render.main(["--metric", "kerr_boyer"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not os.path.exists("x.y4m") and not os.path.exists("x.png")


def test_fps_and_camera_paths():
    assert render.parse_fps("24") == (24, 1) and render.parse_fps("30000/1001") == (30000, 1001)
    poses = render.camera_path([0, 0, -8, 0], [0, 0, 0, 1], [0, 4, -4, 2], [0, 1, 0, 0], 5)
    assert len(poses) == 5 and poses[0] == ([0, 0, -8, 0], [0, 0, 0, 1])
    assert np.allclose(poses[2][0], [0, 2, -6, 1]) and np.allclose(poses[4][0], [0, 4, -4, 2])
    assert np.allclose(poses[4][1], [0, 1, 0, 0]) and np.allclose(poses[2][1], [0, np.sqrt(0.5), 0, np.sqrt(0.5)])   # half of a half turn about y
    for _, q in poses:
        assert abs(np.linalg.norm(q) - 1) < 1e-12
    still = render.camera_path([0, 0, -8, 0], None, None, None, 3)
    assert all(pose == still[0] for pose in still)
    far = render.camera_path(None, [0, 0, 0, 1], None, [0, 0, 0.1, -1], 3)   # the shorter arc: -q is the same orientation
    assert far[1][1][3] > 0.99
    with pytest.raises(ValueError):
        render.camera_path(None, [0, 0, 0, 0], None, None, 2)
