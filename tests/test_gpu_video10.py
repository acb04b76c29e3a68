"""GPU tests (-m gpu) of 10-bit video frames encoded on the device: gr_present_yuv420p10 (kernels/present.hip) on its own against the host
definition (gr_rgb10_to_yuv420p10 of gr_frame_to_rgb10 of the box filter restated in numpy), word for word, at every shape at which the
kernel takes another path, factors 1 to 4, both layouts, between guard bytes and from a source of exactly its size; a frame that holds
every finite threshold of the table with its two neighbours, NaN, both infinities and -0; whole frames of gr_render_frame_yuv420p10
against the same state's float frame, with the state's other formats unchanged around them; the refusal of strips; the CLI's file.
Kerr (scripts/kerr_boyer.js), a = 0.45."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib, render  # noqa: E402
from geodesic_raytracing_amd.pipeline import (DeviceBuffer, frame_to_rgb10, rgb10_to_yuv420p10, srgb10_thresholds, yuv420_bytes,  # noqa: E402
                                              yuv420p10_bytes)
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

GUARD = 256               # bytes either side of a destination (a multiple of 8: the destination stays aligned)
GUARD_BYTE = 0xA5
LAYOUTS = [gra.YUV420_I420, gra.YUV420_NV12]
# 1x1 ... 5x7: less than a lane's block, odd edges, the word-store path; 8x2: the 8-byte path in one lane pair; 65x9: two waves' worth of
# columns with an odd edge; 64x6: the 8-byte path with lanes that leave after the table copy; 260x10: two workgroups each way, 8-byte path
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 7), (8, 2), (65, 9), (260, 10), (64, 6)]
_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def thresholds():
    if "table" not in _shared:
        _shared["table"] = srgb10_thresholds()
    return _shared["table"]


def source(tw, th, seed):
    """float32 [th, tw, 4]: uniform in [-0.1, 1.2], a tenth exactly 0, a tenth exactly 1, a fifth a table threshold or a neighbour of one"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.1, 1.2, size=(th, tw, 4)).astype(np.float32)
    kind = rs.uniform(size=v.shape)
    v[kind < 0.1] = 0
    v[(kind >= 0.1) & (kind < 0.2)] = 1
    t = thresholds()
    finite = t[np.isfinite(t)][1:].view(np.uint32).astype(np.int64)
    near = (finite[rs.randint(0, len(finite), size=v.shape)] + rs.randint(-2, 3, size=v.shape)).astype(np.uint32).view(np.float32)
    at = (kind >= 0.2) & (kind < 0.4)
    v[at] = near[at]
    return v


def box_filter(src, f):
    """box_average<F> of kernels/resolve.hip restated: the block summed in fp32 in the kernel's order, times the rounded 1 / f^2"""
    total = src[0::f, 0::f].copy()
    with np.errstate(invalid="ignore"):
        for j in range(f):
            for i in range(f):
                if i or j:
                    total = total + src[j::f, i::f]
        return total * (np.float32(1.0) / np.float32(f * f)) if f > 1 else total


def host_definition(src, f, layout):
    """the words the definition gives for the traced frame `src`: a NaN's code is 0 (the device's rule; the host's is undefined)"""
    resolved = box_filter(src, f)
    resolved[np.isnan(resolved)] = 0
    return rgb10_to_yuv420p10(frame_to_rgb10(resolved), layout)


def present_yuv420p10(src, w, h, f, layout):
    """gr_present_yuv420p10 of the host array `src` (float4, traced size, uploaded into a buffer of exactly its size) into
    yuv420p10_bytes(w, h) bytes between guard bytes; returns the words after checking the guards"""
    _, prog, _ = kerr()
    n = yuv420p10_bytes(w, h)
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    assert dsrc.nbytes == w * f * h * f * 16
    ddst = DeviceBuffer.from_numpy(0, np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8))
    check(lib.gr_present_yuv420p10(prog.handle, None, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD), w, h, f, layout))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.uint8, (n + 2 * GUARD,))
    assert (back[:GUARD] == GUARD_BYTE).all() and (back[GUARD + n:] == GUARD_BYTE).all(), "guard bytes were written"
    return back[GUARD:GUARD + n].copy().view("<u2")


def same_words(got, want, what):
    differing = np.flatnonzero(got != want)
    assert got.tobytes() == want.astype("<u2").tobytes(), (what, len(differing), differing[:8], got[differing[:8]], want[differing[:8]])


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_kernel_alone_equals_the_host_definition(w, h):
    for f in (1, 2, 3, 4):
        src = source(w * f, h * f, 10000 * f + 100 * w + h)
        for layout in LAYOUTS:
            got = present_yuv420p10(src, w, h, f, layout)
            same_words(got, host_definition(src, f, layout), (f, layout))
            assert (got & 63 == 0).all() if layout == gra.YUV420_NV12 else (got <= 1023).all()


@pytest.mark.parametrize("f", [1, 2, 3, 4])
def test_every_threshold_its_neighbours_and_the_values_that_are_no_numbers(f):
    """260 x 10 (7 800 colour channels): every finite entry of the table, the float below and the float above it, then NaNs, +inf, -inf,
    -0, 0 and 1.  At f = 1 the frame is the source.  At f = 2 and 4 the first traced pixel of a block holds f^2 times the value and the
    others 0: v f^2 + 0 + ... + 0 is exact and so is the product with 1 / f^2, so the resolved value IS that float (the sum of f^2 equal
    floats in the kernel's order is not: 3 v rounds).  At f = 3, where 1 / 9 rounds, the block holds the value f^2 times and the
    resolved values are whatever the definition makes of them."""
    w, h = 260, 10
    t = thresholds()
    finite = t[np.isfinite(t)][1:].view(np.uint32).astype(np.int64)
    assert len(finite) in (1022, 1023)
    exact = np.concatenate([finite - 1, finite, finite + 1]).astype(np.uint32)
    odd = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000, 0x80000000, 0, 0x3f800000], dtype=np.uint32)
    values = np.concatenate([exact, np.tile(odd, 40)]).view(np.float32)
    assert len(values) <= w * h * 3
    pixels = np.random.RandomState(f).uniform(-0.1, 1.2, size=(h, w, 4)).astype(np.float32)
    colour = pixels[..., :3].reshape(-1)
    colour[np.random.RandomState(100 + f).permutation(colour.size)[:len(values)]] = values
    pixels[..., :3] = colour.reshape(h, w, 3)
    if f == 3:
        src = np.repeat(np.repeat(pixels, f, axis=0), f, axis=1)
    else:
        src = np.zeros((h * f, w * f, 4), dtype=np.float32)
        with np.errstate(invalid="ignore"):
            src[0::f, 0::f] = pixels * np.float32(f * f)   # (a power of two: exact)
        assert np.array_equal(box_filter(src, f), pixels, equal_nan=True)   # (-0 comes back as 0 at f > 1: the same code)
    codes = frame_to_rgb10(np.nan_to_num(pixels, nan=0.0, posinf=np.inf, neginf=-np.inf))
    assert len(np.unique(codes)) == len(finite) + 1   # every code there is appears
    for layout in LAYOUTS:
        same_words(present_yuv420p10(src, w, h, f, layout), host_definition(src, f, layout), (f, layout))


def frame(state, kind, layout=None, **options):
    """one frame of `state` for the default camera: "float" float32 [h, w, 4], "rgba8" uint8 [h, w, 4], "yuv420" uint8 [yuv420_bytes],
    "yuv420p10" uint16 [yuv420p10_bytes / 2]"""
    metric, prog, cfgv = kerr()
    w, h = state.width, state.height
    feats = metric.features(adaptive_sampling=0)
    dbg, levels = background()
    bg = (dbg.ptr, 1024, 512, levels)
    opts = gra.frame_options(mode=gra.MODE_FUSED, **options)
    if kind == "yuv420p10":
        out = DeviceBuffer.from_numpy(0, np.full(yuv420p10_bytes(w, h), GUARD_BYTE, dtype=np.uint8))
        state.render_yuv420p10(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts, layout=layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420p10_bytes(w, h),)).copy().view("<u2")
    if kind == "yuv420":
        out = DeviceBuffer(0, yuv420_bytes(w, h))
        state.render_yuv420(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts, layout=layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420_bytes(w, h),))
    out = DeviceBuffer(0, w * h * (4 if kind == "rgba8" else 16))
    (state.render_rgba8 if kind == "rgba8" else state.render)(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts)
    state.synchronize()
    return out.to_numpy(np.uint8 if kind == "rgba8" else np.float32, (h, w, 4))


@pytest.mark.parametrize("f", [1, 2])
def test_a_10_bit_frame_is_the_float_frame_converted_and_leaves_the_other_formats_alone(f):
    w, h = 64, 48
    state = gra.RenderState(w, h, 0, supersample=f)
    before = [frame(state, "float"), frame(state, "rgba8"), frame(state, "yuv420", gra.YUV420_I420), frame(state, "yuv420", gra.YUV420_NV12)]
    assert np.isfinite(before[0]).all()
    codes = frame_to_rgb10(before[0])
    assert len(np.unique(codes)) > 64
    for layout in LAYOUTS:
        got = frame(state, "yuv420p10", layout)
        same_words(got, rgb10_to_yuv420p10(codes, layout), layout)
        assert len(np.unique(got[w * h:])) > 4   # the picture has colour: the chroma planes are not flat
    after = [frame(state, "float"), frame(state, "rgba8"), frame(state, "yuv420", gra.YUV420_I420), frame(state, "yuv420", gra.YUV420_NV12)]
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("f", [1, 2])
def test_strips_are_refused_and_nothing_is_written(f):
    w, h = 64, 48
    state = gra.RenderState(w, h, 0, supersample=f)
    metric, prog, cfgv = kerr()
    dbg, levels = background()
    n = yuv420p10_bytes(w, h)
    out = DeviceBuffer.from_numpy(0, np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8))
    with pytest.raises(gra.GeodesicError, match="gr_render_frame_yuv420p10.*gr_render_frame_tiled_as"):
        state.render_yuv420p10(prog, metric, gra.default_camera(), ctypes.c_void_p(out.ptr.value + GUARD), (dbg.ptr, 1024, 512, levels),
                               metric.features(adaptive_sampling=0), cfgv, gra.frame_options(mode=gra.MODE_FUSED, strip_count=2, strip_rank=0, block_rows=8))
    check(lib.gr_device_synchronize(0))
    assert (out.to_numpy(np.uint8, (n + 2 * GUARD,)) == GUARD_BYTE).all()


def test_the_cli_writes_the_frames_render_returns(tmp_path):
    path = str(tmp_path / "x.y4m")
    w, h = 64, 48
    assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "64x48", "--frames", "3", "--camera", "0,0,-8,0", "--camera-to", "0,2,-7,0",
                        "--bit-depth", "10", "--out", path]) == 0
    frames = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], yuv420=True, bit_depth=10,
                           cameras=render.camera_path([0, 0, -8, 0], None, [0, 2, -7, 0], None, 3))
    assert len(frames) == 3 and all(fr.dtype == np.uint16 and fr.size == yuv420p10_bytes(w, h) // 2 for fr in frames)
    assert frames[0].tobytes() != frames[2].tobytes() and max(fr.max() for fr in frames) <= 1023
    header = b"YUV4MPEG2 W64 H48 F24:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n"
    blob = open(path, "rb").read()
    assert blob == header + b"".join(b"FRAME\n" + fr.astype("<u2").tobytes() for fr in frames)
