"""GPU tests (-m gpu) of video frames encoded on the device: gr_present_yuv420 (kernels/present.hip) on its own against the host
definition (gr_rgba8_to_yuv420 of gr_frame_to_rgba8 of the box filter restated in numpy), byte for byte, at every shape at which the
kernel takes another path, factors 1 to 4, both layouts, between guard bytes; NaN and infinite channels against the device's own RGBA8
bytes; whole frames of gr_render_frame_yuv420 against the same state's gr_render_frame_rgba8; the state's life cycle.  Kerr
(scripts/kerr_boyer.js), a = 0.45."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, encode_srgb8, rgba8_to_yuv420, yuv420_bytes  # noqa: E402
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

GUARD = 256               # bytes either side of a destination (a multiple of 4: the destination stays aligned)
GUARD_BYTE = 0xA5
ONE = 0x3f800000
LAYOUTS = [gra.YUV420_I420, gra.YUV420_NV12]
# 1x1 ... 5x7: less than a lane's block, odd edges; 9, 10, 11 x 4: widths 4k + 1, 2, 3 (the byte-store path); 256x8: one workgroup exactly;
# 257x9, 260x10: one column / row into the next workgroup (260: the 4-byte path); 512x2, 516x6: a wave boundary inside a row pair
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 7), (9, 4), (10, 4), (11, 4), (256, 8), (257, 9), (260, 10), (512, 2), (516, 6)]
_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def thresholds():
    if "table" not in _shared:
        out = (ctypes.c_float * 256)()
        check(lib.gr_srgb8_thresholds(out))
        _shared["table"] = np.array(out[:], dtype=np.float32)
    return _shared["table"]


def source(tw, th, seed):
    """float32 [th, tw, 4]: uniform in [-0.2, 1.3], a tenth exactly 0, a tenth exactly 1, a fifth a table threshold or a neighbour of one"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.2, 1.3, size=(th, tw, 4)).astype(np.float32)
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
    for j in range(f):
        for i in range(f):
            if i or j:
                total = total + src[j::f, i::f]
    return total * (np.float32(1.0) / np.float32(f * f)) if f > 1 else total


def present_yuv420(src, w, h, f, layout):
    """gr_present_yuv420 of the host array `src` (float4, traced size, uploaded into a buffer of exactly its size) into
    yuv420_bytes(w, h) bytes between guard bytes; returns them after checking the guards"""
    _, prog, _ = kerr()
    n = yuv420_bytes(w, h)
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    assert dsrc.nbytes == w * f * h * f * 16
    ddst = DeviceBuffer.from_numpy(0, np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8))
    check(lib.gr_present_yuv420(prog.handle, None, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD), w, h, f, layout))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.uint8, (n + 2 * GUARD,))
    assert (back[:GUARD] == GUARD_BYTE).all() and (back[GUARD + n:] == GUARD_BYTE).all(), "guard bytes were written"
    return back[GUARD:GUARD + n]


def present_rgba8(src, w, h, f):
    _, prog, _ = kerr()
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    ddst = DeviceBuffer(0, w * h * 4)
    check(lib.gr_present_rgba8(prog.handle, None, dsrc.ptr, ddst.ptr, w, h, f, h, 0, 1, 0))
    check(lib.gr_device_synchronize(0))
    return ddst.to_numpy(np.uint8, (h, w, 4))


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_kernel_alone_equals_the_host_definition(w, h):
    for f in (1, 2, 3, 4):
        src = source(w * f, h * f, 10000 * f + 100 * w + h)
        rgba = encode_srgb8(box_filter(src, f))
        for layout in LAYOUTS:
            got, want = present_yuv420(src, w, h, f, layout), rgba8_to_yuv420(rgba, layout)
            differing = np.flatnonzero(got != want)
            assert got.tobytes() == want.tobytes(), (f, layout, len(differing), differing[:8], got[differing[:8]], want[differing[:8]])


@pytest.mark.parametrize("w,h,f", [(67, 5, 1), (12, 6, 2)])
def test_nan_and_infinite_channels_go_through_the_matrix_as_the_rgba8_launch_encodes_them(w, h, f):
    src = np.random.RandomState(5 + f).uniform(0.05, 1.0, size=(h * f, w * f, 4)).astype(np.float32)
    odd = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000], dtype=np.uint32).view(np.float32)   # NaNs, +inf, -inf
    rs = np.random.RandomState(11)
    for k in range(60):
        src[rs.randint(h * f), rs.randint(w * f), rs.randint(4)] = odd[k % len(odd)]
    src[0, 0, :3] = odd[:3]
    src[-1, -1, :3] = odd[3:]
    rgba = present_rgba8(src, w, h, f)
    if f == 1:
        assert (rgba[0, 0, :3] == 0).all()   # three NaNs
    for layout in LAYOUTS:
        assert present_yuv420(src, w, h, f, layout).tobytes() == rgba8_to_yuv420(rgba, layout).tobytes(), layout


def frame(state, kind, layout=None, **options):
    """one frame of `state` for the default camera: "float" float32 [h, w, 4], "rgba8" uint8 [h, w, 4], "yuv420" uint8 [yuv420_bytes]"""
    metric, prog, cfgv = kerr()
    w, h = state.width, state.height
    feats = metric.features(adaptive_sampling=0)
    dbg, levels = background()
    bg = (dbg.ptr, 1024, 512, levels)
    opts = gra.frame_options(mode=gra.MODE_FUSED, **options)
    if kind == "yuv420":
        out = DeviceBuffer.from_numpy(0, np.full(yuv420_bytes(w, h), GUARD_BYTE, dtype=np.uint8))
        state.render_yuv420(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts, layout=layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420_bytes(w, h),))
    out = DeviceBuffer(0, w * h * (4 if kind == "rgba8" else 16))
    (state.render_rgba8 if kind == "rgba8" else state.render)(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts)
    state.synchronize()
    return out.to_numpy(np.uint8 if kind == "rgba8" else np.float32, (h, w, 4))


@pytest.mark.parametrize("w,h,f", [(96, 54, 1), (50, 27, 2)])
def test_a_yuv420_frame_is_the_rgba8_frame_converted(w, h, f):
    state = gra.RenderState(w, h, 0, supersample=f)
    before = frame(state, "float")
    rgba = frame(state, "rgba8")
    assert len(np.unique(rgba[..., :3])) > 32
    for layout in LAYOUTS:
        got = frame(state, "yuv420", layout)
        assert got.tobytes() == rgba8_to_yuv420(rgba, layout).tobytes(), layout
        assert len(np.unique(got[w * h:])) > 4   # the picture has colour: the chroma planes are not flat
    assert frame(state, "float").tobytes() == before.tobytes()
    # a strip-mode call is refused, and leaves the state as it was
    metric, prog, cfgv = kerr()
    dbg, levels = background()
    out = DeviceBuffer(0, yuv420_bytes(w, h))
    with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled_as"):
        state.render_yuv420(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                            gra.frame_options(mode=gra.MODE_FUSED, strip_count=2, strip_rank=0, block_rows=8))
    assert frame(state, "float").tobytes() == before.tobytes()


def test_a_state_used_for_all_three_kinds_of_frame_gives_its_memory_back():
    """float, RGBA8 and YUV frames in turn on one stream of one state, at factors 1 and 2: every kind is what a fresh state gives, and free
    device memory after the state is gone is what it was before it was made (the allowance of tests/test_gpu_lifecycle.py)"""
    from test_gpu_lifecycle import MiB, device_bytes_in_use
    metric, prog, cfgv = kerr()
    background()
    w, h = 64, 32

    def cycle(f):
        stream = ctypes.c_void_p()
        check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
        try:
            state = gra.RenderState(w, h, 0, supersample=f)
            feats = metric.features(adaptive_sampling=0)
            dbg, levels = background()
            bg = (dbg.ptr, 1024, 512, levels)
            opts = gra.frame_options(mode=gra.MODE_FUSED)
            f32, u8, yuv = DeviceBuffer(0, w * h * 16), DeviceBuffer(0, w * h * 4), DeviceBuffer(0, yuv420_bytes(w, h))
            results = []
            for _ in range(2):
                state.render(prog, metric, gra.default_camera(), f32.ptr, bg, feats, cfgv, opts, stream)
                state.render_rgba8(prog, metric, gra.default_camera(), u8.ptr, bg, feats, cfgv, opts, stream)
                state.render_yuv420(prog, metric, gra.default_camera(), yuv.ptr, bg, feats, cfgv, opts, stream)
                check(lib.gr_stream_synchronize(stream))
                results.append((f32.to_numpy(np.float32, (h, w, 4)), u8.to_numpy(np.uint8, (h, w, 4)), yuv.to_numpy(np.uint8, (yuv420_bytes(w, h),))))
            del state, f32, u8, yuv
            gc.collect()
            return results
        finally:
            check(lib.gr_stream_destroy(stream))

    for f in (1, 2):
        first = cycle(f)
        before = device_bytes_in_use()
        for _ in range(5):
            results = cycle(f)
        after = device_bytes_in_use()
        assert after - before < 4 * MiB, (f, before, after)
        for floats, rgba, yuv in results + first:
            assert floats.tobytes() == first[0][0].tobytes()
            assert rgba.tobytes() == encode_srgb8(floats).tobytes()
            assert yuv.tobytes() == rgba8_to_yuv420(rgba).tobytes()
