"""GPU tests (-m gpu) of filtered frames: gr_resolve_filtered (kernels/filter.hip) on its own against the host definition gr_filter_frame,
bit for bit - one pixel, sizes either side of the kernel's 32 x 8 tile (and of the 64- and 16-wide tiles that were candidates), a frame
narrower than the filter; the three named tables and an uneven one that tells a reversed order and swapped passes apart; between guard
bands; with zeros of both signs, infinities and NaN planted.  Whole frames of a state with a filter in every format against
gr_filter_frame of the traced frame a plain state of the traced size renders (tests/test_gpu_supersample.py rests on those two being
the same frame) and the host encodes of that; sub-frames of a shutter; GR_FILTER_BOX set explicitly against an untouched state; tent at
factor 1; the refusals; device memory over create / set filter / render / destroy cycles; the CLI's files.  Kerr (scripts/kerr_boyer.js),
a = 0.45, the substituted program."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib, render  # noqa: E402
from geodesic_raytracing_amd.pipeline import (DeviceBuffer, accumulate_frame, encode_srgb8, filter_frame, filter_taps, frame_to_rgb10,  # noqa: E402
                                              rgb10_to_yuv420p10, rgba8_to_yuv420, yuv420_bytes)
from test_gpu_lifecycle import MiB, device_bytes_in_use  # noqa: E402
from test_gpu_shutter import CAMERAS, bits, delivered, kerr, plain_frame, same_bits, sky, subframe  # noqa: E402

GUARD = 64                # float4 either side of the destination
GUARD_VALUE = np.float32(-777.25)
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4), (5, 3, 2), (67, 9, 3), (130, 2, 4), (64, 8, 1), (33, 17, 4), (65, 5, 2)]   # (w, h, f)
FRAMES = [(48, 24, 2), (40, 24, 3), (24, 16, 4), (37, 21, 2), (48, 24, 1)]
NAMED = ("tent", "gaussian", "mitchell")
# distinct, asymmetric, of both signs (tests/test_filter_abi.py's): 16 taps for an even factor, 15 for an odd one
UNEVEN = {0: np.array([0.01 * (t + 1) * (-1 if t % 3 == 1 else 1) for t in range(16)], dtype=np.float32),
          1: np.array([0.013 * (t + 2) * (-1 if t % 4 == 2 else 1) for t in range(15)], dtype=np.float32)}
_traced = {}


def source(tw, th, seed):
    """float32 [th, tw, 4]: normal-range values of both signs over six decades with +0, -0, both infinities and NaN planted - few enough
    that most 16 x 16 footprints stay finite (no subnormals: what the module does with them is not established)"""
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal((th, tw, 4)) * np.exp(rs.uniform(-7, 7, (th, tw, 4)))).astype(np.float32)
    v[np.abs(v) < 1e-20] = 1
    kind = rs.uniform(size=v.shape)
    for k, (planted, share) in enumerate([(0.0, 0.01), (-0.0, 0.01), (np.inf, 0.0003), (-np.inf, 0.0003), (np.nan, 0.0003)]):
        v[(kind >= 0.01 * k) & (kind < 0.01 * k + share)] = planted
    return v


def resolve_filtered(src, w, h, f, taps):
    """gr_resolve_filtered of the host array `src` into a destination between guard bands that holds NaN beforehand"""
    _, prog, _, _ = kerr()
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    buf = np.full((w * h + 2 * GUARD, 4), GUARD_VALUE, dtype=np.float32)
    buf[GUARD:GUARD + w * h] = np.nan
    ddst = DeviceBuffer.from_numpy(0, buf)
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    assert dsrc.nbytes == w * f * h * f * 16
    check(lib.gr_resolve_filtered(prog.handle, None, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD * 16), w, h, f, taps.ctypes.data_as(ctypes.c_void_p), len(taps)))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.float32, (w * h + 2 * GUARD, 4))
    assert (bits(back[:GUARD]) == bits(GUARD_VALUE)).all() and (bits(back[GUARD + w * h:]) == bits(GUARD_VALUE)).all(), "guard bands were written"
    return back[GUARD:GUARD + w * h].reshape(h, w, 4).copy()


@pytest.mark.parametrize("w,h,f", SHAPES)
def test_the_launcher_alone_equals_the_definition(w, h, f):
    finite = numbers = 0
    src = source(w * f, h * f, 1000 * f + 10 * w + h)
    for taps in [filter_taps(name, f) for name in NAMED] + [UNEVEN[f % 2]]:
        with np.errstate(all="ignore"):
            want = filter_frame(src, f, taps)
        got = resolve_filtered(src, w, h, f, taps)
        same_bits(got, want, (f, len(taps)))
        finite, numbers = finite + int(np.isfinite(want).sum()), numbers + want.size
    if w * h > 1:
        assert finite > numbers // 2   # most of what was compared are numbers
    # a single tap of 1 at factor 1 is the identity on bit patterns, the sign of a zero included
    src = source(w, h, 7 + w)
    got = resolve_filtered(src, w, h, 1, [1.0])
    same_bits(got, src, "identity")
    assert (bits(got)[src == 0] == bits(src)[src == 0]).all()


def test_the_launchers_refusals():
    _, prog, _, _ = kerr()
    src, dst = DeviceBuffer(0, 8 * 8 * 16), DeviceBuffer(0, 4 * 4 * 16)
    good = filter_taps("tent", 2)
    t = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    bad = np.array([0.5, np.nan, 0.25, 0.25], dtype=np.float32)
    for args in ((None, dst.ptr, 4, 4, 2, t(good), 4), (src.ptr, None, 4, 4, 2, t(good), 4), (src.ptr, dst.ptr, 4, 4, 2, None, 4),
                 (src.ptr, dst.ptr, 0, 4, 2, t(good), 4), (src.ptr, dst.ptr, 4, 4, 5, t(good), 4), (src.ptr, dst.ptr, 4, 4, 2, t(good), 3),
                 (src.ptr, dst.ptr, 4, 4, 2, t(good), 17), (src.ptr, dst.ptr, 4, 4, 2, t(bad), 4), (src.ptr, src.ptr, 4, 4, 2, t(good), 4),
                 (src.ptr, dst.ptr, 30000, 20000, 2, t(good), 4)):
        assert lib.gr_resolve_filtered(prog.handle, None, *args) == -1, args
        assert b"gr_resolve_filtered" in lib.gr_last_error()
    check(lib.gr_resolve_filtered(prog.handle, None, src.ptr, dst.ptr, 4, 4, 2, t(good), 4))
    check(lib.gr_device_synchronize(0))


def traced_frame(w, h, f, camera_index=1):
    """the frame a plain state of the traced size renders for CAMERAS[camera_index]: rendered once, shared, never written to"""
    key = (w, h, f, camera_index)
    if key not in _traced:
        frame = plain_frame(gra.RenderState(w * f, h * f, 0), gra.default_camera(*CAMERAS[camera_index]))
        assert np.isfinite(frame).all() and len(np.unique(encode_srgb8(frame))) > 32
        frame.setflags(write=False)
        _traced[key] = frame
    return _traced[key]


@pytest.mark.parametrize("w,h,f", FRAMES)
def test_a_filtered_states_frame_is_the_filter_of_the_traced_frame(w, h, f):
    camera = gra.default_camera(*CAMERAS[1])
    traced = traced_frame(w, h, f)
    seen = []
    for name in NAMED:
        state = gra.RenderState(w, h, 0, supersample=f, filter=name)
        assert state.filter == gra.FILTER_NAMES[name] and state.supersample == f
        want = filter_frame(traced, f, filter_taps(name, f))
        same_bits(plain_frame(state, camera, time_kernels=1), want, name)
        assert state.resolve_ms() > 0   # the filter launch, between the resolve's events
        seen.append(want.tobytes())
    if f > 1:
        assert len(set(seen)) == 3   # the three filters give three pictures
    # the filter may change between frames of one state, to the box and back
    state = gra.RenderState(w, h, 0, supersample=f)
    box = plain_frame(state, camera)
    state.set_filter("mitchell")
    same_bits(plain_frame(state, camera), filter_frame(traced, f, filter_taps("mitchell", f)), "set between frames")
    state.set_filter(gra.FILTER_BOX)
    assert plain_frame(state, camera).tobytes() == box.tobytes()


@pytest.mark.parametrize("w,h,f", [FRAMES[0], FRAMES[3]])
def test_every_format_is_the_encode_of_the_filtered_frame(w, h, f):
    camera = gra.default_camera(*CAMERAS[1])
    want = filter_frame(traced_frame(w, h, f), f, filter_taps("mitchell", f))
    state = gra.RenderState(w, h, 0, supersample=f, filter=gra.FILTER_MITCHELL)
    rgba8 = encode_srgb8(want)
    codes = frame_to_rgb10(want)
    assert plain_frame(state, camera, "rgba8").tobytes() == rgba8.tobytes()
    for layout in (I420, NV12):
        assert plain_frame(state, camera, "yuv420", layout).tobytes() == rgba8_to_yuv420(rgba8, layout).tobytes(), layout
        assert plain_frame(state, camera, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(codes, layout).astype("<u2").tobytes(), layout
    same_bits(plain_frame(state, camera), want, "float4 after the encodes")


def test_three_subframes_of_a_filtered_state():
    w, h, f = FRAMES[0]
    taps = filter_taps("mitchell", f)
    weight = np.float32(1) / np.float32(3)
    want = np.zeros((h, w, 4), dtype=np.float32)
    for j in range(3):
        accumulate_frame(want, filter_frame(traced_frame(w, h, f, j), f, taps), weight, j == 0)
    state = gra.RenderState(w, h, 0, supersample=f, filter="mitchell")
    for j, (position, quat) in enumerate(CAMERAS):
        subframe(state, gra.default_camera(position, quat), weight, j == 0)
    same_bits(delivered(state, "float"), want, "filter, then accumulate")
    assert delivered(state, "rgba8").tobytes() == encode_srgb8(want).tobytes()


@pytest.mark.parametrize("f", [1, 2])
def test_the_box_set_explicitly_is_an_untouched_state(f):
    w, h = 48, 24
    camera = gra.default_camera(*CAMERAS[1])
    untouched, box = gra.RenderState(w, h, 0, supersample=f), gra.RenderState(w, h, 0, supersample=f, filter="tent")
    box.set_filter(gra.FILTER_BOX)
    assert untouched.filter == gra.FILTER_BOX == box.filter
    assert plain_frame(box, camera).tobytes() == plain_frame(untouched, camera).tobytes()
    assert plain_frame(box, camera, "rgba8").tobytes() == plain_frame(untouched, camera, "rgba8").tobytes()
    for layout in (I420, NV12):
        assert plain_frame(box, camera, "yuv420", layout).tobytes() == plain_frame(untouched, camera, "yuv420", layout).tobytes()
        assert plain_frame(box, camera, "yuv420p10", layout).tobytes() == plain_frame(untouched, camera, "yuv420p10", layout).tobytes()
    subframe(box, camera, 1.0, True)
    subframe(untouched, camera, 1.0, True)
    assert delivered(box, "float").tobytes() == delivered(untouched, "float").tobytes()


def test_tent_at_factor_one_is_the_plain_frame():
    w, h = 48, 24
    camera = gra.default_camera(*CAMERAS[1])
    state = gra.RenderState(w, h, 0, filter="tent")
    assert plain_frame(state, camera).tobytes() == traced_frame(w, h, 1).tobytes()
    assert plain_frame(state, camera, "rgba8").tobytes() == encode_srgb8(traced_frame(w, h, 1)).tobytes()


def test_split_frames_refuse_a_filtered_state():
    w, h = 48, 24
    metric, prog, cfgv, feats = kerr()
    camera = gra.default_camera(*CAMERAS[1])
    out = DeviceBuffer(0, w * h * 16)
    for f in (1, 2):
        state = gra.RenderState(w, h, 0, supersample=f, filter="gaussian")
        for kind in ("float", "rgba8"):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame.*filter.*strip_count"):
                plain_frame(state, camera, kind, strip_count=2, strip_rank=0, block_rows=8)
        with pytest.raises(gra.GeodesicError, match="gr_render_subframe.*strip_count"):
            subframe(state, camera, 1.0, True, strip_count=2, strip_rank=0, block_rows=8)
        (part,) = gra.TiledFrame.local([0], w, h, 8)
        opts = gra.frame_options(mode=gra.MODE_FUSED)
        if f == 1:
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled:.*filter"):
                part.render(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)
        for rgba8 in (False, True):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled_as:.*filter"):
                part.render_as(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts, rgba8=rgba8)
        # nothing was rendered or allocated by the refused calls: the state's first frame is the filtered frame all the same
        same_bits(plain_frame(state, camera), filter_frame(traced_frame(w, h, f), f, filter_taps("gaussian", f)), "after the refusals")
        state.set_filter("box")
        part.render_as(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)   # the box state is taken
        state.synchronize()
        part.close()
    with pytest.raises(gra.GeodesicError, match="gr_render_state_set_filter.*unknown filter"):
        gra.RenderState(w, h, 0).set_filter(4)


def one_cycle(size, f, name):
    state = gra.RenderState(size[0], size[1], 0, supersample=f)
    state.set_filter(name)
    camera = gra.default_camera(*CAMERAS[0])
    assert plain_frame(state, camera, "yuv420", I420).size == yuv420_bytes(*size)
    assert plain_frame(state, camera).shape == (size[1], size[0], 4)
    del state
    gc.collect()


def test_the_filtered_frame_is_freed_with_the_state():
    """tests/test_gpu_lifecycle.py's method: two cycles first (runtime pools, code objects, the sky), then ten between two readings of
    hipMemGetInfo.  A 640 x 360 filtered frame is 3.5 MiB: one that stayed behind per cycle would show ten times over."""
    one_cycle((640, 360), 1, "mitchell")
    one_cycle((320, 180), 2, "tent")
    before = device_bytes_in_use()
    for k in range(10):
        one_cycle((640, 360), 1 if k % 2 else 2, NAMED[k % 3])
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


def test_the_cli_writes_filtered_files(tmp_path):
    """--filter mitchell --supersample 2: a PNG and a 2-frame .y4m hold the encodes of the filtered frames render() returns, which are
    gr_filter_frame of the traced frames"""
    w, h, f = 48, 24, 2
    base = ["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", f"{w}x{h}", "--camera", "0,0,-8,0", "--filter", "mitchell", "--supersample", str(f)]
    png = str(tmp_path / "x.png")
    assert render.main(base + ["--encode", "device", "--out", png]) == 0
    traced = render.render("kerr_boyer", w * f, h * f, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0])
    want = filter_frame(traced, f, filter_taps("mitchell", f))
    got = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], supersample=f, filter="mitchell")
    same_bits(got, want, "render(filter=)")
    assert render.read_png(png).tobytes() == encode_srgb8(want).tobytes()
    assert render.read_png(png).tobytes() != encode_srgb8(render.render("kerr_boyer", w, h, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], supersample=f)).tobytes()
    y4m = str(tmp_path / "x.y4m")
    assert render.main(base + ["--camera-to", "0,2,-7,0", "--frames", "2", "--out", y4m]) == 0
    cameras = render.camera_path([0, 0, -8, 0], None, [0, 2, -7, 0], None, 2)
    frames = [filter_frame(fr, f, filter_taps("mitchell", f)) for fr in render.render("kerr_boyer", w * f, h * f, cfg={"a": 0.45}, cameras=cameras)]
    header = b"YUV4MPEG2 W48 H24 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert open(y4m, "rb").read() == header + b"".join(b"FRAME\n" + rgba8_to_yuv420(encode_srgb8(fr)).tobytes() for fr in frames)
