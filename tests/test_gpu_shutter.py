"""GPU tests (-m gpu) of motion-blurred frames: gr_shutter_accumulate (kernels/shutter.hip) on its own against the definition in numpy
float32 - the box filter restated, then one rounded multiply and one rounded add a sub-frame - bit for bit, at sizes below, at and
above a workgroup, factors 1 to 4, one to eight sub-frames, between guard bands and into a buffer full of NaN; whole frames of
gr_render_subframe / gr_deliver_accumulated in every format against the same cameras through gr_render_frame on a second state,
accumulated and encoded on the host; one sub-frame of weight 1 against the plain entry points; the camera on its geodesic; the refusals
that need a state; device memory over create / accumulate / deliver / destroy cycles; the CLI's file.  Kerr (scripts/kerr_boyer.js), a = 0.45, the
substituted program."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib, render  # noqa: E402
from geodesic_raytracing_amd.pipeline import (DeviceBuffer, encode_srgb8, frame_to_rgb10, rgb10_to_yuv420p10, rgba8_to_yuv420,  # noqa: E402
                                              yuv420_bytes, yuv420p10_bytes)
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402
from test_gpu_lifecycle import MiB, device_bytes_in_use  # noqa: E402

GUARD = 64                # float4 either side of an accumulation frame
GUARD_VALUE = np.float32(-777.25)
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
# one lane; less than a wave; exactly one workgroup; one more column and one more row than that; three workgroups along a row
SIZES = [(1, 1), (3, 2), (64, 4), (65, 5), (130, 3)]
WEIGHTS = [[np.float32(1)], [np.float32(1) / np.float32(2)] * 2, [np.float32(1) / np.float32(3)] * 3, [np.float32(1) / np.float32(8)] * 8,
           [np.float32(0.5), np.float32(0.25), np.float32(0.25)]]
# three cameras a few pixels apart at 64 x 36 (fov 90: a pixel is about 1 / 32 rad)
CAMERAS = [([0.0, 0.0, -8.0, 0.0], None), ([0.0, 0.25, -8.0, 0.1], None), ([0.0, 0.5, -7.9, 0.2], None)]
_shared = {}


def kerr():
    """the substituted program of a = 0.45 without adaptive sampling (the one the benchmark renders with), shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        cfgv = metric.cfg_values(a=0.45)
        feats = metric.features(adaptive_sampling=0)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(features=feats, static=True, cfg_values=cfgv), 0), cfgv, feats)
    return _shared["kerr"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what=None):
    """bit patterns equal wherever the value is a number, a NaN exactly where a NaN is wanted (which NaN an operation returns is the one
    thing IEEE 754 leaves open, and the host's and the device's differ)"""
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    differing = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    differing = differing[~nan.reshape(-1)[differing]]
    assert len(differing) == 0, (what, len(differing), differing[:8], got.reshape(-1)[differing[:8]], want.reshape(-1)[differing[:8]])


def source(tw, th, seed):
    """float32 [th, tw, 4]: normal-range values of both signs over six decades, with +0, -0, both infinities and NaN planted (no
    subnormals: what the module does with them is not established)"""
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal((th, tw, 4)) * np.exp(rs.uniform(-7, 7, (th, tw, 4)))).astype(np.float32)
    v[np.abs(v) < 1e-20] = 1
    kind = rs.uniform(size=v.shape)
    for k, (planted, share) in enumerate([(0.0, 0.02), (-0.0, 0.02), (np.inf, 0.002), (-np.inf, 0.002), (np.nan, 0.002)]):
        v[(kind >= 0.02 * k) & (kind < 0.02 * k + share)] = planted   # (few enough that most 4 x 4 blocks of eight sub-frames stay finite)
    return v


def box_filter(src, f):
    """box_average<F> of kernels/resolve.hip restated: the block summed in fp32 in the kernel's order, times the rounded 1 / f^2"""
    total = src[0::f, 0::f].copy()
    with np.errstate(all="ignore"):
        for j in range(f):
            for i in range(f):
                if i or j:
                    total = total + src[j::f, i::f]
        return total * (np.float32(1.0) / np.float32(f * f)) if f > 1 else total


def step(accum, frame, weight, first):
    """the definition: one rounded fp32 multiply, one rounded fp32 add"""
    with np.errstate(all="ignore"):
        product = np.float32(weight) * frame
        assert product.dtype == np.float32
        return product if first else accum + product


def shutter_accumulate(sources, w, h, f, weights, prefill):
    """gr_shutter_accumulate of the host arrays `sources` in turn, the first with `first`, into an accumulation frame between guard bands
    that holds `prefill` beforehand; returns the frame after checking the guards"""
    _, prog, _, _ = kerr()
    buf = np.full((w * h + 2 * GUARD, 4), GUARD_VALUE, dtype=np.float32)
    buf[GUARD:GUARD + w * h] = prefill
    daccum = DeviceBuffer.from_numpy(0, buf)
    for j, (src, weight) in enumerate(zip(sources, weights)):
        dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
        assert dsrc.nbytes == w * f * h * f * 16
        check(lib.gr_shutter_accumulate(prog.handle, None, dsrc.ptr, ctypes.c_void_p(daccum.ptr.value + GUARD * 16), w, h, f, float(weight), int(j == 0)))
        check(lib.gr_device_synchronize(0))
    back = daccum.to_numpy(np.float32, (w * h + 2 * GUARD, 4))
    assert (bits(back[:GUARD]) == bits(GUARD_VALUE)).all() and (bits(back[GUARD + w * h:]) == bits(GUARD_VALUE)).all(), "guard bands were written"
    return back[GUARD:GUARD + w * h].reshape(h, w, 4).copy()


@pytest.mark.parametrize("w,h", SIZES)
def test_the_launcher_alone_equals_the_definition(w, h):
    finite = numbers = 0
    for f in (1, 2, 3, 4):
        for k, weights in enumerate(WEIGHTS):
            sources = [source(w * f, h * f, 100000 * f + 1000 * k + 100 * j + w + h) for j in range(len(weights))]
            want = None
            for j, (src, weight) in enumerate(zip(sources, weights)):
                want = step(want, box_filter(src, f), weight, j == 0)
            # the frame holds NaN beforehand: with `first` it is written and not read
            got = shutter_accumulate(sources, w, h, f, weights, np.float32(np.nan))
            same_bits(got, want, (f, [float(x) for x in weights]))
            finite, numbers = finite + int(np.isfinite(want).sum()), numbers + want.size
    assert finite > numbers // 2   # most of what was compared are numbers
    # a weight of 1 at factor 1 is the identity on bit patterns, the sign of a zero included
    src = source(w, h, 7 + w)
    got = shutter_accumulate([src], w, h, 1, [np.float32(1)], np.float32(0))
    same_bits(got, src, "identity")
    assert (bits(got)[src == 0] == bits(src)[src == 0]).all()


def sky():
    dbg, levels = background()
    return (dbg.ptr, 1024, 512, levels)


def plain_frame(state, camera, kind="float", layout=None, **options):
    """one frame of `state` through the plain entry points: "float" float32 [h, w, 4], "rgba8" uint8 [h, w, 4], "yuv420" uint8, "yuv420p10" uint16"""
    metric, prog, cfgv, feats = kerr()
    w, h = state.width, state.height
    opts = gra.frame_options(mode=gra.MODE_FUSED, **options)
    if kind == "yuv420p10":
        out = DeviceBuffer(0, yuv420p10_bytes(w, h))
        state.render_yuv420p10(prog, metric, camera, out.ptr, sky(), feats, cfgv, opts, layout=layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420p10_bytes(w, h),)).copy().view("<u2")
    if kind == "yuv420":
        out = DeviceBuffer(0, yuv420_bytes(w, h))
        state.render_yuv420(prog, metric, camera, out.ptr, sky(), feats, cfgv, opts, layout=layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420_bytes(w, h),))
    out = DeviceBuffer(0, w * h * (4 if kind == "rgba8" else 16))
    (state.render_rgba8 if kind == "rgba8" else state.render)(prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)
    state.synchronize()
    return out.to_numpy(np.uint8 if kind == "rgba8" else np.float32, (h, w, 4))


def subframe(state, camera, weight, first, **options):
    metric, prog, cfgv, feats = kerr()
    state.render_subframe(prog, metric, camera, weight, first, sky(), feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED, **options))


def delivered(state, kind="float", layout=I420):
    """the state's accumulation through gr_deliver_accumulated, in the shapes plain_frame returns"""
    _, prog, _, _ = kerr()
    w, h = state.width, state.height
    if kind == "yuv420p10":
        out = DeviceBuffer(0, yuv420p10_bytes(w, h))
        state.deliver_accumulated(prog, out.ptr, gra.FRAME_YUV420P10, layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420p10_bytes(w, h),)).copy().view("<u2")
    if kind == "yuv420":
        out = DeviceBuffer(0, yuv420_bytes(w, h))
        state.deliver_accumulated(prog, out.ptr, gra.FRAME_YUV420, layout)
        state.synchronize()
        return out.to_numpy(np.uint8, (yuv420_bytes(w, h),))
    out = DeviceBuffer(0, w * h * (4 if kind == "rgba8" else 16))
    state.deliver_accumulated(prog, out.ptr, gra.FRAME_RGBA8 if kind == "rgba8" else gra.FRAME_F32)
    state.synchronize()
    return out.to_numpy(np.uint8 if kind == "rgba8" else np.float32, (h, w, 4))


def every_delivery_is_the_encode_of(state, want):
    """the state's accumulation in all six deliveries against the host definitions applied to the float frame `want` (finite: no NaN rule)"""
    assert np.isfinite(want).all()
    same_bits(delivered(state, "float"), want, "float4")
    rgba8 = encode_srgb8(want)
    assert delivered(state, "rgba8").tobytes() == rgba8.tobytes()
    codes = frame_to_rgb10(want)
    for layout in (I420, NV12):
        assert delivered(state, "yuv420", layout).tobytes() == rgba8_to_yuv420(rgba8, layout).tobytes(), layout
        assert delivered(state, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(codes, layout).astype("<u2").tobytes(), layout
    same_bits(delivered(state, "float"), want, "float4 again: a delivery leaves the accumulation as it is")


@pytest.mark.parametrize("w,h,f", [(64, 36, 1), (66, 38, 2)])
def test_three_subframes_are_the_three_frames_accumulated(w, h, f):
    """rests on schedules never changing a pixel (tests/test_gpu_schedule.py): the sub-frames are consecutive frames of one state, the
    yardstick's are frames of another"""
    cameras = [gra.default_camera(position, quat) for position, quat in CAMERAS]
    weight = np.float32(1) / np.float32(3)
    yardstick = gra.RenderState(w, h, 0, supersample=f)
    frames = [plain_frame(yardstick, camera) for camera in cameras]
    assert frames[0].tobytes() != frames[1].tobytes() != frames[2].tobytes()   # the cameras differ in the picture
    want = None
    for j, fr in enumerate(frames):
        want = step(want, fr, weight, j == 0)
    state = gra.RenderState(w, h, 0, supersample=f)
    for j, camera in enumerate(cameras):
        subframe(state, camera, weight, j == 0, next_camera=ctypes.pointer(cameras[j + 1]) if j + 1 < len(cameras) else None)
    every_delivery_is_the_encode_of(state, want)
    assert len(np.unique(encode_srgb8(want))) > 32
    # a second shutter on the same state starts over (first = 1), with uneven weights and without the look-ahead
    want = None
    for j, (fr, wt) in enumerate(zip(frames[::-1], WEIGHTS[4])):
        want = step(want, fr, wt, j == 0)
    for j, (camera, wt) in enumerate(zip(cameras[::-1], WEIGHTS[4])):
        subframe(state, camera, wt, j == 0)
    same_bits(delivered(state, "float"), want, "second shutter")


@pytest.mark.parametrize("f", [1, 2])
def test_one_subframe_of_weight_one_is_the_plain_frame(f):
    w, h = 64, 36
    camera = gra.default_camera(*CAMERAS[1])
    state = gra.RenderState(w, h, 0, supersample=f)
    subframe(state, camera, 1.0, True, time_kernels=1)
    assert state.resolve_ms() > 0   # the accumulate launch, between the resolve's events
    other = gra.RenderState(w, h, 0, supersample=f)
    assert delivered(state, "float").tobytes() == plain_frame(other, camera).tobytes()
    assert delivered(state, "rgba8").tobytes() == plain_frame(other, camera, "rgba8").tobytes()
    for layout in (I420, NV12):
        assert delivered(state, "yuv420", layout).tobytes() == plain_frame(other, camera, "yuv420", layout).tobytes()
        assert delivered(state, "yuv420p10", layout).tobytes() == plain_frame(other, camera, "yuv420p10", layout).tobytes()


def test_the_geodesic_camera():
    w, h = 64, 36
    metric, prog, cfgv, feats = kerr()
    camera = gra.default_camera([0.0, 0.0, -8.0, 0.0])
    path = gra.GeodesicCamera(device=0)
    steps, tau = path.snapshot(prog, metric, camera, [0.0, 0.3, 0.0], feats, cfgv)
    assert steps > 10 and tau > 2.0
    times = [0.5, 1.5]
    on_the_path = [dict(geodesic=path.handle.value, geodesic_time=t, parallel_transport_observer=1) for t in times]
    yardstick = gra.RenderState(w, h, 0)
    frames = [plain_frame(yardstick, camera, **o) for o in on_the_path]
    assert frames[0].tobytes() != frames[1].tobytes()
    half = np.float32(0.5)
    want = step(step(None, frames[0], half, True), frames[1], half, False)
    state = gra.RenderState(w, h, 0)
    subframe(state, camera, half, True, next_camera=ctypes.pointer(camera), next_geodesic_time=times[1], **on_the_path[0])
    subframe(state, camera, half, False, **on_the_path[1])
    same_bits(delivered(state, "float"), want, "geodesic")


def test_refusals_that_need_a_state():
    w, h = 64, 36
    metric, prog, cfgv, feats = kerr()
    camera = gra.default_camera()
    state = gra.RenderState(w, h, 0)
    out = DeviceBuffer(0, yuv420p10_bytes(w, h) + 16)
    with pytest.raises(gra.GeodesicError, match="gr_render_subframe.*no accumulation"):
        subframe(state, camera, 0.5, False)
    with pytest.raises(gra.GeodesicError, match="gr_deliver_accumulated.*no accumulation"):
        state.deliver_accumulated(prog, out.ptr)
    with pytest.raises(gra.GeodesicError, match="gr_render_subframe.*strip_count"):
        subframe(state, camera, 0.5, True, strip_count=2, strip_rank=0, block_rows=8)
    with pytest.raises(gra.GeodesicError, match="gr_render_subframe.*weight"):
        subframe(state, camera, float("nan"), True)
    with pytest.raises(gra.GeodesicError, match="gr_deliver_accumulated.*no accumulation"):
        state.deliver_accumulated(prog, out.ptr)   # none of the refused calls started one
    subframe(state, camera, 1.0, True)
    for frame_format, offset in ((gra.FRAME_YUV420, 2), (gra.FRAME_YUV420, 1), (gra.FRAME_YUV420P10, 4), (gra.FRAME_YUV420P10, 2)):
        with pytest.raises(gra.GeodesicError, match="gr_deliver_accumulated.*aligned"):
            state.deliver_accumulated(prog, ctypes.c_void_p(out.ptr.value + offset), frame_format)
    with pytest.raises(gra.GeodesicError, match="gr_deliver_accumulated.*format"):
        state.deliver_accumulated(prog, out.ptr, 4)
    with pytest.raises(gra.GeodesicError, match="gr_deliver_accumulated.*layout"):
        state.deliver_accumulated(prog, out.ptr, gra.FRAME_YUV420, 2)
    # the state still renders a plain frame, and it is the frame of a state that was never refused anything
    assert plain_frame(state, camera).tobytes() == plain_frame(gra.RenderState(w, h, 0), camera).tobytes()
    assert delivered(state, "float").tobytes() == plain_frame(state, camera).tobytes()   # and its accumulation is still there


def one_cycle(size, f):
    state = gra.RenderState(size[0], size[1], 0, supersample=f)
    weight = np.float32(1) / np.float32(3)
    for j, (position, quat) in enumerate(CAMERAS):
        subframe(state, gra.default_camera(position, quat), weight, j == 0)
    frame = delivered(state, "yuv420")
    assert frame.size == yuv420_bytes(*size)
    del state
    gc.collect()


def test_the_accumulation_frame_is_freed_with_the_state():
    """tests/test_gpu_lifecycle.py's method: two cycles first (runtime pools, code objects, the sky), then ten between two readings of
    hipMemGetInfo.  A 640 x 360 accumulation frame is 3.5 MiB: one that stayed behind per cycle would show ten times over."""
    one_cycle((640, 360), 1)
    one_cycle((320, 180), 2)
    before = device_bytes_in_use()
    for k in range(10):
        one_cycle((640, 360), 1 if k % 2 else 2)
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


def test_the_cli_writes_the_accumulations_of_the_frames_render_returns(tmp_path):
    """--shutter: the file's frames are the encodes of the plain float frames of the sub-frames' cameras (camera_path_at of shutter_times),
    accumulated on the host with the box weight - for a .y4m, and for a PNG of a supersampled state encoded on the device"""
    w, h, frames, samples = 64, 36, 3, 2
    path = str(tmp_path / "x.y4m")
    pan = ["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", f"{w}x{h}", "--frames", str(frames), "--camera", "0,0,-8,0", "--camera-to", "0,2,-7,0",
           "--shutter", "0.5", "--shutter-samples", str(samples)]
    assert render.main(pan + ["--out", path]) == 0
    moments = render.shutter_times(frames, 0.5, samples)
    assert moments.shape == (frames, samples) and moments[2, 1] == 2.375
    cameras = render.camera_path_at([0, 0, -8, 0], None, [0, 2, -7, 0], None, frames, moments.ravel())
    weight = np.float32(1) / np.float32(samples)

    def accumulated(plain):
        assert len(plain) == frames * samples
        out = []
        for k in range(frames):
            total = None
            for j in range(samples):
                total = step(total, plain[k * samples + j], weight, j == 0)
            out.append(total)
        return out

    want = accumulated(render.render("kerr_boyer", w, h, cfg={"a": 0.45}, cameras=cameras))
    assert want[0].tobytes() != want[2].tobytes()
    blob = open(path, "rb").read()
    header = b"YUV4MPEG2 W64 H36 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert blob == header + b"".join(b"FRAME\n" + rgba8_to_yuv420(encode_srgb8(fr)).tobytes() for fr in want)
    # render() itself, as float4 and as 10-bit words
    got = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, cameras=cameras, shutter_samples=samples)
    assert len(got) == frames and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    deep = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, cameras=cameras, shutter_samples=samples, yuv420=True, bit_depth=10)
    assert all(a.tobytes() == rgb10_to_yuv420p10(frame_to_rgb10(b)).astype("<u2").tobytes() for a, b in zip(deep, want))
    # PNGs of a supersampled state, encoded on the device
    assert render.main(pan + ["--supersample", "2", "--encode", "device", "--out", str(tmp_path / "y.png")]) == 0
    want2 = accumulated(render.render("kerr_boyer", w, h, cfg={"a": 0.45}, cameras=cameras, supersample=2))
    for k in range(frames):
        assert render.read_png(str(tmp_path / f"y_{k:03d}.png")).tobytes() == encode_srgb8(want2[k]).tobytes(), k
