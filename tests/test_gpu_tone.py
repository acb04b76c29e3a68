"""GPU tests (-m gpu) of the meter and the tone curve: gr_meter_frame (kernels/tone.hip) against the host histogram, exactly - one pixel,
sizes either side of a wave, of the workgroup's tile of 1024 pixels and of one stride of the 1024-workgroup grid, a frame of one value
(90 000 in one counter), a black frame, the bin edges - between guard words; gr_meter_solve_device against the host solve bit for bit;
gr_apply_tone against gr_tone_frame bit for bit, three curves, in place and out of place, between guard bands, the gain from the device
word and from the argument block.  Whole frames of a state with a tone in every format against the format's host encode of gr_tone_frame
of the frame the same state delivers without it, with the gain of the host solve of the host histogram of that frame: over a star sky and
a sky image, without and with a glare, supersampled through the Mitchell filter, four sub-frames, set / cleared / set again, a five-frame
adaptation, the refusals, device memory over ten cycles, the CLI's file.  Kerr (scripts/kerr_boyer.js), a = 0.45, the substituted program."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib, render  # noqa: E402
from geodesic_raytracing_amd.pipeline import (DeviceBuffer, apply_tone, encode_srgb8, frame_to_rgb10, glare_frame, glare_gaussians, meter_frame,  # noqa: E402
                                              meter_histogram, meter_solve, meter_solve_device, rgb10_to_yuv420p10, rgba8_to_yuv420, tone_frame,
                                              yuv420_bytes)
import tone_model as tm  # noqa: E402
from test_gpu_lifecycle import MiB, device_bytes_in_use  # noqa: E402
from test_gpu_shutter import CAMERAS, delivered, kerr, plain_frame, same_bits, sky, subframe  # noqa: E402

GUARD = 16                       # words either side of the 385 counters; float4 either side of a toned frame
GUARD_WORD = 0xA5A55A5A
GUARD_VALUE = np.float32(-777.25)
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
# one pixel; 63, 64, 65: either side of a wave; 255 x 1 and 257 x 3: of the 256 lanes; 1023 and 1025: of the workgroup's tile of 1024 pixels;
# 1024 x 1024 - 1 and + 1: of one stride of the grid (1024 workgroups x 1024 pixels), where a workgroup starts its second trip
SHAPES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (257, 3), (1000, 7), (513, 129), (1023, 1), (1025, 1), (1048575, 1), (1048577, 1)]
TONE_SHAPES = SHAPES[:10]
_shared = {}


def metered(frame):
    """gr_meter_frame of the host array `frame` into 385 counters between guard words that hold something else beforehand"""
    _, prog, _, _ = kerr()
    h, w = frame.shape[:2]
    words = np.full(385 + 2 * GUARD, GUARD_WORD, dtype=np.uint32)
    words[GUARD:GUARD + 385] = 123456789   # (the launcher zeroes the counters itself)
    dhist = DeviceBuffer.from_numpy(0, words)
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(frame, dtype=np.float32))
    meter_frame(prog, dsrc.ptr, w, h, ctypes.c_void_p(dhist.ptr.value + 4 * GUARD))
    check(lib.gr_device_synchronize(0))
    back = dhist.to_numpy(np.uint32, (385 + 2 * GUARD,))
    assert (back[:GUARD] == GUARD_WORD).all() and (back[GUARD + 385:] == GUARD_WORD).all(), "guard words were written"
    return back[GUARD:GUARD + 385].copy()


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_meter_alone_equals_the_host_histogram(w, h):
    frame = tm.random_frame(w, h, 1000 + w % 9973 + h)
    got, want = metered(frame), meter_histogram(frame)
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], int(got.sum()), w * h)
    assert int(got.sum()) == w * h


def test_a_frame_of_one_value_a_black_frame_and_the_edges():
    one = np.full((300, 300, 4), np.float32(0.37), dtype=np.float32)
    got = metered(one)
    assert np.array_equal(got, meter_histogram(one)) and got.max() == 90000 and (got > 0).sum() == 1 and got[384] == 0   # above a 16-bit counter
    black = np.zeros((300, 300, 4), dtype=np.float32)
    black[..., 3] = 1
    black[7, 9, :3] = -0.0
    got = metered(black)
    assert got[384] == 90000 and got[:384].sum() == 0
    # two values a wave, as a star frame has them, and three
    stars = black.copy()
    stars[::3, ::2, :3] = 0.02
    stars[5::17, 1::13, :3] = 350.0
    assert np.array_equal(metered(stars), meter_histogram(stars))
    edges = tm.edge_frame()
    got = metered(edges)
    assert np.array_equal(got, meter_histogram(edges)) and np.array_equal(got, tm.histogram(edges)) and (got > 0).all()


def solved(hist, tone, adapted, primed):
    """gr_meter_solve_device on uploaded counters and an uploaded state -> (adapted, primed, gain, q)"""
    _, prog, _, _ = kerr()
    state = gra.ToneStateStruct(adapted, 1 if primed else 0, 12345, -1.0, 777)
    dstate = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(state), dtype=np.uint8))
    dhist = DeviceBuffer.from_numpy(0, np.ascontiguousarray(hist, dtype=np.uint32))
    meter_solve_device(prog, dhist.ptr, tone, dstate.ptr)
    check(lib.gr_device_synchronize(0))
    back = gra.ToneStateStruct.from_buffer_copy(dstate.to_numpy(np.uint8, (24,)).tobytes())
    assert np.array_equal(dhist.to_numpy(np.uint32, (385,)), hist) and back.reserved == 777
    return back.adapted, bool(back.primed), np.float32(back.gain), back.q


def same_solution(got, want, what):
    assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes() and got[1] == want[1], (what, got, want)
    assert tm.bits(got[2]) == tm.bits(want[2]) and got[3] == want[3], (what, got, want)


def test_the_solve_on_the_device_is_the_host_solve():
    for name, (hist, tone, adapted, primed) in tm.solve_cases().items():
        same_solution(solved(hist, tone, adapted, primed), meter_solve(hist, tone, adapted, primed), name)
    for rate in (1.0, 0.5, 2.0 ** -6):
        tone = gra.tone(auto=True, rate=rate, low=0.25, high=0.9)
        device, host = (0.0, False), (0.0, False)
        for k, hist in enumerate(tm.sequence(20)):
            got, want = solved(hist, tone, *device), meter_solve(hist, tone, *host)
            same_solution(got, want, (rate, k))
            device, host = got[:2], want[:2]


def toned_on_device(frame, tone, gain, in_place, from_device_word):
    """gr_apply_tone of the host array `frame` between guard bands; the gain from a device word or from the argument block"""
    _, prog, _, _ = kerr()
    h, w = frame.shape[:2]
    buf = np.full((w * h + 2 * GUARD, 4), GUARD_VALUE, dtype=np.float32)
    if in_place:
        buf[GUARD:GUARD + w * h] = frame.reshape(-1, 4)
    else:
        buf[GUARD:GUARD + w * h] = np.nan
    ddst = DeviceBuffer.from_numpy(0, buf)
    dst = ctypes.c_void_p(ddst.ptr.value + GUARD * 16)
    dsrc = None if in_place else DeviceBuffer.from_numpy(0, np.ascontiguousarray(frame, dtype=np.float32))
    state = gra.ToneStateStruct(0.0, 1, 0, float(gain), 0)
    dstate = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(state), dtype=np.uint8))
    gain_ptr = ctypes.c_void_p(dstate.ptr.value + gra.ToneStateStruct.gain.offset) if from_device_word else None
    apply_tone(prog, dst if in_place else dsrc.ptr, dst, w, h, tone, gain_ptr, 55.0 if from_device_word else float(gain))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.float32, (w * h + 2 * GUARD, 4))
    assert (tm.bits(back[:GUARD]) == tm.bits(GUARD_VALUE)).all() and (tm.bits(back[GUARD + w * h:]) == tm.bits(GUARD_VALUE)).all(), "guard bands were written"
    if dsrc is not None:
        assert dsrc.to_numpy(np.float32, frame.shape).tobytes() == np.ascontiguousarray(frame, dtype=np.float32).tobytes()
    return back[GUARD:GUARD + w * h].reshape(h, w, 4).copy()


@pytest.mark.parametrize("w,h", TONE_SHAPES)
def test_the_curves_on_the_device_are_the_host_curves(w, h):
    frame = tm.colours(w, h, 500 + 3 * w + h)
    for k, (name, curve) in enumerate(tm.CURVES.items()):
        tone = gra.tone(curve=curve, white=(4.0, 0.37, 4.0)[k])
        gain = np.float32(2.0 ** ((-37, 75, 3)[k] / 16.0))
        want = tone_frame(frame, tone, gain)
        for in_place in (False, True):
            got = toned_on_device(frame, tone, gain, in_place, from_device_word=(k + in_place) % 2 == 0)
            assert tm.same_frame(got, want), (name, in_place, int((tm.bits(got) != tm.bits(want)).sum()))
    assert tm.same_frame(want, tm.toned(frame, gain, curve, 4.0))


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
W, H = 96, 54


def star_sky():
    if "stars" not in _shared:
        _, prog, _, _ = kerr()
        _shared["stars"] = render.parse_sky("stars:2000:7").on(prog)
    return _shared["stars"]


def state_of(f=1, filter="box", with_stars=True, **more):
    return gra.RenderState(W, H, 0, supersample=f, filter=filter, stars=star_sky() if with_stars else None, **more)


def expected(plain, tone, adapted=0.0, primed=False):
    """(the frame a state with `tone` delivers of `plain`, the state after it): the host statements, one after the other"""
    solution = meter_solve(meter_histogram(plain), tone, adapted, primed)
    return tone_frame(plain, tone, solution[2]), solution


def every_format_is_the_encode_of(state, camera, want):
    """(a state whose rate is 1: every delivery meters the same frame to the same gain)"""
    rgba8, codes = encode_srgb8(want), frame_to_rgb10(want)
    assert plain_frame(state, camera, "rgba8").tobytes() == rgba8.tobytes()
    for layout in (I420, NV12):
        assert plain_frame(state, camera, "yuv420", layout).tobytes() == rgba8_to_yuv420(rgba8, layout).tobytes(), layout
        assert plain_frame(state, camera, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(codes, layout).astype("<u2").tobytes(), layout
    same_bits(plain_frame(state, camera), want, "float4 after the encodes")


@pytest.mark.parametrize("with_stars", [True, False])
@pytest.mark.parametrize("with_glare", [False, True])
def test_every_format_is_the_encode_of_the_tone_of_the_plain_frame(with_stars, with_glare):
    camera = gra.default_camera(*CAMERAS[1])
    g = glare_gaussians([1.5, 4.0], [0.06, 0.03])
    for tone in (gra.tone(auto=True, curve="filmic"), gra.tone(auto=True, curve="reinhard", white=3.0, low=0.2, high=0.95, key_stops=-1.5), gra.tone(stops=1.3125, curve="reinhard")):
        state = state_of(with_stars=with_stars)
        assert state.tone is None
        plain = plain_frame(state, camera)
        assert np.isfinite(plain).all() and len(np.unique(plain[..., :3])) > 10
        if with_glare:
            state.set_glare(g)
            plain = glare_frame(plain, g)
        state.set_tone(tone)
        assert bytes(state.tone) == bytes(tone)
        want, solution = expected(plain, tone)
        same_bits(plain_frame(state, camera, time_kernels=1), want, (with_stars, with_glare, tone.mode))
        assert state.resolve_ms() > 0   # the meter, the solve and the curve lie between the resolve's events
        stops, gain = state.exposure()
        assert tm.bits(np.float32(gain)) == tm.bits(solution[2]) and stops == solution[3] / 16.0
        every_format_is_the_encode_of(state, camera, want)
        assert (tm.bits(want) != tm.bits(plain)).any()


def test_supersampled_through_the_mitchell_filter_and_four_subframes():
    camera = gra.default_camera(*CAMERAS[1])
    tone = gra.tone(auto=True, curve="filmic")
    state = state_of(2, "mitchell")
    plain = plain_frame(state, camera)
    state.set_tone(tone)
    want, _ = expected(plain, tone)
    same_bits(plain_frame(state, camera), want, "supersample 2, mitchell")
    every_format_is_the_encode_of(state, camera, want)
    # four sub-frames accumulate untoned; the delivery meters and tones the accumulation once, after its glare
    g = glare_gaussians([1.5], [0.1])
    state = state_of(2)
    state.set_glare(g)
    state.set_tone(tone)
    poses = CAMERAS + [([0.0, 0.75, -7.8, 0.3], None)]
    for j, (position, quat) in enumerate(poses):
        subframe(state, gra.default_camera(position, quat), np.float32(0.25), j == 0)
    with_tone, with_tone8 = delivered(state, "float"), delivered(state, "rgba8")
    state.set_tone(None)
    state.set_glare(None)
    accumulation = delivered(state, "float")
    want, _ = expected(glare_frame(accumulation, g), tone)
    same_bits(with_tone, want, "the tone of the glare of the accumulation")
    assert with_tone8.tobytes() == encode_srgb8(want).tobytes()
    state.set_glare(g)
    state.set_tone(tone)
    for layout in (I420, NV12):
        assert delivered(state, "yuv420", layout).tobytes() == rgba8_to_yuv420(encode_srgb8(want), layout).tobytes()
        assert delivered(state, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(frame_to_rgb10(want), layout).astype("<u2").tobytes()
    state.set_tone(None)
    state.set_glare(None)
    assert delivered(state, "float").tobytes() == accumulation.tobytes()


def test_set_cleared_and_set_again_and_a_five_frame_adaptation():
    cameras = [gra.default_camera(*pose) for pose in CAMERAS + [([0.0, 0.75, -7.8, 0.3], None), ([0.0, 1.0, -7.7, 0.4], None)]]
    tone = gra.tone(auto=True, rate=0.5, curve="reinhard")
    untouched, state = state_of(), state_of()
    plains = [plain_frame(untouched, camera) for camera in cameras]
    state.set_tone(tone)
    adapted, primed = 0.0, False
    seen = []
    for k, camera in enumerate(cameras):   # the host recursion, frame by frame
        want, solution = expected(plains[k], tone, adapted, primed)
        same_bits(plain_frame(state, camera), want, f"frame {k}")
        assert state.exposure()[0] == solution[3] / 16.0
        adapted, primed = solution[:2]
        seen.append(adapted)
    assert len(set(seen)) > 1
    # cleared: the untoned state's frames, bit for bit, and a factor-1 box state renders straight into `out` again
    state.set_tone(None)
    assert state.tone is None
    assert plain_frame(state, cameras[0], time_kernels=1).tobytes() == plains[0].tobytes() and not state.resolve_ms() > 0
    assert plain_frame(state, cameras[0], "rgba8").tobytes() == plain_frame(untouched, cameras[0], "rgba8").tobytes()
    # set again: the adaptation starts again
    state.set_tone(tone)
    want, solution = expected(plains[3], tone)
    same_bits(plain_frame(state, cameras[3]), want, "set again")
    assert solution[0] != adapted


def test_split_frames_refuse_a_state_with_a_tone():
    metric, prog, cfgv, feats = kerr()
    camera = gra.default_camera(*CAMERAS[1])
    out = DeviceBuffer(0, W * H * 16)
    tone = gra.tone(auto=True)
    for f in (1, 2):
        state = state_of(f, with_stars=False)
        plain = plain_frame(state, camera)
        state.set_tone(tone)
        for kind in ("float", "rgba8"):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame.*tone.*strip_count.*histogram"):
                plain_frame(state, camera, kind, strip_count=2, strip_rank=0, block_rows=8)
        (part,) = gra.TiledFrame.local([0], W, H, 8)
        opts = gra.frame_options(mode=gra.MODE_FUSED)
        if f == 1:
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled:.*tone.*histogram"):
                part.render(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)
        for rgba8 in (False, True):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled_as:.*tone.*histogram"):
                part.render_as(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts, rgba8=rgba8)
        same_bits(plain_frame(state, camera), expected(plain, tone)[0], "after the refusals")
        part.close()
    bad = gra.tone(auto=True)
    bad.low = 0.99
    with pytest.raises(gra.GeodesicError, match="gr_render_state_set_tone.*low >= high"):
        gra.RenderState(W, H, 0).set_tone(bad)
    with pytest.raises(gra.GeodesicError, match="gr_render_state_exposure.*no tone"):
        gra.RenderState(W, H, 0).exposure()


def one_cycle(size, f, filter):
    state = gra.RenderState(size[0], size[1], 0, supersample=f, filter=filter, tone=gra.tone(auto=True, curve="filmic"))
    camera = gra.default_camera(*CAMERAS[0])
    assert plain_frame(state, camera, "yuv420", I420).size == yuv420_bytes(*size)
    assert plain_frame(state, camera).shape == (size[1], size[0], 4)
    subframe(state, camera, 1.0, True)
    assert delivered(state, "rgba8").shape == (size[1], size[0], 4)
    del state
    gc.collect()


def test_the_tones_memory_is_freed_with_the_state():
    """tests/test_gpu_lifecycle.py's method: two cycles first, then ten between two readings of hipMemGetInfo.  A 640 x 360 float4 frame is
    3.5 MiB and a state with a tone owns one more of them and the meter's words: one that stayed behind per cycle would show ten times over."""
    one_cycle((640, 360), 1, "box")
    one_cycle((320, 180), 2, "mitchell")
    before = device_bytes_in_use()
    for k in range(10):
        one_cycle((640, 360), 1 if k % 2 else 2, "box" if k % 3 else "mitchell")
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


def test_the_cli_writes_a_metered_and_toned_star_frame(tmp_path, capsys):
    base = ["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", f"{W}x{H}", "--camera", "0,0,-8,0", "--sky", "stars:2000:7"]
    png = str(tmp_path / "x.png")
    assert render.main(base + ["--auto-exposure", "--meter", "0.25:0.9", "--tone", "filmic", "--out", png]) == 0
    printed = capsys.readouterr().out
    field = render.parse_sky("stars:2000:7")
    plain = render.render("kerr_boyer", W, H, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], sky=field)
    tone = gra.tone(auto=True, low=0.25, high=0.9, curve="filmic")
    want, solution = expected(plain, tone)
    exposures = []
    got = render.render("kerr_boyer", W, H, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], sky=field, tone=tone, exposures=exposures)
    same_bits(got, want, "render(tone=)")
    assert exposures == [(solution[3] / 16.0, float(solution[2]))] and f"frame 0: exposure {solution[3] / 16.0:+.4f} stops" in printed
    assert render.read_png(png).tobytes() == encode_srgb8(want).tobytes() != encode_srgb8(plain).tobytes()
