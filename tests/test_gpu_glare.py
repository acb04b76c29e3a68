"""GPU tests (-m gpu) of the glare: gr_apply_glare (kernels/glare.hip) on its own against the host definition gr_glare_frame, bit for bit -
one pixel, frames narrower and lower than the PSF, sizes either side of the kernels' tiles and of a wave; no component, one of 1, 3, 15
and 129 taps, four of mixed lengths, asymmetric tables; between guard bands; with zeros of both signs, infinities and NaN planted.  Whole
frames of a state with a glare in every format against gr_glare_frame of the float4 frame the same state delivers without it and the
host encodes of that, over a star sky and over a sky image, at factors 1 to 4 with the box and the Mitchell filter; star pixels above 1
whose neighbours the glare lights up in 8 bits; a shutter's accumulation; a glare set and cleared against an untouched state; the
refusals; device memory over create / set glare / render / destroy cycles; the CLI's file.  Kerr (scripts/kerr_boyer.js), a = 0.45, the
substituted program."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib, render  # noqa: E402
from geodesic_raytracing_amd.pipeline import (DeviceBuffer, apply_glare, encode_srgb8, frame_to_rgb10, glare_exposure, glare_frame,  # noqa: E402
                                              glare_gaussians, glare_scratch_bytes, rgb10_to_yuv420p10, rgba8_to_yuv420, yuv420_bytes)
from glare_model import UNEVEN7, UNEVEN15, UNEVEN129, bits, make_glare, source  # noqa: E402
from test_gpu_filter import FRAMES  # noqa: E402
from test_gpu_lifecycle import MiB, device_bytes_in_use  # noqa: E402
from test_gpu_shutter import CAMERAS, delivered, kerr, plain_frame, same_bits, sky, subframe  # noqa: E402

GUARD = 64                # float4 either side of the destination and of the scratch
GUARD_VALUE = np.float32(-777.25)
I420, NV12 = gra.YUV420_I420, gra.YUV420_NV12
# one pixel; narrower and lower than any PSF; 15 and 17 columns: either side of gr_glare_columns' 16-wide tile; 63 and 70 rows: either side of
# its 64-row tile; 65 columns: one more than a wave; 130 x 70: several column tiles both ways; 257 columns: one more than gr_glare_rows' 256
SHAPES = [(1, 1), (2, 1), (1, 3), (5, 3), (15, 9), (17, 8), (65, 63), (130, 70), (257, 3)]
_shared = {}


def glares():
    """no component; one of 1, 3, 15 and 129 taps; four of mixed lengths and signs; the asymmetric tables of tests/test_glare_abi.py"""
    return {"gain": make_glare(1.75), "one tap": make_glare(0.5, [0.25], [[2.0]]), "three": make_glare(0.9, [0.1], [[0.25, 0.5, 0.25]]),
            "uneven 15": make_glare(-0.3, [1.5], [UNEVEN15]), "uneven 129": make_glare(0.0, [0.7], [UNEVEN129]),
            "four": make_glare(0.8, [0.3, -0.2, 0.05, 1.0], [UNEVEN7, UNEVEN129, [1.0], UNEVEN15[::-1]]),
            "gaussians": glare_gaussians([1.5, 10.0], [0.06, 0.03])}


def applied(src, g):
    """gr_apply_glare of the host array `src` into a destination between guard bands that holds NaN beforehand, through a scratch between
    guard bands of its own"""
    _, prog, _, _ = kerr()
    h, w = src.shape[:2]
    n = glare_scratch_bytes(w, h)
    assert n == w * h * 16
    buf = np.full((w * h + 2 * GUARD, 4), GUARD_VALUE, dtype=np.float32)
    dscratch = DeviceBuffer.from_numpy(0, buf)
    buf[GUARD:GUARD + w * h] = np.nan
    ddst = DeviceBuffer.from_numpy(0, buf)
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    apply_glare(prog, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD * 16), ctypes.c_void_p(dscratch.ptr.value + GUARD * 16), n, w, h, g)
    check(lib.gr_device_synchronize(0))
    back, scratch = ddst.to_numpy(np.float32, (w * h + 2 * GUARD, 4)), dscratch.to_numpy(np.float32, (w * h + 2 * GUARD, 4))
    for band in (back[:GUARD], back[GUARD + w * h:], scratch[:GUARD], scratch[GUARD + w * h:]):
        assert (bits(band) == bits(GUARD_VALUE)).all(), "guard bands were written"
    assert dsrc.to_numpy(np.float32, src.shape).tobytes() == np.ascontiguousarray(src, dtype=np.float32).tobytes()   # the source is read only
    return back[GUARD:GUARD + w * h].reshape(h, w, 4).copy()


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_launcher_alone_equals_the_definition(w, h):
    finite = numbers = 0
    src = source(w, h, 1000 + 10 * w + h, planted=True)
    src[h // 2, w // 2, 3] = np.nan                 # alpha passes bit for bit, whatever it holds
    calm = src.copy()                               # under 129 taps one NaN or infinity covers a frame of these sizes: the wide tables get none
    calm[..., :3][~np.isfinite(calm[..., :3])] = 2.5
    for name, g in glares().items():
        frame = calm if max(g.taps[:]) > 15 else src
        with np.errstate(all="ignore"):
            want = glare_frame(frame, g)
        got = applied(frame, g)
        same_bits(got, want, name)
        assert np.array_equal(bits(got[..., 3]), bits(frame[..., 3])), name
        finite, numbers = finite + int(np.isfinite(want).sum()), numbers + want.size
    assert finite > numbers // 2                    # most of what was compared are numbers
    # core 1 with no component is the identity on bit patterns, the sign of a zero included
    got = applied(src, make_glare(1.0))
    same_bits(got, src, "identity")
    assert (bits(got)[src == 0] == bits(src)[src == 0]).all()


def test_the_launchers_refusals():
    _, prog, _, _ = kerr()
    src, dst, scratch = DeviceBuffer(0, 4 * 4 * 16), DeviceBuffer(0, 4 * 4 * 16), DeviceBuffer(0, 4 * 4 * 16 + 16)
    good, bad = make_glare(0.5, [0.5], [[0.25, 0.5, 0.25]]), make_glare(0.5, [0.5], [[0.25, np.nan, 0.25]])
    n = 4 * 4 * 16
    off = ctypes.c_void_p(scratch.ptr.value + 4)
    for args in ((None, dst.ptr, scratch.ptr, n, 4, 4, good), (src.ptr, None, scratch.ptr, n, 4, 4, good), (src.ptr, dst.ptr, None, n, 4, 4, good),
                 (src.ptr, dst.ptr, scratch.ptr, n, 0, 4, good), (src.ptr, dst.ptr, scratch.ptr, n - 16, 4, 4, good), (src.ptr, dst.ptr, off, n, 4, 4, good),
                 (src.ptr, src.ptr, scratch.ptr, n, 4, 4, good), (src.ptr, dst.ptr, dst.ptr, n, 4, 4, good), (src.ptr, dst.ptr, src.ptr, n, 4, 4, good),
                 (src.ptr, dst.ptr, scratch.ptr, n, 4, 4, bad)):
        with pytest.raises(gra.GeodesicError, match="gr_apply_glare"):
            apply_glare(prog, *args)
    apply_glare(prog, src.ptr, dst.ptr, scratch.ptr, n, 4, 4, good)
    check(lib.gr_device_synchronize(0))


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
# a few thousand generated stars; the generator's fluxes suit a 4K pixel and a pixel of these frames covers a few thousand times the sky, so
# they are scaled until the brighter stars stand far above 1, as lensed stars of a 4K frame do
STARS, SEED, BRIGHTER = 4000, 9, 1.0e5


def two_gaussians():
    return glare_gaussians([1.5, 4.0], [0.06, 0.03])


def stars():
    """(StarSky, catalogue) on the shared program's device, built once"""
    if "stars" not in _shared:
        _, prog, _, _ = kerr()
        uv, flux = gra.star_field_random(SEED, STARS)
        _shared["stars"] = (gra.StarSky(min_footprint=2.0 ** -16, background=np.array([[0.0, 0.0, 0.02], [0.0, 0.0, 0.02]], dtype=np.float32)),
                            gra.StarCatalogue(prog, uv, flux * np.float32(BRIGHTER), 64, 32))
    return _shared["stars"]


def state_of(w, h, f=1, filter="box", with_stars=True):
    star_sky, catalogue = stars()
    return gra.RenderState(w, h, 0, supersample=f, filter=filter, stars=(star_sky, catalogue, catalogue) if with_stars else None)


def every_format_is_the_encode_of(state, camera, want):
    rgba8, codes = encode_srgb8(want), frame_to_rgb10(want)
    assert plain_frame(state, camera, "rgba8").tobytes() == rgba8.tobytes()
    for layout in (I420, NV12):
        assert plain_frame(state, camera, "yuv420", layout).tobytes() == rgba8_to_yuv420(rgba8, layout).tobytes(), layout
        assert plain_frame(state, camera, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(codes, layout).astype("<u2").tobytes(), layout
    same_bits(plain_frame(state, camera), want, "float4 after the encodes")


@pytest.mark.parametrize("filter", ["box", "mitchell"])
@pytest.mark.parametrize("w,h,f", FRAMES)
def test_every_format_is_the_encode_of_the_glare_of_the_plain_frame(w, h, f, filter):
    camera = gra.default_camera(*CAMERAS[1])
    g = two_gaussians()
    state = state_of(w, h, f, filter)
    assert state.glare is None
    plain = plain_frame(state, camera)
    assert np.isfinite(plain).all() and len(np.unique(plain[..., :3])) > 100   # a picture: stars are seen
    state.set_glare(g)
    assert bytes(state.glare) == bytes(g)
    want = glare_frame(plain, g)
    same_bits(plain_frame(state, camera, time_kernels=1), want, (f, filter))
    assert state.resolve_ms() > 0   # the resolve and the glare's launches, between the resolve's events
    every_format_is_the_encode_of(state, camera, want)
    assert (bits(want) != bits(plain)).mean() > 0.25   # (the glare changed the picture)


def test_a_frame_over_a_sky_image():
    w, h, f = FRAMES[0]
    camera = gra.default_camera(*CAMERAS[1])
    g = glare_exposure(two_gaussians(), -1.0)
    for factor, filter in ((1, "box"), (f, "mitchell")):
        state = state_of(w, h, factor, filter, with_stars=False)
        plain = plain_frame(state, camera)
        state.set_glare(g)
        every_format_is_the_encode_of(state, camera, glare_frame(plain, g))


def test_a_star_above_one_lights_its_neighbours_in_eight_bits():
    """the visible point of the feature: values above 1 clamp in RGBA8, so without a glare a star of 1 and one of 400 are the same white
    pixel; with one, the brighter star's neighbours are brighter"""
    w, h = 96, 54
    camera = gra.default_camera(*CAMERAS[0])
    state = state_of(w, h)
    plain = plain_frame(state, camera)
    plain8 = plain_frame(state, camera, "rgba8")
    peak = plain[1:-1, 1:-1, :3].max(axis=2)
    print(f"star frame {w}x{h}: max {plain[..., :3].max():.1f}, {(plain[..., :3].max(axis=2) > 1).sum()} pixels above 1")
    assert (peak > 1).sum() >= 1, "no star pixel above 1: choose another count or seed"
    y, x = np.unravel_index(np.argmax(peak), peak.shape)
    y, x = y + 1, x + 1
    state.set_glare(two_gaussians())
    glared8 = plain_frame(state, camera, "rgba8")
    assert glared8.tobytes() == encode_srgb8(glare_frame(plain, two_gaussians())).tobytes()
    ring = np.ones((3, 3), dtype=bool)
    ring[1, 1] = False
    before = plain8[y - 1:y + 2, x - 1:x + 2, :3].astype(np.int64)[ring]
    after = glared8[y - 1:y + 2, x - 1:x + 2, :3].astype(np.int64)[ring]
    print(f"brightest star {plain[y, x, :3]} at ({x}, {y}): neighbours' bytes {before.sum()} -> {after.sum()}")
    assert after.sum() > before.sum()


def test_a_shutters_accumulation_is_glared_once_at_delivery():
    w, h, f = 66, 38, 2
    g = two_gaussians()
    weight = np.float32(0.25)
    state = state_of(w, h, f)
    state.set_glare(g)
    poses = CAMERAS + [([0.0, 0.75, -7.8, 0.3], None)]
    for j, (position, quat) in enumerate(poses):
        subframe(state, gra.default_camera(position, quat), weight, j == 0)
    with_glare = delivered(state, "float")
    with_glare8 = delivered(state, "rgba8")
    state.set_glare(None)
    accumulation = delivered(state, "float")
    want = glare_frame(accumulation, g)
    same_bits(with_glare, want, "the glare of the accumulation")
    assert with_glare8.tobytes() == encode_srgb8(want).tobytes()
    # ... which is the accumulation of the four frames without a glare, and stays as it is
    yardstick = state_of(w, h, f)
    for j, (position, quat) in enumerate(poses):
        subframe(yardstick, gra.default_camera(position, quat), weight, j == 0)
    assert delivered(yardstick, "float").tobytes() == accumulation.tobytes()
    state.set_glare(g)
    for layout in (I420, NV12):
        assert delivered(state, "yuv420", layout).tobytes() == rgba8_to_yuv420(encode_srgb8(want), layout).tobytes()
        assert delivered(state, "yuv420p10", layout).tobytes() == rgb10_to_yuv420p10(frame_to_rgb10(want), layout).astype("<u2").tobytes()
    state.set_glare(None)
    assert delivered(state, "float").tobytes() == accumulation.tobytes()


@pytest.mark.parametrize("f", [1, 2])
def test_a_glare_set_and_cleared_is_an_untouched_state(f):
    w, h = 48, 24
    camera = gra.default_camera(*CAMERAS[1])
    untouched, cleared = state_of(w, h, f), state_of(w, h, f)
    cleared.set_glare(two_gaussians())
    assert plain_frame(cleared, camera, time_kernels=1).shape == (h, w, 4) and cleared.resolve_ms() > 0
    cleared.set_glare(None)
    assert cleared.glare is None and untouched.glare is None
    assert plain_frame(cleared, camera, time_kernels=1).tobytes() == plain_frame(untouched, camera, time_kernels=1).tobytes()
    assert (cleared.resolve_ms() > 0) == (untouched.resolve_ms() > 0) == (f > 1)   # a factor-1 box state renders straight into `out` again
    assert plain_frame(cleared, camera, "rgba8").tobytes() == plain_frame(untouched, camera, "rgba8").tobytes()
    for layout in (I420, NV12):
        assert plain_frame(cleared, camera, "yuv420", layout).tobytes() == plain_frame(untouched, camera, "yuv420", layout).tobytes()
        assert plain_frame(cleared, camera, "yuv420p10", layout).tobytes() == plain_frame(untouched, camera, "yuv420p10", layout).tobytes()
    subframe(cleared, camera, 1.0, True)
    subframe(untouched, camera, 1.0, True)
    assert delivered(cleared, "float").tobytes() == delivered(untouched, "float").tobytes()


def test_split_frames_refuse_a_state_with_a_glare():
    w, h = 48, 24
    metric, prog, cfgv, feats = kerr()
    camera = gra.default_camera(*CAMERAS[1])
    out = DeviceBuffer(0, w * h * 16)
    g = two_gaussians()
    for f in (1, 2):
        state = state_of(w, h, f, with_stars=False)
        plain = plain_frame(state, camera)
        state.set_glare(g)
        for kind in ("float", "rgba8"):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame.*glare.*strip_count.*PSF"):
                plain_frame(state, camera, kind, strip_count=2, strip_rank=0, block_rows=8)
        (part,) = gra.TiledFrame.local([0], w, h, 8)
        opts = gra.frame_options(mode=gra.MODE_FUSED)
        if f == 1:
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled:.*glare.*PSF"):
                part.render(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)
        for rgba8 in (False, True):
            with pytest.raises(gra.GeodesicError, match="gr_render_frame_tiled_as:.*glare.*PSF"):
                part.render_as(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts, rgba8=rgba8)
        same_bits(plain_frame(state, camera), glare_frame(plain, g), "after the refusals")
        state.set_glare(None)
        part.render_as(state, prog, metric, camera, out.ptr, sky(), feats, cfgv, opts)   # without a glare the state is taken
        state.synchronize()
        part.close()
    bad = make_glare(1.0, [0.5], [[0.5, 0.5]])
    with pytest.raises(gra.GeodesicError, match=r"gr_render_state_set_glare.*taps\[0\]"):
        gra.RenderState(w, h, 0).set_glare(bad)


def one_cycle(size, f, filter):
    state = gra.RenderState(size[0], size[1], 0, supersample=f, filter=filter)
    state.set_glare(two_gaussians())
    camera = gra.default_camera(*CAMERAS[0])
    assert plain_frame(state, camera, "yuv420", I420).size == yuv420_bytes(*size)
    assert plain_frame(state, camera).shape == (size[1], size[0], 4)
    subframe(state, camera, 1.0, True)
    assert delivered(state, "rgba8").shape == (size[1], size[0], 4)
    del state
    gc.collect()


def test_the_glares_frames_are_freed_with_the_state():
    """tests/test_gpu_lifecycle.py's method: two cycles first (runtime pools, code objects, the sky), then ten between two readings of
    hipMemGetInfo.  A 640 x 360 float4 frame is 3.5 MiB and a state with a glare owns up to three more of them: one that stayed behind per
    cycle would show ten times over."""
    one_cycle((640, 360), 1, "box")
    one_cycle((320, 180), 2, "mitchell")
    before = device_bytes_in_use()
    for k in range(10):
        one_cycle((640, 360), 1 if k % 2 else 2, "box" if k % 3 else "mitchell")
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


def test_the_cli_writes_a_glared_star_frame(tmp_path):
    """--sky stars:20000:7 --glare 0.06:1.5,0.03:10 --exposure 1: the PNG holds the encode of gr_glare_frame of the frame render() returns
    without the two switches"""
    w, h = 96, 54
    base = ["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", f"{w}x{h}", "--camera", "0,0,-8,0", "--sky", "stars:20000:7"]
    png = str(tmp_path / "x.png")
    assert render.main(base + ["--glare", "0.06:1.5,0.03:10", "--exposure", "1", "--out", png]) == 0
    field = render.parse_sky("stars:20000:7")
    plain = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], sky=field)
    g = glare_exposure(glare_gaussians([1.5, 10.0], [0.06, 0.03]), 1.0)
    want = glare_frame(plain, g)
    got = render.render("kerr_boyer", w, h, cfg={"a": 0.45}, camera_pos=[0, 0, -8, 0], sky=field, glare=[(0.06, 1.5), (0.03, 10.0)], exposure=1.0)
    same_bits(got, want, "render(glare=, exposure=)")
    assert render.read_png(png).tobytes() == encode_srgb8(want).tobytes()
    assert render.read_png(png).tobytes() != encode_srgb8(plain).tobytes()
    # on the device too, and the exposure alone
    assert render.main(base + ["--exposure", "-1", "--encode", "device", "--out", png]) == 0
    assert render.read_png(png).tobytes() == encode_srgb8(glare_frame(plain, glare_exposure(glare_gaussians(), -1.0))).tobytes()
