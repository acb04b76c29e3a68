"""GPU tests (-m gpu) of the sky's mip slices built on the device: gr_build_mipped_background (kernels/background.hip) against the host
packer that stays the yardstick (gr_pack_mipped_background), byte for byte, out of place and in place, between guard bytes; frames
rendered from a device-built sky on the build's own stream; two skies in one frame; the refusals; the CLI switch; the life cycle.
Kerr (scripts/kerr_boyer.js), a = 0.45."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, build_background, pack_background  # noqa: E402
from test_gpu_fullsize import SCRIPTS  # noqa: E402

GUARD = 256               # bytes either side of the packed buffer and of the scratch
GUARD_BYTE = 0xA5
SENTINEL = 0x5C           # fills a packed buffer before it is built
SIZES = [(1, 1), (5, 1), (2, 2), (3, 2), (37, 19), (19, 70), (64, 33), (1100, 1024)]   # width x height
_shared = {}


def kerr():
    """the dynamic program, shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def random_image(w, h):
    return np.random.RandomState(1000 * w + h).randint(0, 256, size=(h, w, 4)).astype(np.uint8)


def all_bytes_image():
    """16 x 16, every byte value in every channel (each channel in an order of its own)"""
    k = np.arange(256)
    return np.stack([k, (k * 7 + 3) % 256, 255 - k, (k * 13 + 101) % 256], axis=-1).astype(np.uint8).reshape(16, 16, 4)


def host_packed(name, rgba):
    """pack_background of a test image, computed once per image and not written to"""
    if name not in _shared:
        packed, levels = pack_background(rgba)
        packed.setflags(write=False)
        _shared[name] = (packed, levels)
    return _shared[name]


def scratch_bytes(w, h):
    need = ctypes.c_size_t()
    check(lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)))
    return need.value


def built(rgba, in_place, levels):
    """gr_build_mipped_background of `rgba` into a packed buffer between guard bytes, with a scratch between guard bytes; returns the
    packed bytes [levels, h, w, 4] after checking the function's answer and all four guards"""
    _, prog, _ = kerr()
    h, w = rgba.shape[:2]
    n, need = levels * w * h * 4, scratch_bytes(w, h)
    host = np.full(n + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
    host[GUARD:GUARD + n] = SENTINEL
    if in_place:
        host[GUARD:GUARD + w * h * 4] = rgba.reshape(-1)
    dpacked = DeviceBuffer.from_numpy(0, host)
    dscratch = DeviceBuffer.from_numpy(0, np.full(need + 2 * GUARD, GUARD_BYTE, dtype=np.uint8))
    dimage = None if in_place else DeviceBuffer.from_numpy(0, rgba)
    packed_at = ctypes.c_void_p(dpacked.ptr.value + GUARD)
    scratch_at = ctypes.c_void_p(dscratch.ptr.value + GUARD) if need else None
    assert lib.gr_build_mipped_background(prog.handle, None, packed_at if in_place else dimage.ptr, w, h, packed_at, scratch_at, need) == levels, lib.gr_last_error()
    check(lib.gr_device_synchronize(0))
    back = dpacked.to_numpy(np.uint8, (n + 2 * GUARD,))
    assert (back[:GUARD] == GUARD_BYTE).all() and (back[GUARD + n:] == GUARD_BYTE).all(), "guard bytes of the packed buffer were written"
    around = dscratch.to_numpy(np.uint8, (need + 2 * GUARD,))
    assert (around[:GUARD] == GUARD_BYTE).all() and (around[GUARD + need:] == GUARD_BYTE).all(), "guard bytes of the scratch were written"
    return back[GUARD:GUARD + n].reshape(levels, h, w, 4)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_build_equals_the_host_packer(w, h, in_place):
    """random bytes; 1100 x 1024 is the smallest shape that hits the ten-level cap with a last level wider than one texel (two launches of
    the reduction), 37 x 19 and 19 x 70 break the 16-byte alignment of rows and slices, 1 x 1 and 5 x 1 are one level"""
    rgba = random_image(w, h)
    want, levels = host_packed((w, h), rgba)
    assert built(rgba, in_place, levels).tobytes() == want.tobytes()


@pytest.mark.parametrize("in_place", [False, True])
def test_every_byte_value_in_every_channel(in_place):
    rgba = all_bytes_image()
    want, levels = host_packed("all bytes", rgba)
    assert levels == 5 and want[0].tobytes() == rgba.tobytes()
    assert built(rgba, in_place, levels).tobytes() == want.tobytes()


def sky(seed):
    """a 1024 x 512 sky: (image, host-packed slices on the device, levels)"""
    name = ("sky", seed)
    if name not in _shared:
        rgba = gra.synthetic_background(1024, 512, seed=seed)
        packed, levels = pack_background(rgba)
        _shared[name] = (rgba, DeviceBuffer.from_numpy(0, packed), levels)
    return _shared[name]


def kerr_frame(bg1, bg2, levels, stream=None):
    """a 64 x 32 fused Kerr frame from the two skies (device pointers), enqueued on `stream` and downloaded after synchronising it"""
    metric, prog, cfgv = kerr()
    w, h = 64, 32
    state = gra.RenderState(w, h, 0)
    out = DeviceBuffer(0, w * h * 16)
    state.render(prog, metric, gra.default_camera(), out.ptr, ((bg1, bg2), 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                 gra.frame_options(mode=gra.MODE_FUSED), stream)
    check(lib.gr_stream_synchronize(stream))
    return out.to_numpy(np.float32, (h, w, 4))


def test_a_frame_on_the_builds_own_stream_sees_the_built_sky():
    """upload, build and render on one stream of the library's own, nothing synchronised between build and frame: the frame is, bit for
    bit, the one rendered from the host-packed sky"""
    _, prog, _ = kerr()
    rgba, dhost, levels = sky(0x5EED)
    want = kerr_frame(dhost.ptr, dhost.ptr, levels)
    assert np.isfinite(want).all() and want[..., :3].max() > 0.1 and len(np.unique(want)) > 32
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    try:
        dpacked = DeviceBuffer.from_numpy(0, np.full(levels * rgba.nbytes, SENTINEL, dtype=np.uint8))
        check(lib.gr_device_upload(0, dpacked.ptr, rgba.ctypes.data_as(ctypes.c_void_p), rgba.nbytes))   # (blocking: done before the build is enqueued)
        need = scratch_bytes(1024, 512)
        dscratch = DeviceBuffer(0, need)
        assert lib.gr_build_mipped_background(prog.handle, stream, dpacked.ptr, 1024, 512, dpacked.ptr, dscratch.ptr, need) == levels
        got = kerr_frame(dpacked.ptr, dpacked.ptr, levels, stream)
    finally:
        check(lib.gr_stream_destroy(stream))
    assert got.tobytes() == want.tobytes()


def test_two_device_built_skies_in_one_frame():
    _, prog, _ = kerr()
    (rgba1, dhost1, levels), (rgba2, dhost2, _) = sky(0x5EED), sky(0xBEEF)
    assert rgba1.tobytes() != rgba2.tobytes()
    want = kerr_frame(dhost1.ptr, dhost2.ptr, levels)
    assert want.tobytes() != kerr_frame(dhost2.ptr, dhost1.ptr, levels).tobytes()   # (the frame tells the two skies apart)
    (built1, l1), (built2, l2) = build_background(prog, rgba1), build_background(prog, rgba2)
    assert l1 == l2 == levels and built1.nbytes == levels * rgba1.nbytes
    assert kerr_frame(built1.ptr, built2.ptr, levels).tobytes() == want.tobytes()


def test_a_short_scratch_and_partial_overlap_are_refused_and_nothing_is_written():
    _, prog, _ = kerr()
    w, h = 64, 33
    rgba = random_image(w, h)
    levels, need, image_bytes = 6, scratch_bytes(w, h), w * h * 4
    n = levels * image_bytes
    dpacked = DeviceBuffer.from_numpy(0, np.full(n + image_bytes, SENTINEL, dtype=np.uint8))
    dscratch = DeviceBuffer.from_numpy(0, np.full(need, SENTINEL, dtype=np.uint8))
    dimage = DeviceBuffer.from_numpy(0, rgba)
    at = lambda buffer, offset: ctypes.c_void_p(buffer.ptr.value + offset)   # noqa: E731
    for word, args in (("needed", (dimage.ptr, w, h, dpacked.ptr, dscratch.ptr, need - 1)),
                       ("overlap", (at(dpacked, 16), w, h, dpacked.ptr, dscratch.ptr, need)),             # the image inside slice 0, not at its start
                       ("overlap", (at(dpacked, n - 16), w, h, dpacked.ptr, dscratch.ptr, need)),         # the image's start in the last slice
                       ("overlap", (dimage.ptr, w, h, dpacked.ptr, at(dpacked, n - 16), need)),           # scratch on the packed buffer's end
                       ("overlap", (dpacked.ptr, w, h, dpacked.ptr, at(dpacked, image_bytes), need))):    # in place, scratch in slice 1
        assert lib.gr_build_mipped_background(prog.handle, None, *args) == -1, word
        message = lib.gr_last_error()
        assert b"gr_build_mipped_background" in message and word.encode() in message, message
    check(lib.gr_device_synchronize(0))
    assert (dpacked.to_numpy(np.uint8, (n + image_bytes,)) == SENTINEL).all() and (dscratch.to_numpy(np.uint8, (need,)) == SENTINEL).all()
    assert dimage.to_numpy(np.uint8, rgba.shape).tobytes() == rgba.tobytes()


def test_the_cli_writes_the_same_png_either_way(tmp_path):
    from geodesic_raytracing_amd import render
    paths = {}
    for where in ("host", "device"):
        paths[where] = str(tmp_path / f"kerr_{where}.png")
        assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "64x32", "--mips", where, "--out", paths[where]]) == 0
    host, device = open(paths["host"], "rb").read(), open(paths["device"], "rb").read()
    assert len(host) > 1000 and host == device
    assert render.read_png(paths["device"]).shape == (32, 64, 4)


def test_built_skies_give_their_memory_back():
    """ten rounds of build / destroy of a 1024 x 512 sky (20 MiB packed, 2.7 MiB of scratch): device memory in use comes back to where
    it was, within the allowance of tests/test_gpu_lifecycle.py, read as that file reads it"""
    from test_gpu_lifecycle import MiB, device_bytes_in_use
    _, prog, _ = kerr()
    rgba, _, levels = sky(0x5EED)

    def cycle():
        packed, made = build_background(prog, rgba)
        assert made == levels
        del packed
        gc.collect()

    cycle()
    before = device_bytes_in_use()
    for _ in range(10):
        cycle()
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)
