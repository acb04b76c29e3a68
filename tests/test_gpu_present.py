"""GPU tests (-m gpu) of 8-bit sRGB frames encoded on the device: gr_present_rgba8 (kernels/present.hip) on its own against the host encode
(gr_frame_to_rgba8) of the same values and of gr_resolve_supersampled's output, byte for byte; strips of it; whole frames of
gr_render_frame_rgba8 against the host encode of gr_render_frame's; a state used for both; the objects' life cycle, the pinned download
and the CLI switch.  Kerr (scripts/kerr_boyer.js), a = 0.45."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer, encode_srgb8  # noqa: E402
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

GUARD = 256               # bytes either side of a destination
GUARD_BYTE = 0xA5
SENTINEL = 0x5C           # fills a destination whose rows are not all written
SENTINEL_FLOAT = np.full(4, SENTINEL, dtype=np.uint8).view(np.float32)[0]   # the float of four such bytes (finite)
ONE = 0x3f800000
_shared = {}


def kerr():
    """the dynamic program (adaptive sampling is one of its run-time features), shared by every test of this file"""
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


def present(src, w, h, f, block_rows=0, rank=0, count=1, compact=0, fill=None):
    """gr_present_rgba8 of the host array `src` (float4, traced size) into w x h x 4 bytes between guard bytes; returns the destination
    (prefilled with `fill` when given) as uint8 [h, w, 4] after checking the guards"""
    _, prog, _ = kerr()
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    host = np.full(w * h * 4 + 2 * GUARD, GUARD_BYTE, dtype=np.uint8)
    if fill is not None:
        host[GUARD:GUARD + w * h * 4] = fill
    ddst = DeviceBuffer.from_numpy(0, host)
    check(lib.gr_present_rgba8(prog.handle, None, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD), w, h, f, block_rows, rank, count, compact))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.uint8, (w * h * 4 + 2 * GUARD,))
    assert (back[:GUARD] == GUARD_BYTE).all() and (back[GUARD + w * h * 4:] == GUARD_BYTE).all(), "guard bytes were written"
    return back[GUARD:GUARD + w * h * 4].reshape(h, w, 4)


def resolved(src, w, h, f):
    """gr_resolve_supersampled of the same source, downloaded"""
    _, prog, _ = kerr()
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    ddst = DeviceBuffer(0, w * h * 16)
    check(lib.gr_resolve_supersampled(prog.handle, None, dsrc.ptr, ddst.ptr, w, h, f, 0, 0, 1, 0))
    check(lib.gr_device_synchronize(0))
    return ddst.to_numpy(np.float32, (h, w, 4))


def edge_values(w, h, seed):
    """frames of w * h * 4 floats that between them hold every finite threshold and its +-1 and +-2 ulp neighbours and what lies outside
    [0, 1] - at most half of a frame, as many frames as that takes - and random bit patterns of [0, 1] for the rest; shuffled, so that
    every channel and lane position meets some of each"""
    rs = np.random.RandomState(seed)
    t = thresholds()
    finite = t[np.isfinite(t)].view(np.uint32).astype(np.int64)
    near = (finite[:, None] + np.arange(-2, 3)[None, :]).reshape(-1)
    near = near[(near >= 0) & (near <= ONE + 2)].astype(np.uint32).view(np.float32)
    tiny = np.finfo(np.float32).tiny
    odd = np.array([-0.0, -1e-30, -0.5, -3.0, -np.inf, 1e-45, tiny / 2, tiny, 1.0000001, 1.25, 1.5, 2.0, np.inf], dtype=np.float32)
    n = w * h * 4
    special = rs.permutation(np.concatenate([odd, near]))
    assert np.isin(thresholds()[1:255], special).all() and len(special) >= 255 * 5
    for start in range(0, len(special), n // 2):
        some = special[start:start + n // 2]
        rest = rs.randint(0, ONE + 1, size=n - len(some)).astype(np.uint32).view(np.float32)
        yield rs.permutation(np.concatenate([some, rest])).reshape(h, w, 4)


@pytest.mark.parametrize("w,h", [(5, 3), (67, 9), (130, 2), (64, 8)])
def test_the_kernel_alone_at_factor_one_equals_the_host_encode(w, h):
    frames = list(edge_values(w, h, 100 + w))
    for src in frames:
        assert present(src, w, h, 1).tobytes() == encode_srgb8(src).tobytes()


def test_a_nan_channel_is_zero_and_its_neighbours_are_untouched():
    w, h = 67, 3
    src = np.random.RandomState(5).uniform(0.05, 1.0, size=(h, w, 4)).astype(np.float32)
    clean = encode_srgb8(src)
    assert (clean > 0).all()
    holes = [(0, 0, 0), (0, 1, 1), (1, 63, 2), (1, 64, 3), (2, 66, 0), (2, 66, 3)]   # (row, pixel, channel): every channel position
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7fc00000, 0xff800001], dtype=np.uint32).view(np.float32)
    for (y, x, c), v in zip(holes, nan):
        src[y, x, c] = v
    want = clean.copy()
    for y, x, c in holes:
        want[y, x, c] = 0
    assert present(src, w, h, 1).tobytes() == want.tobytes()


def fused_frame(w, h, seed):
    """float32 in [-0.25, 1.25], a tenth of the values exactly 0"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.25, 1.25, size=(h, w, 4)).astype(np.float32)
    v[rs.uniform(size=v.shape) < 0.1] = 0
    return v


@pytest.mark.parametrize("w,h,f", [(5, 3, 2), (67, 9, 3), (130, 2, 4)])
def test_the_fused_launch_is_the_resolve_encoded(w, h, f):
    src = fused_frame(w * f, h * f, 1000 * f + w)
    assert present(src, w, h, f).tobytes() == encode_srgb8(resolved(src, w, h, f)).tobytes()


@pytest.mark.parametrize("w,h,f", [(24, 40, 2), (24, 37, 3)])
def test_strips_of_the_kernel_equal_the_whole_image(w, h, f):
    """block_rows 8, three devices: by global row into one buffer, or each device's blocks back to back from its blocks of the traced
    frame back to back; 37 rows: the last block is a partial one.  Rows a device does not own keep the sentinel."""
    block_rows, count = 8, 3
    src = fused_frame(w * f, h * f, 77 + h)
    whole = present(src, w, h, f)
    assert whole.tobytes() == encode_srgb8(resolved(src, w, h, f)).tobytes()
    total_blocks = (h + block_rows - 1) // block_rows
    together = None
    for rank in range(count):
        mine = list(range(rank, total_blocks, count))
        assert lib.gr_strip_local_blocks(h, block_rows, rank, count) == len(mine)
        part = present(src, w, h, f, block_rows, rank, count, 0, fill=SENTINEL)
        owned = np.zeros(h, dtype=bool)
        for b in mine:
            owned[b * block_rows:(b + 1) * block_rows] = True
        assert part[owned].tobytes() == whole[owned].tobytes() and (part[~owned] == SENTINEL).all()
        together = part.copy() if together is None else np.where(owned[:, None, None], part, together)
        compact_src = np.zeros((h * f, w * f, 4), dtype=np.float32)
        for i, b in enumerate(mine):
            rows = src[b * block_rows * f:(b + 1) * block_rows * f]
            compact_src[i * block_rows * f:i * block_rows * f + len(rows)] = rows
        packed = present(compact_src, w, h, f, block_rows, rank, count, 1, fill=SENTINEL)
        used = 0
        for i, b in enumerate(mine):
            rows = whole[b * block_rows:(b + 1) * block_rows]
            assert packed[i * block_rows:i * block_rows + len(rows)].tobytes() == rows.tobytes(), (rank, b)
            used = i * block_rows + len(rows)
        assert (packed[used:] == SENTINEL).all()
    assert together.tobytes() == whole.tobytes()


def frame(state, rgba8, mode, adaptive, **options):
    """one frame of `state`: float32 [h, w, 4] of render(), or uint8 [h, w, 4] of render_rgba8(); the destination starts as sentinels"""
    metric, prog, cfgv = kerr()
    w, h = state.width, state.height
    feats = metric.features(adaptive_sampling=adaptive)
    dbg, levels = background()
    bg = (dbg.ptr, 1024, 512, levels)
    opts = gra.frame_options(mode=mode, **options)
    if rgba8:
        out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), SENTINEL, dtype=np.uint8))
        state.render_rgba8(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts)
        state.synchronize()
        return out.to_numpy(np.uint8, (h, w, 4))
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), SENTINEL_FLOAT, dtype=np.float32))
    state.render(prog, metric, gra.default_camera(), out.ptr, bg, feats, cfgv, opts)
    state.synchronize()
    return out.to_numpy(np.float32, (h, w, 4))


@pytest.mark.parametrize("f,mode,adaptive", [(1, gra.MODE_FUSED, 0), (2, gra.MODE_FUSED, 0), (2, gra.MODE_REFERENCE, 1)])
def test_an_rgba8_frame_is_the_float_frame_encoded(f, mode, adaptive):
    w, h = 96, 54
    got = frame(gra.RenderState(w, h, 0, supersample=f), True, mode, adaptive)
    floats = frame(gra.RenderState(w, h, 0, supersample=f), False, mode, adaptive)
    assert np.isfinite(floats).all() and floats[..., :3].max() > 0.1
    want = encode_srgb8(floats)
    assert len(np.unique(want)) > 32
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("compact", [0, 1])
def test_strips_of_an_rgba8_frame_are_the_float_strips_encoded(compact):
    """factor 1, fused, three devices, blocks of 8 rows (54 rows: the last block is a partial one): only the device's rows are written,
    laid out as gr_render_frame lays out its float rows"""
    w, h, block_rows, count = 96, 54, 8, 3
    for rank in range(count):
        options = dict(strip_rank=rank, strip_count=count, block_rows=block_rows, compact_out=compact)
        got = frame(gra.RenderState(w, h, 0), True, gra.MODE_FUSED, 0, **options)
        floats = frame(gra.RenderState(w, h, 0), False, gra.MODE_FUSED, 0, **options)
        written = (floats != SENTINEL_FLOAT).all(axis=(1, 2))
        assert 0 < written.sum() < h and np.isfinite(floats[written]).all()
        assert got[written].tobytes() == encode_srgb8(floats[written]).tobytes() and (got[~written] == SENTINEL).all(), rank


def test_a_state_used_for_both_kinds_of_frame_renders_the_same_floats():
    """render, render_rgba8, render on one state (a factor-1 state gets its traced frame with the first 8-bit frame): its float frames
    are, bit for bit, those of a state that never rendered an 8-bit one"""
    for f in (1, 2):
        both, plain = gra.RenderState(96, 54, 0, supersample=f), gra.RenderState(96, 54, 0, supersample=f)
        first = frame(both, False, gra.MODE_FUSED, 0)
        bytes8 = frame(both, True, gra.MODE_FUSED, 0)
        again = frame(both, False, gra.MODE_FUSED, 0)
        want = [frame(plain, False, gra.MODE_FUSED, 0) for _ in range(3)]
        assert first.tobytes() == want[0].tobytes() and again.tobytes() == want[2].tobytes()
        assert bytes8.tobytes() == encode_srgb8(want[1]).tobytes()


def test_rgba8_states_give_their_memory_back():
    """25 rounds of create / render_rgba8 / destroy of a 64x32 state at factors 1 and 2: free device memory comes back to where it was,
    within the allowance of tests/test_gpu_lifecycle.py, read through the HIP runtime the library itself runs on as that file does.  (The
    table of the encode is part of the program's code object: a program owns no buffer for it.)"""
    from test_gpu_lifecycle import MiB, device_bytes_in_use

    def cycle(f):
        state = gra.RenderState(64, 32, 0, supersample=f)
        pixels = frame(state, True, gra.MODE_FUSED, 0)
        assert (pixels[..., 3] > 0).any()
        del state
        gc.collect()

    for f in (1, 2):
        cycle(f)
        before = device_bytes_in_use()
        for _ in range(25):
            cycle(f)
        after = device_bytes_in_use()
        assert after - before < 4 * MiB, (f, before, after)


def test_a_refused_frame_allocates_nothing():
    """a factor-1 state gets its traced frame with its first 8-bit frame - but not from a call that is refused: without a sky the call
    returns GR_ERROR_INVALID_ARGUMENT and the state's 16 MiB traced frame (1024 x 1024 float4) has not been allocated"""
    from test_gpu_lifecycle import MiB, device_bytes_in_use
    metric, prog, cfgv = kerr()
    state = gra.RenderState(1024, 1024, 0)
    out = DeviceBuffer(0, 1024 * 1024 * 4)
    before = device_bytes_in_use()
    entry_args = (prog.handle, metric.handle, None, ctypes.byref(gra.default_camera()), None, None, 0, None, None, 0, 0, 0, out.ptr, None)
    assert lib.gr_render_frame_rgba8(state.handle, *entry_args) == -1
    assert device_bytes_in_use() - before < 4 * MiB
    dbg, levels = background()
    state.render_rgba8(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                       gra.frame_options(mode=gra.MODE_FUSED))
    state.synchronize()
    assert device_bytes_in_use() - before >= 16 * MiB   # (the same call with a sky does allocate it: the reading above could have seen it)


def test_a_pinned_download_gives_the_bytes_of_a_blocking_one():
    data = np.random.RandomState(9).randint(0, 256, size=96 * 54 * 4).astype(np.uint8)
    dev = DeviceBuffer.from_numpy(0, data)
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    pinned = PinnedBuffer(data.nbytes)
    try:
        pinned.view()[:] = 0
        pinned.download_async(stream, dev.ptr, data.nbytes)
        check(lib.gr_stream_synchronize(stream))
        assert pinned.view().tobytes() == dev.to_numpy(np.uint8, data.shape).tobytes() == data.tobytes()
        with pytest.raises(ValueError):
            pinned.download_async(stream, dev.ptr, data.nbytes + 1)
    finally:
        pinned.free()
        check(lib.gr_stream_destroy(stream))


@pytest.mark.parametrize("supersample", [1, 2])
def test_the_cli_writes_the_same_png_either_way(tmp_path, supersample):
    from geodesic_raytracing_amd import render
    paths = {}
    for where in ("host", "device"):
        paths[where] = str(tmp_path / f"kerr_{where}.png")
        assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "64x32", "--supersample", str(supersample), "--encode", where,
                            "--out", paths[where]]) == 0
    host, device = open(paths["host"], "rb").read(), open(paths["device"], "rb").read()
    assert len(host) > 1000 and host == device
    assert render.read_png(paths["device"]).shape == (32, 64, 4)
