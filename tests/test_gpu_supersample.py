"""GPU tests (-m gpu) of supersampled frames: gr_resolve_supersampled (kernels/resolve.hip) on its own against numpy, whole frames and
strips of a state made by gr_render_state_create_supersampled against the same frame traced by a plain state of the traced size and
resolved by the same kernel (bit for bit), and the object's life cycle and the CLI switch.  Kerr (scripts/kerr_boyer.js), a = 0.45."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, RENDER_DATA_DTYPE, box_resolve, download  # noqa: E402
from test_gpu_fullsize import SCRIPTS, background  # noqa: E402

GUARD = 64                # float4 pixels either side of a destination
DEADBEEF = 0xdeadbeef
SENTINEL = np.float32(-7.0)
_shared = {}


def kerr():
    """the dynamic program (adaptive sampling is one of its run-time features), shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45))
    return _shared["kerr"]


def random_frame(w, h, seed):
    """float32 in [-2, 2], a tenth of the values exactly 0, no subnormals"""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-2.0, 2.0, size=(h, w, 4)).astype(np.float32)
    v[np.abs(v) < np.finfo(np.float32).tiny] = 0
    v[rs.uniform(size=v.shape) < 0.1] = 0
    return v


def resolve(src, w, h, f, block_rows=0, rank=0, count=1, compact=0, fill=None):
    """gr_resolve_supersampled of the host array `src` (the traced frame, or a device's compact blocks) into a destination of w x h
    float4 surrounded by guard pixels; returns the destination (prefilled with `fill` when given) after checking the guards"""
    _, prog, _ = kerr()
    dsrc = DeviceBuffer.from_numpy(0, np.ascontiguousarray(src, dtype=np.float32))
    host = np.full((w * h + 2 * GUARD) * 4, DEADBEEF, dtype=np.uint32)
    if fill is not None:
        host[GUARD * 4:(GUARD + w * h) * 4] = np.full(w * h * 4, fill, dtype=np.float32).view(np.uint32)
    ddst = DeviceBuffer.from_numpy(0, host)
    check(lib.gr_resolve_supersampled(prog.handle, None, dsrc.ptr, ctypes.c_void_p(ddst.ptr.value + GUARD * 16), w, h, f, block_rows, rank, count, compact))
    check(lib.gr_device_synchronize(0))
    back = ddst.to_numpy(np.uint32, ((w * h + 2 * GUARD) * 4,))
    assert (back[:GUARD * 4] == DEADBEEF).all() and (back[(GUARD + w * h) * 4:] == DEADBEEF).all(), "guard pixels were written"
    return back[GUARD * 4:(GUARD + w * h) * 4].view(np.float32).reshape(h, w, 4)


def assert_within_the_summation_bound(gpu, reference, traced, f):
    """fp32 summation of n = f^2 terms in any order, a rounded reciprocal and one multiply: |gpu - mean| <= (n + 2) 2^-24 mean(|v|),
    every pixel, every channel"""
    h, w, c = gpu.shape
    n = f * f
    magnitude = np.abs(traced.astype(np.float64)).reshape(h, f, w, f, c).mean(axis=(1, 3))
    error = np.abs(gpu.astype(np.float64) - reference.astype(np.float64))
    bound = (n + 2) * 2.0 ** -24 * magnitude
    worst = float((error / np.maximum(bound, 1e-300)).max())
    print(f"resolve {w}x{h} f={f}: largest error {float(error.max()):.3e}, {worst:.3f} of the bound")
    assert (error <= bound).all(), (w, h, f, float(error.max()), worst)


@pytest.mark.parametrize("w,h,f", [(5, 3, 2), (67, 9, 3), (130, 2, 4), (64, 8, 1)])
def test_the_kernel_alone_against_numpy(w, h, f):
    src = random_frame(w * f, h * f, 1000 * f + w)
    out = resolve(src, w, h, f)
    if f == 1:
        assert out.tobytes() == src.tobytes()
        return
    mean64 = src.astype(np.float64).reshape(h, f, w, f, 4).mean(axis=(1, 3))
    assert_within_the_summation_bound(out, mean64, src, f)


@pytest.mark.parametrize("w,h,f", [(24, 40, 2), (24, 37, 3)])
def test_strips_of_the_kernel_equal_the_whole_image(w, h, f):
    """block_rows 8, three devices: written by global row into one buffer, or each device's blocks back to back from its blocks of the
    traced frame back to back (a traced block is f * 8 rows); 37 rows: the last block is a partial one"""
    block_rows, count = 8, 3
    src = random_frame(w * f, h * f, 77 + h)
    whole = resolve(src, w, h, f)
    total_blocks = (h + block_rows - 1) // block_rows
    together = None
    for rank in range(count):
        mine = list(range(rank, total_blocks, count))
        assert lib.gr_strip_local_blocks(h, block_rows, rank, count) == len(mine)
        # by global row: only this device's rows are written
        part = resolve(src, w, h, f, block_rows, rank, count, 0, fill=SENTINEL)
        owned = np.zeros(h, dtype=bool)
        for b in mine:
            owned[b * block_rows:(b + 1) * block_rows] = True
        assert part[owned].tobytes() == whole[owned].tobytes() and (part[~owned] == SENTINEL).all()
        together = part.copy() if together is None else np.where(owned[:, None, None], part, together)
        # compact: source and destination hold the device's blocks back to back
        compact_src = np.zeros((h * f, w * f, 4), dtype=np.float32)
        for i, b in enumerate(mine):
            rows = src[b * block_rows * f:(b + 1) * block_rows * f]
            compact_src[i * block_rows * f:i * block_rows * f + len(rows)] = rows
        packed = resolve(compact_src, w, h, f, block_rows, rank, count, 1, fill=SENTINEL)
        used = 0
        for i, b in enumerate(mine):
            rows = whole[b * block_rows:(b + 1) * block_rows]
            assert packed[i * block_rows:i * block_rows + len(rows)].tobytes() == rows.tobytes(), (rank, b)
            used = i * block_rows + len(rows)
        assert (packed[used:] == SENTINEL).all()
    assert together.tobytes() == whole.tobytes()


def frame(w, h, supersample, mode, adaptive, **options):
    """one frame of a fresh state; returns (pixels [h, w, 4], the state)"""
    metric, prog, cfgv = kerr()
    feats = metric.features(adaptive_sampling=adaptive)
    state = gra.RenderState(w, h, 0, supersample=supersample)
    dbg, levels = background()
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), SENTINEL, dtype=np.float32))
    state.render(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), feats, cfgv, gra.frame_options(mode=mode, **options))
    state.synchronize()
    return out.to_numpy(np.float32, (h, w, 4)), state


@pytest.mark.parametrize("w,h,f,mode,adaptive", [(48, 24, 2, gra.MODE_FUSED, 0), (40, 24, 3, gra.MODE_FUSED, 0), (24, 16, 4, gra.MODE_FUSED, 0),
                                                 (37, 21, 2, gra.MODE_FUSED, 0),      # traced width 74: no multiple of 8
                                                 (48, 24, 2, gra.MODE_REFERENCE, 1), (48, 24, 2, gra.MODE_FUSED, 1)])
def test_a_supersampled_frame_is_the_traced_frame_resolved(w, h, f, mode, adaptive):
    got, state = frame(w, h, f, mode, adaptive)
    assert (state.supersample, state.traced_size) == (f, (w * f, h * f))
    traced, plain = frame(w * f, h * f, 1, mode, adaptive)
    assert (plain.supersample, plain.traced_size) == (1, (w * f, h * f))
    assert np.isfinite(traced).all() and traced[..., :3].max() > 0.1 and (traced != SENTINEL).all()
    assert got.tobytes() == resolve(traced, w, h, f).tobytes()
    assert_within_the_summation_bound(got, box_resolve(traced, f), traced, f)


def test_factor_one_through_the_new_constructor_is_the_plain_frame():
    metric, prog, cfgv = kerr()
    handle = ctypes.c_void_p()
    check(lib.gr_render_state_create_supersampled(0, 48, 24, 1, ctypes.byref(handle)))
    try:
        factor, tw, th = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib.gr_render_state_supersample(handle, ctypes.byref(factor), ctypes.byref(tw), ctypes.byref(th)))
        assert (factor.value, tw.value, th.value) == (1, 48, 24)
        feats = metric.features(adaptive_sampling=0)
        dbg, levels = background()
        out = DeviceBuffer.from_numpy(0, np.full((24, 48, 4), SENTINEL, dtype=np.float32))
        opts = gra.frame_options(mode=gra.MODE_FUSED)
        check(lib.gr_render_frame(handle, prog.handle, metric.handle, None, ctypes.byref(gra.default_camera()), ctypes.byref(feats),
                                  (ctypes.c_float * len(cfgv))(*cfgv), len(cfgv), dbg.ptr, dbg.ptr, 1024, 512, levels, out.ptr, ctypes.byref(opts)))
        check(lib.gr_device_synchronize(0))
        one = out.to_numpy(np.float32, (24, 48, 4))
    finally:
        lib.gr_render_state_destroy(handle)
    plain, _ = frame(48, 24, 1, gra.MODE_FUSED, 0)
    assert one.tobytes() == plain.tobytes()
    assert gra.RenderState(48, 24, 0, supersample=1).traced_size == (48, 24)


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("compact", [0, 1])
def test_strips_of_a_supersampled_frame_assemble_to_the_whole(count, compact):
    """gr_render_frame's strip mode on a supersampled state: 48x40 at factor 2, blocks of 8 output rows (16 traced rows)"""
    w, h, f, block_rows = 48, 40, 2, 8
    if "whole_48x40" not in _shared:
        _shared["whole_48x40"] = frame(w, h, f, gra.MODE_FUSED, 0)[0]
    whole = _shared["whole_48x40"]
    total_blocks = h // block_rows
    covered = np.zeros(h, dtype=bool)
    for rank in range(count):
        part, _ = frame(w, h, f, gra.MODE_FUSED, 0, strip_rank=rank, strip_count=count, block_rows=block_rows, compact_out=compact)
        mine = list(range(rank, total_blocks, count))
        if compact:
            for i, b in enumerate(mine):
                assert part[i * block_rows:(i + 1) * block_rows].tobytes() == whole[b * block_rows:(b + 1) * block_rows].tobytes(), (rank, b)
            assert (part[len(mine) * block_rows:] == SENTINEL).all()
        else:
            owned = np.zeros(h, dtype=bool)
            for b in mine:
                owned[b * block_rows:(b + 1) * block_rows] = True
            assert part[owned].tobytes() == whole[owned].tobytes() and (part[~owned] == SENTINEL).all()
        for b in mine:
            assert not covered[b * block_rows:(b + 1) * block_rows].any()
            covered[b * block_rows:(b + 1) * block_rows] = True
    assert covered.all()


def test_without_an_output_frame_nothing_is_resolved():
    w, h, f = 48, 24, 2
    metric, prog, cfgv = kerr()
    feats = metric.features(adaptive_sampling=0)
    state = gra.RenderState(w, h, 0, supersample=f)
    factor, tw, th = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib.gr_render_state_supersample(state.handle, ctypes.byref(factor), ctypes.byref(tw), ctypes.byref(th)))
    assert (factor.value, tw.value, th.value) == (f, w * f, h * f)
    opts = gra.frame_options(mode=gra.MODE_FUSED, time_kernels=1)
    state.render(prog, metric, gra.default_camera(), None, None, feats, cfgv, opts)
    state.synchronize()
    assert state.resolve_ms() == 0.0 and state.stage_ms()["render"] == 0.0 and state.stage_ms()["trace"] > 0.0
    # the records are the traced frame's
    records = download(0, state.buffer(gra.BUF_RENDER_DATA), RENDER_DATA_DTYPE, w * f * h * f)
    plain = gra.RenderState(w * f, h * f, 0)
    plain.render(prog, metric, gra.default_camera(), None, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
    plain.synchronize()
    assert records.tobytes() == download(0, plain.buffer(gra.BUF_RENDER_DATA), RENDER_DATA_DTYPE, w * f * h * f).tobytes()
    assert (records["terminated"] == 1).any()
    # ... and with one the resolve is a launch of its own, timed by its own pair of events
    dbg, levels = background()
    out = DeviceBuffer(0, w * h * 16)
    state.render(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), feats, cfgv, opts)
    state.synchronize()
    assert state.resolve_ms() > 0.0 and state.stage_ms()["render"] > 0.0


def test_a_split_frame_refuses_a_supersampled_state():
    """gr_render_frame_tiled is not built for such a state yet: participants of this process (peer copies, no communicator) say so"""
    metric, prog, cfgv = kerr()
    dbg, levels = background()
    parts = gra.TiledFrame.local([0, 0], 48, 40, 8)
    try:
        state = gra.RenderState(48, 40, 0, supersample=2)
        out = DeviceBuffer(0, 48 * 40 * 16)
        with pytest.raises(gra.GeodesicError, match="supersampled"):
            parts[0].render(state, prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 1024, 512, levels), metric.features(adaptive_sampling=0), cfgv,
                            gra.frame_options(mode=gra.MODE_FUSED))
    finally:
        for p in parts:
            p.close()


def test_supersampled_states_give_their_memory_back():
    """ten create / render / destroy cycles of a 64x32 state at factor 4 (a traced frame of 512 KiB each): free device memory comes back
    to where it was, within the allowance of tests/test_gpu_lifecycle.py.  Asked of the HIP runtime the library itself runs on, as
    that file does (hipMemGetInfo - the figures of torch.cuda.mem_get_info): torch's CUDA side would bring a second runtime into this
    process (geodesic_raytracing_amd/__init__.py)."""
    from test_gpu_lifecycle import MiB, device_bytes_in_use

    def cycle():
        pixels, state = frame(64, 32, 4, gra.MODE_FUSED, 0)
        assert np.isfinite(pixels).all()
        del state
        gc.collect()

    cycle()
    before = device_bytes_in_use()
    for _ in range(10):
        cycle()
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


def test_the_cli_writes_a_frame_of_the_size_asked_for(tmp_path):
    from geodesic_raytracing_amd import render
    path = str(tmp_path / "kerr_ss2.png")
    assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "64x32", "--supersample", "2", "--out", path]) == 0
    png = render.read_png(path)
    assert png.shape == (32, 64, 4)
    pixels = np.ascontiguousarray(render.render("kerr_boyer", 64, 32, cfg=dict(a=0.45), supersample=2), dtype=np.float32)
    assert pixels.shape == (32, 64, 4)
    rgba = np.empty((32, 64, 4), dtype=np.uint8)
    check(lib.gr_frame_to_rgba8(pixels.ctypes.data_as(ctypes.c_void_p), 64, 32, rgba.ctypes.data_as(ctypes.c_void_p)))
    assert png.tobytes() == rgba.tobytes()
    plain = render.render("kerr_boyer", 64, 32, cfg=dict(a=0.45))
    assert plain.shape == (32, 64, 4) and plain.tobytes() != pixels.tobytes()
