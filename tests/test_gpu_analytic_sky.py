"""GPU tests (-m gpu) of the analytic sky: gr_render_analytic (kernels/shading.hip) on records made by hand against the float64 model of
tests/analytic_sky_model.py, its strips against its whole frame, whole frames of states with a sky, and the same sky sent down the
texture path (gr_render on gr_analytic_sky_image's 4096 x 2048 image), which ties the definition to the path the reference pins.

The harness is that of tests/test_gpu_shading.py: the records sit in the middle of a larger device buffer, 64 poison records
(terminated, random coordinates) either side; the frame is filled with a marker and has guard floats either side; every test shades with
the Kerr dynamic program; a second run over other poison must give the same bits.

Bounds, per case and over EVERY shaded record in front of the count (none is set aside: the floor on the footprint makes the
definition continuous): max |rgb error| <= max(2e-4, 2 x the fp32 restatement's own max error against the model on that case),
RMSE <= max(1e-5, 2 x its RMSE).  2e-4 and 1e-5 are the render stage's tolerances in this project; the factor 2 allows for contraction
and the hardware log2 / exp2 of the device build, which the restatement has none of.  They were fixed before the first run on a
device.  The restatement's figures are 1e-9 to 1.3e-5 (profiles/analytic_sky_synthetic.txt), so the floors are the bound in every
case today.  Whole frames are held to the same bounds, with the restatement run on the state's own records."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import analytic_sky_model as am  # noqa: E402
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import RENDER_DATA_DTYPE, DeviceBuffer, download  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "geodesic_raytracing_amd", "scripts")
POISON = 64               # records either side of the frame's
GUARD = 256               # floats either side of the frame
GUARD_VALUE = np.float32(12345.0)
MARKER = np.float32(-7.25)
_shared = {}


def program(name, **cfg):
    """(metric, its dynamic program, cfg values), once per metric"""
    if name not in _shared:
        metric = gra.Metric(name, SCRIPTS)
        _shared[name] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(**cfg))
    return _shared[name]


def sky_struct(sky):
    return gra.AnalyticSky(meridians=sky["meridians"], parallels=sky["parallels"], line_width=float(sky["line_width"]), quadrant=sky["quadrant"], line=sky["line"])


def launch(c, strips=None, compact=0, poison_seed=1):
    """one launch over the case's records -> the frame buffer as it is afterwards, [height * width][4] (the guards checked)"""
    metric, prog, cfgv = program("kerr_boyer", a=0.45)
    cfg = DeviceBuffer.from_numpy(0, np.array(cfgv, dtype=np.float32))
    w, h, n = c["width"], c["height"], len(c["records"])
    rng = np.random.default_rng(poison_seed)
    host = np.zeros(n + 2 * POISON, dtype=RENDER_DATA_DTYPE)
    host["terminated"], host["side"] = 1, 1
    host["tex_coord"] = rng.random((n + 2 * POISON, 2), dtype=np.float32)
    host["sx"], host["sy"] = rng.integers(0, w, n + 2 * POISON), rng.integers(0, h, n + 2 * POISON)
    host[POISON:POISON + n] = c["records"]
    records = DeviceBuffer.from_numpy(0, host)
    frame = np.full(GUARD + 4 * n + GUARD, GUARD_VALUE, dtype=np.float32)
    frame[GUARD:GUARD + 4 * n] = MARKER
    out = DeviceBuffer.from_numpy(0, frame)
    records_at = ctypes.c_void_p(records.ptr.value + POISON * RENDER_DATA_DTYPE.itemsize)
    out_at = ctypes.c_void_p(out.ptr.value + GUARD * 4)
    dfg = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(gra.default_features(**c["features"])), dtype=np.uint8))
    sky = sky_struct(c["sky"])
    if strips is None:
        count = DeviceBuffer.from_numpy(0, np.array([c["count"]], dtype=np.int32))
        check(lib.gr_render_analytic(prog.handle, None, records_at, count.ptr, n, out_at, ctypes.byref(sky.struct), w, h, cfg.ptr, dfg.ptr))
    else:
        rank, ranks, block_rows = strips
        check(lib.gr_render_analytic_strips(prog.handle, None, records_at, out_at, ctypes.byref(sky.struct), w, h, block_rows, rank, ranks, compact,
                                            cfg.ptr, dfg.ptr))
    check(lib.gr_device_synchronize(0))
    back = out.to_numpy(np.float32, (GUARD + 4 * n + GUARD,))
    assert (back[:GUARD] == GUARD_VALUE).all() and (back[GUARD + 4 * n:] == GUARD_VALUE).all(), "guard floats around the frame were written"
    return back[GUARD:GUARD + 4 * n].reshape(n, 4)


def rendered(c):
    """gr_render_analytic's frame of a case, [n][4] in pixel (= record) order, once per case and not written to"""
    key = ("frame", c["name"])
    if key not in _shared:
        frame = launch(c)
        frame.setflags(write=False)
        _shared[key] = frame
    return _shared[key]


def assert_within_bounds(name, got, want, restated, records, count=None):
    want_max, want_rmse = am.errors(restated, want, records, count)
    bound_max, bound_rmse = am.bounds(want_max, want_rmse)
    mx, rm = am.errors(got, want, records, count)
    print(f"{name}: gpu max {mx:.2e} rmse {rm:.2e} (bounds {bound_max:.1e} {bound_rmse:.1e}; restatement max {want_max:.2e} rmse {want_rmse:.2e})")
    assert mx <= bound_max and rm <= bound_rmse, (name, mx, rm, bound_max, bound_rmse)


@pytest.mark.parametrize("name", am.case_names())
def test_gr_render_analytic_against_the_float64_model(name):
    c = am.case(name)
    px = rendered(c)
    r = c["records"]
    assert (r["sx"] + r["sy"] * c["width"] == np.arange(len(r))).all()              # records in pixel order: px is in record order
    behind = np.arange(len(px)) >= c["count"]
    assert (px[behind] == MARKER).all(), "a record behind the count was shaded"
    assert np.isfinite(px[~behind]).all()
    black = (r["terminated"] != 1) & ~behind
    assert (px[black] == (0, 0, 0, 1)).all()                                        # terminated 0 and 2: exactly (0, 0, 0, 1)
    shaded = ~black & ~behind
    assert (px[shaded, 3] == 1).all()
    assert px[shaded, :3].min() >= 0 and px[shaded, :3].max() <= 1
    again = launch(c, poison_seed=2)
    assert again.tobytes() == px.tobytes(), "the frame depends on records outside it"
    assert_within_bounds(name, px, am.model_of(c), am.restatement_of(c), r, c["count"])


SHAPES = ["frame_67x5", "centres", "sides_and_black", "frame_1x7"]   # 67 x 5, 20 x 12, 24 x 9, 1 x 7


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("strips", [(0, 1, None), (1, 3, 2), (2, 3, 2), (0, 2, 4), (1, 2, 4)])
@pytest.mark.parametrize("name", SHAPES)
def test_strips_are_gr_render_analytics_rows_bit_for_bit(name, strips, compact):
    """gr_render_analytic_strips: the row blocks of one rank (block-cyclic), in place or back to back; the marker everywhere else"""
    c = am.case(name)
    w, h = c["width"], c["height"]
    rank, ranks, block_rows = strips[0], strips[1], strips[2] or h
    whole = rendered(c)
    got = launch(c, (rank, ranks, block_rows), compact)
    want = np.full((h * w, 4), MARKER, dtype=np.float32)
    blocks = range(rank, (h + block_rows - 1) // block_rows, ranks)
    assert len(blocks) == lib.gr_strip_local_blocks(h, block_rows, rank, ranks)
    for i, b in enumerate(blocks):
        rows = slice(b * block_rows * w, min((b + 1) * block_rows, h) * w)
        at = i * block_rows * w if compact else rows.start
        want[at:at + (rows.stop - rows.start)] = whole[rows]
    assert got.tobytes() == want.tobytes()


# ---- whole frames of a state with a sky --------------------------------------------------------------------------------------------
FRAMES = [("minkowski", 128, 72, {}), ("schwarzschild", 128, 72, {}), ("kerr_boyer", 96, 54, dict(a=0.45))]


def sky_frame(name, w, h, cfg, mode, supersample=1, rgba8=False, sky=None):
    """one frame of a fresh state with a sky and NULL backgrounds -> (the frame, the state's records)"""
    metric, prog, cfgv = program(name, **cfg)
    state = gra.RenderState(w, h, 0, supersample=supersample, sky=sky or gra.AnalyticSky())
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    feats = metric.features(adaptive_sampling=0)
    state.render(prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=mode), rgba8=rgba8)
    state.synchronize()
    tw, th = state.traced_size
    records = download(0, state.buffer(gra.BUF_RENDER_DATA), RENDER_DATA_DTYPE, tw * th)
    if rgba8:
        return out.to_numpy(np.uint8, (h, w, 4)), records
    return out.to_numpy(np.float32, (h, w, 4)), records


def float_frame(name, w, h, cfg, mode):
    key = ("whole", name, w, h, mode)
    if key not in _shared:
        _shared[key] = sky_frame(name, w, h, cfg, mode)
    return _shared[key]


@pytest.mark.parametrize("mode", [gra.MODE_FUSED, gra.MODE_REFERENCE])
@pytest.mark.parametrize("name,w,h,cfg", FRAMES)
def test_a_state_with_a_sky_renders_the_model_of_its_own_records(name, w, h, cfg, mode):
    frame, records = float_frame(name, w, h, cfg, mode)
    assert (frame != MARKER).all() and np.isfinite(frame).all()
    assert (records["sx"] + records["sy"] * w == np.arange(w * h)).all()
    sky = am.sky_of(gra.AnalyticSky())
    want, restated = am.evaluate(records, w, h, sky), am.restate32(records, w, h, sky)
    got = frame.reshape(w * h, 4)
    black = records["terminated"] != 1
    assert (got[black] == (0, 0, 0, 1)).all() and (got[:, 3] == 1).all()
    assert (~black).sum() > w * h // 4 and len(np.unique(np.round(got[~black, :3], 2), axis=0)) > 8   # a picture: quadrants, lines, blends
    assert_within_bounds(f"{name} {w}x{h} mode {mode}", got, want, restated, records)


def test_the_rgba8_frame_is_the_encoded_float_frame():
    name, w, h, cfg = FRAMES[1]
    frame, _ = float_frame(name, w, h, cfg, gra.MODE_FUSED)
    got, _ = sky_frame(name, w, h, cfg, gra.MODE_FUSED, rgba8=True)
    assert got.tobytes() == gra.encode_srgb8(frame).tobytes()


def test_a_sky_set_and_cleared_leaves_the_texture_path_as_it_was():
    name, w, h, cfg = FRAMES[1]
    metric, prog, cfgv = program(name, **cfg)
    packed, levels = gra.pack_background(gra.synthetic_background(256, 128))
    dbg = DeviceBuffer.from_numpy(0, packed)
    feats = metric.features(adaptive_sampling=0)
    frames = []
    for with_sky in (False, True):
        state = gra.RenderState(w, h, 0)
        out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
        if with_sky:
            state.set_sky(gra.AnalyticSky(meridians=12))
            assert state.sky.meridians == 12
            state.render(prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
            state.synchronize()
            between = out.to_numpy(np.float32, (h, w, 4))
            state.set_sky(None)
            assert state.sky is None
            with pytest.raises(gra.GeodesicError, match="background"):      # ... and needs its textures again
                state.render(prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
        state.render(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 256, 128, levels), feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
        state.synchronize()
        frames.append(out.to_numpy(np.float32, (h, w, 4)))
    assert frames[0].tobytes() == frames[1].tobytes()
    assert np.abs(between - frames[0]).max() > 0.05                         # (the sky frame was another picture)


def test_a_supersampled_state_delivers_the_resolved_sky_frame():
    """factor 2: the frame is the box average of the frame a plain state of the traced size renders with the same sky (within the
    resolve's summation bound, (4 + 2) 2^-24 of values in [0, 1])"""
    name, w, h, cfg = "schwarzschild", 64, 36, {}
    got, records = sky_frame(name, w, h, cfg, gra.MODE_FUSED, supersample=2)
    assert len(records) == 4 * w * h
    traced, _ = float_frame(name, 2 * w, 2 * h, cfg, gra.MODE_FUSED)
    assert np.abs(got.astype(np.float64) - gra.box_resolve(traced, 2)).max() <= 6 * 2.0 ** -24


def test_a_split_frame_on_two_participants_is_the_whole_frame():
    name, w, h, cfg = FRAMES[1]
    metric, prog, cfgv = program(name, **cfg)
    whole, _ = float_frame(name, w, h, cfg, gra.MODE_FUSED)
    feats = metric.features(adaptive_sampling=0)
    parts = gra.TiledFrame.local([0, 0], w, h, 16)
    states = [gra.RenderState(w, h, 0, sky=gra.AnalyticSky()) for _ in parts]
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    for r in (0, 1):
        parts[r].render_as(states[r], prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
    parts[0].join()
    check(lib.gr_device_synchronize(0))
    got = out.to_numpy(np.float32, (h, w, 4))
    for p in parts:
        p.close()
    assert got.tobytes() == whole.tobytes()


def test_the_same_sky_down_the_texture_path():
    """The texture cross-check: the default sky rasterised by gr_analytic_sky_image at 4096 x 2048, packed, and rendered through
    gr_render on the 128 x 72 Schwarzschild frame, against the analytic frame of the same records.  The two definitions differ - an
    8-bit image filtered by Gaussian-weighted trilinear probes against an exact box - by D, the mean |rgb difference| between
    shading_model on that image and the analytic model on the same records, both in float64 on the CPU
    (profiles/analytic_sky_synthetic.txt holds the figure).  The two device frames must be no further apart than that plus the render
    stage's tolerance: mean |difference| <= D + 2e-4.  Neither kernel is measured against itself."""
    name, w, h, cfg = FRAMES[1]
    metric, prog, cfgv = program(name, **cfg)
    analytic, records = float_frame(name, w, h, cfg, gra.MODE_FUSED)
    sky = gra.AnalyticSky()
    sides = set(np.where(records["side"][records["terminated"] == 1] >= 1, 1, 0))
    assert len(sides) == 1                                                       # no wormhole: one sky is read, handed over as both
    packed, levels = gra.pack_background(sky.image(4096, 2048, side=sides.pop()))
    dbg = DeviceBuffer.from_numpy(0, packed)
    state = gra.RenderState(w, h, 0)
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    state.render(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 4096, 2048, levels), metric.features(adaptive_sampling=0), cfgv,
                 gra.frame_options(mode=gra.MODE_FUSED, max_probes=8))
    state.synchronize()
    textured = out.to_numpy(np.float32, (h, w, 4))
    again = download(0, state.buffer(gra.BUF_RENDER_DATA), RENDER_DATA_DTYPE, w * h)
    assert again.tobytes() == records.tobytes()                                  # the same records under both frames
    shaded = records["terminated"] == 1
    on_image = am.texture_model(records, w, h, packed, 8)
    in_closed_form = am.evaluate(records, w, h, am.sky_of(sky))
    D = float(np.abs(on_image[shaded, :3] - in_closed_form[shaded, :3]).mean())
    got = float(np.abs(textured.reshape(-1, 4)[shaded, :3].astype(np.float64) - analytic.reshape(-1, 4)[shaded, :3]).mean())
    print(f"texture cross-check: {int(shaded.sum())} shaded records, D = {D:.3e} (models), device frames {got:.3e}, bound {D + 2e-4:.3e}")
    assert got <= D + 2e-4
    # ... and record by record: each device frame is within the render stage's tolerance of its own model (2e-4 at the most on the
    # records no decision of the texture path sets aside, which the mean takes in as they come), so the two differences - device
    # against device, model against model - are within twice that of each other on average
    apart = float(np.abs((textured.reshape(-1, 4)[shaded, :3].astype(np.float64) - analytic.reshape(-1, 4)[shaded, :3]) -
                         (on_image[shaded, :3] - in_closed_form[shaded, :3])).mean())
    print(f"texture cross-check: the two differences are {apart:.3e} apart on average (bound 4e-4)")
    assert apart <= 4e-4
