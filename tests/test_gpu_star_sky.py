"""GPU tests (-m gpu) of the star sky: gr_render_stars (kernels/shading.hip) on records made by hand against the float64 model of
tests/star_sky_model.py, its strips against its whole frame, and whole frames of states with stars.

The harness is that of tests/test_gpu_analytic_sky.py, copied: the records sit in the middle of a larger device buffer, 64 poison records
(terminated, random coordinates) either side; the frame is filled with a marker and has guard floats either side; every test shades with
the Kerr dynamic program; a second run over other poison must give the same bits.

Bounds, per case and over EVERY shaded record in front of the count (none is set aside: the regime is decided in fp32 by single IEEE
operations, so the model repeats the device's decision, and a pixel whose regime differs shows as an error far above any bound): with
e = |got - want| / max(1, want), max e <= max(2e-4, 2 x the fp32 restatement's own max on that case), RMS e <= max(1e-5, 2 x its RMS).
2e-4 and 1e-5 are the render stage's tolerances in this project; the factor 2 allows for contraction and the hardware log2 / exp2 of the
device build.  The restatement's figures are in profiles/star_sky_synthetic.txt.  Whole frames are held to the same bounds, with the
restatement run on the state's own records."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import star_sky_model as ssm  # noqa: E402
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


def on_device(prog, cat):
    """a model catalogue built on the device (None stays None)"""
    return None if cat is None else gra.StarCatalogue(prog, cat["uv"], cat["flux"], cat["cells_u"], cat["cells_v"])


def star_sky(sky):
    return gra.StarSky(min_footprint=sky["min_footprint"], background=sky["background"])


def catalogues_of(c):
    key = ("catalogues", c["name"])
    if key not in _shared:
        prog = program("kerr_boyer", a=0.45)[1]
        _shared[key] = (on_device(prog, c["cats"][0]), on_device(prog, c["cats"][1]))   # (far, near)
    return _shared[key]


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
    sky = star_sky(c["sky"])
    far, near = catalogues_of(c)
    near_at, far_at = near.handle if near else None, far.handle if far else None
    if strips is None:
        count = DeviceBuffer.from_numpy(0, np.array([c["count"]], dtype=np.int32))
        check(lib.gr_render_stars(prog.handle, None, records_at, count.ptr, n, out_at, ctypes.byref(sky.struct), near_at, far_at, w, h, cfg.ptr, dfg.ptr))
    else:
        rank, ranks, block_rows = strips
        check(lib.gr_render_stars_strips(prog.handle, None, records_at, out_at, ctypes.byref(sky.struct), near_at, far_at, w, h, block_rows, rank, ranks,
                                         compact, cfg.ptr, dfg.ptr))
    check(lib.gr_device_synchronize(0))
    back = out.to_numpy(np.float32, (GUARD + 4 * n + GUARD,))
    assert (back[:GUARD] == GUARD_VALUE).all() and (back[GUARD + 4 * n:] == GUARD_VALUE).all(), "guard floats around the frame were written"
    return back[GUARD:GUARD + 4 * n].reshape(n, 4)


def rendered(c):
    """gr_render_stars' frame of a case, [n][4] in pixel (= record) order, once per case and not written to"""
    key = ("frame", c["name"])
    if key not in _shared:
        frame = launch(c)
        frame.setflags(write=False)
        _shared[key] = frame
    return _shared[key]


def assert_within_bounds(name, got, want, restated, records, count=None):
    want_max, want_rms = ssm.errors(restated, want, records, count)
    bound_max, bound_rms = ssm.bounds(want_max, want_rms)
    mx, rm = ssm.errors(got, want, records, count)
    print(f"{name}: gpu max {mx:.2e} rms {rm:.2e} (bounds {bound_max:.1e} {bound_rms:.1e}; restatement max {want_max:.2e} rms {want_rms:.2e})")
    assert mx <= bound_max and rm <= bound_rms, (name, mx, rm, bound_max, bound_rms)


@pytest.mark.parametrize("name", ssm.case_names())
def test_gr_render_stars_against_the_float64_model(name):
    c = ssm.case(name)
    px = rendered(c)
    r = c["records"]
    assert (r["sx"] + r["sy"] * c["width"] == np.arange(len(r))).all()              # records in pixel order: px is in record order
    behind = np.arange(len(px)) >= c["count"]
    assert (px[behind] == MARKER).all(), "a record behind the count was shaded"
    assert np.isfinite(px[~behind]).all()
    black = (r["terminated"] != 1) & ~behind
    assert (px[black] == (0, 0, 0, 1)).all()                                        # terminated 0 and 2: exactly (0, 0, 0, 1)
    shaded = ~black & ~behind
    # (not ">= 0": a far pixel over an empty stretch of sky is the difference of four table terms, a residue of either sign of some
    # 2^-53 of the table's total over the footprint's area - 2e-14 here)
    assert (px[shaded, 3] == 1).all() and px[shaded, :3].min() >= -1e-9
    if c["cats"][0] is None:                                                        # no far catalogue: the far side is its background alone
        far_side = shaded & (r["side"] < 1)
        assert far_side.any() and len(np.unique(px[far_side, :3], axis=0)) == 1
    again = launch(c, poison_seed=2)
    assert again.tobytes() == px.tobytes(), "the frame depends on records outside it"
    assert_within_bounds(name, px, ssm.model_of(c), ssm.restatement_of(c), r, c["count"])


SHAPES = ["ordinary_67x5", "span_u_20x12", "sides_and_black_24x9", "frame_1x7"]   # 67 x 5, 20 x 12, 24 x 9, 1 x 7


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("strips", [(0, 1, None), (1, 3, 2), (2, 3, 2), (0, 2, 4), (1, 2, 4)])
@pytest.mark.parametrize("name", SHAPES)
def test_strips_are_gr_render_stars_rows_bit_for_bit(name, strips, compact):
    """gr_render_stars_strips: the row blocks of one rank (block-cyclic), in place or back to back; the marker everywhere else"""
    c = ssm.case(name)
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


# ---- whole frames of a state with stars --------------------------------------------------------------------------------------------
FRAMES = {"kerr": ("kerr_boyer", 96, 54, dict(a=0.45)), "minkowski": ("minkowski", 128, 72, {})}
BRIGHTER = 3000.0   # the generator's fluxes suit a 4K pixel; a pixel of these frames covers a thousand times the sky


def field():
    """the model's catalogue of 20 000 generated stars at 64 x 32 cells, and the StarSky of the frames"""
    if "field" not in _shared:
        uv, flux = gra.star_field_random(9, 20000)
        _shared["field"] = ssm.catalogue(uv, flux * np.float32(BRIGHTER), 64, 32)
    return _shared["field"], dict(min_footprint=2.0 ** -16, background=np.array([[0.0, 0.0, 0.02], [0.0, 0.0, 0.02]], dtype=np.float32))


def stars_for(prog):
    key = ("field on device", id(prog))
    if key not in _shared:
        _shared[key] = on_device(prog, field()[0])
    return _shared[key]


def star_frame(which, supersample=1, rgba8=False, size=None):
    """one frame of a fresh state with stars and NULL backgrounds -> (the frame, the state's records)"""
    name, w, h, cfg = FRAMES[which]
    w, h = size or (w, h)
    metric, prog, cfgv = program(name, **cfg)
    cat = stars_for(prog)
    state = gra.RenderState(w, h, 0, supersample=supersample, stars=(star_sky(field()[1]), cat, cat))
    assert state.stars[0].min_footprint == 2.0 ** -16 and state.stars[1] is cat and state.sky is None
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    state.render(prog, metric, gra.default_camera(), out.ptr, None, metric.features(adaptive_sampling=0), cfgv, gra.frame_options(mode=gra.MODE_FUSED), rgba8=rgba8)
    state.synchronize()
    tw, th = state.traced_size
    records = download(0, state.buffer(gra.BUF_RENDER_DATA), RENDER_DATA_DTYPE, tw * th)
    return out.to_numpy(np.uint8 if rgba8 else np.float32, (h, w, 4)), records


def float_frame(which, size=None):
    key = ("whole", which, size)
    if key not in _shared:
        _shared[key] = star_frame(which, size=size)
    return _shared[key]


def launcher_frame(which, records, w, h):
    """gr_render_stars over a state's records -> [h][w][4]"""
    name, _, _, cfg = FRAMES[which]
    metric, prog, cfgv = program(name, **cfg)
    cat = stars_for(prog)
    cfgd = DeviceBuffer.from_numpy(0, np.array(cfgv, dtype=np.float32))
    dfg = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(metric.features(adaptive_sampling=0)), dtype=np.uint8))
    rec = DeviceBuffer.from_numpy(0, records)
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    count = DeviceBuffer.from_numpy(0, np.array([w * h], dtype=np.int32))
    sky = star_sky(field()[1])
    check(lib.gr_render_stars(prog.handle, None, rec.ptr, count.ptr, w * h, out.ptr, ctypes.byref(sky.struct), cat.handle, cat.handle, w, h, cfgd.ptr, dfg.ptr))
    check(lib.gr_device_synchronize(0))
    return out.to_numpy(np.float32, (h, w, 4))


@pytest.mark.parametrize("which", ["kerr", "minkowski"])
def test_a_state_with_stars_renders_the_model_of_its_own_records(which):
    _, w, h, _ = FRAMES[which]
    frame, records = float_frame(which)
    assert (frame != MARKER).all() and np.isfinite(frame).all()
    assert (records["sx"] + records["sy"] * w == np.arange(w * h)).all()
    cat, sky = field()
    want, restated = ssm.evaluate(records, w, h, sky, (cat, cat)), ssm.restate32(records, w, h, sky, (cat, cat))
    got = frame.reshape(w * h, 4)
    black = records["terminated"] != 1
    assert (got[black] == (0, 0, 0, 1)).all() and (got[:, 3] == 1).all()
    near = ssm.regimes(records, w, h, sky, (cat, cat))
    print(f"{which}: {int((~black).sum())} shaded records, {int((~near & ~black).sum())} of them far")
    assert (~black).sum() > w * h // 4 and (got[~black, :3].max(axis=1) > 0.05).sum() > 100        # a picture: stars are seen
    if which == "kerr":
        assert (~near & ~black).sum() > 20 and (near & ~black).sum() > 1000                        # both regimes occur
    assert_within_bounds(f"{which} {w}x{h}", got, want, restated, records)
    assert frame.tobytes() == launcher_frame(which, records, w, h).tobytes()                       # the state launches the launcher's kernel


def test_the_rgba8_frame_is_the_encoded_float_frame():
    frame, _ = float_frame("kerr")
    got, _ = star_frame("kerr", rgba8=True)
    assert got.tobytes() == gra.encode_srgb8(frame).tobytes()


def test_a_supersampled_state_delivers_the_resolved_star_frame():
    """factor 2: the box average of what the launcher gives on the traced records (within the resolve's summation bound, 6 x 2^-24 of the
    largest value averaged)"""
    w, h = 48, 27
    got, records = star_frame("kerr", supersample=2, size=(w, h))
    assert len(records) == 4 * w * h
    traced = launcher_frame("kerr", records, 2 * w, 2 * h)
    want = gra.box_resolve(traced, 2)
    largest = traced.reshape(h, 2, w, 2, 4).max(axis=(1, 3))
    assert (np.abs(got.astype(np.float64) - want) <= 6 * 2.0 ** -24 * np.maximum(1.0, largest)).all()


def test_a_split_frame_on_two_participants_is_the_whole_frame():
    name, w, h, cfg = FRAMES["minkowski"]
    metric, prog, cfgv = program(name, **cfg)
    whole, _ = float_frame("minkowski")
    cat = stars_for(prog)
    parts = gra.TiledFrame.local([0, 0], w, h, 16)
    states = [gra.RenderState(w, h, 0, stars=(star_sky(field()[1]), cat, cat)) for _ in parts]
    out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
    for r in (0, 1):
        parts[r].render_as(states[r], prog, metric, gra.default_camera(), out.ptr, None, metric.features(adaptive_sampling=0), cfgv, gra.frame_options(mode=gra.MODE_FUSED))
    parts[0].join()
    check(lib.gr_device_synchronize(0))
    got = out.to_numpy(np.float32, (h, w, 4))
    for p in parts:
        p.close()
    assert got.tobytes() == whole.tobytes()


def test_stars_set_and_cleared_leave_the_texture_path_as_it_was():
    name, w, h, cfg = FRAMES["minkowski"]
    metric, prog, cfgv = program(name, **cfg)
    packed, levels = gra.pack_background(gra.synthetic_background(256, 128))
    dbg = DeviceBuffer.from_numpy(0, packed)
    feats = metric.features(adaptive_sampling=0)
    cat = stars_for(prog)
    frames = []
    for with_stars in (False, True):
        state = gra.RenderState(w, h, 0)
        out = DeviceBuffer.from_numpy(0, np.full((h, w, 4), MARKER, dtype=np.float32))
        if with_stars:
            state.set_stars(star_sky(field()[1]), cat, None)
            assert state.stars[1] is cat and state.stars[2] is None
            state.render(prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
            state.synchronize()
            between = out.to_numpy(np.float32, (h, w, 4))
            state.set_stars(None)
            assert state.stars is None
            with pytest.raises(gra.GeodesicError, match="background"):      # ... and needs its textures again
                state.render(prog, metric, gra.default_camera(), out.ptr, None, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
        state.render(prog, metric, gra.default_camera(), out.ptr, (dbg.ptr, 256, 128, levels), feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
        state.synchronize()
        frames.append(out.to_numpy(np.float32, (h, w, 4)))
    assert frames[0].tobytes() == frames[1].tobytes()
    assert np.abs(between - frames[0]).max() > 0.05                         # (the star frame was another picture)


def test_a_state_refuses_stars_beside_an_analytic_sky_and_bad_fields():
    state = gra.RenderState(32, 18, 0)
    prog = program("minkowski")[1]
    cat = stars_for(prog)
    for min_footprint, field_name in ((3 * 2.0 ** -18, "min_footprint"), (2.0 ** -7, "min_footprint")):
        bad = gra.StarSky()
        bad.struct.min_footprint = min_footprint
        with pytest.raises(gra.GeodesicError, match=f"gr_render_state_set_stars.*{field_name}"):
            state.set_stars(bad, cat, cat)
    bad = gra.StarSky()
    bad.struct.background[1][2] = 1.5
    with pytest.raises(gra.GeodesicError, match=r"gr_render_state_set_stars.*background\[1\]\[2\]"):
        state.set_stars(bad, cat, cat)
    assert state.stars is None
    state.set_sky(gra.AnalyticSky())
    with pytest.raises(gra.GeodesicError, match="gr_render_state_set_stars.*analytic sky"):
        state.set_stars(gra.StarSky(), cat, cat)
    state.set_sky(None)
    state.set_stars(gra.StarSky(), cat, cat)
    with pytest.raises(gra.GeodesicError, match="gr_render_state_set_sky.*stars"):
        state.set_sky(gra.AnalyticSky())
    assert state.sky is None and state.stars[1] is cat
