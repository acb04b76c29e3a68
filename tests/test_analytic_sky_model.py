"""CPU tests of the analytic sky (include/geodesic_hip_internal.h, "Analytic sky"): the float64 model of tests/analytic_sky_model.py at
values worked out by hand, its fp32 restatement against it, the host rasteriser gr_analytic_sky_image against the model at the texel
footprint, every refusal by message, the defaults, and the struct's layout.  None of it needs a device."""
import ctypes

import numpy as np
import pytest

import analytic_sky_model as am
import geodesic_raytracing_amd as gra
import shading_model as sm
from geodesic_raytracing_amd import AnalyticSkyStruct, lib


def refused(rc, *words):
    message = lib.gr_last_error().decode()
    assert rc == -1, (rc, message)                      # GR_ERROR_INVALID_ARGUMENT
    for word in words:
        assert word in message, (word, message)


def test_struct_layout():
    assert ctypes.sizeof(AnalyticSkyStruct) == 132
    offsets = {name: getattr(AnalyticSkyStruct, name).offset for name, _ in AnalyticSkyStruct._fields_}
    assert offsets == dict(meridians=0, parallels=4, line_width=8, quadrant=12, line=108)
    s = AnalyticSkyStruct()
    s.quadrant[1][2][0] = 0.25                          # [side][q][rgb]: side is the slowest index
    assert np.frombuffer(bytes(s), dtype=np.float32)[3 + (1 * 4 + 2) * 3 + 0] == 0.25
    s.line[1][2] = 0.5
    assert np.frombuffer(bytes(s), dtype=np.float32)[27 + 1 * 3 + 2] == 0.5


def test_defaults():
    s = gra.AnalyticSky()
    assert (s.meridians, s.parallels) == (36, 18) and s.line_width == np.float32(0.08)
    q, line = s.quadrant, s.line
    assert q.shape == (2, 4, 3) and line.shape == (2, 3)
    assert q.min() >= 0 and q.max() <= 1
    colours = [tuple(c) for c in q.reshape(8, 3)]
    assert len(set(colours)) == 8                       # four distinct quadrant colours per side, another palette on side 1
    assert line.max() <= 0.05                           # near-black lines
    assert lib.gr_analytic_sky_default(None) == -1 and b"gr_analytic_sky_default" in lib.gr_last_error()


def test_hand_computed_coverages():
    w = 0.08
    # a footprint much larger than the sky: the lines cover their share w of it, each half of the quadrants half
    assert am.line_coverage(0.3137, 1000.0, 36, w) == pytest.approx(w, abs=1e-4)
    assert am.line_coverage(0.4219, 1000.0, 18, w) == pytest.approx(w, abs=1e-4)
    assert am.upper_half_u(0.3137, 1000.0) == pytest.approx(0.5, abs=1e-3)
    # (G is not continued past the unit: of a box from -1000 to 1000 the half above 1/2 is one half less a quarter of a thousandth)
    assert am.upper_half_v(0.4219, 1000.0) == pytest.approx(0.5, abs=1e-3)
    assert am.upper_half_v(0.5, 1000.0) == 0.5
    # a pixel centred on a meridian whose footprint is the line: a = w / 2
    for k in (0, 7, 35):
        assert am.line_coverage(k / 36, (w / 2) / 36, 36, w) == pytest.approx(1.0, abs=1e-12)
    # centred mid-cell with a < (1 - w) / 2: no line
    for a in (1e-3, 0.2, 0.4599):
        assert am.line_coverage(7.5 / 36, a / 36, 36, w) == 0.0
    # at u = 0.5 the footprint is half below, half above the edge, whatever its size
    for hu in (2.0 ** -14, float(np.float32(1e-3)), float(np.float32(0.1)), 0.5):   # (fp32 values, as a footprint is: 0.5 +- hu is exact in float64)
        assert am.upper_half_u(0.5, hu) == 0.5
        assert am.upper_half_v(0.5, hu) == 0.5
    assert am.upper_half_u(0.25, 0.1) == 0.0 and am.upper_half_u(0.75, 0.1) == pytest.approx(1.0, abs=1e-12)
    assert am.upper_half_v(0.25, 0.1) == 0.0 and am.upper_half_v(0.75, 0.1) == pytest.approx(1.0, abs=1e-12)
    # the pulse train is periodic, past the poles too, and no lines means no coverage
    assert am.line_coverage(-0.013, 0.004, 18, w) == pytest.approx(am.line_coverage(1 - 0.013, 0.004, 18, w), abs=1e-12)
    assert am.line_coverage(0.013, 0.004, 18, 0.0) == 0.0
    # widest lines: half of every cell
    assert am.line_coverage(0.2, 5.0, 36, 0.5) == pytest.approx(0.5, abs=1e-3)


def test_the_seam_is_half_a_turn_from_the_quadrant_edge():
    """u = 0.9995 beside 0.0005 (the texture's seam between them) is the same pair shifted by half a turn, 0.4995 beside 0.5005, with
    the quadrants swapped: the footprint comes from the WRAPPED difference, 0.001 and not 0.999, and 36 meridians repeat after half a turn"""
    sky = am.sky_of(gra.AnalyticSky(line_width=0.01))   # (thin lines: the meridian at 0 and 0.5 leaves most of the footprint to the quadrants)
    swapped = dict(sky, quadrant=sky["quadrant"][:, [1, 0, 3, 2]])
    v = np.full((1, 2), 0.31)
    e = 2.0 ** -11                                      # 0.00049: 1 - e, e and 0.5 -+ e are fp32 values, so the shift is exact in the records
    at_seam = sm.make_records(2, 1, np.array([[1 - e, e]]), v)
    shifted = sm.make_records(2, 1, np.array([[0.5 - e, 0.5 + e]]), v)
    hu, hv = am.footprint(at_seam, 2, 1)
    assert hu == pytest.approx(e, abs=1e-9) and (hv == am.FLOOR).all()
    a, b = am.evaluate(at_seam, 2, 1, sky), am.evaluate(shifted, 2, 1, swapped)
    assert np.abs(a - b).max() <= 1e-7
    assert np.abs(a - am.evaluate(shifted, 2, 1, sky)).max() > 0.05     # (the swap matters)


def test_black_records_and_alpha():
    c = am.case("sides_and_black")
    rgba = am.model_of(c)
    black = c["records"]["terminated"] != 1
    assert black.any() and (~black).any() and (rgba[black] == (0, 0, 0, 1)).all() and (rgba[:, 3] == 1).all()
    assert set(c["records"]["terminated"]) == {0, 1, 2} and set(c["records"]["side"]) == {0, 1, 2}
    both = c["records"][~black]
    other = both.copy()
    other["side"] = np.where(both["side"] >= 1, 0, 1)
    apart = np.abs(am.colour(both["tex_coord"][:, 0], both["tex_coord"][:, 1], 0.01, 0.01, np.where(both["side"] >= 1, 1, 0), c["sky"]) -
                   am.colour(both["tex_coord"][:, 0], both["tex_coord"][:, 1], 0.01, 0.01, np.where(other["side"] >= 1, 1, 0), c["sky"])).max(axis=1)
    assert np.median(apart) > 0.1                       # the two sides have palettes of their own


@pytest.mark.parametrize("name", am.case_names())
def test_restatement_against_the_model(name):
    """fp32 against float64 on every synthetic case, no record set aside: what an fp32 evaluation of the definition costs (the device's
    bounds are twice these figures where that exceeds the render stage's tolerances)"""
    c = am.case(name)
    mx, rm = am.errors(am.restatement_of(c), am.model_of(c), c["records"], c["count"])
    print(f"{name}: restatement max {mx:.2e} rmse {rm:.2e}")
    assert np.isfinite(am.restatement_of(c)).all()
    assert mx <= 2e-3 and rm <= 2e-4                    # a few ulps of a cell over a footprint of 2^-14 at the very worst


def test_profile_holds_the_restatements_figures():
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "analytic_sky_synthetic.txt")
    rows = {line.split()[0]: line.split() for line in open(path).read().splitlines() if line and not line.startswith("#")}
    now = {line.split()[0]: line.split() for line in am.table().splitlines() if not line.startswith("#")}
    assert sorted(rows) == sorted(now) == sorted(am.case_names())
    for name, fields in now.items():
        assert rows[name][1] == fields[1], name                                   # records
        for k in (2, 3):                                                          # max, RMSE: numpy's fp32 pow and tanh may differ by an ulp between machines
            assert float(rows[name][k]) == pytest.approx(float(fields[k]), rel=0.1, abs=1e-9), (name, rows[name], fields)
        assert rows[name][-2:] == fields[-2:], name                               # the bounds they give


def test_the_lazy_texture_model_is_shading_models_own():
    """am.texture_model: shading_model.evaluate with texels converted on lookup - the same bits on skies small enough for both"""
    for name, sky in (("anisotropy_30deg_p8", "sky1"), ("sides", "sky2"), ("seams_37x19_up", "sky1"), ("redshift_new_noise", "sky1")):
        c = sm.case(name)
        args = (c["max_probes"], c["features"]["redshift"], c["features"]["use_old_redshift"])
        want = sm.evaluate(c["records"], c["width"], c["height"], c[sky], c[sky], *args)["rgba"]
        assert np.array_equal(am.texture_model(c["records"], c["width"], c["height"], c[sky], *args), want)
    assert sm._sample.__module__ == "shading_model"                              # put back


def test_the_command_line_takes_a_sky():
    from geodesic_raytracing_amd.render import main, parse_sky
    s = parse_sky("grid")
    assert (s.meridians, s.parallels, s.line_width) == (36, 18, np.float32(0.08))
    s = parse_sky("grid:12x6")
    assert (s.meridians, s.parallels, s.line_width) == (12, 6, np.float32(0.08))
    s = parse_sky("grid:360x180:0.5")
    assert (s.meridians, s.parallels, s.line_width) == (360, 180, 0.5)
    for bad in ("stars", "grid:12", "grid:12x6x3", "grid:axb", "grid:12x6:wide", "grid:12x6:0.1:7", ""):
        with pytest.raises(ValueError):
            parse_sky(bad)
    for bad, field in (("grid:1x6", "meridians"), ("grid:12x0", "parallels"), ("grid:12x6:0.6", "line_width")):
        with pytest.raises(gra.GeodesicError, match=field):
            parse_sky(bad)


@pytest.mark.parametrize("extra,words", [(["--background", "sky.png"], "--sky with --background / --mips"), (["--mips", "host"], "--sky with --background / --mips"),
                                         (["--mips", "device"], "--sky with --background / --mips"), ([], None)])
def test_the_command_line_refuses_a_sky_beside_an_image(extra, words, capsys):
    """before anything is rendered or read; with words = None the sky itself is out of range and the library's message is handed on"""
    from geodesic_raytracing_amd.render import main
    sky = "grid" if words else "grid:500x2"
    with pytest.raises(SystemExit) as e:
        main(["--metric", "kerr_boyer", "--sky", sky, "--out", "never.png"] + extra)
    assert e.value.code == 2
    assert (words or "meridians 500") in capsys.readouterr().err


def test_the_mips_default_is_still_host(capsys):
    """--mips has no argparse default any more (None tells "not given" from "host", for the refusal above); what a command line without it
    does is unchanged, and --help still says which that is"""
    from geodesic_raytracing_amd.render import main
    with pytest.raises(SystemExit):
        main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "and upload all of them (default: host)" in text


@pytest.mark.parametrize("size", [(64, 32), (257, 129), (1, 1)])
@pytest.mark.parametrize("side", [0, 1])
def test_sky_image_against_the_model(size, side):
    """gr_analytic_sky_image: the definition at the footprint of one texel, within 1 LSB (the rounding of the 8-bit store)"""
    w, h = size
    for sky in (gra.AnalyticSky(), gra.AnalyticSky(meridians=7, parallels=5, line_width=0.31)):
        got = sky.image(w, h, side)
        assert got.shape == (h, w, 4) and (got[..., 3] == 255).all()
        want = am.image(am.sky_of(sky), side, w, h) * 255.0
        assert np.abs(got[..., :3].astype(np.float64) - want).max() <= 1.0
        if w > 1:
            assert np.abs(got[..., :3].astype(np.float64) - want).mean() <= 0.4   # rounded to the nearest (0.25 on average), not truncated (0.5)
    if w > 1:
        img = gra.AnalyticSky().image(w, h, side)
        assert len(np.unique(img.reshape(-1, 4), axis=0)) > 8                    # quadrants, lines and their blends


def _bad_skies():
    def sky(**kw):
        s = gra.AnalyticSky()
        for k, v in kw.items():
            setattr(s.struct, k, v)
        return s

    def coloured(field, index, value):
        s = gra.AnalyticSky()
        a = np.ctypeslib.as_array(getattr(s.struct, field))
        a[index] = value
        return s
    nan, inf = float("nan"), float("inf")
    return [(sky(meridians=1), "meridians"), (sky(meridians=361), "meridians"), (sky(meridians=-4), "meridians"),
            (sky(parallels=0), "parallels"), (sky(parallels=181), "parallels"),
            (sky(line_width=-0.01), "line_width"), (sky(line_width=0.51), "line_width"), (sky(line_width=nan), "line_width"), (sky(line_width=inf), "line_width"),
            (coloured("quadrant", (0, 0, 0), -0.1), "quadrant[0][0][0]"), (coloured("quadrant", (1, 3, 2), 1.5), "quadrant[1][3][2]"),
            (coloured("quadrant", (1, 2, 1), nan), "quadrant[1][2][1]"), (coloured("quadrant", (0, 1, 0), inf), "quadrant[0][1][0]"),
            (coloured("line", (0, 1), 1.01), "line[0][1]"), (coloured("line", (1, 2), nan), "line[1][2]"), (coloured("line", (1, 0), -inf), "line[1][0]")]


def test_every_refusal_names_the_function_and_the_field():
    """before any device call: none of these needs a device, a program or a state that exists"""
    somewhere = ctypes.c_void_p(4096)   # never dereferenced: the sky is refused first
    out = np.zeros((4, 4, 4), dtype=np.uint8)
    good = gra.AnalyticSky()
    for sky, field in _bad_skies():
        ref = ctypes.byref(sky.struct)
        refused(lib.gr_analytic_sky_image(ref, 0, 4, 4, out.ctypes.data_as(ctypes.c_void_p)), "gr_analytic_sky_image", field)
        refused(lib.gr_render_analytic(None, None, somewhere, somewhere, 16, somewhere, ref, 4, 4, None, None), "gr_render_analytic", field)
        refused(lib.gr_render_analytic_strips(None, None, somewhere, somewhere, ref, 4, 4, 4, 0, 1, 0, None, None), "gr_render_analytic_strips", field)
        refused(lib.gr_render_state_set_sky(somewhere, ref), "gr_render_state_set_sky", field)   # (the sky is looked at before the state)
    ref = ctypes.byref(good.struct)
    # a NULL
    refused(lib.gr_analytic_sky_image(None, 0, 4, 4, out.ctypes.data_as(ctypes.c_void_p)), "gr_analytic_sky_image", "null")
    refused(lib.gr_analytic_sky_image(ref, 0, 4, 4, None), "gr_analytic_sky_image", "null")
    refused(lib.gr_render_analytic(None, None, somewhere, somewhere, 16, somewhere, None, 4, 4, None, None), "gr_render_analytic", "null sky")
    refused(lib.gr_render_analytic_strips(None, None, somewhere, somewhere, None, 4, 4, 4, 0, 1, 0, None, None), "gr_render_analytic_strips", "null sky")
    refused(lib.gr_render_state_set_sky(None, ref), "gr_render_state_set_sky", "null")
    is_set = ctypes.c_int()
    refused(lib.gr_render_state_sky(None, ref, ctypes.byref(is_set)), "gr_render_state_sky", "null")
    # what gr_render and gr_render_strips refuse: a NULL buffer, bad strip parameters - and a NULL program, after the sky
    for args in ((None, somewhere, 16, somewhere), (somewhere, None, 16, somewhere), (somewhere, somewhere, 16, None)):
        refused(lib.gr_render_analytic(None, None, *args, ref, 4, 4, None, None), "gr_render_analytic", "NULL")
    refused(lib.gr_render_analytic_strips(None, None, None, somewhere, ref, 4, 4, 4, 0, 1, 0, None, None), "gr_render_analytic_strips", "NULL")
    refused(lib.gr_render_analytic_strips(None, None, somewhere, None, ref, 4, 4, 4, 0, 1, 0, None, None), "gr_render_analytic_strips", "NULL")
    for block_rows, rank, ranks in ((0, 0, 1), (4, 0, 0), (4, -1, 2), (4, 2, 2)):
        refused(lib.gr_render_analytic_strips(None, None, somewhere, somewhere, ref, 4, 4, block_rows, rank, ranks, 0, None, None),
                "gr_render_analytic_strips", "strip")
    refused(lib.gr_render_analytic(None, None, somewhere, somewhere, 16, somewhere, ref, 4, 4, None, None), "null program")
    refused(lib.gr_render_analytic_strips(None, None, somewhere, somewhere, ref, 4, 4, 4, 0, 1, 0, None, None), "null program")
    # the rasteriser's own arguments
    refused(lib.gr_analytic_sky_image(ref, 2, 4, 4, out.ctypes.data_as(ctypes.c_void_p)), "gr_analytic_sky_image", "side")
    refused(lib.gr_analytic_sky_image(ref, 0, 0, 4, out.ctypes.data_as(ctypes.c_void_p)), "gr_analytic_sky_image", "width")
    # ... and the Python layer hands the library's message on
    with pytest.raises(gra.GeodesicError, match="parallels"):
        gra.AnalyticSky(parallels=500).image(4, 4)


@pytest.mark.parametrize("name", ["gr_render_strips", "gr_render_seams"])
def test_the_texture_strip_launchers_refuse_a_null_buffer_first(name):
    """as gr_render_analytic_strips does: a NULL rdata, out, bg1 or bg2 under the function's name, then the geometry, then the program -
    none of it needs a device"""
    call = getattr(lib, name)
    somewhere = ctypes.c_void_p(4096)   # never dereferenced: no call gets as far as a launch
    for missing in range(4):
        buffers = [None if k == missing else somewhere for k in range(4)]
        refused(call(None, None, *buffers, 16, 8, 1, 8, 8, 8, 0, 1, 0, 4, None, None), name, "NULL")
        refused(call(None, None, *buffers, 16, 8, 1, 8, 8, 0, 3, 2, 0, 4, None, None), name, "NULL")   # (before the geometry's refusals)
    good = [somewhere] * 4
    for block_rows, rank, ranks in ((0, 0, 1), (8, 0, 0), (8, -1, 2), (8, 2, 2)):
        refused(lib.gr_render_strips(None, None, *good, 16, 8, 1, 8, 8, block_rows, rank, ranks, 0, 4, None, None), "strip")
    refused(lib.gr_render_seams(None, None, *good, 16, 8, 1, 8, 8, 4, 0, 2, 0, 4, None, None), "gr_render_seams", "multiples of 8")
    refused(lib.gr_render_seams(None, None, *good, 16, 8, 1, 12, 8, 8, 0, 1, 0, 4, None, None), "gr_render_seams", "multiples of 8")
    refused(call(None, None, *good, 16, 8, 1, 8, 8, 8, 0, 1, 0, 4, None, None), "null program")
