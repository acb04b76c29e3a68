"""CPU tests of the star sky (include/geodesic_hip_internal.h, "Star sky"): properties of the float64 model of tests/star_sky_model.py
that follow from the definition alone (the tents' partition of unity, the magnification law), the library's generator against the numpy
one, every refusal that needs no device, the command line, and the committed figures of the fp32 restatement."""
import ctypes
import os

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
import shading_model as sm
import star_sky_model as ssm
from geodesic_raytracing_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_A_PROGRAM = ctypes.c_void_p(0x1000)   # every refusal below comes before the program is looked into


def lattice(width, height, origin, spacing):
    """records on a regular lattice of exactly representable coordinates"""
    u = origin[0] + spacing[0] * np.arange(width)[None, :] + np.zeros((height, 1))
    v = origin[1] + spacing[1] * np.arange(height)[:, None] + np.zeros((1, width))
    r = sm.make_records(width, height, u, v)
    assert (r["tex_coord"][:, 0].astype(np.float64) == u.reshape(-1)).all() and (r["tex_coord"][:, 1].astype(np.float64) == v.reshape(-1)).all()
    return r


def test_the_tents_are_a_partition_of_unity():
    """records on a regular lattice: sum of S 4 hu hv over the pixels = the summed flux of the stars strictly inside, to 1e-12"""
    w, h, origin, spacing = 24, 17, (0.25, 0.375), (2.0 ** -9, 2.0 ** -10)
    r = lattice(w, h, origin, spacing)
    rng = np.random.default_rng(5)
    n = 4000
    uv = np.stack([origin[0] + rng.uniform(-3, w + 2, n) * spacing[0], origin[1] + rng.uniform(-3, h + 2, n) * spacing[1]], axis=1).astype(np.float32)
    # a star outside the lattice but within one spacing of it lies under the outermost pixels' tents with part of its weight: it is
    # neither inside nor out of reach, and the statement is about the other two kinds
    a, b = (uv[:, 0].astype(np.float64) - origin[0]) / spacing[0], (uv[:, 1].astype(np.float64) - origin[1]) / spacing[1]
    in_the_hull = (a > 0) & (a < w - 1) & (b > 0) & (b < h - 1)
    out_of_reach = (a < -1) | (a > w) | (b < -1) | (b > h)
    uv = uv[in_the_hull | out_of_reach]
    n = len(uv)
    assert out_of_reach.sum() > 300
    flux = rng.uniform(0, 1e-6, (n, 3)).astype(np.float32)
    cat = ssm.catalogue(uv, flux, 64, 32)
    sky = dict(min_footprint=2.0 ** -16, background=np.zeros((2, 3), dtype=np.float32))
    assert ssm.regimes(r, w, h, sky, (cat, cat)).all()                            # every pixel sums the stars themselves
    S = ssm.evaluate(r, w, h, sky, (cat, cat))[:, :3]
    hu, hv = ssm.footprint64(r, w, h, sky["min_footprint"])
    assert np.allclose(hu, spacing[0] / 2, rtol=1e-13) and np.allclose(hv, spacing[1] / 2, rtol=1e-13)   # the tent's half-width is the spacing
    got = (S * (4 * hu * hv)[:, None]).sum(axis=0)
    us, vs = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    inside = (us > origin[0]) & (us < origin[0] + (w - 1) * spacing[0]) & (vs > origin[1]) & (vs < origin[1] + (h - 1) * spacing[1])
    assert 500 < inside.sum() < n - 500
    want = flux[inside].astype(np.float64).sum(axis=0)
    assert np.abs(got - want).max() <= 1e-12 * want.max()


def test_halving_the_spacing_multiplies_an_isolated_stars_peak_by_four():
    origin, star = (0.5, 0.25), (0.5 + 8 * 2.0 ** -9, 0.25 + 6 * 2.0 ** -10)
    cat = ssm.catalogue(np.array([star]), np.array([[3e-7, 2e-7, 1e-7]]), 64, 32)
    sky = dict(min_footprint=2.0 ** -20, background=np.zeros((2, 3), dtype=np.float32))
    peaks = []
    for halvings in (0, 1, 2):
        k = 2 ** halvings
        r = lattice(16 * k + 1, 12 * k + 1, origin, (2.0 ** -9 / k, 2.0 ** -10 / k))
        S = ssm.evaluate(r, 16 * k + 1, 12 * k + 1, sky, (cat, cat))[:, :3]
        assert (S > 0).any(axis=1).sum() == 1                                     # the star sits on a lattice point: one pixel holds it
        peaks.append(S.max(axis=0))
    for coarse, fine in zip(peaks, peaks[1:]):
        assert np.abs(fine / coarse - 4).max() <= 1e-12
    # ... down to the floor and no further: below min_footprint the star is no longer a point
    sky["min_footprint"] = 2.0 ** -10
    r = lattice(65, 49, origin, (2.0 ** -11, 2.0 ** -12))
    capped = ssm.evaluate(r, 65, 49, sky, (cat, cat))[:, :3].max(axis=0)
    assert np.allclose(capped, np.array([3e-7, 2e-7, 1e-7], dtype=np.float32).astype(np.float64) / (4 * 2.0 ** -20), rtol=1e-12)


@pytest.mark.parametrize("seed,n", [(0, 1), (7, 1000), (2 ** 64 - 1, 4097)])
def test_the_librarys_generator_is_the_numpy_one(seed, n):
    uv, flux = gra.star_field_random(seed, n)
    want_uv, want_flux = ssm.star_field_random(seed, n)
    assert uv.dtype == np.float32 and uv.shape == (n, 2) and flux.shape == (n, 3)
    assert uv.tobytes() == want_uv.tobytes()                                      # positions: to the last bit of the float
    assert np.abs(flux / want_flux - 1).max() <= 1e-6
    assert (uv[:, 0] >= 0).all() and (uv[:, 0] < 1).all() and (uv[:, 1] >= 0).all() and (uv[:, 1] <= 1).all() and (flux >= 0).all()
    if n >= 1000:   # uniform on the sphere: cos(pi v) is uniform, and so is u
        assert abs(np.cos(np.pi * uv[:, 1].astype(np.float64)).mean()) < 0.1 and abs(uv[:, 0].mean() - 0.5) < 0.05


def refused(rc, *words):
    assert rc != 0
    message = lib.gr_last_error().decode()
    for word in words:
        assert word in message, (message, word)


def create(n, uv, flux, cells_u=64, cells_v=32, program=NOT_A_PROGRAM, out=True):
    handle = ctypes.c_void_p()
    uv = None if uv is None else np.ascontiguousarray(uv, dtype=np.float32)
    flux = None if flux is None else np.ascontiguousarray(flux, dtype=np.float32)
    return lib.gr_star_catalogue_create(program, n, None if uv is None else uv.ctypes.data_as(ctypes.c_void_p),
                                        None if flux is None else flux.ctypes.data_as(ctypes.c_void_p), cells_u, cells_v, ctypes.byref(handle) if out else None)


def test_the_catalogue_refuses_by_field_name():
    uv, flux = np.full((4, 2), 0.5), np.full((4, 3), 1e-6)
    who = "gr_star_catalogue_create"
    refused(create(4, uv, flux, program=None), who, "program")
    refused(create(4, None, flux), who, "uv")
    refused(create(4, uv, None), who, "flux")
    refused(create(4, uv, flux, out=False), who, "out")
    for n in (0, -1, 2 ** 24 + 1):
        refused(create(n, uv, flux), who, "n ")
    for cells in (8, 15, 48, 100, 8192, -16):
        refused(create(4, uv, flux, cells_u=cells), who, "cells_u")
        refused(create(4, uv, flux, cells_v=cells), who, "cells_v")
    for bad in (1.0, -1e-9, np.nan, np.inf):
        wrong = uv.copy()
        wrong[2, 0] = bad
        refused(create(4, wrong, flux), who, "uv", "u of star 2")
    for bad in (1.0000001, -1e-9, np.nan, -np.inf):
        wrong = uv.copy()
        wrong[3, 1] = bad
        refused(create(4, wrong, flux), who, "uv", "v of star 3")
    for bad in (-1e-12, np.nan, np.inf):
        wrong = flux.copy()
        wrong[1, 2] = bad
        refused(create(4, uv, wrong), who, "flux", "star 1")
    refused(lib.gr_star_catalogue_info(None, None, None, None), "gr_star_catalogue_info")
    refused(lib.gr_star_catalogue_download(None, None, None, None), "gr_star_catalogue_download")
    lib.gr_star_catalogue_destroy(None)
    out = np.zeros(8, dtype=np.float32)
    at = out.ctypes.data_as(ctypes.c_void_p)
    refused(lib.gr_star_field_random(1, 1, None, at), "gr_star_field_random", "out_uv")
    refused(lib.gr_star_field_random(1, 1, at, None), "gr_star_field_random", "out_flux")
    refused(lib.gr_star_field_random(1, 0, at, at), "gr_star_field_random", "n ")
    refused(lib.gr_star_sky_default(None), "gr_star_sky_default")


def _bad_star_skies():
    def sky(min_footprint=None, background=None):
        s = gra.StarSky()
        if min_footprint is not None:
            s.struct.min_footprint = min_footprint
        if background is not None:
            s.struct.background[background[0]][background[1]] = background[2]
        return s
    out = [(sky(min_footprint=m), "min_footprint") for m in (0.0, -2.0 ** -16, 2.0 ** -21, 2.0 ** -7, 3 * 2.0 ** -18, float("nan"), float("inf"))]
    out += [(sky(background=(side, c, bad)), f"background[{side}][{c}]") for side, c, bad in ((0, 0, -0.1), (1, 2, 1.5), (0, 1, float("nan")))]
    return out


def test_the_launchers_refuse_by_field_name():
    """gr_render_stars and gr_render_stars_strips, before any device call: the pointers here are no buffers at all"""
    some = ctypes.c_void_p(0x2000)
    good = gra.StarSky()
    for who, call in (("gr_render_stars", lambda sky, rdata=some, out=some: lib.gr_render_stars(NOT_A_PROGRAM, None, rdata, some, 16, out, sky, None, None, 4, 4, None, None)),
                      ("gr_render_stars_strips", lambda sky, rdata=some, out=some, rows=2: lib.gr_render_stars_strips(NOT_A_PROGRAM, None, rdata, out, sky, None, None, 4, 4, rows, 0, 2, 0, None, None))):
        refused(call(ctypes.byref(good.struct), rdata=None), who, "NULL")
        refused(call(ctypes.byref(good.struct), out=None), who, "NULL")
        refused(call(None), who, "sky")
        for sky, field in _bad_star_skies():
            refused(call(ctypes.byref(sky.struct)), who, field)
    refused(lib.gr_render_stars(NOT_A_PROGRAM, None, some, None, 16, some, ctypes.byref(good.struct), None, None, 4, 4, None, None), "gr_render_stars", "NULL")
    for rows, rank, count in ((0, 0, 2), (2, 2, 2), (2, -1, 2), (2, 0, 0)):
        refused(lib.gr_render_stars_strips(NOT_A_PROGRAM, None, some, some, ctypes.byref(good.struct), None, None, 4, 4, rows, rank, count, 0, None, None),
                "gr_render_stars_strips", "strip")
    refused(lib.gr_render_state_set_stars(None, ctypes.byref(good.struct), None, None), "gr_render_state_set_stars", "render state")
    refused(lib.gr_render_state_stars(None, None, None, None, None), "gr_render_state_stars")


def test_the_struct_and_its_defaults():
    s = gra.StarSky()
    assert ctypes.sizeof(s.struct) == 28 and s.min_footprint == 2.0 ** -16 and (s.background == 0).all()
    s = gra.StarSky(min_footprint=2.0 ** -12, background=[[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    assert s.min_footprint == 2.0 ** -12 and np.allclose(s.background, [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])


def test_the_command_line_takes_stars():
    from geodesic_raytracing_amd.render import StarField, parse_sky
    s = parse_sky("stars:5000")
    assert isinstance(s, StarField) and (s.n, s.seed, s.min_footprint) == (5000, 1, 2.0 ** -16)
    s = parse_sky("stars:200000:7:0.0009765625")
    assert (s.n, s.seed, s.min_footprint) == (200000, 7, 2.0 ** -10)
    for bad in ("stars", "stars:0", "stars:many", "stars:10:x", "stars:10:1:0.001", "stars:10:1:0.5", "stars:10:1:6e-8", "stars:10:1:2:3", "stars:16777217"):
        with pytest.raises(ValueError):
            parse_sky(bad)


@pytest.mark.parametrize("extra", [["--background", "sky.png"], ["--mips", "host"], ["--mips", "device"]])
def test_the_command_line_refuses_stars_beside_an_image(extra, capsys):
    from geodesic_raytracing_amd.render import main
    with pytest.raises(SystemExit) as e:
        main(["--metric", "kerr_boyer", "--sky", "stars:1000", "--out", "never.png"] + extra)
    assert e.value.code == 2 and "--sky with --background / --mips" in capsys.readouterr().err


@pytest.mark.parametrize("name", ssm.case_names())
def test_restatement_against_the_model(name):
    """fp32 against float64 on every synthetic case, and what the cases are there for"""
    c = ssm.case(name)
    mx, rm = ssm.errors(ssm.restatement_of(c), ssm.model_of(c), c["records"], c["count"])
    print(f"{name}: restatement max {mx:.2e} rms {rm:.2e}")
    assert np.isfinite(ssm.restatement_of(c)).all() and np.isfinite(ssm.model_of(c)).all()
    shaded = c["records"]["terminated"] == 1
    assert (ssm.model_of(c)[shaded, :3].max(axis=1) > 0.01).sum() >= max(2, shaded.sum() // 6)    # stars are seen: the frame is no black one
    assert mx <= 2e-3 and rm <= 2e-4


def test_the_cases_reach_both_sides_of_the_regime():
    du, _ = ssm.spans(ssm.case("span_u_20x12"))
    _, dv = ssm.spans(ssm.case("span_v_20x12"))
    assert set(np.unique(du)) == {3, 4} and set(np.unique(dv)) == {3, 4}
    assert (du == 3).sum() > 20 and (du == 4).sum() > 20 and (dv == 3).sum() > 20 and (dv == 4).sum() > 20
    c = ssm.case("hu_half_24x9")
    assert np.allclose(ssm.footprint32(c["records"], 24, 9, 2.0 ** -16)[0], 0.5, atol=1e-6)
    c = ssm.case("floor_67x5")
    hu, hv = ssm.footprint32(c["records"], 67, 5, 2.0 ** -16)
    assert (hu == np.float32(2.0 ** -16)).all() and (hv == np.float32(2.0 ** -16)).all()


def test_profile_holds_the_restatements_figures():
    path = os.path.join(ROOT, "profiles", "star_sky_synthetic.txt")
    rows = {line.split()[0]: line.split() for line in open(path).read().splitlines() if line and not line.startswith("#")}
    now = {line.split()[0]: line.split() for line in ssm.table().splitlines() if not line.startswith("#")}
    assert sorted(rows) == sorted(now) == sorted(ssm.case_names())
    for name, fields in now.items():
        assert rows[name][1:3] == fields[1:3], name                               # records, far records
        for k in (3, 4):                                                          # max, RMS: numpy's fp32 pow and tanh may differ by an ulp between machines
            assert float(rows[name][k]) == pytest.approx(float(fields[k]), rel=0.1, abs=1e-9), (name, rows[name], fields)
