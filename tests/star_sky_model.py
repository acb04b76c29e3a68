"""A float64 model of the star sky, its fp32 restatement, the catalogue and the generator in numpy, and the synthetic records they are
held against (tests/test_star_sky_model.py on the CPU, tests/test_gpu_star_catalogue.py and tests/test_gpu_star_sky.py on the device).

Written from the definition in include/geodesic_hip_internal.h ("Star sky"), step by step; it imports nothing of the library and shares
no arithmetic with kernels/stars.hip or kernels/shading.hip.  What it takes from the other models are the wrapped differences and the
colour curves the definition takes over from gr_render unchanged (tests/shading_model.py, tests/analytic_sky_model.py).

  * the regime (step 2) is decided in numpy's float32, operation by operation as the header states it, so that the model and the
    device agree on every pixel: a pixel whose regime differs is a failure, not a tolerance case;
  * the near sum (step 3) is a brute-force sum over ALL stars of the side's catalogue - no cells - which checks the kernel's cell walk;
  * the table (step 4) is np.cumsum along u, then along v, of the cells' sums taken in ascending catalogue index;
  * restate32() is steps 3 to 5 once more in float32 (the far integral in double from the fp32 footprint, as the definition has it):
    its own distance from the model, case by case, sets the device's bounds (profiles/star_sky_synthetic.txt;
    `python tests/star_sky_model.py` prints it).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (run as a script: the record layout lives in oracle/)

import analytic_sky_model as am
import shading_model as sm

F = np.float32
MARGIN = F(2.0 ** -22)
DEFAULT_MIN_FOOTPRINT = 2.0 ** -16


# ---- the generator -----------------------------------------------------------------------------------------------------------------
SPECTRAL_COLOURS = np.array([[0.61, 0.71, 1.0], [0.68, 0.77, 1.0], [0.80, 0.85, 1.0], [0.97, 0.96, 1.0], [1.0, 0.92, 0.82], [1.0, 0.78, 0.56], [1.0, 0.58, 0.33]])


def splitmix64(seed, count):
    """draws 1 ... count of the stream -> float64 in [0, 1)"""
    with np.errstate(over="ignore"):
        state = np.uint64(seed) + np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = state
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def star_field_random(seed, n):
    """gr_star_field_random's recipe -> (uv float32 [n][2], flux float64 [n][3] before it is stored as float)"""
    x = splitmix64(seed, 4 * n).reshape(n, 4)
    u = x[:, 0].astype(F)
    u[u >= 1] = 0
    V = np.arccos(1 - 2 * x[:, 1]) / np.pi
    brightness = 2e-9 * np.minimum((1 - x[:, 2]) ** (-2.0 / 3.0), 1e4)
    k = np.minimum(np.floor(7 * x[:, 3]).astype(np.int64), 6)
    area = 2 * np.pi ** 2 * np.maximum(np.sin(np.pi * V), 1e-3)
    return np.stack([u, V.astype(F)], axis=1), brightness[:, None] * SPECTRAL_COLOURS[k] / area[:, None]


# ---- the catalogue -----------------------------------------------------------------------------------------------------------------
def catalogue(uv, flux, cells_u, cells_v):
    """-> dict: uv, flux (float32 as uploaded), cells_u, cells_v, cell [n], cell_start [cells + 1], order [n], table [3][cells_v + 1][cells_u + 1]"""
    uv, flux = np.ascontiguousarray(uv, dtype=F), np.ascontiguousarray(flux, dtype=F)
    i = np.minimum(np.floor(uv[:, 0] * F(cells_u)).astype(np.int64), cells_u - 1)
    j = np.minimum(np.floor(uv[:, 1] * F(cells_v)).astype(np.int64), cells_v - 1)
    cell = j * cells_u + i
    cells = cells_u * cells_v
    cell_start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=cells))]).astype(np.int32)
    order = np.argsort(cell, kind="stable").astype(np.int32)           # ascending catalogue index within a cell
    sums = np.zeros((cells, 3))
    np.add.at(sums, cell, flux.astype(np.float64))                       # unbuffered, in index order: ascending catalogue index
    table = np.zeros((3, cells_v + 1, cells_u + 1))
    table[:, 1:, 1:] = sums.reshape(cells_v, cells_u, 3).transpose(2, 0, 1)
    table = np.cumsum(np.cumsum(table, axis=2), axis=1)                  # along u, then along v
    return dict(uv=uv, flux=flux, cells_u=cells_u, cells_v=cells_v, cell=cell, cell_start=cell_start, order=order, table=table)


# ---- step 1 and step 2 ---------------------------------------------------------------------------------------------------------------
def footprint64(records, width, height, min_footprint):
    r = np.asarray(records)
    beside, below = am.neighbours(r, width, height)
    tl = r["tex_coord"]
    d = lambda other, axis: np.abs(sm._wrapped_difference(tl[:, axis], other[:, axis])[0])
    return np.maximum((d(beside, 0) + d(below, 0)) / 2, min_footprint), np.maximum((d(beside, 1) + d(below, 1)) / 2, min_footprint)


def footprint32(records, width, height, min_footprint):
    r = np.asarray(records)
    beside, below = am.neighbours(r, width, height)
    tl = r["tex_coord"].astype(F)
    d = lambda other, axis: np.abs(am._wrapped_difference32(tl[:, axis], other[:, axis].astype(F)))
    return np.maximum(F(0.5) * (d(beside, 0) + d(below, 0)), F(min_footprint)), np.maximum(F(0.5) * (d(beside, 1) + d(below, 1)), F(min_footprint))


def regime32(u, v, hu, hv, cells_u, cells_v):
    """step 2 in float32 -> (i0, i1, j0, j1, near)"""
    u, v, hu, hv = (np.asarray(a, dtype=F) for a in (u, v, hu, hv))
    ru, rv = F(2) * hu + MARGIN, F(2) * hv + MARGIN
    assert ru.dtype == F and ((u - ru) * F(cells_u)).dtype == F
    i0, i1 = np.floor((u - ru) * F(cells_u)).astype(np.int64), np.floor((u + ru) * F(cells_u)).astype(np.int64)
    j0, j1 = np.floor((v - rv) * F(cells_v)).astype(np.int64), np.floor((v + rv) * F(cells_v)).astype(np.int64)
    return i0, i1, j0, j1, (i1 - i0 <= 3) & (j1 - j0 <= 3)


# ---- steps 3 and 4, float64 ----------------------------------------------------------------------------------------------------------
def near_sum(u, v, hu, hv, cat, dtype=np.float64, chunk=256):
    """S of step 3 for every given pixel, over ALL stars of the catalogue -> [n][3]"""
    T = dtype
    us, vs, flux = cat["uv"][:, 0].astype(T), cat["uv"][:, 1].astype(T), cat["flux"].astype(T)
    out = np.zeros((len(u), 3), dtype=T)
    for at in range(0, len(u), chunk):
        pu, pv = u[at:at + chunk, None].astype(T), v[at:at + chunk, None].astype(T)
        inv_u, inv_v = T(1) / (T(2) * hu[at:at + chunk, None].astype(T)), T(1) / (T(2) * hv[at:at + chunk, None].astype(T))
        du = us[None, :] - pu
        if T is np.float64:
            du = du - np.rint(du)
        else:   # the fp32 evaluation the header prescribes: no position is rounded against the turn
            du = np.where(du > T(0.5), (us[None, :] - T(1)) - pu, np.where(du < T(-0.5), us[None, :] - (pu - T(1)), du))
        weight = np.maximum(T(1) - np.abs(du) * inv_u, T(0)) * np.maximum(T(1) - np.abs(vs[None, :] - pv) * inv_v, T(0))
        out[at:at + chunk] = weight @ flux
    return out / (T(4) * hu.astype(T) * hv.astype(T))[:, None]


def table_at(table, x, y):
    """I(x, y) of step 4 -> [n][3]"""
    cells_v, cells_u = table.shape[1] - 1, table.shape[2] - 1
    turns = np.floor(x)
    X, Y = (x - turns) * cells_u, y * cells_v
    i, j = np.clip(np.floor(X).astype(np.int64), 0, cells_u - 1), np.clip(np.floor(Y).astype(np.int64), 0, cells_v - 1)
    a, b = (X - i)[None, :], (Y - j)[None, :]
    inside = (1 - a) * (1 - b) * table[:, j, i] + a * (1 - b) * table[:, j, i + 1] + (1 - a) * b * table[:, j + 1, i] + a * b * table[:, j + 1, i + 1]
    return (inside + turns[None, :] * ((1 - b) * table[:, j, cells_u] + b * table[:, j + 1, cells_u])).T


def far_sum(u, v, hu, hv, cat):
    """S of step 4 in float64 from whatever precision the footprint comes in -> [n][3]"""
    u, v, hu, hv = (np.asarray(a).astype(np.float64) for a in (u, v, hu, hv))
    v0, v1 = np.maximum(v - hv, 0.0), np.minimum(v + hv, 1.0)
    t = cat["table"]
    total = table_at(t, u + hu, v1) - table_at(t, u - hu, v1) - table_at(t, u + hu, v0) + table_at(t, u - hu, v0)
    return total / (4 * hu * hv)[:, None]


def regimes(records, width, height, sky, cats):
    """per record: True near, False far (the fp32 decision; records of a side without a catalogue, and black ones: near)"""
    r = np.asarray(records)
    hu, hv = footprint32(r, width, height, sky["min_footprint"])
    side = np.where(r["side"] >= 1, 1, 0)
    near = np.ones(len(r), dtype=bool)
    for s in (0, 1):
        if cats[s] is not None:
            sel = side == s
            near[sel] = regime32(r["tex_coord"][sel, 0], r["tex_coord"][sel, 1], hu[sel], hv[sel], cats[s]["cells_u"], cats[s]["cells_v"])[4]
    return near


def _redshift_linear(lin, z, use_old_redshift):
    """apply_redshift on a linear colour (shading_model._redshift without its srgb_to_linear), float64"""
    test_wavelength = 555 / 299792458.0
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        local_wavelength = test_wavelength / (z + 1)
        lum = 0.2126 * lin[..., 0] + 0.7152 * lin[..., 1] + 0.0722 * lin[..., 2]
        new_lum = np.clip(local_wavelength ** 3 * lum / test_wavelength ** 3, 0.0, 1.0)
        gate = lum > 0.00001
        lin = np.where(gate[..., None], np.clip((new_lum / np.where(gate, lum, 1.0))[..., None] * lin, 0.0, 1.0), lin)
        energy = sm._energy_of(lin)
        red = np.array([1 / 0.2125, 0, 0]) * energy[..., None]
        blue = np.array([0, 0, 1 / 0.0721]) * energy[..., None]
        to_red = lin + (red - lin) * np.tanh(z)[..., None]
        col = lin + (blue - lin) * np.tanh(1 / (1 + z) - 1)[..., None]
        if not use_old_redshift:
            remaining = sm._energy_of(col) - sm._energy_of(np.clip(col, 0.0, 1.0))
            col = col.copy()
            col[..., 0] += remaining / 0.2125
            col[..., 1] += remaining / 0.7154
        return np.clip(np.where((z > 0)[..., None], to_red, col), 0.0, 1.0)


def _shade(records, width, height, sky, cats, redshift, use_old_redshift, linear_framebuffer, single):
    r = np.asarray(records)
    T = F if single else np.float64
    u, v = r["tex_coord"][:, 0].astype(T), r["tex_coord"][:, 1].astype(T)
    hu32, hv32 = footprint32(r, width, height, sky["min_footprint"])
    hu, hv = (hu32, hv32) if single else footprint64(r, width, height, sky["min_footprint"])
    side = np.where(r["side"] >= 1, 1, 0)
    shaded = r["terminated"] == 1
    S = np.zeros((len(r), 3), dtype=T)
    for s in (0, 1):
        cat = cats[s]
        if cat is None:
            continue
        sel = shaded & (side == s)
        near = regime32(r["tex_coord"][:, 0], r["tex_coord"][:, 1], hu32, hv32, cat["cells_u"], cat["cells_v"])[4]
        a, b = sel & near, sel & ~near
        if a.any():
            S[a] = near_sum(u[a], v[a], hu[a], hv[a], cat, T)
        if b.any():
            S[b] = far_sum(u[b], v[b], hu[b], hv[b], cat).astype(T)
    background = np.asarray(sky["background"], dtype=F).reshape(2, 3)
    if single:
        rgb = (am._srgb_to_lin32(background)[side] + S).astype(F)
        if redshift:
            rgb = am._redshift32(rgb, r["z_shift"].astype(F), use_old_redshift)
        if not linear_framebuffer:
            rgb = am._lin_to_srgb32(rgb)
    else:
        rgb = sm._srgb_to_lin(background.astype(np.float64))[side] + S
        if redshift:
            rgb = _redshift_linear(rgb, r["z_shift"].astype(np.float64), use_old_redshift)
        if not linear_framebuffer:
            rgb = sm._lin_to_srgb(rgb)
    rgba = np.concatenate([rgb, np.ones((len(r), 1), dtype=T)], axis=1).astype(T)
    rgba[~shaded] = (0, 0, 0, 1)
    return rgba


def evaluate(records, width, height, sky, cats, redshift=0, use_old_redshift=0, linear_framebuffer=True):
    """every record shaded -> rgba [n][4] in float64.  sky: dict(min_footprint, background [2][3]); cats: (far, near) = [side], None = no stars"""
    return _shade(records, width, height, sky, cats, redshift, use_old_redshift, linear_framebuffer, single=False)


def restate32(records, width, height, sky, cats, redshift=0, use_old_redshift=0, linear_framebuffer=True):
    """evaluate() with steps 3 to 5 in float32 -> rgba [n][4] float32"""
    return _shade(records, width, height, sky, cats, redshift, use_old_redshift, linear_framebuffer, single=True)


# ---- errors and bounds ---------------------------------------------------------------------------------------------------------------
def errors(got, want, records, count=None):
    """(max e, RMS e) with e = |got - want| / max(1, want), over every shaded record in front of the count: none is set aside"""
    sel = np.asarray(records)["terminated"] == 1
    if count is not None:
        sel = sel & (np.arange(len(sel)) < count)
    assert sel.any()
    want = np.asarray(want)[sel, :3].astype(np.float64)
    e = np.abs(np.asarray(got)[sel, :3].astype(np.float64) - want) / np.maximum(1.0, want)
    return float(e.max()), float(np.sqrt((e ** 2).mean()))


def bounds(restatement_max, restatement_rms):
    return max(2e-4, 2 * restatement_max), max(1e-5, 2 * restatement_rms)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CELLS = (64, 32)   # of the cases' catalogues: a footprint of a hundredth of a turn reaches both regimes


def _sky(min_footprint=DEFAULT_MIN_FOOTPRINT, background=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))):
    return dict(min_footprint=float(min_footprint), background=np.array(background, dtype=F))


def _stars_for(records, width, height, sky, seed, every=3, base=1500, extra_uv=(), base_flux=2e-4):
    """a catalogue's (uv, flux): `base` random stars, one star inside the tent of every `every`-th shaded record (a fraction of the
    footprint off its centre, of a flux that gives the pixel about one), and extra_uv"""
    rng = np.random.default_rng(seed)
    r = np.asarray(records)
    hu, hv = footprint64(r, width, height, sky["min_footprint"])
    pick = np.flatnonzero(r["terminated"] == 1)[::every]
    u = np.mod(r["tex_coord"][pick, 0] + rng.uniform(-1.2, 1.2, len(pick)) * hu[pick], 1.0)
    v = np.clip(r["tex_coord"][pick, 1] + rng.uniform(-1.2, 1.2, len(pick)) * hv[pick], 0.0, 1.0)
    flux = (4 * hu[pick] * hv[pick])[:, None] * rng.uniform(0.2, 1.5, (len(pick), 3))
    extra = np.asarray(extra_uv, dtype=np.float64).reshape(-1, 2)
    uv = np.concatenate([np.stack([u, v], axis=1), rng.random((base, 2)), extra])
    flux = np.concatenate([flux, rng.uniform(0, base_flux, (base, 3)), np.full((len(extra), 3), float(np.median(flux)) if len(flux) else base_flux)])
    uv = uv.astype(F)
    uv[uv[:, 0] >= 1, 0] = 0
    return uv, flux.astype(F)


def _case(name, width, height, records, sky=None, count=None, seed=1, cats="both", extra_uv=(), **features):
    sky = sky or _sky()
    made = {}
    for s, label in ((0, "far"), (1, "near")):
        if cats == "both" or cats == label:
            uv, flux = _stars_for(records, width, height, sky, 100 * seed + s, extra_uv=extra_uv)
            made[s] = catalogue(uv, flux, *CELLS)
    return dict(name=name, width=width, height=height, records=records, sky=sky, cats=(made.get(0), made.get(1)),
                count=len(records) if count is None else count, features={**dict(redshift=0, use_old_redshift=0), **features})


def spans(c):
    """(i1 - i0, j1 - j0) of a case's shaded records, the fp32 decision against the near catalogue's cells"""
    r = c["records"]
    hu, hv = footprint32(r, c["width"], c["height"], c["sky"]["min_footprint"])
    i0, i1, j0, j1, _ = regime32(r["tex_coord"][:, 0], r["tex_coord"][:, 1], hu, hv, *CELLS)
    sel = r["terminated"] == 1
    return (i1 - i0)[sel], (j1 - j0)[sel]


def _build_cases():
    out = []
    lm = am.linear_map
    # footprints at the floor: neighbours 1e-7 apart, under 2^-16 and under 2^-20
    u, v = lm(67, 5, (0.3137, 0.4219), (1e-7, 2e-8), (-3e-8, 1e-7))
    out.append(_case("floor_67x5", 67, 5, sm.make_records(67, 5, u, v), seed=1))
    out.append(_case("floor_2^-20_67x5", 67, 5, sm.make_records(67, 5, u, v), sky=_sky(2.0 ** -20, ((0.1, 0.2, 0.3), (0.3, 0.2, 0.1))), seed=2))
    # ordinary footprints: a fifth of a cell
    u, v = lm(67, 5, (0.3137, 0.4219), (0.0031, 0.0007), (-0.0011, 0.0043))
    out.append(_case("ordinary_67x5", 67, 5, sm.make_records(67, 5, u, v), seed=3))
    # the regime's two sides: 2 r_u cells_u = 3.55 cells, so that the span along u is 3 (near) or 4 (far) with the place in the cell ...
    u, v = lm(20, 12, (0.0131, 0.2117), (0.0273, 0.0005), (0.0004, 0.0271))
    out.append(_case("span_u_20x12", 20, 12, sm.make_records(20, 12, u, v), seed=4))
    # ... and the same along v: 2 r_v cells_v = 3.53 cells
    u, v = lm(20, 12, (0.4131, 0.1017), (0.0131, 0.0004), (0.0005, 0.0547))
    out.append(_case("span_v_20x12", 20, 12, sm.make_records(20, 12, u, v), seed=5))
    # hu = 0.5: neighbours half a turn away in u, the box is the whole turn
    u, v = lm(24, 9, (0.2113, 0.3831), (0.5, 0.0009), (0.5, 0.0113))
    out.append(_case("hu_half_24x9", 24, 9, sm.make_records(24, 9, u, v), seed=6))
    # the u seam (columns fall through 0 between 11 and 12) and both poles (rows 0 and 8), with stars on the seam's two sides and on the poles
    u = np.mod((np.arange(24)[None, :] - 11.5) * 0.0009 + (np.arange(9)[:, None] - 4) * 0.0002, 1.0)
    v = np.array([0.0, 2.0 ** -12, 0.013, 0.31, 0.5, 0.77, 0.991, 1 - 2.0 ** -12, 1.0])[:, None] + np.zeros((1, 24))
    on_the_edges = [(0.0, 0.0), (1 - 2.0 ** -24, 0.0), (0.0, 1.0), (1 - 2.0 ** -24, 1.0), (0.0, 0.31), (1 - 2.0 ** -24, 0.31), (0.0004, 0.5), (0.9996, 0.5)]
    out.append(_case("seam_and_poles_24x9", 24, 9, sm.make_records(24, 9, u, v), seed=7, extra_uv=on_the_edges))
    # ... and at the floor, where a seam pixel's tent is 2^-15 wide and a position rounded against the turn would show
    u = np.mod((np.arange(24)[None, :] - 11.5) * 2e-6 + (np.arange(9)[:, None] - 4) * 1e-6, 1.0)
    out.append(_case("seam_at_the_floor_24x9", 24, 9, sm.make_records(24, 9, u, v), seed=8, extra_uv=on_the_edges))
    # a tent's edge within an ulp of a star: a frame one pixel wide, rows 2^-10 apart in u (the tent is 2^-10 to either side), and
    # stars one float either side of every second pixel's two edges
    u = (0.25 + 2.0 ** -10 * np.arange(7))[:, None]
    v = (0.4 + 2.0 ** -9 * np.arange(7))[:, None]
    edges = []
    for k in (0, 2, 4, 6):
        for edge in (F(u[k, 0]) + F(2.0 ** -10), F(u[k, 0]) - F(2.0 ** -10)):
            edges += [(np.nextafter(F(edge), F(0)), v[k, 0]), (F(edge), v[k, 0]), (np.nextafter(F(edge), F(1)), v[k, 0])]
    out.append(_case("tent_edge_1x7", 1, 7, sm.make_records(1, 7, u, v), seed=9, extra_uv=edges))
    u, v = lm(1, 7, (0.6137, 0.2219), (0.0, 0.0), (0.0011, 0.0043))
    out.append(_case("frame_1x7", 1, 7, sm.make_records(1, 7, u, v), seed=10))
    # sides 0, 1, 2 and terminated 0, 1, 2 interleaved; another catalogue and another background on each side - and no far catalogue at all
    u, v = lm(24, 9, (0.45, 0.46), (0.004, 0.001), (0.001, 0.009))
    phase = (np.arange(24)[None, :] + 2 * np.arange(9)[:, None]) % 5
    rec = sm.make_records(24, 9, u, v, terminated=np.where(phase == 2, 0, np.where(phase == 4, 2, 1)))
    rec["side"] = (rec["sx"] + 2 * rec["sy"]) % 3
    two_skies = _sky(background=((0.02, 0.03, 0.08), (0.10, 0.04, 0.02)))
    out.append(_case("sides_and_black_24x9", 24, 9, rec, sky=two_skies, seed=11))
    out.append(_case("null_far_24x9", 24, 9, rec, sky=two_skies, seed=12, cats="near"))
    # a count short of the records
    u, v = lm(20, 12, (0.6, 0.2), (0.007, 0.002), (-0.003, 0.011))
    out.append(_case("short_count_20x12", 20, 12, sm.make_records(20, 12, u, v), count=96, seed=13))
    # redshift: z by column, both sides by row, both formulas
    z = np.resize(np.array(sm.REDSHIFT_Z), 24)[None, :] + np.zeros((9, 1))
    for old in (0, 1):
        u, v = lm(24, 9, (0.47, 0.44), (0.0045, 0.0012), (0.0013, 0.0097))
        rec = sm.make_records(24, 9, u, v, z_shift=z)
        rec["side"] = rec["sy"] % 2
        out.append(_case(f"redshift_{'old' if old else 'new'}_24x9", 24, 9, rec, sky=two_skies, seed=14 + old, redshift=1, use_old_redshift=old))
    for c in out:
        c["records"].setflags(write=False)
    return out


_cases = []


def cases():
    if not _cases:
        _cases.extend(_build_cases())
    return _cases


def case(name):
    return next(c for c in cases() if c["name"] == name)


def case_names():
    return [c["name"] for c in cases()]


def model_of(c):
    if "_model" not in c:
        c["_model"] = evaluate(c["records"], c["width"], c["height"], c["sky"], c["cats"], c["features"]["redshift"], c["features"]["use_old_redshift"])
        c["_model"].setflags(write=False)
    return c["_model"]


def restatement_of(c):
    if "_restatement" not in c:
        c["_restatement"] = restate32(c["records"], c["width"], c["height"], c["sky"], c["cats"], c["features"]["redshift"], c["features"]["use_old_redshift"])
        c["_restatement"].setflags(write=False)
    return c["_restatement"]


def table():
    lines = ["# the fp32 restatement (tests/star_sky_model.py restate32) against the float64 model, per synthetic case, every shaded record;",
             "# e = |got - want| / max(1, want)",
             "# case  records  far  max e  RMS e  -> the device's bounds max(2e-4, 2 max), max(1e-5, 2 RMS)"]
    for c in cases():
        mx, rm = errors(restatement_of(c), model_of(c), c["records"], c["count"])
        b = bounds(mx, rm)
        far = int((~regimes(c["records"], c["width"], c["height"], c["sky"], c["cats"]) & (c["records"]["terminated"] == 1)).sum())
        lines.append(f"{c['name']:26s} {len(c['records']):4d} {far:4d}  {mx:.2e}  {rm:.2e}  -> {b[0]:.1e} {b[1]:.1e}")
    return "\n".join(lines)


if __name__ == "__main__":
    print(table())
