"""A float64 model of the shading stage, and the synthetic records it is held against (tests/test_shading_model.py on the CPU,
tests/test_gpu_shading.py on the device).

The model restates the reference's `render` kernel (cl.cl:5453-5846, with read_mipmap 5421-5449, the colour helpers 326-350 and
5366-5413, circular_diff 3598-3610 and the image sampler of OpenCL 1.2, 8.2) from the reference's text, in numpy and in float64
throughout: atan2 / cos / sin for the footprint's angle, atan2(sin d, cos d) for the wrap, pow for the colour curves.  It shares no
arithmetic shortcut with kernels/shading.hip.  One place follows fp32, because there the reference's result is DEFINED by an fp32 value:
circular_diff forms d = float(2 pi b) - float(2 pi a) in fp32, and when |d| comes out as float(pi) = 3.14159274101257324 exactly (8.74e-8
above pi: v = 0.5 next to a black record at (0, 0)) sin d has the sign opposite to d's, so atan2(sin d, cos d) is pi - 8.74e-8 with the
OTHER sign.  The model takes that fp32 d, as a float64, through its own atan2(sin, cos) in exactly that case.

Frames one pixel wide or high: the reference reads the record before the buffer there; this project defines the missing neighbour to
be the pixel itself, and so does the model.

safe_mask() says, from the inputs alone and in float64, which records sit within rounding of a discontinuous decision (the probe
count's rounding, the coarsest-level test, the wrap's branch, the luminance gate, a probe on a mip's seam); those are run but not compared.

cases() is the seeded list of synthetic frames.  Records are analytic maps (u, v) = f(sx, sy), so neighbouring records are
consistent; the skies are white noise through pack_background, so a wrong texel, wrap or slice moves a pixel by tenths.
"""
import numpy as np

from oracle.refpipe import RENDER_DATA_DTYPE

PI_F32 = float(np.float32(np.pi))   # 3.14159274101257324, the fp32 value the exact case is defined by

# z_shift values of the redshift cases.  The issue's list is {-0.999, -0.99, -0.9, -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5, 3, 50, 1e4}; every
# one of them gives a finite frame in the reference object's own run (test_shading_model.py checks that where the object is built;
# calculate_render_data itself never stores a z below -0.999), so all twelve stay.
REDSHIFT_Z = [-0.999, -0.99, -0.9, -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5, 3.0, 50.0, 1e4]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _wrapped_difference(a32, b32):
    """circular_diff(a, b) with period 1 -> (difference, |d| is exactly float(pi), | |d| - pi |, the fp32 d)"""
    two_pi = 2 * np.pi
    g1 = (a32.astype(np.float64) * two_pi).astype(np.float32)
    g2 = (b32.astype(np.float64) * two_pi).astype(np.float32)
    d32 = (g2 - g1).astype(np.float64)
    exact = np.abs(d32) == PI_F32
    d = np.where(exact, d32, (b32.astype(np.float64) - a32.astype(np.float64)) * two_pi)
    near = np.abs(np.abs(np.where(exact, d32, d)) % two_pi - np.pi)
    return np.arctan2(np.sin(d), np.cos(d)) / two_pi, exact, near, d32


def _sample(skies, which, s, t, layer_f):
    """read_imagef with NORMALIZED | REPEAT | LINEAR on a 2D array (OpenCL 1.2, 8.2): skies [2][levels][h][w][4] in [0, 1]"""
    levels, h, w = skies.shape[1:4]
    layer = np.clip(np.rint(layer_f).astype(np.int64), 0, levels - 1)
    u, v = (s - np.floor(s)) * w, (t - np.floor(t)) * h
    i0f, j0f = np.floor(u - 0.5), np.floor(v - 0.5)
    a, b = (u - 0.5) - i0f, (v - 0.5) - j0f
    i0, j0 = i0f.astype(np.int64) % w, j0f.astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    a, b = a[..., None], b[..., None]
    return ((1 - a) * (1 - b) * skies[which, layer, j0, i0] + a * (1 - b) * skies[which, layer, j0, i1] +
            (1 - a) * b * skies[which, layer, j1, i0] + a * b * skies[which, layer, j1, i1])


def _read_mipmap(skies, which, px, py, lod):
    lod = np.maximum(lod, 0.0)
    px, py = np.fmod(px, 1.0), np.fmod(py, 1.0)
    lower, upper = np.floor(lod), np.ceil(lod)
    v1 = _sample(skies, which, px / 2.0 ** lower, py / 2.0 ** lower, lower)
    v2 = _sample(skies, which, px / 2.0 ** upper, py / 2.0 ** upper, upper)
    return v1 + (v2 - v1) * (lod - lower)[..., None]


def _srgb_to_lin(c):
    return np.where(c < 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def _lin_to_srgb(c):
    return np.where(c <= 0.0031308, c * 12.92, 1.055 * np.maximum(c, 0.0) ** (1 / 2.4) - 0.055)


def _energy_of(c):
    return c[..., 0] * 0.2125 + c[..., 1] * 0.7154 + c[..., 2] * 0.0721


def _redshift(rgb, z, use_old_redshift):
    """cl.cl:5697-5831 (DOMINANT_COLOUR off) -> (linear rgb, relative luminance before the shift)"""
    lin = _srgb_to_lin(rgb)
    test_wavelength = 555 / 299792458.0
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        local_wavelength = test_wavelength / (z + 1)
        lum = 0.2126 * lin[..., 0] + 0.7152 * lin[..., 1] + 0.0722 * lin[..., 2]
        new_lum = np.clip(local_wavelength ** 3 * lum / test_wavelength ** 3, 0.0, 1.0)
        gate = lum > 0.00001
        scaled = np.clip((new_lum / np.where(gate, lum, 1.0))[..., None] * lin, 0.0, 1.0)
        lin = np.where(gate[..., None], scaled, lin)
        energy = _energy_of(lin)
        red = np.array([1 / 0.2125, 0, 0]) * energy[..., None]
        blue = np.array([0, 0, 1 / 0.0721]) * energy[..., None]
        to_red = lin + (red - lin) * np.tanh(z)[..., None]
        col = lin + (blue - lin) * np.tanh(1 / (1 + z) - 1)[..., None]
        if not use_old_redshift:
            remaining = _energy_of(col) - _energy_of(np.clip(col, 0.0, 1.0))
            col = col.copy()
            col[..., 0] += remaining / 0.2125     # (red + green).xy = (1 / 0.2125, 1 / 0.7154)
            col[..., 1] += remaining / 0.7154
        lin = np.clip(np.where((z > 0)[..., None], to_red, col), 0.0, 1.0)
    return lin, lum


def evaluate(records, width, height, sky1, sky2, max_probes, redshift=0, use_old_redshift=0, linear_framebuffer=True):
    """every record shaded -> dict of per-record arrays (record order): `rgba` and the intermediates the tests and safe_mask read.
    linear_framebuffer: the reference's LINEAR_FRAMEBUFFER, which every program this project generates defines (as the reference's
    own metric_manager.hpp:78-81 does): the frame holds linear values; without it sRGB ones."""
    r = np.asarray(records)
    n = len(r)
    sx, sy = r["sx"].astype(np.int64), r["sy"].astype(np.int64)
    levels, bh, bw = sky1.shape[:3]
    assert sky2.shape == sky1.shape
    skies = np.stack([np.asarray(sky1), np.asarray(sky2)]).astype(np.float64) / 255.0
    which = np.where(r["side"] >= 1, 0, 1)
    dx = np.where(sx == width - 1, -1, 1)
    dy = np.where(sy == height - 1, -1, 1)
    beside = r["tex_coord"][sy * width + sx + (dx if width > 1 else 0)]
    below = r["tex_coord"][(sy + (dy if height > 1 else 0)) * width + sx]
    tl = r["tex_coord"]
    bias = 1.3
    diffs, exact, near, exact_sign = {}, np.zeros(n, bool), np.full(n, np.inf), np.zeros(n, np.int64)
    for key, other, axis, sign in (("du_dx", beside, 0, dx), ("dv_dx", beside, 1, dx), ("du_dy", below, 0, dy), ("dv_dy", below, 1, dy)):
        d, e, nr, d32 = _wrapped_difference(tl[:, axis], other[:, axis])
        exact_sign |= np.where(e, np.where(d32 > 0, 1, 2), 0)   # bit 0: a d of +float(pi), bit 1: of -float(pi)
        diffs[key] = sign * d / bias * (bw if axis == 0 else bh)
        exact |= e
        near = np.minimum(near, np.where(e, np.inf, nr))
    du_dx, dv_dx, du_dy, dv_dy = diffs["du_dx"], diffs["dv_dx"], diffs["du_dy"], diffs["dv_dy"]
    Ann = dv_dx * dv_dx + dv_dy * dv_dy + 1
    Bnn = -2 * (du_dx * dv_dx + du_dy * dv_dy)
    Cnn = du_dx * du_dx + du_dy * du_dy + 1
    F = Ann * Cnn - Bnn * Bnn / 4
    A, B, C = Ann / F, Bnn / F, Cnn / F
    root = np.sqrt((A - C) * (A - C) + B * B)
    major_raw = 1 / np.sqrt((A + C - root) / 2)
    minor_raw = 1 / np.sqrt((A + C + root) / 2)
    theta = np.arctan2(B, (A - C) / 2)
    major = np.maximum(major_raw, 1.0)
    minor = np.maximum(minor_raw, 1.0)
    major = np.maximum(major, minor)
    wanted = 2 * (major / minor) - 1
    rounded = np.floor(wanted + 0.5).astype(np.int64)
    probes = np.minimum(rounded, max_probes)
    grown = probes < wanted
    minor_used = np.where(grown, 2 * major / (probes + 1), minor)
    lod_raw = np.log2(minor_used)
    max_lod = levels - 1
    past = lod_raw > max_lod
    lod = np.where(past, max_lod, lod_raw)
    probes_used = np.where(past, 1, probes)
    lod = np.where(probes_used < 1, max_lod, lod)
    sxf, syf = tl[:, 0].astype(np.float64), tl[:, 1].astype(np.float64)
    single = _read_mipmap(skies, which, sxf, syf, lod)
    many = probes_used > 1
    line = 2 * (major - minor_used)
    div = np.where(many, probes_used - 1, 1)
    du, dv = np.cos(theta) * line / div, np.sin(theta) * line / div
    start = np.where(probes_used % 2 == 1, -2 * ((probes_used - 1) // 2), -2 * (probes_used // 2) - 1)
    total, accumulated = np.zeros((n, 4)), np.zeros(n)
    seam = np.full(n, np.inf)   # distance of the nearest computed probe position to a seam of the texture, in turns
    for cnt in range(int(probes_used.max()) if n else 0):
        live = many & (cnt < probes_used)
        current = start + 2 * cnt
        weight = np.where(live, np.exp(-2 * (current * current / 4.0) * (du * du + dv * dv) / (major * major)), 0.0)
        cu, cv = sxf + (current / 2.0) * (du / bw), syf + (current / 2.0) * (dv / bh)
        total += weight[:, None] * _read_mipmap(skies, which, cu, cv, lod)
        accumulated += weight
        moved = live & (current != 0)
        for pos in (cu, cv):
            seam = np.minimum(seam, np.where(moved, np.abs(pos - np.rint(pos)), np.inf))
    end = np.where(many[:, None], total / np.where(many, accumulated, 1.0)[:, None], single)
    rgb, lum = end[:, :3], np.full(n, np.nan)
    if redshift:
        rgb, lum = _redshift(rgb, r["z_shift"].astype(np.float64), use_old_redshift)
        if not linear_framebuffer:
            rgb = _lin_to_srgb(rgb)
    elif linear_framebuffer:
        rgb = _srgb_to_lin(rgb)
    rgba = np.concatenate([rgb, end[:, 3:]], axis=1)
    black = r["terminated"] != 1
    rgba[black] = (0, 0, 0, 1)
    return dict(rgba=rgba, black=black, sx=sx, sy=sy, wanted=wanted, rounded=rounded, probes=probes, probes_used=probes_used, grown=grown,
                capped=rounded > max_probes, lod_raw=lod_raw, lod=lod, past_coarsest=past, major=major, minor=minor_used,
                major_raw=major_raw, minor_raw=minor_raw, exact_pi=exact, exact_pi_sign=exact_sign, near_pi=near, luminance=lum, seam=seam, levels=levels,
                du_dx=du_dx, dv_dx=dv_dx, du_dy=du_dy, dv_dy=dv_dy)


def shade(records, width, height, sky1, sky2, max_probes, redshift=0, use_old_redshift=0, linear_framebuffer=True):
    """the frame [height][width][4] in float64 (pixels no record names stay NaN)"""
    e = evaluate(records, width, height, sky1, sky2, max_probes, redshift, use_old_redshift, linear_framebuffer)
    out = np.full((height, width, 4), np.nan)
    out[e["sy"], e["sx"]] = e["rgba"]
    return out


def safe_mask(records, width, height, sky1, sky2, max_probes, redshift=0, use_old_redshift=0, evaluated=None):
    """per record: False where a discontinuous decision of the stage sits within rounding of flipping (black records are safe: they
    take no decision).  The first five are the list of the stage's branches; the sixth is the sampler's own discontinuity - above
    level 0 a slice does not wrap onto itself (the mip sits in its corner with the edge replicated), so a probe whose COMPUTED
    position lands within 1e-6 of a seam reads another texel in fp32 than in float64.  (A probe at the record's own coordinates is
    not computed, and safe.)"""
    e = evaluated or evaluate(records, width, height, sky1, sky2, max_probes, redshift, use_old_redshift)
    wanted, probes = e["wanted"], e["probes"]
    scale = 1e-3 * np.maximum(wanted, 1.0)
    why = {"rounding": np.abs((wanted + 0.5) - np.rint(wanted + 0.5)) <= scale}            # the rounding of the probe count
    # probes < wanted.  The branch it guards is continuous: taken, the short radius becomes 2 long / (probes + 1), which differs from
    # the short radius by |wanted - probes| / (probes + 1) of it - so a flip moves the result by no more than the rounding that
    # caused it.  It is listed all the same, with the width of that rounding: wanted comes out of two square roots and four
    # quotients of fp32 values, a few 1e-7 of it; 1e-5 is some twenty times that.  (With the 1e-3 of the other tests every footprint
    # below 0.03 texels would be set aside - there the padding makes long / short = 1 + 1e-4 - and those are the commonest records of
    # a real frame.)  Where all four differences are exactly zero (a 1 x 1 frame) the radii are the same number in any precision.
    same = (e["du_dx"] == 0) & (e["dv_dx"] == 0) & (e["du_dy"] == 0) & (e["dv_dy"] == 0)
    why["probes_against_wanted"] = (np.abs(wanted - probes) <= 1e-5 * np.maximum(wanted, 1.0)) & ~same
    why["coarsest"] = np.abs(e["lod_raw"] - (e["levels"] - 1)) <= 1e-4                     # lod against the coarsest level
    why["near_pi"] = e["near_pi"] < 1e-4                                                   # the wrap's branch (not the exact case)
    if redshift:
        why["luminance"] = np.abs(e["luminance"] - 1e-5) <= 1e-6                           # the luminance gate
    why["seam"] = (e["seam"] <= 1e-6) & (e["lod"] > 0)
    unsafe = np.zeros(len(wanted), dtype=bool)
    for k in why:
        why[k] = why[k] & ~e["black"]
        unsafe |= why[k]
    e["unsafe_why"] = why
    return ~unsafe


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
SKY_SIZES = [(1, 1), (5, 1), (2, 2), (37, 19), (19, 70), (64, 33), (128, 64)]   # width x height
_skies = {}


def noise_sky(w, h, seed, quarter_black=False):
    """(packed [levels][h][w][4] uint8, read-only; levels): white noise, opaque; optionally the top-left quarter exactly black"""
    key = (w, h, seed, quarter_black)
    if key not in _skies:
        import geodesic_raytracing_amd as gra
        image = np.random.default_rng(seed).integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        image[..., 3] = 255
        if quarter_black:
            image[:h // 2, :w // 2, :3] = 0
        packed, levels = gra.pack_background(image)
        packed.setflags(write=False)
        _skies[key] = (packed, levels)
    return _skies[key]


def sky_pair(w, h, quarter_black=False):
    return noise_sky(w, h, 1000 * w + h, quarter_black)[0], noise_sky(w, h, 77000 + 1000 * w + h, quarter_black)[0]


def make_records(width, height, u, v, z_shift=0.0, terminated=1, side=1):
    """records in pixel order from [height][width] arrays (or scalars); u and v are stored as they are given, rounded to fp32"""
    r = np.zeros(width * height, dtype=RENDER_DATA_DTYPE)
    yy, xx = np.mgrid[0:height, 0:width]
    full = lambda a, t: np.broadcast_to(np.asarray(a, dtype=t), (height, width)).reshape(-1)
    r["sx"], r["sy"] = xx.reshape(-1), yy.reshape(-1)
    r["tex_coord"][:, 0], r["tex_coord"][:, 1] = full(u, np.float64).astype(np.float32), full(v, np.float64).astype(np.float32)
    r["z_shift"], r["terminated"], r["side"] = full(z_shift, np.float32), full(terminated, np.int32), full(side, np.int32)
    black = r["terminated"] != 1
    r["tex_coord"][black] = 0
    r["z_shift"][black] = 0
    return r


def grid_map(width, height, sky_w, sky_h, along_x, along_y, angle_deg, origin=(0.3137, 0.4219)):
    """(u, v) of a frame whose pixel (sx, sy) looks at  origin + X(sx) e1 + Y(sy) e2  of the sky, in texels: X and Y the running sums
    of `along_x` [width] and `along_y` [height] times the filter bias 1.3, e1 = (cos, sin) of the angle, e2 = (-sin, cos).  The forward
    differences of neighbouring records are then along_x[sx] e1 and along_y[sy] e2 texels after the kernel's division by 1.3."""
    t = np.deg2rad(angle_deg)
    X = 1.3 * np.concatenate([[0.0], np.cumsum(np.broadcast_to(along_x, width))[:-1]])
    Y = 1.3 * np.concatenate([[0.0], np.cumsum(np.broadcast_to(along_y, height))[:-1]])
    px = X[None, :] * np.cos(t) - Y[:, None] * np.sin(t)
    py = X[None, :] * np.sin(t) + Y[:, None] * np.cos(t)
    return np.mod(origin[0] + px / sky_w, 1.0), np.mod(origin[1] + py / sky_h, 1.0)


def _case(name, width, height, records, sky, max_probes=8, count=None, **features):
    sky1, sky2 = sky
    return dict(name=name, width=width, height=height, records=records, sky1=sky1, sky2=sky2, levels=sky1.shape[0], max_probes=max_probes,
                count=len(records) if count is None else count, features={**dict(redshift=0, use_old_redshift=0), **features})


ANISOTROPY_ANGLES = [0, 30, 45, 90, 135]
ANISOTROPY_PROBES = [1, 2, 3, 4, 8, 16]


def anisotropy_records(angle, sky_w=128, sky_h=64):
    """16 x 9: the long axis (along the frame's x, turned by `angle` on the sky) from 24 down to 6 texels across the columns, the short
    one from 0.95 to 0.08 of 24 texels down the rows: long : short from 1 : 1 to 1 : 12, every probe count from 1 to 16 and beyond.
    24 texels: a difference wraps at half the sky, 64 / 2 / 1.3 texels on the 64 rows of the largest sky; and norm = a c - b^2 / 4
    cancels for long rotated footprints, which is the reference's conditioning and not the subject here."""
    long_axis = np.linspace(24.0, 6.0, 16) + 0.333
    short_axis = 24.0 / np.array([1.05, 1.6, 2.3, 3.2, 4.5, 6.3, 8.8, 12.4, 12.4])   # (the last row looks back at the one before)
    return make_records(16, 9, *grid_map(16, 9, sky_w, sky_h, long_axis, short_axis, angle))


def _build_cases():
    out = []
    rng = np.random.default_rng(20240607)
    # magnification: the neighbours' distance swept from 0.01 to 300 texels across 64 columns, the same along the rows.  A wrapped
    # difference is at most half the sky, so a footprint wider than that aliases (which is what the kernel's wrap of |d| > pi is for):
    # on 128 x 64 lod runs from 0 to ~5.5 of 6, on the 1 x 1 sky (one level) every footprint above one texel is past the coarsest level
    for w, h in ((128, 64), (37, 19), (2, 2), (1, 1)):
        step = 0.01 * (300 / 0.01) ** (np.arange(64) / 63.0)
        X = 1.3 * np.concatenate([[0.0], np.cumsum(step)[:-1]])
        u = np.mod(0.113 + X[None, :] / w + np.zeros((8, 1)), 1.0)
        v = np.mod(0.371 + (np.arange(8)[:, None] - 3.5) * 1.3 * step[None, :] / h, 1.0)
        out.append(_case(f"magnification_{w}x{h}", 64, 8, make_records(64, 8, u, v), sky_pair(w, h)))
    # anisotropy
    for angle in ANISOTROPY_ANGLES:
        for probes in ANISOTROPY_PROBES:
            out.append(_case(f"anisotropy_{angle}deg_p{probes}", 16, 9, anisotropy_records(angle), sky_pair(128, 64), max_probes=probes))
    # seams: u falls through 0 between columns 7 and 8 and v between rows 3 and 4 (and both at the corner), upwards and downwards;
    # moderate footprints so that probes straddle the seam; on skies that are not powers of two, and taller than wide
    for (w, h), direction in (((37, 19), 1), ((19, 70), -1), ((64, 33), 1), ((5, 1), -1)):
        ax, ay = 0.013 * direction, 0.021 * direction
        u = np.mod((np.arange(16)[None, :] - 7.5) * ax + (np.arange(8)[:, None] - 3.5) * 0.003, 1.0)
        v = np.mod((np.arange(8)[:, None] - 3.5) * ay + (np.arange(16)[None, :] - 7.5) * 0.002, 1.0)
        out.append(_case(f"seams_{w}x{h}_{'up' if direction > 0 else 'down'}", 16, 8, make_records(16, 8, u, v), sky_pair(w, h)))
    # ... and records whose coordinates are exactly 0, 1, the float below 1 and 0.5, in every pairing (a 16 x 8 frame: u by column, v by
    # row, each value next to itself and next to another), a checkerboard of exact values among slightly moved ones
    below_one = np.nextafter(np.float32(1), np.float32(0))
    special = np.array([0.0, 1.0, below_one, 0.5, 0.5, below_one, 1.0, 0.0])
    for w, h in ((128, 64), (37, 19)):
        jitter = 0.0047 * rng.random((8, 16))
        keep = (np.arange(8)[:, None] + np.arange(16)[None, :]) % 2 == 0
        u = np.where(keep, np.tile(special, 2)[None, :], np.mod(np.tile(special, 2)[None, :] + jitter, 1.0))
        v = np.where(keep, special[:, None], np.mod(special[:, None] + jitter[:, ::-1], 1.0))
        out.append(_case(f"seams_exact_{w}x{h}", 16, 8, make_records(16, 8, u, v), sky_pair(w, h)))
    # shadow_edge: 12 x 8 (even-rowed); v = 0.5 exactly on rows 3 and 4, black records (terminated 0 and 2) right of and below them:
    # d = -float(pi) for v (0.5 -> 0) and, where u = 0.5 too, for u.  d = +float(pi) is the same step the other way: records at 0
    # exactly whose neighbour is at 0.5 (row 0 above row 1, and one pair along row 6 for u)
    u = np.mod(0.21 + 0.0113 * np.arange(12)[None, :] + 0.0031 * np.arange(8)[:, None], 1.0)
    v = np.mod(0.18 + 0.0702 * np.arange(8)[:, None] + 0.0017 * np.arange(12)[None, :], 1.0)
    v[3:5, :] = 0.5
    u[3:5, 4:6] = 0.5
    v[0, :] = 0.0          # d = +float(pi) ...
    v[1, 2:9] = 0.5        # ... towards these
    u[6, 3], u[6, 4] = 0.0, 0.5
    term = np.ones((8, 12), dtype=np.int32)
    term[3, 6:], term[4, 7:] = 0, 2
    term[5, 1:4] = 2
    term[2, 10] = 0
    out.append(_case("shadow_edge", 12, 8, make_records(12, 8, u, v, terminated=term), sky_pair(128, 64), max_probes=16))
    # sides: 0, 1 and 2 interleaved over two different skies
    rec = anisotropy_records(30)
    rec["side"] = (rec["sx"] + 2 * rec["sy"]) % 3
    out.append(_case("sides", 16, 9, rec, sky_pair(128, 64)))
    # last column and row: a steep gradient that changes along the frame, so that the mirrored neighbour's difference is not the
    # forward one's; and the frames that have no neighbour at all
    for w, h in ((16, 8), (67, 9), (9, 8), (2, 2), (1, 1), (33, 1), (1, 33), (24, 40)):
        ax = np.linspace(1.0, 9.0, w) if w > 1 else np.array([3.0])
        ay = np.linspace(6.0, 0.5, h) if h > 1 else np.array([2.0])
        out.append(_case(f"last_column_and_row_{w}x{h}", w, h, make_records(w, h, *grid_map(w, h, 64, 33, ax, ay, 20)), sky_pair(64, 33)))
    # redshift: the anisotropy records, z by column
    z = np.resize(np.array(REDSHIFT_Z), 16)[None, :]
    for old in (0, 1):
        for black in (False, True):
            rec = anisotropy_records(45)
            rec["z_shift"] = np.broadcast_to(z.astype(np.float32), (9, 16)).reshape(-1)
            out.append(_case(f"redshift_{'old' if old else 'new'}_{'quarter_black' if black else 'noise'}", 16, 9, rec,
                             sky_pair(128, 64, quarter_black=black), redshift=1, use_old_redshift=old))
    # ... and unfiltered lookups (one probe at level 0) into the quarter-black sky, so that exactly black texels reach the gate
    u, v = np.meshgrid((np.arange(16) + 0.5) / 16 * 0.6, (np.arange(9) + 0.5) / 9 * 0.6)
    rec = make_records(16, 9, u, v, z_shift=np.broadcast_to(z, (9, 16)))
    for old in (0, 1):
        out.append(_case(f"redshift_{'old' if old else 'new'}_gate", 16, 9, rec, sky_pair(128, 64, quarter_black=True), redshift=1, use_old_redshift=old))
    # short_count: two thirds of the records are shaded
    rec = anisotropy_records(135)
    out.append(_case("short_count", 16, 9, rec, sky_pair(128, 64), count=96))
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
    """(evaluate() of a case, its safe mask), cached on the case"""
    if "_model" not in c:
        args = (c["records"], c["width"], c["height"], c["sky1"], c["sky2"], c["max_probes"], c["features"]["redshift"], c["features"]["use_old_redshift"])
        e = evaluate(*args)
        c["_model"] = (e, safe_mask(*args, evaluated=e))
    return c["_model"]


def errors(got, c):
    """(max |rgb error|, RMSE) of a frame [h][w][4] against the model over the case's safe, shaded records"""
    e, safe = model_of(c)
    sel = safe.copy()
    sel[c["count"]:] = False
    assert sel.any(), c["name"]
    d = got[e["sy"][sel], e["sx"][sel], :3].astype(np.float64) - e["rgba"][sel, :3]
    return float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
