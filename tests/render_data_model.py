"""A float64 model of the render-data stage, and the hand-made rays it is held against (tests/test_render_data_model.py on the
CPU, tests/test_gpu_render_data.py on the device).

The model restates make_render_data (kernels/trace.hip; the reference's calculate_render_data, cl.cl:5146-5212, with
fix_ray_position 211-263, get_texture_constant_theta_rotation / angle_to_tex 5024-5100 and the tetrad of 1647-1861) for one list
of rays, in numpy and float64.  It follows the discrete algorithm, not the physics: the same branches in the same order.
  * The metric tensor and the chart -> polar map come from Metric.evaluate (the host's double evaluator of the generated
    expressions, which tests/test_codegen.py ties to the macro strings); closed_form() below states g and the map of
    Schwarzschild, Kerr in Boyer-Lindquist coordinates and Minkowski by hand, and the CPU test holds the evaluator to them.
  * The velocity's transform to polar coordinates is the Jacobian of that map by central differences, step
    h_k = JACOBIAN_STEP * max(1, |x_k|) = 1e-5 max(1, |x_k|): the truncation error is h^2 f''' / 6 ~ 2e-11 of the entry for maps whose
    third derivatives are O(1 / x^3) (sqrt, atan2, log), the rounding error 2^-53 |f| / h ~ 1e-11 |f|; both are four orders below
    the fp32 rounding of the generated derivative.  (A difference of phi across atan2's cut is taken modulo 2 pi.  On the axis of a
    Cartesian chart the map has no derivative; the cases keep such points inside the universe, where the velocity is not read.)
  * Two fp32 numbers are taken as the fp32 values they are defined by: pi in angle_to_tex is float(pi) = 3.14159274 (theta =
    float(pi) exactly takes the wrap branch and comes out as 0), and universe_size is the float the feature struct holds.

safe_mask() says, from the model's own intermediates, which records sit within fp32 rounding of a branch or are ill-conditioned
as inputs; those are run, and checked for flags and range, but not compared.  The margins (relative unless said otherwise):
  MARGIN_R      1e-6     |r| against universe_size, SINGULAR_TERMINATOR and 1 (r is a square root of a sum of fp32 squares in a
                         Cartesian chart, 2e-7 at most; in a polar chart it is the input itself and the test is exact)
  MARGIN_SIGN   1e-6     absolute, r against 0 (side, and the sign fix_ray_position carries through)
  MARGIN_DISCRIM         discrim = b^2 - 4 c is a difference of two fp32 numbers of size 4 |pos|^2: its fp32 error is
                         ~2^-22 * 4 |pos|^2 whatever its value.  A record is unsafe when that error exceeds 1e-3 of |discrim| (the
                         root moves by 5e-4 of itself, the hit point along the ray by that much) - this sets aside every
                         overshoot beyond some 30 universe radii: there the REFERENCE's own fp32 quadratic has lost its
                         discriminant (at 1e4 radii its rounding is 1e5 times its value; the de Sitter fixture is held to the
                         ill-conditioned rule for the same reason) and the kernel, restating it, can do no better.
  MARGIN_ROOTS  1e-4     | |t0| - |t1| | against max(|t0|, |t1|)
  MARGIN_THETA  2e-6     absolute, theta against the multiples of pi other than 0 (fmodf of a theta of two turns carries 2 * 1.7e-7
                         from float(2 pi) - 2 pi, and the theta itself 2e-7; through theta = 0 the map is continuous: no branch).
                         This includes the south pole of a Cartesian chart: atan2f there returns float(pi), which takes the wrap.
  MARGIN_GTT    5e-7     absolute, g_tt against -1e-5 (g_tt = rs / r - 1 in fp32: 1.2e-7)
  MARGIN_Z      1e-4     absolute, z against -0.999 (the stage's own tolerance on z)
and, conditioning: the model is evaluated again on position and velocity moved by one fp32 ulp in every component (all up, all
down, and two fixed random sign patterns); a record whose tex_coord * max(sin theta, 1e-3) moves by more than 1e-6 or whose
z moves by more than 5e-5 (1 + |z|) - half the floors of tests/test_gpu_render_data.py - or which changes branch, is unsafe.

cases() is the seeded list.  Every case is at most 67 x 40 records; sx, sy are a permutation of the frame and initial_quat is a
random unit quaternion per ray."""
import os
import re

import numpy as np

import geodesic_raytracing_amd as gra
from oracle.refpipe import LIGHTRAY_DTYPE, RENDER_DATA_DTYPE, pack_features
from model_common import (JACOBIAN_STEP, _cartesian_to_polar, _frame_basis_with_swap, _jacobian_of, _polar_to_cartesian, _rot_quat,  # noqa: F401
                          _spherical_velocity_to_cartesian)
from shading_model import REDSHIFT_Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "geodesic_raytracing_amd", "scripts")
PI_F32 = float(np.float32(np.pi))
MARGIN_R, MARGIN_SIGN, MARGIN_DISCRIM, MARGIN_ROOTS, MARGIN_THETA, MARGIN_GTT, MARGIN_Z = 1e-6, 1e-6, 1e-3, 1e-4, 2e-6, 5e-7, 1e-4
TEX_FLOOR, Z_FLOOR = 2e-6, 1e-4           # the stage's tolerances (tests/test_gpu_parity.py), the floors of the device's bounds
FIX_NONE, FIX_UNIVERSE, FIX_TERMINATOR = 0, 1, 2
PATH_NONE, PATH_SHORTCUT, PATH_FULL, PATH_DEGENERATE = 0, 1, 2, 3


# ---- programs ----------------------------------------------------------------------------------------------------------------------
# name -> (script, $cfg overrides, macros appended to the script's argument string).  scripts/ has no Kerr metric in ingoing
# coordinates; its horizon-penetrating chart is schwarzschild_ingoing_ef, whose settings say traversable but not singular - and
# metric_codegen.cpp writes TRAVERSABLE_EVENT_HORIZON only for a singular metric, so as it stands that program returns early at
# |r| <= 1 like any other.  The SINGULAR && TRAVERSABLE_EVENT_HORIZON branch, and a redshift inside a horizon, need a program that
# declares both: the same script's argument string with the three macros metric_codegen.cpp writes for "singular": true,
# "singular_terminator": 1.0 - the way a fixture of one of the reference's scripts brings its own string.
PROGRAMS = {
    "kerr_boyer": ("kerr_boyer", dict(a=0.45), ""),
    "kerr_boyer_near_extremal": ("kerr_boyer", dict(a=0.4999), ""),
    "ingoing_ef_singular": ("schwarzschild_ingoing_ef", {}, " -DSINGULAR -DSINGULAR_TERMINATOR=1.0f -DTRAVERSABLE_EVENT_HORIZON"),
    "schwarzschild": ("schwarzschild", {}, ""),
    "kerr_schild": ("kerr_schild", {}, ""),
    "wormhole": ("wormhole", {}, ""),
    "cosmic_string": ("cosmic_string", {}, ""),
}
REFERENCE_TAGS = {"kerr_boyer": "kerr_boyer_script", "kerr_boyer_near_extremal": "kerr_boyer_script", "schwarzschild": "schwarzschild_script"}   # oracle/_ref, where built
_programs = {}


class ProgramOf:
    """the metric of a program, its $cfg values, its argument string and the macros make_render_data reads"""

    def __init__(self, name):
        script, overrides, extra = PROGRAMS[name]
        self.name, self.metric = name, gra.Metric(script, SCRIPTS)
        self.cfg = self.metric.cfg_values(**overrides)
        self.argument_string = self.metric.argument_string() + extra
        tokens = self.argument_string.split()
        self.constant_theta = "-DGENERIC_CONSTANT_THETA" in tokens
        self.singular = "-DSINGULAR" in tokens
        self.traversable = "-DTRAVERSABLE_EVENT_HORIZON" in tokens
        self.terminator = None
        for t in tokens:
            m = re.fullmatch(r"-DSINGULAR_TERMINATOR=([0-9.eE+-]+)f?", t)
            if m:
                self.terminator = float(np.float32(float(m.group(1))))

    def to_polar(self, x):
        return self.metric.evaluate(gra.EVAL_TO_POLAR, x, cfg_values=self.cfg or None)

    def g(self, x):
        return self.metric.evaluate(gra.EVAL_METRIC_TENSOR, x, cfg_values=self.cfg or None).reshape(4, 4)


def program(name):
    if name not in _programs:
        _programs[name] = ProgramOf(name)
    return _programs[name]


def closed_form(name, x, cfg):
    """(g [4][4], polar [4]) of the built-in metrics written by hand, at chart position x (t, ...), rs and a from cfg"""
    t, r, th, ph = x
    g = np.zeros((4, 4))
    if name == "minkowski":                       # Cartesian chart (t, x, y, z)
        g[np.arange(4), np.arange(4)] = (-1, 1, 1, 1)
        X, Y, Z = x[1:]
        return g, np.array([t, np.sqrt(X * X + Y * Y + Z * Z), np.arctan2(np.sqrt(X * X + Y * Y), Z), np.arctan2(Y, X)])
    if name == "schwarzschild":                   # rs = 1
        g[0, 0], g[1, 1], g[2, 2], g[3, 3] = -(1 - 1 / r), 1 / (1 - 1 / r), r * r, r * r * np.sin(th) ** 2
        return g, np.array(x, dtype=np.float64)
    if name == "kerr_boyer":
        rs, a = cfg
        rho2, delta, s2 = r * r + a * a * np.cos(th) ** 2, r * r - rs * r + a * a, np.sin(th) ** 2
        g[0, 0], g[1, 1], g[2, 2] = -(1 - rs * r / rho2), rho2 / delta, rho2
        g[3, 3] = (r * r + a * a + rs * r * a * a * s2 / rho2) * s2
        g[0, 3] = g[3, 0] = -rs * r * a * s2 / rho2
        return g, np.array(x, dtype=np.float64)
    raise KeyError(name)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _fix_ray_position(polar_pos, polar_vel, radius, constant_theta, out):
    """fix_ray_position and fix_ray_position_cart; the discriminant, both roots and the cancellation's size go to `out`"""
    sgn = np.sign(polar_pos[0])
    cpos, vel = polar_pos.copy(), polar_vel.copy()
    cpos[0] = abs(cpos[0])
    vel[0] *= sgn
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cart_vel, pos = _spherical_velocity_to_cartesian(cpos, vel), _polar_to_cartesian(cpos)
        v = cart_vel / np.sqrt(cart_vel @ cart_vel)
        b = 2 * (v @ pos)
        c = pos @ pos - radius * radius
        discrim = b * b - 4 * c
        out["discrim"], out["discrim_scale"] = discrim, b * b + 4 * (pos @ pos) + 4 * radius * radius
        if discrim < 0:
            fixed = pos
        else:
            sq = np.sqrt(discrim)
            t0, t1 = (-b - sq) / 2, (-b + sq) / 2
            out["t0"], out["t1"] = t0, t1
            fixed = pos + (t0 if abs(t0) < abs(t1) else t1) * v
        res = _cartesian_to_polar(fixed)
    if constant_theta:
        res[1] = np.pi / 2
    res[0] *= sgn
    return res


def _timelike_leg(g):
    """e[0] of calculate_tetrads(position, no speed, no orientation) at a position that is not degenerate"""
    which, e = _frame_basis_with_swap(g, 0)
    if which != 0:
        _, e = _frame_basis_with_swap(g, which)
    with np.errstate(invalid="ignore"):
        return 1.0 * e[0] + 0.0 * e[1] + 0.0 * e[2] + 0.0 * e[3]     # the boost by a speed of zero (a leg that is not finite spoils e0)


def _jacobian(prog, x, p0):
    return _jacobian_of(prog.to_polar, x)


def angle_to_tex(theta, phi):
    with np.errstate(invalid="ignore"):
        thetaf, phif = np.fmod(theta, 2 * PI_F32), phi
        wrapped = bool(thetaf >= PI_F32)
        if wrapped:
            phif, thetaf = phif + PI_F32, thetaf - PI_F32
        phif = np.fmod(phif, 2 * PI_F32)
    return np.array([phif / (2 * PI_F32) + 0.5, thetaf / PI_F32]), wrapped


def _one(prog, universe, pos, vel, quat, ku, running):
    """make_render_data of one ray with terminated == 1 -> dict"""
    o = dict(tex=np.zeros(2), z=0.0, z_raw=np.nan, side=1, fix=FIX_NONE, discrim=np.nan, discrim_scale=np.nan, t0=np.nan, t1=np.nan,
             theta_in=np.nan, theta=np.nan, phi=np.nan, wrapped=False, g_tt=np.nan, path=PATH_NONE, early=False, r=np.nan, r_fixed=np.nan,
             z_shortcut=np.nan, z_full=np.nan)
    p = prog.to_polar(pos)
    o["r"], o["theta_in"] = p[1], p[2]
    position = p.copy()
    velocity = None
    needs_velocity = abs(p[1]) >= universe or (prog.singular and prog.traversable and abs(p[1]) < prog.terminator)
    if needs_velocity:
        velocity = _jacobian(prog, pos, p) @ vel
    if prog.constant_theta:
        position[2] = np.pi / 2
        if velocity is not None:
            velocity[2] = 0.0
    if abs(position[1]) >= universe:
        position[1:] = _fix_ray_position(position[1:], velocity[1:], universe, prog.constant_theta, o)
        o["fix"] = FIX_UNIVERSE
    if prog.singular and prog.traversable and abs(position[1]) < prog.terminator:
        position[1:] = _fix_ray_position(position[1:], velocity[1:], prog.terminator, prog.constant_theta, o)
        o["fix"] = FIX_TERMINATOR
    npolar = position[1:]
    if prog.constant_theta:
        npolar = _cartesian_to_polar(_rot_quat(_polar_to_cartesian(position[1:]), quat))
    o["r_fixed"] = npolar[0]
    o["side"] = 0 if p[1] < 0 else 1
    if not prog.traversable and abs(npolar[0]) <= 1:
        o["early"] = True
        return o
    g = prog.g(pos)
    o["g_tt"] = g[0, 0]
    degenerate = not np.isfinite(pos).all()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        def z_of(e0):
            return ((vel / running) @ (g @ e0)) / ku - 1
        shortcut = np.array([1.0, 0, 0, 0]) / np.sqrt(abs(g[0, 0]))
        if degenerate:
            o["path"], e0 = PATH_DEGENERATE, np.array([1.0, 0, 0, 0])
        elif g[0, 0] < -0.00001:
            o["path"], e0 = PATH_SHORTCUT, shortcut
            o["z_shortcut"], o["z_full"] = z_of(shortcut), z_of(_timelike_leg(g))
        else:
            o["path"], e0 = PATH_FULL, _timelike_leg(g)
        o["z_raw"] = z_of(e0)
    o["z"] = float(np.fmax(o["z_raw"], -0.999))
    o["theta"], o["phi"] = npolar[1], npolar[2]
    o["tex"], o["wrapped"] = angle_to_tex(npolar[1], npolar[2])
    return o


_KEYS = ["z", "z_raw", "side", "fix", "discrim", "discrim_scale", "t0", "t1", "theta_in", "theta", "phi", "wrapped", "g_tt", "path", "early", "r",
         "r_fixed", "z_shortcut", "z_full"]


def evaluate(prog, rays, universe, position=None, velocity=None):
    """every ray through the model -> dict of per-ray arrays: the record's fields (tex [n][2], z, side, terminated, sx, sy) and the
    intermediates.  `position` / `velocity` replace the rays' own (float64 [n][4]: the conditioning probe of safe_mask)."""
    n = len(rays)
    universe = float(np.float32(universe))
    pos = rays["position"].astype(np.float64) if position is None else position
    vel = rays["velocity"].astype(np.float64) if velocity is None else velocity
    out = {k: np.zeros(n, dtype=np.float64 if k not in ("side", "fix", "path", "wrapped", "early") else np.int64) for k in _KEYS}
    out["tex"] = np.zeros((n, 2))
    out["side"][:] = 1
    for k in ("z_raw", "discrim", "discrim_scale", "t0", "t1", "theta_in", "theta", "phi", "g_tt", "r", "r_fixed", "z_shortcut", "z_full"):
        out[k][:] = np.nan
    for i in np.flatnonzero(rays["terminated"] == 1):
        o = _one(prog, universe, pos[i], vel[i], rays["initial_quat"][i].astype(np.float64), float(rays["ku_uobsu"][i]),
                 float(rays["running_dlambda_dnew"][i]))
        out["tex"][i] = o["tex"]
        for k in _KEYS:
            out[k][i] = o[k]
    out["terminated"], out["sx"], out["sy"] = rays["terminated"].copy(), rays["sx"].copy(), rays["sy"].copy()
    out["live"] = rays["terminated"] == 1
    return out


def circ_diff(a, b):
    d = np.abs(a - b) % 1.0
    return np.minimum(d, 1.0 - d)


def sin_weight(e):
    """max(sin theta, 1e-3) of the model's sky coordinate, as tests/test_gpu_parity.py::test_render_data weighs its bound"""
    with np.errstate(invalid="ignore"):
        return np.maximum(np.abs(np.sin(np.pi * e["tex"][:, 1])), 1e-3)


def _ulp(a):
    a32 = a.astype(np.float32)
    return (np.nextafter(np.abs(a32), np.float32(np.inf)) - np.abs(a32)).astype(np.float64)


def safe_mask(prog, rays, universe, e):
    """per record: False within rounding of a branch, or ill-conditioned as an input (module docstring); e["unsafe_why"] says which"""
    n = len(rays)
    live = e["live"]
    universe = float(np.float32(universe))
    r, why = np.abs(e["r"]), {}
    with np.errstate(invalid="ignore", divide="ignore"):
        near = lambda x, edge, m: np.abs(x - edge) <= m * edge
        why["r_universe"] = near(r, universe, MARGIN_R)
        why["r_terminator"] = near(r, prog.terminator, MARGIN_R) if (prog.singular and prog.traversable) else np.zeros(n, bool)
        why["r_one"] = near(np.abs(e["r_fixed"]), 1.0, MARGIN_R) if not prog.traversable else np.zeros(n, bool)
        why["r_sign"] = r <= MARGIN_SIGN
        ran = e["fix"] != FIX_NONE
        why["discrim"] = ran & (e["discrim_scale"] * 2.0 ** -22 >= MARGIN_DISCRIM * np.abs(e["discrim"]))
        t0, t1 = np.abs(e["t0"]), np.abs(e["t1"])
        why["roots"] = ran & (np.abs(t0 - t1) <= MARGIN_ROOTS * np.maximum(t0, t1))
        computed = live & (e["early"] == 0)
        k = np.rint(e["theta"] / np.pi)
        why["theta"] = computed & (np.abs(e["theta"] - k * np.pi) <= MARGIN_THETA) & (k != 0)
        why["g_tt"] = computed & (np.abs(e["g_tt"] + 1e-5) <= MARGIN_GTT)
        why["z_clamp"] = computed & (np.abs(e["z_raw"] + 0.999) <= MARGIN_Z)
        # the shortcut's claim fails where the full construction is itself not finite: at sin theta = 0 exactly on a polar chart
        # g_phiphi = 0, Gram-Schmidt divides by it, and the boost by a speed of zero (0 * NaN) spoils e0 - the reference's z there is
        # the clamp's -0.999 by way of fmax(NaN, .), the kernel's shortcut returns the finite value.  No traced ray ends there.
        why["full_tetrad_not_finite"] = computed & (e["path"] == PATH_SHORTCUT) & np.isfinite(e["z_shortcut"]) & ~np.isfinite(e["z_full"])
    # conditioning: one fp32 ulp in every component of position and velocity
    pos, vel = rays["position"].astype(np.float64), rays["velocity"].astype(np.float64)
    up, uv = _ulp(pos), _ulp(vel)
    rng = np.random.default_rng(97)
    moved = np.zeros(n, bool)
    w = sin_weight(e)
    for signs in (np.ones((n, 8)), -np.ones((n, 8)), rng.choice([-1.0, 1.0], (n, 8)), rng.choice([-1.0, 1.0], (n, 8))):
        p = evaluate(prog, rays, universe, pos + signs[:, :4] * up, vel + signs[:, 4:] * uv)
        with np.errstate(invalid="ignore"):
            dtex = (circ_diff(p["tex"], e["tex"]) * w[:, None]).max(axis=1)
            dz = np.abs(p["z"] - e["z"]) / (1 + np.abs(e["z"]))
            branch = (p["fix"] != e["fix"]) | (p["path"] != e["path"]) | (p["early"] != e["early"]) | (p["side"] != e["side"]) | (p["wrapped"] != e["wrapped"])
            moved |= ~(dtex <= TEX_FLOOR / 2) | ~(dz <= Z_FLOOR / 2) | branch
    finite = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1)
    why["conditioning"] = moved & finite        # (a degenerate ray takes no decision that rounding could flip: test_degenerate)
    unsafe = np.zeros(n, bool)
    for key in why:
        why[key] = np.nan_to_num(why[key]).astype(bool) & live
        unsafe |= why[key]
    e["unsafe_why"] = why
    return ~unsafe


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
UNIVERSE = 20.0
W, H = 37, 11                # 407 records: odd, no multiple of 64, two workgroups of gr_calculate_render_data
N = W * H


def make_rays(rng, position, velocity, ku=None, running=None, terminated=None, width=W, height=H):
    n = len(position)
    assert n == width * height
    rays = np.zeros(n, dtype=LIGHTRAY_DTYPE)
    rays["position"], rays["velocity"] = np.asarray(position, dtype=np.float32), np.asarray(velocity, dtype=np.float32)
    q = rng.normal(size=(n, 4))
    rays["initial_quat"] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rays["acceleration"] = rng.normal(size=(n, 4))
    rays["ku_uobsu"] = rng.uniform(0.5, 2.0, n) if ku is None else ku
    rays["running_dlambda_dnew"] = 1.0 if running is None else running
    rays["terminated"] = 1 if terminated is None else terminated
    slot = rng.permutation(n)
    rays["sx"], rays["sy"] = slot % width, slot // width
    return rays


def _case(name, prog, rays, reaches, universe=UNIVERSE, width=W, height=H, degenerate=False):
    rays.setflags(write=False)
    return dict(name=name, program=prog, rays=rays, reaches=reaches, universe=universe, width=width, height=height, degenerate=degenerate)


def _overshoot_factors(n):
    """|r| / universe: most between 1 + 1e-6 and 8, 4 % from 30 to 1e4 (those are unsafe by MARGIN_DISCRIM)"""
    far = max(1, n // 25)
    f = np.concatenate([1 + 10 ** np.linspace(-6, -5.5, 4), 1 + 10 ** np.linspace(-5.4, np.log10(7.0), n - far - 4), 10 ** np.linspace(1.5, 4, far)])
    return f


def _polar_directions(rng, n):
    return np.arccos(rng.uniform(-0.95, 0.95, n)), rng.uniform(-3.1, 3.1, n)


def _overshoot_velocity(rng, n, r):
    """polar (dr, dtheta, dphi): thirds outward, tangent-ish (which misses the sphere from a large overshoot: discrim < 0) and inward;
    every sixth ray exactly radial"""
    kind = np.arange(n) % 3
    dr = np.where(kind == 0, 1.0, np.where(kind == 1, rng.uniform(-0.3, 0.3, n), -1.0))
    tangent = np.where(kind == 1, 1.0, rng.uniform(0.0, 0.4, n)) / np.abs(r)
    dth, dph = tangent * rng.normal(size=n), tangent * rng.normal(size=n)
    radial = np.arange(n) % 6 >= 4
    return dr, np.where(radial, 0.0, dth), np.where(radial, 0.0, dph)


def _build_cases():
    out = []
    rng = np.random.default_rng(20241019)
    t = lambda: rng.uniform(-50.0, 0.0, N)
    # universe_overshoot, polar charts
    for name, signed in (("kerr_boyer", False), ("wormhole", True), ("schwarzschild", False)):
        f = rng.permutation(_overshoot_factors(N))
        r = UNIVERSE * f
        if name == "schwarzschild":       # the constant-theta build, from just outside its terminator: the quaternion's rotation with and without the fix
            r[::5] = rng.uniform(1.06, 19.9, len(r[::5]))
        sign = np.where(rng.random(N) < 0.5, -1.0, 1.0) if signed else np.ones(N)
        th, ph = _polar_directions(rng, N)
        dr, dth, dph = _overshoot_velocity(rng, N, r)
        pos = np.stack([t(), sign * r, th, ph], axis=1)
        vel = np.stack([rng.uniform(-2, -0.5, N), sign * dr, dth, dph], axis=1)
        out.append(_case(f"universe_overshoot_{name}", name, make_rays(rng, pos, vel),
                         "fix_ray_position at |r| = universe (1 + 1e-6) ... 1e4 universe, outward, tangent and inward: discrim < 0, both orders of the roots"
                         + (", both signs of r and both sides" if signed else "") + (", the constant-theta rotation by a quaternion per ray" if name != "kerr_boyer" else "")))
    # ... a Cartesian and a cylindrical chart: the velocity goes through the chart's Jacobian
    for name in ("kerr_schild", "cosmic_string"):
        f = rng.permutation(_overshoot_factors(N))
        r = UNIVERSE * f
        th, ph = _polar_directions(rng, N)
        dr, dth, dph = _overshoot_velocity(rng, N, r)
        c = np.stack([_polar_to_cartesian((r[i], th[i], ph[i])) for i in range(N)])
        v = np.stack([_spherical_velocity_to_cartesian((r[i], th[i], ph[i]), (dr[i], dth[i], dph[i])) for i in range(N)])
        if name == "kerr_schild":
            pos, vel = np.column_stack([t(), c]), np.column_stack([rng.uniform(-2, -0.5, N), v])
        else:                              # (t, rho, phi, z) with x = rho cos phi, y = rho sin phi
            rho = np.hypot(c[:, 0], c[:, 1])
            pos = np.column_stack([t(), rho, np.arctan2(c[:, 1], c[:, 0]), c[:, 2]])
            vel = np.column_stack([rng.uniform(-2, -0.5, N), (c[:, 0] * v[:, 0] + c[:, 1] * v[:, 1]) / rho, (c[:, 0] * v[:, 1] - c[:, 1] * v[:, 0]) / rho ** 2, v[:, 2]])
        out.append(_case(f"universe_overshoot_{name}", name, make_rays(rng, pos, vel),
                         "fix_ray_position behind a chart whose velocity transform is not the identity: discrim < 0 and both orders of the roots"))
    # inside_terminator: the singular-terminator fix of a traversable chart; the same radii on schwarzschild return early
    r = rng.permutation(np.concatenate([10 ** np.linspace(-3, np.log10(0.97), N - 24), 1 - 10 ** np.linspace(-1.6, -4.5, 24)]))
    th, ph = _polar_directions(rng, N)
    dr = np.where(np.arange(N) % 2 == 0, -1.0, 1.0) * rng.uniform(0.2, 1.0, N)
    tangent = rng.uniform(0, 0.6, N)
    pos = np.stack([t(), r, th, ph], axis=1)
    vel = np.stack([rng.uniform(-2, -0.5, N), dr, tangent * rng.normal(size=N), tangent * rng.normal(size=N)], axis=1)
    out.append(_case("inside_terminator", "ingoing_ef_singular", make_rays(rng, pos, vel),
                     "fix_ray_position(..., SINGULAR_TERMINATOR) from r = 1e-3 to just under the terminator, infalling and outgoing"))
    out.append(_case("inside_terminator_schwarzschild", "schwarzschild", make_rays(rng, pos, vel), "the early return at |r| <= 1: tex_coord and z_shift 0, side set"))
    # theta_wrap
    th = rng.uniform(-3 * np.pi, 3 * np.pi, N)
    ph = rng.uniform(-5 * np.pi, 5 * np.pi, N)
    th[:6] = [PI_F32, 0.0, -0.0, -PI_F32, 2 * PI_F32, float(np.float32(3.0)) ]
    pos = np.stack([t(), rng.uniform(3, 19, N), th, ph], axis=1)
    vel = np.stack([rng.uniform(-2, -0.5, N), rng.uniform(-1, 1, N), rng.normal(size=N) / 10, rng.normal(size=N) / 10], axis=1)
    out.append(_case("theta_wrap", "kerr_boyer_near_extremal", make_rays(rng, pos, vel),
                     "angle_to_tex: theta in (-3 pi, 3 pi), phi in (-5 pi, 5 pi), theta = float(pi), 0 and -0 exactly"))
    # axis: a Cartesian chart on and next to x = y = 0, a polar chart with sin theta from 1e-7
    s = np.concatenate([10 ** np.linspace(-7, -5, 30), 10 ** np.linspace(-5, 0, N - 30)])
    rho = rng.uniform(2, 15, N) * s
    ang = rng.uniform(-np.pi, np.pi, N)
    x, y, z = rho * np.cos(ang), rho * np.sin(ang), np.where(np.arange(N) % 2 == 0, 1.0, -1.0) * rng.uniform(2, 15, N)
    x[:8], y[:8] = 0.0, 0.0
    x[8:16], y[8:16] = rng.uniform(-1e-6, 1e-6, 8), rng.uniform(-1e-6, 1e-6, 8)
    order = rng.permutation(N)
    pos = np.stack([t(), x, y, z], axis=1)[order]
    vel = np.column_stack([rng.uniform(-2, -0.5, N), rng.normal(size=(N, 3))])
    out.append(_case("axis_kerr_schild", "kerr_schild", make_rays(rng, pos, vel), "points on and within 1e-6 of the axis of a Cartesian chart, z of both signs"))
    th = np.arcsin(s)
    th = np.where(np.arange(N) % 2 == 0, th, np.pi - th)[order]
    pos = np.stack([t(), rng.uniform(3, 19, N), th, rng.uniform(-3.1, 3.1, N)], axis=1)
    out.append(_case("axis_kerr_boyer", "kerr_boyer", make_rays(rng, pos, vel), "sin theta from 1e-7 upwards at both poles of a polar chart"))
    # ergosphere: g_tt = 1 / r - 1 from -1e-3 through -1e-5 to positive (inside the horizon of the traversable chart).  The radial
    # velocity is of the size of g_tt: z reads dr through g_tr / sqrt|g_tt|, and a dr of order one makes z itself a quotient by
    # sqrt|g_tt| that no fp32 evaluation of 1 / r - 1 can deliver
    n_short, n_edge = 200, 12
    gtt = np.concatenate([-10 ** np.linspace(np.log10(9.9e-4), np.log10(1.3e-5), n_short), np.linspace(-1.2e-5, -0.8e-5, n_edge),
                          10 ** np.linspace(-3, -0.05, N - n_short - n_edge)])
    r = (1 / (1 + gtt)).astype(np.float32).astype(np.float64)
    th, ph = _polar_directions(rng, N)
    mix = rng.permutation(N)
    pos = np.stack([t(), r, th, ph], axis=1)[mix]
    vel = np.stack([rng.uniform(-2, -0.5, N), rng.uniform(-2, 2, N) * np.abs(gtt), rng.normal(size=N) / 5, rng.normal(size=N) / 5], axis=1)[mix]
    out.append(_case("ergosphere", "ingoing_ef_singular", make_rays(rng, pos, vel),
                     "both redshift paths: the shortcut at -1e-3 < g_tt < -1e-5 (where it must equal the full tetrad's) and the full tetrad at g_tt >= -1e-5"))
    # degenerate
    pos = np.stack([t(), rng.uniform(3, 19, N), *_polar_directions(rng, N)], axis=1)
    vel = np.stack([rng.uniform(-2, -0.5, N), rng.uniform(-1, 1, N), rng.normal(size=N) / 10, rng.normal(size=N) / 10], axis=1)
    bad = np.arange(0, N, 7)
    for j, i in enumerate(bad):
        value = (np.nan, np.inf, -np.inf)[j % 3]
        if j % 5 == 4:
            vel[i, j % 4] = np.nan
        else:
            pos[i, j % 4] = value
    out.append(_case("degenerate", "kerr_boyer", make_rays(rng, pos, vel), "NaN and +-Inf in one component of the position, NaN in the velocity, among ordinary rays",
                     degenerate=True))
    # clamp_and_running: the velocity's time component solved for a target z on the shortcut path
    prog = program("kerr_boyer")
    pos = np.stack([t(), rng.uniform(3, 19, N), *_polar_directions(rng, N)], axis=1).astype(np.float32).astype(np.float64)
    target = np.resize(np.array([-5.0, -1.5, -1.05] + REDSHIFT_Z), N)
    target = np.where(target == -0.999, -0.9985, target)     # (the clamp's own value sits on its branch: one either side instead)
    target[15::30] = -0.9995
    running = rng.choice([1.0, 0.25, 7.5], N).astype(np.float32).astype(np.float64)
    ku = (rng.uniform(0.5, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32).astype(np.float64)
    vel = np.stack([np.zeros(N), rng.uniform(-1, 1, N), rng.normal(size=N) / 10, rng.normal(size=N) / 10], axis=1)
    for i in range(N):
        g = prog.g(pos[i])
        s = np.sqrt(abs(g[0, 0]))
        vel[i, 0] = ((target[i] + 1) * s * ku[i] * running[i] - vel[i, 3] * g[0, 3]) / g[0, 0]
    out.append(_case("clamp_and_running", "kerr_boyer", make_rays(rng, pos, vel, ku=ku, running=running),
                     "z from below the -0.999 clamp to 1e4, running_dlambda_dnew of 1, 0.25 and 7.5 mixed per ray, ku_uobsu of both signs"))
    # flags
    pos = np.stack([t(), rng.uniform(3, 25, N), *_polar_directions(rng, N)], axis=1)
    vel = np.stack([rng.uniform(-2, -0.5, N), rng.uniform(0.2, 1, N), rng.normal(size=N) / 100, rng.normal(size=N) / 100], axis=1)
    out.append(_case("flags", "kerr_boyer", make_rays(rng, pos, vel, terminated=np.arange(N) % 3), "terminated 0, 1 and 2 interleaved"))
    return out


_cases = []


def cases():
    if not _cases:
        _cases.extend(_build_cases())
    return _cases


def case(name):
    return next(c for c in cases() if c["name"] == name)


CASE_NAMES = ["universe_overshoot_kerr_boyer", "universe_overshoot_wormhole", "universe_overshoot_schwarzschild", "universe_overshoot_kerr_schild",
              "universe_overshoot_cosmic_string", "inside_terminator", "inside_terminator_schwarzschild", "theta_wrap", "axis_kerr_schild",
              "axis_kerr_boyer", "ergosphere", "degenerate", "clamp_and_running", "flags"]


def features_bytes(c):
    return pack_features(universe_size=c["universe"], redshift=1)


def model_of(c):
    """(evaluate() of a case, its safe mask), cached on the case"""
    if "_model" not in c:
        prog = program(c["program"])
        e = evaluate(prog, c["rays"], c["universe"])
        c["_model"] = (e, safe_mask(prog, c["rays"], c["universe"], e))
    return c["_model"]


def compared(c):
    """the records a comparison covers: terminated == 1, past the early return, safe, and the model's own result finite"""
    e, safe = model_of(c)
    return e["live"] & (e["early"] == 0) & safe & np.isfinite(e["tex"]).all(axis=1) & np.isfinite(e["z_raw"])


def by_record(c, records):
    """records [height * width] (pixel order) -> in the order of the case's rays"""
    r = c["rays"]
    return np.asarray(records)[r["sy"].astype(np.int64) * c["width"] + r["sx"]]


def errors(c, got):
    """(max circ_diff(tex) * max(sin theta, 1e-3), max |dz| / (1 + |z|)) of records in ray order against the model, over compared(c)"""
    e, _ = model_of(c)
    sel = compared(c)
    if not sel.any():       # (every ray returned early: nothing but flags to compare)
        assert (e["early"][e["live"]] == 1).all(), c["name"]
        return 0.0, 0.0
    dtex = circ_diff(got["tex_coord"][sel].astype(np.float64), e["tex"][sel]) * sin_weight(e)[sel, None]
    dz = np.abs(got["z_shift"][sel].astype(np.float64) - e["z"][sel]) / (1 + np.abs(e["z"][sel]))
    return float(dtex.max()), float(dz.max())


def assert_flags(c, got, range_of_the_rest=True):
    """what is exact on every record: terminated, sx, sy, side, and (0, 0), 0 on the records that compute nothing; and the range of
    the records set aside.  tex_coord in [0, 1] is what angle_to_tex gives a theta in [0, pi) and a phi out of atan2.  A record set
    aside for its theta (within rounding of a multiple of pi: the south pole of a Cartesian chart, where atan2f returns float(pi))
    may take the wrap, which adds pi to phi, and the theta_wrap case hands angle_to_tex angles of several turns: of those the
    reference's own fmodf makes tex.x in (-0.5, 1.5) and tex.y in (-1, 1), and that range is what is asserted there."""
    e, safe = model_of(c)
    for f in ("terminated", "sx", "sy"):
        assert (got[f] == c["rays"][f]).all(), (c["name"], f)
    assert (got["side"] == e["side"]).all(), (c["name"], "side")
    nothing = ~e["live"] | (e["early"] == 1)
    assert (got["tex_coord"][nothing] == 0).all() and (got["z_shift"][nothing] == 0).all(), c["name"]
    assert (got["side"][~e["live"]] == 1).all()
    rest = e["live"] & (e["early"] == 0) & ~safe
    if range_of_the_rest and not c["degenerate"]:
        assert np.isfinite(got["tex_coord"][rest]).all() and np.isfinite(got["z_shift"][rest]).all(), c["name"]
        wide = e["unsafe_why"]["theta"] | (c["name"] == "theta_wrap")
        t = got["tex_coord"]
        assert (t[rest & ~wide] >= 0).all() and (t[rest & ~wide] <= 1).all(), c["name"]
        assert (t[rest & wide] >= (-0.5, -1.0)).all() and (t[rest & wide] <= (1.5, 1.0)).all(), c["name"]
    with np.errstate(invalid="ignore"):
        assert not (got["z_shift"][e["live"]] < np.float32(-0.999)).any(), c["name"]
