"""A float64 model of the set-up stage - the camera's chart coordinates, its tetrad, the boost, the inertial ray and the pixel rays -
and the hand-made cameras it is held against (tests/test_setup_model.py on the CPU, tests/test_gpu_setup.py on the device).

The model restates gr_cart_to_generic, calculate_tetrads, gr_boost_tetrad, gr_init_inertial_ray and make_pixel_ray / make_render_ray
(kernels/camera.hip, setup.hip, geodesic_camera.hip) in numpy and float64.  It follows the discrete algorithm, not the physics: the
same branches in the same order.
  * The metric tensor, both chart maps and the acceleration come from Metric.evaluate (the host's double evaluator of the generated
    expressions); tests/test_setup_model.py holds it to render_data_model.closed_form at the poses of this module.
  * Velocities change chart through the Jacobian of the map by central differences (model_common._jacobian_of, the step rule and
    error argument of tests/render_data_model.py).
  * fp32 numbers are taken as the fp32 values they are defined by: pi in pixel_direction and IS_CONSTANT_THETA's theta is float(pi),
    the field of view is the float the feature struct holds, the 1e-5 thresholds are the literals.
  * A stage's input is the fp32 value the stage before it stores: the tetrad is computed at float32(camera), the rays from the
    float32 tetrad.  So each kernel is compared on its own.

cases() is the seeded list (SEED).  A camera case has at most 64 poses (one has 70, to cross a wave); a ray case is one frame."""
import ctypes
import os
import re

import numpy as np

import geodesic_raytracing_amd as gra
from model_common import (_cartesian_to_polar, _cartesian_velocity_to_polar_velocity, _frame_basis_with_swap, _jacobian_of, _polar_to_cartesian,
                          _rot_quat, _spherical_velocity_to_cartesian)
from oracle import build_ref, build_restate
from oracle.refpipe import LIGHTRAY_DTYPE, pack_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "geodesic_raytracing_amd", "scripts")
PI_F32 = float(np.float32(np.pi))
CAMERA_FLOOR, RAY_FLOOR = 2e-6, 2e-5      # the stage's tolerances (tests/test_gpu_parity.py): the floors of every bound here
THIRD_LEG_MARGIN = 1e-6                   # the orientation step's third leg is undefined where less than this share of it is left
WIDEN = 1.5                               # gpu_stages.assert_path_against_float64's factor over the fp32 yardstick
SEED = 20241101
ETA = np.diag([-1.0, 1.0, 1.0, 1.0])

# name -> (script, $cfg overrides)
PROGRAMS = {
    "kerr_boyer": ("kerr_boyer", dict(a=0.45)),
    "kerr_boyer_near_extremal": ("kerr_boyer", dict(a=0.4999)),
    "schwarzschild": ("schwarzschild", {}),
    "schwarzschild_ingoing_ef": ("schwarzschild_ingoing_ef", {}),
    "kerr_schild": ("kerr_schild", {}),
    "cosmic_string": ("cosmic_string", {}),
    "wormhole": ("wormhole", {}),
    "alcubierre": ("alcubierre", {}),
    "time_ripple": ("time_ripple", {}),
    "double_unequal_kerr": ("double_unequal_kerr", {}),
    "kerr_newman_boyer": ("kerr_newman_boyer", {}),
    "minkowski": ("minkowski", {}),
}
REFERENCE_TAGS = {"kerr_boyer": "kerr_boyer_script", "kerr_boyer_near_extremal": "kerr_boyer_script", "schwarzschild": "schwarzschild_script",
                  "minkowski": "minkowski_script", "alcubierre": "alcubierre_script", "double_unequal_kerr": "double_unequal_kerr_script"}
SUBSTITUTED = ("kerr_boyer", "schwarzschild")      # run as the dynamic and as the substituted program
_programs = {}


class ProgramOf:
    """a metric, its $cfg values, its argument string and the macros the set-up stage reads from it"""

    def __init__(self, name=None, metric=None, cfg=None):
        if metric is None:
            script, overrides = PROGRAMS[name]
            metric = gra.Metric(script, SCRIPTS)
            cfg = metric.cfg_values(**overrides)
        self.name, self.metric, self.cfg = name, metric, [float(np.float32(v)) for v in cfg]
        self.argument_string = metric.argument_string()
        tokens = self.argument_string.split()
        self.generic_constant_theta = "-DGENERIC_CONSTANT_THETA" in tokens
        self.is_constant_theta = "-DIS_CONSTANT_THETA" in tokens or any(re.fullmatch(r"-DIS_CONSTANT_THETA=.*", t) for t in tokens)
        self.forward = "-DFORWARD_GEODESIC_PATH" in tokens

    def substituted_string(self):
        """the program with parameters and features baked in, at the features a frame without adaptive sampling uses"""
        return self.metric.argument_string(features=self.metric.features(adaptive_sampling=0), static=True, cfg_values=self.cfg)

    def _eval(self, what, x, v=None):
        return self.metric.evaluate(what, x, v, cfg_values=self.cfg or None)

    def to_polar(self, x):
        return self._eval(gra.EVAL_TO_POLAR, x)

    def from_polar(self, p):
        return self._eval(gra.EVAL_FROM_POLAR, p)

    def g(self, x):
        return self._eval(gra.EVAL_METRIC_TENSOR, x).reshape(4, 4)

    def acceleration(self, x, v):
        return self._eval(gra.EVAL_ACCELERATION, x, v)


def program(name):
    if name not in _programs:
        _programs[name] = ProgramOf(name)
    return _programs[name]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def camera_generic(prog, cart, flip):
    """gr_cart_to_generic of one camera (t, x, y, z) -> chart coordinates (float64)"""
    c = np.asarray(cart, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        polar = _cartesian_to_polar(c[1:])
        if flip > 0:
            polar[0] = -polar[0]
        return prog.from_polar(np.array([c[0], *polar]))


def boost(g, e, speed):
    """the boost of calculate_tetrads and gr_boost_tetrad (calculate_lorentz_boost, cl.cl:1919-1972) of legs e [4][4] by `speed`"""
    e0, e1, e2, e3 = e
    speed = np.asarray(speed, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Y = 1 / np.sqrt(1 - speed @ speed)
        u = Y * e0 + (Y * speed[0]) * e1 + (Y * speed[1]) * e2 + (Y * speed[2]) * e3
        lT, lu = g @ e0, g @ u
        gamma = -(lT @ u)
        L = np.eye(4) + (1 / (1 + gamma)) * np.outer(e0 + u, lT + lu) - 2 * np.outer(u, lT)
        return np.stack([u, L @ e1, L @ e2, L @ e3])


def tetrad(prog, x, speed=(0.0, 0.0, 0.0), trace=None):
    """calculate_tetrads(x, speed, orient) at chart position x -> legs [4][4]; `trace` receives the branches taken and the legs
    before the boost"""
    trace = {} if trace is None else trace
    x = np.asarray(x, dtype=np.float64)
    trace.update(first_nonzero=0, second_pass=False, negative_r=False, degenerate=False, third_leg_defined=True)
    if not np.isfinite(x).all():
        trace["degenerate"] = True
        trace["unboosted"] = np.eye(4)
        return np.eye(4)
    polar = prog.to_polar(x)
    g = prog.g(x)
    t1 = {}
    which, e = _frame_basis_with_swap(g, 0, t1)
    first = t1["first_nonzero"]
    if which != 0:
        trace["second_pass"] = True
        t2 = {}
        _, e = _frame_basis_with_swap(g, which, t2)
        first = max(first, t2["first_nonzero"])
    trace["first_nonzero"] = first
    e0, e1, e2, e3 = e
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        apolar = polar[1:].copy()
        apolar[0] = abs(apolar[0])
        cart = _polar_to_cartesian(apolar)
        m = np.stack([e0, e1, e2, e3], axis=1)
        try:
            inv = np.linalg.inv(m)
        except np.linalg.LinAlgError:
            inv = np.full((4, 4), np.nan)
        s = [_cartesian_velocity_to_polar_velocity(cart, np.eye(3)[k]) for k in range(3)]
        if polar[1] < 0:
            trace["negative_r"] = True
            for v in s:
                v[0] = -v[0]
        J = _jacobian_of(prog.from_polar, polar, angles=(0, 1, 2, 3))
        gx, gy, gz = (J @ np.array([0.0, *v]) for v in s)
        u1, u2, u3 = (inv @ gy)[1:], (inv @ gx)[1:], (inv @ gz)[1:]
        proj = lambda u, v: ((u @ v) / (u @ u)) * u
        whole = np.sqrt(u3 @ u3)
        u2 = u2 - proj(u1, u2)
        u3 = u3 - proj(u1, u3)
        u3 = u3 - proj(u2, u3)
        # what is left of the z direction once y and x are taken out of it, as a share of it: where this is rounding (inside the horizon
        # of ingoing Eddington-Finkelstein it is 1e-16: the three directions span a plane of that tetrad) the third leg is 0 / 0
        trace["third_leg_defined"] = bool(np.sqrt(u3 @ u3) > THIRD_LEG_MARGIN * whole)
        u1, u2, u3 = (u / np.sqrt(u @ u) for u in (u1, u2, u3))
        x_out = u2[0] * e1 + u2[1] * e2 + u2[2] * e3
        y_out = u1[0] * e1 + u1[1] * e2 + u1[2] * e3
        z_out = u3[0] * e1 + u3[1] * e2 + u3[2] * e3
    unboosted = np.stack([e0, x_out, y_out, z_out])
    trace["unboosted"] = boost(g, unboosted, (0.0, 0.0, 0.0))     # what the kernel stores for a speed of zero
    return boost(g, unboosted, speed)


def timelike_vector(speed, e):
    speed = np.asarray(speed, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        Y = 1 / np.sqrt(1 - speed @ speed)
    return Y * e[0] + (Y * speed[0]) * e[1] + (Y * speed[1]) * e[2] + (Y * speed[2]) * e[3]


def pixel_direction(cx, cy, width, height, quat, fov):
    fov = float(np.float32(fov))
    fov_rad = (fov / 360.0) * 2 * PI_F32
    with np.errstate(invalid="ignore", divide="ignore"):
        f_stop = (width / 2) / np.tan(fov_rad / 2)
        d = np.array([cx - width / 2, cy - height / 2, f_stop])
        d = _rot_quat(d / np.sqrt(d @ d), np.asarray(quat, dtype=np.float64))
        return d / np.sqrt(d @ d)


def _theta_adjustment_quat(pixel_dir, polar, angle_sign):
    with np.errstate(invalid="ignore", divide="ignore"):
        n = lambda v: v / np.sqrt(v @ v)
        if np.sqrt(pixel_dir @ pixel_dir) < 0.00001:
            pixel_dir = np.array([0.0, 1.0, 0.0])
        apolar = polar[1:].copy()
        apolar[0] = abs(apolar[0])
        cam = _polar_to_cartesian(apolar)
        bx, by = n(pixel_dir), n(-cam)
        bx = n(n(bx - (bx @ by) * by))
        plane_n = -n(np.cross(bx, by))
        z = np.array([0.0, 0.0, 1.0])
        angle = np.arccos(plane_n @ z) * angle_sign
        axis = n(np.cross(plane_n, z))
        s = np.sin(angle / 2)
        return n(np.array([axis[0] * s, axis[1] * s, axis[2] * s, np.cos(angle / 2)]))


def render_ray(prog, position, velocity, observer):
    """make_render_ray -> dict(position, velocity, initial_quat, acceleration, ku_uobsu)"""
    position, velocity = np.array(position, dtype=np.float64), np.array(velocity, dtype=np.float64)
    quat = np.array([0.0, 0.0, 0.0, 1.0])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if prog.generic_constant_theta:
            polar = prog.to_polar(position)
            vel_sph = _jacobian_of(prog.to_polar, position) @ velocity
            sgn = np.sign(polar[1])
            pos_sph = polar.copy()
            pos_sph[1] = abs(pos_sph[1])
            pos_cart = _polar_to_cartesian(pos_sph[1:])
            vel_cart = _spherical_velocity_to_cartesian(pos_sph[1:], vel_sph[1:])
            q = _theta_adjustment_quat(vel_cart, polar, 1)
            quat = _theta_adjustment_quat(vel_cart, polar, -1)
            pos_cart, vel_cart = _rot_quat(pos_cart, q), _rot_quat(vel_cart, q)
            next_pos = _cartesian_to_polar(pos_cart)
            next_vel = _cartesian_velocity_to_polar_velocity(pos_cart, vel_cart)
            if sgn < 0:
                next_pos[0] = -next_pos[0]
            first, second, first_rate, second_rate = position[0], position[1], velocity[0], velocity[1]
            at = np.array([pos_sph[0], *next_pos])
            if np.isfinite(at).all():
                position = prog.from_polar(at)
                velocity = _jacobian_of(prog.from_polar, at, angles=(0, 1, 2, 3)) @ np.array([vel_sph[0], *next_vel])
            else:
                position, velocity = np.full(4, np.nan), np.full(4, np.nan)
            position[0], position[1], velocity[0], velocity[1] = first, second, first_rate, second_rate
        if prog.is_constant_theta:
            position[2], velocity[2] = float(np.float32(PI_F32) / np.float32(2)), 0.0
        if np.isfinite(position).all() and np.isfinite(velocity).all():
            at, rate = position.copy(), velocity.copy()
            if prog.generic_constant_theta:
                at[2], rate[2] = float(np.float32(PI_F32) / np.float32(2)), 0.0
            acc = prog.acceleration(at, rate)
            if prog.generic_constant_theta:
                acc[2] = 0.0
            ku = velocity @ (prog.g(position) @ np.asarray(observer, dtype=np.float64))
        else:
            acc, ku = np.full(4, np.nan), np.nan
    return dict(position=position, velocity=velocity, initial_quat=quat, acceleration=acc, ku_uobsu=ku)


def inertial_ray(prog, x, e, speed):
    """gr_init_inertial_ray: the observer's own world line as a ray"""
    out = render_ray(prog, x, timelike_vector(speed, e), e[0])
    out["ku_uobsu"] = 1.0
    return out


def pixel_ray(prog, x, e, quat, fov, cx, cy, width, height, flip):
    d = pixel_direction(cx, cy, width, height, quat, fov)
    pixel_t = e[0] if prog.forward else -e[0]
    if flip:
        pixel_t = -pixel_t
    k = d[0] * e[1] + d[1] * e[2] + d[2] * e[3] + pixel_t
    return render_ray(prog, x, k, e[0])


RAY_FIELDS = ("position", "velocity", "acceleration", "initial_quat")


def frame_rays(prog, x, e, quat, fov, width, height, flip):
    """the model's rays of a frame in reference slot order -> dict of float64 arrays [n][4] and ku_uobsu [n]"""
    n = width * height
    out = {f: np.zeros((n, 4)) for f in RAY_FIELDS}
    out["ku_uobsu"] = np.zeros(n)
    for i in range(n):
        r = pixel_ray(prog, x, e, quat, fov, i % width, i // width, width, height, flip)
        for f in out:
            out[f][i] = r[f]
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def vec_err(got, want):
    """|got - want| per 4-vector relative to the vector's largest component, floor 1 (gpu_stages.vec_err with that floor); NaN where
    the model's own vector is not finite: nothing is compared there"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        scale = np.maximum(np.abs(want).max(axis=-1), 1.0)
        err = np.abs(got - want).max(axis=-1) / scale
    err = np.where(np.isfinite(want).all(axis=-1), np.where(np.isnan(err), np.inf, err), np.nan)
    return err


def finite_pattern(a):
    return np.isfinite(np.asarray(a, dtype=np.float64))


def assert_within(name, what, floor, err, yardstick_err):
    """the device's rule, per value (a pose's vector, a ray): err_i <= max(floor, WIDEN * y_i), y_i the largest of the yardstick's
    errors on value i and on its two neighbours in the case's order.  The yardstick's error on one value is one draw of fp32 rounding
    at that value's conditioning, and a second fp32 evaluation of the same value is another draw: on ill-conditioned values two
    correct evaluations differ by more than 1.5 x one of them (measured: at g_tt = -4e-5 the device's tetrad is 7.0e-5 from the
    model, the reference object's 3.2e-5).  The sweeps are ordered by conditioning in steps of a factor 1.8 at most, so a value's
    neighbours are draws at nearly its conditioning; three draws bound the fourth where one does not.  A value whose yardstick
    error and whose neighbours' are within the floor is held to the floor whatever else the case holds.  Where the model is not
    finite (NaN in both) or the yardstick's own result is not (its error is inf) nothing is compared - the callers require the
    device's pattern of finite components to be the yardstick's there.  -> number of values held to the floor"""
    err, y = np.asarray(err, dtype=np.float64).ravel(), np.asarray(yardstick_err, dtype=np.float64).ravel()
    assert (np.isnan(err) == np.isnan(y)).all(), (name, what)
    compared = ~np.isnan(err) & np.isfinite(y)
    if not compared.any():
        return 0
    known = np.where(np.isfinite(y), y, 0.0)
    padded = np.concatenate([[0.0], known, [0.0]])
    nearby = np.maximum(np.maximum(padded[:-2], padded[1:-1]), padded[2:])
    limit = np.maximum(floor, WIDEN * nearby)
    over = compared & (err > limit)
    worst = int(np.argmax(np.where(compared, err / limit, 0.0)))
    assert not over.any(), (name, what, "values over their bound", np.flatnonzero(over).tolist(), "worst (index, error, bound, yardstick)",
                            worst, float(err[worst]), float(limit[worst]), float(y[worst]))
    return int((compared & (limit == floor)).sum())


def shares(floor, yardstick_err):
    """(share of compared values whose yardstick error is beyond the floor, share of all values set aside as not finite)"""
    y = np.asarray(yardstick_err, dtype=np.float64).ravel()
    aside = np.isnan(y)
    compared = y[~aside]
    return (float((compared > floor).mean()) if compared.size else 0.0), float(aside.mean())


RELATIVE_FROM = 0.99      # |v|: from here the orthonormality residual is taken relative to the size of what is summed


def tetrad_invariant(prog, x, e, relative=False):
    """max over a, b of |e_a . g . e_b - eta_ab| of legs e [4][4] at chart position x, g in float64.  relative: each residual over
    max(1, sum_ij |g_ij e_a^i e_b^j|) - asked for at |v| >= RELATIVE_FROM only, where the legs have components of 7 to 22 and
    e_a . g . e_b is a sum of terms of size 50 to 500 that cancel to 1: its fp32 rounding is 6e-8 times that size in any order of
    summation, and which order comes out nearer is chance (on the 0.999 c poses the device's plain residual was 1.81e-4, the
    restatement's own 1.89e-4 through the one-step tetrad and 1.01e-4 through the boost of stored legs)."""
    g = prog.g(np.asarray(x, dtype=np.float64))
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        residual = np.abs(e @ g @ e.T - ETA)
        if relative:
            residual = residual / np.maximum(1.0, np.einsum("ij,ai,bj->ab", np.abs(g), np.abs(e), np.abs(e)))
        return float(residual.max())


def ray_invariants(prog, e, position, velocity, ku, observer=None):
    """(|k.g.k| / sum |g_ij k_i k_j|, |ku - k.g.e0|, | |spatial part of k in the tetrad| - 1 |) of one ray; the tetrad sits at the
    camera, so the last is asked of programs that do not rotate the ray (callers pass e = None otherwise)"""
    g = prog.g(np.asarray(position, dtype=np.float64))
    k = np.asarray(velocity, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        terms = g * np.outer(k, k)
        null = abs(terms.sum()) / np.abs(terms).sum()
        out = [float(null)]
        if observer is not None:
            out.append(float(abs(ku - k @ (g @ np.asarray(observer, dtype=np.float64))) / max(1.0, np.abs(k).max())))
        if e is not None:
            comps = np.linalg.solve(np.asarray(e, dtype=np.float64).T, k)
            out.append(float(abs(np.sqrt(comps[1:] @ comps[1:]) - 1)))
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _camera_case(name, kind, prog, cart, flip, speeds, reaches, generic=None):
    """cart [n][4] fp32 cameras (t, x, y, z); speeds [n][3] per pose; flip per case.  `generic` gives chart positions directly (the
    sweeps that are stated in chart coordinates): then gr_cart_to_generic is not part of the case."""
    cart = None if cart is None else np.asarray(cart, dtype=np.float32)
    n = len(cart) if cart is not None else len(generic)
    speeds = np.asarray(speeds, dtype=np.float32).reshape(n, 3)
    c = dict(name=name, kind=kind, program=prog, cart=cart, flip=float(flip), speeds=speeds, reaches=reaches, count=n,
             generic=None if generic is None else np.asarray(generic, dtype=np.float32))
    for a in (c["cart"], c["speeds"], c["generic"]):
        if a is not None:
            a.setflags(write=False)
    return c


def _sphere(rng, n, r_lo=1.5, r_hi=30.0, margin_deg=10.0, t_hi=50.0):
    r = rng.uniform(r_lo, r_hi, n)
    lim = np.cos(np.radians(margin_deg))
    th, ph = np.arccos(rng.uniform(-lim, lim, n)), rng.uniform(-np.pi, np.pi, n)
    t = rng.uniform(-t_hi, t_hi, n)
    return np.stack([t, r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], axis=1)


def _speeds(rng, n, top=0.6):
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(0.05, top, n) / np.linalg.norm(v, axis=1))[:, None]
    return v


def _at_rest_and_moving(rng, cart):
    """every pose twice: at rest, then at one random |v| <= 0.6 -> (cart [2n][4], speeds [2n][3]).  The poses at rest share one launch of
    gr_init_basis_vectors (its speed is a scalar argument), every moving one has a launch of its own."""
    speeds = np.zeros((2 * len(cart), 3))
    speeds[1::2] = _speeds(rng, len(cart))
    return np.repeat(cart, 2, axis=0), speeds


ORDINARY = ["kerr_boyer", "kerr_boyer_near_extremal", "schwarzschild", "schwarzschild_ingoing_ef", "kerr_schild", "cosmic_string", "wormhole",
            "alcubierre", "time_ripple", "double_unequal_kerr", "kerr_newman_boyer"]
BOOSTS = (0.0, 0.1, 0.9, 0.99, 0.999)


def _axis_sweep(rng):
    """sin theta of 48 poses: logarithmic from 1e-6 to 0.1, where fp32 loses sqrt(1 - z^2 / r^2) (its error is 6e-8 / sin^2 theta), and
    28 poses from 0.35 to 1 where it does not: the sweep of six decades has five of them beyond the floor, so it is thinned at the
    edge end for the cap of one half to hold"""
    return np.concatenate([10 ** np.linspace(-6, -1, 20), rng.uniform(0.35, 1.0, 28)])


def _build_camera_cases():
    out = []
    rng = np.random.default_rng(SEED)
    for name in ORDINARY:
        n = 35 if name == "kerr_boyer" else 12
        cart, speeds = _at_rest_and_moving(rng, _sphere(rng, n))
        if name == "time_ripple":      # the late times are an edge case of their own: fp32 loses the ripple's phase as t grows
            late = _sphere(rng, 48)
            late[:, 0] = np.where(np.arange(48) % 2 == 0, 1.0, -1.0) * np.concatenate([rng.uniform(0, 50, 26), 10 ** np.linspace(np.log10(50), 4, 22)])
            out.append(_camera_case("late_time_ripple", "edge", name, late, 0.0, _speeds(rng, 48),
                                    "|t| to 1e4 (22 poses, logarithmic from 50) among 26 poses at |t| <= 50"))
        if name == "wormhole":      # both sides: flip = 1 puts the camera at r < 0
            far, far_speeds = _at_rest_and_moving(rng, _sphere(rng, n))
            out.append(_camera_case("ordinary_wormhole_far_side", "ordinary", name, far, 1.0, far_speeds,
                                    "negative r, flip: the orientation step's sign flip at random poses"))
        out.append(_camera_case(f"ordinary_{name}", "ordinary", name, cart, 0.0, speeds,
                                "random poses over the sphere, 10 degrees off the axes, each at rest and moving" + (", 70 records: two waves" if n == 35 else "")))
    # axis, polar charts: sin theta from 1e-6 to 1 at both poles
    for name in ("kerr_boyer", "kerr_newman_boyer"):
        n = 48
        s = _axis_sweep(rng)
        th = np.where(np.arange(n) % 2 == 0, np.arcsin(s), np.pi - np.arcsin(s))
        r, ph = rng.uniform(3, 20, n), rng.uniform(-np.pi, np.pi, n)
        cart = np.stack([rng.uniform(-50, 50, n), r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], axis=1)
        out.append(_camera_case(f"axis_{name}", "edge", name, cart, 0.0, np.zeros((n, 3)), "sin theta from 1e-6 to 0.1 (20 poses, logarithmic) and from 0.35 to 1 (28 poses) at both poles of a polar chart"))
    n = 48
    s = _axis_sweep(rng)
    r, ph = rng.uniform(3, 20, n), rng.uniform(-np.pi, np.pi, n)
    z = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * r * np.sqrt(1 - s * s)
    cart = np.stack([rng.uniform(-50, 50, n), r * s * np.cos(ph), r * s * np.sin(ph), z], axis=1)
    out.append(_camera_case("axis_cosmic_string", "edge", "cosmic_string", cart, 0.0, np.zeros((n, 3)), "rho / r from 1e-6 to 0.1 (20 poses, logarithmic) and from 0.35 to 1 (28 poses) in a cylindrical chart"))
    # axis of a Cartesian chart: on it (not finite: set aside) and within 1e-6 of it, among ordinary poses
    n = 48
    cart = _sphere(rng, n)
    cart[0:2, 1:3] = 0.0
    cart[0, 3], cart[1, 3] = 5.0, -7.0
    near = np.arange(2, 14)
    cart[near, 1] = rng.uniform(-1e-6, 1e-6, len(near))
    cart[near, 2] = rng.uniform(-1e-6, 1e-6, len(near))
    cart[near, 3] = np.where(near % 2 == 0, 1.0, -1.0) * rng.uniform(2, 15, len(near))
    out.append(_camera_case("axis_kerr_schild", "edge", "kerr_schild", cart, 0.0, np.zeros((n, 3)),
                            "two cameras on x = y = 0 (set aside: the model is not finite there), twelve within 1e-6 of it, z of both signs"))
    # ergosphere of near-extremal Kerr in the equatorial plane: g_tt = rs / r - 1 there, from -0.3 through +-1e-5 to just outside
    # the horizon r+ = (1 + sqrt(1 - 4 a^2)) / 2 = 0.51
    gtt = np.concatenate([-10 ** np.linspace(np.log10(0.3), -5.5, 20), [-1.2e-5, -0.9e-5, 0.9e-5, 1.2e-5], 10 ** np.linspace(-5.5, np.log10(0.9), 24)])
    r = 1 / (1 + gtt)
    n = len(r)
    generic = np.stack([rng.uniform(-50, 50, n), r, np.full(n, np.pi / 2), rng.uniform(-np.pi, np.pi, n)], axis=1)
    out.append(_camera_case("ergosphere_kerr_boyer", "edge", "kerr_boyer_near_extremal", None, 0.0, np.zeros((n, 3)),
                            "second frame_basis pass: g_tt > 0 inside the static limit (the timelike leg is not in slot 0), and |g_tt| <= 1e-5 "
                            "on it (first_nonzero != 0)", generic=generic))
    # horizon of ingoing Eddington-Finkelstein: g_rr = 0 everywhere, g_tt > 0 inside
    r = np.concatenate([np.linspace(3, 1.05, 49), 1 + 10 ** np.linspace(-1.5, -4.5, 12), [1 - 1e-3, 0.8, 0.5]])
    n = len(r)
    lim = np.cos(np.radians(10))
    generic = np.stack([rng.uniform(-50, 50, n), r, np.arccos(rng.uniform(-lim, lim, n)), rng.uniform(-np.pi, np.pi, n)], axis=1)
    out.append(_camera_case("horizon_ingoing_ef", "edge", "schwarzschild_ingoing_ef", None, 0.0, np.tile([0.1, -0.2, 0.2], (n, 1)),
                            "first_nonzero != 0 (g_rr = 0 everywhere) from r = 3 to 0.5; g_tt > 0 inside r = 1: second frame_basis pass.  Inside, "
                            "the orientation step's third leg is the normalised remainder of a projection that vanishes identically (the radial "
                            "direction has no spatial part in that tetrad): rounding noise in the reference's own algorithm, in any precision - "
                            "such poses are set aside (the model says so from the size of that remainder), and the sweep is cut to three of 64 poses there for "
                            "the cap of 5 % to hold; |g_tt| <= 1e-5, where no leg of the first pass is finite, is left out for the same cap", generic=generic))
    # boost: |v| along each leg and along random directions, one pose per direction
    for name in ("kerr_boyer", "kerr_schild", "minkowski"):
        dirs = np.concatenate([np.eye(3), -np.eye(3)[:1], rng.normal(size=(4, 3))])
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        speeds = np.concatenate([v * dirs for v in BOOSTS])
        n = len(speeds)
        out.append(_camera_case(f"boost_{name}", "edge", name, _sphere(rng, n), 0.0, speeds, "|v| = 0, 0.1, 0.9, 0.99, 0.999 along each leg and random directions"))
    # degenerate: NaN or +-Inf in one component among ordinary cameras
    n = 64
    cart = _sphere(rng, n)
    for j, i in enumerate((7, 30, 63)):      # three of 64: the cap on values set aside is 5 %
        cart[i, (1, 3, 0)[j]] = (np.nan, np.inf, -np.inf)[j]
    out.append(_camera_case("degenerate_kerr_boyer", "edge", "kerr_boyer", cart, 0.0, np.tile([0.2, -0.3, 0.1], (n, 1)),     # one speed: one launch of 64
                            "degenerate: NaN and +-Inf in one component of the camera: the identity tetrad, the neighbours untouched"))
    return out


# the two orientations of the fixtures: the default camera and tests/golden/make_golden.py's TILTED_QUAT
FIXTURE_QUATS = ([-0.7071067811865475, -0.0, -0.0, 0.7071067811865476], [-0.6805373836277301, 0.1920126805321033, -0.0529833041248791, 0.7051189754105407])
FRAMES = [(1, 1), (2, 2), (3, 2), (8, 8), (67, 3)]
FOVS = [1.0, 45.0, 110.0, 179.0]


def _build_ray_cases():
    """one frame each: (program, pose kind) runs through the frames, fields of view and quaternions in turn"""
    out = []
    rng = np.random.default_rng(SEED + 1)
    quats = [np.array([0.0, 0.0, 0.0, 1.0]), np.array(FIXTURE_QUATS[0]), np.array(FIXTURE_QUATS[1]), np.array([1.0, 0, 0, 0]), np.array([0, 1.0, 0, 0]), np.array([0, 0, 1.0, 0])]
    for _ in range(6):
        q = rng.normal(size=4)
        quats.append(q / np.linalg.norm(q))
    quats.append(3.0 * quats[6])
    quats.append(1e-3 * quats[7])
    k = 0
    for name in ("kerr_boyer", "schwarzschild", "schwarzschild_ingoing_ef", "kerr_schild", "wormhole"):
        for pose in ("ordinary", "axis", "boosted", "far_side"):
            if (pose == "far_side") != (name == "wormhole" and pose == "far_side"):
                continue
            cart = _sphere(rng, 1, r_lo=2.0, r_hi=12.0)[0]
            if pose == "axis":
                r, s, ph = 6.0, 1e-3, 0.7
                cart[1:] = [r * s * np.cos(ph), r * s * np.sin(ph), r * np.sqrt(1 - s * s)]
            speed = np.array([0.5, -0.6, 0.45]) if pose == "boosted" else np.zeros(3)      # |v| = 0.9
            flip = 1 if pose == "far_side" else 0
            out.append(dict(name=f"rays_{name}_{pose}", kind="ordinary" if pose in ("ordinary", "far_side") else "edge", program=name,
                            cart=cart.astype(np.float32), flip=flip, speed=speed.astype(np.float32), quat=quats[k % len(quats)].astype(np.float32),
                            fov=FOVS[k % 4], width=FRAMES[k % 5][0], height=FRAMES[k % 5][1],
                            reaches=f"{pose} pose" + (", negative r, flip" if flip else "")))
            k += 1
    # the quaternions and frames the rotation above did not reach, on kerr_boyer at an ordinary pose
    while k < 28:
        cart = _sphere(rng, 1, r_lo=2.0, r_hi=12.0)[0]
        out.append(dict(name=f"rays_kerr_boyer_more_{k}", kind="ordinary" if FOVS[k % 4] < 179 else "edge", program="kerr_boyer",
                        cart=cart.astype(np.float32), flip=0, speed=np.zeros(3, dtype=np.float32), quat=quats[k % len(quats)].astype(np.float32),
                        fov=FOVS[k % 4], width=FRAMES[k % 5][0], height=FRAMES[k % 5][1], reaches="ordinary pose"))
        k += 1
    # the substituted programs bake the default field of view in: one frame of it on the two programs that are run both ways
    for name in SUBSTITUTED:
        cart = _sphere(rng, 1, r_lo=2.0, r_hi=12.0)[0]
        out.append(dict(name=f"rays_{name}_default_fov", kind="ordinary", program=name, cart=cart.astype(np.float32), flip=0,
                        speed=np.zeros(3, dtype=np.float32), quat=np.array(FIXTURE_QUATS[0], dtype=np.float32), fov=90.0, width=8, height=8,
                        reaches="the field of view of the substituted program", substituted=True))
    # schwarzschild: the centre pixel (cx - w / 2 = 0) of a frame whose camera looks along -position: exactly radial, where the
    # constant-theta rotation has no plane (the model is not finite there: set aside)
    out.append(dict(name="rays_schwarzschild_radial_centre", kind="edge", program="schwarzschild", cart=np.array([0.0, 0.0, 0.0, -5.0], dtype=np.float32),
                    flip=0, speed=np.zeros(3, dtype=np.float32), quat=np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32), fov=45.0, width=8, height=8,
                    reaches="a camera on the -z axis looking along +z: the centre pixel looks exactly at the origin"))
    for c in out:
        c.setdefault("substituted", False)
        for a in (c["cart"], c["speed"], c["quat"]):
            a.setflags(write=False)
    return out


_cases = {}


def camera_cases():
    if "camera" not in _cases:
        _cases["camera"] = _build_camera_cases()
    return _cases["camera"]


def ray_cases():
    if "ray" not in _cases:
        _cases["ray"] = _build_ray_cases()
    return _cases["ray"]


CAMERA_CASE_NAMES = ["ordinary_kerr_boyer", "ordinary_kerr_boyer_near_extremal", "ordinary_schwarzschild", "ordinary_schwarzschild_ingoing_ef",
                     "ordinary_kerr_schild", "ordinary_cosmic_string", "ordinary_wormhole_far_side", "ordinary_wormhole", "ordinary_alcubierre",
                     "late_time_ripple", "ordinary_time_ripple", "ordinary_double_unequal_kerr", "ordinary_kerr_newman_boyer", "axis_kerr_boyer", "axis_kerr_newman_boyer",
                     "axis_cosmic_string", "axis_kerr_schild", "ergosphere_kerr_boyer", "horizon_ingoing_ef", "boost_kerr_boyer", "boost_kerr_schild",
                     "boost_minkowski", "degenerate_kerr_boyer"]


def camera_case(name):
    return next(c for c in camera_cases() if c["name"] == name)


def ray_case(name):
    return next(c for c in ray_cases() if c["name"] == name)


def case_bytes():
    """every input of every case, for the determinism test"""
    parts = []
    for c in camera_cases():
        parts += [c["name"].encode(), c["speeds"].tobytes(), np.float32(c["flip"]).tobytes()]
        parts += [a.tobytes() for a in (c["cart"], c["generic"]) if a is not None]
    for c in ray_cases():
        parts += [c["name"].encode(), c["cart"].tobytes(), c["speed"].tobytes(), c["quat"].tobytes(), np.float32(c["fov"]).tobytes(),
                  bytes([c["width"], c["height"], c["flip"]])]
    return b"".join(parts)


def features_bytes(fov=90.0):
    return pack_features(field_of_view=fov, adaptive_sampling=0)


def camera_model(c):
    """the model of a camera case, cached: camera [n][4] (float64; NaN rows where the case states chart positions), generic32 (what the
    tetrad kernels are given), tetrad [n][4][4], unboosted [n][4][4], inertial rays, and the branches per pose"""
    if "_model" in c:
        return c["_model"]
    prog, n = program(c["program"]), c["count"]
    m = dict(camera=np.full((n, 4), np.nan), tetrad=np.zeros((n, 4, 4)), unboosted=np.zeros((n, 4, 4)), trace=[])
    if c["cart"] is not None:
        for i in range(n):
            m["camera"][i] = camera_generic(prog, c["cart"][i], c["flip"])
        m["generic32"] = m["camera"].astype(np.float32)
        # a camera the model cannot place (on the axis of a Cartesian chart) is given to the tetrad kernels as it is: NaN, degenerate
    else:
        m["generic32"] = c["generic"].copy()
    for i in range(n):
        t = {}
        m["tetrad"][i] = tetrad(prog, m["generic32"][i], c["speeds"][i], t)
        m["unboosted"][i] = t.pop("unboosted")
        if not t["third_leg_defined"]:      # the model has no value there: set aside, like a value that is not finite
            m["tetrad"][i], m["unboosted"][i] = np.nan, np.nan
        m["trace"].append(t)
    m["unboosted32"], m["tetrad32"] = m["unboosted"].astype(np.float32), m["tetrad"].astype(np.float32)
    # gr_boost_tetrad is given the fp32 legs before the boost, gr_init_inertial_ray the fp32 boosted legs and a speed of its own
    m["reboosted"] = np.zeros((n, 4, 4))
    m["inertial"] = {f: np.zeros((n, 4)) for f in RAY_FIELDS}
    for i in range(n):
        x = m["generic32"][i].astype(np.float64)
        if np.isfinite(x).all():
            m["reboosted"][i] = boost(prog.g(x), m["unboosted32"][i].astype(np.float64), c["speeds"][i])
            r = inertial_ray(prog, x, m["tetrad32"][i].astype(np.float64), c["speeds"][i] * np.float32(0.5))
        else:
            m["reboosted"][i] = np.nan
            r = {f: np.full(4, np.nan) for f in RAY_FIELDS}
        for f in RAY_FIELDS:
            m["inertial"][f][i] = r[f]
    c["_model"] = m
    return m


def ray_model(c):
    """the model of a ray case, cached: generic32 [4], tetrad32 [4][4] (the inputs of gr_init_rays_generic) and the rays"""
    if "_model" in c:
        return c["_model"]
    prog = program(c["program"])
    generic32 = camera_generic(prog, c["cart"], c["flip"]).astype(np.float32)
    t = {}
    tetrad32 = tetrad(prog, generic32, c["speed"], t).astype(np.float32)
    rays = frame_rays(prog, generic32.astype(np.float64), tetrad32.astype(np.float64), c["quat"], c["fov"], c["width"], c["height"], c["flip"])
    c["_model"] = dict(generic32=generic32, tetrad32=tetrad32, rays=rays, trace=t)
    return c["_model"]


def ray_errors(c, got):
    """per ray: the largest vec_err over position, velocity, acceleration and quaternion and |ku - model| / max(1, |model|) of records
    `got` (LIGHTRAY_DTYPE, reference slot order) against the model; NaN where the model's own ray is not finite"""
    m = ray_model(c)["rays"]
    err = np.stack([vec_err(got[f], m[f]) for f in RAY_FIELDS])
    with np.errstate(invalid="ignore"):
        ku = np.abs(got["ku_uobsu"].astype(np.float64) - m["ku_uobsu"]) / np.maximum(1.0, np.abs(m["ku_uobsu"]))
    ku = np.where(np.isfinite(m["ku_uobsu"]), np.where(np.isnan(ku), np.inf, ku), np.nan)
    err = np.concatenate([err, ku[None]])
    aside = np.isnan(err).any(axis=0)
    return np.where(aside, np.nan, np.nanmax(np.where(np.isnan(err), 0, err), axis=0))


def slot_order(records, width, height):
    """records of a tiled or linear launch -> the frame's records in reference slot order"""
    inside = records["sx"] >= 0
    r = records[inside]
    assert len(r) == width * height
    return r[np.argsort(r["sy"].astype(np.int64) * width + r["sx"], kind="stable")]



# ---- the fp32 yardstick ------------------------------------------------------------------------------------------------------------
_yardsticks, _figures = {}, {}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Yardstick:
    """the fp32 CPU evaluation of the stage for one program: the reference's own object where oracle/_ref holds one for the
    program's string, the restatement otherwise.  Never the code under test."""

    def __init__(self, program_name):
        prog = program(program_name)
        tag = REFERENCE_TAGS.get(program_name)
        so = build_ref.prebuilt(tag, prog.argument_string) if tag else None
        self.kind = "reference object" if so else "restatement"
        self.lib = ctypes.CDLL(so or build_restate.build(prog.argument_string))
        self.cfg = np.array(prog.cfg or [0.0], dtype="<f4")

    def camera(self, cart, flip):
        out = np.zeros((len(cart), 4), dtype="<f4")
        for i in range(len(cart)):
            self.lib.ref_cart_to_generic(_p(np.ascontiguousarray(cart[i], dtype="<f4")), _p(out[i]), ctypes.c_float(flip), _p(self.cfg))
        return out

    def tetrads(self, generic32, speeds):
        out = np.zeros((len(generic32), 4, 4), dtype="<f4")
        for i in range(len(generic32)):
            x, s = np.ascontiguousarray(generic32[i], dtype="<f4"), np.ascontiguousarray(speeds[i], dtype="<f4")
            self.lib.ref_init_basis_vectors(_p(x), _p(s), _p(out[i, 0]), _p(out[i, 1]), _p(out[i, 2]), _p(out[i, 3]), _p(self.cfg))
        return out

    def boosted(self, generic32, speeds, legs32):
        out = np.array(legs32, dtype="<f4")
        for i in range(len(generic32)):
            x, s = np.ascontiguousarray(generic32[i], dtype="<f4"), np.zeros(4, dtype="<f4")
            s[:3] = speeds[i]
            self.lib.ref_boost_tetrad(_p(x), _p(s), _p(out[i, 0]), _p(out[i, 1]), _p(out[i, 2]), _p(out[i, 3]), _p(self.cfg))
        return out

    def inertial(self, generic32, legs32, speeds):
        out = np.zeros(len(generic32), dtype=LIGHTRAY_DTYPE)
        count = np.zeros(1, dtype="<i4")
        for i in range(len(generic32)):
            x, s, e = np.ascontiguousarray(generic32[i], dtype="<f4"), np.zeros(4, dtype="<f4"), np.array(legs32[i], dtype="<f4")
            s[:3] = speeds[i]
            ray = np.zeros(1, dtype=LIGHTRAY_DTYPE)
            self.lib.ref_init_inertial_ray(_p(x), _p(ray), _p(count), _p(e[0]), _p(e[1]), _p(e[2]), _p(e[3]), _p(s), _p(self.cfg))
            out[i] = ray[0]
        return out

    def rays(self, generic32, quat, legs32, width, height, fov, flip):
        n = width * height
        rays, count, term = np.zeros(n, dtype=LIGHTRAY_DTYPE), np.zeros(1, dtype="<i4"), np.zeros(n, dtype="<i4")
        dfg = np.frombuffer(features_bytes(fov), dtype=np.uint8).copy()
        x, q, e = np.ascontiguousarray(generic32, dtype="<f4"), np.ascontiguousarray(quat, dtype="<f4"), np.array(legs32, dtype="<f4")
        self.lib.ref_init_rays_generic(_p(x), _p(q), _p(rays), _p(count), width, height, _p(term), width, height, int(flip), _p(e[0]), _p(e[1]),
                                       _p(e[2]), _p(e[3]), _p(self.cfg), _p(dfg), 0, 1)
        assert int(count[0]) == n
        return slot_order(rays, width, height)


def yardstick(program_name):
    if program_name not in _yardsticks:
        _yardsticks[program_name] = Yardstick(program_name)
    return _yardsticks[program_name]


def inertial_speeds(c):
    return c["speeds"] * np.float32(0.5)


def camera_errors(c, got):
    """per pose: vec_err of a camera case's outputs `got` (dict of fp32 arrays: camera, tetrad, reboosted, inertial) against the model;
    the camera's spatial part is the vector compared; its time, where the chart passes it through, is compared exactly (an error there
    counts as infinite), and relative to max(1, |t|) where the chart computes it"""
    m = camera_model(c)
    out = {}
    if c["cart"] is not None:
        space = vec_err(got["camera"][:, 1:], m["camera"][:, 1:])
        t_in, t_model, t_got = c["cart"][:, 0].astype(np.float64), m["camera"][:, 0], got["camera"][:, 0].astype(np.float64)
        with np.errstate(invalid="ignore"):
            through = np.where(t_got == t_in, 0.0, np.inf)
            computed = np.abs(t_got - t_model) / np.maximum(1.0, np.abs(t_model))
        time = np.where(t_model == t_in, through, np.where(np.isnan(computed), np.inf, computed))
        out["camera"] = np.where(np.isnan(space) | ~np.isfinite(t_model), np.nan, np.maximum(np.nan_to_num(space, nan=0.0), time))
    out["tetrad"] = np.stack([vec_err(got["tetrad"][:, a], m["tetrad"][:, a]) for a in range(4)]).max(axis=0)
    out["reboosted"] = np.stack([vec_err(got["reboosted"][:, a], m["reboosted"][:, a]) for a in range(4)]).max(axis=0)
    out["inertial"] = np.stack([vec_err(got["inertial"][f], m["inertial"][f]) for f in RAY_FIELDS]).max(axis=0)
    return out


def camera_invariants(c, got):
    """per pose: max |e_a.g.e_b - eta_ab| of the stored tetrads, g of the model at the camera the tetrad kernels were given (NaN where
    the model's own tetrad is not finite)"""
    m, prog = camera_model(c), program(c["program"])
    out = {}
    for key in ("tetrad", "reboosted"):
        v = np.full(c["count"], np.nan)
        for i in range(c["count"]):
            if np.isfinite(m[key][i]).all() and not m["trace"][i]["degenerate"]:
                fast = float(np.linalg.norm(c["speeds"][i].astype(np.float64))) >= RELATIVE_FROM
                r = tetrad_invariant(prog, m["generic32"][i], got[key][i], relative=fast)
                v[i] = r if np.isfinite(r) else np.inf
        out[key] = v
    return out


def yardstick_camera(c):
    """the yardstick's outputs of a camera case, its errors and invariants against the model, cached"""
    key = ("camera", c["name"])
    if key not in _figures:
        y, m = yardstick(c["program"]), camera_model(c)
        got = dict(tetrad=y.tetrads(m["generic32"], c["speeds"]), reboosted=y.boosted(m["generic32"], c["speeds"], m["unboosted32"]),
                   inertial=y.inertial(m["generic32"], m["tetrad32"], inertial_speeds(c)))
        if c["cart"] is not None:
            got["camera"] = y.camera(c["cart"], c["flip"])
        _figures[key] = (got, camera_errors(c, got), camera_invariants(c, got), y.kind)
    return _figures[key]


def frame_invariants(c, got):
    """per ray of a frame: (null residual, |ku - k.g.e0|, |spatial length - 1| or NaN, |rot(initial_quat) undoes the rotation| or NaN)"""
    prog, m = program(c["program"]), ray_model(c)
    e = m["tetrad32"].astype(np.float64)
    n = len(got)
    out = np.full((n, 4), np.nan)
    for i in range(n):
        if not all(np.isfinite(m["rays"][f][i]).all() for f in RAY_FIELDS):
            continue
        pos, vel = got["position"][i].astype(np.float64), got["velocity"][i].astype(np.float64)
        if not (np.isfinite(pos).all() and np.isfinite(vel).all()):
            out[i, :2] = np.inf
            continue
        rotated = prog.generic_constant_theta
        r = ray_invariants(prog, None if rotated else e, pos, vel, float(got["ku_uobsu"][i]), observer=e[0])
        out[i, :len(r)] = r
        if rotated:      # initial_quat turns the equatorial-plane direction of the camera back to where the camera is
            polar = prog.to_polar(pos)
            polar[1] = abs(polar[1])
            back = _rot_quat(_polar_to_cartesian(polar[1:]), got["initial_quat"][i].astype(np.float64))
            cam = prog.to_polar(m["generic32"].astype(np.float64))
            cam[1] = abs(cam[1])
            out[i, 3] = np.abs(back - _polar_to_cartesian(cam[1:])).max() / max(1.0, cam[1])
    return out


def yardstick_rays(c):
    key = ("rays", c["name"])
    if key not in _figures:
        y, m = yardstick(c["program"]), ray_model(c)
        got = y.rays(m["generic32"], c["quat"], m["tetrad32"], c["width"], c["height"], c["fov"], c["flip"])
        _figures[key] = (got, ray_errors(c, got), frame_invariants(c, got), y.kind)
    return _figures[key]


assert LIGHTRAY_DTYPE.itemsize == 96
