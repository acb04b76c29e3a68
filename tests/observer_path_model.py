"""A float64 model of the observer-path stage - parallel transport along a stored path and the interpolation of the stored path at a
proper time - and the hand-made paths it is held against (tests/test_observer_path_model.py on the CPU,
tests/test_gpu_observer_path.py on the device).

The model restates gr_parallel_transport_quantity and gr_handle_interpolating_geodesic (kernels/geodesic_camera.hip) in numpy and
float64.  It follows the discrete algorithm, not the physics: the same branches in the same order.
  * g and its partial derivatives come from Metric.evaluate (the host's double evaluator of the generated expressions, the
    derivatives as [k][i][j] = d g_ij / d x^k); the inverse is numpy.linalg.inv.  tests/test_observer_path_model.py holds the
    derivatives to central differences of g (model_common.JACOBIAN_STEP's step rule) at every sample of every case.
  * A stage's input is the fp32 array the stage before would have stored; the paths are made by hand and are no geodesics: the
    kernels integrate and mix whatever they are given.
  * The interpolation's running proper time is the kernel's sequential fp32 sum: it decides a branch, so it is the fp32 value the
    stage is defined by.  Everything after the branch is float64.

The rule, per value (one 4-vector of one observer at one step): the device's vec_err against the model is at most
max(floor, WIDEN x the fp32 yardstick's vec_err on that same value); copies are compared bit for bit.  The floors: INTERPOLATION_FLOOR
for the pure mix, setup_model.CAMERA_FLOOR for recomputed tetrads, setup_model.RAY_FLOOR for the first path records and
TRANSPORT_FLOOR, measured from the yardstick (profiles/observer_path_synthetic.txt), for transport - times count / 8 on paths longer
than 8 samples.

Every path has at most MAX_SAMPLES samples and every launch at most MAX_OBSERVERS observers."""
import ctypes

import numpy as np

import geodesic_raytracing_amd as gra
import gpu_stages
import setup_model as sm
from model_common import JACOBIAN_STEP
from oracle import build_restate
from oracle.refpipe import OraclePipeline, pack_features

SEED = 20250301
MAX_SAMPLES, MAX_OBSERVERS = 40, 70
WIDEN = sm.WIDEN
INTERPOLATION_FLOOR = 1e-5      # tests/test_gpu_geodesic_camera.py::test_interpolation_from_golden_path's tolerance of the pure mix
# profiles/observer_path_synthetic.txt: the largest vec_err of the yardstick against the model over the ordinary transport cases of 8
# samples or fewer is TRANSPORT_MEASURED; doubled for a second fp32 evaluation order and rounded up to one significant digit
TRANSPORT_MEASURED = 1.51e-7     # schwarzschild_ingoing_ef_8_ratio_100, the restatement (no reference object is built for that program)
TRANSPORT_FLOOR = 4e-7
# central differences against the generated derivatives, relative to max(1, max |dg|) at the sample: see central_derivatives.  On the
# set-aside path |dg| reaches 2 500, so the check tolerates 0.025 there in absolute terms; the ordinary kerr_boyer cases hold the same
# generated expressions where |dg| is of order 1.
DERIVATIVE_BOUND = 1e-5
# The set-aside case.  Two fp32 evaluations of it that are both right - the CPU restatement and the reference's own object - do not
# meet the per-value rule against each other: on 26 of its 85 values one is beyond max(floor, 1.5 x the other), by a factor of up to 12
# (and so on every other path drawn to 1.02 of the horizon's radius: shorter, steeper, ending at the dip).  An error there is one draw
# of the rounding at the ill-conditioned samples, carried along the rest of the path.  So on this case the size of an error is held to
# the yardstick's largest over the case, doubled - the factor TRANSPORT_FLOOR takes from a yardstick's maximum to a bound on a second
# fp32 evaluation order - and the number of values beyond the floor to the yardstick's, both ways, within 1.5 x + 2.
SET_ASIDE_WIDEN = 2.0


def transport_floor(count):
    return TRANSPORT_FLOOR * max(1.0, count / 8)


def vec_err(got, want):
    """gpu_stages.vec_err with a floor of 1, the largest component per 4-vector; NaN where the model's own vector is not finite (nothing
    is compared there), inf where only `got` is not"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = gpu_stages.vec_err(got, want, floor=1.0).max(axis=-1)
    return np.where(np.isfinite(want).all(axis=-1), np.where(np.isnan(err), np.inf, err), np.nan)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def metric_derivatives(prog, x):
    """d g_ij / d x^k as [k][i][j] from the generated expressions"""
    return prog._eval(gra.EVAL_METRIC_DERIVATIVES, np.asarray(x, dtype=np.float64)).reshape(4, 4, 4)


def central_derivatives(prog, x):
    """the same by central differences of g, step JACOBIAN_STEP * max(1, |x_k|) = h: truncation h^2 g''' / 6 and rounding 1e-16 |g| / h,
    1e-10 and 1e-11 of the scale of g on a smooth metric - and 1e-6 of d g where g varies on a scale of 0.02 (the set-aside path at 1.02 of
    a horizon radius); a derivative in the wrong slot is wrong by the size of d g itself"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((4, 4, 4))
    for k in range(4):
        h = JACOBIAN_STEP * max(1.0, abs(x[k]))
        up, down = x.copy(), x.copy()
        up[k] += h
        down[k] -= h
        out[k] = (prog.g(up) - prog.g(down)) / (2 * h)
    return out


def connection(prog, x, dg=None):
    """Gamma^a_bs = 1/2 g^-1[a][m] (d_s g_mb + d_b g_ms - d_m g_bs) at chart position x -> [a][b][s]"""
    x = np.asarray(x, dtype=np.float64)
    dg = metric_derivatives(prog, x) if dg is None else dg
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        try:
            ginv = np.linalg.inv(prog.g(x))
        except np.linalg.LinAlgError:
            ginv = np.full((4, 4), np.nan)
        lowered = np.einsum("smb->mbs", dg) + np.einsum("bms->mbs", dg) - dg      # (dg itself is [m][b][s] = d_m g_bs)
        return 0.5 * np.einsum("am,mbs->abs", ginv, lowered)


def transport_velocity(prog, X, x, v, gamma=None):
    """parallel_transport_velocity: dX^a / dlambda = -Gamma^a_bs X^b Y^s of quantity X at position x along velocity v"""
    gamma = connection(prog, x) if gamma is None else gamma
    with np.errstate(invalid="ignore", over="ignore"):
        return -np.einsum("abs,b,s->a", gamma, np.asarray(X, dtype=np.float64), np.asarray(v, dtype=np.float64))


def connections(prog, path32, count):
    return [connection(prog, path32[k]) for k in range(count)]


def transport(prog, path32, vel32, ds32, q32, count=None, gammas=None):
    """gr_parallel_transport_quantity of one observer: the Heun step over count - 1 segments -> records [count][4]; count 0 writes
    nothing, count 1 the input.  `gammas`: connections(prog, path32, count) where several quantities ride one path."""
    count = len(path32) if count is None else count
    out = np.zeros((count, 4))
    if count == 0:
        return out
    current = np.asarray(q32, dtype=np.float64).copy()
    out[0] = current
    if count == 1:
        return out
    vel, ds = np.asarray(vel32, dtype=np.float64), np.asarray(ds32, dtype=np.float64)
    gammas = connections(prog, path32, count) if gammas is None else gammas
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(count - 1):
            f = transport_velocity(prog, current, None, vel[k], gammas[k])
            predictor = current + f * ds[k]
            following = current + (0.5 * ds[k]) * (f + transport_velocity(prog, predictor, None, vel[k + 1], gammas[k + 1]))
            out[k] = current
            current = following
    out[count - 1] = current
    return out


def interpolate(prog, path32, vel32, ds32, legs32, target, count, parallel_transport, speed):
    """gr_handle_interpolating_geodesic: legs32 [4][n][4] -> dict(camera, velocity, tetrad [4][4], branch = (segment, dx, exit)); the
    exits are "empty" (count 0: nothing is written, the three values are None), "single" (count 1), "before" (the target precedes the
    segment: dx is overridden to 0), "inside" and "last" (the fall-through)"""
    if count == 0:
        return dict(camera=None, velocity=None, tetrad=None, branch=(-1, 0.0, "empty"))
    path, vel, legs = (np.asarray(a, dtype=np.float64) for a in (path32, vel32, legs32))

    def tetrad_at(x, mixed):
        return mixed if parallel_transport else sm.tetrad(prog, x, np.asarray(speed, dtype=np.float32))

    def sample(i, which):
        return dict(camera=path[i].copy(), velocity=vel[i].copy(), tetrad=tetrad_at(path[i], legs[:, i].copy()), branch=(i, 0.0, which))

    if count == 1:
        return sample(0, "single")
    target = np.float32(target)
    proper_time = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(count - 1):
            next_proper_time = np.float32(proper_time + np.float32(ds32[i]))
            if (target >= proper_time and target < next_proper_time) or target < proper_time:
                before = bool(target < proper_time)
                dx = 0.0 if before else (float(target) - float(proper_time)) / (float(next_proper_time) - float(proper_time))
                mix = lambda a, b: a + (b - a) * dx
                fin = mix(path[i], path[i + 1])
                return dict(camera=fin, velocity=mix(vel[i], vel[i + 1]), tetrad=tetrad_at(fin, mix(legs[:, i], legs[:, i + 1])),
                            branch=(i, dx, "before" if before else "inside"))
            proper_time = next_proper_time
    return sample(count - 1, "last")


# ---- the fp32 yardsticks -----------------------------------------------------------------------------------------------------------
_pipes = {}


def yardstick_pipeline(program_name):
    """(OraclePipeline, kind) of the stage's yardstick: the reference's own object where one is built for the program's string, the
    CPU restatement otherwise (setup_model.Yardstick)"""
    key = ("yardstick", program_name)
    if key not in _pipes:
        y = sm.yardstick(program_name)
        _pipes[key] = (OraclePipeline(y.lib), y.kind)
    return _pipes[key]


def restatement_pipeline(program_name):
    key = ("restatement", program_name)
    if key not in _pipes:
        _pipes[key] = (OraclePipeline(build_restate.build(sm.program(program_name).argument_string)), "restatement")
    return _pipes[key]


def features_bytes(**overrides):
    return pack_features(adaptive_sampling=0, **overrides)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _frozen(c):
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _curve(prog, polar_at, ds32):
    """samples of the curve polar_at(lambda) (t, r, theta, phi) at the running sums of ds32, in the program's chart -> (path32, vel32);
    the velocity is the chart tangent by central differences"""
    lam = np.concatenate([[0.0], np.cumsum(ds32[:-1].astype(np.float64))])
    at = lambda l: prog.from_polar(np.asarray(polar_at(l), dtype=np.float64))
    h = 1e-4
    path = np.stack([at(l) for l in lam])
    vel = np.stack([(at(l + h) - at(l - h)) / (2 * h) for l in lam])
    assert np.isfinite(path).all() and np.isfinite(vel).all()
    return path.astype(np.float32), vel.astype(np.float32)


def _line(rng, r_lo=3.6, r_hi=10.0):
    """a smooth curve: each polar coordinate linear in lambda, r >= r_lo - 2 and theta within 32 degrees of the equator over the 8 units
    of lambda a path of 40 samples spans"""
    start = np.array([rng.uniform(-5, 5), rng.uniform(r_lo, r_hi), np.radians(rng.uniform(50, 130)), rng.uniform(-2.5, 2.5)])
    rate = np.array([rng.uniform(1.1, 1.5), rng.uniform(-0.25, 0.25), rng.uniform(-0.04, 0.04), rng.uniform(-0.08, 0.08)])
    return lambda l: start + rate * l


def _steps(kind, n):
    if kind == "uniform":
        ds = np.full(n, 0.2)
    elif kind == "ratio_100":      # 0.004 and 0.4 in turn
        ds = np.where(np.arange(n) % 2 == 0, 0.004, 0.4)
    else:      # one zero entry, in the first segment of a path of two samples and inside a longer one
        ds = np.full(n, 0.2)
        ds[0 if n == 2 else n // 2] = 0.0
    return ds.astype(np.float32)


ARBITRARY = np.array([0.7, -1.3, 0.4, 2.1], dtype=np.float32)      # the fifth quantity: no leg, not of unit length
TRANSPORT_PROGRAMS = ["kerr_boyer", "schwarzschild", "schwarzschild_ingoing_ef", "kerr_schild", "alcubierre", "wormhole", "double_unequal_kerr",
                      "minkowski"]
SAMPLES = (2, 3, 8, 40)
STEP_KINDS = ("uniform", "ratio_100", "zero_entry")


def _quantities(prog, path32):
    """the four legs of the tetrad at the first sample and the arbitrary vector, fp32 [5][4]"""
    legs = sm.tetrad(prog, path32[0].astype(np.float64))
    assert np.isfinite(legs).all()
    return np.concatenate([legs, ARBITRARY[None].astype(np.float64)]).astype(np.float32)


def _transport_case(name, kind, program, path32, vel32, ds32, reaches, quantities=None, count=None):
    prog = sm.program(program)
    count = len(path32) if count is None else count
    assert count <= len(path32) <= MAX_SAMPLES
    return _frozen(dict(name=name, kind=kind, program=program, path32=path32, vel32=vel32, ds32=ds32, count=count,
                        quantities32=_quantities(prog, path32) if quantities is None else quantities, reaches=reaches,
                        substituted=program in sm.SUBSTITUTED))


def _build_transport_cases():
    out = []
    rng = np.random.default_rng(SEED)
    for j, program in enumerate(TRANSPORT_PROGRAMS):
        prog = sm.program(program)
        for i, n in enumerate(SAMPLES):      # every program meets every number of samples, and the kinds of step in turn
            steps = STEP_KINDS[(i + j) % 3]
            ds32 = _steps(steps, n)
            far = program == "double_unequal_kerr"      # (the two holes of that metric sit on the axis at |z| <= 2.5)
            path32, vel32 = _curve(prog, _line(rng, 7.0 if far else 3.6, 12.0 if far else 10.0), ds32)
            out.append(_transport_case(f"{program}_{n}_{steps}", "ordinary", program, path32, vel32, ds32,
                                       f"{n} samples, ds {steps}" + (": d g = 0, every record is the input" if program == "minkowski" else "")))
    # off-diagonal heavy: near-extremal Kerr next to the equator, a mostly azimuthal velocity - the g_t_phi terms carry the result
    prog = sm.program("kerr_boyer_near_extremal")
    start, rate = np.array([0.5, 1.6, np.pi / 2 - 0.02, 0.3]), np.array([1.2, 0.02, 0.005, 0.9])
    ds32 = _steps("uniform", 8)
    path32, vel32 = _curve(prog, lambda l: start + rate * l, ds32)
    out.append(_transport_case("off_diagonal_kerr", "ordinary", "kerr_boyer_near_extremal", path32, vel32, ds32,
                               "a = 0.4999 at r = 1.6 rs, 0.02 from the equator, d phi / d lambda = 0.9: the g_t_phi terms carry the result"))
    # set aside: the path dips to 1.02 of the outer horizon's radius of Kerr (a = 0.45) in Boyer-Lindquist coordinates, where the inverse
    # of g is ill-conditioned (g_rr = 1 / 0.02 there)
    prog = sm.program("kerr_boyer")
    horizon = (1 + np.sqrt(1 - 4 * 0.45 ** 2)) / 2
    ds32 = np.full(17, 0.1, dtype=np.float32)
    total = 1.6
    dip = lambda l: np.array([1.2 * l, horizon * (1.02 + 1.2 * (l / total - 0.5) ** 2), 1.2 + 0.1 * l, -0.4 + 0.3 * l])
    path32, vel32 = _curve(prog, dip, ds32)
    assert abs(path32[8, 1] / horizon - 1.02) < 1e-3
    out.append(_transport_case("set_aside_horizon_kerr_boyer", "set_aside", "kerr_boyer", path32, vel32, ds32,
                               "set aside: from 1.32 to 1.02 of the horizon's radius and back, 17 samples"))
    return out


OBSERVER_COUNTS = (40, 0, 2, 3, 17, 1)


def _build_observers_case():
    """70 observers in one launch, each on a path of its own with a count of its own: 40, 0, 2, 3, 17, 1 in turn, and 40, 0, 40, 1 in
    lanes 62 to 65 - a lane with count 0 or 1 next to one with 40 on either side of the wave's edge.  Every lane holds 40 samples
    whatever its count, so a neighbour's count or a wrong stride reads values that are there.  Step-major: [k * 70 + id]."""
    rng = np.random.default_rng(SEED + 1)
    prog = sm.program("kerr_boyer")
    n, m = MAX_OBSERVERS, MAX_SAMPLES
    counts = np.array([OBSERVER_COUNTS[i % 6] for i in range(n)], dtype=np.int32)
    counts[62:66] = (40, 0, 40, 1)
    path, vel, ds = np.zeros((m, n, 4), dtype=np.float32), np.zeros((m, n, 4), dtype=np.float32), np.zeros((m, n), dtype=np.float32)
    quantity = np.zeros((n, 4), dtype=np.float32)
    for i in range(n):
        ds[:, i] = _steps(STEP_KINDS[i % 3], m) * np.float32(rng.uniform(0.5, 1.0))
        path[:, i], vel[:, i] = _curve(prog, _line(rng), ds[:, i])
        quantity[i] = _quantities(prog, path[:, i])[i % 5]
    return _frozen(dict(name="observers_70_kerr_boyer", program="kerr_boyer", path32=path, vel32=vel, ds32=ds, counts=counts, quantity32=quantity))


# the interpolation: ds of exactly representable values, so that the fp32 running sum is exact: 0, 0.25, 0.75, 0.875, 1.125, 1.5, 2, 2.25,
# 2.375 (the ninth entry belongs to no segment)
EXACT_DS = (0.25, 0.5, 0.125, 0.25, 0.375, 0.5, 0.25, 0.125, 0.25)
EXACT_TOTAL = 2.375
# (name, target, (segment, dx, exit)) on the path of nine samples
EXACT_TARGETS = [
    ("negative", -1.0, (0, 0.0, "before")),
    ("zero_first_sample", 0.0, (0, 0.0, "inside")),
    ("inner_sample", 0.875, (3, 0.0, "inside")),
    ("dx_2^-20", 0.25 + 0.5 * 2.0 ** -20, (1, 2.0 ** -20, "inside")),
    ("dx_half", 0.5, (1, 0.5, "inside")),
    ("dx_1-2^-20", 0.75 - 0.5 * 2.0 ** -20, (1, 1 - 2.0 ** -20, "inside")),
    ("last_segment", 2.3125, (7, 0.5, "inside")),
    ("last_sample_total", EXACT_TOTAL, (8, 0.0, "last")),
    ("past_total", 10.0, (8, 0.0, "last")),
    ("plus_inf", np.inf, (8, 0.0, "last")),
    ("nan", np.nan, (8, 0.0, "last")),
]
TWO_TARGETS = [("negative", -0.5, (0, 0.0, "before")), ("dx_half", 0.125, (0, 0.5, "inside")), ("total", 0.25, (1, 0.0, "last")),
               ("past_total", 3.0, (1, 0.0, "last"))]
INTERPOLATION_PROGRAMS = ["kerr_boyer", "kerr_schild", "minkowski"]      # spherical-type, Cartesian-type, flat
SPEEDS = np.array([[0.2, -0.1, 0.3], [0.5, -0.6, 0.45]], dtype=np.float32)      # |v| = 0.37 and 0.9: the recomputed-tetrad mode's basis_speed
INEXACT_FRACTIONS = ((0, 0.3), (3, 0.62), (5, 1e-4), (7, 1 - 1e-4))      # (segment, dx) on the path whose ds is not representable


def _interpolation_case(name, program, rng, ds, count, targets, reaches):
    prog = sm.program(program)
    ds32 = np.asarray(ds, dtype=np.float32)
    # (the curve is sampled as if a zero entry were 0.2: the two samples that share a time differ in value)
    path32, vel32 = _curve(prog, _line(rng, 4.0, 9.0), np.where(ds32 == 0, np.float32(0.2), ds32))
    legs32 = rng.uniform(-2, 2, (4, len(ds32), 4)).astype(np.float32)      # whatever a stage before stored: the kernel mixes them
    return _frozen(dict(name=name, program=program, path32=path32, vel32=vel32, ds32=ds32, legs32=legs32, count=count, targets=list(targets),
                        reaches=reaches))


def _build_interpolation_cases():
    out = []
    rng = np.random.default_rng(SEED + 2)
    for program in INTERPOLATION_PROGRAMS:
        out.append(_interpolation_case(f"{program}_nine", program, rng, EXACT_DS, 9, EXACT_TARGETS, "every exit of a path of nine samples, exact ds"))
        out.append(_interpolation_case(f"{program}_two", program, rng, EXACT_DS[:2], 2, TWO_TARGETS, "count 2: one segment"))
        out.append(_interpolation_case(f"{program}_one", program, rng, EXACT_DS[:2], 1, [("any", 0.1, (0, 0.0, "single"))], "count 1: the first sample"))
        out.append(_interpolation_case(f"{program}_none", program, rng, EXACT_DS[:2], 0, [("any", 0.1, (-1, 0.0, "empty"))], "count 0: nothing is written"))
        # a segment of length zero and a target equal to its time: sample 1 and sample 2 share the time 0.25 and differ in value, the
        # segment after them is chosen with dx = 0: the result is sample 2
        out.append(_interpolation_case(f"{program}_zero_segment", program, rng, (0.25, 0.0, 0.5, 0.25), 4, [("on_the_pair", 0.25, (2, 0.0, "inside"))],
                                       "a zero-length segment, the target at its time: the next segment, no division by zero"))
        ds = rng.uniform(0.05, 0.4, 9).astype(np.float32)
        sums = np.concatenate([[np.float32(0)], np.cumsum(ds[:-1], dtype=np.float32)])      # numpy sums a short fp32 array in sequence
        targets = [(f"segment_{i}_dx_{dx:g}", float(np.float32(float(sums[i]) + dx * float(ds[i]))), (i, dx, "inside")) for i, dx in INEXACT_FRACTIONS]
        out.append(_interpolation_case(f"{program}_inexact", program, rng, ds, 9, targets,
                                       "ds that is not representable, targets at least 1e-4 of the segment from its ends"))
    return out


_cases = {}


def transport_cases():
    if "transport" not in _cases:
        _cases["transport"] = _build_transport_cases()
    return _cases["transport"]


def observers_case():
    if "observers" not in _cases:
        _cases["observers"] = _build_observers_case()
    return _cases["observers"]


def interpolation_cases():
    if "interpolation" not in _cases:
        _cases["interpolation"] = _build_interpolation_cases()
    return _cases["interpolation"]


TRANSPORT_CASE_NAMES = [f"{p}_{n}_{STEP_KINDS[(i + j) % 3]}" for j, p in enumerate(TRANSPORT_PROGRAMS) for i, n in enumerate(SAMPLES)] + [
    "off_diagonal_kerr", "set_aside_horizon_kerr_boyer"]
INTERPOLATION_CASE_NAMES = [f"{p}_{k}" for p in INTERPOLATION_PROGRAMS for k in ("nine", "two", "one", "none", "zero_segment", "inexact")]


TRANSPORT_CASE_PROGRAMS = dict({f"{p}_{n}_{STEP_KINDS[(i + j) % 3]}": p for j, p in enumerate(TRANSPORT_PROGRAMS) for i, n in enumerate(SAMPLES)},
                               off_diagonal_kerr="kerr_boyer_near_extremal", set_aside_horizon_kerr_boyer="kerr_boyer")
SUBSTITUTED_CASE_NAMES = [n for n in TRANSPORT_CASE_NAMES if TRANSPORT_CASE_PROGRAMS[n] in sm.SUBSTITUTED]      # (no case is built for this list)


def transport_case(name):
    return next(c for c in transport_cases() if c["name"] == name)


def interpolation_case(name):
    return next(c for c in interpolation_cases() if c["name"] == name)


def case_bytes():
    """every input of every case, for the determinism test"""
    parts = []
    for c in transport_cases() + interpolation_cases() + [observers_case()]:
        parts += [c["name"].encode()] + [a.tobytes() for a in c.values() if isinstance(a, np.ndarray)]
    return b"".join(parts)


# ---- the model and the yardstick on the cases --------------------------------------------------------------------------------------
def transport_model(c):
    """records [5][count][4] of a transport case, cached"""
    if "_model" not in c:
        prog = sm.program(c["program"])
        gammas = connections(prog, c["path32"], c["count"])
        c["_model"] = np.stack([transport(prog, c["path32"], c["vel32"], c["ds32"], q, c["count"], gammas) for q in c["quantities32"]])
    return c["_model"]


def transport_errors(c, got):
    """vec_err [5][count] of records `got` [5][count][4] against the model"""
    return vec_err(got, transport_model(c))


def yardstick_transport(c, pipeline=yardstick_pipeline):
    """(records [5][count][4] fp32, their errors, which yardstick) of a transport case"""
    pipe, kind = pipeline(c["program"])
    cfg = sm.program(c["program"]).cfg
    got = np.stack([pipe.parallel_transport(c["path32"], c["vel32"], c["ds32"], q, c["count"], cfg)[:c["count"]] for q in c["quantities32"]])
    return got, transport_errors(c, got), kind


def observers_model(c, lane):
    """the model's records [counts[lane]][4] of one lane of the launch of 70"""
    key = ("_model", lane)
    if key not in c:
        c[key] = transport(sm.program(c["program"]), c["path32"][:, lane], c["vel32"][:, lane], c["ds32"][:, lane], c["quantity32"][lane],
                           int(c["counts"][lane]))
    return c[key]


def interpolation_runs(c):
    """every launch of an interpolation case: (label, target, expected branch, parallel_transport, speed) - each target with transported
    legs and with tetrads recomputed at the slower speed, and at |v| = 0.9 the targets that fall strictly between two samples"""
    runs = []
    for label, target, branch in c["targets"]:
        runs.append((label, target, branch, 1, SPEEDS[0]))
        runs.append((label, target, branch, 0, SPEEDS[0]))
        if branch[2] == "inside" and 0 < branch[1] < 1:
            runs.append((label, target, branch, 0, SPEEDS[1]))
    return runs


def interpolation_model(c):
    """the model of every run of a case, cached, in interpolation_runs' order"""
    if "_model" not in c:
        prog = sm.program(c["program"])
        c["_model"] = [interpolate(prog, c["path32"], c["vel32"], c["ds32"], c["legs32"], target, c["count"], pt, speed)
                       for _, target, _, pt, speed in interpolation_runs(c)]
    return c["_model"]


FILL = np.float32(-77.25)      # what the yardstick's outputs hold before a call


def yardstick_interpolation(c, pipeline=yardstick_pipeline):
    """([(camera, tetrad, velocity) fp32 per run], which yardstick); outputs nothing wrote hold FILL"""
    pipe, kind = pipeline(c["program"])
    cfg = sm.program(c["program"]).cfg
    return [pipe.interpolate(c["path32"], c["vel32"], c["ds32"], c["legs32"], target, c["count"], pt, speed, cfg, fill=FILL)
            for _, target, _, pt, speed in interpolation_runs(c)], kind


def is_copy(model, parallel_transport):
    """does this exit store samples unchanged?  (camera and velocity, the legs too)"""
    unchanged = model["branch"][2] in ("single", "last")
    return unchanged, unchanged and bool(parallel_transport)


def interpolation_errors(model, got):
    """vec_err of one run's (camera, tetrad, velocity) against the model -> [6]: camera, velocity, four legs"""
    camera, tetrad, velocity = got
    return np.concatenate([vec_err(camera, model["camera"])[None], vec_err(velocity, model["velocity"])[None], vec_err(tetrad, model["tetrad"])])


def interpolation_floors(parallel_transport):
    """the floor of each of interpolation_errors' six values: the mix's for camera, velocity and transported legs, the camera stage's for
    recomputed legs"""
    leg = INTERPOLATION_FLOOR if parallel_transport else sm.CAMERA_FLOOR
    return np.array([INTERPOLATION_FLOOR, INTERPOLATION_FLOOR, leg, leg, leg, leg])


def assert_set_aside(name, floor, err, yardstick_err):
    """the set-aside case's bounds (SET_ASIDE_WIDEN has the argument): every value within max(floor, 2 x the yardstick's largest error
    over the case), and the counts of values beyond the floor equal within 1.5 x + 2, both ways -> (count, the yardstick's count)"""
    err, y = np.asarray(err, dtype=np.float64), np.asarray(yardstick_err, dtype=np.float64)
    assert np.isfinite(err).all() and np.isfinite(y).all(), name
    limit = max(floor, SET_ASIDE_WIDEN * float(y.max()))
    assert float(err.max()) <= limit, (name, "largest error, bound, the yardstick's largest", float(err.max()), limit, float(y.max()))
    over, yard_over = int((err > floor).sum()), int((y > floor).sum())
    assert over <= WIDEN * yard_over + 2 and yard_over <= WIDEN * over + 2, (name, "values beyond the floor: mine, the yardstick's", over, yard_over)
    return over, yard_over


def assert_by_the_rule(name, floor, err, yardstick_err):
    """per value: err <= max(floor, WIDEN x the yardstick's error on that value); where the model (NaN) or the yardstick (inf) is not
    finite nothing is compared -> (values compared, values set aside)"""
    err, y = np.asarray(err, dtype=np.float64), np.asarray(yardstick_err, dtype=np.float64)
    floor = np.broadcast_to(np.asarray(floor, dtype=np.float64), err.shape)
    assert (np.isnan(err) == np.isnan(y)).all(), name
    compared = ~np.isnan(err) & np.isfinite(y)
    limit = np.maximum(floor, WIDEN * np.where(compared, y, 0.0))
    over = compared & ~(err <= limit)
    assert not over.any(), (name, "values over their bound (index, error, bound, yardstick)",
                            [(tuple(int(v) for v in i), float(err[tuple(i)]), float(limit[tuple(i)]), float(y[tuple(i)])) for i in np.argwhere(over)][:8])
    return int(compared.sum()), int((~compared).sum())
