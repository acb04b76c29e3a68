"""GPU tests (-m gpu) of the observer-path stage on paths made by hand: gr_parallel_transport_quantity and
gr_handle_interpolating_geodesic (kernels/geodesic_camera.hip) against the float64 model of tests/observer_path_model.py on the
cases that module lists, and gr_get_geodesic_path structurally and on its first eight records.

The rule, per value (one 4-vector of one observer at one step): the device's vec_err against the model is at most
max(floor, 1.5 x the fp32 yardstick's on that same value).  The yardstick is the reference's own object where one is built for the
program's string and the CPU restatement otherwise, computed here; tests/test_observer_path_model.py asserts that on ordinary cases
the floor is the bound that applies.  The floors: 1e-5 for the interpolation's mix, setup_model.CAMERA_FLOOR for recomputed tetrads,
setup_model.RAY_FLOOR for the first path records, observer_path_model.TRANSPORT_FLOOR (measured from the yardstick) for transport.
Values that are copies - the record at step 0, a count of 1, the interpolation's exits that store a sample - are compared bit for
bit.  On the one set-aside case two right fp32 evaluations do not meet that rule against each other
(observer_path_model.SET_ASIDE_WIDEN): there every value is held to twice the yardstick's largest error over the case, and the number
of values beyond the floor to the yardstick's, both ways, within 1.5 x + 2.

Every output sits between eight records of guard bytes, and what a kernel must not write keeps its fill bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import observer_path_model as om  # noqa: E402
import setup_model as sm  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from test_gpu_setup import GUARD_BYTE, Guarded, device_program, init_inertial_ray, up  # noqa: E402


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == GUARD_BYTE).all()


# ---- transport ---------------------------------------------------------------------------------------------------------------------
def transport_launch(p, cfg, path, vel, ds, quantity, counts):
    """one launch of len(counts) observers on step-major arrays [records][n] -> records [records][n][4], fill bytes where none was written"""
    records, n = path.shape[0], len(counts)
    assert path.shape == vel.shape == (records, n, 4) and ds.shape == (records, n) and quantity.shape == (n, 4) and (counts <= records).all()
    out = Guarded(records * n, 16)
    d_path, d_vel, d_ds, d_q, d_counts = up(path), up(vel), up(ds), up(quantity), up(counts.astype(np.int32))
    check(lib.gr_parallel_transport_quantity(p.handle, None, d_path.ptr, d_vel.ptr, d_ds.ptr, d_q.ptr, d_counts.ptr, n, out.ptr, cfg.ptr))
    check(lib.gr_device_synchronize(0))
    return out.read(np.float32, (records, n, 4))


def transport_alone(p, cfg, path, vel, ds, quantity, count):
    """one observer -> records [len(path)][4]"""
    return transport_launch(p, cfg, path[:, None], vel[:, None], ds[:, None], quantity[None], np.array([count]))[:, 0]


def assert_transport_case(c, substituted):
    p, cfg = device_program(c["program"], substituted)
    n = c["count"]
    got = np.stack([transport_alone(p, cfg, c["path32"], c["vel32"], c["ds32"], q, n) for q in c["quantities32"]])
    assert untouched(got[:, n:])
    got = got[:, :n]
    assert got[:, 0].tobytes() == c["quantities32"].tobytes(), "the record at step 0 is the input"
    yard, yard_err, kind = om.yardstick_transport(c)
    err = om.transport_errors(c, got)
    floor = om.transport_floor(n)
    program = "substituted" if substituted else "dynamic"
    print(f"{c['name']} [{program}]: gpu {np.nanmax(err):.2e} yardstick ({kind}) {np.nanmax(yard_err):.2e} floor {floor:.1e}")
    aside = ~(np.isfinite(om.transport_model(c)).all(axis=-1) & np.isfinite(yard).all(axis=-1))
    assert (np.isfinite(got)[aside] == np.isfinite(yard)[aside]).all(), "the pattern of finite components is the yardstick's"
    if c["program"] == "minkowski":      # d g = 0: every record is the input
        assert (got == c["quantities32"][:, None, :]).all()
    if c["kind"] == "ordinary":
        om.assert_by_the_rule(c["name"], floor, err, yard_err)
    else:      # set aside (observer_path_model.SET_ASIDE_WIDEN): the size by the yardstick's largest error, the counts both ways
        over, yard_over = om.assert_set_aside(c["name"], floor, err, yard_err)
        print(f"{c['name']} [{program}]: values beyond the floor: gpu {over} yardstick {yard_over} of {err.size}")


@pytest.mark.parametrize("name", om.TRANSPORT_CASE_NAMES)
def test_transport_against_the_float64_model(name):
    assert_transport_case(om.transport_case(name), False)


@pytest.mark.parametrize("name", om.SUBSTITUTED_CASE_NAMES)
def test_transport_of_the_substituted_program_against_the_float64_model(name):
    assert_transport_case(om.transport_case(name), True)


def test_seventy_observers_share_one_transport_launch():
    """70 paths with counts of 0, 1, 2, 3, 17 and 40 in one launch: every lane's records are those of its own launch alone, bit for
    bit, and within the rule of the model; records from a lane's count on, and the whole column of a lane with count 0, keep their fill
    bytes"""
    c = om.observers_case()
    p, cfg = device_program(c["program"])
    counts = c["counts"]
    whole = transport_launch(p, cfg, c["path32"], c["vel32"], c["ds32"], c["quantity32"], counts)
    pipe, kind = om.yardstick_pipeline(c["program"])
    worst = 0.0
    for lane in range(len(counts)):
        n = int(counts[lane])
        assert untouched(whole[n:, lane]), (lane, n)
        path, vel, ds = (np.ascontiguousarray(c[k][:, lane]) for k in ("path32", "vel32", "ds32"))
        alone = transport_alone(p, cfg, path, vel, ds, c["quantity32"][lane], n)
        assert alone.tobytes() == whole[:, lane].tobytes(), (lane, n)
        if n:
            assert whole[0, lane].tobytes() == c["quantity32"][lane].tobytes()
            model = om.observers_model(c, lane)
            yard = pipe.parallel_transport(path, vel, ds, c["quantity32"][lane], n, sm.program(c["program"]).cfg)[:n]
            err = om.vec_err(whole[:n, lane], model)
            om.assert_by_the_rule(f"{c['name']} lane {lane}", om.transport_floor(n), err, om.vec_err(yard, model))
            worst = max(worst, float(err.max()))
    print(f"{c['name']}: gpu {worst:.2e} (yardstick: {kind})")


# ---- interpolation -----------------------------------------------------------------------------------------------------------------
def interpolate_launch(p, cfg, c, target, parallel_transport, speed):
    """-> (camera [4], tetrad [4][4], velocity [4]); fill bytes where nothing was written"""
    camera, velocity, e = Guarded(1, 16), Guarded(1, 16), [Guarded(1, 16) for _ in range(4)]
    speed4 = np.zeros(4, dtype=np.float32)
    speed4[:3] = speed
    d_path, d_vel, d_ds, d_speed, d_count = up(c["path32"]), up(c["vel32"]), up(c["ds32"]), up(speed4), up(np.array([c["count"]], dtype=np.int32))
    legs = [up(c["legs32"][a]) for a in range(4)]
    check(lib.gr_handle_interpolating_geodesic(p.handle, None, d_path.ptr, d_vel.ptr, d_ds.ptr, camera.ptr, legs[0].ptr, legs[1].ptr, legs[2].ptr,
                                               legs[3].ptr, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, float(target), d_count.ptr,
                                               int(parallel_transport), d_speed.ptr, velocity.ptr, cfg.ptr))
    check(lib.gr_device_synchronize(0))
    return camera.read(np.float32, (4,)), np.stack([b.read(np.float32, (4,)) for b in e]), velocity.read(np.float32, (4,))


@pytest.mark.parametrize("name", om.INTERPOLATION_CASE_NAMES)
def test_interpolation_against_the_float64_model(name):
    c = om.interpolation_case(name)
    p, cfg = device_program(c["program"])
    yards, kind = om.yardstick_interpolation(c)
    worst = {0: 0.0, 1: 0.0}
    for (label, target, branch, pt, speed), m, yard in zip(om.interpolation_runs(c), om.interpolation_model(c), yards):
        camera, tetrad, velocity = got = interpolate_launch(p, cfg, c, target, pt, speed)
        what = (name, label, pt, speed.tolist())
        if m["branch"][2] == "empty":
            assert untouched(camera) and untouched(tetrad) and untouched(velocity), what
            continue
        copied, legs_copied = om.is_copy(m, pt)
        i = m["branch"][0]
        if copied:
            assert camera.tobytes() == c["path32"][i].tobytes() and velocity.tobytes() == c["vel32"][i].tobytes(), what
        if legs_copied:
            assert tetrad.tobytes() == c["legs32"][:, i].tobytes(), what
        if m["branch"][1] == 0:      # dx = 0: a + (b - a) * 0 is a, in any precision and order
            assert (camera == c["path32"][i]).all() and (velocity == c["vel32"][i]).all(), what
            if pt:
                assert (tetrad == c["legs32"][:, i]).all(), what
        err = om.interpolation_errors(m, got)
        om.assert_by_the_rule(what, om.interpolation_floors(pt), err, om.interpolation_errors(m, yard))
        worst[pt] = max(worst[pt], float(err.max() if pt else err[:2].max()))
        if not pt:
            worst["legs"] = max(worst.get("legs", 0.0), float(err[2:].max()))
    print(f"{name}: gpu: mix {max(worst[0], worst[1]):.2e}, recomputed legs {worst.get('legs', 0.0):.2e} (yardstick: {kind})")


# ---- gr_get_geodesic_path ----------------------------------------------------------------------------------------------------------
UNIVERSE = 20.0
FEATURES = om.features_bytes(universe_size=UNIVERSE)
PATH_PROGRAMS = ("schwarzschild", "kerr_boyer", "minkowski")
_rays = {}


def hand_made_rays(program, polar, speeds):
    """timelike rays of gr_init_inertial_ray: observers at polar (t, r, theta, phi) [n][4] moving at `speeds` [n][3] in the tetrad at rest"""
    prog = sm.program(program)
    p, cfg = device_program(program)
    generic32 = np.stack([prog.from_polar(x) for x in np.asarray(polar, dtype=np.float64)]).astype(np.float32)
    legs32 = np.stack([sm.tetrad(prog, x.astype(np.float64)) for x in generic32]).astype(np.float32)
    rays = init_inertial_ray(p, cfg, generic32, legs32, np.asarray(speeds, dtype=np.float32))
    assert np.isfinite(rays["position"]).all() and np.isfinite(rays["velocity"]).all() and np.isfinite(rays["acceleration"]).all()
    return generic32, rays


def seventy_rays(program):
    """70 observers, radius and speed spread so that neighbours take different numbers of steps within 40: slow ones near the
    middle run the whole length, fast ones near the edge of the universe leave it after a handful of steps, two start outside"""
    if program not in _rays:
        rng = np.random.default_rng(om.SEED + 7)
        n = om.MAX_OBSERVERS
        r = np.where(np.arange(n) % 2 == 0, rng.uniform(7.0, 9.5, n), rng.uniform(14.0, 19.9, n))
        r[[5, 64]] = (UNIVERSE + 0.5, UNIVERSE + 3.0)
        polar = np.stack([rng.uniform(-5, 5, n), r, np.radians(rng.uniform(50, 130, n)), rng.uniform(-2.5, 2.5, n)], axis=1)
        outward = np.where(np.arange(n) % 2 == 0, rng.uniform(0.0, 0.3, n), rng.uniform(0.3, 0.9, n))
        # (the tetrad's second leg points along -r at these poses or not, whichever: half of the fast ones run inwards)
        speeds = np.stack([np.zeros(n), outward * np.where(np.arange(n) % 4 < 2, 1.0, -1.0), np.zeros(n)], axis=1)
        _rays[program] = hand_made_rays(program, polar, speeds)
    return _rays[program]


def geodesic_path(program, rays, max_length, records=None, velocities=True, steps=True):
    """one launch over len(rays) rays -> dict(count [n], path [records][n][4], velocity, ds [records][n]); fill bytes where nothing was written"""
    p, cfg = device_program(program)
    n = len(rays)
    records = max_length if records is None else records
    assert records >= max_length
    pos, vel, ds, count = Guarded(records * n, 16), Guarded(records * n, 16), Guarded(records * n, 4), Guarded(n, 4)
    d_rays, d_n, d_features = up(rays), up(np.array([n], dtype=np.int32)), up(np.frombuffer(FEATURES, dtype=np.uint8))
    check(lib.gr_get_geodesic_path(p.handle, None, d_rays.ptr, n, pos.ptr, vel.ptr if velocities else None, ds.ptr if steps else None, d_n.ptr,
                                   max_length, cfg.ptr, d_features.ptr, count.ptr))
    check(lib.gr_device_synchronize(0))
    return dict(count=count.read(np.int32, (n,)), path=pos.read(np.float32, (records, n, 4)), velocity=vel.read(np.float32, (records, n, 4)),
                ds=ds.read(np.float32, (records, n)))


@pytest.mark.parametrize("program", PATH_PROGRAMS)
def test_a_path_stops_at_its_maximum_length(program):
    """a ray that would run longer, max_path_length of 1, 2 and 7: that many records, nothing behind them, and the records of the
    shorter run are the first of the longer"""
    _, rays = seventy_rays(program)
    ray = rays[0:1]
    longest = None
    for length in (7, 2, 1):
        r = geodesic_path(program, ray, length, records=10)
        assert r["count"].tolist() == [length]
        for k in ("path", "velocity", "ds"):
            assert untouched(r[k][length:]) and np.isfinite(r[k][:length]).all(), (k, length)
            if longest is not None:
                assert r[k][:length].tobytes() == longest[k][:length].tobytes(), (k, length)
        longest = r if longest is None else longest


@pytest.mark.parametrize("program", PATH_PROGRAMS)
def test_a_ray_outside_the_universe_stores_its_start(program):
    generic32, rays = seventy_rays(program)
    prog = sm.program(program)
    for lane in (5, 64):
        r = geodesic_path(program, rays[lane:lane + 1], 12)
        assert r["count"].tolist() == [1]
        for k in ("path", "velocity", "ds"):
            assert untouched(r[k][1:]), k
        if prog.generic_constant_theta:      # the record is turned back out of the equatorial plane the ray was turned into
            assert om.vec_err(r["path"][0, 0], generic32[lane].astype(np.float64)) <= sm.RAY_FLOOR
        else:
            assert r["path"][0, 0].tobytes() == generic32[lane].tobytes() == rays["position"][lane].tobytes()
            assert r["velocity"][0, 0].tobytes() == rays["velocity"][lane].tobytes()


@pytest.mark.parametrize("program", PATH_PROGRAMS)
def test_optional_outputs_may_be_null(program):
    _, rays = seventy_rays(program)
    some = np.ascontiguousarray(rays[[0, 1, 5, 6]])
    both = geodesic_path(program, some, 12)
    for missing in ("velocity", "ds"):
        r = geodesic_path(program, some, 12, velocities=missing != "velocity", steps=missing != "ds")
        assert untouched(r[missing])
        for k in ("count", "path", "velocity", "ds"):
            if k != missing:
                assert r[k].tobytes() == both[k].tobytes(), (missing, k)


@pytest.mark.parametrize("program", PATH_PROGRAMS)
def test_seventy_rays_share_one_path_launch(program):
    """70 different rays in one launch: each lane's count and records are those of its own launch alone, bit for bit; records past a
    lane's count keep their fill bytes; neighbouring lanes take different numbers of steps"""
    _, rays = seventy_rays(program)
    m = om.MAX_SAMPLES
    whole = geodesic_path(program, rays, m)
    counts = whole["count"]
    print(f"{program}: counts {counts.tolist()}")
    assert counts[5] == counts[64] == 1 and counts.max() == m and ((counts > 1) & (counts < 10)).any()
    assert (np.diff(counts) != 0).mean() >= 0.5 and counts[63] != counts[64]
    for lane in range(len(rays)):
        n = int(counts[lane])
        alone = geodesic_path(program, rays[lane:lane + 1], m)
        assert alone["count"].tolist() == [n], lane
        for k in ("path", "velocity", "ds"):
            assert untouched(whole[k][n:, lane]), (k, lane)
            assert alone[k][:, 0].tobytes() == whole[k][:, lane].tobytes(), (k, lane)


FIXED_STEP_PROGRAMS = ("schwarzschild", "minkowski")      # of PATH_PROGRAMS: no step-size controller


@pytest.mark.parametrize("program", FIXED_STEP_PROGRAMS)
def test_the_first_eight_records_against_float64(program):
    """eight fixed-size steps from r >= 6 rs amplify nothing: positions, velocities and step lengths against the float64 evaluation of
    the same discrete algorithm (oracle ref_get_geodesic_path_f64), by the rule with setup_model.RAY_FLOOR"""
    assert program in PATH_PROGRAMS and "-DADAPTIVE_PRECISION" not in sm.program(program).argument_string.split()
    _, rays = seventy_rays(program)
    cfg = sm.program(program).cfg
    pipe, kind = om.yardstick_pipeline(program)
    restatement, _ = om.restatement_pipeline(program)
    for lane in (0, 2, 62, 66):      # r from 7 to 9.5, |v| <= 0.3: none of them ends within eight steps
        ray = rays[lane:lane + 1]
        got = geodesic_path(program, ray, 8)
        assert got["count"].tolist() == [8]
        p64, v64, ds64 = restatement.geodesic_path_f64(ray, cfg, FEATURES, 8)
        yp, yv, yds = pipe.geodesic_path(ray, cfg, FEATURES, 8)
        assert len(p64) == len(yp) == 8 and float(np.sqrt((p64[:, 1:] ** 2).sum(axis=1)).min() if program == "minkowski" else p64[:, 1].min()) >= 6
        err = np.stack([om.vec_err(got["path"][:, 0], p64), om.vec_err(got["velocity"][:, 0], v64), np.abs(got["ds"][:, 0] - ds64) / np.maximum(1.0, np.abs(ds64))])
        yard_err = np.stack([om.vec_err(yp, p64), om.vec_err(yv, v64), np.abs(yds - ds64) / np.maximum(1.0, np.abs(ds64))])
        om.assert_by_the_rule((program, lane), sm.RAY_FLOOR, err, yard_err)
        print(f"{program} lane {lane}: gpu {err.max():.2e} yardstick ({kind}) {yard_err.max():.2e} floor {sm.RAY_FLOOR:.0e}")
