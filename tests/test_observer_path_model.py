"""CPU tests of the observer-path stage's float64 model and its hand-made paths (tests/observer_path_model.py): the derivatives the
model reads agree with central differences of g at every sample of every case; the case list is deterministic and every
interpolation case takes the branch it records; and both fp32 yardsticks - the CPU restatement oracle/restate.cpp and, where it is
built, the reference's own object - meet the conditions the device's bounds rest on: within the floor on every value of every
ordinary case, nothing set aside as not finite there, copies bit for bit.  Only the named set-aside case may exceed the floor.

Run as a script (PYTHONPATH=. python tests/test_observer_path_model.py) this prints the CPU part of
profiles/observer_path_synthetic.txt, the measurement of TRANSPORT_FLOOR among it."""
import math

import numpy as np
import pytest

import observer_path_model as om
import setup_model as sm

PIPELINES = (om.restatement_pipeline, om.yardstick_pipeline)


def measured_floor(measured):
    """twice the measured error, rounded up to one significant digit"""
    doubled = 2 * measured
    unit = 10.0 ** math.floor(math.log10(doubled))
    return math.ceil(doubled / unit - 1e-9) * unit


def test_the_case_list_is_deterministic_and_the_one_named():
    assert [c["name"] for c in om.transport_cases()] == om.TRANSPORT_CASE_NAMES
    assert [c["name"] for c in om.interpolation_cases()] == om.INTERPOLATION_CASE_NAMES
    first = om.case_bytes()
    om._cases.clear()
    assert om.case_bytes() == first
    for c in om.transport_cases():
        assert 0 < c["count"] <= om.MAX_SAMPLES and c["kind"] in ("ordinary", "set_aside") and c["quantities32"].shape == (5, 4)
    assert [c["name"] for c in om.transport_cases() if c["kind"] == "set_aside"] == ["set_aside_horizon_kerr_boyer"]
    assert {c["program"] for c in om.transport_cases()} >= set(om.TRANSPORT_PROGRAMS)
    for program in om.TRANSPORT_PROGRAMS:
        mine = [c for c in om.transport_cases() if c["program"] == program and c["kind"] == "ordinary"]
        assert sorted(c["count"] for c in mine) == [2, 3, 8, 40]
    assert all(any(c["name"].endswith(k) for c in om.transport_cases()) for k in om.STEP_KINDS)
    o = om.observers_case()
    counts = o["counts"]
    assert len(counts) == om.MAX_OBSERVERS == 70 and o["path32"].shape == (om.MAX_SAMPLES, 70, 4)
    assert set(counts.tolist()) == {0, 1, 2, 3, 17, 40} and counts[62:66].tolist() == [40, 0, 40, 1]
    assert len(np.unique(o["path32"][0], axis=0)) == 70
    for c in om.interpolation_cases():
        assert c["count"] <= len(c["path32"]) <= om.MAX_SAMPLES
    assert sorted({c["count"] for c in om.interpolation_cases()}) == [0, 1, 2, 4, 9]


def _samples(c):
    if "counts" in c:
        return c["path32"].reshape(-1, 4)
    return c["path32"]


@pytest.mark.parametrize("name", om.TRANSPORT_CASE_NAMES + om.INTERPOLATION_CASE_NAMES + ["observers_70_kerr_boyer"])
def test_the_generated_derivatives_against_central_differences(name):
    """at every sample of every case, relative to max(1, the largest derivative there): observer_path_model.central_derivatives has the
    error argument.  So the model inherits no error of the generated derivative expressions."""
    c = next(c for c in om.transport_cases() + om.interpolation_cases() + [om.observers_case()] if c["name"] == name)
    prog = sm.program(c["program"])
    worst = 0.0
    for x in _samples(c).astype(np.float64):
        generated, central = om.metric_derivatives(prog, x), om.central_derivatives(prog, x)
        worst = max(worst, float(np.abs(generated - central).max() / max(1.0, np.abs(generated).max())))
    print(f"{name}: derivatives against central differences {worst:.1e}")
    assert worst <= om.DERIVATIVE_BOUND, (name, worst)


def test_flat_space_transports_nothing():
    """Minkowski in Cartesian coordinates: d g = 0, every record of the model is the input, exactly"""
    for c in om.transport_cases():
        if c["program"] == "minkowski":
            m = om.transport_model(c)
            assert (m == c["quantities32"].astype(np.float64)[:, None, :]).all(), c["name"]


def measure_transport():
    """(the yardstick's largest error over the ordinary transport cases of 8 samples or fewer, the case and yardstick it is on)"""
    measured, which = 0.0, None
    for c in om.transport_cases():
        if c["kind"] == "ordinary" and c["count"] <= 8:
            _, err, kind = om.yardstick_transport(c, om.yardstick_pipeline)
            if float(np.nanmax(err)) > measured:
                measured, which = float(np.nanmax(err)), f"{c['name']} ({kind})"
    return measured, which


def test_the_transport_floor_is_twice_the_measurement():
    measured, which = measure_transport()
    assert f"{measured:.2e}" == f"{om.TRANSPORT_MEASURED:.2e}", (measured, which)
    assert om.TRANSPORT_MEASURED > 0 and om.TRANSPORT_FLOOR == measured_floor(om.TRANSPORT_MEASURED)
    assert om.transport_floor(2) == om.transport_floor(8) == om.TRANSPORT_FLOOR and om.transport_floor(40) == 5 * om.TRANSPORT_FLOOR


def transport_figures(c, pipeline):
    got, err, kind = om.yardstick_transport(c, pipeline)
    floor = om.transport_floor(c["count"])
    return got, err, kind, floor


@pytest.mark.parametrize("name", om.TRANSPORT_CASE_NAMES)
def test_the_yardsticks_meet_the_conditions_on_transport_cases(name):
    c = om.transport_case(name)
    for pipeline in PIPELINES:
        got, err, kind, floor = transport_figures(c, pipeline)
        aside = float(np.isnan(err).mean())
        over = int((err[~np.isnan(err)] > floor).sum())
        print(f"{name}: {kind}: {np.nanmax(err):.2e} (floor {floor:.0e}), {over} of {err.size} values over it, set aside {100 * aside:.1f} %")
        assert got[:, 0].tobytes() == c["quantities32"].tobytes(), "the record at step 0 is the input"
        if c["kind"] == "ordinary":
            assert over == 0 and aside == 0, (name, kind, float(np.nanmax(err)))
        else:      # set aside: the other yardstick meets the bounds the device is held to
            assert aside <= 0.05, (name, kind, aside)
            other = om.yardstick_transport(c, PIPELINES[1 - PIPELINES.index(pipeline)])[1]
            print(f"{name}: {kind}: values beyond the floor (mine, the other yardstick's): {om.assert_set_aside(name, floor, err, other)}")
        if c["program"] == "minkowski":
            assert (got == c["quantities32"][:, None, :]).all()


def test_the_yardsticks_meet_the_conditions_on_the_launch_of_seventy():
    """every lane alone (the CPU yardsticks run one observer at a time): within the floor of its own count"""
    c = om.observers_case()
    cfg = sm.program(c["program"]).cfg
    for pipeline in PIPELINES:
        pipe, kind = pipeline(c["program"])
        for lane in range(len(c["counts"])):
            n = int(c["counts"][lane])
            got = pipe.parallel_transport(c["path32"][:, lane], c["vel32"][:, lane], c["ds32"][:, lane], c["quantity32"][lane], n, cfg, fill=om.FILL)
            assert (got[n:] == om.FILL).all(), (lane, "records from count on are not written")
            if n:
                err = om.vec_err(got[:n], om.observers_model(c, lane))
                assert err.max() <= om.transport_floor(n), (kind, lane, float(err.max()))
                assert got[0].tobytes() == c["quantity32"][lane].tobytes()


@pytest.mark.parametrize("name", om.INTERPOLATION_CASE_NAMES)
def test_interpolation_cases_take_the_branch_they_record(name):
    c = om.interpolation_case(name)
    for (label, target, branch, pt, speed), m in zip(om.interpolation_runs(c), om.interpolation_model(c)):
        segment, dx, which = m["branch"]
        assert (segment, which) == (branch[0], branch[2]), (name, label, m["branch"], branch)
        if name.endswith("inexact"):
            assert abs(dx - branch[1]) <= 1e-5 and 5e-5 <= dx <= 1 - 5e-5, (name, label, dx)
        else:
            assert dx == branch[1], (name, label, dx, branch[1])


def test_the_interpolation_cases_cover_every_exit():
    seen = {}
    for c in om.interpolation_cases():
        for (label, target, branch, pt, speed), m in zip(om.interpolation_runs(c), om.interpolation_model(c)):
            seen.setdefault((c["program"], pt), set()).add(m["branch"][2])
            if pt == 0 and float(np.linalg.norm(speed)) > 0.89:
                seen.setdefault((c["program"], "fast"), set()).add(0 < m["branch"][1] < 1)
    for program in om.INTERPOLATION_PROGRAMS:
        for pt in (0, 1):
            assert seen[(program, pt)] == {"empty", "single", "before", "inside", "last"}, (program, pt)
        assert seen[(program, "fast")] == {True}      # |v| = 0.9 at positions strictly between two samples
    nine = om.interpolation_case("kerr_boyer_nine")
    dxs = {m["branch"][1] for m in om.interpolation_model(nine) if m["branch"][2] == "inside"}
    assert dxs >= {0.0, 2.0 ** -20, 0.5, 1 - 2.0 ** -20}
    targets = [t for _, t, _ in nine["targets"]]
    assert any(np.isnan(t) for t in targets) and np.inf in targets and min(targets) < 0 and om.EXACT_TOTAL in targets
    sums = np.concatenate([[0.0], np.cumsum(np.array(om.EXACT_DS[:-1]))])
    assert sums[-1] == om.EXACT_TOTAL and (np.cumsum(np.array(om.EXACT_DS[:-1], dtype=np.float32)).astype(np.float64) == sums[1:]).all()


def interpolation_figures(c, pipeline):
    """per run: (errors [6], floors [6], copies) of the yardstick, after the exact comparisons"""
    got, kind = om.yardstick_interpolation(c, pipeline)
    out = []
    for run, m, g in zip(om.interpolation_runs(c), om.interpolation_model(c), got):
        label, target, branch, pt, speed = run
        camera, tetrad, velocity = g
        if m["branch"][2] == "empty":
            assert (camera == om.FILL).all() and (tetrad == om.FILL).all() and (velocity == om.FILL).all(), (c["name"], "count 0 writes nothing")
            continue
        copied, legs_copied = om.is_copy(m, pt)
        if copied:
            i = m["branch"][0]
            assert camera.tobytes() == c["path32"][i].tobytes() and velocity.tobytes() == c["vel32"][i].tobytes(), (c["name"], label)
        if legs_copied:
            assert tetrad.tobytes() == c["legs32"][:, m["branch"][0]].tobytes(), (c["name"], label)
        out.append((run, om.interpolation_errors(m, g), om.interpolation_floors(pt)))
    return out, kind


@pytest.mark.parametrize("name", om.INTERPOLATION_CASE_NAMES)
def test_the_yardsticks_meet_the_conditions_on_interpolation_cases(name):
    c = om.interpolation_case(name)
    for pipeline in PIPELINES:
        figures, kind = interpolation_figures(c, pipeline)
        for (label, target, branch, pt, speed), err, floors in figures:
            assert not np.isnan(err).any() and (err <= floors).all(), (name, kind, label, pt, speed.tolist(), err.tolist())
        if figures:
            mix = max(float(e[:2].max()) if not pt else float(e.max()) for (_, _, _, pt, _), e, _ in figures)
            legs = max([float(e[2:].max()) for (_, _, _, pt, _), e, _ in figures if not pt] or [0.0])
            print(f"{name}: {kind}: mix {mix:.2e} (floor {om.INTERPOLATION_FLOOR:.0e}), recomputed legs {legs:.2e} (floor {sm.CAMERA_FLOOR:.0e})")


def report():
    print("# the observer-path stage on paths made by hand: the largest vec_err against the float64 model per case")
    print("# (tests/observer_path_model.py).  CPU columns: PYTHONPATH=. python tests/test_observer_path_model.py; the device's figures (MI355X)")
    print("# are the lines pytest -m gpu -s tests/test_gpu_observer_path.py prints.")
    print("# transport case                                samples  restatement  reference object     floor")
    for c in om.transport_cases():
        rest = om.yardstick_transport(c, om.restatement_pipeline)[1]
        _, yard, kind = om.yardstick_transport(c, om.yardstick_pipeline)
        ref = f"{np.nanmax(yard):.2e}" if kind == "reference object" else "       -"
        print(f"  {c['name']:46s} {c['count']:7d}     {np.nanmax(rest):.2e}          {ref}   {om.transport_floor(c['count']):.1e}")
    measured, which = measure_transport()
    print(f"# TRANSPORT_MEASURED: the yardstick's largest over the ordinary cases of 8 samples or fewer: {measured:.2e}, on {which}")
    print(f"# TRANSPORT_FLOOR: twice that, rounded up to one significant digit: {measured_floor(measured):.0e}; times count / 8 on longer paths")
    print("# interpolation case                      mix: restatement  reference object   recomputed legs: restatement  reference object")
    for c in om.interpolation_cases():
        cols = []
        for pipeline in PIPELINES:
            figures, kind = interpolation_figures(c, pipeline)
            mix = max([float(e[:2].max()) if not pt else float(e.max()) for (_, _, _, pt, _), e, _ in figures] or [0.0])
            legs = max([float(e[2:].max()) for (_, _, _, pt, _), e, _ in figures if not pt] or [0.0])
            cols.append((f"{mix:.2e}", f"{legs:.2e}") if pipeline is om.restatement_pipeline or kind == "reference object" else ("       -", "       -"))
        print(f"  {c['name']:40s}      {cols[0][0]}          {cols[1][0]}                     {cols[0][1]}          {cols[1][1]}")


if __name__ == "__main__":
    report()
