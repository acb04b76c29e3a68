"""CPU tests of the render-data stage's float64 model and its hand-made rays (tests/render_data_model.py): every case is well-posed
(few records within rounding of a branch) and reaches what its description names; the closed forms of three metrics agree with the
host evaluator the model reads; the CPU oracles - the restatement oracle/restate.cpp and, where it is built, the reference's own
object - compute the cases to within their fp32 error of the model; the shortcut of the redshift's timelike leg returns the value
of the full tetrad at -1e-3 < g_tt < -1e-5.

`PYTHONPATH=. python tests/test_render_data_model.py` prints the table of the oracles' errors kept in
profiles/render_data_synthetic.txt (its device column comes from tests/test_gpu_render_data.py's printed lines)."""
import numpy as np
import pytest

import geodesic_raytracing_amd as gra
import render_data_model as rm
from oracle import build_ref, build_restate
from oracle.refpipe import OraclePipeline

_pipes, _records = {}, {}


def restatement(program_name):
    key = ("restate", program_name)
    if key not in _pipes:
        _pipes[key] = OraclePipeline(build_restate.build(rm.program(program_name).argument_string))
    return _pipes[key]


def reference_object(program_name):
    """the reference's own calculate_render_data for a program, where oracle/_ref holds it (None otherwise)"""
    key = ("ref", program_name)
    if key not in _pipes:
        tag = rm.REFERENCE_TAGS.get(program_name)
        so = build_ref.prebuilt(tag, rm.program(program_name).argument_string) if tag else None
        _pipes[key] = OraclePipeline(so) if so else None
    return _pipes[key]


def oracle_records(kind, c):
    """a CPU oracle's records of a case in ray order, once per case and not written to (None: no such oracle here)"""
    key = (kind, c["name"])
    if key not in _records:
        pipe = restatement(c["program"]) if kind == "restatement" else reference_object(c["program"])
        got = None
        if pipe is not None:
            prog = rm.program(c["program"])
            got = rm.by_record(c, pipe.render_data(c["rays"], c["width"], c["height"], prog.cfg, rm.features_bytes(c)))
            got.setflags(write=False)
        _records[key] = got
    return _records[key]


def restatement_figures(c):
    """(tex, z) error of the restatement against the model on a case: what the device's bound is taken from"""
    return rm.errors(c, oracle_records("restatement", c))


def test_the_case_list_is_the_one_named():
    assert [c["name"] for c in rm.cases()] == rm.CASE_NAMES


@pytest.mark.parametrize("name", rm.CASE_NAMES)
def test_cases_are_well_posed_and_reach_what_they_name(name):
    c = rm.case(name)
    rays, prog = c["rays"], rm.program(c["program"])
    n = len(rays)
    assert c["width"] <= 67 and c["height"] <= 40 and n == c["width"] * c["height"] and c["reaches"]
    assert sorted(rays["sy"].astype(np.int64) * c["width"] + rays["sx"]) == list(range(n))          # a permutation of the frame
    assert np.abs(np.linalg.norm(rays["initial_quat"], axis=1) - 1).max() < 1e-6 and len(np.unique(rays["initial_quat"], axis=0)) == n
    e, safe = rm.model_of(c)
    assert (~safe).mean() <= 0.05, (name, float((~safe).mean()), {k: int(v.sum()) for k, v in e["unsafe_why"].items()})
    live, sel = e["live"], rm.compared(c)
    ratio = np.abs(e["r"]) / np.float32(c["universe"])
    if name.startswith("universe_overshoot"):
        ran = e["fix"] == rm.FIX_UNIVERSE
        assert ran.mean() > 0.7 and ratio[ran].min() <= 1 + 3e-6 and ratio[ran].max() >= 0.99e4
        assert ((e["discrim"] < 0) & ran & sel).sum() >= 10                                       # the early return of the quadratic
        near_first, far_first = np.abs(e["t0"]) < np.abs(e["t1"]), np.abs(e["t0"]) > np.abs(e["t1"])
        assert (near_first & sel).sum() >= 30 and (far_first & sel).sum() >= 30                   # both orders of the roots
        assert (sel & ran & (ratio > 5)).any()                                                    # a large overshoot that is compared
        if name.endswith("wormhole"):
            assert set(e["side"][sel & ran]) == {0, 1} and (e["r"][sel] < -20).any() and (e["r"][sel] > 20).any()
        if name.endswith("schwarzschild") or name.endswith("wormhole"):
            assert prog.constant_theta and (sel & ~ran).any() == name.endswith("schwarzschild")
        if name.endswith("kerr_schild") or name.endswith("cosmic_string"):
            assert not np.allclose(prog.to_polar([0.0, 3.0, 1.0, 2.0]), [0.0, 3.0, 1.0, 2.0])     # the chart is not the polar one
    if name == "inside_terminator":
        assert prog.singular and prog.traversable and prog.terminator == 1.0
        assert (e["fix"][live] == rm.FIX_TERMINATOR).all() and e["r"].min() <= 1.01e-3 and e["r"].max() > 0.9999
        assert (rays["velocity"][:, 1] < 0).sum() > 100 and (rays["velocity"][:, 1] > 0).sum() > 100
        assert np.abs(e["r_fixed"][sel] - 1).max() < 1e-9 and (e["path"][sel] == rm.PATH_FULL).sum() > 300   # lands on the terminator
    if name == "inside_terminator_schwarzschild":
        assert not prog.traversable and (e["early"][live] == 1).all() and (e["tex"] == 0).all() and (e["z"] == 0).all()
        assert (rays["position"] == rm.case("inside_terminator")["rays"]["position"]).all()
    if name == "theta_wrap":
        th, ph = rays["position"][:, 2], rays["position"][:, 3]
        assert th.min() < -2.9 * np.pi and th.max() > 2.9 * np.pi and ph.min() < -4.9 * np.pi and ph.max() > 4.9 * np.pi
        assert (th == np.float32(np.pi)).any() and ((th == 0) & ~np.signbit(th)).any() and ((th == 0) & np.signbit(th)).any()
        assert (e["wrapped"][sel] == 1).sum() > 60 and (e["wrapped"][sel] == 0).sum() > 60
        assert (sel & (th < 0)).sum() > 100 and (sel & (np.abs(ph) > 2 * np.pi)).sum() > 100
    if name.startswith("axis"):
        s = np.abs(np.sin(e["theta"]))
        assert s.min() <= 1.1e-7 and (sel & (s < 1e-5)).sum() >= 10 and (sel & (e["theta"] > 3)).any() and (sel & (e["theta"] < 0.1)).any()
        if name == "axis_kerr_schild":
            x, y, z = rays["position"][:, 1], rays["position"][:, 2], rays["position"][:, 3]
            on, beside = (x == 0) & (y == 0), (np.hypot(x, y) > 0) & (np.hypot(x, y) < 1.5e-6)
            assert on.sum() >= 8 and beside.sum() >= 8 and (z[on] > 0).any() and (z[on] < 0).any() and (e["fix"] == rm.FIX_NONE).all()
    if name == "ergosphere":
        assert prog.traversable and prog.singular
        short, full = sel & (e["path"] == rm.PATH_SHORTCUT), sel & (e["path"] == rm.PATH_FULL)
        assert (short & (e["g_tt"] > -1e-3) & (e["g_tt"] < -1e-5)).sum() >= 150 and (short & (e["g_tt"] > -2e-5)).any()
        assert (full & (e["g_tt"] > 0)).sum() >= 100 and ((e["path"] == rm.PATH_FULL) & (e["g_tt"] < 0)).any()
    if name == "degenerate":
        bad_position, bad_velocity = ~np.isfinite(rays["position"]).all(axis=1), ~np.isfinite(rays["velocity"]).all(axis=1)
        assert np.isnan(rays["position"]).any() and (rays["position"] == np.inf).any() and (rays["position"] == -np.inf).any()
        assert bad_velocity.sum() >= 5 and (e["path"][bad_position] == rm.PATH_DEGENERATE).all() and (rays["terminated"] == 1).all()
        assert all(~np.isfinite(rays["position"][:, k]).all() or ~np.isfinite(rays["position"][:, k]).any() for k in range(4))
        assert (sel & bad_position).any()                               # a degenerate time component leaves a defined record
    if name == "clamp_and_running":
        raw = e["z_raw"]
        assert (raw[sel] < -0.9991).sum() >= 50 and (e["z"][raw < -0.999] == -0.999).all() and raw.max() > 0.99e4
        for z in rm.REDSHIFT_Z:
            if z != -0.999:
                assert (np.abs(raw[sel] - z) <= 1e-3 * (1 + abs(z))).any(), z
        assert set(rays["running_dlambda_dnew"]) == {np.float32(1), np.float32(0.25), np.float32(7.5)}
        assert (rays["ku_uobsu"][sel] < 0).sum() > 100 and (rays["ku_uobsu"][sel] > 0).sum() > 100
    if name == "flags":
        assert (rays["terminated"] == np.arange(n) % 3).all()
        dead = ~live
        assert (e["tex"][dead] == 0).all() and (e["z"][dead] == 0).all() and (e["side"][dead] == 1).all()


def test_the_shortcut_returns_the_full_tetrads_value_just_below_its_threshold():
    """kernels/trace.hip: "e0 = d/dt / sqrt|g_tt|, the value the full construction returns" - held in float64 on the ergosphere
    case's records with -1e-3 < g_tt < -1e-5, and on every other compared record that takes the shortcut"""
    held = 0
    for c in rm.cases():
        e, _ = rm.model_of(c)
        sel = rm.compared(c) & (e["path"] == rm.PATH_SHORTCUT)
        d = np.abs(e["z_shortcut"][sel] - e["z_full"][sel]) / (1 + np.abs(e["z_full"][sel]))
        assert not sel.any() or d.max() <= 1e-9, (c["name"], float(d.max()))
        if c["name"] == "ergosphere":
            held = int((sel & (e["g_tt"] > -1e-3) & (e["g_tt"] < -1e-5)).sum())
    assert held >= 150


@pytest.mark.parametrize("name", ["minkowski", "schwarzschild", "kerr_boyer"])
def test_closed_forms_agree_with_the_host_evaluator(name):
    metric = gra.Metric(name, rm.SCRIPTS)
    cfg = metric.cfg_values(a=0.45) if name == "kerr_boyer" else metric.cfg_values()
    rng = np.random.default_rng(5)
    for _ in range(200):
        x = np.array([rng.uniform(-5, 5), rng.uniform(1.2, 30), rng.uniform(0.05, 3.1), rng.uniform(-3.1, 3.1)])
        if name == "minkowski":
            x[1:] = rng.uniform(-20, 20, 3)
        g, polar = rm.closed_form(name, x, [float(np.float32(v)) for v in cfg])
        got_g = metric.evaluate(gra.EVAL_METRIC_TENSOR, x, cfg_values=cfg or None).reshape(4, 4)
        got_polar = metric.evaluate(gra.EVAL_TO_POLAR, x, cfg_values=cfg or None)
        assert np.abs(got_g - g).max() <= 1e-12 * max(1.0, np.abs(g).max()), (name, x)
        assert np.abs(got_polar - polar).max() <= 1e-12 * max(1.0, np.abs(polar).max()), (name, x)


@pytest.mark.parametrize("name", rm.CASE_NAMES)
def test_the_restatement_computes_the_cases_as_the_model_does(name):
    """the reference's own fp32 error on these inputs, which the device's bound is taken from: below 1e-3 on both figures, or the
    case is ill-conditioned as an input.  Flags are exact on every record."""
    c = rm.case(name)
    got = oracle_records("restatement", c)
    rm.assert_flags(c, got)
    tex, z = rm.errors(c, got)
    print(f"{name}: restatement tex {tex:.2e} z {z:.2e}")
    assert tex < 1e-3 and z < 1e-3, (name, tex, z)


@pytest.mark.parametrize("name", [n for n in rm.CASE_NAMES if rm.case(n)["program"] in rm.REFERENCE_TAGS])
def test_the_reference_object_computes_the_cases_as_the_model_does(name):
    c = rm.case(name)
    if reference_object(c["program"]) is None:
        pytest.skip("the reference's object is only built where its sources are")
    got = oracle_records("reference", c)
    # (flags only: the object is built with unsafe-math optimisations, and its fmax hands a NaN through where the full tetrad is not
    # finite - the two theta = 0 records of theta_wrap)
    rm.assert_flags(c, got, range_of_the_rest=False)
    tex, z = rm.errors(c, got)
    print(f"{name}: reference object tex {tex:.2e} z {z:.2e}")
    assert tex < 1e-3 and z < 1e-3, (name, tex, z)


def cpu_figures():
    """per case: (name, unsafe share, restatement tex, z, reference object tex, z or None)"""
    rows = []
    for c in rm.cases():
        ref = (None, None)
        if c["program"] in rm.REFERENCE_TAGS and reference_object(c["program"]) is not None:
            ref = rm.errors(c, oracle_records("reference", c))
        rows.append((c["name"], float((~rm.model_of(c)[1]).mean())) + restatement_figures(c) + tuple(ref))
    return rows


if __name__ == "__main__":
    print("# oracle errors against the float64 model on the compared records of every case (tests/render_data_model.py):")
    print("# max circ_diff(tex_coord) * max(sin theta, 1e-3), max |dz| / (1 + |z|); unsafe: share of records set aside")
    print(f"# {'case':34s} {'unsafe':>6s} {'restatement':>19s} {'reference object':>19s}")
    for name, unsafe, tex, z, rtex, rz in cpu_figures():
        ref = f"{rtex:9.2e} {rz:9.2e}" if rtex is not None else f"{'-':>9s} {'-':>9s}"
        print(f"  {name:34s} {unsafe:6.3f} {tex:9.2e} {z:9.2e} {ref}")
