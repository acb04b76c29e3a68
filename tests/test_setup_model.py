"""CPU tests of the set-up stage's float64 model and its hand-made cameras (tests/setup_model.py): the model reproduces every
committed fixture's camera, tetrad and initial rays within the stage's floors; the evaluator it reads agrees with closed forms at
the new poses; its own tetrads are orthonormal and its rays null to 1e-12; the case list is deterministic and every case takes the
branch it names; and the fp32 yardstick - the CPU restatement oracle/restate.cpp or, where it is built, the reference's own object -
meets the conditions the device's bounds rest on: within the floor on every ordinary case, on an edge case at most half of the
compared values beyond it and at most 5 % set aside as not finite.  The shares are printed per case (pytest -s).

The yardstick's figures are shared with tests/test_gpu_setup.py, which takes the device's bounds from them."""
import numpy as np
import pytest

import geodesic_raytracing_amd as gra
import gpu_stages as gs
import render_data_model as rm
import setup_model as sm

# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def _program_of(meta):
    return sm.ProgramOf(name=meta["metric"], metric=gs.metric_for(meta), cfg=meta["cfg"])


@pytest.mark.parametrize("name", gs.golden_names())
def test_the_model_reproduces_the_fixtures(name):
    """camera_generic and tetrad abs 2e-6, rays_init abs 2e-5 (tests/test_gpu_parity.py's floors and measure) - the rays on every
    seventh pixel and the four corners.  (pixel_ray's flip is 0 whatever the fixture's: that argument of gr_init_rays_generic is
    what the frame driver passes, and it passes 0 always - the fixture's `flip` puts the camera at r < 0, in gr_cart_to_generic.)"""
    meta, z = gs.load_golden(name)
    prog = _program_of(meta)
    cam = sm.camera_generic(prog, np.array(meta["camera_pos"], dtype=np.float32), meta.get("flip", 0.0))
    tet = sm.tetrad(prog, z["camera_generic"], np.array(meta["basis_speed"], dtype=np.float32))
    assert np.abs(cam - z["camera_generic"]).max() <= sm.CAMERA_FLOOR
    if cam[0] == meta["camera_pos"][0]:        # the chart keeps the time coordinate (ingoing Eddington-Finkelstein does not): it passes through
        assert z["camera_generic"][0] == np.float32(meta["camera_pos"][0])
    assert np.abs(tet - z["tetrad"]).max() <= sm.CAMERA_FLOOR
    assert sm.tetrad_invariant(prog, z["camera_generic"], tet) <= 1e-12
    w, h, rays = meta["width"], meta["height"], z["rays_init"]
    fov = meta["features"].get("field_of_view", 90.0)
    x, e, quat = z["camera_generic"].astype(np.float64), z["tetrad"].astype(np.float64), np.array(meta["camera_quat"], dtype=np.float32)
    pixel = rays["sy"].astype(np.int64) * w + rays["sx"]
    chosen = np.flatnonzero((pixel % 7 == 0) | np.isin(pixel, [0, w - 1, w * (h - 1), w * h - 1]))
    worst = 0.0
    for i in chosen:
        m = sm.pixel_ray(prog, x, e, quat, fov, int(rays["sx"][i]), int(rays["sy"][i]), w, h, 0)
        worst = max([worst, abs(m["ku_uobsu"] - rays["ku_uobsu"][i])] + [np.abs(m[f] - rays[f][i]).max() for f in sm.RAY_FIELDS])
    assert len(chosen) >= min(len(rays), 4) and worst <= sm.RAY_FLOOR, (name, worst)


@pytest.mark.parametrize("name", gs.path_golden_names())
def test_the_model_reproduces_the_path_fixtures(name):
    """tetrad_boosted (gr_boost_tetrad of the stored tetrad) abs 2e-6 and the inertial ray abs 2e-5"""
    meta, z = gs.load_path_golden(name)
    prog = _program_of(meta)
    x, speed = z["camera_generic"].astype(np.float64), np.array(meta["basis_speed"], dtype=np.float32)
    boosted = sm.boost(prog.g(x), z["tetrad"].astype(np.float64), speed)
    assert np.abs(boosted - z["tetrad_boosted"]).max() <= sm.CAMERA_FLOOR
    ray, want = sm.inertial_ray(prog, x, z["tetrad_boosted"].astype(np.float64), speed), z["ray"][0]
    for f in sm.RAY_FIELDS:
        assert np.abs(ray[f] - want[f]).max() <= sm.RAY_FLOOR, (name, f)
    assert want["ku_uobsu"] == 1 and want["running_dlambda_dnew"] == 1 and want["terminated"] == 0


# ---- the model itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["minkowski", "schwarzschild", "kerr_boyer", "kerr_boyer_near_extremal"])
def test_closed_forms_agree_with_the_host_evaluator_at_the_new_poses(name):
    prog, closed = sm.program(name), "kerr_boyer" if name.startswith("kerr_boyer") else name
    poses = [sm.camera_model(c)["generic32"] for c in sm.camera_cases() if c["program"] == name]
    poses += [sm.ray_model(c)["generic32"][None] for c in sm.ray_cases() if c["program"] == name]
    held = 0
    for x in np.concatenate(poses).astype(np.float64):
        if not np.isfinite(x).all():
            continue
        g, polar = rm.closed_form(closed, x, prog.cfg)
        assert np.abs(prog.g(x) - g).max() <= 1e-12 * max(1.0, np.abs(g).max()), (name, x)
        assert np.abs(prog.to_polar(x) - polar).max() <= 1e-12 * max(1.0, np.abs(polar).max()), (name, x)
        held += 1
    assert held >= 20


def test_the_case_list_is_deterministic_and_the_one_named():
    assert [c["name"] for c in sm.camera_cases()] == sm.CAMERA_CASE_NAMES
    first = sm.case_bytes()
    sm._cases.clear()
    assert sm.case_bytes() == first
    for c in sm.camera_cases():
        assert c["count"] <= 64 or (c["name"] == "ordinary_kerr_boyer" and c["count"] == 70)
        assert c["kind"] in ("ordinary", "edge") and c["reaches"]
    sizes = {(c["width"], c["height"]) for c in sm.ray_cases()}
    assert sizes == set(sm.FRAMES) and {c["fov"] for c in sm.ray_cases()} >= set(sm.FOVS)
    norms = sorted(float(np.linalg.norm(c["quat"])) for c in sm.ray_cases())
    assert norms[0] < 1.1e-3 and norms[-1] > 2.9


@pytest.mark.parametrize("name", sm.CAMERA_CASE_NAMES)
def test_camera_cases_take_the_branch_they_name(name):
    c = sm.camera_case(name)
    trace = sm.camera_model(c)["trace"]
    for word, key in (("first_nonzero", "first_nonzero"), ("second frame_basis pass", "second_pass"), ("negative r", "negative_r"), ("degenerate", "degenerate")):
        if word in c["reaches"]:
            assert any(bool(t[key]) for t in trace), (name, word)
    if "flip" in c["reaches"]:
        assert c["flip"] > 0
    if c["kind"] == "ordinary":
        assert not any(t["degenerate"] for t in trace)


@pytest.mark.parametrize("name", [n for n in sm.CAMERA_CASE_NAMES if n.startswith("ordinary")])
def test_the_models_own_invariants_hold_on_ordinary_cases(name):
    """float64 legs are orthonormal in g, the boost of the stored legs too, the inertial ray's velocity has g(u, u) = -1: 1e-12"""
    c = sm.camera_case(name)
    m, prog = sm.camera_model(c), sm.program(c["program"])
    for i in range(c["count"]):
        x = m["generic32"][i]
        assert sm.tetrad_invariant(prog, x, m["tetrad"][i]) <= 1e-12 and sm.tetrad_invariant(prog, x, m["unboosted"][i]) <= 1e-12, (name, i)


@pytest.mark.parametrize("name", [c["name"] for c in sm.ray_cases() if c["kind"] == "ordinary"])
def test_the_models_rays_are_null_on_ordinary_cases(name):
    c = sm.ray_case(name)
    prog, m = sm.program(c["program"]), sm.ray_model(c)
    e = m["tetrad32"].astype(np.float64)
    rays = m["rays"]
    for i in range(c["width"] * c["height"]):
        k = np.linalg.solve(e.T, sm.pixel_ray(prog, m["generic32"].astype(np.float64), e, c["quat"], c["fov"], i % c["width"], i // c["width"],
                                              c["width"], c["height"], c["flip"])["velocity"]) if not prog.generic_constant_theta else None
        if k is not None:
            assert abs(np.sqrt(k[1:] @ k[1:]) - 1) <= 1e-12 and abs(abs(k[0]) - 1) <= 1e-12
        assert abs(rays["ku_uobsu"][i] - rays["velocity"][i] @ (prog.g(rays["position"][i]) @ e[0])) <= 1e-12 * max(1.0, np.abs(rays["velocity"][i]).max())


# ---- the yardstick's conditions ----------------------------------------------------------------------------------------------------
def assert_conditions(name, kind, floor, err, what):
    beyond, aside = sm.shares(floor, err)
    worst = float(np.nanmax(err)) if np.isfinite(np.nan_to_num(err, nan=0.0)).any() and not np.isnan(err).all() else 0.0
    print(f"{name}: {what}: yardstick {worst:.2e} (floor {floor:.0e}), on the widened bound {100 * beyond:.1f} %, set aside {100 * aside:.1f} %")
    if kind == "ordinary":
        assert beyond == 0 and aside == 0, (name, what, worst)
    else:
        assert beyond <= 0.5 and aside <= 0.05, (name, what, beyond, aside)


@pytest.mark.parametrize("name", sm.CAMERA_CASE_NAMES)
def test_the_yardstick_meets_the_conditions_on_camera_cases(name):
    c = sm.camera_case(name)
    got, err, inv, kind = sm.yardstick_camera(c)
    print(f"{name}: yardstick: {kind}")
    for what, e in err.items():
        assert_conditions(name, c["kind"], sm.RAY_FLOOR if what == "inertial" else sm.CAMERA_FLOOR, e, what)
    for what, e in inv.items():
        assert_conditions(name, c["kind"], sm.CAMERA_FLOOR, e, what + " orthonormality")


@pytest.mark.parametrize("name", [c["name"] for c in sm.ray_cases()])
def test_the_yardstick_meets_the_conditions_on_ray_cases(name):
    c = sm.ray_case(name)
    got, err, inv, kind = sm.yardstick_rays(c)
    print(f"{name}: yardstick: {kind}")
    assert_conditions(name, c["kind"], sm.RAY_FLOOR, err, "rays")
    for j, what in enumerate(("null", "ku_uobsu", "spatial length", "initial_quat")):
        if not np.isnan(inv[:, j]).all():
            assert_conditions(name, c["kind"], sm.RAY_FLOOR, inv[:, j], what)
    assert (got["sx"] == np.tile(np.arange(c["width"]), c["height"])).all() and (got["terminated"] == 0).all() and (got["running_dlambda_dnew"] == 1).all()


if __name__ == "__main__":
    print("# the yardstick's largest vec_err against the float64 model per case (tests/setup_model.py) and which yardstick ran")
    for c in sm.camera_cases():
        _, err, _, kind = sm.yardstick_camera(c)
        print(f"  {c['name']:36s} " + " ".join(f"{k} {np.nanmax(v) if not np.isnan(v).all() else 0:.2e}" for k, v in err.items()) + f"  [{kind}]")
    for c in sm.ray_cases():
        _, err, _, kind = sm.yardstick_rays(c)
        print(f"  {c['name']:36s} rays {np.nanmax(err) if not np.isnan(err).all() else 0:.2e}  [{kind}]")
