"""GPU parity tests (-m gpu): the HIP kernels, called through the C ABI, against the golden vectors produced by
the reference's own cl.cl (tests/golden/*.npz).  Each stage is fed the GOLDEN output of the previous stage so the
tolerance of one stage is not polluted by the one before it; an end-to-end test then runs the whole chain.

Tolerances (fp32; the reference is built with -cl-unsafe-math-optimizations, both sides differ in reassociation
and libm, and rays near photon orbits amplify 1-ulp differences - SURVEY.md section 8d):
  camera / tetrad          abs 2e-6
  initial rays             abs 2e-5 (position, velocity, acceleration, quaternion, k.u)
                           (the same two floors on cameras made by hand, against a float64 model: tests/test_gpu_setup.py)
  traced rays              termination flags differ for <= 0.5 % of rays (1 % super-extremal Kerr); per ray: a ray is
                           "ordinary" when it took fewer than twice the frame's median number of Verlet attempts, and
                           every ordinary ray that terminated on both sides agrees in position to 1e-3 (position_err:
                           relative to the 4-vector's scale) - all but `slack` of them (gpu_stages.assert_traced_positions;
                           the slack and which approximation owns it: profiles/r03_trace_slack_owner.txt); the 90th
                           percentile of all terminated rays is held to the same 1e-3; total attempts within 0.3 %
  render_data              tex_coord abs 2e-6 (periodic), z_shift 1e-4 relative to |1 + z|, flags exact
                           (the same two on rays made by hand, against a float64 model: tests/test_gpu_render_data.py)
  render (pixels)          RMSE <= 1e-5, max 2e-4 from golden render_data
                           (the same two on records made by hand, against a float64 model: tests/test_gpu_shading.py)
  end to end (pixels)      RMSE <= 1e-4 after masking pixels off by > 1e-3; mask <= 0.5 %
                           (super-extremal Kerr, a naked singularity with chaotic orbits: mask <= 10 %, RMSE <= 3e-4)
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from gpu_stages import FROZEN, Stages, assert_pixels, assert_traced_positions, load_frozen, backgrounds, circ_diff, golden_names, load_golden, metric_for, ordinary_rays, rel_err  # noqa: E402

ADAPTIVE = ["kerr_adaptive_sampling", "schwarzschild_adaptive_black_features"]
PLAIN = [n for n in golden_names() if not n.endswith("_prepass") and n not in ADAPTIVE]
CHAOTIC = {"kerr_superextremal", "double_unequal_kerr_hyperextreme"}


@pytest.mark.parametrize("name", golden_names())
def test_camera_and_tetrad(name):
    meta, z = load_golden(name)
    cam, tet = Stages(meta).camera()
    assert np.abs(cam - z["camera_generic"]).max() <= 2e-6
    assert np.abs(tet - z["tetrad"]).max() <= 2e-6


@pytest.mark.parametrize("name", PLAIN)
def test_init_rays(name):
    meta, z = load_golden(name)
    got = Stages(meta).init_rays(z["camera_generic"], z["tetrad"])
    want = z["rays_init"]
    assert len(got) == len(want)
    for f in ("position", "velocity", "acceleration", "initial_quat"):
        assert np.abs(got[f] - want[f]).max() <= 2e-5, f
    assert np.abs(got["ku_uobsu"] - want["ku_uobsu"]).max() <= 2e-5
    for f in ("sx", "sy", "terminated"):
        assert (got[f] == want[f]).all(), f
    assert np.abs(got["running_dlambda_dnew"] - 1).max() == 0


@pytest.mark.parametrize("size", [(50, 30), (67, 3), (8, 8), (1, 1)])
def test_init_rays_of_frames_that_do_not_fill_their_last_wave(size):
    """gr_init_rays_generic stores a wave's 64 records as one run of bytes (staged through LDS): frames whose slot count is no multiple
    of 64 - the last wave's run is shorter - in reference slot order and in tile order (where slots outside the image are dead records):
    the records of a pixel are the same bits in both orders and in a larger frame's launch shape, nothing is written behind the last
    record, and the struct's padding is zero"""
    from geodesic_raytracing_amd.pipeline import DeviceBuffer
    from gpu_stages import LIGHTRAY_DTYPE, buf
    meta, z = load_golden("kerr")
    w, h = size
    st = Stages(dict(meta, width=w, height=h))
    e = [buf(z["tetrad"][i].astype(np.float32)) for i in range(4)]
    cam = buf(z["camera_generic"].astype(np.float32))
    term = buf(np.zeros(w * h, dtype=np.int32))
    records = {}
    for tiled in (0, 1):
        slots = gra.lib.gr_tiled_slot_count(w, h) if tiled else w * h
        raw = DeviceBuffer.from_numpy(0, np.full((slots + 8) * 96, 0xA5, dtype=np.uint8))   # eight records of guard bytes behind the list
        count = buf(np.zeros(1, dtype=np.int32))
        gra.check(gra.lib.gr_init_rays_generic(st.p, None, cam.ptr, st.quat.ptr, raw.ptr, count.ptr, w, h, term.ptr, w, h, 0, e[0].ptr, e[1].ptr,
                                               e[2].ptr, e[3].ptr, st.cfg.ptr, st.dfg.ptr, 0, tiled))
        got = raw.to_numpy(np.uint8, ((slots + 8) * 96,))
        assert int(count.to_numpy(np.int32, 1)[0]) == slots
        assert (got[slots * 96:] == 0xA5).all()
        rays = got[:slots * 96].view(LIGHTRAY_DTYPE)
        assert (rays["pad"] == 0).all()
        inside = rays["sx"] >= 0
        assert inside.sum() == w * h and (rays["terminated"][~inside] == 2).all()
        order = np.argsort(rays["sy"][inside].astype(np.int64) * w + rays["sx"][inside], kind="stable")
        records[tiled] = rays[inside][order]
    assert records[0].tobytes() == records[1].tobytes()
    assert (records[0]["sx"] == np.tile(np.arange(w), h)).all() and (records[0]["sy"] == np.repeat(np.arange(h), w)).all()


@pytest.mark.parametrize("name", PLAIN)
def test_trace(name):
    meta, z = load_golden(name)
    got = Stages(meta).trace(z["rays_init"])
    want = z["rays"]
    mismatch = (got["terminated"] != want["terminated"]).mean()
    assert mismatch <= (0.01 if name in CHAOTIC else 0.005)
    assert_traced_positions(name, got, want, ordinary_rays(meta, z), chaotic=name in CHAOTIC)
    # rays that did not terminate keep their initial record (the reference only writes on termination)
    lost = (got["terminated"] == 0) & (want["terminated"] == 0)
    assert (got["position"][lost] == z["rays_init"]["position"][lost]).all()


@pytest.mark.parametrize("name", PLAIN)
def test_render_data(name):
    meta, z = load_golden(name)
    got = Stages(meta).render_data(z["rays"])
    want = z["render_data"]
    for f in ("terminated", "sx", "sy", "side"):
        assert (got[f] == want[f]).all(), f
    ok = want["terminated"] == 1
    # a ray that ends near a pole has ill-conditioned sky angles (theta = acos(z/r), phi = atan2: both ~ eps / sin theta),
    # so the bound is on the angular distance on the sphere, i.e. weighted by sin(theta)
    dtex = circ_diff(got["tex_coord"][ok], want["tex_coord"][ok])
    sin_theta = np.maximum(np.sin(np.pi * want["tex_coord"][ok][:, 1]), 1e-3)
    assert (dtex * sin_theta[:, None]).max() <= 2e-6
    assert np.percentile(dtex, 99) <= 2e-6
    # rays stopped just outside the horizon evaluate 1/sqrt|g_tt| with g_tt = 1/r - 1 -> 0: ill-conditioned, so bound the
    # bulk tightly and the worst case relative to |1 + z|
    dz = np.abs(got["z_shift"][ok] - want["z_shift"][ok])
    assert (dz / (1 + np.abs(want["z_shift"][ok]))).max() <= 1e-4


@pytest.mark.parametrize("name", PLAIN)
def test_render_pixels(name):
    meta, z = load_golden(name)
    bg, bg2, levels = backgrounds(meta)
    got = Stages(meta).render(z["render_data"], bg, bg2, levels, meta["max_probes"])
    d = got[..., :3] - z["pixels"][..., :3]
    assert np.sqrt((d ** 2).mean()) <= 1e-5
    assert np.abs(d).max() <= 2e-4
    assert (got[..., 3] == z["pixels"][..., 3]).all() or np.abs(got[..., 3] - z["pixels"][..., 3]).max() <= 1e-6


@pytest.mark.parametrize("name", PLAIN)
def test_end_to_end(name):
    meta, z = load_golden(name)
    st = Stages(meta)
    cam, tet = st.camera()
    rays = st.trace(st.init_rays(cam, tet))
    bg, bg2, levels = backgrounds(meta)
    px = st.render(st.render_data(rays), bg, bg2, levels, meta["max_probes"])
    d = px[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= (0.10 if name in CHAOTIC else 0.005)
    assert np.sqrt((d[~bad] ** 2).mean()) <= (3e-4 if name in CHAOTIC else 1e-4)


def _frame(meta, mode, tiled=0, options=None, substituted=False, extra_arguments=""):
    """whole frame through gr_render_frame; substituted = the program with $cfg values and features baked in (the one
    bench.py times, metric_manager.hpp:153-166) instead of the dynamic one; extra_arguments: appended to the argument string"""
    from geodesic_raytracing_amd.pipeline import DeviceBuffer
    metric = metric_for(meta)
    feats = gra.default_features(**meta["features"])
    if substituted:
        prog = gra.Program(metric.argument_string(features=feats, static=True, cfg_values=meta["cfg"]) + extra_arguments, 0)
    else:
        prog = gra.Program(metric.argument_string() + extra_arguments, 0)
    w, h = meta["width"], meta["height"]
    state = gra.RenderState(w, h, 0)
    bg, bg2, levels = backgrounds(meta)
    dbg, dbg2 = DeviceBuffer.from_numpy(0, bg), DeviceBuffer.from_numpy(0, bg2)
    out = DeviceBuffer(0, w * h * 16)
    cam = gra.default_camera(meta["camera_pos"], meta["camera_quat"])
    cam.basis_speed = (gra.c_float * 3)(*meta["basis_speed"])
    cam.flip = float(meta.get("flip", 0.0))
    opts = gra.frame_options(mode=mode, tiled=tiled, use_prepass=int(meta["prepass"]), **dict(dict(max_probes=meta["max_probes"]), **(options or {})))
    state.render(prog, metric, cam, out.ptr, ((dbg.ptr, dbg2.ptr), bg.shape[2], bg.shape[1], levels), feats, meta["cfg"], opts)
    state.synchronize()
    return out.to_numpy(np.float32, (h, w, 4)), state


@pytest.mark.parametrize("name", ["kerr_prepass", "kerr_schild_prepass"])
def test_prepass_matches_reference(name):
    """termination buffer, the terminated == 2 stencil and the final image with the prepass on (cl.cl:3213-3232, 5008-5020)"""
    from geodesic_raytracing_amd.pipeline import download
    meta, z = load_golden(name)
    px, state = _frame(meta, gra.MODE_REFERENCE)
    pw, ph = meta["width"] // 16, meta["height"] // 16
    term = download(0, state.buffer(gra.BUF_TERMINATION), np.int32, pw * ph).reshape(ph, pw)
    assert (term != z["termination"]).mean() <= 0.01
    st = Stages(meta)
    rays = st.init_rays(z["camera_generic"], z["tetrad"], termination=z["termination"].reshape(-1), prepass_size=(pw, ph))
    # the stencil cell is round(cx / width * prepass_width) (cl.cl:3217-3221); where that product is an exact .5 tie the
    # result depends on how a compiler rounds/reassociates the fp32 quotient (true of the reference itself on any OpenCL
    # device), so tie columns/rows are excluded from the exact comparison
    tie_x = (rays["sx"] * pw * 2) % (2 * meta["width"]) == meta["width"]
    tie_y = (rays["sy"] * ph * 2) % (2 * meta["height"]) == meta["height"]
    certain = ~(tie_x | tie_y)
    assert certain.mean() > 0.85
    assert (rays["terminated"][certain] == z["rays_init"]["terminated"][certain]).all()
    assert (rays["terminated"] == 2).sum() > 0
    d = px[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= 0.005
    assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_sampling_matches_reference(name):
    """quarter-resolution primary rays + refinement (handle_adaptive_sampling, cl.cl:5223-5345)"""
    from geodesic_raytracing_amd.pipeline import download
    meta, z = load_golden(name)
    px, state = _frame(meta, gra.MODE_REFERENCE)
    n_new = int(download(0, state.buffer(gra.BUF_RAYS_ADAPTIVE_COUNT), np.int32, 1)[0])
    assert abs(n_new - meta["adaptive_count"]) <= 6
    d = px[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= 0.01
    assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_sampling_on_the_fused_path_matches_reference(name):
    """the golden frames through the fused kernels: half-resolution lattice (gr_trace_fused_launch, lattice = 2), gr_adaptive_refine,
    second fused launch over the marked pixels.  The decision is taken on the ray end states the lattice launch leaves in lattice_rays -
    the reference's get_intersection_position of every lattice ray, also of those whose record is black.  (Until the adaptive soak -
    tests/fuzz_parity.py with FUZZ_ADAPTIVE=1 - it read them back out of the records' texture coordinates, which are 0, 0 for a black
    record: in schwarzschild_adaptive_black_features, a frame full of thin black features, 223 of 2 304 pixels came out wrong.)"""
    from geodesic_raytracing_amd.pipeline import download
    meta, z = load_golden(name)
    px, state = _frame(meta, gra.MODE_FUSED)
    n_new = int(download(0, state.buffer(gra.BUF_RAYS_ADAPTIVE_COUNT), np.int32, 1)[0])
    assert abs(n_new - meta["adaptive_count"]) <= 12
    rd = download(0, state.buffer(gra.BUF_RENDER_DATA), gra.pipeline.RENDER_DATA_DTYPE, meta["width"] * meta["height"])
    assert (rd["terminated"] >= 0).all()             # no record left pending
    d = px[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= 0.01
    assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4
    # ... and the substituted program, with the metric's prepass on as in the GUI
    px2, _ = _frame(dict(meta, prepass=True), gra.MODE_FUSED, substituted=True)
    d = px2[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= 0.01


@pytest.mark.parametrize("name", ["kerr", "schwarzschild_redshift", "alcubierre", "kerr_prepass", "kerr_schild_prepass"])
def test_fused_and_tiled_paths_equal_reference_sequence(name):
    """the 8x8-tiled ray order is bit-identical to the reference order (same kernels); the fused kernel is the same
    device functions inlined into another kernel, where the compiler contracts/reassociates differently, so it is held
    to the end-to-end tolerance instead"""
    meta, z = load_golden(name)
    ref, _ = _frame(meta, gra.MODE_REFERENCE, tiled=0)
    tiled, _ = _frame(meta, gra.MODE_REFERENCE, tiled=1)
    fused, _ = _frame(meta, gra.MODE_FUSED)
    assert np.array_equal(ref, tiled)
    for other in (ref, z["pixels"]):
        d = fused[..., :3] - other[..., :3]
        bad = np.abs(d).max(axis=2) > 1e-3
        assert bad.mean() <= 0.005
        assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4


SUBSTITUTED = ["schwarzschild_adaptive", "schwarzschild_adaptive_rs", "kerr", "kerr_tilted", "kerr_far", "kerr_prepass", "kerr_newman", "kerr_schild", "kerr_schild_prepass", "kerr_moving_observer", "kerr_reparameterised", "schwarzschild_redshift",
               "alcubierre", "ingoing_ef", "double_unequal_kerr", "cosmic_string", "wormhole_through"]


@pytest.mark.parametrize("name", SUBSTITUTED)
@pytest.mark.parametrize("mode", ["fused", "reference"])
def test_substituted_program_matches_reference(name, mode):
    """the program bench.py times (parameters and features folded into literals) against the reference's pixels, through the
    fused kernel and through the reference-shaped kernel sequence"""
    meta, z = load_golden(name)
    px, _ = _frame(meta, gra.MODE_FUSED if mode == "fused" else gra.MODE_REFERENCE, substituted=True)
    d = px[..., :3] - z["pixels"][..., :3]
    bad = np.abs(d).max(axis=2) > 1e-3
    assert bad.mean() <= 0.005
    assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4


@pytest.mark.parametrize("name", ["kerr", "kerr_far", "kerr_tilted", "alcubierre", "schwarzschild", "ingoing_ef", "cosmic_string", "kerr_newman",
                                  "kerr_schild"])
def test_step_attempts_match_oracle(name):
    """the number of Verlet attempts is a sensitive summary of the step-size controller (a wrong precision-radius test or a
    lagging step length changes it by percent while end pixels barely move): GPU kernels - dynamic and substituted, fused
    and reference-shaped - against the CPU restatement, which is pinned to the reference's own kernels"""
    import ctypes
    from oracle import build_restate
    from oracle.refpipe import OraclePipeline, pack_features
    meta, z = load_golden(name)
    metric = metric_for(meta)
    pipe = OraclePipeline(build_restate.build(metric.argument_string()))
    pipe.frame(meta["width"], meta["height"], meta["cfg"], pack_features(**meta["features"]), camera_pos=meta["camera_pos"],
               camera_quat=meta["camera_quat"], basis_speed=meta["basis_speed"], flip=float(meta.get("flip", 0.0)), stages="trace", nthreads=4)
    pipe.lib.ref_last_attempts.restype = ctypes.c_uint64
    want = int(pipe.lib.ref_last_attempts())
    got = {}
    _, att = Stages(meta).trace(z["rays_init"], count_attempts=True)
    got["dynamic reference-shaped"] = att
    for substituted in (False, True):
        _, state = _frame(meta, gra.MODE_FUSED, options=dict(count_attempts=1), substituted=substituted)
        got["substituted fused" if substituted else "dynamic fused"] = state.attempts()
    for label, att in got.items():
        assert abs(att - want) <= 0.003 * want, (label, att, want)


def test_randomised_poses_and_features_match_the_oracle():
    """one random case per shipped metric - eleven, the wormhole with its two skies among them - (parameters, camera pose and orientation, observer speed, redshift / reparameterisation /
    field of view / universe size), dynamic and substituted program, against the CPU oracle: tests/fuzz_parity.py with a fixed seed"""
    import importlib.util
    import os
    import sys
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_parity.py")
    spec = importlib.util.spec_from_file_location("fuzz_parity", path)
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    argv = sys.argv
    try:
        sys.argv = ["fuzz_parity.py", "11", "7"]
        assert fuzz.main() == 0
    finally:
        sys.argv = argv


POLAR = ["kerr_newman_axis_13_3", "kerr_axis_14_212", "kerr_newman_axis_14_593", "kerr_axis_21_122", "kerr_axis_22_142", "kerr_newman_axis_23_63",
         "kerr_axis_32_135", "kerr_axis_32_267", "kerr_axis_33_575", "double_kerr_axis_33_541",
         "kerr_newman_axis_41_4", "kerr_newman_axis_41_48", "kerr_newman_axis_41_114", "cosmic_string_axis_42_1"]


def sky_error(position, position_f64):
    """largest error of the two angular coordinates (Boyer-Lindquist theta, phi) of final positions against the float64 run"""
    d = np.abs(np.asarray(position, dtype=np.float64)[:, 2:] - position_f64[:, 2:])
    return d.max(axis=1)


@pytest.mark.parametrize("name", POLAR)
def test_polar_axis_cases_of_the_soak(name):
    """The cases of the randomised soaks (three of 1 270 in round 1, three of 897 in round 2, eight of 2 120 in round 3) in which > 1 % of the pixels were off by > 1e-3 (tests/golden/polar, inputs as
    the soak drew them, expected output from the reference's cl.cl): rays grazing the polar axis of a Boyer-Lindquist chart.  There
    d phi / d lambda ~ 1 / sin^2 theta amplifies every last-place difference, so two fp32 builds agree only as far as they share
    their roundings - the CPU restatement (same operation order as the reference) disagrees with it in 11-30 pixels, the GPU
    (contraction, reassociation) in 24-52 - and the reference itself is off from a float64 evaluation of the same algorithm
    (oracle ref_trace_f64) in as many rays as the GPU is.  Rules: flags equal; the GPU is not further from the float64 evaluation
    than the reference is (rays whose sky angles are off by > 1e-3: at most 1.5x the reference's count + 4); and its pixels differ
    from the reference's in at most twice as many places as the larger of (CPU restatement vs reference) and (reference vs
    float64) + 4.  Measured (dynamic / substituted program): 13/3 27/24 pixels (CPU 22), 14/212 51/52 (CPU 11, reference vs float64
    48 rays), 14/593 32/29 (CPU 30), 21/122 35-37 (CPU 38, reference vs float64 34 rays), 22/142 55-58 (CPU 58, reference vs float64 75 rays), 23/63 32-37 (CPU 16, reference vs float64 56 rays), 32/135 225-226 (CPU 157), 32/267 102-109 (CPU 95), 33/575 125 (CPU 107), 33/541 28-30 (CPU 25: double Kerr, the camera near the symmetry axis of the Weyl chart) - the round-3 Kerr cases have the camera itself near the axis at r ~ 11, so a tenth
    of the frame's rays pass it; GR_LIBM_TRIG, correctly rounded divide/sqrt and no contraction change none of it.  Seed 41 (after the tile history went in): three
    Kerr-Newman cameras at r ~ 11, outside the precision radius, 110 degree view, universe 30 - 41/4 and 41/114 have the axis inside the
    view (the pixels that differ are one strip three or four columns wide: CPU restatement 22 and 27 pixels, reference vs float64 19 and
    27 rays), 41/48 sits 8 degrees from it (CPU 29, reference vs float64 111 rays).  Seed 42 (600 cases; the soak now holds its outliers
    against the reference's x86 build and the float64 evaluation itself): two more of the kind, explained on the spot, and a cosmic-string
    camera 16 degrees from the string - the axis of that chart - at r ~ 10.4: CPU 12 pixels, reference vs float64 65 rays, GPU 46-47."""
    from oracle import build_restate
    from oracle.refpipe import OraclePipeline, pack_features
    meta, z = load_golden("polar/" + name)
    pipe = OraclePipeline(build_restate.build(metric_for(meta).argument_string()))
    feats = pack_features(**meta["features"])
    p64, t64 = pipe.trace_f64(z["rays_init"], meta["cfg"], feats, nthreads=8)
    want = z["rays"]
    got = Stages(meta).trace(z["rays_init"])
    assert (got["terminated"] != want["terminated"]).mean() <= 0.005
    both = (t64 == 1) & (want["terminated"] == 1) & (got["terminated"] == 1)
    reference_off = int((sky_error(want["position"][both], p64[both]) > 1e-3).sum())
    gpu_off = int((sky_error(got["position"][both], p64[both]) > 1e-3).sum())
    assert gpu_off <= 1.5 * reference_off + 4, (gpu_off, reference_off)
    # pixels, end to end, both programs
    bg, bg2, levels = backgrounds(meta)
    cpu = pipe.frame(meta["width"], meta["height"], meta["cfg"], feats, camera_pos=meta["camera_pos"], camera_quat=meta["camera_quat"],
                     basis_speed=meta["basis_speed"], background=(bg, bg2, levels), nthreads=8)
    cpu_bad = int((np.abs(cpu["pixels"][..., :3] - z["pixels"][..., :3]).max(axis=2) > 1e-3).sum())
    for substituted in (False, True):
        px, _ = _frame(meta, gra.MODE_FUSED, substituted=substituted)
        d = px[..., :3] - z["pixels"][..., :3]
        bad = np.abs(d).max(axis=2) > 1e-3
        assert bad.sum() <= 2 * max(cpu_bad, reference_off) + 4, (int(bad.sum()), cpu_bad, reference_off)
        assert np.sqrt((d[~bad] ** 2).mean()) <= 1e-4


@pytest.mark.parametrize("program", ["dynamic", "substituted"])
@pytest.mark.parametrize("name", FROZEN)
def test_frames_match_the_fixtures_frozen_before_the_generator_changed(name, program):
    """tests/golden/frozen/ (README there): cl.cl's pixels from the strings the generator wrote BEFORE round 5 added cancellation rules and
    re-ordered operands - never regenerated - against today's programs (today's strings, today's device lowering) on the GPU, with the
    end-to-end rule of the ordinary fixtures.  What moves values rather than roundings fails here."""
    meta, z = load_frozen(name)
    px, _ = _frame(meta, gra.MODE_FUSED, substituted=program == "substituted")
    assert_pixels(name, meta, z, px)


@pytest.mark.parametrize("name,scripts,cfg_kw,camera_pos,size", [
    ("kerr_boyer", True, dict(a=0.45), [0.0, 0.0, -4.0, 0.0], (96, 54)),
    ("kerr_boyer", False, dict(a=0.45), [0.0, 0.5, -5.0, 1.0], (64, 36)),
    ("alcubierre", True, {}, [0.0, 0.0, -6.0, 0.5], (64, 36)),
    ("schwarzschild", True, {}, [0.0, 0.0, -4.0, 0.0], (128, 72)),   # (at 64 x 36 the shadow's edge alone is 12 of 2 304 pixels: 0.52 % against the rule's 0.5 %)
    ("double_unequal_kerr", True, {}, [0.0, 0.0, -6.0, 0.5], (48, 27))])
def test_gpu_frames_against_the_reference_object_itself(name, scripts, cfg_kw, camera_pos, size):
    """a GPU-box parity job whose checker is the reference's own code - /root/reference/cl.cl compiled for x86-64 in the build
    container (oracle/_ref/libref_<metric>.so, oracle/build_ref.py; it travels with the tree since round 6) - RUN HERE on a pose no
    fixture holds, not read back from a fixture and not the restatement.  Whole frames, fused path, dynamic and substituted program,
    the end-to-end rule of the fixtures.  Skipped where the object did not travel (a fresh clone: the fixtures and the restatement remain)."""
    import os
    from oracle import build_ref
    from oracle.refpipe import OraclePipeline, pack_features
    from gpu_stages import SCRIPTS_DIR
    metric = gra.Metric(name, SCRIPTS_DIR if scripts else None)
    so = build_ref.prebuilt(name + ("_script" if scripts else ""), metric.argument_string())
    if so is None:
        pytest.skip("no oracle/_ref object for this macro string on this box")
    w, h = size
    cfg = metric.cfg_values(**cfg_kw)
    fkw = dict(adaptive_sampling=0, max_acceleration_change=metric.info.max_acceleration_change)
    meta = dict(metric=name, scripts=scripts, width=w, height=h, cfg=cfg, features=fkw, camera_pos=camera_pos, camera_quat=list(gra.default_camera().quat),
                prepass=False, bg_size=[256, 128], bg_seed=1234, bg_seed2=4321, basis_speed=[0.0, 0.0, 0.0], max_probes=8)
    bg, bg2, levels = backgrounds(meta)
    ref = OraclePipeline(so).frame(w, h, cfg, pack_features(**fkw), camera_pos=camera_pos, camera_quat=meta["camera_quat"], use_prepass=False,
                                   background=(bg, bg2, levels), basis_speed=[0.0, 0.0, 0.0], nthreads=os.cpu_count() or 4, max_probes=8)
    for substituted in (False, True):
        px, _ = _frame(meta, gra.MODE_FUSED, substituted=substituted)
        assert_pixels(name, meta, {"pixels": ref["pixels"]}, px)
