"""The one-ray Verlet loop's paths for a wave whose live rays are all inside the precision radius (kernels/integrator.hip,
GR_UNIFORM_WAVE_PATHS): the step selection, the far step and - where the host says the radii are ordered, program_build.cpp
radius_exits_ordered - the outer boundary test are skipped there.  They are the same values with fewer instructions, so a frame must
be that of a build with the paths compiled out (-DGR_NO_UNIFORM_WAVE_PATHS) BIT FOR BIT, attempts included.  No tolerance: no value
may change.  The host-side condition itself is tested without a GPU."""
import os

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "geodesic_raytracing_amd", "scripts")
W, H = 256, 144
WITHOUT = " -DGR_NO_UNIFORM_WAVE_PATHS"


def ordered(text):
    return lib.gr_argument_string_radius_exits_ordered(text.encode())


def substituted(name, cfg=None, **features):
    metric = gra.Metric(name, SCRIPTS)
    cfgv = metric.cfg_values(**(cfg or {}))
    feats = metric.features(adaptive_sampling=0, **features)
    return metric, cfgv, feats, metric.argument_string(feats, static=True, cfg_values=cfgv)


# ---- the host-side condition (no GPU) -------------------------------------------------------------------------------------------

def test_host_condition_over_the_shipped_scripts():
    """-DGR_RADIUS_EXITS_ORDERED is passed exactly when the program is substituted, its distance function is the polar radius (decided
    on the generated expressions) and SINGULAR_TERMINATOR < max_precision_radius < universe_size"""
    for name, is_radius in (("kerr_boyer", True), ("kerr_newman_boyer", True), ("schwarzschild", True), ("wormhole", True), ("kerr_schild", False),
                            ("alcubierre", False)):
        metric, _, _, text = substituted(name)
        assert ordered(text) == (1 if is_radius else 0), name               # defaults: terminator (1.05 where there is one) < 10 < 20
        assert ordered(metric.argument_string()) == 0, name                  # features set at run time: nothing is known when it is built
    assert lib.gr_argument_string_radius_exits_ordered(None) == -1


def test_host_condition_follows_the_feature_values():
    for radius, universe, expected in ((10.0, 20.0, 1), (19.5, 20.0, 1), (20.0, 20.0, 0), (25.0, 20.0, 0), (10.0, 5.0, 0)):
        assert ordered(substituted("kerr_boyer", dict(a=0.45), max_precision_radius=radius, universe_size=universe)[3]) == expected, (radius, universe)
    # a SINGULAR metric: the terminator (1.05) bounds the radius from below
    for radius, expected in ((10.0, 1), (1.5, 1), (1.0, 0), (0.5, 0)):
        text = substituted("schwarzschild", max_precision_radius=radius)[3]
        assert "-DSINGULAR" in text.split()
        assert ordered(text) == expected, radius
    # a distance function that is not the variable v2, or a composed form that is not the bare chart radius, is never taken for ordered
    text = substituted("kerr_boyer", dict(a=0.45))[3]
    assert "-DDISTANCE_FUNC=v2 " in text and "-DGR_DISTANCE_OF_GENERIC=v2 " in text
    assert ordered(text.replace("-DDISTANCE_FUNC=v2 ", "-DDISTANCE_FUNC=(v2*1.5f) ")) == 0
    assert ordered(text.replace("-DGR_DISTANCE_OF_GENERIC=v2 ", "-DGR_DISTANCE_OF_GENERIC=(v2+v1) ")) == 0
    # ... nor one whose feature values are not plain literals
    assert ordered(text.replace("-DFEATURE_universe_size=20.0f", "-DFEATURE_universe_size=(10.0f+10.0f)")) == 0


# ---- frames, bit for bit --------------------------------------------------------------------------------------------------------

def frame_and_attempts(text, metric, cfgv, feats, camera, **options):
    from geodesic_raytracing_amd.pipeline import DeviceBuffer
    from test_gpu_fullsize import background
    prog = gra.Program(text, 0)
    state = gra.RenderState(W, H, 0)
    dbg, levels = background()
    out = DeviceBuffer.from_numpy(0, np.full((H, W, 4), np.nan, dtype=np.float32))
    state.render(prog, metric, camera, out.ptr, (dbg.ptr, 1024, 512, levels), feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED, count_attempts=1, **options))
    state.synchronize()
    return out.to_numpy(np.float32, (H, W, 4)), state.attempts()


CASES = {
    # every ray starts inside the precision radius (10): all-inside waves until the rays leave it, then mixed and all-outside ones
    "kerr_camera_inside": ("kerr_boyer", dict(a=0.45), {}, (0, 0, -4, 0), 1, None),
    "kerr_a09_camera_inside": ("kerr_boyer", dict(a=0.9), {}, (0, 0, -4, 0), 1, None),
    # a camera far outside it: waves wholly outside from their first attempt, mixed ones where the rays enter and leave
    "kerr_camera_outside": ("kerr_boyer", dict(a=0.45), {}, (0, 0, -15, 0), 1, None),
    # the host-side condition false - the precision radius beyond the universe: every ray reaches the outer boundary in an all-inside
    # wave, which therefore has to test it
    "kerr_radius_beyond_universe": ("kerr_boyer", dict(a=0.45), dict(max_precision_radius=25.0), (0, 0, -4, 0), 0, None),
    # ... and the radius below the terminator of a SINGULAR metric (1.05)
    "schwarzschild_radius_below_terminator": ("schwarzschild", {}, dict(max_precision_radius=1.0), (0, 0, -4, 0), 0, None),
    "schwarzschild": ("schwarzschild", {}, {}, (0, 0, -4, 0), 1, None),
    # charts whose loop compares squares (the outer boundary is tested in every wave), two holes (the distance is not the chart radius)
    "kerr_schild": ("kerr_schild", {}, {}, (0, 0, -4, 0), 0, None),
    "double_unequal_kerr": ("double_unequal_kerr", {}, {}, (0, 0, -4, 0), None, None),
    # reparameterisation on: `running` is not the constant 1 in the runaway test's ballot
    "kerr_reparameterised": ("kerr_boyer", dict(a=0.45), dict(reparameterisation=1), (0, 0, -4, 0), 1, None),
    # the PARKABLE instance of the same attempt (kernels/trace.hip gr_trace_fused_parking): waves hand their last rays over and take them up
    "kerr_a09_parking": ("kerr_boyer", dict(a=0.9), {}, (0, 0, -4, 0), 1, (" -DGR_PARKING", dict(park_lanes=16, park_trips=64))),
    "alcubierre_camera_outside": ("alcubierre", {}, {}, (0, 0, -15, 0), 0, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_frames_are_those_of_the_build_without_the_shortcuts(case):
    name, cfg, features, position, expect_ordered, build = CASES[case]
    metric, cfgv, feats, text = substituted(name, cfg, **features)
    flags, options = build or ("", {})
    if expect_ordered is not None:
        assert ordered(text) == expect_ordered
    camera = gra.default_camera(position=position)
    got, got_attempts = frame_and_attempts(text + flags, metric, cfgv, feats, camera, **options)
    want, want_attempts = frame_and_attempts(text + flags + WITHOUT, metric, cfgv, feats, camera, **options)
    differing = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
    print(f"{case}: {differing} of {W * H} pixels differ, attempts {got_attempts} vs {want_attempts}")
    assert got_attempts > 0 and got_attempts == want_attempts
    assert differing == 0 and got.tobytes() == want.tobytes()
    assert np.isfinite(got[..., :3]).all() and float(got[..., :3].std()) > 0   # (a picture, not two equal blanks)
