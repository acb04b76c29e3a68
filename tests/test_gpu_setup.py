"""GPU tests (-m gpu) of the set-up stage on cameras made by hand: gr_cart_to_generic, gr_init_basis_vectors, gr_boost_tetrad,
gr_init_inertial_ray, gr_init_rays_generic and gr_camera_setup (kernels/camera.hip, geodesic_camera.hip, setup.hip) against the
float64 model of tests/setup_model.py, on the cases that module lists.

The rule (gpu_stages.assert_path_against_float64's factor, with the stage's own floors), per value - a pose's vector, a ray: the
device's vec_err against the model is at most max(floor, 1.5 x the fp32 yardstick's on that same value) - floor 2e-6 for camera and
tetrad, 2e-5 for rays - so a value on which the yardstick is within the floor is held to the floor whatever else its case holds; the yardstick is the reference's own object where one is built for the program's string, the CPU restatement otherwise
(tests/test_setup_model.py, which asserts that on ordinary cases the floor is the bound that applies).  Where the model's own value
or the yardstick's result is not finite nothing is compared, and the pattern of finite components equals the yardstick's.  The invariants - legs orthonormal in
g, rays null, ku_uobsu = k.g.e0, unit spatial part, initial_quat undoing the rotation - are computed in float64 from the device's own
output and bounded the same way (the orthonormality residual is the plain one, and relative to the size of what is summed at
|v| >= 0.99 only: setup_model.tetrad_invariant says why).

Every output sits between eight records of guard bytes."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import setup_model as sm  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, download  # noqa: E402
from oracle.refpipe import LIGHTRAY_DTYPE  # noqa: E402

GUARD = 8                 # records either side of every output
GUARD_BYTE = 0xA5
_shared = {}


def device_program(name, substituted=False):
    key = ("program", name, substituted)
    if key not in _shared:
        prog = sm.program(name)
        cfg = DeviceBuffer.from_numpy(0, np.array(prog.cfg or [0.0], dtype=np.float32))
        _shared[key] = (gra.Program(prog.substituted_string() if substituted else prog.argument_string, 0), cfg)
    return _shared[key]


class Guarded:
    """a device array of `count` records of `size` bytes between guard records; `initial` fills the records (in / out arguments)"""

    def __init__(self, count, size, initial=None):
        self.count, self.size = count, size
        raw = np.full((count + 2 * GUARD) * size, GUARD_BYTE, dtype=np.uint8)
        if initial is not None:
            raw[GUARD * size:(GUARD + count) * size] = np.ascontiguousarray(initial).view(np.uint8).ravel()
        self.buffer = DeviceBuffer.from_numpy(0, raw)
        self.ptr = ctypes.c_void_p(self.buffer.ptr.value + GUARD * size)

    def read(self, dtype, shape):
        raw = self.buffer.to_numpy(np.uint8, ((self.count + 2 * GUARD) * self.size,))
        lo, hi = GUARD * self.size, (GUARD + self.count) * self.size
        assert (raw[:lo] == GUARD_BYTE).all() and (raw[hi:] == GUARD_BYTE).all(), "guard records were written"
        return raw[lo:hi].copy().view(dtype).reshape(shape)


def up(a):
    """an input on the device; the caller holds the buffer in a name until its launch has finished (a DeviceBuffer frees its memory
    when it is collected)"""
    return DeviceBuffer.from_numpy(0, np.ascontiguousarray(a))


def cart_to_generic(p, cfg, cart, flip):
    out, d_cart = Guarded(len(cart), 16), up(cart.astype(np.float32))
    check(lib.gr_cart_to_generic(p.handle, None, d_cart.ptr, out.ptr, len(cart), float(flip), cfg.ptr))
    check(lib.gr_device_synchronize(0))
    return out.read(np.float32, (len(cart), 4))


def init_basis_vectors(p, cfg, generic32, speeds):
    """one launch per distinct speed (the kernel's speed is a scalar argument) -> tetrads [n][4][4]"""
    n = len(generic32)
    out = np.zeros((n, 4, 4), dtype=np.float32)
    for speed in np.unique(speeds, axis=0):
        rows = np.flatnonzero((speeds == speed).all(axis=1))
        e, d_generic = [Guarded(len(rows), 16) for _ in range(4)], up(generic32[rows])
        check(lib.gr_init_basis_vectors(p.handle, None, d_generic.ptr, len(rows), (ctypes.c_float * 3)(*[float(v) for v in speed]),
                                        e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, cfg.ptr))
        check(lib.gr_device_synchronize(0))
        for a in range(4):
            out[rows, a] = e[a].read(np.float32, (len(rows), 4))
    return out


def _speed4(speeds):
    s = np.zeros((len(speeds), 4), dtype=np.float32)
    s[:, :3] = speeds
    return s


def boost_tetrad(p, cfg, generic32, speeds, legs32):
    n = len(generic32)
    e = [Guarded(n, 16, legs32[:, a]) for a in range(4)]
    d_generic, d_speed = up(generic32), up(_speed4(speeds))
    check(lib.gr_boost_tetrad(p.handle, None, d_generic.ptr, n, d_speed.ptr, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, cfg.ptr))
    check(lib.gr_device_synchronize(0))
    return np.stack([e[a].read(np.float32, (n, 4)) for a in range(4)], axis=1)


def init_inertial_ray(p, cfg, generic32, legs32, speeds):
    n = len(generic32)
    rays, count = Guarded(n, LIGHTRAY_DTYPE.itemsize), Guarded(1, 4, np.array([-7], dtype=np.int32))
    e = [up(legs32[:, a]) for a in range(4)]
    d_generic, d_speed = up(generic32), up(_speed4(speeds))
    check(lib.gr_init_inertial_ray(p.handle, None, d_generic.ptr, n, rays.ptr, count.ptr, e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr,
                                   d_speed.ptr, cfg.ptr))
    check(lib.gr_device_synchronize(0))
    assert int(count.read(np.int32, (1,))[0]) == n
    return rays.read(LIGHTRAY_DTYPE, (n,))


def init_rays(p, cfg, c, tiled):
    m = sm.ray_model(c)
    w, h = c["width"], c["height"]
    slots = lib.gr_tiled_slot_count(w, h) if tiled else w * h
    rays, count = Guarded(slots, LIGHTRAY_DTYPE.itemsize), Guarded(1, 4, np.array([-7], dtype=np.int32))
    e = [up(m["tetrad32"][a]) for a in range(4)]
    dfg = up(np.frombuffer(bytes(gra.default_features(field_of_view=c["fov"], adaptive_sampling=0)), dtype=np.uint8))
    d_generic, d_quat, d_term = up(m["generic32"]), up(c["quat"]), up(np.zeros(w * h, dtype=np.int32))
    check(lib.gr_init_rays_generic(p.handle, None, d_generic.ptr, d_quat.ptr, rays.ptr, count.ptr, w, h,
                                   d_term.ptr, w, h, int(c["flip"]), e[0].ptr, e[1].ptr, e[2].ptr, e[3].ptr, cfg.ptr,
                                   dfg.ptr, 0, tiled))
    check(lib.gr_device_synchronize(0))
    assert int(count.read(np.int32, (1,))[0]) == slots
    got = rays.read(LIGHTRAY_DTYPE, (slots,))
    assert (got["pad"] == 0).all() and (got["terminated"][got["sx"] < 0] == 2).all()
    return sm.slot_order(got, w, h)


def run_camera_case(c, substituted=False):
    """every camera kernel of a case, each on the fp32 inputs the model states for it -> dict like the yardstick's"""
    key = ("camera", c["name"], substituted)
    if key not in _shared:
        p, cfg = device_program(c["program"], substituted)
        m = sm.camera_model(c)
        got = dict(tetrad=init_basis_vectors(p, cfg, m["generic32"], c["speeds"]),
                   reboosted=boost_tetrad(p, cfg, m["generic32"], c["speeds"], m["unboosted32"]),
                   inertial=init_inertial_ray(p, cfg, m["generic32"], m["tetrad32"], sm.inertial_speeds(c)))
        if c["cart"] is not None:
            got["camera"] = cart_to_generic(p, cfg, c["cart"], c["flip"])
        _shared[key] = got
    return _shared[key]


def assert_same_finite_pattern(name, what, got, yard, model):
    """in every record (a pose's vector, a ray's) where the model's own value or the yardstick's result is not finite: a component
    the model has finite is finite on the device, and on the others the device's pattern of finite components is the yardstick's.
    (The first clause is correct_lightray's: on a constant-theta chart the kernel, and the model with it, keeps a ray's first two
    coordinates and their rates as they went in, where the reference takes them through the rotation - with a tetrad that is not
    finite the reference's come back NaN and the kernel's are the camera's.)"""
    got, yard, model = (np.asarray(a, dtype=np.float64) for a in (got, yard, model))
    aside = ~(np.isfinite(model).all(axis=-1) & np.isfinite(yard).all(axis=-1))
    expected = np.where(np.isfinite(model) & ~np.isfinite(model).all(axis=-1, keepdims=True), True, np.isfinite(yard))
    differ = aside & (np.isfinite(got) != expected).any(axis=-1)
    assert not differ.any(), (name, what, np.argwhere(differ).tolist(), got[differ].tolist(), yard[differ].tolist(), model[differ].tolist())


def _worst(a):
    a = np.asarray(a, dtype=np.float64)
    a = a[np.isfinite(a)]
    return float(a.max()) if a.size else 0.0


def assert_camera_case(c, substituted):
    got = run_camera_case(c, substituted)
    yard, yard_err, yard_inv, kind = sm.yardstick_camera(c)
    m = sm.camera_model(c)
    err, inv = sm.camera_errors(c, got), sm.camera_invariants(c, got)
    program = "substituted" if substituted else "dynamic"
    # the patterns first: where the yardstick is not finite the figures below say nothing
    if c["cart"] is not None:
        assert_same_finite_pattern(c["name"], "camera", got["camera"], yard["camera"], m["camera"])
    for what in ("tetrad", "reboosted"):
        assert_same_finite_pattern(c["name"], what, got[what], yard[what], m[what])
    for f in sm.RAY_FIELDS:
        assert_same_finite_pattern(c["name"], f, got["inertial"][f], yard["inertial"][f], m["inertial"][f])
    for what, e in err.items():
        floor = sm.RAY_FLOOR if what == "inertial" else sm.CAMERA_FLOOR
        held = sm.assert_within(c["name"], what, floor, e, yard_err[what])
        print(f"{c['name']} [{program}]: {what}: gpu {_worst(e):.2e} yardstick ({kind}) {_worst(yard_err[what]):.2e}, {held} of {len(e)} poses held to the floor {floor:.0e}")
    for what, e in inv.items():
        print(f"{c['name']} [{program}]: {what} orthonormality: gpu {_worst(e):.2e} yardstick {_worst(yard_inv[what]):.2e}")
        sm.assert_within(c["name"], what + " orthonormality", sm.CAMERA_FLOOR, e, yard_inv[what])
    ray = got["inertial"]
    assert (ray["ku_uobsu"] == 1).all() and (ray["running_dlambda_dnew"] == 1).all() and (ray["terminated"] == 0).all()
    assert (ray["sx"] == 0).all() and (ray["sy"] == 0).all()
    for i, t in enumerate(m["trace"]):
        if t["degenerate"]:      # the early return: the identity tetrad
            assert (got["tetrad"][i] == np.eye(4, dtype=np.float32)).all(), (c["name"], i)


@pytest.mark.parametrize("name", sm.CAMERA_CASE_NAMES)
def test_camera_kernels_against_the_float64_model(name):
    assert_camera_case(sm.camera_case(name), False)


@pytest.mark.parametrize("name", [n for n in sm.CAMERA_CASE_NAMES if sm.camera_case(n)["program"] in sm.SUBSTITUTED])
def test_camera_kernels_of_the_substituted_program_against_the_float64_model(name):
    assert_camera_case(sm.camera_case(name), True)


def assert_ray_case(c, substituted):
    p, cfg = device_program(c["program"], substituted)
    yard, yard_err, yard_inv, kind = sm.yardstick_rays(c)
    m = sm.ray_model(c)["rays"]
    linear, tiled = init_rays(p, cfg, c, 0), init_rays(p, cfg, c, 1)
    assert linear.tobytes() == tiled.tobytes(), "a pixel's record differs between reference slot order and tile order"
    n, w = c["width"] * c["height"], c["width"]
    assert (linear["sx"] == np.arange(n) % w).all() and (linear["sy"] == np.arange(n) // w).all()
    assert (linear["terminated"] == 0).all() and (linear["running_dlambda_dnew"] == 1).all()
    for f in sm.RAY_FIELDS:
        assert_same_finite_pattern(c["name"], f, linear[f], yard[f], m[f])
    err = sm.ray_errors(c, linear)
    program = "substituted" if substituted else "dynamic"
    print(f"{c['name']} [{program}]: rays: gpu {_worst(err):.2e} yardstick ({kind}) {_worst(yard_err):.2e}")
    sm.assert_within(c["name"], "rays", sm.RAY_FLOOR, err, yard_err)
    inv = sm.frame_invariants(c, linear)
    for j, what in enumerate(("null", "ku_uobsu", "spatial length", "initial_quat")):
        if np.isnan(inv[:, j]).all():
            continue
        print(f"{c['name']} [{program}]: {what}: gpu {_worst(inv[:, j]):.2e} yardstick {_worst(yard_inv[:, j]):.2e}")
        sm.assert_within(c["name"], what, sm.RAY_FLOOR, inv[:, j], yard_inv[:, j])


@pytest.mark.parametrize("name", [c["name"] for c in sm.ray_cases()])
def test_gr_init_rays_generic_against_the_float64_model(name):
    assert_ray_case(sm.ray_case(name), False)


@pytest.mark.parametrize("name", [c["name"] for c in sm.ray_cases() if c["substituted"]])
def test_gr_init_rays_generic_of_the_substituted_program_against_the_float64_model(name):
    assert_ray_case(sm.ray_case(name), True)


def test_lanes_are_independent():
    """pose i of a 70-pose launch equals the same pose launched alone, bit for bit: lanes 0, 63, 64 (the second wave's first) and 69.
    Every pose is given the same speed, so that gr_init_basis_vectors too (its speed is a scalar argument) takes all 70 in one launch."""
    c = sm.camera_case("ordinary_kerr_boyer")
    assert c["count"] == 70
    p, cfg = device_program(c["program"])
    m = sm.camera_model(c)
    speeds = np.tile(np.array([0.3, -0.2, 0.4], dtype=np.float32), (70, 1))
    assert len(np.unique(speeds, axis=0)) == 1
    whole = dict(camera=cart_to_generic(p, cfg, c["cart"], c["flip"]), tetrad=init_basis_vectors(p, cfg, m["generic32"], speeds),
                 reboosted=boost_tetrad(p, cfg, m["generic32"], speeds, m["unboosted32"]),
                 inertial=init_inertial_ray(p, cfg, m["generic32"], m["tetrad32"], speeds))
    assert len(np.unique(whole["tetrad"].reshape(70, 16), axis=0)) == 35      # (the case holds every pose twice)
    for i in (0, 63, 64, 69):
        one = slice(i, i + 1)
        assert cart_to_generic(p, cfg, c["cart"][one], c["flip"]).tobytes() == whole["camera"][one].tobytes(), i
        assert init_basis_vectors(p, cfg, m["generic32"][one], speeds[one]).tobytes() == whole["tetrad"][one].tobytes(), i
        assert boost_tetrad(p, cfg, m["generic32"][one], speeds[one], m["unboosted32"][one]).tobytes() == whole["reboosted"][one].tobytes(), i
        alone = init_inertial_ray(p, cfg, m["generic32"][one], m["tetrad32"][one], speeds[one])
        assert alone.tobytes() == whole["inertial"][one].tobytes(), i


def test_degenerate_cameras_leave_their_neighbours_alone():
    """the degenerate case is one launch of 64 per kernel (one common speed): the poses next to a NaN or Inf camera are the bits of the
    same poses launched without the degenerate ones"""
    c = sm.camera_case("degenerate_kerr_boyer")
    assert len(np.unique(c["speeds"], axis=0)) == 1 and c["count"] == 64
    p, cfg = device_program(c["program"])
    m, whole = sm.camera_model(c), run_camera_case(c)
    good = np.array([not t["degenerate"] for t in m["trace"]])
    assert (~good).sum() == 3 and not good[63] and good[62]
    assert cart_to_generic(p, cfg, c["cart"][good], c["flip"]).tobytes() == whole["camera"][good].tobytes()
    assert init_basis_vectors(p, cfg, m["generic32"][good], c["speeds"][good]).tobytes() == whole["tetrad"][good].tobytes()
    assert boost_tetrad(p, cfg, m["generic32"][good], c["speeds"][good], m["unboosted32"][good]).tobytes() == whole["reboosted"][good].tobytes()


@pytest.mark.parametrize("name", [n for n in sm.CAMERA_CASE_NAMES if n.startswith("ordinary")])
def test_gr_camera_setup_stores_what_the_two_launchers_store(name):
    """the frame driver's one-launch form: a 16 x 8 frame through RenderState at the case's second pose (a moving observer), then
    BUF_CAMERA_GENERIC and BUF_TETRAD0..3 against gr_cart_to_generic followed by gr_init_basis_vectors - the same functions in the same
    IEEE module: bit-identical"""
    c = sm.camera_case(name)
    prog = sm.program(c["program"])
    p, cfg = device_program(c["program"])
    i = 1
    camera = gra.default_camera(position=[float(v) for v in c["cart"][i]], quat=[0.0, 0.0, 0.0, 1.0])
    camera.basis_speed = (ctypes.c_float * 3)(*[float(v) for v in c["speeds"][i]])
    camera.flip = c["flip"]
    state = gra.RenderState(16, 8, 0)
    state.render(p, prog.metric, camera, None, None, prog.metric.features(adaptive_sampling=0), prog.cfg or None,
                 gra.frame_options(mode=gra.MODE_FUSED, use_prepass=0))
    state.synchronize()
    read = lambda which: download(0, state.buffer(which), np.float32, 4)
    generic = cart_to_generic(p, cfg, c["cart"][i:i + 1], c["flip"])
    tetrad = init_basis_vectors(p, cfg, generic, c["speeds"][i:i + 1])
    assert np.abs(c["speeds"][i]).max() > 0
    assert read(gra.BUF_CAMERA_GENERIC).tobytes() == generic[0].tobytes()
    for a, which in enumerate((gra.BUF_TETRAD0, gra.BUF_TETRAD1, gra.BUF_TETRAD2, gra.BUF_TETRAD3)):
        assert read(which).tobytes() == tetrad[0, a].tobytes(), (name, a)
