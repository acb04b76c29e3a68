"""GPU tests (-m gpu) of the render-data stage on rays made by hand: gr_calculate_render_data (kernels/trace.hip, make_render_data)
against the float64 model of tests/render_data_model.py, on the cases that module lists - the universe fix from an overshoot of
1e-6 to 1e4 radii behind polar, Cartesian and cylindrical charts, the singular-terminator fix of a traversable chart, the early
return, sky angles of several turns, both poles, both redshift paths either side of g_tt = -1e-5, degenerate rays, the clamp and
the reparameterisation's quotient, the three termination flags.

The rays sit in the middle of a larger device buffer, 64 poison rays (terminated, random positions, sx and sy inside the frame)
either side; the record buffer is filled with a marker and has guard bytes either side, and so has the record count.

Bounds, per case, on the records render_data_model.compared keeps (terminated, past the early return, safe): max
circ_diff(tex_coord) * max(sin theta, 1e-3) <= max(2e-6, 2 x the CPU restatement's own figure against the model on that case), max
|dz| / (1 + |z|) <= max(1e-4, 2 x the restatement's).  2e-6 and 1e-4 are the stage's tolerances (tests/test_gpu_parity.py); the factor
2 over the reference's fp32 error is the one tests/test_gpu_shading.py fixed for contraction, reassociation and hardware
transcendentals.  It was fixed before the first run on a device.  Flags, and the records that compute nothing, are exact on every
record; records set aside are finite and in range."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import render_data_model as rm  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from oracle.refpipe import LIGHTRAY_DTYPE, RENDER_DATA_DTYPE  # noqa: E402
from test_render_data_model import oracle_records, reference_object, restatement_figures  # noqa: E402

POISON = 64               # rays either side of the case's
GUARD = 256               # bytes either side of the records
GUARD_BYTE, MARKER_BYTE = 0x5C, 0xA5
_shared = {}


def device_program(name):
    if ("program", name) not in _shared:
        prog = rm.program(name)
        cfg = DeviceBuffer.from_numpy(0, np.array(prog.cfg or [0.0], dtype=np.float32))
        _shared[("program", name)] = (gra.Program(prog.argument_string, 0), cfg)
    return _shared[("program", name)]


def launch(program_name, rays, width, height, universe, count=None, poison_seed=1):
    """one launch of gr_calculate_render_data over `rays` -> (records [height * width] as they are afterwards, marker where nothing
    was stored; the record count as it is afterwards).  The guards are checked here."""
    prog, cfg = device_program(program_name)
    n, slots = len(rays), width * height
    rng = np.random.default_rng(poison_seed)
    host = np.zeros(n + 2 * POISON, dtype=LIGHTRAY_DTYPE)
    host["position"] = rng.uniform(2, 30, (n + 2 * POISON, 4))
    host["velocity"] = rng.normal(size=(n + 2 * POISON, 4))
    host["initial_quat"] = (0, 0, 0, 1)
    host["ku_uobsu"], host["running_dlambda_dnew"], host["terminated"] = 1, 1, 1
    host["sx"], host["sy"] = rng.integers(0, width, n + 2 * POISON), rng.integers(0, height, n + 2 * POISON)
    host[POISON:POISON + n] = rays
    d_rays = DeviceBuffer.from_numpy(0, host)
    raw = np.full(GUARD + 32 * slots + GUARD, GUARD_BYTE, dtype=np.uint8)
    raw[GUARD:GUARD + 32 * slots] = MARKER_BYTE
    d_records = DeviceBuffer.from_numpy(0, raw)
    d_count = DeviceBuffer.from_numpy(0, np.array([n if count is None else count], dtype=np.int32))
    d_rcount = DeviceBuffer.from_numpy(0, np.array([-7, -7, -7], dtype=np.int32))
    dfg = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(gra.default_features(universe_size=universe, redshift=1)), dtype=np.uint8))
    rays_at = ctypes.c_void_p(d_rays.ptr.value + POISON * LIGHTRAY_DTYPE.itemsize)
    records_at = ctypes.c_void_p(d_records.ptr.value + GUARD)
    rcount_at = ctypes.c_void_p(d_rcount.ptr.value + 4)
    check(lib.gr_calculate_render_data(prog.handle, None, rays_at, d_count.ptr, n, records_at, rcount_at, width, height, cfg.ptr, dfg.ptr))
    check(lib.gr_device_synchronize(0))
    back = d_records.to_numpy(np.uint8, (GUARD + 32 * slots + GUARD,))
    assert (back[:GUARD] == GUARD_BYTE).all() and (back[GUARD + 32 * slots:] == GUARD_BYTE).all(), "guard bytes around the records were written"
    rcount = d_rcount.to_numpy(np.int32, 3)
    assert rcount[0] == -7 and rcount[2] == -7, "the ints around the record count were written"
    assert d_rays.to_numpy(np.uint8, (host.nbytes,)).tobytes() == host.tobytes(), "the rays were written"
    return back[GUARD:GUARD + 32 * slots].copy().view(RENDER_DATA_DTYPE), int(rcount[1])


def fields(records):
    """the 28 bytes of a record's fields, per record (the struct's last four bytes are padding, which a store may or may not write)"""
    return np.ascontiguousarray(records).view(np.uint8).reshape(len(records), 32)[:, :28]


def is_marker(records):
    return (fields(records) == MARKER_BYTE).all(axis=1)


def computed(c):
    """gr_calculate_render_data's records of a case in ray order, once per case and not written to"""
    key = ("records", c["name"])
    if key not in _shared:
        records, rcount = launch(c["program"], c["rays"], c["width"], c["height"], c["universe"])
        assert rcount == c["width"] * c["height"]
        assert not is_marker(records).any()                       # sx, sy are a permutation of the frame: every record is stored
        again, _ = launch(c["program"], c["rays"], c["width"], c["height"], c["universe"], poison_seed=2)
        assert fields(again).tobytes() == fields(records).tobytes(), "the records depend on rays outside the list"
        got = rm.by_record(c, records)
        got.setflags(write=False)
        _shared[key] = got
    return _shared[key]


@pytest.mark.parametrize("name", rm.CASE_NAMES)
def test_gr_calculate_render_data_against_the_float64_model(name):
    c = rm.case(name)
    got = computed(c)
    rm.assert_flags(c, got)
    want_tex, want_z = restatement_figures(c)
    tex, z = rm.errors(c, got)
    bound_tex, bound_z = max(rm.TEX_FLOOR, 2 * want_tex), max(rm.Z_FLOOR, 2 * want_z)
    print(f"{name}: gpu tex {tex:.2e} z {z:.2e} (bounds {bound_tex:.1e} {bound_z:.1e}; restatement tex {want_tex:.2e} z {want_z:.2e})")
    assert tex <= bound_tex and z <= bound_z, (name, tex, z, bound_tex, bound_z)


@pytest.mark.parametrize("name", [n for n in rm.CASE_NAMES if rm.case(n)["program"] in rm.REFERENCE_TAGS])
def test_gr_calculate_render_data_against_the_reference_object(name):
    """the same rays through the reference's own calculate_render_data (x86-64 build), where it travelled: the stage's tolerances"""
    c = rm.case(name)
    if reference_object(c["program"]) is None:
        pytest.skip("the reference's object is only built where its sources are")
    got, want, sel = computed(c), oracle_records("reference", c), rm.compared(c)
    for f in ("terminated", "sx", "sy", "side"):
        assert (got[f] == want[f]).all(), f
    if not sel.any():
        assert (got["tex_coord"] == want["tex_coord"]).all() and (got["z_shift"] == want["z_shift"]).all()
        return
    e, _ = rm.model_of(c)
    dtex = (rm.circ_diff(got["tex_coord"][sel].astype(np.float64), want["tex_coord"][sel].astype(np.float64)) * rm.sin_weight(e)[sel, None]).max()
    dz = (np.abs(got["z_shift"][sel].astype(np.float64) - want["z_shift"][sel]) / (1 + np.abs(want["z_shift"][sel]))).max()
    print(f"{name}: gpu against the reference object tex {dtex:.2e} z {dz:.2e}")
    assert dtex <= rm.TEX_FLOOR and dz <= rm.Z_FLOOR


def edge_rays(width, height):
    rng = np.random.default_rng(1000 * width + height)
    n = width * height
    pos = np.stack([rng.uniform(-50, 0, n), rng.uniform(3, 40, n), np.arccos(rng.uniform(-0.95, 0.95, n)), rng.uniform(-3.1, 3.1, n)], axis=1)
    vel = np.stack([rng.uniform(-2, -0.5, n), rng.uniform(0.2, 1, n), rng.normal(size=n) / 100, rng.normal(size=n) / 100], axis=1)
    return rm.make_rays(rng, pos, vel, width=width, height=height)


@pytest.mark.parametrize("size", [(67, 3), (1, 1)])
def test_padding_slots_a_short_count_and_the_record_count(size):
    """the kernel's own edges: rays of the tiled layout's padding slots (sx = -1, sx = width, sy = height) store nothing, a count
    shorter than the list leaves the records of the rays behind it alone, the record count is width * height, and nothing but the
    rays of the list shows in the records"""
    w, h = size
    rays = edge_rays(w, h)
    n = len(rays)
    slot = rays["sy"].astype(np.int64) * w + rays["sx"]
    whole, rcount = launch("kerr_boyer", rays, w, h, rm.UNIVERSE)
    assert rcount == w * h and not is_marker(whole).any()
    assert (whole["sx"][slot] == rays["sx"]).all() and (whole["sy"][slot] == rays["sy"]).all() and (whole["terminated"] == 1).all()
    again, _ = launch("kerr_boyer", rays, w, h, rm.UNIVERSE, poison_seed=2)
    assert fields(again).tobytes() == fields(whole).tobytes()
    for k, (field, value) in enumerate((("sx", -1), ("sx", w), ("sy", h))):
        padded = rays.copy()
        i = (7 * k + 3) % n
        padded[field][i] = value
        got, rcount = launch("kerr_boyer", padded, w, h, rm.UNIVERSE)
        want = whole.copy()
        want.view(np.uint8).reshape(w * h, 32)[slot[i]] = MARKER_BYTE
        assert fields(got).tobytes() == fields(want).tobytes(), (field, value)
        assert rcount == w * h                      # (the ray of index 0 stores the count whether or not its slot is padding)
    count = 2 * n // 3
    got, rcount = launch("kerr_boyer", rays, w, h, rm.UNIVERSE, count=count)
    want = whole.copy()
    want.view(np.uint8).reshape(w * h, 32)[slot[count:]] = MARKER_BYTE
    assert fields(got).tobytes() == fields(want).tobytes()
    assert rcount == (w * h if count > 0 else -7)   # an empty list launches no ray that could store it
