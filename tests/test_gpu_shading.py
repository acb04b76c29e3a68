"""GPU tests (-m gpu) of the shading stage on records made by hand: gr_render (kernels/shading.hip) against the float64 model of
tests/shading_model.py, on the synthetic cases that module lists - white-noise skies of odd shapes, footprints from a hundredth of a
texel to past the coarsest level, every probe count from 1 to 16, both seams, exact coordinates, the shadow's edge, both skies, the
last column and row, frames without neighbours, redshifts from -0.999 to 1e4, a short record count.

The records sit in the middle of a larger device buffer, 64 poison records (terminated, random coordinates) either side; the frame is
filled with a marker and has guard floats either side.  Nothing outside the frame may be written and nothing outside the records may
show in it.

Bounds, per case, on the records tests/shading_model.safe_mask keeps: max |rgb error| <= max(2e-4, 2 x the CPU restatement's own max
error against the model on that case), RMSE <= max(1e-5, 2 x its RMSE).  2e-4 and 1e-5 are the render stage's tolerances
(tests/test_gpu_parity.py); the factor 2 over the reference's fp32 error allows for contraction, reassociation and the hardware
log2 / exp2 of the device build, which the restatement has none of.  It was fixed before the first run on a device.  The
restatement's figures are 1e-7 to 3e-6 (profiles/shading_synthetic.txt), so the floors are the bound in every case today.
Records set aside as unsafe: finite, in [0, 1], alpha as exact as everywhere."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import shading_model as sm  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from oracle.refpipe import RENDER_DATA_DTYPE  # noqa: E402
from test_shading_model import NO_NEIGHBOUR, SCRIPTS, oracle_frame, reference_object, restatement, shaded  # noqa: E402

POISON = 64               # records either side of the frame's
GUARD = 256               # floats either side of the frame
GUARD_VALUE = np.float32(12345.0)
MARKER = np.float32(-7.25)
_shared = {}


def kerr():
    """the dynamic program every test of this file shades with (render reads nothing of the metric)"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        cfg = DeviceBuffer.from_numpy(0, np.array(metric.cfg_values(a=0.45), dtype=np.float32))
        _shared["kerr"] = (gra.Program(metric.argument_string(), 0), cfg)
    return _shared["kerr"]


def device_sky(c):
    key = ("sky", c["sky1"].ctypes.data, c["sky2"].ctypes.data)
    if key not in _shared:
        _shared[key] = (DeviceBuffer.from_numpy(0, c["sky1"]), DeviceBuffer.from_numpy(0, c["sky2"]))
    return _shared[key]


def launch(c, kind="render", strips=None, compact=0, poison_seed=1):
    """one launch over the case's records -> the frame buffer as it is afterwards, [height * width][4] (the guards checked)"""
    prog, cfg = kerr()
    w, h, n = c["width"], c["height"], len(c["records"])
    rng = np.random.default_rng(poison_seed)
    host = np.zeros(n + 2 * POISON, dtype=RENDER_DATA_DTYPE)
    host["terminated"], host["side"] = 1, 1
    host["tex_coord"] = rng.random((n + 2 * POISON, 2), dtype=np.float32)
    host["sx"], host["sy"] = rng.integers(0, w, n + 2 * POISON), rng.integers(0, h, n + 2 * POISON)
    host[POISON:POISON + n] = c["records"]
    records = DeviceBuffer.from_numpy(0, host)
    frame = np.full(GUARD + 4 * n + GUARD, GUARD_VALUE, dtype=np.float32)
    frame[GUARD:GUARD + 4 * n] = MARKER
    out = DeviceBuffer.from_numpy(0, frame)
    records_at = ctypes.c_void_p(records.ptr.value + POISON * RENDER_DATA_DTYPE.itemsize)
    out_at = ctypes.c_void_p(out.ptr.value + GUARD * 4)
    sky1, sky2 = device_sky(c)
    bh, bw = c["sky1"].shape[1:3]
    dfg = DeviceBuffer.from_numpy(0, np.frombuffer(bytes(gra.default_features(**c["features"])), dtype=np.uint8))
    if kind == "render":
        count = DeviceBuffer.from_numpy(0, np.array([c["count"]], dtype=np.int32))
        check(lib.gr_render(prog.handle, None, records_at, count.ptr, n, out_at, sky1.ptr, sky2.ptr, bw, bh, c["levels"], w, h,
                            c["max_probes"], cfg.ptr, dfg.ptr))
    else:
        rank, ranks, block_rows = strips
        call = lib.gr_render_strips if kind == "strips" else lib.gr_render_seams
        check(call(prog.handle, None, records_at, out_at, sky1.ptr, sky2.ptr, bw, bh, c["levels"], w, h, block_rows, rank, ranks, compact,
                   c["max_probes"], cfg.ptr, dfg.ptr))
    check(lib.gr_device_synchronize(0))
    back = out.to_numpy(np.float32, (GUARD + 4 * n + GUARD,))
    assert (back[:GUARD] == GUARD_VALUE).all() and (back[GUARD + 4 * n:] == GUARD_VALUE).all(), "guard floats around the frame were written"
    return back[GUARD:GUARD + 4 * n].reshape(n, 4)


def rendered(c):
    """gr_render's frame of a case [height][width][4], once per case and not written to"""
    key = ("frame", c["name"])
    if key not in _shared:
        frame = launch(c).reshape(c["height"], c["width"], 4)
        frame.setflags(write=False)
        _shared[key] = frame
    return _shared[key]


def assert_against_model(c, got, want_max, want_rmse, who):
    e, safe, sel = shaded(c)
    mx, rm = sm.errors(got, c)
    bound_max, bound_rmse = max(2e-4, 2 * want_max), max(1e-5, 2 * want_rmse)
    print(f"{c['name']}: gpu max {mx:.2e} rmse {rm:.2e} (bounds {bound_max:.1e} {bound_rmse:.1e}; {who} max {want_max:.2e} rmse {want_rmse:.2e})")
    assert mx <= bound_max and rm <= bound_rmse, (c["name"], mx, rm, bound_max, bound_rmse)


@pytest.mark.parametrize("name", sm.case_names())
def test_gr_render_against_the_float64_model(name):
    c = sm.case(name)
    got = rendered(c)
    e, safe, sel = shaded(c)
    px = got[e["sy"], e["sx"]]                                                      # in record order
    behind = np.arange(len(px)) >= c["count"]
    assert (px[behind] == MARKER).all(), "a record behind the count was shaded"
    assert np.isfinite(px[~behind]).all()
    black = e["black"] & ~behind
    assert (px[black] == (0, 0, 0, 1)).all()                                        # terminated 0 and 2: exactly (0, 0, 0, 1)
    assert np.abs(px[sel, 3] - e["rgba"][sel, 3]).max() <= 1e-6                     # alpha: the sampled alpha of an opaque sky
    assert px[sel, :3].min() >= 0 and px[sel, :3].max() <= 1                        # unsafe records included
    # nothing of the poison shows: the same frame, bit for bit, over other poison (with the parent's indexing a frame one
    # pixel wide or high took its footprint from the poison record before it)
    again = launch(c, poison_seed=2).reshape(got.shape)
    assert again.tobytes() == got.tobytes(), "the frame depends on records outside it"
    want_max, want_rmse = sm.errors(oracle_frame(restatement(), c), c)
    assert_against_model(c, got, want_max, want_rmse, "restatement")


@pytest.mark.parametrize("name", [n for n in sm.case_names() if n not in NO_NEIGHBOUR])
def test_gr_render_against_the_reference_object(name):
    """the same records through the reference's own render (x86-64 build), where it travelled: the render stage's tolerances"""
    if reference_object() is None:
        pytest.skip("the reference's object is only built where its sources are")
    c = sm.case(name)
    e, safe, sel = shaded(c)
    keep = sel & safe
    d = (rendered(c).astype(np.float64) - oracle_frame(reference_object(), c))[e["sy"][keep], e["sx"][keep], :3]
    print(f"{name}: gpu against the reference object max {np.abs(d).max():.2e} rmse {np.sqrt((d ** 2).mean()):.2e}")
    assert np.abs(d).max() <= 2e-4 and np.sqrt((d ** 2).mean()) <= 1e-5


SHAPES = ["magnification_128x64", "last_column_and_row_16x8", "last_column_and_row_24x40"]   # 64 x 8, 16 x 8, 24 x 40


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("strips", [(0, 1, None), (1, 3, 8), (1, 2, 16)])
@pytest.mark.parametrize("name", SHAPES)
def test_strips_are_gr_renders_rows_bit_for_bit(name, strips, compact):
    """gr_render_strips: the row blocks of one rank (block-cyclic), in place or back to back; the marker everywhere else"""
    c = sm.case(name)
    w, h = c["width"], c["height"]
    rank, ranks, block_rows = strips[0], strips[1], strips[2] or h
    whole = rendered(c).reshape(h * w, 4)
    got = launch(c, "strips", (rank, ranks, block_rows), compact)
    want = np.full((h * w, 4), MARKER, dtype=np.float32)
    blocks = range(rank, (h + block_rows - 1) // block_rows, ranks)
    assert len(blocks) == lib.gr_strip_local_blocks(h, block_rows, rank, ranks)
    for i, b in enumerate(blocks):
        rows = slice(b * block_rows * w, min((b + 1) * block_rows, h) * w)
        at = i * block_rows * w if compact else rows.start
        want[at:at + (rows.stop - rows.start)] = whole[rows]
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", SHAPES)
def test_seams_are_the_last_column_and_row_of_every_tile(name):
    """gr_render_seams: exactly the pixels an in-tile shading launch leaves, with gr_render's values; the marker everywhere else"""
    c = sm.case(name)
    w, h = c["width"], c["height"]
    whole = rendered(c)
    got = launch(c, "seams", (0, 1, 0)).reshape(h, w, 4)
    yy, xx = np.mgrid[0:h, 0:w]
    seam = (xx % 8 == 7) | (yy % 8 == 7)
    want = np.where(seam[..., None], whole, MARKER).astype(np.float32)
    assert seam.any() and not seam.all() and got.tobytes() == want.tobytes()
