"""GPU tests (-m gpu) of every consumer of the prepass grid against the exact integer model of tests/prepass_model.py, on grids made
by hand: gr_init_rays_generic's chain of early_terminate calls, trace_tile's early_terminate_stencil and (with the cells traced by the
same launch) early_terminate_stencil_when_known, prepass_skips_pixel of the pair and the compaction kernel, tile_cost_class with the
promise trace_fused_body takes from it, and cell_row_matters.

The built-in Minkowski program carries the hand-made grids: every ray ends after a handful of steps, so a record is terminated == 2
exactly where the device skipped the pixel and 1 elsewhere.  The two tests that need real verdicts take them from the built-in Kerr
program at the default camera (and the cell-row test from the built-in Schwarzschild program too, whose verdicts are all 0: its rays
into the hole end at the singular terminator r = 1.05, so nothing of that frame is ever in shadow).  Every assertion is an equality
of integers or bytes: no tolerance, no mask, no pixel set aside.
Every output sits between eight records of guard bytes, and starts as guard bytes, so a record that is still guard bytes was not
written.  No grid holds a negative value: -1 is GR_CELL_UNKNOWN, which a launch with cells in flight waits on."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import prepass_model as pm  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, LIGHTRAY_DTYPE, RENDER_DATA_DTYPE  # noqa: E402

GUARD = 8                 # records either side of every output
GUARD_BYTE = 0xA5
LIST_BY_PREPASS = 0x50524550   # the word behind gr_order_tiles' list: its last class is a promise
_shared = {}
SHAPE_IDS = [f"{w}x{h}" for w, h in pm.SHAPES]


class Guarded:
    """a device array of `count` records of `size` bytes between guard records; the records start as guard bytes too, or as `initial`"""

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
    return DeviceBuffer.from_numpy(0, np.ascontiguousarray(a))


class Scene:
    """a built-in metric's dynamic program with the default camera's coordinates, tetrad, parameters and features on the device (a
    16 x 8 frame is rendered once to fill a render state's buffers: none of them depends on the frame's size)"""

    def __init__(self, name):
        self.metric = gra.Metric(name)
        self.program = gra.Program(self.metric.argument_string(), 0)
        self.state = gra.RenderState(16, 8, 0)
        self.state.render(self.program, self.metric, gra.default_camera(), None, None, self.metric.features(adaptive_sampling=0),
                          self.metric.cfg_values() or None, gra.frame_options(mode=gra.MODE_FUSED, use_prepass=0))
        self.state.synchronize()
        b = self.state.buffer
        self.p = self.program.handle
        self.camera, self.quat = b(gra.BUF_CAMERA_GENERIC), b(gra.BUF_CAMERA_QUAT)
        self.tetrad = [b(gra.BUF_TETRAD0), b(gra.BUF_TETRAD1), b(gra.BUF_TETRAD2), b(gra.BUF_TETRAD3)]
        self.cfg, self.dfg = b(gra.BUF_CFG), b(gra.BUF_DFG)


def scene(name):
    if name not in _shared:
        _shared[name] = Scene(name)
    return _shared[name]


def minkowski():
    return scene("minkowski")


def kerr():
    return scene("kerr_boyer")


def grids_of(w, h):
    pw, ph = pm.grid_size(w, h)
    return [(name, pm.hand_made_grid(name, pw, ph)) for name in pm.GRID_NAMES]


def model_skips(name, term, w, h):
    """skips() of a hand-made grid, computed once per (grid, shape) and left unchanged"""
    key = ("skips", name, w, h)
    if key not in _shared:
        s = pm.skips(term, w, h, term.shape[1], term.shape[0])
        s.setflags(write=False)
        _shared[key] = s
    return _shared[key]


# ---- launches ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["fused", "pair", "compact 1", "compact 32", "lattice"]


def trace(sc, kind, w, h, term, block_rows=0, rank=0, count=1, **launch):
    """one trace launch over a frame whose records start as guard bytes -> records [h, w]"""
    ph, pw = term.shape
    records, d_term = Guarded(w * h, RENDER_DATA_DTYPE.itemsize), up(term.astype(np.int32))
    head = (sc.p, None, sc.camera, sc.quat, records.ptr, w, h, block_rows, rank, count, d_term.ptr, pw, ph, *sc.tetrad, sc.cfg, sc.dfg, None)
    if kind == "fused" and not launch:
        check(lib.gr_trace_fused(*head))
    elif kind == "pair":
        check(lib.gr_trace_pair(*head))
    elif kind.startswith("compact"):
        check(lib.gr_trace_compact(*head, int(kind.split()[1])))
    else:
        a = gra.TraceFusedArgs(camera_generic=sc.camera, camera_quat=sc.quat, render_data=records.ptr, width=w, height=h, block_rows=block_rows,
                               strip_rank=rank, strip_count=count, termination_buffer=d_term.ptr, prepass_width=pw, prepass_height=ph,
                               e0=sc.tetrad[0], e1=sc.tetrad[1], e2=sc.tetrad[2], e3=sc.tetrad[3], cfg=sc.cfg, dfg=sc.dfg,
                               lattice=2 if kind == "lattice" else 1, **launch)
        check(lib.gr_trace_fused_launch(sc.p, None, ctypes.byref(a)))
    check(lib.gr_device_synchronize(0))
    return records.read(RENDER_DATA_DTYPE, (h, w))


def unwritten(records):
    return (records.view(np.uint8).reshape(records.shape + (RENDER_DATA_DTYPE.itemsize,)) == GUARD_BYTE).all(axis=-1)


def assert_records(what, records, skipped, written):
    """the records of the pixels in `written` follow `skipped`, a skipped record is exactly the one trace_tile writes, and no other
    record was touched"""
    h, w = skipped.shape
    assert np.array_equal(unwritten(records), ~written), (what, "records written", np.argwhere(unwritten(records) == written)[:8].tolist())
    got = records["terminated"] == 2
    assert np.array_equal(got[written], skipped[written]), (what, "terminated == 2 where the model says otherwise (y, x)",
                                                            np.argwhere((got != skipped) & written)[:8].tolist())
    assert (records["terminated"][written & ~skipped] == 1).all(), what
    ys, xs = np.mgrid[0:h, 0:w]
    assert (records["sx"][written] == xs[written]).all() and (records["sy"][written] == ys[written]).all(), what
    s = records[written & skipped]
    assert (s["tex_coord"].view(np.uint32) == 0).all() and (s["z_shift"].view(np.uint32) == 0).all() and (s["side"] == 1).all(), what


def lattice_pixels(w, h):
    written = np.zeros((h, w), dtype=bool)
    written[0:2 * (h // 2):2, 0:2 * (w // 2):2] = True
    return written


def kernels_of(sc):
    return [k for k in KERNELS if k != "pair" or lib.gr_program_has_trace_pair(sc.p)]


# ---- 1. gr_init_rays_generic ----------------------------------------------------------------------------------------------------------
def init_rays(sc, w, h, term, tiled):
    ph, pw = term.shape
    slots = lib.gr_tiled_slot_count(w, h) if tiled else w * h
    rays, count = Guarded(slots, LIGHTRAY_DTYPE.itemsize), Guarded(1, 4, np.array([-7], dtype=np.int32))
    d_term = up(term.astype(np.int32))
    check(lib.gr_init_rays_generic(sc.p, None, sc.camera, sc.quat, rays.ptr, count.ptr, w, h, d_term.ptr, pw, ph, 0, *sc.tetrad, sc.cfg, sc.dfg, 0, tiled))
    check(lib.gr_device_synchronize(0))
    assert int(count.read(np.int32, (1,))[0]) == slots
    return rays.read(LIGHTRAY_DTYPE, (slots,))


def assert_init_rays(what, sc, w, h, term, skipped):
    linear = init_rays(sc, w, h, term, 0)
    n = np.arange(w * h)
    assert (linear["sx"] == n % w).all() and (linear["sy"] == n // w).all(), what
    assert np.array_equal(linear["terminated"], np.where(skipped.reshape(-1), 2, 0)), (what, "linear", np.argwhere((linear["terminated"] == 2).reshape(h, w) != skipped)[:8].tolist())
    tiled = init_rays(sc, w, h, term, 1)
    t = pm.device_tiles(w, h, 0, 0, 1)
    x, y, valid = t["x"].reshape(-1), t["y"].reshape(-1), t["valid"].reshape(-1)
    assert len(tiled) == len(x)
    assert np.array_equal(tiled["sx"], np.where(valid, x, -1)) and np.array_equal(tiled["sy"], np.where(valid, y, -1)), what
    want = np.full(len(x), 2)
    want[valid] = np.where(skipped[y[valid], x[valid]], 2, 0)
    assert np.array_equal(tiled["terminated"], want), (what, "tiled")


@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
def test_gr_init_rays_generic_follows_the_model(shape):
    w, h = shape
    sc = minkowski()
    skipped_anywhere = 0
    for name, term in grids_of(w, h):
        skipped = model_skips(name, term, w, h)
        assert_init_rays((shape, name), sc, w, h, term, skipped)
        skipped_anywhere += int(skipped.sum())
    print(f"{w}x{h}: {skipped_anywhere} skipped pixels over {len(pm.GRID_NAMES)} grids")
    assert (skipped_anywhere > 0) == (w >= 48 and h >= 48)   # a 1 x 1 grid: every cell touches the border


def test_a_grid_as_wide_as_the_frame_skips_nothing():
    """pw == w but ph != h: the reference's rule is `and`, so no consumer looks at the grid"""
    w = h = 48
    sc, term = minkowski(), np.ones((3, 48), dtype=np.int32)
    nothing = pm.skips(term, w, h, 48, 3)
    assert not nothing.any()
    assert_init_rays("degenerate", sc, w, h, term, nothing)
    for kind in kernels_of(sc):
        written = lattice_pixels(w, h) if kind == "lattice" else np.ones((h, w), dtype=bool)
        assert_records(("degenerate", kind), trace(sc, kind, w, h, term), nothing, written)


# ---- 2. the trace kernels on whole frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
def test_trace_kernels_follow_the_model(shape):
    """gr_trace_fused, gr_trace_pair, gr_trace_compact (keep_lanes 1 and 32) and the lattice launch (lattice = 2 without lattice_rays:
    the records of the even pixels, verdicts at full-frame coordinates)"""
    w, h = shape
    sc = minkowski()
    kinds = kernels_of(sc)
    print(f"{w}x{h}: kernels {kinds}")
    assert {"fused", "compact 1", "compact 32", "lattice"} <= set(kinds)
    everything, even = np.ones((h, w), dtype=bool), lattice_pixels(w, h)
    for name, term in grids_of(w, h):
        skipped = model_skips(name, term, w, h)
        for kind in kinds:
            assert_records((shape, name, kind), trace(sc, kind, w, h, term), skipped, even if kind == "lattice" else everything)


# ---- 3. split frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(100, 60), (121, 77)], ids=["100x60", "121x77"])
def test_split_frames_follow_the_model(shape):
    w, h = shape
    sc = minkowski()
    launches = 0
    for name, term in grids_of(w, h):
        skipped = model_skips(name, term, w, h)
        whole = trace(sc, "fused", w, h, term)
        assert_records((shape, name, "whole"), whole, skipped, np.ones((h, w), dtype=bool))
        for count in (2, 3):
            for block_rows in (8, 16):
                if pm.split_is_refused(h, block_rows, count):   # (the entry refuses it: the last row must not start a block)
                    continue
                union = np.zeros((h, w), dtype=bool)
                for rank in range(count):
                    mine = pm.device_pixels(w, h, block_rows, rank, count)
                    part = trace(sc, "fused", w, h, term, block_rows, rank, count)
                    assert_records((shape, name, block_rows, rank, count), part, skipped, mine)
                    assert part[mine].tobytes() == whole[mine].tobytes(), (shape, name, block_rows, rank, count)
                    union |= mine
                    launches += 1
                assert union.all()
    assert launches >= len(pm.GRID_NAMES) * 10


# ---- 4. gr_order_tiles ------------------------------------------------------------------------------------------------------------------
def order_tiles(sc, w, h, term, attempts, block_rows, rank, count):
    """-> (counts [16], the listed tiles, every tile's class)"""
    ph, pw = term.shape
    nbytes = lib.gr_tile_order_bytes(w, h, block_rows, rank, count)
    order, d_term, d_attempts = Guarded(nbytes // 4, 4), up(term.astype(np.int32)), up(attempts.astype(np.uint32))
    check(lib.gr_order_tiles(sc.p, None, d_term.ptr, d_attempts.ptr, pw, ph, w, h, block_rows, rank, count, order.ptr))
    check(lib.gr_device_synchronize(0))
    words = order.read(np.uint32, (nbytes // 4,))
    n = (nbytes // 4 - 32) // 2
    counts, cursors, listed, classes = words[:16], words[16:32], words[32:32 + n], words[32 + n:].copy()
    assert counts.sum() == n and (cursors == counts).all() and np.array_equal(np.sort(listed), np.arange(n, dtype=np.uint32))
    assert classes[0] == LIST_BY_PREPASS   # (where tile 0's class was: the list itself still shows that)
    classes[0] = np.searchsorted(np.cumsum(counts), int(np.flatnonzero(listed == 0)[0]), side="right")
    assert (np.diff(classes[listed].astype(np.int64)) >= 0).all() and np.array_equal(np.bincount(classes, minlength=16), counts)
    return counts, listed, classes.astype(np.int64), order


def assert_tile_classes(what, sc, w, h, term, skipped, attempts, block_rows, rank, count):
    _, _, classes, _ = order_tiles(sc, w, h, term, attempts, block_rows, rank, count)
    tiles = pm.device_tiles(w, h, block_rows, rank, count)
    promise, edge, empty = pm.tile_classes(term, tiles, w, h, term.shape[1], term.shape[0])
    assert len(classes) == tiles["count"]
    last = classes == pm.TILE_CLASSES - 1
    # safety first, by itself: a tile of the last class is written as skipped without a look-up
    for t in np.flatnonzero(last):
        v = tiles["valid"][t]
        assert skipped[tiles["y"][t][v], tiles["x"][t][v]].all(), (what, "a pixel of a last-class tile needs a ray", int(t))
    assert np.array_equal(last, promise | empty), (what, "last class", np.flatnonzero(last != (promise | empty))[:8].tolist())
    assert np.array_equal(classes == 0, edge), (what, "class 0", np.flatnonzero((classes == 0) != edge)[:8].tolist())
    return int(promise.sum()), int(edge.sum())


@pytest.mark.parametrize("shape", pm.SHAPES, ids=SHAPE_IDS)
def test_gr_order_tiles_promises_what_the_model_promises(shape):
    w, h = shape
    sc = minkowski()
    pw, ph = pm.grid_size(w, h)
    promised = edges = 0
    for i, (name, term) in enumerate(grids_of(w, h)):
        skipped = model_skips(name, term, w, h)
        attempts = np.random.default_rng(100 + i).integers(1, 20001, size=(ph, pw))
        splits = [(0, 0, 1)] + [(16, rank, 3) for rank in range(3) if lib.gr_strip_local_blocks(h, 16, rank, 3) > 0]
        for block_rows, rank, count in splits:
            a, b = assert_tile_classes((shape, name, block_rows, rank, count), sc, w, h, term, skipped, attempts, block_rows, rank, count)
            promised, edges = promised + a, edges + b
    print(f"{w}x{h}: {promised} promised tiles, {edges} edge tiles")
    assert edges > 0 and (promised > 0) == (pw >= 5 and ph >= 5)


# ---- 5. the promise is taken ------------------------------------------------------------------------------------------------------------
def compute_units():
    """torch.cuda.get_device_properties' figure, asked in a process of its own: a torch.cuda call in this one would bring up torch's copy
    of the HIP runtime beside the library's, and the GPU tests after it would find no device (tests/test_abi.py)"""
    ask = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    return int(subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", ask], capture_output=True, text=True, check=True).stdout.split()[-1])


def test_promised_tiles_are_written_without_a_look_up():
    """a persistent launch that follows gr_order_tiles' list hands the last class out in chunks and writes its pixels as skipped without
    reading the grid (trace_fused_body: known_skipped): with the grid swapped for zeros behind the list's back, exactly the promised
    tiles still come out skipped"""
    sc = minkowski()
    units = compute_units()
    w, h = 400, 240
    while -(-w // 8) * -(-h // 8) <= 4 * units:
        h += 8
    assert -(-w // 8) * -(-h // 8) > 4 * units   # more tiles than one wave per SIMD holds: the launch draws tickets
    pw, ph = pm.grid_size(w, h)
    rng = np.random.default_rng(5)
    grid = (rng.random((ph, pw)) < 0.5).astype(np.int32)
    grid[3:12, 8:17] = 1
    attempts = rng.integers(1, 20001, size=(ph, pw))
    skipped = pm.skips(grid, w, h, pw, ph)
    tiles = pm.device_tiles(w, h, 0, 0, 1)
    promise, _, empty = pm.tile_classes(grid, tiles, w, h, pw, ph)
    assert not empty.any() and promise.sum() >= 50 and (~promise).sum() >= 50
    counts, _, classes, order = order_tiles(sc, w, h, grid, attempts, 0, 0, 1)
    assert np.array_equal(classes == pm.TILE_CLASSES - 1, promise) and counts[15] == promise.sum()
    promised_pixels = np.zeros((h, w), dtype=bool)
    v = tiles["valid"] & promise[:, None]
    promised_pixels[tiles["y"][v], tiles["x"][v]] = True
    assert not (promised_pixels & ~skipped).any()
    everything = np.ones((h, w), dtype=bool)
    blind = trace(sc, "fused", w, h, np.zeros_like(grid), tile_order=order.ptr, waves_per_simd=1)
    assert_records("the list with a grid of zeros", blind, promised_pixels, everything)
    listed = trace(sc, "fused", w, h, grid, tile_order=order.ptr, waves_per_simd=1)
    plain = trace(sc, "fused", w, h, grid)
    assert_records("the list", listed, skipped, everything)
    assert listed.tobytes() == plain.tobytes()
    print(f"{w}x{h}, {units} compute units: {int(promise.sum())} of {tiles['count']} tiles promised, {int(skipped.sum())} pixels skipped")


# ---- 6. gr_prepass_fused_strips ---------------------------------------------------------------------------------------------------------
SENTINEL, ATTEMPTS_SENTINEL = 7, 0xdeadbeef


def prepass_strips(sc, pw, ph, image_height, block_rows, rank, count, margin):
    term = Guarded(pw * ph, 4, np.full(pw * ph, SENTINEL, dtype=np.int32))
    attempts = Guarded(pw * ph, 4, np.full(pw * ph, ATTEMPTS_SENTINEL, dtype=np.uint32))
    check(lib.gr_prepass_fused_strips(sc.p, None, sc.camera, sc.quat, term.ptr, pw, ph, *sc.tetrad, sc.cfg, sc.dfg, image_height, block_rows, rank,
                                      count, attempts.ptr, margin))
    check(lib.gr_device_synchronize(0))
    return term.read(np.int32, (ph, pw)), attempts.read(np.uint32, (ph, pw))


@pytest.mark.parametrize("program", ["schwarzschild", "kerr_boyer"])
@pytest.mark.parametrize("grid", [(8, 6, 96), (7, 4, 77), (7, 7, 115)], ids=["8x6 of 96 rows", "7x4 of 77 rows", "7x7 of 115 rows"])
def test_gr_prepass_fused_strips_traces_the_rows_of_the_rule(grid, program):
    """115 rows: over eight devices in blocks of 8 rows, three (device, cell row) pairs are kept only by the one row of slack below
    the rule's lower bound (cell_row_matters: `- 1`) - at 96 and 77 rows that slack decides nothing"""
    pw, ph, H = grid
    sc = scene(program)
    single, single_attempts = prepass_strips(sc, pw, ph, H, 8, 0, 1, 0)
    assert np.isin(single, (0, 1)).all() and (single_attempts != ATTEMPTS_SENTINEL).all()
    assert (single == 0).any() and (single == 1).any() == (program == "kerr_boyer")
    surplus = launches = 0
    for count in (2, 3, 8):
        for block_rows in (8, 16):
            for margin in (0, 2):
                for rank in range(count):
                    term, attempts = prepass_strips(sc, pw, ph, H, block_rows, rank, count, margin)
                    what = (grid, count, block_rows, margin, rank)
                    written = term != SENTINEL
                    rule = np.array([pm.cell_row_rule(cy, ph, H, block_rows, rank, count, margin) for cy in range(ph)])
                    assert np.array_equal(written, np.broadcast_to(rule[:, None], (ph, pw))), (what, written.all(axis=1).tolist(), rule.tolist())
                    assert np.array_equal(term[written], single[written]), what
                    need = pm.cell_rows_needed(ph, H, block_rows, rank, count, margin)
                    assert need <= set(np.flatnonzero(written.all(axis=1)).tolist()), (what, sorted(need))
                    assert np.array_equal(attempts != ATTEMPTS_SENTINEL, written), what
                    surplus += int(rule.sum()) - len(need)
                    launches += 1
    print(f"{pw}x{ph} cells, {H} rows: {launches} launches, {surplus} cell rows traced without need; single device: {int(single.sum())} cells in shadow")


# ---- 7. the prepass inside the launch ---------------------------------------------------------------------------------------------------
def test_tiles_that_wait_for_cells_in_flight_follow_the_model():
    """inline_prepass = 1: the cells are the launch's first tickets and the tiles read them with early_terminate_stencil_when_known.
    (The built-in Kerr program: the built-in Schwarzschild program's grid holds no 1 - see the head of this file - and this test
    needs both.)"""
    w, h = 264, 136
    pw, ph = pm.grid_size(w, h)
    sc = kerr()
    alone = Guarded(pw * ph, 4, np.full(pw * ph, SENTINEL, dtype=np.int32))
    check(lib.gr_prepass_fused(sc.p, None, sc.camera, sc.quat, alone.ptr, pw, ph, *sc.tetrad, sc.cfg, sc.dfg))
    check(lib.gr_device_synchronize(0))
    want = alone.read(np.int32, (ph, pw))
    assert (want == 0).any() and (want == 1).any() and np.isin(want, (0, 1)).all()
    records, term = Guarded(w * h, RENDER_DATA_DTYPE.itemsize), Guarded(pw * ph, 4, np.full(pw * ph, SENTINEL, dtype=np.int32))
    a = gra.TraceFusedArgs(camera_generic=sc.camera, camera_quat=sc.quat, render_data=records.ptr, width=w, height=h, block_rows=0, strip_rank=0,
                           strip_count=1, termination_buffer=term.ptr, prepass_width=pw, prepass_height=ph, e0=sc.tetrad[0], e1=sc.tetrad[1],
                           e2=sc.tetrad[2], e3=sc.tetrad[3], cfg=sc.cfg, dfg=sc.dfg, inline_prepass=1)
    check(lib.gr_trace_fused_launch(sc.p, None, ctypes.byref(a)))
    check(lib.gr_device_synchronize(0))
    got = term.read(np.int32, (ph, pw))
    assert np.array_equal(got, want)
    rec = records.read(RENDER_DATA_DTYPE, (h, w))
    skipped = pm.skips(got, w, h, pw, ph)
    assert not unwritten(rec).any()
    assert np.array_equal(rec["terminated"] == 2, skipped), np.argwhere((rec["terminated"] == 2) != skipped)[:8].tolist()
    s = rec[skipped]
    ys, xs = np.mgrid[0:h, 0:w]
    assert (s["sx"] == xs[skipped]).all() and (s["sy"] == ys[skipped]).all() and (s["side"] == 1).all()
    assert (s["tex_coord"].view(np.uint32) == 0).all() and (s["z_shift"].view(np.uint32) == 0).all()
    print(f"{w}x{h}: {int((want == 1).sum())} of {pw * ph} cells in shadow, {int(skipped.sum())} pixels skipped")
