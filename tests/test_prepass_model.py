"""The integer model of the prepass verdict (tests/prepass_model.py) against exact rational arithmetic, against the arguments the
device code rests on (a pixel's cell is at most one from its tile centre's: the promise of gr_order_tiles' last class; cell_row_matters
keeps every cell row a device reads) and against the reference's own frames.  No GPU; every assertion is an equality of integers."""
import json
import os

import numpy as np
import pytest

import prepass_model as pm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = range(16, 701)   # with pn = w // 16: every cell size from 16 to just below 32 pixels, grids of 1 to 43 cells


def test_cell_rule_is_the_rational_rule_off_the_ties():
    ties = 0
    for w in WIDTHS:
        pw = w // 16
        c = np.arange(w)
        tie = pm.is_tie(c, w, pw)
        got, want = pm.cell_of(c, w, pw), pm.cell_exact(c, w, pw)
        assert np.array_equal(got[~tie], want[~tie]), (w, c[~tie & (got != want)].tolist())
        # on a tie the fp32 product decides between the two cells either side, nothing else
        assert ((got[tie] == want[tie]) | (got[tie] == want[tie] - 1)).all(), w
        ties += int(tie.sum())
    print(f"cell rule: {ties} tie pixels over the widths {WIDTHS[0]} .. {WIDTHS[-1]}")
    assert ties > 0


def test_a_pixels_cell_is_at_most_one_from_its_tile_centres():
    """what the last class of gr_order_tiles promises rests on (tile_cost_class, trace.hip): the centre is the tile's pixel 4 of 8, or
    its pixel 0 where that one lies outside the image; the same along a halo piece would not hold, and is not claimed"""
    failing = []
    for n in WIDTHS:
        pn = n // 16
        c = np.arange(n)
        first = (c // 8) * 8
        centre = np.where(first + 4 < n, first + 4, first)
        if (np.abs(pm.cell_of(c, n, pn) - pm.cell_of(centre, n, pn)) > 1).any():
            failing.append(n)
    assert failing == []


def _splits(w, h):
    yield 0, 0, 1
    for count in (2, 3):
        for block_rows in (8, 16):
            if not pm.split_is_refused(h, block_rows, count):
                for rank in range(count):
                    yield block_rows, rank, count


@pytest.mark.parametrize("shape", pm.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pixel_of_a_promised_tile_is_skipped(shape):
    w, h = shape
    pw, ph = pm.grid_size(w, h)
    promised = 0
    grids = [pm.hand_made_grid(name, pw, ph) for name in pm.GRID_NAMES]
    rng = np.random.default_rng(w * 1000 + h)
    grids += [(rng.random((ph, pw)) < p).astype(np.int32) for p in (0.7, 0.9, 0.97) for _ in range(8)]
    for term in grids:
        skipped = pm.skips(term, w, h, pw, ph)
        for block_rows, rank, count in _splits(w, h):
            tiles = pm.device_tiles(w, h, block_rows, rank, count)
            promise, edge, empty = pm.tile_classes(term, tiles, w, h, pw, ph)
            assert not (promise & edge).any() and not (promise & empty).any() and not (promise & tiles["halo"]).any()
            for t in np.flatnonzero(promise):
                v = tiles["valid"][t]
                assert skipped[tiles["y"][t][v], tiles["x"][t][v]].all(), (shape, block_rows, rank, count, int(t))
                assert pm.tile_class_is_promise(term, int(t), tiles, w, h, pw, ph) and not pm.tile_class_is_edge(term, int(t), tiles, w, h, pw, ph)
            promised += int(promise.sum())
    print(f"{w}x{h}: {promised} promised tiles over {len(grids)} grids")
    if pw >= 5 and ph >= 5:
        assert promised > 0


@pytest.mark.parametrize("shape", pm.SHAPES + [(50, 30), (8, 8), (400, 240)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_tiles_deal_every_pixel_once(shape):
    """the whole frame: every pixel in exactly one tile; a split frame: every pixel in exactly one rank's blocks, and the row under a
    block a second time as that rank's halo row"""
    w, h = shape
    whole = pm.device_tiles(w, h, 0, 0, 1)
    assert whole["count"] == -(-w // 8) * -(-h // 8) and not whole["halo"].any()
    seen = np.zeros((h, w), dtype=np.int64)
    np.add.at(seen, (whole["y"][whole["valid"]], whole["x"][whole["valid"]]), 1)
    assert (seen == 1).all()
    for count in (2, 3):
        for block_rows in (8, 16):
            own, halo = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
            for rank in range(count):
                t = pm.device_tiles(w, h, block_rows, rank, count)
                blocks = pm.local_blocks(h, block_rows, rank, count)
                assert t["count"] == blocks * (-(-w // 8) * (block_rows // 8) + -(-w // 64))
                for which, into in ((~t["halo"], own), (t["halo"], halo)):
                    v = t["valid"] & which[:, None]
                    np.add.at(into, (t["y"][v], t["x"][v]), 1)
            assert (own == 1).all()
            rows_under_blocks = np.zeros(h, dtype=np.int64)
            rows_under_blocks[block_rows::block_rows] = 1
            assert (halo == rows_under_blocks[:, None]).all()


def test_cell_row_rule_keeps_every_row_a_device_reads():
    cells = missing = surplus = 0
    for H in (17, 33, 48, 50, 97, 100, 135, 200):
        ph = H // 16
        for block_rows in (8, 16, 48):
            if pm.split_is_refused(H, block_rows, 2):
                continue
            for count in (2, 3, 8):
                for margin in (0, 2):
                    for rank in range(count):
                        need = pm.cell_rows_needed(ph, H, block_rows, rank, count, margin)
                        kept = {cy for cy in range(ph) if pm.cell_row_rule(cy, ph, H, block_rows, rank, count, margin)}
                        assert need <= kept, (H, block_rows, count, margin, rank, sorted(need - kept))
                        cells += ph
                        missing += len(need - kept)
                        surplus += len(kept - need)
    print(f"cell-row rule: of {cells} cell rows, {missing} needed but not traced, {surplus} traced without need")
    assert missing == 0 and cells > 0
    assert all(pm.cell_row_rule(cy, 6, 96, 16, 0, 1, 0) for cy in range(6))   # one device: every row


@pytest.mark.parametrize("name", ["kerr_prepass", "kerr_schild_prepass"])
def test_model_on_the_references_own_frames(name):
    """skips() of the fixture's termination buffer against the terminated == 2 flags the reference's x86 build wrote, on every pixel
    that is not an exact tie (the set tests/test_gpu_parity.py::test_prepass_matches_reference checks); how the ties fell is printed:
    they are that build's, not a rule"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    w, h = meta["width"], meta["height"]
    pw, ph = w // 16, h // 16
    assert z["termination"].shape == (ph, pw)
    want = (z["rays_init"]["terminated"] == 2).reshape(h, w)
    got = pm.skips(z["termination"], w, h, pw, ph)
    tie = pm.is_tie(np.arange(w), w, pw)[None, :] | pm.is_tie(np.arange(h), h, ph)[:, None]
    assert np.array_equal(got[~tie], want[~tie])
    assert want.any() and (~want).any() and (~tie).mean() > 0.85
    print(f"{name}: {int(tie.sum())} tie pixels, the model agrees with the reference's build on {int((got == want)[tie].sum())} of them")
