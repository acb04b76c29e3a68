"""The prepass verdict as an exact integer model (numpy only): which pixels of a frame get no ray, given the grid of 0 / 1 verdicts
of the low-resolution prepass, and which cells and tiles the consumers of that grid deal with.

The rule is init_rays_generic's (cl.cl:3213-3232): a pixel (cx, cy) of a w x h frame looks at the cell (lx, ly) =
(round(cx / w * pw), round(cy / h * ph)) of the pw x ph grid and is skipped when the five cells (lx, ly), (lx +- 1, ly), (lx, ly +- 1)
all lie inside the grid and all hold exactly 1 - and only when pw != w and ph != h.  The device states it six times
(kernels/setup.hip: early_terminate, early_terminate_stencil, early_terminate_stencil_when_known; kernels/trace.hip: prepass_skips_pixel,
tile_cost_class, cell_row_matters); tests/test_gpu_prepass.py holds every one of them to this module, tests/test_prepass_model.py holds
this module to exact rational arithmetic and to the reference's own frames."""
import numpy as np

TILE = 8               # GR_TILE: a tile-wave is 8 x 8 pixels
HALO_PIECE = 64        # ... or 64 pixels of the row under a block of a split frame
TILE_CLASSES = 16      # GR_TILE_CLASSES: gr_order_tiles' classes; the last one is the promise "no pixel of this tile needs a ray"


def cell_of(c, n, pn):
    """round_half_away(fl32(fl32(c / n) * fl32(pn))): the quotient rounded once from the exact value (exact_ratio, setup.hip: a
    double quotient of two ints below 2^24 rounds to the float the exact quotient rounds to), one IEEE fp32 multiply, roundf (exact).
    No special case for ties: the fp32 product decides them."""
    quotient = (np.asarray(c, dtype=np.float64) / np.float64(n)).astype(np.float32)
    product = (quotient * np.float32(pn)).astype(np.float32)
    return np.floor(product.astype(np.float64) + 0.5).astype(np.int64)   # the product is >= 0: half away from zero is half up


def cell_exact(c, n, pn):
    """floor(c * pn / n + 1/2) in integers: the rule without rounding errors"""
    c = np.asarray(c, dtype=np.int64)
    return (2 * c * pn + n) // (2 * n)


def is_tie(c, n, pn):
    """c * pn / n lies exactly half way between two cells"""
    c = np.asarray(c, dtype=np.int64)
    return (2 * c * pn) % (2 * n) == n


def _shadow(term, pw, ph, reach):
    """term == 1 inside the grid, false in a border of `reach` cells around it: [ph + 2 reach, pw + 2 reach]"""
    term = np.asarray(term).reshape(ph, pw)
    padded = np.zeros((ph + 2 * reach, pw + 2 * reach), dtype=bool)
    padded[reach:reach + ph, reach:reach + pw] = term == 1
    return padded


def skips(term, w, h, pw, ph):
    """bool [h, w]: the pixels that get no ray"""
    out = np.zeros((h, w), dtype=bool)
    if not (pw != w and ph != h):   # (the reference's rule: `and`)
        return out
    lx, ly = cell_of(np.arange(w), w, pw), cell_of(np.arange(h), h, ph)
    assert lx.min() >= 0 and lx.max() <= pw and ly.min() >= 0 and ly.max() <= ph
    s = _shadow(term, pw, ph, 2)
    x, y = lx[None, :] + 2, ly[:, None] + 2
    return s[y, x] & s[y, x - 1] & s[y, x + 1] & s[y - 1, x] & s[y + 1, x]


def whole_frame_block_rows(h):
    return ((h + TILE - 1) // TILE) * TILE


def local_blocks(h, block_rows, rank, count):
    """gr_strip_local_blocks"""
    total = (h + block_rows - 1) // block_rows
    return (total - rank + count - 1) // count if rank < total else 0


def device_tiles(w, h, block_rows, rank, count):
    """The tile-waves of a device's share, in the numbering of trace_tile / trace_slot_to_pixel (trace.hip): image rows are dealt in
    blocks of block_rows rows, block b to device b % count; a block is tiles_x * block_rows / 8 tiles of 8 x 8 pixels (lane l: pixel
    (l % 8, l / 8) of the tile) and, when the frame is split (count > 1), the row under the block in pieces of 64 pixels.  count <= 1:
    one block covering the frame.  Returns a dict of arrays over the tiles: x, y [tiles, 64], valid [tiles, 64] (the pixel lies in the
    image: tiles at the right and bottom edges are partial, or empty), halo [tiles]."""
    if count <= 1:
        count, rank, block_rows = 1, 0, whole_frame_block_rows(h)
    assert block_rows > 0 and block_rows % TILE == 0 and 0 <= rank < count
    tiles_x, tile_rows = (w + TILE - 1) // TILE, block_rows // TILE
    halo_waves = (w + HALO_PIECE - 1) // HALO_PIECE if count > 1 else 0
    per_block = tiles_x * tile_rows + halo_waves
    n = per_block * local_blocks(h, block_rows, rank, count)
    wave, lane = np.arange(n)[:, None], np.arange(64)[None, :]
    block, within = wave // per_block, wave % per_block
    r0 = (block * count + rank) * block_rows
    halo = within >= tiles_x * tile_rows
    x = np.where(halo, (within - tiles_x * tile_rows) * HALO_PIECE + lane, (within % tiles_x) * TILE + lane % TILE)
    y = np.where(halo, r0 + block_rows, r0 + (within // tiles_x) * TILE + lane // TILE)
    valid = (x < w) & (y < h)
    return dict(x=x, y=y, valid=valid, halo=np.broadcast_to(halo, (n, 1))[:, 0].copy(), count=n)


def device_pixels(w, h, block_rows, rank, count):
    """bool [h, w]: the pixels a device writes records of (its blocks' rows and the halo rows under them)"""
    t = device_tiles(w, h, block_rows, rank, count)
    out = np.zeros((h, w), dtype=bool)
    out[t["y"][t["valid"]], t["x"][t["valid"]]] = True
    return out


def _tile_cells(term, tiles, w, h, pw, ph):
    """per tile: (has a pixel, how many of the 5 x 5 cells around its centre's cell lie inside the grid and hold 1) - tile_cost_class:
    the centre is the tile's pixel 36 = (4, 4), or its pixel 0 where that one lies outside the image"""
    valid = tiles["valid"]
    lane = np.where(valid[:, 36], 36, 0)
    rows = np.arange(tiles["count"])
    has_pixel = valid[rows, lane]
    lx = cell_of(tiles["x"][rows, lane], w, pw) + 3
    ly = cell_of(tiles["y"][rows, lane], h, ph) + 3
    s = _shadow(term, pw, ph, 3)
    lx, ly = np.where(has_pixel, lx, 3), np.where(has_pixel, ly, 3)
    in_shadow = sum(s[ly + dy, lx + dx].astype(np.int64) for dy in range(-2, 3) for dx in range(-2, 3))
    return has_pixel, in_shadow


def tile_classes(term, tiles, w, h, pw, ph):
    """(promise, edge, empty), bool arrays over the tiles of device_tiles.  promise: the 25 cells are all inside the grid and all 1 and
    the tile is no halo piece - gr_order_tiles' last class, whose pixels trace_fused_body marks skipped without a look-up.  edge: some
    of the 25 cells are 1 but it is no promise - class 0.  empty: no pixel of the tile lies in the image (the bottom tile rows of a
    block that the image ends in) - filed in the last class too, there is nothing to trace and nothing is written."""
    has_pixel, in_shadow = _tile_cells(term, tiles, w, h, pw, ph)
    promise = has_pixel & (in_shadow == 25) & ~tiles["halo"]
    edge = has_pixel & (in_shadow > 0) & ~promise
    return promise, edge, ~has_pixel


def tile_class_is_promise(term, tile, tiles, w, h, pw, ph):
    return bool(tile_classes(term, tiles, w, h, pw, ph)[0][tile])


def tile_class_is_edge(term, tile, tiles, w, h, pw, ph):
    return bool(tile_classes(term, tiles, w, h, pw, ph)[1][tile])


def _c_div(a, b):
    """a / b of C: truncated towards zero (b > 0)"""
    return a // b if a >= 0 else -((-a) // b)


def cell_row_rule(cy, ph, H, block_rows, rank, count, margin):
    """cell_row_matters (trace.hip) with C integer semantics: does a device of a split frame trace the prepass cells of row cy?"""
    if count <= 1:
        return True
    lo = _c_div((2 * cy - 3) * H, 2 * ph) - 1 - margin
    hi = _c_div((2 * cy + 3) * H + 2 * ph - 1, 2 * ph) + 1 + margin
    lo, hi = max(lo, 0), min(hi, H - 1)
    b_lo, b_hi = max(_c_div(lo - 1, block_rows), 0), _c_div(hi, block_rows)
    first = b_lo + ((rank - b_lo) % count + count) % count      # (Python's % of a positive modulus is already non-negative)
    return first <= b_hi


def cell_rows_needed(ph, H, block_rows, rank, count, margin):
    """brute force: the cell rows that the stencils of the device's pixel rows read - the rows of its blocks, the halo row under each,
    and `margin` rows either side of those"""
    rows = set()
    for b in range(rank, (H + block_rows - 1) // block_rows, count):
        rows.update(y for y in range(b * block_rows - margin, min((b + 1) * block_rows, H - 1) + margin + 1) if 0 <= y < H)
    need = set()
    for y in rows:
        ly = int(cell_of(y, H, ph))
        need.update(c for c in (ly - 1, ly, ly + 1) if 0 <= c < ph)
    return need


def split_is_refused(h, block_rows, count):
    """the host's condition (plan_trace, csrc/trace_plan.cpp): the last image row must not start a block of a split frame"""
    return count > 1 and h > 1 and (h - 1) % block_rows == 0


# ---- the grids made by hand (tests/test_gpu_prepass.py; tests/test_prepass_model.py runs the promise on them) --------------------------
# w x h; the grid is w // 16 x h // 16 (frame.cpp).  656 is the smallest side at which roundf(p) and (int)(p + 0.5f) part: pixel 8 is a
# tie, fl32(8 / 656) * 41 is 0.5 - 5 * 2^-28 exactly, the fp32 product is the float below 0.5 and the cell is 0, while p + 0.5f rounds to 1
SHAPES = [(16, 16), (48, 48), (96, 54), (100, 60), (121, 77), (264, 136), (656, 48)]
GRID_NAMES = ["ones", "zeros", "one_zero", "plus", "checkerboard", "random_a", "random_b", "not_only_ones"]


def grid_size(w, h):
    return w // 16, h // 16


def hand_made_grid(name, pw, ph):
    """int32 [ph, pw]; never a negative value (-1 is GR_CELL_UNKNOWN: a launch whose cells are in flight waits on it)"""
    seed = GRID_NAMES.index(name) * 1000 + pw * 31 + ph
    rng = np.random.default_rng(seed)
    if name == "ones":
        g = np.ones((ph, pw), dtype=np.int32)
    elif name == "zeros":
        g = np.zeros((ph, pw), dtype=np.int32)
    elif name == "one_zero":
        g = np.ones((ph, pw), dtype=np.int32)
        g[ph // 2, pw // 2] = 0
    elif name == "plus":
        g = np.zeros((ph, pw), dtype=np.int32)
        if pw >= 3 and ph >= 3:
            cx, cy = max(1, min(pw - 2, pw // 2)), max(1, min(ph - 2, ph // 2))
            g[cy, cx - 1:cx + 2] = 1
            g[cy - 1:cy + 2, cx] = 1
    elif name == "checkerboard":
        g = ((np.arange(pw)[None, :] + np.arange(ph)[:, None]) % 2).astype(np.int32)
    elif name in ("random_a", "random_b"):
        g = (rng.random((ph, pw)) < 0.7).astype(np.int32)
    elif name == "not_only_ones":   # only exactly 1 is shadow
        g = np.ones(ph * pw, dtype=np.int32)
        other = rng.permutation(ph * pw)[:max(1, ph * pw // 4)]
        g[other] = np.array([2, 3, 0x101, 0x7fffffff], dtype=np.int32)[np.arange(len(other)) % 4]
        g = g.reshape(ph, pw)
    else:
        raise KeyError(name)
    assert g.min() >= 0
    return np.ascontiguousarray(g)
