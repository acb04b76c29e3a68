"""What a launch of the trace stage decides (csrc/trace_plan.cpp), checked without a GPU: tests/trace_plan_check.cpp is compiled
together with trace_plan.cpp only - host compiler, AddressSanitizer and UBSan, no HIP - and run as a program of its own with every
GR_* variable removed; it prints one or two lines per row of the table below.  The expectations were derived by reading trace_launch,
gr_trace_pending, gr_do_generic_rays_scheduled, gr_trace_compact and the nine strip normalisations as they stood in csrc/capi.cpp
before they moved, not from what the new code prints; the arithmetic is written out beside the rows.  The device of the rows has 256
compute units and holds 8 workgroups of 256 lanes of every trace kernel per unit: 2 048 workgroups, 8 192 waves.  What looked odd
while deriving them is kept and listed in DESIGN.md."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "trace_plan_check.cpp"), os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "trace_plan.cpp")]


def plan(kernel, grid, tiles, ticket=0, ticket_tiles=1, prepass=0, strips="64/0/1", word=0, resets="0/0/0"):
    return (f"{kernel} wg=256 grid={grid} tiles={tiles} ticket={ticket} ticket_tiles={ticket_tiles} prepass_tickets={prepass} strips={strips} "
            f"word={word} resets={resets} asked=1")


def refused(text):   # GR_ERROR_INVALID_ARGUMENT, and the device was not asked
    return f'refused asked=0 code=-1 "{text}"'


INLINE = ("inline_prepass: gr_trace_fused on every pixel of its rows (or the lattice launch of adaptive sampling), in image order or the order of "
          "gr_order_tiles_by_history (gr_order_tiles' needs the prepass first), with a prepass grid")
LATTICE = "lattice / pending_only: gr_trace_fused only"
PARKING_BUILD = "parking: the program was built without -DGR_PARKING in its argument string (gr_program_has_parking)"
PARKING_LAUNCH = "parking: gr_trace_fused on every pixel of its rows, one ray per lane, no in-tile shading"
PARKING_LOT = "parking: records and words (gr_parking_lot_bytes), 1 <= lanes <= 64, trips >= 1, 64 <= slots <= 2^24, groups >= 1"
NO_PAIR = "this program has no gr_trace_pair kernel (its expressions do not instantiate on pairs)"
STRIPS = "block_rows must be a positive multiple of 8 and 0 <= strip_rank < strip_count"
LAST_ROW = "the last image row must not start a block (its filter reads the row above)"
TOO_MANY = "too many tiles"
SHADING_BUILD = "in-tile shading: the program was built without -DGR_TILE_SHADING in its argument string"
SHADING_LAUNCH = "in-tile shading: gr_trace_fused on every pixel of an image whose sides are multiples of 8"
TILE_COST = "tile_cost: gr_trace_fused on every pixel of its rows, or the lattice launch of a whole frame"
THE_LOT = "shading out=0 probes=0 compact=0 lot=1/1/16/512/4096/100"   # its words: (16 + 100 groups) * 4 = 464 bytes
PREPASS = dict(ticket=1, prepass=6, resets="960/0/0")   # 3 x 2 cell waves of 8 x 8 cells; 20 * 12 * 4 bytes of verdicts; (64 + 6) * 64 / 256 -> 18

EXPECTED = {
    # ---- whole frames: 8 x 8 tiles, four tile-waves to a workgroup; by ticket only where the workgroups wanted exceed the 2 048 resident
    "64 x 64": plan("fused", 16, 64),
    "64 x 64, two rays per lane": plan("pair", 8, 64),           # a pair wave takes two tiles: 32 waves
    "64 x 64, lattice 2": plan("fused", 4, 16),                  # the half-resolution grid: 4 x 4 tiles
    "60 x 60": plan("fused", 16, 64),                            # the one block is 64 rows
    # 480 x 270 tiles, 32 400 workgroups wanted; 8 192 waves draw (129 600 + 8 191) / 8 192 = 16 tickets each: one tile a ticket
    "3840 x 2160": plan("fused", 2048, 129600, 1, 1, strips="2160/0/1"),
    # 256 workgroups, 1 024 waves, 127 tickets each: (127 + 31) / 32 = 4 tiles a ticket
    "3840 x 2160, waves_per_simd 1": plan("fused", 256, 129600, 1, 4, strips="2160/0/1"),
    "3840 x 2160, waves_per_simd 9": plan("fused", 2048, 129600, 1, 1, strips="2160/0/1"),   # outside 1..8: what fits
    # 64 workgroups, 256 waves, 507 tickets each: 16 tiles a ticket, capped at 8
    "3840 x 2160, 64 compute units, waves_per_simd 1": plan("fused", 64, 129600, 1, 8, strips="2160/0/1"),
    "64 x 64, tile_cost": plan("fused", 16, 64, resets="0/256/0"),
    "64 x 64, lattice 2, guessed": plan("fused", 4, 16, 1),      # pixels traced ahead need the ticket order whatever the size
    # ---- split frames: two blocks of 16 rows to either rank, each 8 x 2 tiles and one halo piece of 64 pixels
    "split, rank 0": plan("fused", 9, 34, strips="16/0/2"),
    "split, rank 1": plan("fused", 9, 34, strips="16/1/2"),
    "split, height 65": refused(LAST_ROW),
    "split, a rank without blocks": "nothing asked=0",
    "no width": "nothing asked=0",
    # ---- the prepass inside the launch: a ticket is drawn although everything fits
    "prepass 20 x 12": plan("fused", 18, 64, **PREPASS),
    "prepass 20 x 12, cell_rows": plan("fused", 17, 64, 1, prepass=4, resets="960/0/0"),   # 240 cells in waves of 64; (64 + 4) * 64 / 256 -> 17
    "prepass, history order": plan("fused", 18, 64, word=5 << 8, **PREPASS),
    "prepass, history order, parking": [plan("parking", 18, 64, ticket=1, prepass=6, resets="960/0/464"), THE_LOT],   # no speculative tiles with a lot
    "history order, no prepass": plan("fused", 16, 64),
    "prepass, history order, speculative_classes -1": plan("fused", 18, 64, **PREPASS),
    "prepass, history order, speculative_classes 3": plan("fused", 18, 64, word=3 << 8, **PREPASS),
    "prepass, history order, speculative_classes 20": plan("fused", 18, 64, word=14 << 8, **PREPASS),
    # ---- which kernel: parking, else pair (above), else the lattice launch that leaves its rays, else gr_trace_fused
    "kernel parking": [plan("parking", 16, 64, 1, resets="0/0/464"), THE_LOT],
    "kernel lattice with rays": plan("lattice", 4, 16),
    "kernel fused, shading": [plan("fused", 16, 64), "shading out=1 probes=7 compact=0 lot=0/0/0/0/0/0"],   # compact_out is a split frame's
    "kernel fused, shading, split": [plan("fused", 9, 34, strips="16/1/2"), "shading out=1 probes=7 compact=1 lot=0/0/0/0/0/0"],
    # ---- what is refused, in the order the launcher looked
    "refused 1, prepass with gr_order_tiles' list": refused(INLINE),
    "refused 1, prepass grid as wide as the image": refused(INLINE),
    "refused 2, lattice 0": refused(LATTICE),
    "refused 2, pending_only, two rays per lane": refused(LATTICE),
    "refused 3, parking without the kernel": refused(PARKING_BUILD),
    "refused 4, parking with shading": refused(PARKING_LAUNCH),
    "refused 5, a lot of 63 slots": refused(PARKING_LOT),
    "refused 6, no pair kernel": refused(NO_PAIR),
    "refused 7, block_rows 12": refused(STRIPS),
    "refused 7, rank 2 of 2": refused(STRIPS),
    "refused 7, no height": refused(STRIPS),
    "refused 8, the last row starts a block": refused(LAST_ROW),
    "refused 9, too many tiles": refused(TOO_MANY),              # 2^17 x 2^17 tiles
    "refused 10, shading without the build option": refused(SHADING_BUILD),
    "refused 11, shading, 60 x 64": refused(SHADING_LAUNCH),
    "refused 12, tile_cost, pending_only": refused(TILE_COST),
    "refused 12, tile_cost, lattice 2 of a split frame": refused(TILE_COST),
    "refused 13, the device does not answer": "refused asked=1 code=-4 no text",   # the callable's status, after everything else
    "two faults, 1 and 6": refused(INLINE),
    "two faults, 7 and 10": refused(STRIPS),
    "two faults, 10 and 12": refused(SHADING_BUILD),
    "an empty share with fault 10": "nothing asked=0",
    # ---- the strip rule: the whole frame's block is the height rounded up to 8 | 8 | the height
    "strips whole frame of 60 rows": "64/0/1 8/0/1 60/0/1",
    "strips count 0": "64/0/1 8/0/1 60/0/1",
    "strips 12 rows, rank 1 of 2": "12/1/2 12/1/2 12/1/2",       # a multiple of 8 is the traced launches' own condition
    "strips no rows to a block": "bad bad bad",
    "strips rank 2 of 2": "bad bad bad",
    "strips rank -1": "bad bad bad",
    "strips whole frame without rows": "bad 8/0/1 bad",
    # 64 x 64; 60 x 60; rank 1 of 2 in blocks of 16; 100 x 40 in blocks of 8, rank 2 of 3: one block of 13 tiles and 2 halo pieces; no width
    "device tiles": "64 64 34 15 0",
    # ---- 2 x 2, 64 x 64, 3840 x 2160 (and that with waves_per_simd 1): min(resident, worst case), at least 1
    "pending groups": "1 12 2048 256",       # three pixels of every lattice cell at worst: 3, 3 072, 6 220 800 entries in workgroups of 256
    "scheduled groups": "1 64 8192",         # one tile a workgroup of 64 lanes, 32 of them resident per unit
    "compact groups": "1 16 2048",           # four tiles a workgroup, at most 32 waves per unit: 256 * 32 * 64 / 256
    # ---- switches: unset; then by the table - unset, accepted, out of range
    "switches unset": "256 1 0 0 5 2 0",
    "GR_TRACE_BLOCK": "256 64 128 256 256 256 256",
    "GR_TRACE_PERSISTENT": "1 0 1 1 0 1",    # off only where the text begins with '0'
    "GR_TRACE_WAVES_PER_SIMD": "0 1 8 0 0",
    "GR_TICKET_TILES": "0 1 64 0 0",
    "GR_SPECULATIVE_CLASSES": "5 0 14 0 0",  # out of range is none, not the default (as found)
    "GR_TILE_HISTORY_REACH": "2 0 8 2 2",
    "GR_SCHEDULED_WAVES_PER_SIMD": "0 1 8 0 0",
    "switches set after their first reading": "256 1 0 16 5 2 0",   # only GR_TICKET_TILES is read again
    "3840 x 2160, GR_TICKET_TILES=16": plan("fused", 2048, 129600, 1, 16, strips="2160/0/1"),
    "64 x 64, GR_TICKET_TILES=16": plan("fused", 16, 64),        # no ticket, nothing to override
    "3840 x 2160, GR_TICKET_TILES=65": plan("fused", 2048, 129600, 1, 1, strips="2160/0/1"),
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    work = tmp_path_factory.mktemp("trace_plan")
    out = str(work / "trace_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer"] + SOURCES + ["-o", out])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GR_")}   # no switches set
    r = subprocess.run([out], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(": ")
        rows.setdefault(name, []).append(rest)
    return rows


def test_the_table_has_every_row_and_no_other(printed):
    assert sorted(printed) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_decision(printed, name):
    want = EXPECTED[name]
    print(name, printed[name])
    assert printed[name] == (want if isinstance(want, list) else [want])
