"""What a fused frame decides (csrc/frame_plan.cpp: frame_plan::plan_fused), checked without a GPU: tests/frame_plan_check.cpp is compiled
together with frame_plan.cpp - host compiler, AddressSanitizer and UBSan, no HIP - and run as a program of its own; it prints one line per
row of the table below.  The expectations were derived by reading gr_render_frame's decisions as they stood before they moved into
frame_plan.cpp (one function, csrc/frame.cpp), not from what the new code prints.

Common to all rows unless a row says otherwise: 256 x 256 (prepass grid 16 x 16), fused mode, prepass on, Cartesian camera, not
prefetched, default tuning, no environment switch set, device idle, enough wave slots and a large enough tile order buffer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "frame_plan_check.cpp"), os.path.join(ROOT, "geodesic_raytracing_amd", "csrc", "frame_plan.cpp")]

# row 2 before any history was recorded: a program without the pair kernel records, traces its prepass in the trace launch, follows nothing
BASE = dict(rays_per_lane=1, keep_lanes=0, history_wanted=1, guesses_wanted=0, asked=1, record_history=1, invalidate=0, order_capable=0,
            inline_prepass=1, order_tiles=0, history_order=0, shape="{256,0,1}", history="256x256", margin=0)
INVALID = "refused=INVALID_ARGUMENT asked=1 "   # (the idle question is asked before anything is refused, and these frames want a history)


def plan(**changes):
    return " ".join(f"{k}={v}" for k, v in dict(BASE, **changes).items())


EXPECTED = {
    # a program WITH gr_trace_pair resolves rays_per_lane to 2: no history is recorded (what is there goes stale), the prepass stays in front
    "1 pair": plan(rays_per_lane=2, record_history=0, invalidate=1, inline_prepass=0),
    "2 no pair, no history yet": plan(),
    "2 no pair, history": plan(history_order=1),   # costs of shape {256, 0, 1} from the same camera
    "3 busy": plan(record_history=0, invalidate=1),   # an earlier frame of another stream still runs: inline_prepass all the same
    # strip_count 2, rank 1, block_rows 16: no history and nobody asked; the prepass in front, its costs order the tiles
    "4 share": plan(history_wanted=0, asked=0, record_history=0, order_capable=1, inline_prepass=0, order_tiles=1, shape="{16,1,2}"),
    # adaptive: rays_per_lane is 2 all the same, although neither launch of an adaptive frame is the pair kernel's
    "5 pair, adaptive": plan(rays_per_lane=2, guesses_wanted=1, record_history=0, invalidate=1, inline_prepass=0, shape="{-128,0,1}",
                             history="128x128", margin=2),
    "6 no pair, adaptive": plan(guesses_wanted=1, shape="{-128,0,1}", history="128x128", margin=2),   # the history of the 128 x 128 lattice
    "7 tile_history=0": plan(history_wanted=0, asked=0, record_history=0),
    # the camera turned about z: 48.64 px is more than the 48 px of motion, but a turn of up to 64 px with both origins on screen is followed
    # (the two figures: gr_picture_motion of the commit before for these cameras, 90 degrees, 256 wide)
    "8 motion": ["48.6399994", "65.2799988"],
    "8 turned 48.64 px": plan(history_order=1),
    "8 turned 65.28 px": plan(history_order=0),
    "9 adaptive, ray_compaction": INVALID + '"ray_compaction > 0 with adaptive sampling: gr_trace_compact traces every pixel (switch one of them off)"',
    "9 adaptive, rays_per_lane=2": INVALID + '"rays_per_lane = 2 with adaptive sampling: gr_trace_pair traces every pixel (switch one of them off)"',
    "9 adaptive, fused_shading": INVALID + '"fused_shading = 1 needs one ray per lane, no compaction and no adaptive sampling"',
    "9 rays_per_lane=2, no pair": INVALID + '"rays_per_lane = 2: this program has no gr_trace_pair kernel"',
    "10 prefetched": plan(inline_prepass=0),
    "11 no prepass": plan(inline_prepass=0),
    "12 width 8": plan(inline_prepass=0, history="8x256"),   # (a prepass grid below 1 x 1: the caller has cleared use_prepass)
    "13 small order buffer": plan(history_wanted=0, asked=0, record_history=0),
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_check")
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
