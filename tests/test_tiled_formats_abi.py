"""CPU tests of split frames in either format (gr_render_frame_tiled_as, gr_tiled_exchange_as): what the headers declare and the library
exports, the refusals that come before any device call, and the transfer step of a float and of a byte frame driven over host memory
with a recording gr_transport - every rank of a world, every rotation, unequal shares with a short last block."""
import ctypes
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.distributed import StripPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, RGBA8 = 0, 1
WIDTH, HEIGHT, BLOCK = 40, 88, 16   # five blocks of 16 rows and one of 8


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def test_both_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    assert "gr_render_frame_tiled_as" in contract and "gr_render_frame_tiled_as" not in internal
    assert "gr_tiled_exchange_as" in internal and "gr_tiled_exchange_as" not in contract
    for name in ("gr_render_frame_tiled_as", "gr_tiled_exchange_as"):
        assert hasattr(gra.lib, name), name
        assert name in gra.EXPORTED_SYMBOLS, name
    public = open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()
    assert re.search(r"^enum \{ GR_FRAME_F32 = 0, GR_FRAME_RGBA8 = 1 \};$", public, flags=re.M)
    assert (gra.FRAME_F32, gra.FRAME_RGBA8) == (F32, RGBA8)
    # the format is an argument: the old entry point's arguments and one more, nothing new in the options
    old, new = gra.lib.gr_render_frame_tiled.argtypes, gra.lib.gr_render_frame_tiled_as.argtypes
    assert list(new[:-1]) == list(old) and new[-1] is ctypes.c_int
    body = public[public.index("typedef struct gr_frame_options {"):public.index("} gr_frame_options;")]
    assert "format" not in body and len(re.findall(r"^\s{4}[a-z].*?;", body, flags=re.M)) <= 15
    assert len(public.splitlines()) <= 350 and len(contract) <= 80
    assert hasattr(gra.TiledFrame, "render_as")


class _Nobody:
    """a transport nobody may call: the refusals below come first"""

    def __init__(self):
        T = gra.Transport

        def never(*_):
            raise AssertionError("the transport was called")

        self.keep = (T.GROUP(never), T.GROUP(never), T.SEND(never), T.RECV(never))
        self.table = T(None, *self.keep)


def participant(world, rank, transport, width=WIDTH, height=HEIGHT, block=BLOCK):
    """a participant without a device (the schedule tests' kind): everything up to the first device call works on it"""
    h = ctypes.c_void_p()
    gra.check(gra.lib.gr_tiled_create_custom(world, rank, -1, ctypes.byref(transport), width, height, block, ctypes.byref(h)))
    return h


def frame_as(part, state, frame, fmt, program=4096, metric=4096):
    """gr_render_frame_tiled_as with stand-in handles that a call refused on the host never dereferences"""
    cam, feats = gra.default_camera(), gra.default_features()
    v = ctypes.c_void_p
    return gra.lib.gr_render_frame_tiled_as(part, v(state) if state else None, v(program), v(metric), None, ctypes.byref(cam), ctypes.byref(feats), None, 0,
                                            None, None, 0, 0, 0, frame, None, 0, fmt), (gra.lib.gr_last_error() or b"").decode()


def test_refusals_that_come_before_any_device_call():
    """(this box has no GPU and none of the answers is GR_ERROR_DEVICE.  The two refusals that read a render state - its output size, and
    block_rows x factor beyond an int - need a state, which needs a device: tests/test_gpu_tiled_formats.py holds them)"""
    nobody = _Nobody()
    root, other = participant(2, 0, nobody.table), participant(2, 1, nobody.table)
    frame = ctypes.c_void_p(1 << 20)   # never dereferenced
    try:
        for fmt in (2, -1, 7):
            rc, text = frame_as(root, None, frame, fmt)
            assert rc == -1 and "format" in text and str(fmt) in text and "GR_FRAME_RGBA8" in text, text
            assert gra.lib.gr_tiled_exchange_as(root, None, frame, 0, None, fmt) == -1
            assert b"format" in gra.lib.gr_last_error() and str(fmt).encode() in gra.lib.gr_last_error()
        for fmt in (F32, RGBA8):
            rc, text = frame_as(root, 4096, None, fmt)
            assert rc == -1 and "root needs the frame" in text, text
            rc, text = frame_as(other, None, None, fmt)          # elsewhere the frame may be NULL; the state may not
            assert rc == -1 and "null argument" in text, text
            rc, text = frame_as(None, 4096, frame, fmt)
            assert rc == -1 and "null argument" in text, text
            # a participant without a device is refused as gr_render_frame_tiled refuses it
            rc, text = frame_as(root, 4096, frame, fmt)
            assert rc == -1 and "without a device" in text, text
            rc, text = frame_as(other, 4096, None, fmt)
            assert rc == -1 and "without a device" in text, text
    finally:
        gra.lib.gr_tiled_destroy(root)
        gra.lib.gr_tiled_destroy(other)


def test_the_cli_refuses_adaptive_sampling_on_a_split_frame(capsys):
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--devices", "0,0", "--adaptive", "--out", "x.png"])
    assert e.value.code == 2 and "--adaptive" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--devices", "0,x", "--out", "x.png"])
    assert e.value.code == 2 and "--devices" in capsys.readouterr().err
    assert not os.path.exists("x.png")
    assert render.split_block_rows(48) == 16 and render.split_block_rows(33) == 24 and render.split_block_rows(1) == 16


class _Mailbox:
    """A recording point-to-point transport on host memory (gr_transport, GR_TRANSPORT_CUSTOM): every rank's calls are logged with the
    address they were given; sends and receives between two ranks are matched in issue order - NCCL's rule - once every rank has issued
    its frame, and the words are then moved."""

    def __init__(self):
        self.sends, self.recvs, self.log, self.keep = {}, {}, [], []

    def table(self, rank):
        T = gra.Transport

        def begin(_):
            self.log.append((rank, "begin"))
            return 0

        def end(_):
            self.log.append((rank, "end"))
            return 0

        def send(_, data, words, peer, stream):
            self.log.append((rank, "send", peer, words, stream, data))
            self.sends.setdefault((rank, peer), []).append(ctypes.string_at(data, words * 4))
            return 0

        def recv(_, data, words, peer, stream):
            self.log.append((rank, "recv", peer, words, stream, data))
            self.recvs.setdefault((peer, rank), []).append((data, words))
            return 0

        t = T(None, T.GROUP(begin), T.GROUP(end), T.SEND(send), T.RECV(recv))
        self.keep.append((t, begin, end, send, recv))
        return t

    def deliver(self):
        assert set(self.sends) == set(self.recvs)
        for pair, sent in self.sends.items():
            want = self.recvs[pair]
            assert len(sent) == len(want), pair
            for payload, (dst, words) in zip(sent, want):
                assert len(payload) == words * 4, pair   # a size mismatch hangs or corrupts with the real library
                ctypes.memmove(dst, payload, len(payload))
        self.sends.clear()
        self.recvs.clear()


def exchange(world, rotation, fmt, entry):
    """one frame of `fmt` cut into the shares of `rotation`, staged as each participant's render would leave it, exchanged through
    `entry` (gr_tiled_exchange_as, or gr_tiled_exchange for the float frame) and delivered; returns the calls that were recorded, with
    addresses as offsets into the caller's staging (sends) or frame (receives)"""
    pixel_bytes = 16 if fmt == F32 else 4
    row_bytes = WIDTH * pixel_bytes
    plan = StripPlan(HEIGHT, world, BLOCK)
    assert [b - a for a, b in plan.blocks_of((HEIGHT // BLOCK) % world)][-1] == 8   # somebody's last local block is the short one
    assert len({sum(b - a for a, b in plan.blocks_of(s)) for s in range(world)}) == 2                  # and the shares are unequal
    box = _Mailbox()
    parts = [participant(world, r, box.table(r)) for r in range(world)]
    rng = np.random.default_rng(1000 * world + 10 * rotation + fmt)
    truth = rng.integers(0, 256, size=(HEIGHT, row_bytes), dtype=np.uint8)   # every byte pattern, NaNs and all: the step moves bytes
    assembled = np.full((HEIGHT, row_bytes), 0xA5, np.uint8)
    stream = ctypes.c_void_p(0x2000 + rotation)
    staging, calls = {}, []
    try:
        for r in range(world):
            assert gra.lib.gr_tiled_staging_bytes(parts[r]) == plan.blocks_per_rank * BLOCK * WIDTH * 16   # the ring is sized for float rows
            share = gra.lib.gr_tiled_share(parts[r], rotation)
            assert share == (r + rotation) % world
            args = (rotation, stream) if entry is gra.lib.gr_tiled_exchange else (rotation, stream, fmt)
            if r == 0:   # the root renders its own share in place
                for a, b in plan.blocks_of(share):
                    assembled[a:b] = truth[a:b]
                gra.check(entry(parts[r], None, assembled.ctypes.data, *args))
            else:        # compact rows, block i at i * block_rows * row_bytes: a byte frame fills the first quarter of the slot
                buf = np.full(gra.lib.gr_tiled_staging_bytes(parts[r]), 0x5A, np.uint8)
                for i, (a, b) in enumerate(plan.blocks_of(share)):
                    buf[i * BLOCK * row_bytes:i * BLOCK * row_bytes + (b - a) * row_bytes] = truth[a:b].reshape(-1)
                staging[r] = buf
                gra.check(entry(parts[r], buf.ctypes.data, None, *args))
        for e in box.log:
            if e[1] in ("send", "recv"):
                base = assembled.ctypes.data if e[0] == 0 else staging[e[0]].ctypes.data
                calls.append((e[0], e[1], e[2], e[3], e[4], e[5] - base))
            else:
                calls.append(e)
        box.deliver()
    finally:
        for h in parts:
            gra.lib.gr_tiled_destroy(h)
    assert np.array_equal(assembled, truth), (world, rotation, fmt)
    # the schedule: per rank one group around all of its calls, the frame's stream on every call, the root only receives
    for r in range(world):
        mine = [e for e in calls if e[0] == r]
        assert mine[0][1] == "begin" and mine[-1][1] == "end" and [e[1] for e in mine].count("begin") == 1
        share = (r + rotation) % world
        if r == 0:
            want = [(0, "recv", peer, (b - a) * row_bytes // 4, stream.value, a * row_bytes)
                    for peer in range(1, world) for a, b in plan.blocks_of((peer + rotation) % world)]
        else:
            want = [(r, "send", 0, (b - a) * row_bytes // 4, stream.value, i * BLOCK * row_bytes) for i, (a, b) in enumerate(plan.blocks_of(share))]
        assert mine[1:-1] == want, (world, rotation, fmt, r)
    return calls


@pytest.mark.parametrize("fmt", [F32, RGBA8])
@pytest.mark.parametrize("world", [2, 3])
def test_exchange_of_either_format_with_a_recording_transport(world, fmt):
    """40 x 88 in blocks of 16 rows: every rotation from 0 to world.  The assembled frame equals the source bytes; each participant's send
    for its local block i starts at i x block_rows x row_bytes of its staging; the word counts are width x rows for a byte frame and
    4 x width x rows for a float frame (all three asserted in exchange())"""
    per_row = WIDTH if fmt == RGBA8 else 4 * WIDTH
    plan, seen = StripPlan(HEIGHT, world, BLOCK), set()
    for rotation in range(world + 1):
        calls = exchange(world, rotation, fmt, gra.lib.gr_tiled_exchange_as)
        words = [e[3] for e in calls if e[1] == "send"]
        assert sum(words) == sum((b - a) * per_row for s in range(world) if s != rotation % world for a, b in plan.blocks_of(s))
        seen.update(words)
    assert seen == {8 * per_row, 16 * per_row}   # (the short block travels in every rotation but the one that gives it to the root)


@pytest.mark.parametrize("world", [2, 3])
def test_the_old_exchange_records_what_the_float_case_records(world):
    for rotation in range(world + 1):
        assert exchange(world, rotation, F32, gra.lib.gr_tiled_exchange) == exchange(world, rotation, F32, gra.lib.gr_tiled_exchange_as)
