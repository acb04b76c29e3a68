"""GPU tests (-m gpu) of split frames in either format (gr_render_frame_tiled_as): participants of one process on device 0 (peer copies)
render rotating shares of supersampled float frames and of 8-bit frames, and participant 0's frame is, bit for bit, the frame one render
state renders alone; frames of both formats in flight through one staging ring; the object's life cycle; one frame across two processes
(gr_tiled_create_ipc); and the CLI's --devices.  Kerr (scripts/kerr_boyer.js), a = 0.45, a 512 x 256 synthetic sky, 160 x 88 pixels in
blocks of 16 rows: five full blocks and one of 8, so the shares are unequal and one participant's last block is short."""
import ctypes
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BLOCK = 160, 88, 16
_shared = {}


def kerr():
    """metric, dynamic program, parameters, features and sky, shared by every test of this file"""
    if "kerr" not in _shared:
        metric = gra.Metric("kerr_boyer")
        packed, levels = gra.pack_background(gra.synthetic_background(512, 256))
        sky = DeviceBuffer.from_numpy(0, packed)
        _shared["kerr"] = (metric, gra.Program(metric.argument_string(), 0), metric.cfg_values(a=0.45), metric.features(adaptive_sampling=0),
                           (sky.ptr, 512, 256, levels), sky)
    return _shared["kerr"][:5]


def camera(k):
    return gra.default_camera([0, 0.1 * k, -4 - 0.3 * k, 0.05 * k])


def alone(k, factor, rgba8):
    """camera k's frame as one render state of that factor renders it: float32 [H, W, 4] of render(), uint8 [H, W, 4] of render_rgba8().
    Rendered once and shared (read-only)."""
    key = ("alone", k, factor, rgba8)
    if key not in _shared:
        metric, prog, cfgv, feats, bg = kerr()
        state = gra.RenderState(W, H, 0, supersample=factor)
        out = DeviceBuffer(0, W * H * (4 if rgba8 else 16))
        (state.render_rgba8 if rgba8 else state.render)(prog, metric, camera(k), out.ptr, bg, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED))
        state.synchronize()
        frame = out.to_numpy(np.uint8 if rgba8 else np.float32, (H, W, 4))
        frame.setflags(write=False)
        assert frame.any()
        _shared[key] = frame
    return _shared[key]


def filled(nbytes):
    """a frame buffer that starts as 0xCD bytes: a row nobody wrote shows"""
    return DeviceBuffer.from_numpy(0, np.full(nbytes, 0xCD, np.uint8))


def split_frames(world, factor, rgba8, cameras=3):
    """`cameras` frames, frame k with rotation k and the next frame's camera announced, by `world` participants with a state each"""
    metric, prog, cfgv, feats, bg = kerr()
    parts = gra.TiledFrame.local([0] * world, W, H, BLOCK)
    try:
        states = [gra.RenderState(W, H, 0, supersample=factor) for _ in range(world)]
        cams = [camera(k) for k in range(cameras)]
        got = []
        for k in range(cameras):
            frame = filled(W * H * (4 if rgba8 else 16))
            for r in range(world):
                o = gra.frame_options(mode=gra.MODE_FUSED)
                if k + 1 < cameras:
                    o.next_camera = ctypes.pointer(cams[k + 1])
                parts[r].render_as(states[r], prog, metric, cams[k], frame.ptr, bg, feats, cfgv, o, rotation=k, rgba8=rgba8)
            parts[0].join()
            check(lib.gr_device_synchronize(0))
            got.append(frame.to_numpy(np.uint8 if rgba8 else np.float32, (H, W, 4)))
        return got
    finally:
        for p in parts:
            p.close()


def rows_that_differ(got, want):
    return np.flatnonzero((got.view(np.uint8).reshape(H, -1) != want.view(np.uint8).reshape(H, -1)).any(axis=1)).tolist()


@pytest.mark.parametrize("factor", [2, 3])
def test_a_supersampled_split_frame_is_the_single_state_frame(factor):
    """float frames, three participants: every share is traced at factor x, resolved where it was traced and shipped as 160 x rows float4"""
    for k, got in enumerate(split_frames(3, factor, False)):
        want = alone(k, factor, False)
        assert got.tobytes() == want.tobytes(), (factor, k, rows_that_differ(got, want))


@pytest.mark.parametrize("factor", [1, 2])
def test_an_8_bit_split_frame_is_the_single_state_frame(factor):
    """byte frames: the rows travel at 4 bytes a pixel, packed into the first quarter of a staging slot sized for float rows"""
    for k, got in enumerate(split_frames(3, factor, True)):
        want = alone(k, factor, True)
        assert got.tobytes() == want.tobytes(), (factor, k, rows_that_differ(got, want))


def test_frames_of_both_formats_in_flight_through_one_ring():
    """two participants, each with two states on two streams: six frames issued back to back, even ones float at factor 2 on stream 0,
    odd ones 8-bit at factor 1 on stream 1, the share rotating - more frames than the ring has slots, so a slot is reused by a frame of the
    other format.  One join at the end."""
    metric, prog, cfgv, feats, bg = kerr()
    world, count = 2, 6
    factor = {False: 2, True: 1}
    parts = gra.TiledFrame.local([0] * world, W, H, BLOCK)
    streams = []
    try:
        for _ in range(world * 2):
            s = ctypes.c_void_p()
            check(lib.gr_stream_create(0, 0, ctypes.byref(s)))
            streams.append(s)
        states = [[gra.RenderState(W, H, 0, supersample=factor[bool(j)]) for j in range(2)] for _ in range(world)]
        frames = [filled(W * H * (4 if k % 2 else 16)) for k in range(count)]
        cams = [camera(k % 3) for k in range(count)]
        for k in range(count):
            j = k % 2
            for r in range(world):
                parts[r].render_as(states[r][j], prog, metric, cams[k], frames[k].ptr, bg, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED),
                                   stream=streams[2 * r + j], rotation=k, rgba8=bool(j))
        parts[0].join(streams[0])
        check(lib.gr_device_synchronize(0))
        for k in range(count):
            rgba8 = bool(k % 2)
            got, want = frames[k].to_numpy(np.uint8 if rgba8 else np.float32, (H, W, 4)), alone(k % 3, factor[rgba8], rgba8)
            assert got.tobytes() == want.tobytes(), (k, rows_that_differ(got, want))
    finally:
        for p in parts:
            p.close()
        for s in streams:
            check(lib.gr_stream_destroy(s))


def test_what_a_state_makes_a_participant_refuse():
    """the two refusals that read the render state (the others: tests/test_tiled_formats_abi.py): a state whose OUTPUT size is not the
    participant's - a plain state of the traced size is not a supersampled state of the frame's size - and blocks whose traced rows an
    int does not count.  Both before anything is allocated or launched; and the old entry point still names the new one."""
    metric, prog, cfgv, feats, bg = kerr()
    frame = filled(W * H * 16)
    parts = gra.TiledFrame.local([0, 0], W, H, BLOCK)
    huge = gra.TiledFrame.local([0, 0], W, H, 0x40000000)   # twice that is 2^31
    try:
        right = gra.RenderState(W, H, 0, supersample=2)
        for wrong in (gra.RenderState(2 * W, 2 * H, 0), gra.RenderState(W // 2, H // 2, 0, supersample=2), gra.RenderState(W, H + 8, 0)):
            for rgba8 in (False, True):
                with pytest.raises(gra.GeodesicError, match="not of the size"):
                    parts[1].render_as(wrong, prog, metric, camera(0), frame.ptr, bg, feats, cfgv, rgba8=rgba8)
        for rgba8 in (False, True):
            with pytest.raises(gra.GeodesicError, match="more rows than an int counts"):
                huge[1].render_as(right, prog, metric, camera(0), frame.ptr, bg, feats, cfgv, rgba8=rgba8)
        with pytest.raises(gra.GeodesicError, match="root needs the frame"):
            parts[0].render_as(right, prog, metric, camera(0), None, bg, feats, cfgv)
        with pytest.raises(gra.GeodesicError, match="format"):
            check(lib.gr_render_frame_tiled_as(parts[0].handle, right.handle, prog.handle, metric.handle, None, ctypes.byref(camera(0)), ctypes.byref(feats),
                                               None, 0, None, None, 0, 0, 0, frame.ptr, None, 0, 2))
        with pytest.raises(gra.GeodesicError, match="supersampled.*gr_render_frame_tiled_as"):
            parts[0].render(right, prog, metric, camera(0), frame.ptr, bg, feats, cfgv)
        check(lib.gr_device_synchronize(0))
        assert (frame.to_numpy(np.uint8, (W * H * 16,)) == 0xCD).all()   # nothing was rendered
    finally:
        for p in parts + huge:
            p.close()


def test_one_participant_falls_through_to_the_frame_entry_points():
    metric, prog, cfgv, feats, bg = kerr()
    (one,) = gra.TiledFrame.local([0], W, H, BLOCK)
    try:
        state = gra.RenderState(W, H, 0, supersample=2)
        for rgba8 in (False, True):
            frame = filled(W * H * (4 if rgba8 else 16))
            one.render_as(state, prog, metric, camera(1), frame.ptr, bg, feats, cfgv, rotation=5, rgba8=rgba8)
            check(lib.gr_device_synchronize(0))
            assert frame.to_numpy(np.uint8 if rgba8 else np.float32, (H, W, 4)).tobytes() == alone(1, 2, rgba8).tobytes()
    finally:
        one.close()


def test_participants_and_their_states_give_their_memory_back():
    """ten create / render / close cycles of two participants with a factor-2 state each, a float and a byte frame per cycle: free device
    memory comes back within the allowance of tests/test_gpu_lifecycle.py, read through the HIP runtime the library itself runs on"""
    from test_gpu_lifecycle import MiB, device_bytes_in_use

    def cycle():
        for rgba8 in (False, True):
            (got,) = split_frames(2, 2, rgba8, cameras=1)
            assert got.tobytes() == alone(0, 2, rgba8).tobytes()
        gc.collect()

    cycle()
    before = device_bytes_in_use()
    for _ in range(10):
        cycle()
    after = device_bytes_in_use()
    assert after - before < 4 * MiB, (before, after)


IPC_CHILD = r"""
import sys
import numpy as np
import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd.pipeline import DeviceBuffer
rank, session, out_path = int(sys.argv[1]), sys.argv[2], sys.argv[3]
W, H, BLOCK = 160, 88, 16
metric = gra.Metric("kerr_boyer")
prog = gra.Program(metric.argument_string(), 0)
packed, levels = gra.pack_background(gra.synthetic_background(512, 256))
sky = DeviceBuffer.from_numpy(0, packed)
part = gra.TiledFrame.ipc(2, rank, 0, session, W, H, BLOCK)   # collective
state = gra.RenderState(W, H, 0, supersample=2)
frame = DeviceBuffer.from_numpy(0, np.full(W * H * 4, 0xCD, np.uint8)) if rank == 0 else None
part.render_as(state, prog, metric, gra.default_camera([0, 0.1 * 1, -4 - 0.3 * 1, 0.05 * 1]), frame.ptr if rank == 0 else None, (sky.ptr, 512, 256, levels),
               metric.features(adaptive_sampling=0), metric.cfg_values(a=0.45), gra.frame_options(mode=gra.MODE_FUSED), rotation=1, rgba8=True)
gra.check(gra.lib.gr_device_synchronize(0))
if rank == 0:
    np.save(out_path, frame.to_numpy(np.uint8, (H, W, 4)))
part.close()
"""


def test_an_8_bit_frame_across_two_processes(tmp_path):
    """gr_tiled_create_ipc, world 2, factor 2, one byte frame with rotation 1 (rank 0 renders share 1, rank 1's share holds the short
    block): the point-to-point path - a group, a send of width x rows words per block, the matching receives - between two processes"""
    session = f"f{os.getpid()}"
    out = str(tmp_path / "frame.npy")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), GR_TILED_IPC_TIMEOUT="30")
    children = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, "-c", IPC_CHILD, str(rank), session, out], env=env,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rank in range(2)]
    outputs = [c.communicate()[0] for c in children]
    codes = [c.returncode for c in children]
    assert codes == [0, 0], (codes, [o[-1500:] for o in outputs])   # (nothing below runs on the device unless both ended well)
    got, want = np.load(out), alone(1, 2, True)
    assert got.tobytes() == want.tobytes(), rows_that_differ(got, want)


def test_the_cli_writes_the_same_png_over_two_participants(tmp_path):
    from geodesic_raytracing_amd import render
    paths = {}
    for how, more in (("one", []), ("split", ["--devices", "0,0"])):
        paths[how] = str(tmp_path / f"kerr_{how}.png")
        assert render.main(["--metric", "kerr_boyer", "--cfg", "a=0.45", "--size", "64x48", "--supersample", "2", "--encode", "device", *more,
                            "--out", paths[how]]) == 0
    one, split = open(paths["one"], "rb").read(), open(paths["split"], "rb").read()
    assert len(one) > 1000 and one == split
    assert render.read_png(paths["split"]).shape == (48, 64, 4)
    # ... and as floats, sky built on the device, the share rotating over three frames: each is the whole frame
    whole = render.render("kerr_boyer", 64, 48, cfg=dict(a=0.45), supersample=2, mips="device")
    frames = render.render_split("kerr_boyer", 64, 48, [0, 0, 0], cfg=dict(a=0.45), supersample=2, mips="device", frames=3)
    assert len(frames) == 3 and all(f.tobytes() == whole.tobytes() for f in frames)
