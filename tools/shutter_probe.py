"""What the shutter of motion-blurred frames costs (GPU box):
    PYTHONPATH=. python tools/shutter_probe.py [--out profiles/shutter_accumulate.txt]
 (1) "launch": at 3840x2160 output, factors 1 and 2, from a rendered Kerr source: gr_shutter_accumulate (kernels/shutter.hip) with `first`
     (reads the source, writes the accumulation frame) and without (reads both, writes it), against gr_resolve_supersampled on the same
     source - the parent's kernel, the yardstick, launched twice in every round so that the spread between two equal launches of this
     session is on the same page - and against device-to-device hipMemcpyAsyncs of HALF the bytes each accumulate launch moves (a copy
     reads and writes its size: the same traffic, the floor).  The shader clock the driver reports (read, never set) before and after.
 (2) "sequence": 24 delivered 1920x1080 frames with 8 sub-frames each through gr_render_subframe + one gr_deliver_accumulated and a pinned
     download a frame, against the same 192 cameras as plain frames through gr_render_frame_yuv420 with a download each; host clock around
     each whole sequence, in turn.  The ratio is reported, nothing is gated on it: the accumulate launch should vanish beside eight traces.
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path, one frame at a time).  Every section is a child process of its
own under a time limit of its own, started only if the one before it ended well: a fault, an abort or a time limit ends the probe there,
and what was measured until then is on file.  HIP events on a stream of the library's own runtime for (1), WARMUP rounds untimed, STEPS
timed one by one in turn, the median (min, p90)."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer, yuv420_bytes  # noqa: E402
from geodesic_raytracing_amd.render import camera_path_at, shutter_times  # noqa: E402
from tools.present_yuv_probe import alternating, kerr, shader_clock  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZE = (3840, 2160)
FACTORS = (1, 2)
WARMUP, STEPS = 5, 30
SEQUENCE_SIZE, SEQUENCE, SAMPLES, SEQUENCE_ROUNDS = (1920, 1080), 24, 8, 2
SECTIONS = {"launch": 240, "sequence": 300}   # name: seconds the child may take


def section_launch(stream):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    lines = [f"(1) the launch alone, {w}x{h} output; substituted program {prog.build_key} (the frame path's build key); {WARMUP} warm-up + {STEPS} timed "
             f"launches each, in turn, HIP events, median (min, p90)", f"    shader clock before: {shader_clock()}"]
    for f in FACTORS:
        tw, th = w * f, h * f
        read_bytes, frame_bytes = tw * th * 16, w * h * 16
        plain = gra.RenderState(tw, th, 0)
        traced = DeviceBuffer(0, read_bytes)
        accum, out = DeviceBuffer(0, frame_bytes), DeviceBuffer(0, frame_bytes)
        first_copy, add_copy = (read_bytes + frame_bytes) // 2, (read_bytes + 2 * frame_bytes) // 2
        copy_src, copy_dst = DeviceBuffer(0, add_copy), DeviceBuffer(0, add_copy)
        check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(add_copy // 4, dtype=np.float32).ctypes.data_as(ctypes.c_void_p), add_copy))
        plain.render(prog, metric, gra.default_camera(), traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        del plain
        weight = float(np.float32(1) / np.float32(8))

        def first():
            check(lib.gr_shutter_accumulate(prog.handle, stream, traced.ptr, accum.ptr, w, h, f, weight, 1))

        def add():   # (the sum grows by a bounded amount a launch: 35 launches of weight 1/8 stay far from overflow)
            check(lib.gr_shutter_accumulate(prog.handle, stream, traced.ptr, accum.ptr, w, h, f, weight, 0))

        def resolve():
            check(lib.gr_resolve_supersampled(prog.handle, stream, traced.ptr, out.ptr, w, h, f, h, 0, 1, 0))

        def resolve_again():   # the same launch a second time in every round: the spread between two equal launches in this session
            resolve()

        def copy_first():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, first_copy, 3, stream) == 0   # hipMemcpyDeviceToDevice

        def copy_add():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, add_copy, 3, stream) == 0

        t = alternating(timer, {"first": first, "resolve": resolve, "add": add, "resolve again": resolve_again, "copy first": copy_first, "copy add": copy_add})
        m = {k: float(np.median(v)) for k, v in t.items()}
        lines += ["", f"    factor {f} (source {tw}x{th}): every launch reads {read_bytes / 1e6:.0f} MB of source; the frame is {frame_bytes / 1e6:.0f} MB - written by the "
                      "resolve and by `first`, read and written without it",
                  f"    gr_shutter_accumulate, first     {say(t['first'])}   {(read_bytes + frame_bytes) / m['first'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_shutter_accumulate, adding    {say(t['add'])}   {(read_bytes + 2 * frame_bytes) / m['add'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_resolve_supersampled          {say(t['resolve'])}   {(read_bytes + frame_bytes) / m['resolve'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_resolve_supersampled again    {say(t['resolve again'])}   (|again - first| = {abs(m['resolve again'] - m['resolve']):.4f} ms: the session's spread)",
                  f"    hipMemcpyAsync D2D of {first_copy / 1e6:4.0f} MB    {say(t['copy first'])}   {2 * first_copy / m['copy first'] / 1e6:7.0f} GB/s read + written (the traffic of `first`)",
                  f"    hipMemcpyAsync D2D of {add_copy / 1e6:4.0f} MB    {say(t['copy add'])}   {2 * add_copy / m['copy add'] / 1e6:7.0f} GB/s read + written (the traffic of adding)",
                  f"    first - resolve = {m['first'] - m['resolve']:+.4f} ms, adding - resolve = {m['add'] - m['resolve']:+.4f} ms;  first / resolve = "
                  f"{m['first'] / m['resolve']:.3f}, first / its copy = {m['first'] / m['copy first']:.2f}, adding / its copy = {m['add'] / m['copy add']:.2f}"]
        del traced, accum, out, copy_src, copy_dst
    lines.append(f"    shader clock after:  {shader_clock()}")
    return lines


def section_sequence(stream):
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED)
    w, h = SEQUENCE_SIZE
    moments = shutter_times(SEQUENCE, 0.5, SAMPLES).ravel()
    cameras = [gra.default_camera(position, quat) for position, quat in camera_path_at([0, 0, -8, 0], None, [0, 3, -6, 0], None, SEQUENCE, moments)]
    weight = float(np.float32(1) / np.float32(SAMPLES))
    n = yuv420_bytes(w, h)
    state = gra.RenderState(w, h, 0)
    out, pinned = DeviceBuffer(0, n), PinnedBuffer(n)
    lines = [f"(2) {SEQUENCE} delivered frames of {w}x{h} with {SAMPLES} sub-frames each (a pan, shutter 0.5) against the same {len(cameras)} cameras as plain frames; "
             f"substituted program {prog.build_key}; host clock around each whole sequence, the two in turn, 1 warm-up + {SEQUENCE_ROUNDS} timed sequences each"]

    def blurred():
        for k, cam in enumerate(cameras):
            state.render_subframe(prog, metric, cam, weight, k % SAMPLES == 0, bg, feats, cfgv, opts, stream)
            if k % SAMPLES == SAMPLES - 1:
                state.deliver_accumulated(prog, out.ptr, gra.FRAME_YUV420, gra.YUV420_I420, stream)
                pinned.download_async(stream, out.ptr, n)
                check(lib.gr_stream_synchronize(stream))

    def plain():
        for cam in cameras:
            state.render_yuv420(prog, metric, cam, out.ptr, bg, feats, cfgv, opts, stream)
            pinned.download_async(stream, out.ptr, n)
            check(lib.gr_stream_synchronize(stream))

    times = {"blurred": [], "plain": []}
    for k in range(1 + SEQUENCE_ROUNDS):
        for name, work in (("blurred", blurred), ("plain", plain)):
            t0 = time.perf_counter()
            work()
            if k:
                times[name].append((time.perf_counter() - t0) * 1e3)
    b, p = np.sort(np.array(times["blurred"])), np.sort(np.array(times["plain"]))
    lines += [f"    {len(cameras)} x gr_render_subframe + {SEQUENCE} x (gr_deliver_accumulated + download)   {float(np.median(b)):9.2f} ms a sequence (min {b[0]:.2f}, max {b[-1]:.2f}), "
              f"{float(np.median(b)) / SEQUENCE:.3f} ms a delivered frame",
              f"    {len(cameras)} x (gr_render_frame_yuv420 + download)                             {float(np.median(p)):9.2f} ms a sequence (min {p[0]:.2f}, max {p[-1]:.2f}), "
              f"{float(np.median(p)) / len(cameras):.3f} ms a frame",
              f"    blurred / plain = {float(np.median(b)) / float(np.median(p)):.3f} (the blurred sequence encodes and downloads {SEQUENCE} frames, the plain one {len(cameras)})"]
    pinned.free()
    return lines


def child(section):
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("shutter_probe: no GPU (there is nothing to measure without one)")
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    lines = {"launch": section_launch, "sequence": section_sequence}[section](stream)
    check(lib.gr_stream_destroy(stream))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter_accumulate.txt"))
    ap.add_argument("--section", choices=sorted(SECTIONS), default=None, help="run this section in this process and print it (what the probe starts for each)")
    a = ap.parse_args()
    if a.section:
        child(a.section)
        return 0
    text = ["shutter_probe: kerr_boyer a = 0.45, fused path, one frame in flight"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for section, limit in SECTIONS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", section], cwd=ROOT, capture_output=True, text=True, timeout=limit)
            code, out, err = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as e:
            code, out, err = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), f"time limit of {limit} s"
        text += ["", out.rstrip()] if code == 0 else ["", f"section {section!r} ended with status {code}; nothing after it was started", err[-3000:]]
        print("\n".join(text[-2:]), flush=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(text) + "\n")
        if code != 0:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
