"""What video frames encoded on the device cost (GPU box):
    PYTHONPATH=. python tools/present_yuv_probe.py [--out profiles/present_yuv420.txt]
At 3840x2160, factors 1 and 2:
 (1) gr_present_yuv420 (kernels/present.hip, I420 and NV12) against gr_present_rgba8 on the same source, twice each in every round - the
     second RGBA8 launch shows the spread between two equal launches of this session, the yardstick the new launch is held to - and
     against a device-to-device hipMemcpyAsync of HALF the bytes the YUV launch moves (a copy reads and writes its size: the same traffic);
 (2) the pinned download (gr_device_download_async + a stream synchronise, host clock) of 1.5, 4 and 16 bytes a pixel;
 (3) a sequence of 24 frames through gr_render_frame_yuv420 + the pinned download of each, against the same sequence through
     gr_render_frame_rgba8 + its download + the host conversion (gr_rgba8_to_yuv420), host clock around each whole sequence, in turn.
 (4) gr_present_yuv420p10 (10-bit samples in 16-bit words: yuv420p10le and P010) against gr_present_yuv420 on the same source, the 8-bit
     launch twice in every round as in (1); the shader clock the driver reports (read, never set) before and after is noted.
     Section "launch10"; alone:  python tools/present_yuv_probe.py --section launch10
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path, one frame at a time); the sources of (1) are rendered frames.
Every section is a child process of its own under a time limit of its own, started only if the one before it ended well: a fault, an
abort or a time limit ends the probe there, and what was measured until then is on file.  HIP events on a stream of the library's own
runtime for (1), WARMUP rounds untimed, STEPS timed one by one in turn, the median (min, p90)."""
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
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer, rgba8_to_yuv420, yuv420_bytes, yuv420p10_bytes  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZE = (3840, 2160)
FACTORS = (1, 2)
WARMUP, STEPS = 5, 30
SEQUENCE, SEQUENCE_ROUNDS = 24, 3
SECTIONS = {"launch": 240, "download": 120, "sequence": 420, "launch10": 240}   # name: seconds the child may take


def alternating(timer, works):
    for _ in range(WARMUP):
        for work in works.values():
            timer.one(work)
    times = {name: [] for name in works}
    for _ in range(STEPS):
        for name, work in works.items():
            times[name].append(timer.one(work))
    return {name: np.sort(np.array(t)) for name, t in times.items()}


def host_timed(work, warmup, rounds):
    t = []
    for _ in range(warmup + rounds):
        t0 = time.perf_counter()
        work()
        t.append((time.perf_counter() - t0) * 1e3)
    return np.sort(np.array(t[warmup:]))


def kerr():
    metric = gra.Metric("kerr_boyer", os.path.join(os.path.dirname(gra.__file__), "scripts"))
    cfgv = metric.cfg_values(a=0.45)
    feats = metric.features(adaptive_sampling=0)
    prog = gra.Program(metric.argument_string(feats, static=True, cfg_values=cfgv), 0)
    packed, levels = gra.pack_background(gra.synthetic_background(2048, 1024))
    dbg = DeviceBuffer.from_numpy(0, packed)
    return metric, cfgv, feats, prog, dbg, (dbg.ptr, packed.shape[2], packed.shape[1], levels)


def section_launch(stream):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    lines = [f"(1) the launch alone, {w}x{h} output; substituted program {prog.build_key} (the frame path's build key); {WARMUP} warm-up + {STEPS} timed "
             f"launches each, in turn, HIP events, median (min, p90)"]
    for f in FACTORS:
        tw, th = w * f, h * f
        read_bytes, yuv_bytes, rgba_bytes = tw * th * 16, yuv420_bytes(w, h), w * h * 4
        copy_bytes = (read_bytes + yuv_bytes) // 2 // 16 * 16
        plain = gra.RenderState(tw, th, 0)
        traced = DeviceBuffer(0, read_bytes)
        out_yuv, out8 = DeviceBuffer(0, yuv_bytes), DeviceBuffer(0, rgba_bytes)
        copy_src, copy_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
        check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(copy_bytes // 4, dtype=np.float32).ctypes.data_as(ctypes.c_void_p), copy_bytes))
        plain.render(prog, metric, gra.default_camera(), traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        del plain

        def i420():
            check(lib.gr_present_yuv420(prog.handle, stream, traced.ptr, out_yuv.ptr, w, h, f, gra.YUV420_I420))

        def nv12():
            check(lib.gr_present_yuv420(prog.handle, stream, traced.ptr, out_yuv.ptr, w, h, f, gra.YUV420_NV12))

        def rgba8():
            check(lib.gr_present_rgba8(prog.handle, stream, traced.ptr, out8.ptr, w, h, f, h, 0, 1, 0))

        def rgba8_again():   # the same launch a second time in every round: the spread between two equal launches in this session
            rgba8()

        def copy():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, copy_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice

        t = alternating(timer, {"i420": i420, "rgba8": rgba8, "nv12": nv12, "rgba8 again": rgba8_again, "copy": copy})
        m = {k: float(np.median(v)) for k, v in t.items()}
        spread = abs(m["rgba8 again"] - m["rgba8"])
        lines += ["", f"    factor {f} (source {tw}x{th}): the YUV launch reads {read_bytes / 1e6:.0f} MB and writes {yuv_bytes / 1e6:.1f} MB, the RGBA8 launch writes {rgba_bytes / 1e6:.1f} MB",
                  f"    gr_present_yuv420, I420          {say(t['i420'])}   {(read_bytes + yuv_bytes) / m['i420'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_yuv420, NV12          {say(t['nv12'])}   {(read_bytes + yuv_bytes) / m['nv12'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_rgba8                 {say(t['rgba8'])}   {(read_bytes + rgba_bytes) / m['rgba8'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_rgba8 again           {say(t['rgba8 again'])}   (|again - first| = {spread:.4f} ms: the session's spread)",
                  f"    hipMemcpyAsync D2D of {copy_bytes / 1e6:4.0f} MB    {say(t['copy'])}   {2 * copy_bytes / m['copy'] / 1e6:7.0f} GB/s read + written",
                  f"    I420 - rgba8 = {m['i420'] - m['rgba8']:+.4f} ms, NV12 - rgba8 = {m['nv12'] - m['rgba8']:+.4f} ms;  I420 / rgba8 = {m['i420'] / m['rgba8']:.3f}, "
                  f"I420 / copy = {m['i420'] / m['copy']:.2f}"]
        del traced, out_yuv, out8, copy_src, copy_dst
    return lines


def shader_clock():
    """the shader clock levels the driver reports for the first card that has them, the current one starred (read only)"""
    import glob
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            with open(path) as fh:
                levels = [line.strip() for line in fh if line.strip()]
        except OSError:
            continue
        if levels:
            return ", ".join(levels)
    return "not readable"


def section_launch10(stream):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    lines = [f"(4) 10-bit against 8-bit, the launch alone, {w}x{h} output; substituted program {prog.build_key}; {WARMUP} warm-up + {STEPS} timed launches "
             f"each, in turn, HIP events, median (min, p90)", f"    shader clock before: {shader_clock()}"]
    for f in FACTORS:
        tw, th = w * f, h * f
        read_bytes, bytes8, bytes10 = tw * th * 16, yuv420_bytes(w, h), yuv420p10_bytes(w, h)
        plain = gra.RenderState(tw, th, 0)
        traced = DeviceBuffer(0, read_bytes)
        out8, out10 = DeviceBuffer(0, bytes8), DeviceBuffer(0, bytes10)
        plain.render(prog, metric, gra.default_camera(), traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        del plain

        def planar10():
            check(lib.gr_present_yuv420p10(prog.handle, stream, traced.ptr, out10.ptr, w, h, f, gra.YUV420_I420))

        def p010():
            check(lib.gr_present_yuv420p10(prog.handle, stream, traced.ptr, out10.ptr, w, h, f, gra.YUV420_NV12))

        def i420():
            check(lib.gr_present_yuv420(prog.handle, stream, traced.ptr, out8.ptr, w, h, f, gra.YUV420_I420))

        def i420_again():   # the same launch a second time in every round: the spread between two equal launches in this session
            i420()

        t = alternating(timer, {"planar10": planar10, "i420": i420, "p010": p010, "i420 again": i420_again})
        m = {k: float(np.median(v)) for k, v in t.items()}
        lines += ["", f"    factor {f} (source {tw}x{th}): both launches read {read_bytes / 1e6:.0f} MB; 8 bits write {bytes8 / 1e6:.1f} MB, 10 bits {bytes10 / 1e6:.1f} MB",
                  f"    gr_present_yuv420p10, yuv420p10le  {say(t['planar10'])}   {(read_bytes + bytes10) / m['planar10'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_yuv420p10, P010         {say(t['p010'])}   {(read_bytes + bytes10) / m['p010'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_yuv420, I420            {say(t['i420'])}   {(read_bytes + bytes8) / m['i420'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_present_yuv420, I420 again      {say(t['i420 again'])}   (|again - first| = {abs(m['i420 again'] - m['i420']):.4f} ms: the session's spread)",
                  f"    yuv420p10le - I420 = {m['planar10'] - m['i420']:+.4f} ms, P010 - I420 = {m['p010'] - m['i420']:+.4f} ms;  yuv420p10le / I420 = "
                  f"{m['planar10'] / m['i420']:.3f}, P010 / I420 = {m['p010'] / m['i420']:.3f}"]
        del traced, out8, out10
    lines.append(f"    shader clock after:  {shader_clock()}")
    return lines


def section_download(stream):
    w, h = SIZE
    lines = [f"(2) pinned download of a {w}x{h} frame (gr_device_download_async + gr_stream_synchronize), host clock, {WARMUP} warm-up + 12 timed"]
    for name, nbytes in (("YUV 4:2:0, 1.5 B a pixel", yuv420_bytes(w, h)), ("RGBA8, 4 B a pixel", w * h * 4), ("float4, 16 B a pixel", w * h * 16)):
        dev = DeviceBuffer(0, nbytes)
        check(lib.gr_device_upload(0, dev.ptr, np.zeros(nbytes, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p), nbytes))
        pinned = PinnedBuffer(nbytes)

        def through_pinned():
            pinned.download_async(stream, dev.ptr, nbytes)
            check(lib.gr_stream_synchronize(stream))

        t = host_timed(through_pinned, WARMUP, 12)
        lines.append(f"    {name:26s} {nbytes / 1e6:6.1f} MB  {say(t)}   {nbytes / float(np.median(t)) / 1e6:6.1f} GB/s")
        pinned.free()
        del dev
    return lines


def section_sequence(stream):
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    lines = [f"(3) {SEQUENCE} frames of {w}x{h}, one at a time, host clock around the whole sequence, the two ways in turn, 1 warm-up + {SEQUENCE_ROUNDS} timed sequences each"]
    cameras = [gra.default_camera([0, 0, -8 + 0.05 * k, 0]) for k in range(SEQUENCE)]
    for f in FACTORS:
        state = gra.RenderState(w, h, 0, supersample=f)
        n = yuv420_bytes(w, h)
        out_yuv, out8 = DeviceBuffer(0, n), DeviceBuffer(0, w * h * 4)
        pinned_yuv, pinned8 = PinnedBuffer(n), PinnedBuffer(w * h * 4)

        def on_device():
            for cam in cameras:
                state.render_yuv420(prog, metric, cam, out_yuv.ptr, bg, feats, cfgv, opts, stream)
                pinned_yuv.download_async(stream, out_yuv.ptr, n)
                check(lib.gr_stream_synchronize(stream))

        def on_host():
            for cam in cameras:
                state.render_rgba8(prog, metric, cam, out8.ptr, bg, feats, cfgv, opts, stream)
                pinned8.download_async(stream, out8.ptr, w * h * 4)
                check(lib.gr_stream_synchronize(stream))
                rgba8_to_yuv420(pinned8.view(np.uint8, (h, w, 4)))

        times = {"device": [], "host": []}
        for k in range(1 + SEQUENCE_ROUNDS):
            for name, work in (("device", on_device), ("host", on_host)):
                t0 = time.perf_counter()
                work()
                if k:
                    times[name].append((time.perf_counter() - t0) * 1e3 / SEQUENCE)
        d, o = np.sort(np.array(times["device"])), np.sort(np.array(times["host"]))
        lines += [f"    factor {f}: gr_render_frame_yuv420 + download                         {float(np.median(d)):8.3f} ms a frame (min {d[0]:.3f}, max {d[-1]:.3f})",
                  f"    factor {f}: gr_render_frame_rgba8 + download + gr_rgba8_to_yuv420     {float(np.median(o)):8.3f} ms a frame (min {o[0]:.3f}, max {o[-1]:.3f})"]
        pinned_yuv.free()
        pinned8.free()
        del state, out_yuv, out8
    return lines


def child(section):
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("present_yuv_probe: no GPU (there is nothing to measure without one)")
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    lines = {"launch": section_launch, "download": section_download, "sequence": section_sequence, "launch10": section_launch10}[section](stream)
    check(lib.gr_stream_destroy(stream))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_yuv420.txt"))
    ap.add_argument("--section", choices=sorted(SECTIONS), default=None, help="run this section in this process and print it (what the probe starts for each)")
    a = ap.parse_args()
    if a.section:
        child(a.section)
        return 0
    text = ["present_yuv_probe: kerr_boyer a = 0.45, fused path, one frame in flight"]
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
