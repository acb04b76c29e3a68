"""What 8-bit frames encoded on the device cost (GPU box):
    PYTHONPATH=. python tools/present_probe.py [--out profiles/present_rgba8.txt] [--parent DIR]
 (a) gr_present_rgba8 (kernels/present.hip) alone against a device-to-device hipMemcpyAsync of HALF the bytes it moves - a copy reads and
     writes its size, so that is the same traffic - and, at factors 2 and 3, against gr_resolve_supersampled (kernels/resolve.hip, which this
     feature leaves as it was: the one timed is this build's, whose set-up module holds both kernels) on the same source: the fused launch
     reads the same bytes and writes a quarter of them;
 (b) whole frames of one factor-2 state at 1920x1080, gr_render_frame_rgba8 alternating with gr_render_frame;
 (c) the download of a 3840x2160 frame as float4 and as RGBA8, pageable (gr_device_download) and pinned (gr_device_download_async + a
     stream synchronise), timed on the host;
 (d) with --parent DIR, a built checkout of the parent commit: bench.py --gpus 1 --steps 20 --warmup 3 of that tree and of this one in
     turn, BENCH_RUNS each, every run a child process with a time limit of its own; the headline figure and the frame path's build key
     (gr_program_build_key) of both, which must be equal - the new kernel is in the set-up module only.
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path, one frame at a time); the sources of (a) are rendered frames.  HIP
events on a stream of the library's own runtime, WARMUP launches untimed, STEPS timed one by one in turn, the median (and the spread)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

CASES = [(3840, 2160, 1), (3840, 2160, 2), (2560, 1440, 3)]   # output size, factor
FRAME = (1920, 1080, 2)
DOWNLOAD = (3840, 2160)
WARMUP, STEPS = 5, 30
BENCH_RUNS, BENCH_LIMIT_S = 4, 240
BENCH_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "3"]


def alternating(timer, works):
    """the launches of `works` in turn, WARMUP rounds untimed, STEPS rounds timed (this file's counts): {name: ms per launch, sorted}"""
    for _ in range(WARMUP):
        for work in works.values():
            timer.one(work)
    times = {name: [] for name in works}
    for _ in range(STEPS):
        for name, work in works.items():
            times[name].append(timer.one(work))
    return {name: np.sort(np.array(t)) for name, t in times.items()}


def bench_line(tree):
    """one bench.py run of a tree in a child process: its JSON result line"""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + BENCH_ARGS, cwd=tree, capture_output=True, text=True, timeout=BENCH_LIMIT_S)
    if r.returncode != 0:
        raise SystemExit(f"present_probe: bench.py of {tree} failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def host_timed(work, rounds=WARMUP + 12):
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        work()
        t.append((time.perf_counter() - t0) * 1e3)
    return np.sort(np.array(t[WARMUP:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "present_rgba8.txt"))
    ap.add_argument("--parent", default="", metavar="DIR", help="a built checkout of the parent commit: section (d)")
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("present_probe: no GPU (there is nothing to measure without one)")
    hip = hip_runtime()
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    timer = Timer(hip, stream)
    scripts = os.path.join(os.path.dirname(gra.__file__), "scripts")
    metric = gra.Metric("kerr_boyer", scripts)
    cfgv = metric.cfg_values(a=0.45)
    feats = metric.features(adaptive_sampling=0)
    prog = gra.Program(metric.argument_string(feats, static=True, cfg_values=cfgv), 0)
    packed, levels = gra.pack_background(gra.synthetic_background(2048, 1024))
    dbg = DeviceBuffer.from_numpy(0, packed)
    bg = (dbg.ptr, packed.shape[2], packed.shape[1], levels)
    camera = gra.default_camera()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    lines = [f"present_probe: kerr_boyer a = 0.45, substituted program {prog.build_key} (the frame path's build key), fused path, one frame in flight; "
             f"{WARMUP} warm-up + {STEPS} timed launches each, in turn, HIP events, median (min, p90)"]

    for w, h, f in CASES:
        tw, th = w * f, h * f
        read_bytes, write_bytes, float_bytes = tw * th * 16, w * h * 4, w * h * 16
        copy_bytes = (read_bytes + write_bytes) // 2 // 16 * 16
        plain = gra.RenderState(tw, th, 0)
        traced = DeviceBuffer(0, read_bytes)
        out8, out32 = DeviceBuffer(0, write_bytes), DeviceBuffer(0, float_bytes)
        copy_src, copy_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
        check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(copy_bytes // 4, dtype=np.float32).ctypes.data_as(ctypes.c_void_p), copy_bytes))
        plain.render(prog, metric, camera, traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        del plain

        def present():
            check(lib.gr_present_rgba8(prog.handle, stream, traced.ptr, out8.ptr, w, h, f, h, 0, 1, 0))

        def resolve():
            check(lib.gr_resolve_supersampled(prog.handle, stream, traced.ptr, out32.ptr, w, h, f, h, 0, 1, 0))

        def copy():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, copy_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice

        def copy_again():   # the same copy a second time in every round: the spread between two equal launches in this session
            copy()

        works = {"present": present, "copy": copy, "copy again": copy_again}
        if f > 1:
            works["resolve"] = resolve
        t = alternating(timer, works)
        p, c, c2 = (float(np.median(t[k])) for k in ("present", "copy", "copy again"))
        lines += ["", f"(a) {w}x{h} output, factor {f} (source {tw}x{th}): the launch reads {read_bytes / 1e6:.0f} MB and writes {write_bytes / 1e6:.1f} MB",
                  f"    gr_present_rgba8                 {say(t['present'])}   {(read_bytes + write_bytes) / p / 1e6:7.0f} GB/s read + written",
                  f"    hipMemcpyAsync D2D of {copy_bytes / 1e6:4.0f} MB    {say(t['copy'])}   {2 * copy_bytes / c / 1e6:7.0f} GB/s read + written",
                  f"    the same copy again              {say(t['copy again'])}   (copy again / copy = {c2 / c:.3f}: the session's spread)",
                  f"    present / copy = {p / c:.2f}"]
        if f > 1:
            r = float(np.median(t["resolve"]))
            lines += [f"    gr_resolve_supersampled          {say(t['resolve'])}   {(read_bytes + float_bytes) / r / 1e6:7.0f} GB/s read + written (writes {float_bytes / 1e6:.0f} MB)",
                      f"    present / resolve = {p / r:.2f}   (the resolve of this build: resolve.hip is the parent's file unchanged, in a module that now also holds the new kernel)"]
        del traced, out8, out32, copy_src, copy_dst

    # (b) whole frames of one state, 8-bit and float in turn
    w, h, f = FRAME
    state = gra.RenderState(w, h, 0, supersample=f)
    out8, out32 = DeviceBuffer(0, w * h * 4), DeviceBuffer(0, w * h * 16)

    def frame8():
        state.render_rgba8(prog, metric, camera, out8.ptr, bg, feats, cfgv, opts, stream)

    def frame32():
        state.render(prog, metric, camera, out32.ptr, bg, feats, cfgv, opts, stream)

    t = alternating(timer, {"rgba8": frame8, "float": frame32})
    e, fl = float(np.median(t["rgba8"])), float(np.median(t["float"]))
    lines += ["", f"(b) whole frames of one state, {w}x{h} at factor {f}, in turn",
              f"    gr_render_frame_rgba8            {say(t['rgba8'])}",
              f"    gr_render_frame                  {say(t['float'])}",
              f"    rgba8 - float = {e - fl:+.3f} ms"]
    del state, out8, out32

    # (c) downloads, on the host's clock: the call and the wait for it
    w, h = DOWNLOAD
    lines += ["", f"(c) download of a {w}x{h} frame, host clock around the call and its wait, {WARMUP} warm-up + 12 timed"]
    for name, nbytes in (("float4", w * h * 16), ("RGBA8", w * h * 4)):
        dev = DeviceBuffer(0, nbytes)
        check(lib.gr_device_upload(0, dev.ptr, np.zeros(nbytes, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p), nbytes))
        pageable = np.empty(nbytes, dtype=np.uint8)
        pinned = PinnedBuffer(nbytes)

        def blocking():
            check(lib.gr_device_download(0, pageable.ctypes.data_as(ctypes.c_void_p), dev.ptr, nbytes))

        def through_pinned():
            pinned.download_async(stream, dev.ptr, nbytes)
            check(lib.gr_stream_synchronize(stream))

        for label, work in (("pageable, gr_device_download", blocking), ("pinned, gr_device_download_async", through_pinned)):
            t = host_timed(work)
            lines.append(f"    {name:6s} {nbytes / 1e6:6.1f} MB  {label:34s} {say(t)}   {nbytes / float(np.median(t)) / 1e6:6.1f} GB/s")
        pinned.free()
        del dev
    check(lib.gr_stream_destroy(stream))

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    print("\n".join(lines), flush=True)
    write()   # (a) - (c) are on file before the long part starts
    shown = len(lines)

    # (d) the headline bench of the parent's tree and of this one in turn
    if a.parent:
        trees = {"parent": os.path.abspath(a.parent), "this": ROOT}
        runs = {name: [] for name in trees}
        for _ in range(BENCH_RUNS):
            for name, tree in trees.items():
                runs[name].append(bench_line(tree))
        lines += ["", f"(d) bench.py {' '.join(BENCH_ARGS)}, the parent's tree and this one in turn, {BENCH_RUNS} runs each, one child process a run"]
        for name in trees:
            keys = sorted({r["config"]["build_key"] for r in runs[name]})
            values = [r["value"] for r in runs[name]]
            lines.append(f"    {name:6s}  {' / '.join(f'{v:.1f}' for v in values)} {runs[name][0]['unit']}   median {float(np.median(values)):.1f}   frame-path build key {', '.join(keys)}")
        pk, tk = ({r["config"]["build_key"] for r in runs[name]} for name in ("parent", "this"))
        mp, mt = (float(np.median([r["value"] for r in runs[name]])) for name in ("parent", "this"))
        lines.append(f"    build keys {'equal' if pk == tk and len(pk) == 1 else 'DIFFERENT'};  this / parent = {mt / mp:.4f} (medians)")
    else:
        lines += ["", "(d) not run: no --parent DIR given"]
    print("\n".join(lines[shown:]), flush=True)
    write()


if __name__ == "__main__":
    main()
