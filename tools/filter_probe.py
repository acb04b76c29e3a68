"""What the separable reconstruction filters of a supersampled frame cost (GPU box):
    PYTHONPATH=. python tools/filter_probe.py [--out profiles/filter_resolve.txt] [--parent DIR]
 (1) "launch": at 3840x2160 output, factors 1, 2 and 4, from a rendered Kerr source: gr_resolve_filtered (kernels/filter.hip) with the
     Mitchell and the tent table, against gr_resolve_supersampled on the same source - the parent's kernel, the yardstick, launched twice
     in every round so that the spread between two equal launches of this session is on the same page - and against a device-to-device
     hipMemcpyAsync of HALF the algorithmic traffic (the traced frame read once, the output written once; a copy reads and writes its
     size).  The shader clock the driver reports (read, never set) before and after.
 (2) "sequence": 24 delivered 1920x1080 .y4m frames (8-bit I420, a pan) at factor 2 of a Mitchell state against a box state, with a pinned
     download a frame; host clock around each whole sequence, in turn.
 (3) "headline" (with --parent DIR, a built checkout of the parent commit): bench.py --gpus 1 --steps 20 --warmup 3 of this tree and of the
     parent's in turn, three runs each, and the frame path's build key of both, which must be equal - the new kernel is in the set-up
     module only.
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path, one frame at a time).  Every section is a child process of its own
under a time limit of its own, started only if the one before it ended well: a fault, an abort or a time limit ends the probe there, and
what was measured until then is on file.  HIP events on a stream of the library's own runtime for (1), WARMUP rounds untimed, STEPS timed
one by one in turn, the median (min, p90).  Nothing is gated on a time: nobody had measured this kernel."""
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
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer, filter_taps, yuv420_bytes  # noqa: E402
from geodesic_raytracing_amd.render import camera_path  # noqa: E402
from tools.present_yuv_probe import alternating, kerr, shader_clock  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZE = (3840, 2160)
FACTORS = (1, 2, 4)
WARMUP, STEPS = 5, 30   # (present_yuv_probe.alternating's counts are the same)
SEQUENCE_SIZE, SEQUENCE, SEQUENCE_FACTOR, SEQUENCE_ROUNDS = (1920, 1080), 24, 2, 2
BENCH_ARGS, BENCH_RUNS = ["--gpus", "1", "--steps", "20", "--warmup", "3"], 3
SECTIONS = {"launch": 300, "sequence": 300, "headline": 900}   # name: seconds the child may take


def section_launch(stream, _parent):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    lines = [f"(1) the launch alone, {w}x{h} output; substituted program {prog.build_key} (the frame path's build key); {WARMUP} warm-up + {STEPS} timed "
             f"launches each, in turn, HIP events, median (min, p90); kernels/filter.hip with a 32 x 8 tile, the rows pass served by the vector L1",
             f"    shader clock before: {shader_clock()}"]
    for f in FACTORS:
        tw, th = w * f, h * f
        read_bytes, frame_bytes = tw * th * 16, w * h * 16
        plain = gra.RenderState(tw, th, 0)
        traced, out = DeviceBuffer(0, read_bytes), DeviceBuffer(0, frame_bytes)
        copy_bytes = (read_bytes + frame_bytes) // 2
        copy_src, copy_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
        check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(copy_bytes // 4, dtype=np.float32).ctypes.data_as(ctypes.c_void_p), copy_bytes))
        plain.render(prog, metric, gra.default_camera(), traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        del plain
        tables = {name: filter_taps(name, f) for name in ("mitchell", "tent")}

        def filtered(name):
            taps = tables[name]
            return lambda: check(lib.gr_resolve_filtered(prog.handle, stream, traced.ptr, out.ptr, w, h, f, taps.ctypes.data_as(ctypes.c_void_p), len(taps)))

        def resolve():
            check(lib.gr_resolve_supersampled(prog.handle, stream, traced.ptr, out.ptr, w, h, f, h, 0, 1, 0))

        def copy():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, copy_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice

        t = alternating(timer, {"mitchell": filtered("mitchell"), "resolve": resolve, "tent": filtered("tent"), "resolve again": resolve, "copy": copy})
        m = {k: float(np.median(v)) for k, v in t.items()}
        traffic = read_bytes + frame_bytes
        n_mitchell, n_tent = len(tables["mitchell"]), len(tables["tent"])
        lines += ["", f"    factor {f} (source {tw}x{th}): the algorithmic traffic is {read_bytes / 1e6:.0f} MB read + {frame_bytes / 1e6:.0f} MB written",
                  f"    gr_resolve_filtered, mitchell ({n_mitchell:2d} taps)  {say(t['mitchell'])}   {traffic / m['mitchell'] / 1e6:7.0f} GB/s of that traffic",
                  f"    gr_resolve_filtered, tent     ({n_tent:2d} taps)  {say(t['tent'])}   {traffic / m['tent'] / 1e6:7.0f} GB/s of that traffic",
                  f"    gr_resolve_supersampled (box)            {say(t['resolve'])}   {traffic / m['resolve'] / 1e6:7.0f} GB/s read + written",
                  f"    gr_resolve_supersampled again            {say(t['resolve again'])}   (|again - first| = {abs(m['resolve again'] - m['resolve']):.4f} ms: the session's spread)",
                  f"    hipMemcpyAsync D2D of {copy_bytes / 1e6:5.0f} MB           {say(t['copy'])}   {2 * copy_bytes / m['copy'] / 1e6:7.0f} GB/s read + written",
                  f"    mitchell / box = {m['mitchell'] / m['resolve']:.2f}, mitchell / copy = {m['mitchell'] / m['copy']:.2f};  tent / box = {m['tent'] / m['resolve']:.2f}, "
                  f"tent / copy = {m['tent'] / m['copy']:.2f}"]
        del traced, out, copy_src, copy_dst
    lines.append(f"    shader clock after:  {shader_clock()}")
    return lines


def section_sequence(stream, _parent):
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED)
    w, h = SEQUENCE_SIZE
    cameras = [gra.default_camera(position, quat) for position, quat in camera_path([0, 0, -8, 0], None, [0, 3, -6, 0], None, SEQUENCE)]
    n = yuv420_bytes(w, h)
    states = {"mitchell": gra.RenderState(w, h, 0, supersample=SEQUENCE_FACTOR, filter="mitchell"), "box": gra.RenderState(w, h, 0, supersample=SEQUENCE_FACTOR)}
    out, pinned = DeviceBuffer(0, n), PinnedBuffer(n)
    lines = [f"(2) {SEQUENCE} delivered .y4m frames (8-bit I420) of {w}x{h} at factor {SEQUENCE_FACTOR}, a pan, a Mitchell state against a box state; substituted "
             f"program {prog.build_key}; host clock around each whole sequence, the two in turn, 1 warm-up + {SEQUENCE_ROUNDS} timed sequences each"]

    def sequence(state):
        for cam in cameras:
            state.render_yuv420(prog, metric, cam, out.ptr, bg, feats, cfgv, opts, stream)
            pinned.download_async(stream, out.ptr, n)
            check(lib.gr_stream_synchronize(stream))

    times = {name: [] for name in states}
    for k in range(1 + SEQUENCE_ROUNDS):
        for name, state in states.items():
            t0 = time.perf_counter()
            sequence(state)
            if k:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, what in (("mitchell", "gr_resolve_filtered + gr_present_yuv420 at factor 1"), ("box", "gr_present_yuv420 at factor 2")):
        lines.append(f"    {name:9s} {med[name]:9.2f} ms a sequence (min {min(times[name]):.2f}, max {max(times[name]):.2f}), {med[name] / SEQUENCE:.3f} ms a frame   ({what})")
    lines.append(f"    mitchell / box = {med['mitchell'] / med['box']:.3f}")
    pinned.free()
    return lines


def bench_line(tree):
    """one bench.py run of a tree in a child process: its JSON result line"""
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + BENCH_ARGS, cwd=tree, capture_output=True, text=True, timeout=280)
    if r.returncode != 0:
        raise SystemExit(f"filter_probe: bench.py of {tree} failed ({r.returncode}):\n{r.stdout[-1000:]}{r.stderr[-3000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def section_headline(_stream, parent):
    if not parent:
        return ["(3) the headline: not run (no --parent DIR given)"]
    runs = {"this": [], "parent": []}
    for _ in range(BENCH_RUNS):
        for name, tree in (("this", ROOT), ("parent", os.path.abspath(parent))):
            runs[name].append(bench_line(tree))
    lines = [f"(3) the headline, bench.py {' '.join(BENCH_ARGS)}, this tree and the parent commit's in turn, {BENCH_RUNS} runs each"]
    for name in ("this", "parent"):
        keys = sorted({r["config"]["build_key"] for r in runs[name]})
        values = " / ".join(f"{r['value']:.4f}" for r in runs[name])
        lines.append(f"    {name:6s}  {values} {runs[name][0]['unit']}   frame-path build key {', '.join(keys)}")
    tk, pk = ({r["config"]["build_key"] for r in runs[name]} for name in ("this", "parent"))
    mt, mp = (float(np.median([r["value"] for r in runs[name]])) for name in ("this", "parent"))
    lines.append(f"    build keys {'equal' if pk == tk and len(pk) == 1 else 'DIFFERENT'};  this / parent = {mt / mp:.4f} (medians)")
    return lines


def child(section, parent):
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("filter_probe: no GPU (there is nothing to measure without one)")
    stream = None
    if section != "headline":   # (the benchmark's children open the device themselves)
        stream = ctypes.c_void_p()
        check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    lines = {"launch": section_launch, "sequence": section_sequence, "headline": section_headline}[section](stream, parent)
    if stream is not None:
        check(lib.gr_stream_destroy(stream))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_resolve.txt"))
    ap.add_argument("--parent", default="", metavar="DIR", help="a built checkout of the parent commit: section (3)")
    ap.add_argument("--section", choices=sorted(SECTIONS), default=None, help="run this section in this process and print it (what the probe starts for each)")
    a = ap.parse_args()
    if a.section:
        child(a.section, a.parent)
        return 0
    text = ["filter_probe: kerr_boyer a = 0.45, fused path, one frame in flight"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for section, limit in SECTIONS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--section", section, "--parent", a.parent], cwd=ROOT, capture_output=True, text=True,
                               timeout=limit)
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
