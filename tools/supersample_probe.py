"""What supersampling costs (GPU box):    PYTHONPATH=. python tools/supersample_probe.py [--out profiles/supersample_resolve.txt]
 (a) the resolve launch alone (gr_resolve_supersampled, kernels/resolve.hip) against a device-to-device hipMemcpyAsync of HALF the bytes the
     resolve moves - a copy reads and writes its size, so that is the same traffic: (read + write) / 2 each way;
 (b) a whole frame of a supersampled state against the frame of a plain state of the traced size (what the factor-1 path launches) and
     the resolve of (a): the expectation is plain + resolve and nothing else.
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path, one frame at a time); HIP events on a stream of the library's own
runtime, WARMUP launches untimed, STEPS timed one by one, the median (and the spread) reported."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402

CASES = [(3840, 2160, 2), (2560, 1440, 3)]   # output size, factor
WARMUP, STEPS = 5, 30


def hip_runtime():
    """the libamdhip64 the library is linked against (already mapped: the loader hands back the same copy)"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "torch" not in line})
    if not paths:
        raise RuntimeError("the library's HIP runtime is not mapped")
    hip = ctypes.CDLL(paths[0])
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    return hip


class Timer:
    def __init__(self, hip, stream):
        self.hip, self.stream = hip, stream
        self.start, self.stop = ctypes.c_void_p(), ctypes.c_void_p()
        assert hip.hipEventCreate(ctypes.byref(self.start)) == 0 and hip.hipEventCreate(ctypes.byref(self.stop)) == 0

    def one(self, work):
        assert self.hip.hipEventRecord(self.start, self.stream) == 0
        work()
        assert self.hip.hipEventRecord(self.stop, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.stop) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.start, self.stop) == 0
        return ms.value

    def alternating(self, works):
        """the launches of `works` in turn, WARMUP rounds untimed, STEPS rounds timed: {name: ms per launch, sorted}"""
        for _ in range(WARMUP):
            for work in works.values():
                self.one(work)
        times = {name: [] for name in works}
        for _ in range(STEPS):
            for name, work in works.items():
                times[name].append(self.one(work))
        return {name: np.sort(np.array(t)) for name, t in times.items()}


def say(t):
    return f"{np.median(t):8.3f} ms  (min {t[0]:.3f}, p90 {t[int(0.9 * (len(t) - 1))]:.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supersample_resolve.txt"))
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("supersample_probe: no GPU (there is nothing to measure without one)")
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
    lines = [f"supersample_probe: kerr_boyer a = 0.45, substituted program {prog.build_key}, fused path, one frame in flight; "
             f"{WARMUP} warm-up + {STEPS} timed launches each, alternating, HIP events, median (min, p90)"]

    for w, h, f in CASES:
        tw, th = w * f, h * f
        read_bytes, write_bytes = tw * th * 16, w * h * 16
        copy_bytes = (read_bytes + write_bytes) // 2
        # (a) the launch alone: a traced frame of rendered pixels, a copy of half the traffic's size
        state = gra.RenderState(w, h, 0, supersample=f)
        plain = gra.RenderState(tw, th, 0)
        traced = DeviceBuffer(0, read_bytes)
        out = DeviceBuffer(0, write_bytes)
        copy_src, copy_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
        check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(copy_bytes // 4, dtype=np.float32).ctypes.data_as(ctypes.c_void_p), copy_bytes))
        # frames repeat one camera: every frame still does its own camera set-up and prepass, as bench.py's do
        opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
        plain.render(prog, metric, camera, traced.ptr, bg, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))

        def resolve():
            check(lib.gr_resolve_supersampled(prog.handle, stream, traced.ptr, out.ptr, w, h, f, h, 0, 1, 0))

        def copy():
            assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, copy_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice

        t = timer.alternating({"resolve": resolve, "copy": copy})
        r, c = float(np.median(t["resolve"])), float(np.median(t["copy"]))
        lines += ["", f"(a) {w}x{h} output, factor {f} (traced {tw}x{th}): the resolve reads {read_bytes / 1e6:.0f} MB and writes {write_bytes / 1e6:.0f} MB",
                  f"    gr_resolve_supersampled          {say(t['resolve'])}   {(read_bytes + write_bytes) / r / 1e6:7.0f} GB/s read + written",
                  f"    hipMemcpyAsync D2D of {copy_bytes / 1e6:4.0f} MB    {say(t['copy'])}   {2 * copy_bytes / c / 1e6:7.0f} GB/s read + written",
                  f"    resolve / copy = {r / c:.2f}   (expectation: within 1.5)"]

        # (b) whole frames
        def supersampled_frame():
            state.render(prog, metric, camera, out.ptr, bg, feats, cfgv, opts, stream)

        def plain_frame():
            plain.render(prog, metric, camera, traced.ptr, bg, feats, cfgv, opts, stream)

        t = timer.alternating({"supersampled": supersampled_frame, "plain": plain_frame})
        s_ms, p_ms = float(np.median(t["supersampled"])), float(np.median(t["plain"]))
        timed = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0, time_kernels=1)
        inside = []
        for _ in range(WARMUP + STEPS):
            state.render(prog, metric, camera, out.ptr, bg, feats, cfgv, timed, stream)
            check(lib.gr_stream_synchronize(stream))
            inside.append(state.resolve_ms())
        inside = np.sort(np.array(inside[WARMUP:]))
        counted = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0, count_attempts=1)
        plain.render(prog, metric, camera, traced.ptr, bg, feats, cfgv, counted, stream)
        check(lib.gr_stream_synchronize(stream))
        lines += [f"(b) whole frames, {w}x{h} at factor {f} against {tw}x{th} plain (shader clock of the trace launch: {plain.shader_clock_mhz():.0f} MHz)",
                  f"    supersampled state               {say(t['supersampled'])}",
                  f"    plain state of the traced size   {say(t['plain'])}",
                  f"    resolve inside the frame         {say(inside)}   (gr_render_state_resolve_ms)",
                  f"    supersampled - plain = {s_ms - p_ms:.3f} ms;  resolve alone {r:.3f} ms;  unaccounted {s_ms - p_ms - r:+.3f} ms"]
        del state, plain, traced, out, copy_src, copy_dst
    check(lib.gr_stream_destroy(stream))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
