"""What the meter and the tone curve cost (GPU box):
    PYTHONPATH=. python tools/tone_probe.py [--out profiles/tone_meter.txt]
On two 3840x2160 float4 frames - a rendered Kerr frame over 200 000 stars, where nearly all pixels fall into `black` or one or two bins, and
a rendered Kerr frame over a sky image, where the bins are spread: gr_meter_frame (the zeroing of the 385 counters and gr_meter_histogram,
kernels/tone.hip), gr_meter_solve_device (one wave) and gr_apply_tone (filmic, the gain from the device word), each against the yardstick
the glare's probe used: one factor-1 gr_resolve_supersampled launch of the same frame - a frame read and a frame written; the histogram
reads the frame and writes next to nothing, half that traffic.  The occupied bins of each frame are counted from the host histogram.  The
shader clock the driver reports (read, never set) before and after.
Kerr (scripts/kerr_boyer.js, a = 0.45, substituted program, fused path).  The measurement is a child process of its own under a time
limit: a fault, an abort or a time limit ends the probe, and what was printed until then is on file.  HIP events on a stream of the
library's own runtime, WARMUP rounds untimed, STEPS timed one by one in turn, the median (min, p90).  Nothing is gated on a time: nobody
had measured these kernels."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, apply_tone, meter_frame, meter_histogram, meter_solve_device  # noqa: E402
from tools.present_yuv_probe import alternating, kerr, shader_clock  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZE = (3840, 2160)
WARMUP, STEPS = 5, 30   # (present_yuv_probe.alternating's counts are the same)
LIMIT = 300             # seconds the child may take


def measure(stream):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    frame_bytes = w * h * 16
    cat = gra.StarCatalogue.random(prog, 7, 200000)
    states = {"stars": (gra.RenderState(w, h, 0, stars=(gra.StarSky(), cat, cat)), None), "sky image": (gra.RenderState(w, h, 0), bg)}
    dst = DeviceBuffer(0, frame_bytes)
    words = DeviceBuffer.from_numpy(0, np.zeros(32 // 4 + 385, dtype=np.uint32))   # a gr_tone_state, then the counters
    counters, gain = ctypes.c_void_p(words.ptr.value + 32), ctypes.c_void_p(words.ptr.value + gra.ToneStateStruct.gain.offset)
    tone = gra.tone(auto=True, curve="filmic")
    lines = [f"gr_meter_frame, gr_meter_solve_device and gr_apply_tone alone, {w}x{h} float4 ({frame_bytes / 1e6:.0f} MB a frame); substituted program {prog.build_key} "
             f"(the frame path's build key); {WARMUP} warm-up + {STEPS} timed rounds, in turn, HIP events, median (min, p90); kernels/tone.hip: 1024 workgroups of 256 lanes, "
             "tiles of 1024 pixels, a sub-histogram a wave in LDS, `black` and two peeled values a wave",
             f"    shader clock before: {shader_clock()}"]
    for name, (state, sky) in states.items():
        src = DeviceBuffer(0, frame_bytes)
        state.render(prog, metric, gra.default_camera(), src.ptr, sky, feats, cfgv, opts, stream)
        check(lib.gr_stream_synchronize(stream))
        hist = meter_histogram(src.to_numpy(np.float32, (h, w, 4)))
        top = np.sort(hist)[::-1]
        works = {"meter": lambda src=src: meter_frame(prog, src.ptr, w, h, counters, stream),
                 "copy": lambda src=src: check(lib.gr_resolve_supersampled(prog.handle, stream, src.ptr, dst.ptr, w, h, 1, h, 0, 1, 0)),
                 "solve": lambda: meter_solve_device(prog, counters, tone, words.ptr, stream),
                 "tone": lambda src=src: apply_tone(prog, src.ptr, dst.ptr, w, h, tone, gain, 1.0, stream)}
        t = alternating(timer, works)
        m = {k: float(np.median(v)) for k, v in t.items()}
        lines += [f"    {name}: {int((hist > 0).sum())} counters occupied, black {100 * hist[384] / hist.sum():.1f} %, the two fullest {100 * top[:2].sum() / hist.sum():.1f} % of the pixels",
                  f"        gr_meter_frame (memset + histogram)      {say(t['meter'])}   meter / copy = {m['meter'] / m['copy']:.2f}; {frame_bytes / m['meter'] / 1e6:.0f} GB/s read",
                  f"        gr_resolve_supersampled, factor 1       {say(t['copy'])}   {2 * frame_bytes / m['copy'] / 1e6:.0f} GB/s read + written",
                  f"        gr_meter_solve_device (one wave)        {say(t['solve'])}   solve / copy = {m['solve'] / m['copy']:.2f}",
                  f"        gr_apply_tone, filmic, device gain      {say(t['tone'])}   tone / copy = {m['tone'] / m['copy']:.2f}"]
    lines += [f"    shader clock after:  {shader_clock()}"]
    return lines


def child():
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("tone_probe: no GPU (there is nothing to measure without one)")
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    lines = measure(stream)
    check(lib.gr_stream_destroy(stream))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone_meter.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process and print (what the probe starts)")
    a = ap.parse_args()
    if a.child:
        child()
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, capture_output=True, text=True, timeout=LIMIT)
        code, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:
        code, out, err = 124, (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), f"time limit of {LIMIT} s"
    text = ["tone_probe: kerr_boyer a = 0.45, fused path", "", out.rstrip()] + ([] if code == 0 else [f"the measurement ended with status {code}", err[-3000:]])
    print("\n".join(text), flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if code == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
