"""What the glare costs (GPU box):
    PYTHONPATH=. python tools/glare_probe.py [--out profiles/glare_apply.txt]
On a 3840x2160 float4 frame - a rendered Kerr frame over a star sky, so that the values are a picture's: gr_apply_glare (kernels/glare.hip)
for the PSF of --glare 0.06:1.5,0.03:10 (two components of 11 and 61 taps: four launches), for one component of 129 taps (two launches)
and for an exposure alone (one launch), each against as many factor-1 gr_resolve_supersampled launches of the same frame as the glare
has launches - a device copy of the traffic the algorithm needs, a frame read and a frame written a launch.  Then the time of the whole
4K Kerr frame the glare would follow (time_kernels = 0, events around the frame), for the glare's share of it.  The shader clock the
driver reports (read, never set) before and after.
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
from geodesic_raytracing_amd.pipeline import DeviceBuffer, apply_glare, glare_exposure, glare_gaussians, glare_scratch_bytes  # noqa: E402
from tools.present_yuv_probe import alternating, kerr, shader_clock  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZE = (3840, 2160)
WARMUP, STEPS = 5, 30   # (present_yuv_probe.alternating's counts are the same)
LIMIT = 300             # seconds the child may take


def measure(stream):
    hip = hip_runtime()
    timer = Timer(hip, stream)
    metric, cfgv, feats, prog, _sky, _bg = kerr()
    opts = gra.frame_options(mode=gra.MODE_FUSED, reuse_still_camera=0)
    w, h = SIZE
    frame_bytes = w * h * 16
    cat = gra.StarCatalogue.random(prog, 7, 200000)
    state = gra.RenderState(w, h, 0, stars=(gra.StarSky(), cat, cat))
    src, dst, scratch = DeviceBuffer(0, frame_bytes), DeviceBuffer(0, frame_bytes), DeviceBuffer(0, glare_scratch_bytes(w, h))

    def frame():
        state.render(prog, metric, gra.default_camera(), src.ptr, None, feats, cfgv, opts, stream)

    frame()
    check(lib.gr_stream_synchronize(stream))
    glares = {"0.06:1.5,0.03:10 (11 + 61 taps)": (glare_gaussians([1.5, 10.0], [0.06, 0.03]), 4), "one component of 129 taps": (glare_gaussians([64.0], [0.1]), 2),
              "exposure alone": (glare_exposure(glare_gaussians(), 1.0), 1)}

    def glare(g):
        return lambda: apply_glare(prog, src.ptr, dst.ptr, scratch.ptr, scratch.nbytes, w, h, g, stream)

    def copies(n):
        def work():
            for _ in range(n):
                check(lib.gr_resolve_supersampled(prog.handle, stream, src.ptr, dst.ptr, w, h, 1, h, 0, 1, 0))
        return work

    lines = [f"gr_apply_glare alone, {w}x{h} float4 ({frame_bytes / 1e6:.0f} MB a frame); substituted program {prog.build_key} (the frame path's build key); {WARMUP} "
             f"warm-up + {STEPS} timed rounds, in turn, HIP events, median (min, p90); kernels/glare.hip: rows 256 x 1 a workgroup, columns 16 x 64",
             f"    shader clock before: {shader_clock()}"]
    works = {}
    for name, (g, launches) in glares.items():
        works[name] = glare(g)
        works[f"{launches} x resolve"] = copies(launches)
    works["the 4K Kerr frame over 200 000 stars"] = frame
    t = alternating(timer, works)
    m = {k: float(np.median(v)) for k, v in t.items()}
    whole = m["the 4K Kerr frame over 200 000 stars"]
    for name, (g, launches) in glares.items():
        lines += [f"    {name:34s} {say(t[name])}   {launches} launches",
                  f"    {launches} x gr_resolve_supersampled, factor 1   {say(t[f'{launches} x resolve'])}   glare / copies = {m[name] / m[f'{launches} x resolve']:.2f}; "
                  f"{100 * m[name] / whole:.1f} % of the frame's time"]
    lines += [f"    the 4K Kerr frame, float4            {say(t['the 4K Kerr frame over 200 000 stars'])}", f"    shader clock after:  {shader_clock()}"]
    return lines


def child():
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("glare_probe: no GPU (there is nothing to measure without one)")
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    lines = measure(stream)
    check(lib.gr_stream_destroy(stream))
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glare_apply.txt"))
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
    text = ["glare_probe: kerr_boyer a = 0.45, fused path", "", out.rstrip()] + ([] if code == 0 else [f"the measurement ended with status {code}", err[-3000:]])
    print("\n".join(text), flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(text) + "\n")
    return 0 if code == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
