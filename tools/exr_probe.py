"""What OpenEXR frames encoded on the device cost (GPU box):
    PYTHONPATH=. python tools/exr_probe.py [--out profiles/exr_frames.txt]
At 3840x2160, on the README's Kerr star-sky frame (scripts/kerr_boyer.js, a = 0.45, fused path, --sky stars:200000:7), one float4 frame
already on the device (gr_render_frame):
 - the file's size against the float4 download (16 bytes a pixel) and against raw halfs (6 bytes a pixel), and how many rows are stored raw;
 - the two launches of an encode, gr_exr_histogram and gr_exr_pack (kernels/exr.hip), by the events the encoder brackets them with;
 - frame to file bytes in host memory, the whole gr_exr_encode_f32 call on the host's clock (it ends in a stream synchronise): both
   launches, both round trips, the table and the offsets made on the host, the copy out of the staging buffer;
 - what that replaces when the same pixels are wanted on the host: gr_device_download of the float4 frame (into pageable memory, as
   DeviceBuffer.to_numpy does it), and the same download through pinned memory; and, for scale, the host encoder on the downloaded frame;
 - a check that the device's file is the host encoder's byte for byte.
WARMUP rounds untimed, STEPS timed, the works in turn, the median (min, p90).  Host-clock figures depend on the box's CPU as much as its GPU."""
import argparse
import ctypes
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer  # noqa: E402
from geodesic_raytracing_amd.render import StarField  # noqa: E402
from tools.supersample_probe import say  # noqa: E402

WARMUP, STEPS = 3, 11


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exr_frames.txt"))
    ap.add_argument("--size", default="3840x2160")
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("exr_probe: no GPU (there is nothing to measure without one)")
    w, h = (int(v) for v in a.size.lower().split("x"))
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    scripts = os.path.join(os.path.dirname(gra.__file__), "scripts")
    metric = gra.Metric("kerr_boyer", scripts)
    cfgv = metric.cfg_values(a=0.45)
    prog = gra.Program(metric.argument_string(), 0)
    state = gra.RenderState(w, h, 0, stars=StarField(200000, 7).on(prog))
    frame = DeviceBuffer(0, w * h * 16)
    state.render(prog, metric, gra.default_camera(), frame.ptr, None, metric.features(adaptive_sampling=0), cfgv, gra.frame_options(mode=gra.MODE_FUSED), stream)
    check(lib.gr_stream_synchronize(stream))
    del state
    pixels = frame.to_numpy(np.float32, (h, w, 4))
    encoder = gra.ExrEncoder(prog, w, h)
    encoder.time_launches()
    device_file = encoder.encode(frame.ptr, stream)
    t0 = time.perf_counter()
    host_file = gra.exr_encode_host(pixels)
    host_encoder_ms = (time.perf_counter() - t0) * 1e3
    same = device_file == host_file
    at, raw_rows = 313 + 8 * h, 0
    for _ in range(h):
        (size,) = struct.unpack("<i", device_file[at + 4:at + 8])
        raw_rows += size == 6 * w
        at += 8 + size
    pinned = PinnedBuffer(w * h * 16)
    pageable = np.empty((h, w, 4), np.float32)

    def download():
        check(lib.gr_device_download(0, pageable.ctypes.data_as(ctypes.c_void_p), frame.ptr, pageable.nbytes))

    def download_pinned():
        pinned.download_async(stream, frame.ptr, w * h * 16)
        check(lib.gr_stream_synchronize(stream))

    t = {"histogram": [], "pack": [], "encode": [], "download": [], "pinned": []}
    for step in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        encoder.encode(frame.ptr, stream)
        t1 = time.perf_counter()
        launches = encoder.launch_ms()
        t2 = time.perf_counter()
        download()
        t3 = time.perf_counter()
        download_pinned()
        t4 = time.perf_counter()
        if step >= WARMUP:
            t["histogram"].append(launches[0])
            t["pack"].append(launches[1])
            t["encode"].append((t1 - t0) * 1e3)
            t["download"].append((t3 - t2) * 1e3)
            t["pinned"].append((t4 - t3) * 1e3)
    t = {k: np.sort(np.array(v)) for k, v in t.items()}
    med = {k: float(np.median(v)) for k, v in t.items()}
    lines = [f"exr_probe: kerr_boyer a = 0.45, dynamic program {prog.build_key}, fused path, star sky 200000:7; {WARMUP} warm-up + {STEPS} timed rounds, the "
             "works in turn, median (min, p90); launches by HIP events, whole calls on the host's clock", "",
             f"{w}x{h}: float4 frame {w * h * 16 / 1e6:.1f} MB, raw halfs {w * h * 6 / 1e6:.1f} MB; file {len(device_file) / 1e6:.2f} MB "
             f"({len(device_file) / (w * h * 16):.3f} of the float4 frame, {len(device_file) / (w * h * 6):.3f} of the raw halfs), {raw_rows} of {h} rows stored raw; "
             f"frame maximum {float(np.nanmax(pixels[..., :3])):.1f}; device file {'equals' if same else 'DIFFERS FROM'} the host encoder's",
             f"    gr_exr_histogram                              {say(t['histogram'])}",
             f"    gr_exr_pack                                   {say(t['pack'])}",
             f"    gr_exr_encode_f32, frame to file bytes        {say(t['encode'])}",
             f"    gr_device_download of the float4 frame        {say(t['download'])}   (device path / this = {med['encode'] / med['download']:.3f})",
             f"    ... through pinned memory                     {say(t['pinned'])}   (device path / this = {med['encode'] / med['pinned']:.3f})",
             f"    gr_exr_encode_f32_host of the downloaded frame, once: {host_encoder_ms:.0f} ms (one host thread)"]
    print("\n".join(lines), flush=True)
    pinned.free()
    encoder.close()
    check(lib.gr_stream_destroy(stream))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
