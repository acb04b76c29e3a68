"""What PNG frames encoded on the device cost (GPU box):
    PYTHONPATH=. python tools/png_probe.py [--out profiles/png_frames.txt]
At 3840x2160 and 1920x1080, on a rendered Kerr frame (scripts/kerr_boyer.js, a = 0.45, fused path) over the synthetic sky, plain and with
redshift, one frame already on the device as RGBA8 (gr_render_frame_rgba8):
 - the two launches of an encode, gr_png_histogram and gr_png_pack (kernels/png.hip), by the events the encoder brackets them with;
 - the whole gr_png_encode_rgba8 call on the host's clock (it ends in a stream synchronise): both launches, both round trips, the table
   built on the host, the container and its CRC;
 - a device-to-device hipMemcpyAsync of the traffic both launches have between them: each reads the frame (the pixel above comes from the
   cache), the pack writes the stream; a copy reads and writes its size, so half of (2 x frame + stream) bytes;
 - the path this replaces: the download of 4 bytes a pixel through pinned memory and gr_write_png_rgba8 (filter 0, zlib level 6, one host
   thread), on the host's clock, on the same machine;
 - both files' sizes, and a check that the device's file is the host encoder's byte for byte and decodes to the frame.
WARMUP rounds untimed, STEPS timed, the works in turn, the median (min, p90).  Host-clock figures depend on the box's CPU as much as its GPU."""
import argparse
import ctypes
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer  # noqa: E402
from geodesic_raytracing_amd.render import read_png  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
WARMUP, STEPS = 2, 7


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_frames.txt"))
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("png_probe: no GPU (there is nothing to measure without one)")
    hip = hip_runtime()
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    timer = Timer(hip, stream)
    scripts = os.path.join(os.path.dirname(gra.__file__), "scripts")
    metric = gra.Metric("kerr_boyer", scripts)
    cfgv = metric.cfg_values(a=0.45)
    prog = gra.Program(metric.argument_string(), 0)   # (redshift is a run-time feature of the dynamic program)
    packed, levels = gra.pack_background(gra.synthetic_background(2048, 1024))
    dbg = DeviceBuffer.from_numpy(0, packed)
    bg = (dbg.ptr, packed.shape[2], packed.shape[1], levels)
    camera = gra.default_camera()
    opts = gra.frame_options(mode=gra.MODE_FUSED)
    lines = [f"png_probe: kerr_boyer a = 0.45, dynamic program {prog.build_key}, fused path; {WARMUP} warm-up + {STEPS} timed rounds, the works in turn, "
             "median (min, p90); launches and the copy by HIP events, whole calls on the host's clock"]
    scratch_dir = tempfile.mkdtemp(prefix="png_probe_")

    for w, h in SIZES:
        for redshift in (0, 1):
            feats = metric.features(adaptive_sampling=0, redshift=redshift)
            state = gra.RenderState(w, h, 0)
            frame = DeviceBuffer(0, w * h * 4)
            state.render_rgba8(prog, metric, camera, frame.ptr, bg, feats, cfgv, opts, stream)
            check(lib.gr_stream_synchronize(stream))
            del state
            pixels = frame.to_numpy(np.uint8, (h, w, 4))
            encoder = gra.PngEncoder(prog, w, h)
            encoder.time_launches()
            pinned = PinnedBuffer(w * h * 4)
            host_path = os.path.join(scratch_dir, "host.png").encode()
            device_file = encoder.encode(frame.ptr, stream)
            same = device_file == gra.png_encode_host(pixels)
            check(lib.gr_write_png_rgba8(host_path, pixels.ctypes.data_as(ctypes.c_void_p), w, h))
            host_size = os.path.getsize(host_path)
            with open(os.path.join(scratch_dir, "device.png"), "wb") as f:
                f.write(device_file)
            decodes = np.array_equal(read_png(os.path.join(scratch_dir, "device.png")), pixels)
            traffic = 2 * w * h * 4 + len(device_file)
            copy_bytes = traffic // 2 // 16 * 16
            copy_src, copy_dst = DeviceBuffer(0, copy_bytes), DeviceBuffer(0, copy_bytes)
            check(lib.gr_device_upload(0, copy_src.ptr, np.zeros(copy_bytes, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p), copy_bytes))

            def copy():
                assert hip.hipMemcpyAsync(copy_dst.ptr, copy_src.ptr, copy_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice

            def device_path():
                encoder.encode(frame.ptr, stream)

            def parent_path():
                pinned.download_async(stream, frame.ptr, w * h * 4)
                check(lib.gr_stream_synchronize(stream))
                check(lib.gr_write_png_rgba8(host_path, ctypes.c_void_p(pinned.ptr.value), w, h))

            t = {"histogram": [], "pack": [], "encode": [], "copy": [], "parent": []}
            for step in range(WARMUP + STEPS):
                t0 = time.perf_counter()
                device_path()
                t1 = time.perf_counter()
                launches = encoder.launch_ms()
                c = timer.one(copy)
                t2 = time.perf_counter()
                parent_path()
                t3 = time.perf_counter()
                if step >= WARMUP:
                    t["histogram"].append(launches[0])
                    t["pack"].append(launches[1])
                    t["encode"].append((t1 - t0) * 1e3)
                    t["copy"].append(c)
                    t["parent"].append((t3 - t2) * 1e3)
            t = {k: np.sort(np.array(v)) for k, v in t.items()}
            med = {k: float(np.median(v)) for k, v in t.items()}
            lines += ["", f"{w}x{h}, redshift {redshift}: frame {w * h * 4 / 1e6:.1f} MB raw; device file {len(device_file) / 1e6:.2f} MB, host writer's file {host_size / 1e6:.2f} MB "
                          f"(device / host = {len(device_file) / host_size:.2f}); device file {'equals' if same else 'DIFFERS FROM'} the host encoder's, "
                          f"{'decodes to the frame' if decodes else 'DOES NOT DECODE TO THE FRAME'}",
                      f"    gr_png_histogram                         {say(t['histogram'])}",
                      f"    gr_png_pack                              {say(t['pack'])}",
                      f"    hipMemcpyAsync D2D of {copy_bytes / 1e6:5.1f} MB           {say(t['copy'])}   (both launches / copy = {(med['histogram'] + med['pack']) / med['copy']:.1f})",
                      f"    gr_png_encode_rgba8, whole call          {say(t['encode'])}",
                      f"    download 4 B a pixel + gr_write_png_rgba8 {say(t['parent'])}   (device path / this = {med['encode'] / med['parent']:.3f})"]
            print("\n".join(lines[-6:]), flush=True)
            pinned.free()
            encoder.close()
            del frame, copy_src, copy_dst
    check(lib.gr_stream_destroy(stream))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
