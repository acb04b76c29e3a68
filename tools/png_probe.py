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
WARMUP rounds untimed, STEPS timed, the works in turn, the median (min, p90).  Host-clock figures depend on the box's CPU as much as its GPU.

    PYTHONPATH=. python tools/png_probe.py --streams [--out profiles/png_runs.txt]
The two stream kinds against each other on the same four frames (GR_PNG_STREAM_RUNS: previous-pixel run matches): the sizes of the runs
file, the literal file and the host writer's file - the yardstick -, with a plain statement which side of it the runs file is; the two
launches and the whole gr_png_encode_rgba8 call of a runs encoder, of a literals encoder and of a second literals encoder - the spread
between two equal works -, in turn in the same session, with the shader clock read before and after; and a check that each device file is
its kind's host file and decodes to the frame."""
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


def streams(out_path):
    """the --streams report"""
    from tools.present_yuv_probe import shader_clock
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    scripts = os.path.join(os.path.dirname(gra.__file__), "scripts")
    metric = gra.Metric("kerr_boyer", scripts)
    cfgv = metric.cfg_values(a=0.45)
    prog = gra.Program(metric.argument_string(), 0)
    packed, levels = gra.pack_background(gra.synthetic_background(2048, 1024))
    dbg = DeviceBuffer.from_numpy(0, packed)
    bg = (dbg.ptr, packed.shape[2], packed.shape[1], levels)
    rounds_warm, rounds = 3, 15
    lines = [f"png_probe --streams: kerr_boyer a = 0.45, dynamic program {prog.build_key}, fused path; {rounds_warm} warm-up + {rounds} timed rounds, the "
             "three encoders in turn in every round, median (min, p90); launches by HIP events, whole calls on the host's clock",
             f"shader clock before: {shader_clock()}"]
    scratch_dir = tempfile.mkdtemp(prefix="png_probe_")
    for w, h in SIZES:
        for redshift in (0, 1):
            feats = metric.features(adaptive_sampling=0, redshift=redshift)
            state = gra.RenderState(w, h, 0)
            frame = DeviceBuffer(0, w * h * 4)
            state.render_rgba8(prog, metric, gra.default_camera(), frame.ptr, bg, feats, cfgv, gra.frame_options(mode=gra.MODE_FUSED), stream)
            check(lib.gr_stream_synchronize(stream))
            del state
            pixels = frame.to_numpy(np.uint8, (h, w, 4))
            host_path = os.path.join(scratch_dir, "host.png")
            check(lib.gr_write_png_rgba8(host_path.encode(), pixels.ctypes.data_as(ctypes.c_void_p), w, h))
            host_size = os.path.getsize(host_path)
            encoders = {"runs": gra.PngEncoder(prog, w, h, "runs"), "literals": gra.PngEncoder(prog, w, h), "literals, again": gra.PngEncoder(prog, w, h)}
            files, verdicts = {}, {}
            for name, encoder in encoders.items():
                encoder.time_launches()
                files[name] = encoder.encode(frame.ptr, stream)
                with open(os.path.join(scratch_dir, "device.png"), "wb") as f:
                    f.write(files[name])
                same = files[name] == gra.png_encode_host(pixels, "runs" if name == "runs" else "literals")
                decodes = np.array_equal(read_png(os.path.join(scratch_dir, "device.png")), pixels)
                verdicts[name] = f"{'equals' if same else 'DIFFERS FROM'} its host encoder's file, {'decodes to the frame' if decodes else 'DOES NOT DECODE TO THE FRAME'}"
            t = {name: {"histogram": [], "pack": [], "encode": []} for name in encoders}
            for step in range(rounds_warm + rounds):
                for name, encoder in encoders.items():
                    t0 = time.perf_counter()
                    encoder.encode(frame.ptr, stream)
                    t1 = time.perf_counter()
                    launches = encoder.launch_ms()
                    if step >= rounds_warm:
                        t[name]["histogram"].append(launches[0])
                        t[name]["pack"].append(launches[1])
                        t[name]["encode"].append((t1 - t0) * 1e3)
            runs_size, literal_size = len(files["runs"]), len(files["literals"])
            lines += ["", f"{w}x{h}, redshift {redshift}: frame {w * h * 4 / 1e6:.1f} MB raw",
                      f"    files: runs {runs_size} bytes, literals {literal_size} bytes, host writer (gr_write_png_rgba8) {host_size} bytes; runs / host writer = "
                      f"{runs_size / host_size:.3f}, literals / host writer = {literal_size / host_size:.3f}, runs / literals = {runs_size / literal_size:.3f}",
                      f"    the runs file is {'BELOW' if runs_size < host_size else 'ABOVE' if runs_size > host_size else 'THE SIZE OF'} the host writer's"]
            for name in encoders:
                v = {k: np.sort(np.array(x)) for k, x in t[name].items()}
                lines += [f"    {name}: {verdicts[name]}",
                          f"        histogram launch                 {say(v['histogram'])}",
                          f"        pack launch                      {say(v['pack'])}",
                          f"        gr_png_encode_rgba8, whole call  {say(v['encode'])}"]
            print("\n".join(lines[-15:]), flush=True)
            for encoder in encoders.values():
                encoder.close()
            del frame
    lines += ["", f"shader clock after: {shader_clock()}"]
    check(lib.gr_stream_destroy(stream))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="profiles/png_frames.txt, or profiles/png_runs.txt with --streams")
    ap.add_argument("--streams", action="store_true", help="the runs stream against the literal stream and the host writer")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "png_runs.txt" if a.streams else "png_frames.txt")
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("png_probe: no GPU (there is nothing to measure without one)")
    if a.streams:
        return streams(a.out)
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
