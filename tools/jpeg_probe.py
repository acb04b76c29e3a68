"""What JPEG frames encoded on the device cost (GPU box):
    PYTHONPATH=. python tools/jpeg_probe.py [--out profiles/jpeg_frames.txt]
At 3840x2160 and 1920x1080, quality 90, on a rendered Kerr frame (scripts/kerr_boyer.js, a = 0.45, fused path) over the synthetic sky, one
frame already on the device as RGBA8 (gr_render_frame_rgba8):
 - the three launches of an encode, gr_jpeg_blocks, gr_jpeg_pack and gr_jpeg_gather (kernels/jpeg.hip), by the events the encoder brackets
   them with, and the bytes that come back;
 - the whole gr_jpeg_encode_rgba8 call on the host's clock (it ends in a stream synchronise);
 - a frame end to end: gr_render_frame_rgba8 and the encode behind it on one stream, on the host's clock;
 - gr_png_encode_rgba8 of the same frame, whole call (--png device), and its file's size;
 - the path this replaces: the download of 4 bytes a pixel through pinned memory and PIL's (libjpeg's) encode at the same quality and 4:2:0,
   one host thread, on the same machine - left out where PIL is missing;
 - a check that the device's file is the host encoder's byte for byte.
WARMUP rounds untimed, STEPS timed, the works in turn, the median (min, p90).  Host-clock figures depend on the box's CPU as much as its GPU."""
import argparse
import ctypes
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer, PinnedBuffer  # noqa: E402
from tools.supersample_probe import say  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
QUALITY = 90
WARMUP, STEPS = 2, 7


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_frames.txt"))
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("jpeg_probe: no GPU (there is nothing to measure without one)")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    scripts = os.path.join(os.path.dirname(gra.__file__), "scripts")
    metric = gra.Metric("kerr_boyer", scripts)
    cfgv = metric.cfg_values(a=0.45)
    prog = gra.Program(metric.argument_string(), 0)
    packed, levels = gra.pack_background(gra.synthetic_background(2048, 1024))
    dbg = DeviceBuffer.from_numpy(0, packed)
    bg = (dbg.ptr, packed.shape[2], packed.shape[1], levels)
    camera = gra.default_camera()
    opts = gra.frame_options(mode=gra.MODE_FUSED)
    feats = metric.features(adaptive_sampling=0)
    lines = [f"jpeg_probe: kerr_boyer a = 0.45, dynamic program {prog.build_key}, fused path, quality {QUALITY}; {WARMUP} warm-up + {STEPS} timed rounds, "
             "the works in turn, median (min, p90); launches by HIP events, whole calls on the host's clock"]
    for w, h in SIZES:
        state = gra.RenderState(w, h, 0)
        frame = DeviceBuffer(0, w * h * 4)

        def render_frame():
            state.render_rgba8(prog, metric, camera, frame.ptr, bg, feats, cfgv, opts, stream)

        render_frame()
        check(lib.gr_stream_synchronize(stream))
        pixels = frame.to_numpy(np.uint8, (h, w, 4))
        encoder = gra.JpegEncoder(prog, w, h, QUALITY)
        encoder.time_launches()
        png = gra.PngEncoder(prog, w, h)
        pinned = PinnedBuffer(w * h * 4)
        device_file = encoder.encode(frame.ptr, stream)
        same = device_file == gra.jpeg_encode_host(pixels, QUALITY)
        png_size = len(png.encode(frame.ptr, stream))
        pil_size = [0]

        def parent_path():
            pinned.download_async(stream, frame.ptr, w * h * 4)
            check(lib.gr_stream_synchronize(stream))
            file = io.BytesIO()
            Image.fromarray(pinned.view(np.uint8, (h, w, 4))[..., :3]).save(file, "JPEG", quality=QUALITY, subsampling=2)
            pil_size[0] = file.tell()

        t = {k: [] for k in ("blocks", "pack", "gather", "encode", "frame", "png", "parent")}
        for step in range(WARMUP + STEPS):
            t0 = time.perf_counter()
            encoder.encode(frame.ptr, stream)
            t1 = time.perf_counter()
            launches = encoder.launch_ms()
            t2 = time.perf_counter()
            render_frame()
            encoder.encode(frame.ptr, stream)
            t3 = time.perf_counter()
            png.encode(frame.ptr, stream)
            t4 = time.perf_counter()
            if Image is not None:
                parent_path()
            t5 = time.perf_counter()
            if step >= WARMUP:
                for k, v in zip(t, (*launches, (t1 - t0) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3)):
                    t[k].append(v)
        t = {k: np.sort(np.array(v)) for k, v in t.items()}
        lines += ["", f"{w}x{h}: frame {w * h * 4 / 1e6:.1f} MB raw; device JPEG {len(device_file) / 1e6:.3f} MB shipped ({'equals' if same else 'DIFFERS FROM'} the host "
                      f"encoder's), device PNG {png_size / 1e6:.2f} MB, PIL's JPEG {pil_size[0] / 1e6:.3f} MB",
                  f"    gr_jpeg_blocks                            {say(t['blocks'])}",
                  f"    gr_jpeg_pack                              {say(t['pack'])}",
                  f"    gr_jpeg_gather                            {say(t['gather'])}",
                  f"    gr_jpeg_encode_rgba8, whole call          {say(t['encode'])}",
                  f"    gr_render_frame_rgba8 + the encode        {say(t['frame'])}",
                  f"    gr_png_encode_rgba8, whole call           {say(t['png'])}",
                  f"    download 4 B a pixel + PIL's encode       {say(t['parent']) if Image is not None else 'PIL is not installed here'}"]
        print("\n".join(lines[-8:]), flush=True)
        assert encoder.scratch_intact()
        pinned.free()
        encoder.close()
        png.close()
        del frame, state
    check(lib.gr_stream_destroy(stream))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
