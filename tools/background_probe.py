"""What building the sky's mip slices on the device costs (GPU box):
    PYTHONPATH=. python tools/background_probe.py [--out profiles/background_build.txt] [--parent DIR]
At 4096x2048 and 8192x4096, random bytes:
 (1) gr_build_mipped_background (kernels/background.hip: the reduction's launches and the slice writer together), in place;
 (2) the floor: a device-to-device copy of w*h*4 bytes and a fill of (levels - 1)*w*h*4 bytes - together they read the image once and write
     `levels` times its size, the build's traffic without its float pyramid - and the build's ratio to it;
 (3) wall time on the host: upload of the image + device build + synchronise, against host pack (gr_pack_mipped_background, one thread)
     + upload of all slices.  With --parent DIR (a built checkout of the parent commit) the host pack is that tree's library; without, this
     tree's, whose host packer this feature does not touch.
Not taken here: the set-up module's cold build time against the parent's (every program's set-up module grows by these kernels).
HIP events on a stream of the library's own runtime, WARMUP launches untimed, STEPS timed in turn, the median (and the spread)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd import check, lib  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from tools.supersample_probe import Timer, hip_runtime, say  # noqa: E402

SIZES = [(4096, 2048), (8192, 4096)]
WARMUP, STEPS = 5, 30
WALL_ROUNDS = 3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_build.txt"))
    ap.add_argument("--parent", default="", metavar="DIR", help="a built checkout of the parent commit: its library packs on the host in (3)")
    a = ap.parse_args()
    n = ctypes.c_int(0)
    if lib.gr_device_count(ctypes.byref(n)) != 0 or n.value < 1:
        raise SystemExit("background_probe: no GPU (there is nothing to measure without one)")
    hip = hip_runtime()
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    stream = ctypes.c_void_p()
    check(lib.gr_stream_create(0, 0, ctypes.byref(stream)))
    timer = Timer(hip, stream)
    host_lib = lib
    if a.parent:
        host_lib = ctypes.CDLL(os.path.join(a.parent, "geodesic_raytracing_amd", "libgeodesic_hip.so"))
        host_lib.gr_pack_mipped_background.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    metric = gra.Metric("kerr_boyer", os.path.join(os.path.dirname(gra.__file__), "scripts"))
    prog = gra.Program(metric.argument_string(), 0)
    lines = [f"background_probe: random RGBA8 skies; {WARMUP} warm-up + {STEPS} timed rounds, in turn, HIP events, median (min, p90); wall times: "
             f"host clock, {WALL_ROUNDS} rounds after one untimed, median; host pack by {'the parent tree ' + a.parent if a.parent else 'this tree'}"]
    for w, h in SIZES:
        rgba = np.random.RandomState(w).randint(0, 256, size=(h, w, 4)).astype(np.uint8)
        levels = lib.gr_pack_mipped_background(None, w, h, None)
        need = ctypes.c_size_t()
        check(lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)))
        image_bytes = rgba.nbytes
        packed, scratch = DeviceBuffer(0, levels * image_bytes), DeviceBuffer(0, need.value)
        image, floor_out = DeviceBuffer.from_numpy(0, rgba), DeviceBuffer(0, levels * image_bytes)
        check(lib.gr_device_upload(0, packed.ptr, rgba.ctypes.data_as(ctypes.c_void_p), image_bytes))

        def build():
            assert lib.gr_build_mipped_background(prog.handle, stream, packed.ptr, w, h, packed.ptr, scratch.ptr, need.value) == levels

        def floor():
            assert hip.hipMemcpyAsync(floor_out.ptr, image.ptr, image_bytes, 3, stream) == 0   # hipMemcpyDeviceToDevice
            assert hip.hipMemsetAsync(ctypes.c_void_p(floor_out.ptr.value + image_bytes), 0x5C, (levels - 1) * image_bytes, stream) == 0

        def floor_again():   # the same twice in every round: the spread between two equal works in this session
            floor()

        for _ in range(WARMUP):
            for work in (build, floor, floor_again):
                timer.one(work)
        times = {"build": [], "copy + fill": [], "copy + fill again": []}
        for _ in range(STEPS):
            for name, work in zip(times, (build, floor, floor_again)):
                times[name].append(timer.one(work))
        times = {name: np.sort(np.array(t)) for name, t in times.items()}
        moved = (image_bytes + levels * image_bytes) / 1e9
        lines.append(f"{w}x{h}, {levels} levels: reads {image_bytes / 1e6:.1f} MB, writes {levels * image_bytes / 1e6:.1f} MB packed (+ {need.value / 1e6:.1f} MB of float pyramid written and read)")
        for name, t in times.items():
            lines.append(f"  {name:18s} {say(t)}   {moved / (np.median(t) * 1e-3):8.0f} GB/s of the packed traffic")
        lines.append(f"  build / floor: {np.median(times['build']) / np.median(times['copy + fill']):.2f}")

        def device_wall():
            t0 = time.perf_counter()
            check(lib.gr_device_upload(0, packed.ptr, rgba.ctypes.data_as(ctypes.c_void_p), image_bytes))
            build()
            check(lib.gr_stream_synchronize(stream))
            return (time.perf_counter() - t0) * 1e3

        host_out = np.empty((levels, h, w, 4), dtype=np.uint8)

        def host_wall():
            t0 = time.perf_counter()
            assert host_lib.gr_pack_mipped_background(rgba.ctypes.data_as(ctypes.c_void_p), w, h, host_out.ctypes.data_as(ctypes.c_void_p)) == levels
            t1 = time.perf_counter()
            check(lib.gr_device_upload(0, floor_out.ptr, host_out.ctypes.data_as(ctypes.c_void_p), host_out.nbytes))
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        device_wall()
        dev = np.median([device_wall() for _ in range(WALL_ROUNDS)])
        host_wall()
        host = np.array([host_wall() for _ in range(WALL_ROUNDS)])
        pack, upload = np.median(host[:, 0]), np.median(host[:, 1])
        same = packed.to_numpy(np.uint8, host_out.shape).tobytes() == host_out.tobytes()
        lines.append(f"  wall: upload + device build {dev:.2f} ms; host pack {pack:.1f} ms + upload of {levels} slices {upload:.1f} ms = {pack + upload:.1f} ms "
                     f"({(pack + upload) / dev:.0f} x); bytes {'identical' if same else 'DIFFERENT'}")
        del packed, scratch, image, floor_out
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    check(lib.gr_stream_destroy(stream))


if __name__ == "__main__":
    main()
