"""Headless renderer: metric script -> PNG (the role of the reference's `-start <metric>` + screenshot key).

    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 1920x1080 --out kerr.png
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 1920x1080 --supersample 2 --out kerr_ss2.png
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --encode device --out kerr_4k.png
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --background sky.png --mips device --out kerr_sky.png
    # the PNG itself made on the device (filter, histogram, Huffman coding): only the compressed bytes come back
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --png device --out kerr_4k.png
    # one frame over four GPUs (one process, peer copies): every device traces its rows at 4 x 4 rays a pixel and ships them as 8-bit sRGB
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --devices 0,1,2,3 --supersample 4 --encode device --out poster.png
    python -m geodesic_raytracing_amd.render --metric alcubierre --redshift --camera 0,0,-6,0.5 --background sky.png --out warp.png
    # camera riding its own timelike geodesic: 24 frames, 0.5 units of proper time apart -> fall_000.png .. fall_023.png
    python -m geodesic_raytracing_amd.render --metric schwarzschild --camera 0,0,-8,0 --geodesic-speed 0,0.3,0 \
        --geodesic-time 0 --geodesic-dt 0.5 --frames 24 --out fall.png
    # the same fall as one video file: every frame leaves the device as 8-bit BT.709 Y'CbCr 4:2:0, 1.5 bytes a pixel, into uncompressed YUV4MPEG2
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --geodesic-speed 0,0.3,0 --frames 24 --out fall.y4m
    # a camera that rides no geodesic: position and orientation interpolated from --camera / --quat to --camera-to / --quat-to over --frames
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --camera-to 0,3,-6,0 --frames 48 --fps 30000/1001 --out pan.y4m
    # ... as a 10-bit master (C420p10: 16-bit little-endian words, 3 bytes a pixel come back) for a Main10 / AV1 / ProRes encode
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --camera-to 0,3,-6,0 --frames 48 --bit-depth 10 --out pan10.y4m
    # ... with motion blur: a 180-degree shutter (open for half the frame interval), every frame the average of 8 sub-frames, summed on the device
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --camera-to 0,3,-6,0 --frames 48 --shutter 0.5 --out pan_blur.y4m
    # ... the 16 rays a pixel of --supersample 4 through a Mitchell-Netravali filter of radius 2 instead of a box one pixel wide: less shimmer
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --camera-to 0,3,-6,0 --frames 48 --supersample 4 --filter mitchell --out pan_aa.y4m
    # a baseline JPEG (JFIF, 4:2:0) made on the device - colour conversion, DCT, quantiser, Huffman coding: only the file's bytes come back
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --jpeg device --quality 90 --out kerr_4k.jpg
    # ... and the pan as one Motion-JPEG file that every player opens, an order of magnitude smaller than the .y4m
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --camera 0,0,-8,0 --camera-to 0,3,-6,0 --frames 48 --fps 30000/1001 --jpeg device --out pan.avi
    # lensed point stars with glare: a sharp core inside two Gaussian halos and one stop more exposure, so that a star of 400 outshines a star of 1 in 8 bits
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --sky stars:200000:7 --glare 0.06:1.5,0.03:10 --exposure 1 --out stars.png
    # the same stars as the renderer computed them: scene-linear half floats in an OpenEXR file (ZIPS), nothing clamped at 1; --exr device deflates on the GPU
    python -m geodesic_raytracing_amd.render --metric kerr_boyer --cfg a=0.45 --size 3840x2160 --sky stars:200000:7 --exr device --out stars.exr
"""
import argparse
import ctypes
import math
import os
import sys

import numpy as np

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd.pipeline import FRAME_FORMATS, AviWriter, DeviceBuffer, PinnedBuffer, ProgramManager, Y4MWriter, frame_format_of

HERE = os.path.dirname(os.path.abspath(__file__))


def read_png(path):
    w, h = ctypes.c_int(), ctypes.c_int()
    gra.check(gra.lib.gr_read_png_rgba8(path.encode(), ctypes.byref(w), ctypes.byref(h), None, 0))
    out = np.empty((h.value, w.value, 4), dtype=np.uint8)
    gra.check(gra.lib.gr_read_png_rgba8(path.encode(), ctypes.byref(w), ctypes.byref(h), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
    return out


def write_frame_png(path, frame):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[:2]
    gra.check(gra.lib.gr_write_frame_png(path.encode(), frame.ctypes.data_as(ctypes.c_void_p), w, h))


def write_rgba8_png(path, pixels):
    """a frame that is 8-bit sRGB already (render(..., rgba8=True)): written as it is"""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    h, w = pixels.shape[:2]
    gra.check(gra.lib.gr_write_png_rgba8(path.encode(), pixels.ctypes.data_as(ctypes.c_void_p), w, h))


def write_png_bytes(path, data):
    """a PNG file that is already encoded (render(png="device"), pipeline.PngEncoder.encode)"""
    with open(path, "wb") as f:
        f.write(data)


def write_frame_exr(path, frame):
    """a linear-light float frame [H, W, 4] as an OpenEXR file of half floats (gr_write_frame_exr: pipeline.exr_encode_host's bytes)"""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    h, w = frame.shape[:2]
    gra.check(gra.lib.gr_write_frame_exr(path.encode(), frame.ctypes.data_as(ctypes.c_void_p), w, h))


def write_jpeg_rgba8(path, pixels, quality=90):
    """an 8-bit sRGB frame as a baseline JPEG file, by the host encoder (pipeline.jpeg_encode_host)"""
    write_png_bytes(path, gra.jpeg_encode_host(pixels, quality))


def parse_fps(text):
    """'24' or '30000/1001' -> (numerator, denominator), both >= 1; ValueError otherwise"""
    parts = str(text).split("/")
    if len(parts) not in (1, 2):
        raise ValueError(f"a frame rate of {text!r} is not N or N/D")
    num, den = int(parts[0]), int(parts[1]) if len(parts) == 2 else 1
    if num < 1 or den < 1:
        raise ValueError(f"a frame rate of {text!r}: both parts are at least 1")
    return num, den


def camera_path(position, quat, position_to=None, quat_to=None, frames=1):
    """`frames` poses from (position, quat) to (position_to, quat_to), both ends included: the position (t, x, y, z) linear, the quaternion
    (x, y, z, w) a normalised slerp along the shorter arc.  An end that is None stays where the start is.  Returns [(position, quat)]."""
    p0 = np.array(position if position is not None else gra.default_camera().position[:], dtype=np.float64)
    q0 = np.array(quat if quat is not None else gra.default_camera().quat[:], dtype=np.float64)
    p1 = p0 if position_to is None else np.array(position_to, dtype=np.float64)
    q1 = q0 if quat_to is None else np.array(quat_to, dtype=np.float64)
    if p0.shape != (4,) or p1.shape != (4,) or q0.shape != (4,) or q1.shape != (4,):
        raise ValueError("camera_path: a position is t,x,y,z and a quaternion x,y,z,w")
    if not np.linalg.norm(q0) > 0 or not np.linalg.norm(q1) > 0:
        raise ValueError("camera_path: a quaternion of length zero")
    q0, q1 = q0 / np.linalg.norm(q0), q1 / np.linalg.norm(q1)
    if np.dot(q0, q1) < 0:
        q1 = -q1
    angle = np.arccos(min(1.0, float(np.dot(q0, q1))))
    poses = []
    for k in range(max(int(frames), 1)):
        u = k / (frames - 1) if frames > 1 else 0.0
        if angle < 1e-6:
            q = (1 - u) * q0 + u * q1
        else:
            q = (np.sin((1 - u) * angle) * q0 + np.sin(u * angle) * q1) / np.sin(angle)
        poses.append(([float(v) for v in (1 - u) * p0 + u * p1], [float(v) for v in q / np.linalg.norm(q)]))
    return poses


def shutter_times(frames, shutter, samples):
    """When the sub-frames of a shutter are rendered, in frame numbers: a float64 array [frames, samples] whose entry [k, j] is
    k + shutter * (j + 0.5) / samples.  The shutter of frame k opens at the frame's own time k and stays open for the fraction `shutter`
    (0 < shutter <= 1; 0.5 is the 180-degree film shutter) of the frame interval; sub-frame j sits at the midpoint of the j-th of `samples`
    equal parts of that.  The box weight of every sub-frame is np.float32(1) / np.float32(samples)."""
    frames, samples, shutter = int(frames), int(samples), float(shutter)
    if frames < 1 or samples < 1:
        raise ValueError(f"shutter_times: {frames} frames of {samples} sub-frames (both at least 1)")
    if not 0.0 < shutter <= 1.0:
        raise ValueError(f"shutter_times: a shutter of {shutter!r} (the open fraction of the frame interval: above 0, at most 1)")
    return np.array([[k + shutter * (j + 0.5) / samples for j in range(samples)] for k in range(frames)], dtype=np.float64)


def camera_path_at(position, quat, position_to=None, quat_to=None, frames=1, times=(0.0,)):
    """camera_path's poses at the frame numbers `times`, which need not be whole: u = t / (frames - 1) in camera_path's own expressions (the
    position linear, the quaternion a normalised slerp along the shorter arc), so a whole t gives camera_path's pose exactly and u > 1
    (the sub-frames of the last frame's shutter) continues the same line and the same arc.  Returns [(position, quat)], one per time."""
    p0 = np.array(position if position is not None else gra.default_camera().position[:], dtype=np.float64)
    q0 = np.array(quat if quat is not None else gra.default_camera().quat[:], dtype=np.float64)
    p1 = p0 if position_to is None else np.array(position_to, dtype=np.float64)
    q1 = q0 if quat_to is None else np.array(quat_to, dtype=np.float64)
    if p0.shape != (4,) or p1.shape != (4,) or q0.shape != (4,) or q1.shape != (4,):
        raise ValueError("camera_path_at: a position is t,x,y,z and a quaternion x,y,z,w")
    if not np.linalg.norm(q0) > 0 or not np.linalg.norm(q1) > 0:
        raise ValueError("camera_path_at: a quaternion of length zero")
    q0, q1 = q0 / np.linalg.norm(q0), q1 / np.linalg.norm(q1)
    if np.dot(q0, q1) < 0:
        q1 = -q1
    angle = np.arccos(min(1.0, float(np.dot(q0, q1))))
    poses = []
    for t in np.asarray(times, dtype=np.float64).ravel():
        u = float(t) / (frames - 1) if frames > 1 else 0.0
        if angle < 1e-6:
            q = (1 - u) * q0 + u * q1
        else:
            q = (np.sin((1 - u) * angle) * q0 + np.sin(u * angle) * q1) / np.sin(angle)
        poses.append(([float(v) for v in (1 - u) * p0 + u * p1], [float(v) for v in q / np.linalg.norm(q)]))
    return poses


def glare_of(glare=None, exposure=0.0):
    """render()'s two arguments as one gra.GlareStruct of its own, or None where they ask for nothing"""
    if glare is None and not exposure:
        return None
    if isinstance(glare, gra.GlareStruct):
        made = gra.GlareStruct.from_buffer_copy(glare)
    else:
        pairs = list(glare or [])
        made = gra.glare_gaussians([sigma for _, sigma in pairs], [weight for weight, _ in pairs])
    return gra.glare_exposure(made, exposure) if exposure else made


def parse_glare(text):
    """'W:SIGMA[,W:SIGMA...]' -> [(weight, sigma)], at most four pairs; ValueError otherwise"""
    pairs = []
    for part in text.split(","):
        fields = part.split(":")
        if len(fields) != 2:
            raise ValueError("W:SIGMA[,W:SIGMA...], e.g. 0.06:1.5,0.03:10")
        pairs.append((float(fields[0]), float(fields[1])))
    if len(pairs) > gra.GLARE_MAX_COMPONENTS:
        raise ValueError(f"{len(pairs)} components (at most {gra.GLARE_MAX_COMPONENTS})")
    return pairs


def parse_tone_curve(text):
    """'linear' | 'reinhard[:WHITE]' | 'filmic' -> (gra.TONE_*, white or None); ValueError otherwise"""
    name, _, white = text.partition(":")
    if name not in gra.TONE_CURVE_NAMES or (white and name != "reinhard") or (text.endswith(":")):
        raise ValueError("linear, reinhard[:WHITE] or filmic, e.g. reinhard:4")
    return gra.TONE_CURVE_NAMES[name], float(white) if white else None


def parse_meter(text):
    """'LOW:HIGH' -> (low, high), the metered window as fractions of the non-black pixels; ValueError otherwise"""
    fields = text.split(":")
    if len(fields) != 2:
        raise ValueError("LOW:HIGH, e.g. 0.5:0.98")
    return float(fields[0]), float(fields[1])


def tone_of(auto_exposure=None, meter=None, adapt=None, curve=None):
    """the CLI's four switches as one gra.ToneStruct with checked fields, or None where they ask for nothing.  auto_exposure: None, True
    (the default key) or the key in stops; meter: (low, high); adapt: the rate; curve: (gra.TONE_*, white or None)"""
    if auto_exposure is None and curve is None:
        return None
    low, high = meter if meter is not None else (None, None)
    made = gra.tone(auto=auto_exposure is not None, key_stops=None if auto_exposure in (None, True) else auto_exposure, low=low, high=high, rate=adapt,
                    curve=curve[0] if curve else None, white=curve[1] if curve else None)
    gra.meter_solve(np.zeros(gra.METER_COUNTERS, dtype=np.uint32), made)   # (the library's own check of every field)
    return made


def checked_png_stream(who, png, png_stream):
    """the PNG stream kind as gra.PNG_STREAM_*; a kind other than literals is a property of device-made files"""
    if png_stream not in gra.PNG_STREAM_NAMES and png_stream not in gra.PNG_STREAM_NAMES.values():
        raise ValueError(f"{who}: png_stream={png_stream!r} ({', '.join(gra.PNG_STREAM_NAMES)})")
    kind = gra.PNG_STREAM_NAMES.get(png_stream, png_stream)
    if kind != gra.PNG_STREAM_LITERALS and png != "device":
        raise ValueError(f"{who}: png_stream={png_stream!r} needs png='device' (the host writer has one stream)")
    return kind


def render(metric_name, width, height, scripts=None, cfg=None, camera_pos=None, camera_quat=None, redshift=False, adaptive=False,
           background=None, device=0, fov=90.0, universe=20.0, wait_for_static=True, geodesic_speed=None, geodesic_times=None,
           parallel_transport=True, supersample=1, rgba8=False, mips="host", yuv420=False, cameras=None, bit_depth=8, shutter_samples=0, filter="box",
           png="host", jpeg=None, quality=90, png_stream="literals", sky=None, glare=None, exposure=0.0, exr=None, tone=None, exposures=None):
    """exr: "host" or "device" (float frames only: no rgba8, yuv420, png="device" or jpeg) - every frame returned is the bytes of a finished
    OpenEXR file of scene-linear half floats instead of pixels: with "device" the float4 frame stays on the device and is converted,
    predicted, histogrammed and bit-packed there (pipeline.ExrEncoder), with "host" it comes back and pipeline.exr_encode_host makes the
    file - the same bytes.
    tone: a gra.ToneStruct (pipeline.tone) - every frame delivered is metered (auto mode), exposed and put through the tone curve on the
    device, after the glare and before any encode (RenderState(tone=)); along a sequence the exposure adapts at tone.rate.  exposures: a
    list that receives (stops, gain) of every frame delivered - in auto mode by RenderState.exposure() after the frame's own download, a
    24-byte copy and a wait more a frame (leave it None where frames must stay in flight); a manual tone's pair is computed once on the host.  Whole frames only.
    glare: a gra.GlareStruct (pipeline.glare_gaussians) or [(weight, sigma)], up to four Gaussians of sigma output pixels - every frame
    goes through that point-spread function on the device, in linear light, after the resolve and before any encode (RenderState(glare=):
    pipeline.glare_frame of the frame rendered without it, bit for bit): a star far above 1 keeps a halo in an 8-bit file.  exposure:
    stops, -32 ... 32 - a gain of 2^exposure on the same stage (pipeline.glare_exposure); works alone.  Whole frames only.
    sky: a gra.AnalyticSky - every frame is shaded from it in closed form (RenderState(sky=)) - or a StarField - point stars, lensed on the
    device (RenderState(stars=)); `background` and `mips` are then unused.
    Returns the linear-light float32 frame [H, W, 4]; with geodesic_speed (camera on its own timelike geodesic,
    main.cpp:2675-2760) a list of frames, one per entry of geodesic_times (proper time along the path).  supersample = f (2, 3, 4): traced
    at f x the size per axis and box-averaged on the device (the reference's supersample setting, graphics_settings.hpp:23-24).
    rgba8: the frames are uint8 [H, W, 4] in sRGB instead, encoded on the device (RenderState.render_rgba8) and fetched at 4 bytes a
    pixel through pinned memory - the bytes pipeline.encode_srgb8 makes of the float frame.
    yuv420: the frames are uint8 [yuv420_bytes(W, H)] instead: 8-bit BT.709 Y'CbCr 4:2:0 in I420 order (planes Y, Cb, Cr), made on the device in
    the launch that resolves and encodes (RenderState.render_yuv420) and fetched at 1.5 bytes a pixel through pinned memory - the bytes
    pipeline.rgba8_to_yuv420 makes of the rgba8 frame.  With bit_depth=10 they are uint16 [yuv420p10_bytes(W, H) / 2]: 10-bit samples in
    yuv420p10le order (RenderState.render_yuv420p10), 3 bytes a pixel through pinned memory - the words
    pipeline.rgb10_to_yuv420p10(pipeline.frame_to_rgb10(...)) makes of the float frame.
    cameras: [(position, quat)] (camera_path) - a list of frames, one per pose, of a camera that rides no geodesic (not with geodesic_speed).
    shutter_samples = T > 0 (motion blur): `cameras`, or `geodesic_times`, holds T entries per delivered frame, consecutive ones (shutter_times
    and camera_path_at make them); every frame returned is the sum of its T sub-frames with the box weight np.float32(1) / np.float32(T),
    accumulated on the device in linear light (RenderState.render_subframe: pipeline.accumulate_frame of the frames render() returns
    without it, bit for bit) and delivered in the format asked for (RenderState.deliver_accumulated).  Fused path only (not with adaptive).
    filter: "box" (the mean of a pixel's own samples, as ever), "tent", "gaussian" or "mitchell" (or a gra.FILTER_* value) - the traced frame
    goes through that separable reconstruction filter on the device instead (RenderState(filter=): pipeline.filter_frame with
    pipeline.filter_taps' table of the frame a plain state of the traced size renders, bit for bit), at any supersample, 1 included, and
    in every format; sub-frames of a shutter are filtered before they are accumulated.
    mips: where the sky's mip slices are made - "host" (pack_background, all slices uploaded) or "device" (build_background: the image is
    uploaded and the slices are built there, the same bytes).
    png: "device" (with rgba8) - every frame returned is the bytes of a finished PNG file instead of pixels: the RGBA8 frame stays on the
    device, is filtered, histogrammed and bit-packed there (pipeline.PngEncoder) and only the compressed bytes come back - the file
    pipeline.png_encode_host makes of the rgba8 frame, byte for byte.
    png_stream: "literals" or "runs" (or a gra.PNG_STREAM_* value; other than literals only with png="device") - the stream kind of those
    files: runs adds previous-pixel run matches (pipeline.png_encode_host(pixels, "runs") is then the file, byte for byte).
    jpeg: "host" or "device" (with rgba8; not with png="device") - every frame returned is the bytes of a finished baseline JPEG file at
    `quality` (1 ... 100): with "device" the RGBA8 frame stays on the device and is converted, transformed, quantised and Huffman-coded there
    (pipeline.JpegEncoder), with "host" its pixels come back and pipeline.jpeg_encode_host makes the file - the same bytes."""
    if mips not in ("host", "device"):
        raise ValueError(f"render: mips={mips!r} (host or device)")
    if jpeg not in (None, "host", "device") or (jpeg is not None and (not rgba8 or yuv420 or png == "device")):
        raise ValueError(f"render: jpeg={jpeg!r} (None, or host or device with rgba8=True, no yuv420 and png='host')")
    if jpeg is not None and not 1 <= int(quality) <= 100:
        raise ValueError(f"render: quality={quality!r} (1 to 100)")
    if exr not in (None, "host", "device") or (exr is not None and (rgba8 or yuv420 or png == "device" or jpeg is not None)):
        raise ValueError(f"render: exr={exr!r} (None, or host or device with float frames: no rgba8, yuv420, png='device' or jpeg)")
    if png not in ("host", "device") or (png == "device" and (not rgba8 or yuv420)):
        raise ValueError(f"render: png={png!r} (host, or device with rgba8=True and no yuv420)")
    png_stream = checked_png_stream("render", png, png_stream)
    if bit_depth not in (8, 10) or (bit_depth == 10 and not yuv420):
        raise ValueError(f"render: bit_depth={bit_depth!r} (8, or 10 with yuv420=True)")
    if cameras is not None and geodesic_speed is not None:
        raise ValueError("render: cameras (interpolated poses) and geodesic_speed (a camera on its geodesic) exclude each other")
    if filter not in gra.FILTER_NAMES and filter not in gra.FILTER_NAMES.values():
        raise ValueError(f"render: filter={filter!r} ({', '.join(gra.FILTER_NAMES)})")
    frame_format = frame_format_of(rgba8, yuv420, bit_depth)
    fmt = FRAME_FORMATS[frame_format]
    shutter_samples = int(shutter_samples)
    if shutter_samples:
        moving = cameras if cameras is not None else geodesic_times if geodesic_speed is not None else None
        if shutter_samples < 0 or adaptive or moving is None or len(moving) == 0 or len(moving) % shutter_samples:
            raise ValueError(f"render: shutter_samples={shutter_samples} needs the fused path (no adaptive) and cameras or geodesic_times with that many "
                             "entries per frame")
    metric = gra.Metric(metric_name, scripts or os.path.join(HERE, "scripts"))
    feats = metric.features(adaptive_sampling=int(adaptive), redshift=int(redshift), field_of_view=fov, universe_size=universe)
    cfg_values = metric.cfg_values(**(cfg or {}))
    manager = ProgramManager(metric, device, feats, cfg_values)
    program = manager.current(wait=wait_for_static)
    stars = sky.on(program) if isinstance(sky, StarField) else None   # (point stars: a catalogue built on this device, the same on both sides)
    state = gra.RenderState(width, height, device, supersample=supersample, filter=filter, sky=sky if stars is None else None, stars=stars,
                            glare=glare_of(glare, exposure), tone=tone)
    if sky is None:
        rgba = background if background is not None else gra.synthetic_background(2048, 1024)
        if mips == "device":
            dbg, levels = gra.build_background(program, rgba, device)
        else:
            packed, levels = gra.pack_background(rgba)
            dbg = DeviceBuffer.from_numpy(device, packed)
    out_bytes = fmt.bytes(width, height)
    out = DeviceBuffer(device, out_bytes)
    encoder = (gra.PngEncoder(program, width, height, png_stream) if png == "device" else
               gra.JpegEncoder(program, width, height, quality) if jpeg == "device" else
               gra.ExrEncoder(program, width, height) if exr == "device" else None)
    pinned = PinnedBuffer(out_bytes) if frame_format != gra.FRAME_F32 and encoder is None else None   # (a float frame is downloaded as it always was)
    cam = gra.default_camera(camera_pos, camera_quat)
    mode = gra.MODE_REFERENCE if adaptive else gra.MODE_FUSED
    bg = (dbg.ptr, rgba.shape[1], rgba.shape[0], levels) if sky is None else None   # (an analytic sky: no image, no mips, no upload)

    manual_exposure = state.exposure() if tone is not None and tone.mode != gra.TONE_AUTO else None   # (host arithmetic: no device call)

    def fetch():
        frame = fetched()
        if tone is not None and exposures is not None:   # auto: one more small download behind the frame's, which fetched() has waited for
            exposures.append(state.exposure() if tone.mode == gra.TONE_AUTO else manual_exposure)
        return frame

    def fetched():
        if encoder is not None:
            return encoder.encode(out.ptr, None)   # the frame's stream: the encoder's launches queue behind the frame's
        if pinned is None:
            state.synchronize()
            if exr == "host":
                return gra.exr_encode_host(out.to_numpy(fmt.dtype, fmt.shape(width, height)))
            return out.to_numpy(fmt.dtype, fmt.shape(width, height))
        pinned.download_async(None, out.ptr, out_bytes)   # the frame's stream: copies queue behind its launches
        gra.check(gra.lib.gr_stream_synchronize(None))
        if jpeg == "host":
            return gra.jpeg_encode_host(pinned.view(fmt.dtype, fmt.shape(width, height)), quality)
        return pinned.view(fmt.dtype, fmt.shape(width, height)).copy()

    weight = np.float32(1) / np.float32(shutter_samples) if shutter_samples else None
    subframe = [0]   # sub-frames of the current shutter rendered so far

    def one_frame(options, cam=cam):
        if not shutter_samples:
            state.render(program, metric, cam, out.ptr, bg, feats, cfg_values, options, rgba8=rgba8, yuv420=gra.YUV420_I420 if yuv420 else None,
                         bit_depth=bit_depth)
            return fetch()
        # a sub-frame: accumulated on the device; the last one of a shutter delivers
        state.render_subframe(program, metric, cam, weight, subframe[0] == 0, bg, feats, cfg_values, options)
        subframe[0] = (subframe[0] + 1) % shutter_samples
        if subframe[0]:
            return None
        state.deliver_accumulated(program, out.ptr, frame_format)
        return fetch()

    def frames_of_the_call():
        made = rendered()
        return [frame for frame in made if frame is not None] if shutter_samples else made   # (a sub-frame that delivers nothing gives None)

    def rendered():
        if cameras is not None:
            return [one_frame(gra.frame_options(mode=mode), gra.default_camera(position, quat)) for position, quat in cameras]
        if geodesic_speed is None:
            return one_frame(gra.frame_options(mode=mode))
        gc = gra.GeodesicCamera(device=device)
        steps, tau = gc.snapshot(program, metric, cam, geodesic_speed, feats, cfg_values)
        print(f"geodesic snapshot: {steps} samples covering {tau:.3f} of proper time", file=sys.stderr)
        times = list(geodesic_times or [0.0])
        frames = []
        for i, t in enumerate(times):
            ahead = i + 1 < len(times) and mode == gra.MODE_FUSED
            opts = gra.frame_options(mode=mode, geodesic=gc.handle.value, geodesic_time=t, parallel_transport_observer=int(parallel_transport),
                                     next_camera=ctypes.pointer(cam) if ahead else None, next_geodesic_time=times[i + 1] if ahead else 0.0)
            frames.append(one_frame(opts))
        return frames

    try:
        return frames_of_the_call()
    finally:
        if pinned is not None:   # every frame was copied out of it
            pinned.free()


def split_block_rows(height, block_rows=16):
    """the rows of a block of a split frame: `block_rows`, or the next multiple of 8 with which the image's last row does not start a block
    (its filter reads the row above: gr_tiled_create_local refuses that)"""
    while height > 1 and (height - 1) % block_rows == 0:
        block_rows += 8
    return block_rows


def render_split(metric_name, width, height, devices, scripts=None, cfg=None, camera_pos=None, camera_quat=None, redshift=False, background=None,
                 fov=90.0, universe=20.0, wait_for_static=True, supersample=1, rgba8=False, mips="host", frames=1, block_rows=16, png="host", jpeg=None,
                 quality=90, png_stream="literals", sky=None):
    """sky: as in render().
    render() of a Cartesian camera with the rows of every frame dealt to `devices` (TiledFrame.local: one process, peer copies, participant
    r on devices[r]; a device may be named more than once, which is how a box with one GPU rehearses it).  Every device has its own program,
    sky (with mips="device" built there, once per device) and render state, traces its share at `supersample` x per axis, resolves it
    there and ships width x rows pixels to devices[0] - float4, or with rgba8 4 bytes each (TiledFrame.render_as).  Frame k is rendered
    with rotation k, so the shares go round over `frames`.  Returns the list of frames: the arrays render() returns, bit for bit.  png="device"
    (with rgba8): the finished frame on devices[0] is encoded there (pipeline.PngEncoder) and every frame returned is a PNG file's bytes, in
    the stream kind png_stream ("literals" or "runs", as render() takes it).
    jpeg="host" or "device" (with rgba8, not with png="device"): every frame returned is a JPEG file's bytes at `quality`, made by
    pipeline.jpeg_encode_host of the downloaded frame or on devices[0] (pipeline.JpegEncoder) - the same bytes."""
    if mips not in ("host", "device"):
        raise ValueError(f"render_split: mips={mips!r} (host or device)")
    if png not in ("host", "device") or (png == "device" and not rgba8):
        raise ValueError(f"render_split: png={png!r} (host, or device with rgba8=True)")
    png_stream = checked_png_stream("render_split", png, png_stream)
    if jpeg not in (None, "host", "device") or (jpeg is not None and (not rgba8 or png == "device")) or (jpeg is not None and not 1 <= int(quality) <= 100):
        raise ValueError(f"render_split: jpeg={jpeg!r}, quality={quality!r} (None, or host or device with rgba8=True, png='host' and a quality of 1 to 100)")
    devices = [int(d) for d in devices]
    if not devices:
        raise ValueError("render_split: no devices")
    metric = gra.Metric(metric_name, scripts or os.path.join(HERE, "scripts"))
    feats = metric.features(adaptive_sampling=0, redshift=int(redshift), field_of_view=fov, universe_size=universe)
    cfg_values = metric.cfg_values(**(cfg or {}))
    rgba = (background if background is not None else gra.synthetic_background(2048, 1024)) if sky is None else None
    managers, programs, skies = {}, {}, {}
    for d in devices:   # once per device, however many participants it carries
        if d in programs:
            continue
        managers[d] = ProgramManager(metric, d, feats, cfg_values)
        programs[d] = managers[d].current(wait=wait_for_static)
        if sky is not None:   # an analytic sky: every participant's state shades from it, no device holds an image
            skies[d] = (None, None)
            continue
        if mips == "device":
            dbg, levels = gra.build_background(programs[d], rgba, d)
        else:
            packed, levels = gra.pack_background(rgba)
            dbg = DeviceBuffer.from_numpy(d, packed)
        skies[d] = (dbg, (dbg.ptr, rgba.shape[1], rgba.shape[0], levels))
    parts = gra.TiledFrame.local(devices, width, height, split_block_rows(height, block_rows))
    try:
        if isinstance(sky, StarField):   # a catalogue per device, built once however many participants the device carries
            fields = {d: sky.on(programs[d]) for d in programs}
            states = [gra.RenderState(width, height, d, supersample=supersample, stars=fields[d]) for d in devices]
        else:
            states = [gra.RenderState(width, height, d, supersample=supersample, sky=sky) for d in devices]
        out = DeviceBuffer(devices[0], width * height * (4 if rgba8 else 16))
        cam = gra.default_camera(camera_pos, camera_quat)
        encoder = (gra.PngEncoder(programs[devices[0]], width, height, png_stream) if png == "device" else
                   gra.JpegEncoder(programs[devices[0]], width, height, quality) if jpeg == "device" else None)
        result = []
        for k in range(max(int(frames), 1)):
            for r, d in enumerate(devices):
                parts[r].render_as(states[r], programs[d], metric, cam, out.ptr, skies[d][1], feats, cfg_values, gra.frame_options(mode=gra.MODE_FUSED),
                                   rotation=k, rgba8=rgba8)
            parts[0].join()
            gra.check(gra.lib.gr_device_synchronize(devices[0]))
            if encoder is not None:
                result.append(encoder.encode(out.ptr, None))
            elif jpeg == "host":
                result.append(gra.jpeg_encode_host(out.to_numpy(np.uint8, (height, width, 4)), quality))
            else:
                result.append(out.to_numpy(np.uint8 if rgba8 else np.float32, (height, width, 4)))
        return result
    finally:
        for part in parts:
            part.close()


class StarField:
    """--sky stars:N[:SEED[:MIN_FOOTPRINT]]: N generated stars (gra.star_field_random), the same catalogue on both sides, black behind them"""

    def __init__(self, n, seed=1, min_footprint=2.0 ** -16):
        if not 1 <= n <= 1 << 24:
            raise ValueError("N: 1 to 16777216 stars")
        mantissa, exponent = math.frexp(min_footprint)
        if mantissa != 0.5 or not -20 <= exponent - 1 <= -8:
            raise ValueError("MIN_FOOTPRINT: a power of two from 2^-20 to 2^-8, e.g. 1.52587890625e-05")
        self.n, self.seed, self.min_footprint = n, seed, min_footprint

    def on(self, program):
        """RenderState(stars=...) for a state of the program's device"""
        catalogue = gra.StarCatalogue.random(program, self.seed, self.n)
        return gra.StarSky(min_footprint=self.min_footprint), catalogue, catalogue


def parse_sky(text):
    """--sky grid[:MxP[:WIDTH]] -> gra.AnalyticSky (the library refuses what is out of range); --sky stars:N[:SEED[:MIN_FOOTPRINT]] -> StarField"""
    parts = text.split(":")
    if parts[0] == "stars":
        if not 2 <= len(parts) <= 4:
            raise ValueError("stars:N[:SEED[:MIN_FOOTPRINT]], e.g. stars:200000:7")
        return StarField(int(parts[1]), int(parts[2]) if len(parts) > 2 else 1, float(parts[3]) if len(parts) > 3 else 2.0 ** -16)
    if parts[0] != "grid" or len(parts) > 3:
        raise ValueError("grid[:MxP[:WIDTH]], e.g. grid:36x18:0.08")
    fields = {}
    if len(parts) > 1:
        cells = parts[1].split("x")
        if len(cells) != 2:
            raise ValueError("MxP: meridians a turn and cells between the poles, e.g. 36x18")
        fields["meridians"], fields["parallels"] = int(cells[0]), int(cells[1])
    if len(parts) > 2:
        fields["line_width"] = float(parts[2])
    sky = gra.AnalyticSky(**fields)
    sky.image(1, 1)   # the library's own check of the fields, with its message
    return sky


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--metric", required=True)
    ap.add_argument("--scripts", default=None, help="scripts folder (default: the one shipped with the package)")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--cfg", action="append", default=[], help="NAME=VALUE, a $cfg parameter of the metric (repeatable)")
    ap.add_argument("--camera", default=None, help="t,x,y,z")
    ap.add_argument("--quat", default=None, help="x,y,z,w")
    ap.add_argument("--camera-to", default=None, help="t,x,y,z: the camera's position in the last of --frames frames; frame k is rendered from the "
                    "position interpolated linearly between --camera and this (a camera that rides no geodesic; not with --geodesic-speed)")
    ap.add_argument("--quat-to", default=None, help="x,y,z,w: the orientation in the last frame, reached from --quat by a normalised slerp")
    ap.add_argument("--fov", type=float, default=90.0)
    ap.add_argument("--universe", type=float, default=20.0)
    ap.add_argument("--redshift", action="store_true")
    ap.add_argument("--adaptive", action="store_true", help="quarter-resolution primary rays + refinement (reference mode)")
    ap.add_argument("--background", default=None, help="equirectangular PNG (default: synthetic grid + stars)")
    ap.add_argument("--geodesic-speed", default=None, help="vx,vy,vz (|v| < 1, camera tetrad frame): ride the timelike geodesic "
                    "launched from --camera with this speed")
    ap.add_argument("--geodesic-time", type=float, default=0.0, help="proper time of the first frame")
    ap.add_argument("--geodesic-dt", type=float, default=0.5, help="proper time between frames")
    ap.add_argument("--frames", type=int, default=1)
    ap.add_argument("--recompute-tetrads", action="store_true", help="rebuild the tetrad at every point instead of parallel transport")
    ap.add_argument("--supersample", type=int, choices=[1, 2, 3, 4], default=1, help="anti-aliasing: trace N x N rays per pixel of --size and "
                    "average them on the device (the output keeps the size given by --size)")
    ap.add_argument("--encode", choices=["host", "device"], default="host", help="where the frame becomes 8-bit sRGB: host = download float4 and "
                    "convert there; device = encode on the GPU and download 4 bytes a pixel (the same bytes).  Ignored for --out NAME.y4m, "
                    "whose frames are always encoded on the device")
    ap.add_argument("--png", choices=["host", "device"], default=None, help="where a frame becomes a PNG file: host = the pixels come back and one host "
                    "thread deflates them; device = the 8-bit frame is filtered, histogrammed and Huffman-coded on the GPU (Sub / Up filters, one "
                    "table a frame, no matches) and only the compressed bytes come back.  device implies --encode device; not with --out NAME.y4m")
    ap.add_argument("--png-stream", choices=sorted(gra.PNG_STREAM_NAMES, key=gra.PNG_STREAM_NAMES.get), default=None, help="the stream of a PNG made "
                    "with --png device: literals (the default: no matches) or runs (runs of pixels whose filtered bytes repeat the previous "
                    "pixel's become matches of distance 4: smaller files of the same pixels).  Only with --png device")
    ap.add_argument("--jpeg", choices=["host", "device"], default=None, help="where a frame of --out NAME.jpg or NAME.avi becomes a baseline JPEG file "
                    "(JFIF, 4:2:0, the standard Huffman tables, one restart interval a row of 16 x 16 blocks): host (the default) = the 8-bit pixels "
                    "come back and one host thread encodes them; device = colour conversion, DCT, quantiser and Huffman coding run on the GPU and only "
                    "the file's bytes come back (the same bytes).  device implies --encode device; not with --out NAME.png or NAME.y4m")
    ap.add_argument("--exr", choices=["host", "device"], default=None, help="where a frame of --out NAME.exr becomes an OpenEXR file (scene-linear half "
                    "floats, B G R, ZIPS: one zlib stream a scan line, rows that do not shrink stored raw): host (the default) = the float4 frame comes "
                    "back and one host thread converts and deflates it; device = half conversion, predictor, histogram and Huffman coding run on the "
                    "GPU and only the file's bytes come back (the same bytes).  Only with --out NAME.exr; device not with --devices")
    ap.add_argument("--quality", type=int, default=None, help="of a .jpg or .avi: 1 ... 100, the usual scaling of the standard quantisation tables (90)")
    ap.add_argument("--sky", default=None, help="stars:N[:SEED[:MIN_FOOTPRINT]]: N point stars, generated, binned on the GPU and lensed there - a star's "
                    "brightness in a pixel goes as the inverse of the sky the pixel covers, down to MIN_FOOTPRINT (a power of two, 2^-16).  "
                    "grid[:MxP[:WIDTH]]: the analytic sky - a coloured celestial sphere with M meridians a turn and P cells "
                    "between the poles (36x18), lines of WIDTH of a cell (0.08), antialiased exactly on the device at any magnification; no "
                    "image, no mips, no upload.  Not with --background or --mips")
    ap.add_argument("--mips", choices=["host", "device"], default=None, help="where the sky's mip slices are made: host = pack them on the CPU "
                    "and upload all of them (default: host); device = upload the image and build the slices on the GPU (the same bytes)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--filter", choices=sorted(gra.FILTER_NAMES, key=gra.FILTER_NAMES.get), default="box", help="the reconstruction filter of "
                    "--supersample's samples, applied on the device before any encode: box (the mean of the N x N samples behind a pixel), tent "
                    "(radius 1 pixel), gaussian or mitchell (Mitchell-Netravali, B = C = 1/3; both radius 2) - wider separable filters that fold "
                    "less of what the extra rays resolved back as aliasing.  Works at --supersample 1 too (gaussian and mitchell are a mild "
                    "post-filter there, tent changes nothing).  Not with --devices")
    ap.add_argument("--glare", default=None, metavar="W:SIGMA[,W:SIGMA...]", help="a point-spread function applied on the device in linear light, after the "
                    "resolve and before any encode: up to four Gaussians of SIGMA output pixels, each holding the share W of a pixel's light (the "
                    "core keeps the rest), e.g. 0.06:1.5,0.03:10 - a star far above 1 keeps a halo in an 8-bit file.  Not with --devices")
    ap.add_argument("--exposure", type=float, default=None, metavar="STOPS", help="a gain of 2^STOPS on the same stage, -32 ... 32; works alone.  Not "
                    "with --devices")
    ap.add_argument("--auto-exposure", nargs="?", const="key", default=None, metavar="KEY_STOPS", help="meter every frame on the device - a luminance "
                    "histogram of the finished frame, solved there to the gain that puts the metered level at 2^KEY_STOPS (log2 0.18 = -2.47) - in "
                    "sixteenths of a stop, no host round trip; along --frames the exposure adapts (--adapt) and every frame's stops are printed.  "
                    "Not with --exposure or --devices")
    ap.add_argument("--meter", default=None, metavar="LOW:HIGH", help="with --auto-exposure: the metered window, as fractions of the pixels that are "
                    "not black, ordered by luminance (0.5:0.98)")
    ap.add_argument("--adapt", type=float, default=None, metavar="RATE", help="with --auto-exposure: the share of the way to a frame's own exposure that "
                    "the sequence moves a frame, (0, 1] (1: every frame on its own)")
    ap.add_argument("--tone", default=None, metavar="CURVE", help="linear, reinhard[:WHITE] or filmic: the curve after the gain, on the device before any "
                    "encode - reinhard (white point WHITE, 4) and filmic roll highlights off instead of clipping them at 1.  Not with --devices")
    ap.add_argument("--devices", default=None, help="0,1,2,3: deal the rows of every frame to these GPUs (one process, peer copies; a device may "
                    "repeat); each traces, resolves and - with --encode device - encodes its share, the share rotating over --frames")
    ap.add_argument("--fps", default="24", help="frame rate of a .y4m or .avi file: N or N/D (24; 30000/1001)")
    ap.add_argument("--bit-depth", type=int, choices=[8, 10], default=None, help="bits a sample of a .y4m file: 8 (C420jpeg, 1.5 bytes a pixel) or 10 "
                    "(C420p10: 16-bit little-endian words, 3 bytes a pixel - the master for a 10-bit encode).  Only with --out NAME.y4m")
    ap.add_argument("--shutter", type=float, default=None, help="motion blur: the fraction of the frame interval the shutter is open, above 0 and at "
                    "most 1 (0.5: the 180-degree film shutter; default: no shutter, every frame one instantaneous pose).  Every frame is the "
                    "average of --shutter-samples sub-frames rendered at equally spaced moments of that interval and summed on the device in "
                    "linear light.  Needs a camera that moves: --camera-to / --quat-to or --geodesic-speed")
    ap.add_argument("--shutter-samples", type=int, default=None, help="sub-frames a frame of --shutter, 2 ... 64 (8)")
    ap.add_argument("--out", required=True, help="NAME.png: one PNG, or NAME_000.png ... for a sequence.  NAME.y4m: all frames in one uncompressed "
                    "YUV4MPEG2 file of 8-bit BT.709 Y'CbCr 4:2:0 frames, converted on the device.  NAME.jpg: one baseline JPEG, or NAME_000.jpg ... for a "
                    "sequence.  NAME.avi: all frames in one Motion-JPEG file (AVI 1.0, at most 2 GiB).  NAME.exr: one OpenEXR file of the frame in linear "
                    "light, half floats, or NAME_000.exr ... for a sequence")
    a = ap.parse_args(argv)
    video = a.out.lower().endswith(".y4m")
    avi = a.out.lower().endswith(".avi")
    jpeg_out = avi or a.out.lower().endswith((".jpg", ".jpeg"))
    exr_out = a.out.lower().endswith(".exr")
    if a.exr is not None and not exr_out:
        ap.error(f"--exr {a.exr} with --out {a.out}: --exr says where an OpenEXR file is made; give --out NAME.exr")
    if exr_out:
        for given, flag in ((a.encode == "device", "--encode device"), (a.png is not None, "--png"), (a.jpeg is not None, "--jpeg"),
                            (a.quality is not None, "--quality"), (a.bit_depth is not None, "--bit-depth")):
            if given:
                ap.error(f"{flag} with --out NAME.exr: an OpenEXR file holds the frame in linear light as half floats - there is no 8-bit encode, "
                         "no PNG or JPEG stream and no video bit depth in it; leave the flag out (--exr host|device says where the file is made)")
        a.exr = a.exr or "host"
        if a.exr == "device" and a.devices is not None:
            ap.error("--exr device with --devices: the assembled frame of a split render is not on one device for the encoder to read; "
                     "--exr host works there")
    a.png = a.png or "host"
    a.bit_depth = a.bit_depth or 8
    try:
        fps = parse_fps(a.fps)
    except ValueError as e:
        ap.error(f"--fps: {e}")
    sky = None
    if a.sky is not None:
        if a.background is not None or a.mips is not None:
            ap.error("--sky with --background / --mips: an analytic sky or a star field is no image and has no mip slices; give one or the other")
        try:
            sky = parse_sky(a.sky)
        except (ValueError, gra.GeodesicError) as e:
            ap.error(f"--sky {a.sky}: {e}")
    a.mips = a.mips or "host"
    if a.bit_depth != 8 and not video:
        ap.error("--bit-depth 10 is a depth of video frames: it needs --out NAME.y4m (a PNG is 8-bit sRGB, and so is a JPEG or a Motion-JPEG file)")
    if a.png_stream is not None and a.png != "device":
        ap.error(f"--png-stream {a.png_stream} without --png device: the stream kind is one of device-made PNG files (--png host has one stream); "
                 "give --png device")
    a.png_stream = a.png_stream or "literals"
    if a.png == "device":
        if video:
            ap.error("--png device with --out NAME.y4m: a video file holds no PNG; --png is about --out NAME.png")
        a.encode = "device"
    if jpeg_out:
        if a.png == "device":
            ap.error("--png device with --out NAME.jpg / NAME.avi: the frames of such a file are JPEG files; --png is about --out NAME.png")
        a.jpeg = a.jpeg or "host"
        a.quality = 90 if a.quality is None else a.quality
        if not 1 <= a.quality <= 100:
            ap.error(f"--quality {a.quality}: 1 to 100")
        a.encode = "device"   # a JPEG is made of the 8-bit frame; with --jpeg host its pixels come back at 4 bytes each
    elif a.jpeg is not None or a.quality is not None:
        ap.error("--jpeg / --quality with --out NAME.png / NAME.y4m: they are about JPEG frames; give --out NAME.jpg or NAME.avi")
    if a.shutter_samples is not None and a.shutter is None:
        ap.error("--shutter-samples without --shutter: the sub-frames are those of a shutter; give its open fraction, e.g. --shutter 0.5")
    if a.shutter is not None:
        if not 0.0 < a.shutter <= 1.0:
            ap.error(f"--shutter {a.shutter}: the fraction of the frame interval the shutter is open, above 0 and at most 1")
        if a.shutter_samples is not None and not 2 <= a.shutter_samples <= 64:
            ap.error(f"--shutter-samples {a.shutter_samples}: 2 to 64 sub-frames a frame")
        if a.devices is not None:
            ap.error("--shutter with --devices: a share of a split frame is not accumulated; render the blurred sequence on one device")
        if a.adaptive:
            ap.error("--shutter with --adaptive: the sub-frames of a shutter are rendered on the fused path, adaptive sampling runs in reference mode")
        if not (a.camera_to or a.quat_to or a.geodesic_speed):
            ap.error("--shutter on a camera that does not move: there is no motion to blur; give --camera-to / --quat-to or --geodesic-speed")
    if a.filter != "box" and a.devices is not None:
        ap.error(f"--filter {a.filter} with --devices: a filter wider than a pixel reads across the strips of a split frame; render filtered "
                 "frames on one device (a split frame takes --filter box)")
    glare = None
    if a.glare is not None or a.exposure is not None:
        if a.devices is not None:
            ap.error(f"{'--glare' if a.glare is not None else '--exposure'} with --devices: the point-spread function reads across the strips of a split "
                     "frame, and the gain is a part of that stage; render such frames on one device")
        try:
            glare = glare_of(parse_glare(a.glare) if a.glare is not None else [], a.exposure or 0.0) or gra.glare_gaussians()
        except (ValueError, gra.GeodesicError) as e:
            ap.error(f"--glare {a.glare} --exposure {a.exposure}: {e}")
    tone = None
    given = [name for name, value in (("--auto-exposure", a.auto_exposure), ("--meter", a.meter), ("--adapt", a.adapt), ("--tone", a.tone)) if value is not None]
    if given:
        if a.devices is not None:
            ap.error(f"{given[0]} with --devices: a histogram of a strip is not the frame's, and the curve follows the meter; render such frames on one device")
        if a.auto_exposure is not None and a.exposure is not None:
            ap.error("--auto-exposure with --exposure: the exposure is either metered or given")
        if a.auto_exposure is None and (a.meter is not None or a.adapt is not None):
            ap.error(f"{'--meter' if a.meter is not None else '--adapt'} without --auto-exposure: there is no meter to set")
        try:
            key = None if a.auto_exposure is None else True if a.auto_exposure == "key" else float(a.auto_exposure)
            tone = tone_of(key, parse_meter(a.meter) if a.meter is not None else None, a.adapt, parse_tone_curve(a.tone) if a.tone is not None else None)
        except (ValueError, gra.GeodesicError) as e:
            ap.error(f"{' '.join(given)}: {e}")
    if video and a.devices is not None:
        ap.error("--out NAME.y4m with --devices: a split frame travels as float4 or RGBA8, not as 4:2:0 planes; render the video on one device")
    if (a.camera_to or a.quat_to) and a.geodesic_speed:
        ap.error("--camera-to / --quat-to with --geodesic-speed: the camera either follows the interpolated poses or rides its geodesic")
    if (a.camera_to or a.quat_to) and a.devices is not None:
        ap.error("--camera-to / --quat-to with --devices: a split sequence renders one camera")
    samples = (a.shutter_samples or 8) if a.shutter is not None else 0
    w, h = (int(v) for v in a.size.lower().split("x"))
    cfg = {k: float(v) for k, v in (kv.split("=") for kv in a.cfg)}
    speed = [float(v) for v in a.geodesic_speed.split(",")] if a.geodesic_speed else None
    times = [a.geodesic_time + i * a.geodesic_dt for i in range(max(a.frames, 1))]
    moments = shutter_times(max(a.frames, 1), a.shutter, samples).ravel() if samples else None   # frame numbers, `samples` a frame
    write = write_png_bytes if a.png == "device" or jpeg_out or (exr_out and a.devices is None) else write_frame_exr if exr_out else write_rgba8_png if a.encode == "device" else write_frame_png
    if a.devices is not None:
        try:
            devices = [int(v) for v in a.devices.split(",")]
        except ValueError:
            devices = []
        if not devices or min(devices) < 0:
            ap.error("--devices: a comma-separated list of device numbers, e.g. 0,1,2,3")
        if a.adaptive:
            ap.error("--adaptive with --devices: adaptive sampling runs in reference mode, which renders whole frames (no strips)")
        if speed is not None:
            ap.error("--geodesic-speed with --devices: a split frame takes a Cartesian camera")
        result = render_split(a.metric, w, h, devices, a.scripts, cfg, [float(v) for v in a.camera.split(",")] if a.camera else None,
                              [float(v) for v in a.quat.split(",")] if a.quat else None, a.redshift, read_png(a.background) if a.background else None,
                              a.fov, a.universe, supersample=a.supersample, rgba8=a.encode == "device", mips=a.mips, frames=a.frames, png=a.png,
                              jpeg=a.jpeg, quality=a.quality or 90, png_stream=a.png_stream, sky=sky)
        if avi:
            with AviWriter(a.out, w, h, fps) as stream:
                for frame in result:
                    stream.write(frame)
            print(f"wrote {a.out} ({w}x{h}, {len(result)} frames at {fps[0]}/{fps[1]} a second, Motion-JPEG, {len(devices)} participants)")
            return 0
        stem, ext = os.path.splitext(a.out)
        for i, frame in enumerate(result):
            path = a.out if len(result) == 1 else f"{stem}_{i:03d}{ext}"
            write(path, frame)
            print(f"wrote {path} ({w}x{h}, {len(devices)} participants, rotation {i})")
        return 0
    position, quat = ([float(v) for v in text.split(",")] if text else None for text in (a.camera, a.quat))
    cameras = None
    if a.camera_to or a.quat_to:
        try:
            ends = ([float(v) for v in a.camera_to.split(",")] if a.camera_to else None, [float(v) for v in a.quat_to.split(",")] if a.quat_to else None)
            cameras = camera_path_at(position, quat, *ends, max(a.frames, 1), moments) if samples else camera_path(position, quat, *ends, max(a.frames, 1))
        except ValueError as e:
            ap.error(f"--camera-to / --quat-to: {e}")
    exposures = []
    result = render(a.metric, w, h, a.scripts, cfg, position, quat, a.redshift, a.adaptive,
                    read_png(a.background) if a.background else None, a.device, a.fov, a.universe, geodesic_speed=speed,
                    geodesic_times=[a.geodesic_time + float(t) * a.geodesic_dt for t in moments] if samples else times,
                    parallel_transport=not a.recompute_tetrads, supersample=a.supersample,
                    rgba8=a.encode == "device" and not video, mips=a.mips, yuv420=video, cameras=cameras, bit_depth=a.bit_depth, shutter_samples=samples,
                    filter=a.filter, png=a.png, jpeg=a.jpeg, quality=a.quality or 90, png_stream=a.png_stream, sky=sky, glare=glare, exr=a.exr, tone=tone, exposures=exposures)
    if speed is None and cameras is None:
        result = [result]
    if tone is not None and tone.mode == gra.TONE_AUTO:
        for i, (stops, gain) in enumerate(exposures):
            print(f"frame {i}: exposure {stops:+.4f} stops (gain {gain:.6g})")
    if video:
        with Y4MWriter(a.out, w, h, fps, bit_depth=a.bit_depth) as stream:
            for frame in result:
                stream.write(frame)
        print(f"wrote {a.out} ({w}x{h}, {len(result)} frames at {fps[0]}/{fps[1]} a second, {'10-bit ' if a.bit_depth == 10 else ''}BT.709 Y'CbCr 4:2:0)")
        return 0
    if avi:
        with AviWriter(a.out, w, h, fps) as stream:
            for frame in result:
                stream.write(frame)
        print(f"wrote {a.out} ({w}x{h}, {len(result)} frames at {fps[0]}/{fps[1]} a second, Motion-JPEG at quality {a.quality})")
        return 0
    stem, ext = os.path.splitext(a.out)
    for i, frame in enumerate(result):
        path = a.out if len(result) == 1 else f"{stem}_{i:03d}{ext}"
        write(path, frame)
        print(f"wrote {path} ({w}x{h})" if speed is None and cameras is None else
              f"wrote {path} ({w}x{h}, proper time {times[i]:.3f})" if cameras is None else f"wrote {path} ({w}x{h}, pose {i})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
