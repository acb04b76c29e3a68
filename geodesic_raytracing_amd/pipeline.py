"""Thin object layer over the C ABI: Metric, Program, RenderState (host mirror of the reference's
metric_manager / render_state roles).  All compute happens inside libgeodesic_hip.so."""
import collections
import ctypes
import os

import numpy as np

from . import (AnalyticSkyStruct, GlareStruct, ToneStruct, TONE_AUTO, TONE_MANUAL, TONE_CURVE_NAMES, METER_COUNTERS, GLARE_MAX_COMPONENTS, StarSkyStruct, Camera, Features, FrameOptions, FILTER_BOX, FILTER_MAX_TAPS, FILTER_NAMES, FRAME_F32, FRAME_RGBA8, FRAME_YUV420, FRAME_YUV420P10, YUV420_I420, GeodesicError, MetricInfo, MODE_FUSED, STAGE_NAMES, c_float, c_int,
               c_size_t, c_void_p, check, lib)

LIGHTRAY_DTYPE = np.dtype([("position", "<f4", 4), ("velocity", "<f4", 4), ("initial_quat", "<f4", 4),
                           ("acceleration", "<f4", 4), ("ku_uobsu", "<f4"), ("running_dlambda_dnew", "<f4"),
                           ("terminated", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("pad", "<i4", 3)])
RENDER_DATA_DTYPE = np.dtype([("tex_coord", "<f4", 2), ("z_shift", "<f4"), ("sx", "<i4"), ("sy", "<i4"),
                              ("terminated", "<i4"), ("side", "<i4"), ("pad", "<i4")])
assert LIGHTRAY_DTYPE.itemsize == 96 and RENDER_DATA_DTYPE.itemsize == 32


def default_features(**overrides):
    f = Features()
    lib.gr_features_default(ctypes.byref(f))
    for k, v in overrides.items():
        setattr(f, k, v)
    return f


def default_camera(position=None, quat=None):
    c = Camera()
    lib.gr_camera_default(ctypes.byref(c))
    if position is not None:
        c.position = (c_float * 4)(*position)
    if quat is not None:
        c.quat = (c_float * 4)(*quat)
    return c


def frame_options(**overrides):
    o = FrameOptions()
    lib.gr_frame_options_default(ctypes.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


class Metric:
    """A loaded metric: config + symbolic descriptor (metrics::metric in the reference, metric.hpp:710-715)."""

    def __init__(self, name, scripts_dir=None, _settings=None):
        self.handle = c_void_p()
        self.name = name
        self.stored_strings = None
        if _settings is not None:
            info, names, defaults = _settings
            n = len(names)
            check(lib.gr_metric_from_info(ctypes.byref(info), (ctypes.c_char_p * max(n, 1))(*[v.encode() for v in names]),
                                          (c_float * max(n, 1))(*defaults), ctypes.byref(self.handle)))
        elif scripts_dir is None:
            check(lib.gr_metric_builtin(name.encode(), ctypes.byref(self.handle)))
        else:
            check(lib.gr_metric_load_script(str(scripts_dir).encode(), name.encode(), ctypes.byref(self.handle)))
        self.info = MetricInfo()
        check(lib.gr_metric_get_info(self.handle, ctypes.byref(self.info)))
        n = self.info.num_dynamic_vars
        self.dynamic_vars = [lib.gr_metric_dynamic_var_name(self.handle, i).decode() for i in range(n)]
        self.dynamic_defaults = [lib.gr_metric_dynamic_var_default(self.handle, i) for i in range(n)]

    @classmethod
    def from_info(cls, name, info, dynamic_vars, dynamic_defaults, argument_strings=None):
        """gr_metric_from_info: a metric that is only the settings the frame driver reads (info: dict of gr_metric_info's fields).
        argument_strings = {False: dynamic string, True: substituted string} lets argument_string() hand back stored strings."""
        mi = MetricInfo()
        for k, v in info.items():
            setattr(mi, k, v)
        mi.num_dynamic_vars = len(dynamic_vars)
        m = cls(name, _settings=(mi, list(dynamic_vars), [float(v) for v in dynamic_defaults]))
        m.stored_strings = dict(argument_strings or {})
        return m

    def __del__(self):
        if getattr(self, "handle", None):
            lib.gr_metric_destroy(self.handle)
            self.handle = None

    def cfg_values(self, **params):
        """$cfg values in declaration order, defaults overridden by name."""
        vals = list(self.dynamic_defaults)
        for k, v in params.items():
            vals[self.dynamic_vars.index(k)] = float(v)
        return vals

    def substituted_op_counts(self, cfg_values=None):
        """(acceleration ops, its transcendentals, coordinate ops) of the substituted program for these parameter values"""
        vals = list(cfg_values) if cfg_values is not None else self.cfg_values()
        a, t, c = c_int(), c_int(), c_int()
        check(lib.gr_metric_substituted_op_counts(self.handle, (c_float * len(vals))(*vals), len(vals), ctypes.byref(a), ctypes.byref(t), ctypes.byref(c)))
        return a.value, t.value, c.value

    def evaluate(self, what, position, velocity=None, cfg_values=None):
        """gr_metric_evaluate: the metric's generated expressions at one point, on the host, in double (numpy array: 16 g_ij row-major,
        64 d g_ij / d x^k as [k][i][j], 4 accelerations, 4 polar / chart coordinates, or 1 distance)"""
        from . import lib as _lib
        n = _lib.gr_metric_evaluate_count(int(what))
        out = (ctypes.c_double * max(n, 1))()
        pos = (ctypes.c_double * 4)(*[float(x) for x in position])
        vel = (ctypes.c_double * 4)(*[float(x) for x in velocity]) if velocity is not None else None
        vals = (c_float * len(cfg_values))(*cfg_values) if cfg_values is not None else None
        check(_lib.gr_metric_evaluate(self.handle, int(what), pos, vel, vals, len(cfg_values) if cfg_values is not None else 0, out, n))
        return np.array(out[:n], dtype=np.float64)

    def features(self, **overrides):
        """feature struct with this metric's error tolerance (metric_manager.hpp:50)."""
        return default_features(max_acceleration_change=self.info.max_acceleration_change, **overrides)

    def argument_string(self, features=None, static=False, cfg_values=None):
        if self.stored_strings is not None:
            if bool(static) not in self.stored_strings:
                raise GeodesicError(f"{self.name}: no stored {'substituted' if static else 'dynamic'} argument string")
            return self.stored_strings[bool(static)]
        fptr = ctypes.byref(features) if features is not None else None
        arr, n = None, 0
        if cfg_values is not None:
            n = len(cfg_values)
            arr = (c_float * n)(*cfg_values)
        need = c_size_t()
        lib.gr_metric_argument_string(self.handle, fptr, int(static), arr, n, None, 0, ctypes.byref(need))
        buf = ctypes.create_string_buffer(need.value)
        check(lib.gr_metric_argument_string(self.handle, fptr, int(static), arr, n, buf, need.value, ctypes.byref(need)))
        return buf.value.decode()


class Program:
    """Compiled gfx950 kernels for one argument string (cl::program in the reference)."""

    def __init__(self, argument_string, device=0):
        self.handle = c_void_p()
        self.device = device
        check(lib.gr_program_create(argument_string.encode(), device, ctypes.byref(self.handle)))

    @staticmethod
    def precompile(argument_string):
        check(lib.gr_program_precompile(argument_string.encode()))

    def kernel_info(self, name):
        v, s, l = c_int(), c_int(), c_int()
        check(lib.gr_program_kernel_info(self.handle, name.encode(), ctypes.byref(v), ctypes.byref(s), ctypes.byref(l)))
        return {"vgprs": v.value, "scratch_bytes": l.value}

    @property
    def build_key(self):
        """identity of the code object (kernel source + compile options + hiprtc version), 16 hex digits"""
        return lib.gr_program_build_key(self.handle).decode()

    @property
    def has_trace_pair(self):
        """True when the program has the two-rays-per-lane kernel (gr_trace_pair)"""
        return bool(lib.gr_program_has_trace_pair(self.handle))

    def __del__(self):
        if getattr(self, "handle", None) and not getattr(self, "borrowed", False):
            lib.gr_program_destroy(self.handle)
            self.handle = None


def _frame_arguments(metric, features, cfg_values, background=None):
    """what a frame or a snapshot hands the library for `features`, `cfg_values` and `background` ((device_ptr, width, height, levels) or
    ((ptr1, ptr2), width, height, levels)) -> (features, cfg array or None, its length, sky 1, sky 2, width, height, levels)"""
    arr, n = None, 0
    if cfg_values is not None:
        n = len(cfg_values)
        arr = (c_float * n)(*cfg_values)
    bg1 = bg2 = None
    bw = bh = bl = 0
    if background is not None:
        ptrs, bw, bh, bl = background
        bg1, bg2 = ptrs if isinstance(ptrs, tuple) else (ptrs, ptrs)
    if features is None:
        features = metric.features()
    return features, arr, n, bg1, bg2, bw, bh, bl


class TiledFrame:
    """One participant of a frame split over several GPUs through the C ABI (gr_tiled_*, csrc/tiled.cpp): renders this
    participant's share of the rows and ships the finished float4 blocks straight to their place in participant 0's frame.
    TiledFrame(world, rank, device, unique_id, ...): one process per GPU, RCCL (unique_id = TiledFrame.unique_id() made on rank 0
    and distributed by the caller, e.g. torch.distributed.broadcast).  TiledFrame.local(devices, ...): one process, peer copies."""

    def __init__(self, world, rank, device, unique_id, width, height, block_rows=48, _handle=None):
        self.world, self.rank, self.device = world, rank, device
        if _handle is not None:
            self.handle = _handle
            return
        self.handle = c_void_p()
        buf = (ctypes.c_char * 128).from_buffer_copy(bytes(unique_id)) if unique_id is not None else None
        check(lib.gr_tiled_create(world, rank, device, buf, width, height, block_rows, ctypes.byref(self.handle)))

    @staticmethod
    def unique_id():
        buf = (ctypes.c_char * 128)()
        check(lib.gr_tiled_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def ipc(world, rank, device, session, width, height, block_rows=48):
        """one process per participant, participants may share a device (gr_tiled_create_ipc: RCCL's call pattern over inter-process
        memory handles; collective)"""
        handle = c_void_p()
        check(lib.gr_tiled_create_ipc(world, rank, device, str(session).encode(), width, height, block_rows, ctypes.byref(handle)))
        return TiledFrame(world, rank, device, None, width, height, block_rows, _handle=handle)

    @staticmethod
    def local(devices, width, height, block_rows=48):
        n = len(devices)
        handles = (c_void_p * n)()
        check(lib.gr_tiled_create_local(n, (c_int * n)(*devices), width, height, block_rows, handles))
        return [TiledFrame(n, r, devices[r], None, width, height, block_rows, _handle=c_void_p(handles[r])) for r in range(n)]

    def share(self, rotation):
        return lib.gr_tiled_share(self.handle, rotation)

    def render(self, state, program, metric, camera, frame_ptr, background=None, features=None, cfg_values=None, options=None, stream=None,
               rotation=0):
        """this participant's share of a float frame from a state of factor 1 (gr_render_frame_tiled)"""
        self._render(None, state, program, metric, camera, frame_ptr, background, features, cfg_values, options, stream, rotation)

    def render_as(self, state, program, metric, camera, frame_ptr, background=None, features=None, cfg_values=None, options=None, stream=None,
                  rotation=0, rgba8=False):
        """render() for a state of any supersampling factor, in either format (gr_render_frame_tiled_as): the share is traced at the state's
        factor and resolved on this participant's device; rgba8 = True ships it as 8-bit sRGB, 4 bytes a pixel, and `frame_ptr` (on
        participant 0's device) is then width*height*4 bytes - RenderState.render_rgba8's bytes."""
        self._render(FRAME_RGBA8 if rgba8 else FRAME_F32, state, program, metric, camera, frame_ptr, background, features, cfg_values, options, stream, rotation)

    def _render(self, frame_format, state, program, metric, camera, frame_ptr, background, features, cfg_values, options, stream, rotation):
        features, arr, n, bg1, bg2, bw, bh, bl = _frame_arguments(metric, features, cfg_values, background)
        args = (self.handle, state.handle, program.handle, metric.handle, stream, ctypes.byref(camera), ctypes.byref(features), arr, n, bg1, bg2, bw, bh, bl,
                frame_ptr, ctypes.byref(options) if options is not None else None, rotation)
        check(lib.gr_render_frame_tiled(*args) if frame_format is None else lib.gr_render_frame_tiled_as(*args, frame_format))

    def join(self, stream=None):
        check(lib.gr_tiled_join(self.handle, stream))

    def close(self):
        if self.handle:
            lib.gr_tiled_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ProgramManager:
    """metric_manager (metric_manager.hpp:19-219) - a thin caller of gr_program_manager_* (csrc/capi.cpp): the "dynamic" program
    (reads $cfg / features from memory) is usable at once; the "substituted" program with every parameter baked in is built in
    the background and swapped in when ready.  Changing a parameter (`update`) falls back to the dynamic program until the new
    substituted one is built."""

    def __init__(self, metric, device=0, features=None, cfg_values=None):
        self.metric, self.device = metric, device
        self.handle = c_void_p()
        arr, n = self._values(cfg_values)
        check(lib.gr_program_manager_create(metric.handle, device, ctypes.byref(features) if features is not None else None, arr, n,
                                            ctypes.byref(self.handle)))
        self._dynamic_handle = c_void_p(lib.gr_program_manager_dynamic(self.handle))
        self.features = features if features is not None else metric.features()
        self.cfg_values = list(cfg_values) if cfg_values is not None else metric.cfg_values()
        self.is_substituted = False

    @staticmethod
    def _values(cfg_values):
        if cfg_values is None:
            return None, 0
        return (c_float * len(cfg_values))(*cfg_values), len(cfg_values)

    def _borrowed(self, handle):
        p = Program.__new__(Program)          # the manager owns the program: no gr_program_destroy from this wrapper
        p.handle, p.device, p.borrowed = handle, self.device, True
        p._owner = self                       # ... and lives as long as a program it handed out (ProgramManager(...).current() on a temporary)
        return p

    @property
    def dynamic(self):
        """the dynamic program (usable whatever the parameters)"""
        return self._borrowed(self._dynamic_handle)

    def update(self, features=None, cfg_values=None):
        arr, n = self._values(cfg_values)
        check(lib.gr_program_manager_update(self.handle, ctypes.byref(features) if features is not None else None, arr, n))
        if features is not None:
            self.features = features
        if cfg_values is not None:
            self.cfg_values = list(cfg_values)

    def current(self, wait=False):
        """the program to launch this frame"""
        handle, swapped = c_void_p(), c_int()
        check(lib.gr_program_manager_current(self.handle, int(bool(wait)), ctypes.byref(handle), ctypes.byref(swapped)))
        self.is_substituted = bool(swapped.value)
        return self._borrowed(handle)

    def counters(self):
        """dict: updates taken, substituted programs swapped in, substituted builds started (at most one runs at a time), stale_build_running"""
        out = (ctypes.c_ulonglong * 4)()
        lib.gr_program_manager_counters(self.handle, out)
        return dict(updates=int(out[0]), swaps=int(out[1]), builds_started=int(out[2]), stale_build_running=bool(out[3]))

    def close(self):
        if getattr(self, "handle", None):
            lib.gr_program_manager_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    def __init__(self, device, nbytes):
        self.device, self.nbytes = device, nbytes
        self.ptr = c_void_p()
        check(lib.gr_device_alloc(device, nbytes, ctypes.byref(self.ptr)))

    @classmethod
    def from_numpy(cls, device, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(device, arr.nbytes)
        check(lib.gr_device_upload(device, b.ptr, arr.ctypes.data_as(c_void_p), arr.nbytes))
        return b

    def to_numpy(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib.gr_device_download(self.device, out.ctypes.data_as(c_void_p), self.ptr, out.nbytes))
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            lib.gr_device_free(self.device, self.ptr)
            self.ptr = None


def download(device, ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    check(lib.gr_device_download(device, out.ctypes.data_as(c_void_p), ptr, out.nbytes))
    return out


class PinnedBuffer:
    """Page-locked host memory (gr_host_alloc) that a device copy lands in without staging: download_async enqueues the copy on a
    stream, and view() is valid once that stream has been synchronised."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = c_void_p()
        check(lib.gr_host_alloc(self.nbytes, ctypes.byref(self.ptr)))

    def view(self, dtype=np.uint8, shape=None):
        """a numpy array over the buffer (no copy; it must not outlive the buffer)"""
        arr = np.frombuffer((ctypes.c_ubyte * self.nbytes).from_address(self.ptr.value), dtype=dtype)
        return arr if shape is None else arr[:int(np.prod(shape))].reshape(shape)

    def download_async(self, stream, device_ptr, nbytes=None):
        nbytes = self.nbytes if nbytes is None else int(nbytes)
        if nbytes > self.nbytes:
            raise ValueError(f"PinnedBuffer: {nbytes} bytes asked for, {self.nbytes} allocated")
        check(lib.gr_device_download_async(stream, self.ptr, device_ptr, nbytes))

    def free(self):
        """releases the memory (views of it are dead from here on); raises if the library refuses"""
        ptr, self.ptr = getattr(self, "ptr", None), None
        if ptr:
            check(lib.gr_host_free(ptr))

    def __del__(self):
        try:
            self.free()
        except Exception:   # (a destructor has nobody to raise to; free() called by hand does raise)
            pass


def png_encode_bound(width, height):
    """the capacity both PNG encoders ask for (gr_png_encode_bound)"""
    need = ctypes.c_size_t()
    check(lib.gr_png_encode_bound(int(width), int(height), ctypes.byref(need)))
    return need.value


def png_stream_kind(stream_kind):
    """a stream kind as the library numbers it, from its number or its name ("literals", "runs")"""
    from . import PNG_STREAM_NAMES
    if isinstance(stream_kind, str):
        if stream_kind not in PNG_STREAM_NAMES:
            raise ValueError(f"PNG stream kind {stream_kind!r} (one of {', '.join(PNG_STREAM_NAMES)})")
        return PNG_STREAM_NAMES[stream_kind]
    return int(stream_kind)


def png_encode_host(pixels, stream_kind=None):
    """the PNG file of RGBA8 pixels [H, W, 4] as bytes, by the host encoder that defines PngEncoder's stream (gr_png_encode_rgba8_host:
    Sub / Up filters, one Huffman table a frame, literals only).  stream_kind ("literals", "runs" or PNG_STREAM_*): that kind's file
    (gr_png_encode_rgba8_host_as)"""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ValueError(f"png_encode_host: an image of shape {pixels.shape} is not [H, W, 4]")
    h, w = pixels.shape[:2]
    out = np.empty(png_encode_bound(w, h), dtype=np.uint8)
    size = ctypes.c_size_t()
    if stream_kind is None:
        check(lib.gr_png_encode_rgba8_host(pixels.ctypes.data_as(c_void_p), w, h, out.ctypes.data_as(c_void_p), out.nbytes, ctypes.byref(size)))
    else:
        check(lib.gr_png_encode_rgba8_host_as(pixels.ctypes.data_as(c_void_p), w, h, out.ctypes.data_as(c_void_p), out.nbytes, ctypes.byref(size),
                                              png_stream_kind(stream_kind)))
    return out[:size.value].tobytes()


class _DeviceEncoder:
    """what PngEncoder and JpegEncoder share: the handle of a gr_png_encoder or gr_jpeg_encoder (_prefix: "gr_png_" or "gr_jpeg_"), the
    output array of the encoder's bound, and the calls both kinds answer alike (_launches: the times launch_ms returns).  ExrEncoder is the
    third (_prefix "gr_exr_"): its frames are float4 and its encode call (_encode) is gr_exr_encode_f32"""
    _encode = "encode_rgba8"

    def _create(self, bound, create, *args):
        self.handle = c_void_p()
        check(create(self.program.handle, self.width, self.height, *args, ctypes.byref(self.handle)))
        self._out = np.empty(bound(self.width, self.height), dtype=np.uint8)

    def _call(self, name, *args):
        check(getattr(lib, self._prefix + name)(self.handle, *args))

    def encode(self, device_ptr, stream=None):
        """the file of the frame at device_ptr (width x height RGBA8 pixels) as bytes: the host encoder's (png_encode_host of the same kind,
        jpeg_encode_host of the same quality) of the same pixels"""
        size = ctypes.c_size_t()
        self._call(self._encode, stream, device_ptr, self._out.ctypes.data_as(c_void_p), self._out.nbytes, ctypes.byref(size))
        return self._out[:size.value].tobytes()

    def write(self, path, device_ptr, stream=None):
        """encode() into a file; returns its size"""
        data = self.encode(device_ptr, stream)
        with open(path, "wb") as f:
            f.write(data)
        return len(data)

    def time_launches(self, on=True):
        self._call("encoder_time_launches", int(bool(on)))

    def launch_ms(self):
        """the encoder's launches of the last encode after time_launches(), in milliseconds: (gr_png_histogram, gr_png_pack - or their _runs
        instances), or (gr_jpeg_blocks, gr_jpeg_pack, gr_jpeg_gather)"""
        ms = (c_float * self._launches)()
        self._call("encoder_launch_ms", ms)
        return tuple(ms)

    def scratch_intact(self):
        """True when nothing was written in the encoder's scratch outside what its encodes may write: the guard words, and what lies behind
        the longest stream (PNG) or file (JPEG) it has made"""
        intact = c_int()
        self._call("encoder_scratch_intact", ctypes.byref(intact))
        return bool(intact.value)

    def close(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle:
            getattr(lib, self._prefix + "encoder_destroy")(handle)

    def __del__(self):
        self.close()


class PngEncoder(_DeviceEncoder):
    """A PNG encoder behind RGBA8 frames of one size that are already on the program's device (gr_png_encoder): filtering, histogram and
    bit-packing run there, the compressed bytes come back.  encode() synchronises the stream it is given.  The program must outlive it.
    stream_kind ("literals", "runs" or PNG_STREAM_*): the stream its files are written in (gr_png_encoder_create_as); None: literals."""
    _prefix, _launches = "gr_png_", 2

    def __init__(self, program, width, height, stream_kind=None):
        self.program, self.width, self.height = program, int(width), int(height)   # (the program is borrowed: kept alive here)
        self.stream_kind = 0 if stream_kind is None else png_stream_kind(stream_kind)
        if stream_kind is None:
            self._create(png_encode_bound, lib.gr_png_encoder_create)
        else:
            self._create(png_encode_bound, lib.gr_png_encoder_create_as, self.stream_kind)


def exr_encode_bound(width, height):
    """the capacity both EXR encoders ask for (gr_exr_encode_bound): the size of the file whose every row is stored raw"""
    need = ctypes.c_size_t()
    check(lib.gr_exr_encode_bound(int(width), int(height), ctypes.byref(need)))
    return need.value


def exr_half_bits(values):
    """the half-float bit patterns (uint16, the shape of `values`) the EXR encoders make of float32 values: NaN -> +0, clamped to +-65504,
    round to nearest even with subnormals kept (gr_exr_half_bits)"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(values.shape, np.uint16)
    check(lib.gr_exr_half_bits(values.ctypes.data_as(c_void_p), values.size, out.ctypes.data_as(c_void_p)))
    return out


def exr_encode_host(frame):
    """the OpenEXR file of a float32 frame [H, W, 4] (alpha ignored) as bytes, by the host encoder that defines ExrEncoder's file
    (gr_exr_encode_f32_host: half-float B, G, R planes, ZIPS - one zlib stream a scan line, one Huffman table a frame, literals only, rows
    that do not shrink stored raw)"""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4:
        raise ValueError(f"exr_encode_host: a frame of shape {frame.shape} is not [H, W, 4]")
    h, w = frame.shape[:2]
    if frame.ctypes.data % 16:   # (the encoder takes what a device frame is: 16-byte aligned pixels)
        aligned = np.empty(frame.size + 4, np.float32)
        start = (-aligned.ctypes.data % 16) // 4
        aligned = aligned[start:start + frame.size].reshape(frame.shape)
        aligned[...] = frame
        frame = aligned
    out = np.empty(exr_encode_bound(w, h), dtype=np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_exr_encode_f32_host(frame.ctypes.data_as(c_void_p), w, h, out.ctypes.data_as(c_void_p), out.nbytes, ctypes.byref(size)))
    return out[:size.value].tobytes()


class ExrEncoder(_DeviceEncoder):
    """An OpenEXR encoder behind float4 frames of one size that are already on the program's device (gr_exr_encoder): half conversion,
    predictor, histogram and bit-packing run there, the file's chunks come back.  encode() takes the float4 frame's device pointer, gives
    exr_encode_host's bytes of the same pixels and synchronises the stream it is given.  The program must outlive it."""
    _prefix, _launches, _encode = "gr_exr_", 2, "encode_f32"

    def __init__(self, program, width, height):
        self.program, self.width, self.height = program, int(width), int(height)   # (the program is borrowed: kept alive here)
        self._create(exr_encode_bound, lib.gr_exr_encoder_create)


def jpeg_encode_bound(width, height):
    """the capacity both JPEG encoders ask for (gr_jpeg_encode_bound)"""
    need = ctypes.c_size_t()
    check(lib.gr_jpeg_encode_bound(int(width), int(height), ctypes.byref(need)))
    return need.value


def jpeg_quant_tables(quality):
    """(luminance, chrominance): the quantiser's steps at a quality of 1 ... 100 as uint8 [8, 8] in natural order (gr_jpeg_quant_tables)"""
    luma, chroma = np.empty((8, 8), np.uint8), np.empty((8, 8), np.uint8)
    check(lib.gr_jpeg_quant_tables(int(quality), luma.ctypes.data_as(c_void_p), chroma.ctypes.data_as(c_void_p)))
    return luma, chroma


def jpeg_encode_host(pixels, quality=90):
    """the baseline JPEG file of RGBA8 pixels [H, W, 4] (alpha ignored) as bytes, by the host encoder that defines JpegEncoder's stream
    (gr_jpeg_encode_rgba8_host: JFIF, 4:2:0, the Annex K tables, one restart interval an MCU row)"""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim != 3 or pixels.shape[2] != 4:
        raise ValueError(f"jpeg_encode_host: an image of shape {pixels.shape} is not [H, W, 4]")
    h, w = pixels.shape[:2]
    out = np.empty(jpeg_encode_bound(w, h), dtype=np.uint8)
    size = ctypes.c_size_t()
    check(lib.gr_jpeg_encode_rgba8_host(pixels.ctypes.data_as(c_void_p), w, h, int(quality), out.ctypes.data_as(c_void_p), out.nbytes, ctypes.byref(size)))
    return out[:size.value].tobytes()


class JpegEncoder(_DeviceEncoder):
    """A JPEG encoder behind RGBA8 frames of one size that are already on the program's device (gr_jpeg_encoder): colour conversion, DCT,
    quantiser, Huffman coding and byte stuffing run there, the file's bytes come back.  encode() synchronises the stream it is given.  The
    program must outlive it."""
    _prefix, _launches = "gr_jpeg_", 3

    def __init__(self, program, width, height, quality=90):
        self.program, self.width, self.height, self.quality = program, int(width), int(height), int(quality)   # (the program is borrowed: kept alive here)
        self._create(jpeg_encode_bound, lib.gr_jpeg_encoder_create, self.quality)


class AnalyticSky:
    """gr_analytic_sky: a coloured celestial sphere with a latitude / longitude grid, shaded on the device in closed form from the pixel's
    footprint (include/geodesic_hip_internal.h, "Analytic sky").  The library's defaults, then the overrides: meridians (2 ... 360),
    parallels (1 ... 180), line_width (0 ... 0.5 of a cell), quadrant [2][4][3] and line [2][3] (stored sRGB values in [0, 1];
    [side][q][rgb], q = (u >= 0.5) + 2 (v >= 0.5), side 0 the far sky, side 1 the near one).  Hand it to RenderState(sky=...) or
    RenderState.set_sky; the library refuses a field out of range there."""

    def __init__(self, meridians=None, parallels=None, line_width=None, quadrant=None, line=None):
        self.struct = AnalyticSkyStruct()
        check(lib.gr_analytic_sky_default(ctypes.byref(self.struct)))
        if meridians is not None:
            self.struct.meridians = int(meridians)
        if parallels is not None:
            self.struct.parallels = int(parallels)
        if line_width is not None:
            self.struct.line_width = float(line_width)
        if quadrant is not None:
            self.quadrant = quadrant
        if line is not None:
            self.line = line

    meridians = property(lambda self: self.struct.meridians)
    parallels = property(lambda self: self.struct.parallels)
    line_width = property(lambda self: self.struct.line_width)

    @property
    def quadrant(self):
        return np.ctypeslib.as_array(self.struct.quadrant).copy()

    @quadrant.setter
    def quadrant(self, value):
        np.ctypeslib.as_array(self.struct.quadrant)[...] = np.asarray(value, dtype=np.float32).reshape(2, 4, 3)

    @property
    def line(self):
        return np.ctypeslib.as_array(self.struct.line).copy()

    @line.setter
    def line(self, value):
        np.ctypeslib.as_array(self.struct.line)[...] = np.asarray(value, dtype=np.float32).reshape(2, 3)

    def image(self, width, height, side=1):
        """the same sky as an image, uint8 [height][width][4] (gr_analytic_sky_image: the definition in double at one texel's footprint)"""
        out = np.empty((int(height), int(width), 4), dtype=np.uint8)
        check(lib.gr_analytic_sky_image(ctypes.byref(self.struct), int(side), int(width), int(height), out.ctypes.data_as(c_void_p)))
        return out


def star_field_random(seed, n):
    """gr_star_field_random: n stars uniform on the sphere from a splitmix64 stream, a power law of brightness, colours by spectral class
    (the recipe: include/geodesic_hip_internal.h, "Star sky") -> (uv float32 [n][2], flux float32 [n][3], already per unit of (u, v) area)"""
    uv, flux = np.empty((int(n), 2), dtype=np.float32), np.empty((int(n), 3), dtype=np.float32)
    check(lib.gr_star_field_random(int(seed), int(n), uv.ctypes.data_as(c_void_p), flux.ctypes.data_as(c_void_p)))
    return uv, flux


class StarCatalogue:
    """gr_star_catalogue: n point stars - uv [n][2] in tex_coord's sky coordinates, flux [n][3] linear RGB per unit of (u, v) area - binned,
    ordered and summed on the program's device (kernels/stars.hip).  cells_u x cells_v: powers of two, 16 ... 4096 (None: 1024 x 512).
    The program is borrowed for the build only.  Hand it to RenderState(stars=(StarSky, near, far)) and keep it alive while frames render."""

    def __init__(self, program, uv, flux, cells_u=None, cells_v=None):
        uv, flux = np.ascontiguousarray(uv, dtype=np.float32), np.ascontiguousarray(flux, dtype=np.float32)
        if uv.ndim != 2 or uv.shape[1] != 2 or flux.shape != (uv.shape[0], 3):
            raise ValueError("uv [n][2] and flux [n][3]")
        self.handle = c_void_p()
        check(lib.gr_star_catalogue_create(program.handle, uv.shape[0], uv.ctypes.data_as(c_void_p), flux.ctypes.data_as(c_void_p), int(cells_u or 0),
                                           int(cells_v or 0), ctypes.byref(self.handle)))
        n, cu, cv = c_int(), c_int(), c_int()
        check(lib.gr_star_catalogue_info(self.handle, ctypes.byref(n), ctypes.byref(cu), ctypes.byref(cv)))
        self.n, self.cells_u, self.cells_v = n.value, cu.value, cv.value

    @classmethod
    def random(cls, program, seed, n, cells_u=None, cells_v=None):
        return cls(program, *star_field_random(seed, n), cells_u=cells_u, cells_v=cells_v)

    def download(self):
        """(cell_start int32 [cells + 1], order int32 [n], table float64 [3][cells_v + 1][cells_u + 1]) as the device holds them"""
        cell_start = np.empty(self.cells_u * self.cells_v + 1, dtype=np.int32)
        order = np.empty(self.n, dtype=np.int32)
        table = np.empty((3, self.cells_v + 1, self.cells_u + 1), dtype=np.float64)
        check(lib.gr_star_catalogue_download(self.handle, cell_start.ctypes.data_as(c_void_p), order.ctypes.data_as(c_void_p), table.ctypes.data_as(c_void_p)))
        return cell_start, order, table

    def close(self):
        if self.handle:
            lib.gr_star_catalogue_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        self.close()


class StarSky:
    """gr_star_sky: min_footprint (a power of two, 2^-20 ... 2^-8; the angular size below which a star is no longer a point) and
    background [2][3] (stored sRGB values in [0, 1] behind the stars; side 0 the far sky, side 1 the near one).  The library's defaults
    (2^-16, black), then the overrides."""

    def __init__(self, min_footprint=None, background=None):
        self.struct = StarSkyStruct()
        check(lib.gr_star_sky_default(ctypes.byref(self.struct)))
        if min_footprint is not None:
            self.struct.min_footprint = float(min_footprint)
        if background is not None:
            np.ctypeslib.as_array(self.struct.background)[...] = np.asarray(background, dtype=np.float32).reshape(2, 3)

    min_footprint = property(lambda self: self.struct.min_footprint)

    @property
    def background(self):
        return np.ctypeslib.as_array(self.struct.background).copy()


class RenderState:
    """Per-frame device buffers + the frame sequence (render_state.hpp:97-197, main.cpp:2244-2526)."""

    def __init__(self, width, height, device=0, supersample=1, filter=FILTER_BOX, sky=None, stars=None, glare=None, tone=None):
        """supersample = f > 1 (gr_render_state_create_supersampled; 2, 3 or 4): frames are still width x height, traced at f x that per
        axis and box-averaged on the device (box_resolve says what that means).  Everything else about the state - buffer(), the
        prepass grid, tile history - is of traced_size.  filter (gr_render_state_set_filter): FILTER_BOX, or FILTER_TENT / _GAUSSIAN /
        _MITCHELL or their names - every frame of the state is then filter_frame of the traced frame with filter_taps' table, at
        factor 1 too, whole frames only.  sky (gr_render_state_set_sky): an AnalyticSky - every frame of the state is then shaded from
        it by gr_render_analytic, and render() needs no background.  stars (gr_render_state_set_stars): (StarSky, near StarCatalogue or None, far
        StarCatalogue or None) - every frame is shaded by gr_render_stars from the catalogues; not together with sky.  glare
        (gr_render_state_set_glare): a GlareStruct (glare_gaussians, glare_exposure) - every frame delivered is then glare_frame of the
        frame the state would have delivered as float4, applied on the device before the encode; whole frames only.  tone
        (gr_render_state_set_tone): a ToneStruct (pipeline.tone) - every frame delivered is then metered (auto mode), exposed and put through
        the tone curve on the device, after the glare and before the encode: tone_frame of the frame delivered without it; whole frames only."""
        self.width, self.height, self.device = width, height, device
        self.handle = c_void_p()
        if supersample == 1:
            check(lib.gr_render_state_create(device, width, height, ctypes.byref(self.handle)))
        else:
            check(lib.gr_render_state_create_supersampled(device, width, height, int(supersample), ctypes.byref(self.handle)))
        f, tw, th = c_int(), c_int(), c_int()
        check(lib.gr_render_state_supersample(self.handle, ctypes.byref(f), ctypes.byref(tw), ctypes.byref(th)))
        self.supersample, self.traced_size = f.value, (tw.value, th.value)
        if filter != FILTER_BOX:
            self.set_filter(filter)
        if sky is not None:
            self.set_sky(sky)
        if stars is not None:
            self.set_stars(*stars)
        if glare is not None:
            self.set_glare(glare)
        if tone is not None:
            self.set_tone(tone)

    def set_tone(self, tone):
        """the exposure and tone curve of the frames from here on (a ToneStruct), or None: frames as they were; the adaptation starts again"""
        check(lib.gr_render_state_set_tone(self.handle, ctypes.byref(tone) if tone is not None else None))

    @property
    def tone(self):
        """the state's ToneStruct, or None"""
        out, is_set = ToneStruct(), c_int()
        check(lib.gr_render_state_tone(self.handle, ctypes.byref(out), ctypes.byref(is_set)))
        return out if is_set.value else None

    def exposure(self, stream=None):
        """(stops, gain) of the last delivered frame of a state with a tone (gr_render_state_exposure): waits for `stream`"""
        stops, gain = c_float(), c_float()
        check(lib.gr_render_state_exposure(self.handle, stream, ctypes.byref(stops), ctypes.byref(gain)))
        return stops.value, gain.value

    def set_glare(self, glare):
        """the PSF and exposure of the frames from here on (a GlareStruct), or None: frames as they were"""
        check(lib.gr_render_state_set_glare(self.handle, ctypes.byref(glare) if glare is not None else None))

    @property
    def glare(self):
        """the state's GlareStruct, or None"""
        out, is_set = GlareStruct(), c_int()
        check(lib.gr_render_state_glare(self.handle, ctypes.byref(out), ctypes.byref(is_set)))
        return out if is_set.value else None

    def set_stars(self, star_sky, near=None, far=None):
        """the stars of the frames from here on: a StarSky and the catalogues of the near and the far side (either may be None: no stars
        there), or set_stars(None): back to the background textures.  The state keeps the catalogues alive."""
        check(lib.gr_render_state_set_stars(self.handle, ctypes.byref(star_sky.struct) if star_sky is not None else None,
                                            near.handle if near is not None and star_sky is not None else None,
                                            far.handle if far is not None and star_sky is not None else None))
        self._stars = (star_sky, near, far) if star_sky is not None else None

    @property
    def stars(self):
        """(StarSky, near, far) as set, or None"""
        out, near, far, is_set = StarSky(), c_void_p(), c_void_p(), c_int()
        check(lib.gr_render_state_stars(self.handle, ctypes.byref(out.struct), ctypes.byref(near), ctypes.byref(far), ctypes.byref(is_set)))
        if not is_set.value:
            return None
        return (out,) + tuple(getattr(self, "_stars", None)[1:])

    def set_sky(self, sky):
        """the analytic sky of the frames from here on (an AnalyticSky), or None: back to the background textures"""
        check(lib.gr_render_state_set_sky(self.handle, ctypes.byref(sky.struct) if sky is not None else None))

    @property
    def sky(self):
        """the state's AnalyticSky, or None"""
        out, is_set = AnalyticSky(), c_int()
        check(lib.gr_render_state_sky(self.handle, ctypes.byref(out.struct), ctypes.byref(is_set)))
        return out if is_set.value else None

    def set_filter(self, filter):
        """the reconstruction filter of the frames from here on: a FILTER_* value or a name (box, tent, gaussian, mitchell)"""
        if isinstance(filter, str):
            if filter not in FILTER_NAMES:
                raise ValueError(f"RenderState.set_filter: filter={filter!r} ({', '.join(FILTER_NAMES)})")
            filter = FILTER_NAMES[filter]
        check(lib.gr_render_state_set_filter(self.handle, int(filter)))

    @property
    def filter(self):
        value = c_int()
        check(lib.gr_render_state_filter(self.handle, ctypes.byref(value)))
        return value.value

    def __del__(self):
        if getattr(self, "handle", None):
            lib.gr_render_state_destroy(self.handle)
            self.handle = None

    def render(self, program, metric, camera, out_ptr, background=None, features=None, cfg_values=None, options=None, stream=None, rgba8=False,
               yuv420=None, bit_depth=8):
        """Enqueue one frame. `out_ptr`: device pointer to float4[width*height] (or None to stop after render-data);
        `background`: (device_ptr, width, height, levels) or ((ptr1, ptr2), width, height, levels).  yuv420 = a layout: render_yuv420, or
        with bit_depth = 10 render_yuv420p10."""
        if bit_depth not in (8, 10) or (bit_depth == 10 and yuv420 is None):
            raise ValueError(f"RenderState.render: bit_depth={bit_depth!r} (8, or 10 with a yuv420 layout)")
        features, arr, n, bg1, bg2, bw, bh, bl = _frame_arguments(metric, features, cfg_values, background)
        options = ctypes.byref(options) if options is not None else None
        fmt = FRAME_FORMATS[frame_format_of(rgba8, yuv420 is not None, bit_depth)]
        layout = (int(yuv420),) if fmt.takes_layout else ()
        check(getattr(lib, fmt.entry)(self.handle, program.handle, metric.handle, stream, ctypes.byref(camera), ctypes.byref(features), arr, n, bg1, bg2,
                                      bw, bh, bl, out_ptr, *layout, options))

    def render_rgba8(self, program, metric, camera, out_ptr, background=None, features=None, cfg_values=None, options=None, stream=None):
        """render(), delivered as 8-bit sRGB (gr_render_frame_rgba8): `out_ptr` is a device pointer to width*height*4 bytes, R G B A, rows
        laid out as render() lays out its float rows; every byte is encode_srgb8's of the float render() writes (a NaN gives 0)."""
        self.render(program, metric, camera, out_ptr, background, features, cfg_values, options, stream, rgba8=True)

    def render_yuv420(self, program, metric, camera, out_ptr, background=None, features=None, cfg_values=None, options=None, stream=None,
                      layout=YUV420_I420):
        """render(), delivered as 8-bit BT.709 Y'CbCr 4:2:0 (gr_render_frame_yuv420): `out_ptr` is a device pointer to
        yuv420_bytes(width, height) bytes, aligned to 4, in `layout` (YUV420_I420: planes Y, Cb, Cr; YUV420_NV12: Y, then Cb Cr pairs);
        every byte is rgba8_to_yuv420's of the frame render_rgba8() writes.  Whole frames only."""
        if layout is None:   # (render() would take that for "no video format" and deliver float4 into a buffer of 1.5 bytes a pixel)
            raise ValueError("RenderState.render_yuv420: layout=None (YUV420_I420 or YUV420_NV12)")
        self.render(program, metric, camera, out_ptr, background, features, cfg_values, options, stream, yuv420=layout)

    def render_yuv420p10(self, program, metric, camera, out_ptr, background=None, features=None, cfg_values=None, options=None, stream=None,
                         layout=YUV420_I420):
        """render(), delivered as 10-bit BT.709 Y'CbCr 4:2:0 in 16-bit words (gr_render_frame_yuv420p10): `out_ptr` is a device pointer to
        yuv420p10_bytes(width, height) bytes, aligned to 8 where the width is a multiple of 4 and to 2 otherwise, in `layout` (YUV420_I420:
        yuv420p10le, planes Y, Cb, Cr; YUV420_NV12: P010, Y then Cb Cr pairs, codes in the high ten bits); every word is
        rgb10_to_yuv420p10(frame_to_rgb10(...))'s of the float frame render() writes (a NaN gives code 0).  Whole frames only."""
        if layout is None:
            raise ValueError("RenderState.render_yuv420p10: layout=None (YUV420_I420 or YUV420_NV12)")
        self.render(program, metric, camera, out_ptr, background, features, cfg_values, options, stream, yuv420=layout, bit_depth=10)

    def render_subframe(self, program, metric, camera, weight, first, background=None, features=None, cfg_values=None, options=None, stream=None):
        """One sub-frame of a shutter (gr_render_subframe): the frame render() would write for these arguments is rendered into the state's own
        traced frame and added on the device, times `weight`, to an accumulation frame the state keeps: accum = weight * frame with `first`,
        accum = accum + weight * frame otherwise (accumulate_frame says what that means, bit for bit).  The weights are the caller's and
        are not normalised; `options` are render()'s, next_camera for the next sub-frame's pose included.  Whole frames only."""
        features, arr, n, bg1, bg2, bw, bh, bl = _frame_arguments(metric, features, cfg_values, background)
        options = ctypes.byref(options) if options is not None else None
        check(lib.gr_render_subframe(self.handle, program.handle, metric.handle, stream, ctypes.byref(camera), ctypes.byref(features), arr, n,
                                     bg1, bg2, bw, bh, bl, float(weight), int(bool(first)), options))

    def deliver_accumulated(self, program, out_ptr, frame_format=FRAME_F32, layout=YUV420_I420, stream=None):
        """The accumulation of the sub-frames since the last `first` one, delivered by one launch (gr_deliver_accumulated) into the device
        pointer `out_ptr` as FRAME_F32 (float4[width*height]), FRAME_RGBA8 (what render_rgba8 would make of it), FRAME_YUV420 (render_yuv420;
        yuv420_bytes, aligned to 4) or FRAME_YUV420P10 (render_yuv420p10; yuv420p10_bytes, aligned to 8 where the width is a multiple of 4) in
        `layout`.  The accumulation stays: it can be delivered again in another format."""
        check(lib.gr_deliver_accumulated(self.handle, program.handle, stream, int(frame_format), int(layout), out_ptr))

    def prepass_policy(self):
        """(frames rendered with a prepass, frames the policy rendered without, fraction of cells the last inspected prepass marked)"""
        a, b, f = ctypes.c_ulonglong(), ctypes.c_ulonglong(), c_float()
        check(lib.gr_render_state_prepass_policy(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(f)))
        return a.value, b.value, f.value

    def prepass_reused(self):
        """frames that took the previous frame's camera set-up and prepass as they stood (gr_frame_tuning.reuse_still_camera)"""
        n = ctypes.c_ulonglong()
        check(lib.gr_render_state_prepass_reused(self.handle, ctypes.byref(n)))
        return n.value

    def tile_history(self):
        """(frames that recorded their tiles' costs, frames that followed the costs of the frame before, the last such frame's shift in tiles)"""
        a, b, shift = ctypes.c_ulonglong(), ctypes.c_ulonglong(), (ctypes.c_int * 2)()
        check(lib.gr_render_state_tile_history(self.handle, ctypes.byref(a), ctypes.byref(b), shift))
        return a.value, b.value, (shift[0], shift[1])

    def stage_ms(self):
        out = {}
        for i, name in enumerate(STAGE_NAMES):
            ms = c_float()
            check(lib.gr_render_state_stage_ms(self.handle, i, ctypes.byref(ms)))
            out[name] = ms.value
        return out

    def resolve_ms(self):
        """the resolve launch of the last frame rendered with frame_options(time_kernels=1) by a supersampled state (0.0: it launched none)"""
        ms = c_float()
        check(lib.gr_render_state_resolve_ms(self.handle, ctypes.byref(ms)))
        return ms.value

    def trace_log(self, reset=True):
        """(sum of durations in ms, number) of the trace launches logged with frame_options(time_kernels=2)"""
        total, n = c_float(), ctypes.c_int()
        check(lib.gr_render_state_trace_log(self.handle, ctypes.byref(total), ctypes.byref(n), int(reset)))
        return total.value, n.value

    def shader_clock_mhz(self):
        """average shader clock of the last fused trace launch rendered with count_attempts (0.0 if there was none)"""
        v = ctypes.c_double(0)
        check(lib.gr_render_state_shader_clock(self.handle, ctypes.byref(v)))
        return v.value

    def wave_time(self):
        """(summed wave lifetime in ms, waves) of the same launch"""
        ms, n = ctypes.c_double(0), ctypes.c_ulonglong(0)
        check(lib.gr_render_state_wave_time(self.handle, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def counters(self, count=128):
        words = (ctypes.c_ulonglong * count)()
        check(lib.gr_render_state_counters(self.handle, words, count))
        return list(words)

    def attempts(self):
        v = ctypes.c_ulonglong()
        check(lib.gr_render_state_attempts(self.handle, ctypes.byref(v)))
        return v.value

    def buffer(self, which):
        return lib.gr_render_state_buffer(self.handle, which)

    def synchronize(self):
        check(lib.gr_device_synchronize(self.device))


class GeodesicCamera:
    """Snapshot of the camera's timelike geodesic (main.cpp:2675-2760); pass `handle` as frame_options(geodesic=...)
    together with geodesic_time to render from a point on it."""

    def __init__(self, max_path_length=16384, device=0):
        self.device, self.max_path_length = device, max_path_length
        self.handle = c_void_p()
        check(lib.gr_geodesic_camera_create(device, max_path_length, ctypes.byref(self.handle)))
        self.steps, self.proper_time = 0, 0.0

    def __del__(self):
        if getattr(self, "handle", None):
            lib.gr_geodesic_camera_destroy(self.handle)
            self.handle = None

    def snapshot(self, program, metric, camera, geodesic_basis_speed, features=None, cfg_values=None, stream=None):
        features, arr, n = _frame_arguments(metric, features, cfg_values)[:3]
        steps, tau = ctypes.c_int(), c_float()
        check(lib.gr_geodesic_camera_snapshot(self.handle, program.handle, metric.handle, stream, ctypes.byref(camera),
                                              (c_float * 3)(*geodesic_basis_speed), ctypes.byref(features), arr, n,
                                              ctypes.byref(steps), ctypes.byref(tau)))
        self.steps, self.proper_time = steps.value, tau.value
        return self.steps, self.proper_time

    def interpolate(self, program, proper_time, parallel_transport=True, stream=None):
        cam, tet, vel = (c_float * 4)(), (c_float * 16)(), (c_float * 4)()
        check(lib.gr_geodesic_camera_interpolate(self.handle, program.handle, stream, float(proper_time), int(parallel_transport), cam,
                                                 tet, vel))
        return np.array(cam, dtype=np.float32), np.array(tet, dtype=np.float32).reshape(4, 4), np.array(vel, dtype=np.float32)

    def path(self):
        """(positions[n,4], velocities[n,4], ds[n]) of the current snapshot"""
        n = self.steps
        get = lambda which, dtype, count: download(self.device, lib.gr_geodesic_camera_buffer(self.handle, which), dtype, count)
        return get(0, np.float32, n * 4).reshape(n, 4), get(1, np.float32, n * 4).reshape(n, 4), get(2, np.float32, n)


def box_resolve(frame, factor):
    """What gr_resolve_supersampled computes, on the host: frame [H*f, W*f, C] -> [H, W, C], every output value the mean of its f x f
    block of `frame`, taken in float64 and rounded to float32 once.  (The kernel sums the block in fp32 and multiplies by the rounded
    1 / f^2: it agrees with this to (f^2 + 2) * 2^-24 of the block's mean magnitude, and exactly for f = 1.)"""
    frame = np.asarray(frame)
    f = int(factor)
    if f < 1 or frame.ndim != 3 or frame.shape[0] % f or frame.shape[1] % f:
        raise ValueError(f"box_resolve: a frame of shape {frame.shape} does not divide into {f} x {f} blocks")
    h, w, c = frame.shape[0] // f, frame.shape[1] // f, frame.shape[2]
    return frame.astype(np.float64).reshape(h, f, w, f, c).mean(axis=(1, 3)).astype(np.float32)


def encode_srgb8(frame):
    """The host statement of the 8-bit encode (gr_frame_to_rgba8, the reference's screenshot loop main.cpp:2791-2796): float [H, W, 4] in
    linear light -> uint8 [H, W, 4], every value clamped to [0, 1], through lin_to_srgb, clamped, times 255 and truncated.  What
    gr_present_rgba8 computes on the device (a NaN is undefined here and 0 there)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4:
        raise ValueError(f"encode_srgb8: a frame of shape {frame.shape} is not [H, W, 4]")
    out = np.empty(frame.shape, dtype=np.uint8)
    if frame.size:
        check(lib.gr_frame_to_rgba8(frame.ctypes.data_as(c_void_p), frame.shape[1], frame.shape[0], out.ctypes.data_as(c_void_p)))
    return out


def yuv420_bytes(width, height):
    """the bytes of a width x height frame in 8-bit Y'CbCr 4:2:0, either layout: width*height + 2 * ((width+1)//2) * ((height+1)//2)"""
    return int(lib.gr_yuv420_bytes(int(width), int(height)))


def rgba8_to_yuv420(pixels, layout=YUV420_I420):
    """The host statement of the video encode (gr_rgba8_to_yuv420; include/geodesic_hip.h gives the integer formulas): uint8 [H, W, 4] in
    sRGB -> uint8 [yuv420_bytes(W, H)], BT.709 limited range, one chroma pair per 2 x 2 block (an odd edge counts twice), alpha dropped.
    What gr_present_yuv420 computes on the device from the float frame, byte for byte."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim != 3 or pixels.shape[2] != 4 or pixels.size == 0:
        raise ValueError(f"rgba8_to_yuv420: a frame of shape {pixels.shape} is not [H, W, 4]")
    h, w = pixels.shape[:2]
    out = np.empty(yuv420_bytes(w, h), dtype=np.uint8)
    check(lib.gr_rgba8_to_yuv420(pixels.ctypes.data_as(c_void_p), w, h, int(layout), out.ctypes.data_as(c_void_p)))
    return out


def accumulate_frame(accum, frame, weight, first):
    """The host statement of one step of a shutter's accumulation (gr_accumulate_frame): float32 arrays of one shape, `accum` updated in
    place and returned - with `first` accum = weight * frame, otherwise accum = accum + weight * frame; one float32 multiply and one
    float32 add per value, each rounded (never a fused multiply-add).  What RenderState.render_subframe computes on the device, bit for
    bit, of the frames render() delivers.  The weights are not normalised."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if not (isinstance(accum, np.ndarray) and accum.dtype == np.float32 and accum.flags.c_contiguous and accum.flags.writeable and accum.shape == frame.shape):
        raise ValueError("accumulate_frame: accum is a writeable C-contiguous float32 array of the frame's shape")
    check(lib.gr_accumulate_frame(accum.ctypes.data_as(c_void_p), frame.ctypes.data_as(c_void_p), frame.size, float(weight), int(bool(first))))
    return accum


def filter_taps(filter, factor):
    """The table of a named filter at a supersampling factor (gr_filter_taps): float32 [n] - FILTER_TENT (radius 1), FILTER_GAUSSIAN or
    FILTER_MITCHELL (radius 2), or their names; n = 2 R f taps for an even f, 2 R f - 1 for an odd one, centred on the output pixel,
    normalised in float64 and rounded once (so they need not sum to exactly 1).  FILTER_BOX has no table."""
    if isinstance(filter, str):
        if filter not in FILTER_NAMES:
            raise ValueError(f"filter_taps: filter={filter!r} ({', '.join(FILTER_NAMES)})")
        filter = FILTER_NAMES[filter]
    taps, count = (c_float * FILTER_MAX_TAPS)(), c_int()
    check(lib.gr_filter_taps(int(filter), int(factor), taps, ctypes.byref(count)))
    return np.array(taps[:count.value], dtype=np.float32)


def filter_frame(frame, factor, taps):
    """The host statement of a filtered frame (gr_filter_frame): float32 [H*f, W*f, 4] -> [H, W, 4], the rows pass then the columns pass
    with the same table `taps` (1 to 16 values, as many modulo 2 as f), tap t on the sample at offset (f - n)/2 + t from the pixel's own
    block, samples past an edge taken from the edge; every product and every sum one rounded float32 operation in ascending t.  What a
    RenderState with a filter delivers, bit for bit, of the frame a plain state of the traced size renders."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    f = int(factor)
    if f < 1 or frame.ndim != 3 or frame.shape[2] != 4 or frame.shape[0] % f or frame.shape[1] % f or not frame.size:
        raise ValueError(f"filter_frame: a frame of shape {frame.shape} is not [H*{f}, W*{f}, 4]")
    taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    out = np.empty((frame.shape[0] // f, frame.shape[1] // f, 4), dtype=np.float32)
    check(lib.gr_filter_frame(frame.ctypes.data_as(c_void_p), out.shape[1], out.shape[0], f, taps.ctypes.data_as(c_void_p), taps.size,
                              out.ctypes.data_as(c_void_p)))
    return out


def glare_gaussians(sigma=(), weight=()):
    """The named PSF (gr_glare_gaussians): up to four Gaussians of `sigma` output pixels and `weight` in [0, 1] -> a GlareStruct with
    n = 2 min(ceil(3 sigma), 64) + 1 taps a component, normalised in float64 and rounded once, and core = 1 - the sum of the weights.  None
    given: core 1 and no component, the identity."""
    sigma, weight = np.atleast_1d(np.asarray(sigma, dtype=np.float32)), np.atleast_1d(np.asarray(weight, dtype=np.float32))
    if sigma.ndim != 1 or sigma.shape != weight.shape:
        raise ValueError("glare_gaussians: as many sigmas as weights")
    room = max(len(sigma), GLARE_MAX_COMPONENTS)   # (a count above 4 is the library's to refuse)
    s, w, out = (c_float * room)(*sigma), (c_float * room)(*weight), GlareStruct()
    check(lib.gr_glare_gaussians(s, w, len(sigma), ctypes.byref(out)))
    return out


def glare_exposure(glare, stops):
    """gr_glare_exposure: the core and the weights of `glare` times 2^stops (-32 ... 32), in place; returns it"""
    check(lib.gr_glare_exposure(ctypes.byref(glare), float(stops)))
    return glare


def glare_frame(frame, glare):
    """The host statement of the glare (gr_glare_frame): float32 [H, W, 4] -> [H, W, 4]; per component the rows pass, the columns pass
    and weight x that added to core x the frame, tap t on the sample at offset t - R, samples past an edge taken from the edge; every
    product and every sum one rounded float32 operation in the order written; alpha passes bit for bit.  What a RenderState with a glare
    delivers, bit for bit, of the frame it delivers without."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4 or not frame.size:
        raise ValueError(f"glare_frame: a frame of shape {frame.shape} is not [H, W, 4]")
    out = np.empty_like(frame)
    check(lib.gr_glare_frame(frame.ctypes.data_as(c_void_p), frame.shape[1], frame.shape[0], ctypes.byref(glare), out.ctypes.data_as(c_void_p)))
    return out


def glare_scratch_bytes(width, height):
    """the scratch apply_glare needs for a frame of that size (gr_glare_scratch_bytes)"""
    n = c_size_t()
    check(lib.gr_glare_scratch_bytes(int(width), int(height), ctypes.byref(n)))
    return n.value


def apply_glare(program, src_ptr, dst_ptr, scratch_ptr, scratch_bytes, width, height, glare, stream=None):
    """glare_frame on the program's device (gr_apply_glare), bit for bit, asynchronous on `stream`: src, dst and scratch are device
    pointers to float4[width * height] frames (scratch: glare_scratch_bytes, aligned to 16) that do not overlap"""
    check(lib.gr_apply_glare(program.handle, stream, src_ptr, dst_ptr, scratch_ptr, int(scratch_bytes), int(width), int(height), ctypes.byref(glare)))


def tone(auto=False, stops=0.0, key_stops=None, low=None, high=None, min_stops=None, max_stops=None, rate=None, curve=None, white=None):
    """A ToneStruct (gr_tone_default, then what is given): auto - the exposure is metered on the device from every frame's luminance
    histogram (the mean level of the pixels between the fractions low and high of the non-black ones goes to 2^key_stops, within
    min_stops ... max_stops, approached at `rate` a frame) - or manual `stops`; curve: "linear", "reinhard" (with `white`) or "filmic", or
    TONE_*.  The fields are checked where the struct is used."""
    t = ToneStruct()
    check(lib.gr_tone_default(ctypes.byref(t)))
    t.mode, t.stops = (TONE_AUTO if auto else TONE_MANUAL), float(stops)
    for name, value in (("key_stops", key_stops), ("low", low), ("high", high), ("min_stops", min_stops), ("max_stops", max_stops), ("rate", rate), ("white", white)):
        if value is not None:
            setattr(t, name, float(value))
    if curve is not None:
        if isinstance(curve, str) and curve not in TONE_CURVE_NAMES:
            raise ValueError(f"tone: curve {curve!r} is none of {sorted(TONE_CURVE_NAMES)}")
        t.curve = TONE_CURVE_NAMES[curve] if isinstance(curve, str) else int(curve)
    return t


def _float4_frame(who, frame):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4 or not frame.size:
        raise ValueError(f"{who}: a frame of shape {frame.shape} is not [H, W, 4]")
    return frame


def meter_histogram(frame):
    """The host statement of the meter (gr_meter_histogram_frame): float32 [H, W, 4] -> uint32 [385]: pixels by the exponent and the top
    three mantissa bits of their Rec. 709 luminance, 8 bins an octave from 2^-24; [384] counts the pixels whose luminance is not above 0"""
    frame = _float4_frame("meter_histogram", frame)
    hist = np.zeros(METER_COUNTERS, dtype=np.uint32)
    check(lib.gr_meter_histogram_frame(frame.ctypes.data_as(c_void_p), frame.shape[1], frame.shape[0], hist.ctypes.data_as(c_void_p)))
    return hist


def meter_solve(hist, tone, adapted=0.0, primed=False):
    """The host statement of the solve (gr_meter_solve_host): -> (adapted, primed, gain, q); manual mode leaves the state as given"""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    if hist.shape != (METER_COUNTERS,):
        raise ValueError(f"meter_solve: a histogram of shape {hist.shape} is not [{METER_COUNTERS}]")
    a, p, gain, q = ctypes.c_double(adapted), c_int(1 if primed else 0), c_float(), c_int()
    check(lib.gr_meter_solve_host(hist.ctypes.data_as(c_void_p), ctypes.byref(tone), ctypes.byref(a), ctypes.byref(p), ctypes.byref(gain), ctypes.byref(q)))
    return a.value, bool(p.value), np.float32(gain.value), q.value


def tone_frame(frame, tone, gain, out=None):
    """The host statement of the curve (gr_tone_frame): float32 [H, W, 4] -> [H, W, 4], r, g and b times `gain` through tone.curve, alpha
    bit for bit; out: where to (it may be `frame` itself)"""
    frame = _float4_frame("tone_frame", frame)
    if out is None:
        out = np.empty_like(frame)
    if out.shape != frame.shape or out.dtype != np.float32 or not out.flags.c_contiguous:
        raise ValueError("tone_frame: out is not a contiguous float32 frame of the source's shape")
    check(lib.gr_tone_frame(frame.ctypes.data_as(c_void_p), frame.shape[1], frame.shape[0], ctypes.byref(tone), float(gain), out.ctypes.data_as(c_void_p)))
    return out


def meter_frame(program, src_ptr, width, height, hist_ptr, stream=None):
    """meter_histogram on the program's device (gr_meter_frame), exactly, asynchronous on `stream`: 385 uint32 at hist_ptr, zeroed first"""
    check(lib.gr_meter_frame(program.handle, stream, src_ptr, int(width), int(height), hist_ptr))


def meter_solve_device(program, hist_ptr, tone, state_ptr, stream=None):
    """meter_solve on the program's device (gr_meter_solve_device), bit for bit: state_ptr is a ToneStateStruct in device memory"""
    check(lib.gr_meter_solve_device(program.handle, stream, hist_ptr, ctypes.byref(tone), state_ptr))


def apply_tone(program, src_ptr, dst_ptr, width, height, tone, gain_ptr=None, gain=1.0, stream=None):
    """tone_frame on the program's device (gr_apply_tone), bit for bit: the gain is the float at the device pointer gain_ptr, else `gain`;
    src_ptr == dst_ptr is allowed"""
    check(lib.gr_apply_tone(program.handle, stream, src_ptr, dst_ptr, int(width), int(height), ctypes.byref(tone), gain_ptr, float(gain)))


def yuv420p10_bytes(width, height):
    """the bytes of a width x height frame in 10-bit Y'CbCr 4:2:0 (16-bit words), either layout: 2 * yuv420_bytes(width, height)"""
    return int(lib.gr_yuv420p10_bytes(int(width), int(height)))


# A frame format is a FRAME_* value with a row here: the library's entry point that renders a frame in it, whether that takes a layout, the
# bytes of a width x height frame, and the numpy dtype and shape of one fetched from the device (csrc/frame_format.cpp is the library's table)
FrameFormat = collections.namedtuple("FrameFormat", "entry takes_layout bytes dtype shape")
FRAME_FORMATS = {
    FRAME_F32: FrameFormat("gr_render_frame", False, lambda w, h: w * h * 16, np.float32, lambda w, h: (h, w, 4)),
    FRAME_RGBA8: FrameFormat("gr_render_frame_rgba8", False, lambda w, h: w * h * 4, np.uint8, lambda w, h: (h, w, 4)),
    FRAME_YUV420: FrameFormat("gr_render_frame_yuv420", True, yuv420_bytes, np.uint8, lambda w, h: (yuv420_bytes(w, h),)),
    FRAME_YUV420P10: FrameFormat("gr_render_frame_yuv420p10", True, yuv420p10_bytes, np.uint16, lambda w, h: (yuv420p10_bytes(w, h) // 2,)),
}


def frame_format_of(rgba8=False, yuv420=False, bit_depth=8):
    """the FRAME_* value that render()'s three keyword arguments name between them: a video format wins over rgba8"""
    return FRAME_YUV420P10 if yuv420 and bit_depth == 10 else FRAME_YUV420 if yuv420 else FRAME_RGBA8 if rgba8 else FRAME_F32


def srgb10_thresholds():
    """gr_srgb10_thresholds: float32 [1024], T[k] = the smallest float of [0, 1] whose 10-bit sRGB code is >= k (T[0] = 0, +inf above the code
    of 1.0); the code of c is the number of k in 1 ... 1023 with T[k] <= c.  The table gr_present_yuv420p10 searches."""
    out = np.empty(1024, dtype=np.float32)
    check(lib.gr_srgb10_thresholds(out.ctypes.data_as(ctypes.POINTER(c_float))))
    return out


def frame_to_rgb10(frame):
    """The host statement of the 10-bit encode (gr_frame_to_rgb10): float [H, W, 4] in linear light -> uint16 [H, W, 3], every value of R, G,
    B clamped to [0, 1], through lin_to_srgb, clamped, times 1023 and truncated; alpha is not encoded (a NaN is undefined here, 0 on the device)."""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 4 or frame.size == 0:
        raise ValueError(f"frame_to_rgb10: a frame of shape {frame.shape} is not [H, W, 4]")
    h, w = frame.shape[:2]
    out = np.empty((h, w, 3), dtype=np.uint16)
    check(lib.gr_frame_to_rgb10(frame.ctypes.data_as(c_void_p), w, h, out.ctypes.data_as(c_void_p)))
    return out


def rgb10_to_yuv420p10(codes, layout=YUV420_I420):
    """The host statement of the 10-bit video encode (gr_rgb10_to_yuv420p10; include/geodesic_hip_internal.h gives the integer formulas):
    uint16 [H, W, 3] codes of at most 1023 -> uint16 [yuv420p10_bytes(W, H) / 2], BT.709 limited range, one chroma pair per 2 x 2 block (an
    odd edge counts twice).  YUV420_I420: yuv420p10le; YUV420_NV12: P010 (code << 6).  What gr_present_yuv420p10 computes on the device."""
    codes = np.ascontiguousarray(codes, dtype=np.uint16)
    if codes.ndim != 3 or codes.shape[2] != 3 or codes.size == 0:
        raise ValueError(f"rgb10_to_yuv420p10: codes of shape {codes.shape} are not [H, W, 3]")
    h, w = codes.shape[:2]
    out = np.empty(yuv420p10_bytes(w, h) // 2, dtype=np.uint16)
    check(lib.gr_rgb10_to_yuv420p10(codes.ctypes.data_as(c_void_p), w, h, int(layout), out.ctypes.data_as(c_void_p)))
    return out


class Y4MWriter:
    """An uncompressed YUV4MPEG2 file (gr_y4m_open / _open_depth / _write_frame / _close): one header line, then "FRAME\\n" + the I420 planes
    per frame.  fps: an int, or (numerator, denominator).  bit_depth 8: frames of yuv420_bytes uint8; 10: frames of yuv420p10_bytes / 2
    uint16 (written as little-endian words).  Use as a context manager, or call close()."""

    def __init__(self, path, width, height, fps=24, bit_depth=8):
        num, den = fps if isinstance(fps, tuple) else (fps, 1)
        self.sample = np.dtype(np.uint8) if bit_depth == 8 else np.dtype("<u2")
        self.frame_bytes = yuv420_bytes(width, height) * self.sample.itemsize
        self.handle = c_void_p()
        if bit_depth == 8:
            check(lib.gr_y4m_open(os.fsencode(path), int(width), int(height), int(num), int(den), ctypes.byref(self.handle)))
        else:
            check(lib.gr_y4m_open_depth(os.fsencode(path), int(width), int(height), int(num), int(den), int(bit_depth), ctypes.byref(self.handle)))

    def write(self, i420):
        i420 = np.ascontiguousarray(i420, dtype=self.sample)
        if i420.nbytes != self.frame_bytes:
            raise ValueError(f"Y4MWriter: a frame of {i420.nbytes} bytes, {self.frame_bytes} expected")
        check(lib.gr_y4m_write_frame(self.handle, i420.ctypes.data_as(c_void_p)))

    def close(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle:
            check(lib.gr_y4m_close(handle))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (a destructor has nobody to raise to; close() called by hand does raise)
            pass


class AviWriter:
    """A Motion-JPEG file in plain AVI 1.0 (gr_avi_open / _write_frame / _close): one '00dc' chunk per finished JPEG file, an index, sizes
    patched at close; at most 2^31 - 1 bytes.  fps: an int, or (numerator, denominator).  Use as a context manager, or call close()."""

    def __init__(self, path, width, height, fps=24):
        num, den = fps if isinstance(fps, tuple) else (fps, 1)
        self.handle = c_void_p()
        check(lib.gr_avi_open(os.fsencode(path), int(width), int(height), int(num), int(den), ctypes.byref(self.handle)))

    def write(self, jpeg):
        """appends one frame: the bytes of a JPEG file (JpegEncoder.encode, jpeg_encode_host)"""
        jpeg = bytes(jpeg)
        check(lib.gr_avi_write_frame(self.handle, jpeg, len(jpeg)))

    def close(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle:
            check(lib.gr_avi_close(handle))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # (a destructor has nobody to raise to; close() called by hand does raise)
            pass


def synthetic_background(width=1024, height=512, seed=0x5EED, stars=None):
    """Deterministic equirectangular RGBA8 sky (the reference's PNG backgrounds are missing from the checkout):
    smooth gradient + 10 degree latitude/longitude grid + point stars."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    u, v = x / width, y / height
    img = np.zeros((height, width, 4), dtype=np.float32)
    img[..., 0] = 0.15 + 0.35 * (0.5 + 0.5 * np.sin(2 * np.pi * u))
    img[..., 1] = 0.15 + 0.35 * v
    img[..., 2] = 0.25 + 0.35 * (0.5 + 0.5 * np.cos(2 * np.pi * (u + v)))
    lon = (u * 36.0) % 1.0
    lat = (v * 18.0) % 1.0
    line = (np.minimum(lon, 1 - lon) < 0.04) | (np.minimum(lat, 1 - lat) < 0.04)
    img[line, :3] = 0.9
    if stars is None:
        stars = (width * height) // 400
    sx = rs.randint(0, width, size=stars)
    sy = rs.randint(0, height, size=stars)
    bright = rs.uniform(0.5, 1.0, size=(stars, 1)).astype(np.float32) * rs.uniform(0.6, 1.0, size=(stars, 3)).astype(np.float32)
    img[sy, sx, :3] = bright
    img[..., 3] = 1.0
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def pack_background(rgba):
    """load_mipped_image (graphics_settings.cpp:152-212) -> (uint8 array [levels][h][w][4], levels)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    levels = lib.gr_pack_mipped_background(None, w, h, None)
    out = np.empty((levels, h, w, 4), dtype=np.uint8)
    rc = lib.gr_pack_mipped_background(rgba.ctypes.data_as(c_void_p), w, h, out.ctypes.data_as(c_void_p))
    if rc != levels:
        raise GeodesicError("gr_pack_mipped_background failed")
    return out, levels


def build_background(program, rgba, device=0, stream=None):
    """pack_background on the device (gr_build_mipped_background): uploads the RGBA8 image [h, w, 4] into slice 0 of a new packed buffer
    and builds the other slices in place, on `stream` -> (DeviceBuffer of levels * h * w * 4 bytes, levels), the bytes pack_background
    makes.  The float pyramid the build needs is freed once the stream has been synchronised, which this function does."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError(f"build_background: an image of shape {rgba.shape} is not [H, W, 4]")
    h, w = rgba.shape[:2]
    levels = lib.gr_pack_mipped_background(None, w, h, None)
    if levels <= 0:
        raise GeodesicError("gr_pack_mipped_background failed")
    need = ctypes.c_size_t()
    check(lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)))
    packed = DeviceBuffer(device, levels * rgba.nbytes)
    scratch = DeviceBuffer(device, need.value) if need.value else None
    check(lib.gr_device_upload(device, packed.ptr, rgba.ctypes.data_as(c_void_p), rgba.nbytes))
    rc = lib.gr_build_mipped_background(program.handle, stream, packed.ptr, w, h, packed.ptr, scratch.ptr if scratch else None, need.value)
    if rc != levels:
        check(rc)
        raise GeodesicError(f"gr_build_mipped_background made {rc} levels, gr_pack_mipped_background makes {levels}")
    check(lib.gr_stream_synchronize(stream))   # (the scratch is freed on return)
    return packed, levels
