"""CPU tests of the Motion-JPEG writer (gr_avi_open / _write_frame / _close in csrc/imageio.cpp; include/geodesic_hip_internal.h, "JPEG
frames"): three JPEG frames of different lengths, one of them odd, at 30000/1001 - the RIFF tree parsed here, list sizes, the counts, rate
and scale of 'avih' and 'strh', 'strf', every index entry against its chunk, the frames back byte for byte and through PIL - and the refusal of
a frame that would take the file past its limit, checked by arithmetic on a small limit set through gr_avi_set_size_limit."""
import ctypes
import io
import struct

import numpy as np
import pytest
from PIL import Image

import geodesic_raytracing_amd as gra


def frames_of_three_lengths():
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:16, 0:24]
    gradient = np.stack([x * 9, y * 13, x + y, x * 0 + 255], axis=-1).astype(np.uint8)
    made = [gra.jpeg_encode_host(np.full((16, 24, 4), 90, np.uint8), 90), gra.jpeg_encode_host(gradient, 90)]
    for seed in range(8):   # a third frame whose length differs in parity from the second's, so that one of the three is odd
        noise = gra.jpeg_encode_host(rng.integers(0, 256, (16, 24, 4), dtype=np.uint8), 90)
        if len(noise) % 2 != len(made[1]) % 2:
            return made + [noise]
    raise AssertionError("no frame of the other parity")


def tree(data, at, end):
    """[(tag, list type or None, offset of the chunk's header, data or children)] of the chunks in data[at:end]"""
    found = []
    while at < end:
        tag, (size,) = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])
        assert at + 8 + size <= end, tag
        if tag in (b"RIFF", b"LIST"):
            found.append((tag, data[at + 8:at + 12], at, tree(data, at + 12, at + 8 + size)))
        else:
            found.append((tag, None, at, data[at + 8:at + 8 + size]))
        at += 8 + size + (size & 1)   # chunks are padded to even length
    assert at == end
    return found


def test_the_riff_tree_the_index_and_the_frames(tmp_path):
    frames = frames_of_three_lengths()
    assert len({len(f) for f in frames}) == 3 and any(len(f) % 2 for f in frames)
    path = tmp_path / "three.avi"
    with gra.AviWriter(str(path), 24, 16, fps=(30000, 1001)) as avi:
        for frame in frames:
            avi.write(frame)
    data = path.read_bytes()
    ((riff, form, _, top),) = tree(data, 0, len(data))
    assert riff == b"RIFF" and form == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    assert [(tag, kind) for tag, kind, _, _ in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = top
    (avih, _, _, main), (_, strl_kind, _, strl) = hdrl[3]
    assert avih == b"avih" and len(main) == 56 and strl_kind == b"strl"
    usec, _, _, flags, total, _, streams, buffer_size, width, height = struct.unpack("<10I", main[:40])
    assert (usec, flags & 0x10, total, streams, width, height) == (33367, 0x10, 3, 1, 24, 16) and buffer_size >= max(len(f) for f in frames)
    (strh, _, _, stream), (strf, _, _, fmt) = strl
    assert strh == b"strh" and len(stream) == 56 and stream[:8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack("<4I", stream[20:36])
    assert (scale, rate, start, length) == (1001, 30000, 0, 3)
    assert struct.unpack("<4H", stream[48:56]) == (0, 0, 24, 16)
    assert strf == b"strf" and len(fmt) == 40
    size, w, h, planes, bits, compression, image_bytes = struct.unpack("<IiiHH4sI", fmt[:24])
    assert (size, w, h, planes, bits, compression, image_bytes) == (40, 24, 16, 1, 24, b"MJPG", 24 * 16 * 3)
    chunks = movi[3]
    assert [tag for tag, _, _, _ in chunks] == [b"00dc"] * 3 and [bytes(d) for _, _, _, d in chunks] == frames
    for frame in frames:
        image = Image.open(io.BytesIO(frame))
        image.load()
        assert image.size == (24, 16)
    movi_tag = movi[2] + 8
    assert data[movi_tag:movi_tag + 4] == b"movi"
    entries = [struct.unpack("<4sIII", idx1[3][16 * i:16 * i + 16]) for i in range(3)]
    assert len(idx1[3]) == 48
    for (tag, flags, offset, size), (_, _, at, chunk), frame in zip(entries, chunks, frames):
        assert tag == b"00dc" and flags == 0x10 and movi_tag + offset == at and size == len(frame) == len(chunk)
        assert data[at + 8:at + 8 + size] == frame and at % 2 == 0


def test_a_frame_past_the_limit_is_refused_and_the_file_closes_valid(tmp_path):
    frames = frames_of_three_lengths()
    lib, handle, path = gra.lib, ctypes.c_void_p(), tmp_path / "limited.avi"
    gra.check(lib.gr_avi_open(str(path).encode(), 24, 16, 24, 1, ctypes.byref(handle)))
    assert lib.gr_avi_set_size_limit(handle, 2 ** 31) == -1   # the limit can only be lowered
    padded = lambda f: 8 + len(f) + len(f) % 2
    # 224 bytes of headers, the chunks, an index of 8 + 16 a frame: with the third frame the file would be exactly one byte past this limit
    limit = 224 + sum(padded(f) for f in frames) + 8 + 16 * 3 - 1
    gra.check(lib.gr_avi_set_size_limit(handle, limit))
    gra.check(lib.gr_avi_write_frame(handle, frames[0], len(frames[0])))
    gra.check(lib.gr_avi_write_frame(handle, frames[1], len(frames[1])))
    assert lib.gr_avi_write_frame(handle, frames[2], len(frames[2])) == -1
    message = lib.gr_last_error().decode()
    assert message.startswith("gr_avi_write_frame: ") and f"to {limit + 1} bytes" in message and f"past the {limit}" in message
    gra.check(lib.gr_avi_set_size_limit(handle, limit + 1))   # one byte more and it fits; the default is 2^31 - 1, by the same arithmetic
    gra.check(lib.gr_avi_write_frame(handle, frames[2], len(frames[2])))
    gra.check(lib.gr_avi_set_size_limit(handle, limit + 1))
    assert lib.gr_avi_write_frame(handle, frames[0], len(frames[0])) == -1
    gra.check(lib.gr_avi_close(handle))
    data = path.read_bytes()
    assert len(data) == limit + 1 and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and struct.unpack("<I", data[48:52])[0] == 3
    ((_, _, _, top),) = tree(data, 0, len(data))
    assert [bytes(d) for _, _, _, d in top[1][3]] == frames


def test_refusals():
    lib, handle = gra.lib, ctypes.c_void_p()
    for args, what in (((None, 16, 16, 24, 1, ctypes.byref(handle)), "null"), ((b"/tmp/x.avi", 16, 16, 24, 1, None), "null"),
                       ((b"/tmp/x.avi", 0, 16, 24, 1, ctypes.byref(handle)), "size"), ((b"/tmp/x.avi", 16, 65536, 24, 1, ctypes.byref(handle)), "size"),
                       ((b"/tmp/x.avi", 16, 16, 0, 1, ctypes.byref(handle)), "frame rate"),
                       ((b"/no_such_directory/x.avi", 16, 16, 24, 1, ctypes.byref(handle)), "no_such_directory")):
        assert lib.gr_avi_open(*args) == -1 and not handle.value
        message = lib.gr_last_error().decode()
        assert message.startswith("gr_avi_open: ") and what in message, message
    assert lib.gr_avi_write_frame(None, b"x", 1) == -1 and lib.gr_avi_close(None) == -1
    with pytest.raises(gra.GeodesicError):
        gra.AviWriter("/no_such_directory/x.avi", 16, 16)
