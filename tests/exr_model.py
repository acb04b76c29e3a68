"""What the EXR tests share (tests/test_exr_stream.py, tests/test_gpu_exr.py): an independent reader of the one OpenEXR file the project
writes (include/geodesic_hip_internal.h, "EXR frames") made of struct, zlib and numpy alone - no EXR library is at hand -, numpy's own
float32 -> float16 conversion as the model of the rounding, and the frames the encoders are tried on."""
import struct
import zlib

import numpy as np

MAGIC_AND_VERSION = bytes([0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0])
HEADER_BYTES = 313


def _channel(name):
    return name + b"\0" + struct.pack("<iBBBBii", 1, 0, 0, 0, 0, 1, 1)      # HALF, pLinear 0, three reserved bytes, sampling 1 x 1


def expected_attributes(width, height):
    """[(name, type, value bytes)] in the order the file has them"""
    window = struct.pack("<iiii", 0, 0, width - 1, height - 1)
    return [(b"channels", b"chlist", _channel(b"B") + _channel(b"G") + _channel(b"R") + b"\0"),
            (b"compression", b"compression", bytes([2])),
            (b"dataWindow", b"box2i", window),
            (b"displayWindow", b"box2i", window),
            (b"lineOrder", b"lineOrder", bytes([0])),
            (b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)),
            (b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0)),
            (b"screenWindowWidth", b"float", struct.pack("<f", 1.0))]


def read_exr(data, width, height):
    """(halfs uint16 [height, 3, width] - the planes B, G, R -, kinds: "raw" or "zip" a row, ends: the file offset behind every chunk).
    Every header attribute and the offset table are checked on the way; zlib.decompress checks a compressed row's Adler-32."""
    assert data[:8] == MAGIC_AND_VERSION
    at, found = 8, []
    while data[at] != 0:
        name_end = data.index(b"\0", at)
        type_end = data.index(b"\0", name_end + 1)
        (size,) = struct.unpack("<i", data[type_end + 1:type_end + 5])
        found.append((data[at:name_end], data[name_end + 1:type_end], data[type_end + 5:type_end + 5 + size]))
        at = type_end + 5 + size
    at += 1
    assert found == expected_attributes(width, height)
    assert at == HEADER_BYTES
    offsets = struct.unpack(f"<{height}Q", data[at:at + 8 * height])
    at += 8 * height
    n = 6 * width
    halfs, kinds, ends = np.zeros((height, 3, width), np.uint16), [], []
    for row in range(height):
        assert offsets[row] == at, row
        y, size = struct.unpack("<ii", data[at:at + 8])
        assert y == row and 0 < size <= n, (row, y, size)
        chunk = data[at + 8:at + 8 + size]
        assert len(chunk) == size
        if size == n:
            raw = np.frombuffer(chunk, np.uint8)
            kinds.append("raw")
        else:
            assert chunk[:2] == b"\x78\x01" and chunk[2] & 7 == 5        # BFINAL = 1, BTYPE = 2: the stream's one block
            decoder = zlib.decompressobj()
            predicted = np.frombuffer(decoder.decompress(chunk), np.uint8)
            assert decoder.eof and decoder.unused_data == b"" and len(predicted) == n
            reordered = ((np.cumsum(predicted.astype(np.int64)) - 128 * np.arange(n)) & 255).astype(np.uint8)    # t[i] = t[i - 1] + d[i] - 128
            raw = np.empty(n, np.uint8)
            raw[0::2], raw[1::2] = reordered[:n // 2], reordered[n // 2:]
            kinds.append("zip")
        halfs[row] = raw.view("<u2").reshape(3, width)
        at += 8 + size
        ends.append(at)
    assert at == len(data)
    return halfs, kinds, ends


def expected_halfs(frame):
    """uint16 [height, 3, width]: numpy's halfs of the frame's b, g, r - NaN to 0, clamped to the largest half, round to nearest even"""
    frame = np.asarray(frame, np.float32)
    with np.errstate(all="ignore"):
        halfs = np.clip(np.nan_to_num(frame[..., [2, 1, 0]], nan=0), -65504, 65504).astype(np.float16)
    return np.ascontiguousarray(halfs.view(np.uint16).transpose(0, 2, 1))


def specials():
    values = [np.nan, np.inf, 0.0, 65504.0, 65519.9, 65520.0, 1e30, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 1 + 2.0 ** -11,
              1 + 3 * 2.0 ** -11]
    values = np.array(values, np.float32)
    assert values[-3] > np.float32(2.0 ** -25) and values[-2] != 1 and values[-1] != values[-2]      # (float32 holds them all)
    return np.concatenate([values, -values])


def noise_rows(rng, rows, width):
    """uniform random half bit patterns as floats (infinities and NaNs among them)"""
    return rng.integers(0, 1 << 16, (rows, width, 4), dtype=np.uint16).view(np.float16).astype(np.float32)


def smooth_rows(rows, width):
    x = np.arange(width, dtype=np.float32)[None, :, None] / np.float32(max(width, 2))
    y = np.arange(rows, dtype=np.float32)[:, None, None]
    return (np.float32(0.25) + x * np.array([1.0, 0.5, 2.0, 0.0], np.float32) + y * np.float32(0.01)).astype(np.float32)


def contents(width, height):
    """{name: float32 [height, width, 4]}: zeros, a smooth gradient, random half bit patterns, rows of specials"""
    rng = np.random.default_rng(11 * width + height)
    return {"zero": np.zeros((height, width, 4), np.float32), "smooth": smooth_rows(height, width), "noise": noise_rows(rng, height, width),
            "specials": np.resize(specials(), (height, width, 4)).astype(np.float32)}


def rows_of(kinds, width, seed=5):
    """a frame whose row r is noise ("n") or smooth ("s") as kinds[r] says"""
    rng = np.random.default_rng(seed)
    return np.concatenate([noise_rows(rng, 1, width) if k == "n" else smooth_rows(1, width) + np.float32(0.125 * r) for r, k in enumerate(kinds)])


def mixed(width=257):
    """five rows - noise, smooth, smooth, noise, smooth: rows stored raw beside rows that compress"""
    return rows_of("nssns", width)
