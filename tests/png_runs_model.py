"""What the tests of the PNG runs stream share (tests/test_png_runs_stream.py, tests/test_gpu_png_runs.py; the stream:
include/geodesic_hip_internal.h, "PNG frames", GR_PNG_STREAM_RUNS): frames made from their filtered words, an independent writer of the
stream in numpy - the tokeniser by the stated rule, RFC 1951's length table written out, a bit writer and a container of its own; only the
Huffman table comes from the library (gr_png_build_table_as) -, a decoder made of zlib and a chunk parser, and a reader of a block header's
code lengths."""
import ctypes
import struct
import zlib

import numpy as np

import geodesic_raytracing_amd as gra

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LITERALS, RUNS = 0, 1
GROUP = 64
# RFC 1951 3.2.5: the length symbols 257 ... 285, the first length of each and its extra bits
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA_BITS = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(length):
    """(symbol, extra bits, extra) of a match length 3 ... 257"""
    assert 3 <= length <= 257
    i = max(k for k in range(28) if LENGTH_BASE[k] <= length)
    return 257 + i, LENGTH_EXTRA_BITS[i], length - LENGTH_BASE[i]


# ---------------------------------------------------------------------------------------------------------------- frames

def filtered_words(pixels):
    """q [H, W] uint32: the four filtered bytes of every pixel as one word (R in the low byte) - Sub with bpp 4 on row 0, Up on the others"""
    p = pixels.astype(np.int32)
    f = np.empty_like(p)
    f[0, 0] = p[0, 0]
    f[0, 1:] = p[0, 1:] - p[0, :-1]
    f[1:] = p[1:] - p[:-1]
    return np.ascontiguousarray((f & 255).astype(np.uint8)).view("<u4")[..., 0]


def pixels_of(q):
    """the frame [H, W, 4] uint8 whose filtered words are q [H, W]"""
    f = np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(q.shape[0], q.shape[1], 4).astype(np.uint32)
    f[0] = f[0].cumsum(axis=0)
    return (f.cumsum(axis=0) & 255).astype(np.uint8)


def distinct_words(rng, height, width):
    """words of which no two neighbours in a row are equal: a row without a repeat"""
    q = rng.integers(0, 2 ** 32, (height, width), dtype=np.uint64).astype(np.uint32)
    same = np.zeros_like(q, dtype=bool)
    same[:, 1:] = q[:, 1:] == q[:, :-1]
    q[same] ^= np.uint32(0x5a5a5a5a)
    assert not (q[:, 1:] == q[:, :-1]).any()
    return q


def with_repeats(q, repeat):
    """q with q[y, x] = q[y, x - 1] wherever repeat[y, x] (column 0 never), from the left"""
    q = q.copy()
    for x in range(1, q.shape[1]):
        q[:, x] = np.where(repeat[:, x], q[:, x - 1], q[:, x])
    return q


def contents(width, height):
    """{name: pixels}: frames of this size that exercise the tokeniser - see the tests' docstrings"""
    rng = np.random.default_rng(1000 * width + height)
    xs = np.arange(width)[None, :].repeat(height, axis=0)
    base = distinct_words(rng, height, width)
    gradient = np.zeros((height, width, 4), np.uint8)
    gradient[..., 0] = np.arange(width)[None, :] & 255
    gradient[..., 1] = (np.arange(width)[None, :] * 3) & 255
    gradient[..., 2] = (np.arange(height)[:, None] * 5) & 255
    gradient[..., 3] = 255
    geometric = rng.random((height, width)) < 0.8          # runs of every length, starting anywhere
    return {
        "noise": pixels_of(base),                                                       # no repeat at all
        "zero": np.zeros((height, width, 4), np.uint8),                                 # every pixel but 0 repeats: runs of 63, 64, 64 ...
        "colour": np.full((height, width, 4), (10, 200, 30, 255), np.uint8),            # row 0: pixel 1 does not repeat pixel 0
        "gradient": gradient,                                                           # Sub leaves one delta pixel after pixel
        "random_runs": pixels_of(with_repeats(base, geometric)),
        "ends_on_boundary": pixels_of(with_repeats(base, (xs % GROUP) >= 60)),           # a run that ends with its group
        "straddles_boundary": pixels_of(with_repeats(base, ((xs + 4) % GROUP) < 8)),     # repeats 60 ... 67: two matches
        "at_boundary_only": pixels_of(with_repeats(base, (xs % GROUP) == 0)),            # only pixel 64 g repeats (the group before's last)
    }


def one_literal_one_length():
    """64 x 1 pixels whose filtered words are all 01 01 01 01: the filter byte 1, pixel 0's four literals 1, one match of 63 pixels - the
    frame's only symbols are literal 1, length symbol 284 and end-of-block"""
    return pixels_of(np.full((1, 64), 0x01010101, np.uint32))


def every_run_at_every_phase():
    """64 rows; row p holds, for L = 1 ... 64, L repeats from a pixel at phase p of its group on (x % 64 = p, x >= 64), the pixel in front
    of them and the pixel behind them not repeating: every run length at every starting phase (a run that passes the end of its group
    is two matches)"""
    width = 64 + 64 * 64 + 64 + 64
    rng = np.random.default_rng(5)
    repeat = np.zeros((64, width), dtype=bool)
    for p in range(64):
        x = 64 + p
        for L in range(1, 65):
            repeat[p, x:x + L] = True
            x += 64 if L < 64 else 128
        assert x <= width
    return pixels_of(with_repeats(distinct_words(rng, 64, width), repeat))


# ---------------------------------------------------------------------------------------------------------------- the stream, written here

def tokens_of_row(q_row):
    """run [W]: 0 - four literals; r >= 1 - the head of a match of r pixels; -1 - inside a match.  By the rule: repeat[x] = x >= 1 and
    q[x] == q[x - 1]; in every group of 64 pixels by position every maximal run of repeats is one match"""
    width = len(q_row)
    repeat = np.zeros(width, dtype=bool)
    repeat[1:] = q_row[1:] == q_row[:-1]
    run = np.zeros(width, np.int64)
    for g in range(0, width, GROUP):
        x = g
        end = min(g + GROUP, width)
        while x < end:
            if not repeat[x]:
                x += 1
                continue
            r = 1
            while x + r < end and repeat[x + r]:
                r += 1
            run[x] = r
            run[x + 1:x + r] = -1
            x += r
    return run


def build_table(histogram, kind=RUNS):
    symbols = 285 if kind == RUNS else 257
    histogram = np.ascontiguousarray(histogram, dtype=np.uint64)
    assert histogram.shape == (symbols,)
    lengths, codes, header, bits = np.zeros(symbols, np.uint8), np.zeros(symbols, np.uint16), np.zeros(128, np.uint32), ctypes.c_int()
    gra.check(gra.lib.gr_png_build_table_as(histogram.ctypes.data, kind, lengths.ctypes.data, codes.ctypes.data, header.ctypes.data, ctypes.byref(bits)))
    return lengths, codes, header, bits.value


def packed(values, counts):
    """the bytes of items (value, count <= 32 bits) written one behind the other from bit 0 of byte 0 up; the last byte is padded with 0"""
    values, counts = np.asarray(values, np.uint64), np.asarray(counts, np.int64)
    at = np.concatenate([[0], counts.cumsum()])
    bits = np.zeros((int(at[-1]) + 7) // 8 * 8, np.uint8)
    for b in range(int(counts.max())):
        has = counts > b
        bits[at[:-1][has] + b] = (values[has] >> np.uint64(b)) & np.uint64(1)
    return np.packbits(bits, bitorder="little").tobytes()


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_runs(pixels):
    """the file of the runs stream, written here"""
    height, width = pixels.shape[:2]
    q = filtered_words(pixels)
    filter_of = [1] + [2] * (height - 1)
    runs = [tokens_of_row(q[r]) for r in range(height)]
    q_bytes = np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(height, width, 4)
    histogram = np.zeros(285, np.uint64)
    for r in range(height):
        histogram[filter_of[r]] += 1
        histogram[:256] += np.bincount(q_bytes[r][runs[r] == 0].ravel(), minlength=256).astype(np.uint64)
        for length in runs[r][runs[r] > 0]:
            histogram[length_symbol(4 * int(length))[0]] += 1
    histogram[256] = height
    lengths, codes, header, header_bits = build_table(histogram)
    stream = b"\x78\x01"
    for r in range(height):
        values = [int(header[w]) for w in range((header_bits + 31) // 32)] + [int(codes[filter_of[r]])]
        counts = [min(32, header_bits - 32 * w) for w in range((header_bits + 31) // 32)] + [int(lengths[filter_of[r]])]
        slots_v, slots_c = np.zeros((width, 4), np.uint64), np.zeros((width, 4), np.int64)
        literal = runs[r] == 0
        slots_v[literal] = codes[q_bytes[r][literal]]
        slots_c[literal] = lengths[q_bytes[r][literal]]
        for x in np.flatnonzero(runs[r] > 0):
            symbol, extra_bits, extra = length_symbol(4 * int(runs[r][x]))
            slots_v[x, :3] = (codes[symbol], extra, 0)                  # ... and the one bit of distance code 3: 0
            slots_c[x, :3] = (lengths[symbol], extra_bits, 1)
        values = np.concatenate([values, slots_v.ravel(), [int(codes[256]), 0]])
        counts = np.concatenate([counts, slots_c.ravel(), [int(lengths[256]), 3]])     # end-of-block; BFINAL = 0, BTYPE = 0
        stream += packed(values, counts) + b"\x00\x00\xff\xff"
    raw = b"".join(bytes([filter_of[r]]) + q_bytes[r].tobytes() for r in range(height))
    stream += b"\x03\x00" + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 6, 0, 0, 0)) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")


# ---------------------------------------------------------------------------------------------------------------- reading a file back

def zlib_stream_of(png):
    """(width, height, the IDAT chunks' data joined) with every chunk's CRC checked"""
    assert png[:8] == SIGNATURE
    at, stream, size = 8, b"", None
    while at < len(png):
        (n,) = struct.unpack(">I", png[at:at + 4])
        tag, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF, tag
        if tag == b"IHDR":
            size = struct.unpack(">II", data[:8])
            assert data[8:] == bytes([8, 6, 0, 0, 0])
        if tag == b"IDAT":
            stream += data
        at += 12 + n
    assert at == len(png)
    return size[0], size[1], stream


def decoded(png):
    """the pixels of a file, with zlib (which checks the Adler-32) and the filters undone here"""
    width, height, stream = zlib_stream_of(png)
    rows = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(height, 4 * width + 1)
    assert rows[0, 0] == 1 and (rows[1:, 0] == 2).all()
    first = rows[0, 1:].reshape(width, 4).astype(np.uint32).cumsum(axis=0)
    body = np.concatenate([first.reshape(1, -1), rows[1:, 1:].astype(np.uint32)]).cumsum(axis=0)
    return (body & 255).astype(np.uint8).reshape(height, width, 4)


def first_block_header(png):
    """(HLIT, HDIST, the code lengths sent) of the first deflate block of a file, read bit by bit"""
    data = zlib_stream_of(png)[2][2:]
    value = int.from_bytes(data[:1024], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (value >> at) & ((1 << n) - 1)
        at += n
        return v

    assert take(1) == 0 and take(2) == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    of_code = [0] * 19
    for i in range(hclen):
        of_code[ORDER[i]] = take(3)
    decode, code = {}, 0                       # (length, code read most significant bit first) -> symbol
    for n in range(1, 8):
        for s in range(19):
            if of_code[s] == n:
                decode[(n, code)] = s
                code += 1
        code <<= 1
    sent = []
    while len(sent) < hlit + hdist:
        n, code = 0, 0
        while (n, code) not in decode:
            code = (code << 1) | take(1)
            n += 1
            assert n <= 7
        s = decode[(n, code)]
        if s < 16:
            sent.append(s)
        elif s == 16:
            sent += [sent[-1]] * (3 + take(2))
        else:
            sent += [0] * ((3 + take(3)) if s == 17 else (11 + take(7)))
    assert len(sent) == hlit + hdist
    return hlit, hdist, sent
