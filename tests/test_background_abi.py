"""CPU tests of the device-built sky (gr_build_mipped_background, gr_mipped_background_scratch_bytes): what the header declares and the
library exports, the argument checks that come before any device call, the scratch size, and - the part that also passes without the
feature - a float32 numpy restatement of the mip chain in the form kernels/background.hip computes it (tree reduction of base blocks, odd
edges dropped, no clamps), byte for byte against the host packer that stays the yardstick (gr_pack_mipped_background)."""
import ctypes
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import pack_background

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 1), (2, 2), (3, 2), (37, 19), (19, 70), (64, 33), (1100, 1024)]   # width x height
F = np.float32


def level_count(w, h):
    return min(int(np.floor(np.log2(min(w, h)))) + 1, 10)


def random_image(w, h):
    return np.random.RandomState(1000 * w + h).randint(0, 256, size=(h, w, 4)).astype(np.uint8)


def all_bytes_image():
    """16 x 16, every byte value in every channel (each channel in an order of its own)"""
    k = np.arange(256)
    return np.stack([k, (k * 7 + 3) % 256, 255 - k, (k * 13 + 101) % 256], axis=-1).astype(np.uint8).reshape(16, 16, 4)


def quarter_sum(block):
    """one 2 x 2 reduction of a float32 [2h, 2w, 4] array, summed in the host's order"""
    c00, c01, c10, c11 = block[0::2, 0::2], block[0::2, 1::2], block[1::2, 0::2], block[1::2, 1::2]
    return F(0.25) * (((c00 + c01) + c10) + c11)


def restated(rgba):
    """The chain as the device computes it.  Level l is (w >> l) x (h >> l); its texel (x, y) is the tree reduction of the base block
    [x 2^l, (x + 1) 2^l) x [y 2^l, (y + 1) 2^l): level 0 cut to a multiple of 2^l per axis and halved l times, no clamp anywhere, in
    float32 without re-quantising.  Slice l replicates level l's last column and row, clamps to [0, 1] and truncates v * 255."""
    h, w = rgba.shape[:2]
    levels = level_count(w, h)
    base = rgba.astype(F) / F(255)
    out = np.empty((levels, h, w, 4), dtype=np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    for l in range(levels):
        cw, ch = w >> l, h >> l
        assert cw >= 1 and ch >= 1
        level = base[:ch << l, :cw << l]
        for _ in range(l):
            level = quarter_sum(level)
        assert level.shape == (ch, cw, 4) and level.dtype == F
        full = level[np.minimum(ys, ch - 1)][:, np.minimum(xs, cw - 1)]
        out[l] = (np.clip(full, F(0), F(1)) * F(255)).astype(np.uint8)
    return out, levels


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


@pytest.mark.parametrize("w,h", SIZES)
def test_the_restatement_equals_the_host_packer(w, h):
    rgba = random_image(w, h)
    want, levels = pack_background(rgba)
    got, got_levels = restated(rgba)
    assert got_levels == levels == level_count(w, h)
    assert got.tobytes() == want.tobytes()
    assert want[0].tobytes() == rgba.tobytes()   # slice 0 is the image


def test_the_restatement_equals_the_host_packer_on_every_byte_value():
    rgba = all_bytes_image()
    for c in range(4):
        assert sorted(rgba[..., c].reshape(-1).tolist()) == list(range(256))
    want, levels = pack_background(rgba)
    assert levels == 5 and restated(rgba)[0].tobytes() == want.tobytes() and want[0].tobytes() == rgba.tobytes()
    k = np.arange(256)
    assert (((k.astype(F) / F(255)) * F(255)).astype(np.uint8) == k).all()   # byte -> float -> byte is the identity: slice 0 is a copy


def test_both_functions_are_declared_in_the_public_header_and_exported():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in ("gr_build_mipped_background", "gr_mipped_background_scratch_bytes"):
        assert name in contract and name not in internal, name
        assert hasattr(gra.lib, name), name
        assert name in gra.EXPORTED_SYMBOLS, name
    assert callable(gra.build_background)


def test_the_scratch_size_is_the_float_pyramid():
    need = ctypes.c_size_t(12345)
    for w, h in SIZES + [(16, 16), (4096, 2048), (16384, 8192)]:
        assert gra.lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)) == 0, (w, h)
        assert need.value == 16 * sum((w >> l) * (h >> l) for l in range(1, level_count(w, h))), (w, h)
    assert gra.lib.gr_mipped_background_scratch_bytes(1, 1, ctypes.byref(need)) == 0 and need.value == 0
    for w, h in ((0, 5), (5, 0), (-1, 5), (65536, 65536)):
        assert gra.lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)) == -1, (w, h)
        assert b"gr_mipped_background_scratch_bytes" in gra.lib.gr_last_error()
    assert gra.lib.gr_mipped_background_scratch_bytes(8, 8, None) == -1


def test_the_launcher_checks_its_arguments_before_it_launches():
    """(no GPU here, and the answer is not GR_ERROR_DEVICE: the checks precede every HIP call; the addresses are never dereferenced)"""
    image, packed, scratch = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)
    w, h = 64, 32   # 8 KiB an image, 6 levels, 10 912 bytes of scratch
    need = ctypes.c_size_t()
    assert gra.lib.gr_mipped_background_scratch_bytes(w, h, ctypes.byref(need)) == 0 and need.value == 16 * (512 + 128 + 32 + 8 + 2)
    at = lambda base, offset: ctypes.c_void_p(base.value + offset)   # noqa: E731
    refused = [
        ("null program", (image, w, h, packed, scratch, need.value)),
        ("size", (image, 0, 5, packed, scratch, need.value)),
        ("size", (image, w, -1, packed, scratch, need.value)),
        ("size", (image, 65536, 65536, packed, scratch, need.value)),
        ("NULL", (None, w, h, packed, scratch, need.value)),
        ("NULL", (image, w, h, None, scratch, need.value)),
        ("NULL", (image, w, h, packed, None, need.value)),
        ("needed", (image, w, h, packed, scratch, need.value - 1)),
        ("needed", (image, w, h, packed, scratch, 0)),
        ("aligned", (at(image, 2), w, h, packed, scratch, need.value)),
        ("aligned", (image, w, h, at(packed, 4), scratch, need.value)),
        ("aligned", (image, w, h, packed, at(scratch, 8), need.value)),
        ("overlap", (at(packed, 16), w, h, packed, scratch, need.value)),                  # the image inside the packed buffer, not at its start
        ("overlap", (at(packed, -16), w, h, packed, scratch, need.value)),                # the image's end in slice 0
        ("overlap", (at(packed, 6 * w * h * 4 - 16), w, h, packed, scratch, need.value)),   # the image's start in the last slice
        ("overlap", (image, w, h, packed, at(packed, 6 * w * h * 4 - 16), need.value)),    # scratch on the packed buffer's end
        ("overlap", (image, w, h, packed, at(image, w * h * 4 - 16), need.value)),        # scratch on the image's end
        ("overlap", (packed, w, h, packed, at(packed, 16), need.value)),                 # in place, scratch inside
    ]
    for word, args in refused:
        assert gra.lib.gr_build_mipped_background(None, None, *args) == -1, word
        message = gra.lib.gr_last_error()
        assert b"gr_build_mipped_background" in message and word.encode() in message, (word, message)
    # what is allowed gets as far as the program: in place, buffers that touch without overlapping, a NULL scratch for a one-level image
    for args in ((packed, w, h, packed, scratch, need.value), (at(packed, -w * h * 4), w, h, packed, at(packed, 6 * w * h * 4), need.value),
                 (image, 1, 1, packed, None, 0), (image, 5, 1, packed, None, 0)):
        assert gra.lib.gr_build_mipped_background(None, None, *args) == -1
        assert b"null program" in gra.lib.gr_last_error(), args


def test_build_background_refuses_what_is_not_an_image():
    with pytest.raises(ValueError):
        gra.build_background(None, np.zeros((4, 4, 3), dtype=np.uint8))


def test_the_cli_makes_the_mips_on_the_host_or_on_the_device_only(capsys):
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--mips", "gpu", "--out", "x.png"])
    assert e.value.code == 2 and "--mips" in capsys.readouterr().err
    assert not os.path.exists("x.png")
    with pytest.raises(ValueError):
        render.render("kerr_boyer", 64, 32, mips="gpu")
