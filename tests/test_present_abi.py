"""CPU tests of the 8-bit sRGB interface (gr_render_frame_rgba8, gr_present_rgba8, gr_srgb8_thresholds, the pinned-memory helpers): what the
headers declare and the library exports, the threshold table that defines the device encode against the host encode it was made from,
the argument checks that come before any device call, the host statement, which code object the kernel is built into, the CLI switch."""
import ctypes
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import encode_srgb8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["gr_render_frame_rgba8"]
INTERNAL = ["gr_present_rgba8", "gr_srgb8_thresholds", "gr_host_alloc", "gr_host_free", "gr_device_download_async"]
ONE = 0x3f800000
_shared = {}


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def host_bytes(values):
    """gr_frame_to_rgba8 of a flat float32 array (a multiple of four values), as one 'frame' of a single row"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    assert values.size % 4 == 0
    return encode_srgb8(values.reshape(1, -1, 4)).reshape(-1)


def table():
    if "table" not in _shared:
        out = (ctypes.c_float * 256)()
        assert gra.lib.gr_srgb8_thresholds(out) == 0
        _shared["table"] = np.array(out[:], dtype=np.float32)
    return _shared["table"]


def lookup(values):
    """the device encode as the table defines it: the largest k with T[k] <= c, c the value clamped to [0, 1]"""
    c = np.clip(np.asarray(values, dtype=np.float32), np.float32(0), np.float32(1))
    return (np.searchsorted(table(), c, side="right") - 1).astype(np.uint8)


def test_the_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in PUBLIC:
        assert name in contract and name not in internal, name
    for name in INTERNAL:
        assert name in internal and name not in contract, name
    for name in PUBLIC + INTERNAL:
        assert hasattr(gra.lib, name), name
        assert name in gra.EXPORTED_SYMBOLS, name
    assert gra.lib.gr_srgb8_thresholds(None) == -1


def test_the_table_is_the_host_encode_inverted():
    t = table()
    assert t.dtype == np.float32 and t.shape == (256,) and t[0] == 0 and not np.signbit(t[0])
    finite = np.isfinite(t)
    count = int(finite.sum())
    assert count >= 255 and finite[:count].all() and np.isposinf(t[count:]).all()     # an infinite entry is followed by infinite ones only
    assert (np.diff(t[:count]) > 0).all() and t[count - 1] <= 1.0
    assert count - 1 == host_bytes([1.0, 1.0, 1.0, 1.0])[0]                           # the last reachable byte is that of 1.0
    # every finite T[k] is the smallest float whose byte is >= k
    ks = np.arange(1, count)
    below = (t[ks].view(np.uint32) - 1).view(np.float32)
    pad = (-len(ks)) % 4
    at = host_bytes(np.concatenate([t[ks], np.ones(pad, np.float32)]))[:len(ks)]
    under = host_bytes(np.concatenate([below, np.zeros(pad, np.float32)]))[:len(ks)]
    assert (at >= ks).all() and (under < ks).all()


def test_the_lookup_equals_the_host_encode_and_the_host_encode_is_monotone():
    """every 64th float of [0, 1] and 1.0 itself (16.8 M values of the library's own powf): no inversion, and the table look-up gives the
    same byte; every float within 4 ulps of a threshold; what lies outside [0, 1]"""
    bits = np.arange(0, ONE + 1, 64, dtype=np.uint32)
    assert bits[-1] == ONE and len(bits) % 4 == 1
    values = np.concatenate([bits, np.full(3, ONE, dtype=np.uint32)]).view(np.float32)
    host = host_bytes(values)
    assert (np.diff(host.astype(np.int16)) >= 0).all()
    assert host[0] == 0 and (lookup(values) == host).all()
    t = table()
    finite = t[np.isfinite(t)][1:]
    near = (finite.view(np.uint32)[:, None].astype(np.int64) + np.arange(-4, 5)[None, :]).reshape(-1)
    near = near[(near >= 0) & (near <= ONE)].astype(np.uint32)
    near = np.concatenate([near, np.zeros((-len(near)) % 4, dtype=np.uint32)]).view(np.float32)
    assert (lookup(near) == host_bytes(near)).all()
    tiny = np.finfo(np.float32).tiny
    odd = np.array([-0.0, -1e-30, -1.0, -np.inf, 1e-45, tiny / 2, tiny, 1.0000001, 1.5, 2.0, 1e30, np.inf], dtype=np.float32)
    assert (lookup(odd) == host_bytes(odd)).all()
    assert (host_bytes(odd)[:7] == 0).all() and (host_bytes(odd)[7:] == host_bytes([1.0] * 4)[0]).all()


def test_the_launcher_checks_its_arguments_before_it_launches():
    """(this box has no GPU, and the answer is not GR_ERROR_DEVICE: the checks precede every HIP call)"""
    src = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    for args in ((None, src, 8, 8, 2, 8, 0, 1, 0), (src, None, 8, 8, 2, 8, 0, 1, 0), (src, src, 8, 8, 0, 8, 0, 1, 0), (src, src, 8, 8, 5, 8, 0, 1, 0),
                 (src, src, 0, 8, 2, 8, 0, 1, 0), (src, src, 8, -1, 2, 8, 0, 1, 0), (src, src, 30000, 20000, 2, 8, 0, 1, 0),
                 (src, src, 8, 8, 2, 0, 0, 2, 0), (src, src, 8, 8, 2, 8, 2, 2, 0), (src, src, 8, 8, 2, 8, -1, 2, 0)):
        assert gra.lib.gr_present_rgba8(None, None, *args) == -1, args
        assert b"gr_present_rgba8" in gra.lib.gr_last_error()
    cam, feats, opts = gra.default_camera(), gra.default_features(), gra.frame_options()
    for state, out in ((None, src), (src, None), (None, None)):
        assert gra.lib.gr_render_frame_rgba8(state, None, None, None, ctypes.byref(cam), ctypes.byref(feats), None, 0, src, src, 64, 32, 1, out,
                                             ctypes.byref(opts)) == -1, (state, out)
        assert b"gr_render_frame_rgba8" in gra.lib.gr_last_error()
    assert gra.lib.gr_host_alloc(64, None) == -1
    assert gra.lib.gr_device_download_async(None, None, src, 4) == -1 and gra.lib.gr_device_download_async(None, src, None, 4) == -1


def test_encode_srgb8_by_hand():
    edge = np.float32(0.0031308)
    under, over = np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(1))
    frame = np.array([[[0.0, 0.5, under, over], [-1.0, 2.0, 1.0, edge]]], dtype=np.float32)
    out = encode_srgb8(frame)
    assert out.dtype == np.uint8 and out.shape == (1, 2, 4)
    top = int(255 * np.float32(np.float32(1.055) * np.float32(1.0) - np.float32(0.055)))   # 1.055f - 0.055f need not be 1
    # the linear piece: 0.0031308 * 12.92 * 255 = 10.31; the power piece just above it: (1.055 * 0.0031308^(1/2.4) - 0.055) * 255 = 10.31
    assert out[0, 0].tolist() == [0, 187, 10, 10]
    assert out[0, 1].tolist() == [0, top, top, 10] and top in (254, 255)
    with pytest.raises(ValueError):
        encode_srgb8(np.zeros((4, 4, 3), dtype=np.float32))


def test_the_kernel_is_built_into_the_setup_code_object_only(tmp_path, monkeypatch):
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("kerr_boyer").argument_string().encode()))
    files = sorted(tmp_path.glob("*.hsaco"))
    setups = [f for f in files if f.name.endswith(".setup.hsaco")]
    frames = [f for f in files if f not in setups]
    assert len(setups) == 1 and len(frames) == 1
    setup, frame = setups[0].read_bytes(), frames[0].read_bytes()
    for blob in (setup, frame):
        assert blob[:4] == b"\x7fELF" and b"gfx950" in blob
    assert b"gr_present_rgba8" in setup and b"gr_resolve_supersampled" in setup
    assert b"gr_trace_fused" in frame and b"gr_present_rgba8" not in frame


def test_the_cli_encodes_on_the_host_or_on_the_device_only(capsys):
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--encode", "gpu", "--out", "x.png"])
    assert e.value.code == 2 and "--encode" in capsys.readouterr().err
    assert not os.path.exists("x.png")
