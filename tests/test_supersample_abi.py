"""CPU tests of the supersampling interface (gr_render_state_create_supersampled, gr_resolve_supersampled and their two accessors):
what the headers declare and the library exports, the argument checks that come before any device call, the CLI switch, the host
statement of the box filter, and which code object the kernel is built into."""
import ctypes
import os
import re

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import box_resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUBLIC = ["gr_render_state_create_supersampled"]
INTERNAL = ["gr_resolve_supersampled", "gr_render_state_supersample", "gr_render_state_resolve_ms"]


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def test_the_four_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in PUBLIC:
        assert name in contract and name not in internal, name
    for name in INTERNAL:
        assert name in internal and name not in contract, name
    for name in PUBLIC + INTERNAL:
        assert hasattr(gra.lib, name), name
        assert name in gra.EXPORTED_SYMBOLS, name


def test_the_contract_header_keeps_its_limits():
    """the factor is a property of the state: one line more in the contract, no field more in gr_frame_options"""
    public = open(os.path.join(ROOT, "include", "geodesic_hip.h")).read()
    assert len(public.splitlines()) <= 350
    body = public[public.index("typedef struct gr_frame_options {"):public.index("} gr_frame_options;")]
    assert "supersample" not in body
    assert len(re.findall(r"^\s{4}[a-z].*?;", body, flags=re.M)) <= 15
    lines = [line for line in public.splitlines() if "gr_render_state_create_supersampled" in line]
    assert len(lines) == 1 and lines[0].startswith("int gr_render_state_create_supersampled(int device, int width, int height, int factor, gr_render_state** out);")


@pytest.mark.parametrize("factor", [0, -1, 5])
def test_a_factor_out_of_range_is_refused_before_any_device_call(factor):
    """(this box has no GPU, and the answer is not GR_ERROR_DEVICE: the check precedes hipSetDevice)"""
    state = ctypes.c_void_p()
    assert gra.lib.gr_render_state_create_supersampled(0, 64, 32, factor, ctypes.byref(state)) == -1   # GR_ERROR_INVALID_ARGUMENT
    assert b"factor" in gra.lib.gr_last_error() and str(factor).encode() in gra.lib.gr_last_error()
    assert not state.value
    with pytest.raises(gra.GeodesicError, match="factor"):
        gra.RenderState(64, 32, 0, supersample=factor)


def test_a_traced_size_beyond_int_is_refused_before_any_device_call():
    state = ctypes.c_void_p()
    assert gra.lib.gr_render_state_create_supersampled(0, 16384, 16384, 4, ctypes.byref(state)) == -1   # 2^32 traced pixels
    assert b"factor 4" in gra.lib.gr_last_error()
    assert gra.lib.gr_render_state_create_supersampled(0, 30000, 20000, 2, ctypes.byref(state)) == -1   # 2.4e9
    assert b"factor 2" in gra.lib.gr_last_error()


def test_the_launcher_checks_its_arguments_before_it_launches():
    src = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused on the host
    for args in ((None, src, 8, 8, 2, 8, 0, 1, 0), (src, None, 8, 8, 2, 8, 0, 1, 0), (src, src, 8, 8, 0, 8, 0, 1, 0), (src, src, 8, 8, 5, 8, 0, 1, 0),
                 (src, src, 0, 8, 2, 8, 0, 1, 0), (src, src, 8, -1, 2, 8, 0, 1, 0), (src, src, 30000, 20000, 2, 8, 0, 1, 0),
                 (src, src, 8, 8, 2, 0, 0, 2, 0), (src, src, 8, 8, 2, 8, 2, 2, 0), (src, src, 8, 8, 2, 8, -1, 2, 0)):
        assert gra.lib.gr_resolve_supersampled(None, None, *args) == -1, args
    factor = ctypes.c_int(7)
    assert gra.lib.gr_render_state_supersample(None, ctypes.byref(factor), None, None) == -1 and factor.value == 7
    assert gra.lib.gr_render_state_resolve_ms(None, None) == -1


def test_the_cli_takes_factors_one_to_four_only(capsys):
    with pytest.raises(SystemExit) as e:
        render.main(["--metric", "kerr_boyer", "--supersample", "5", "--out", "x.png"])
    assert e.value.code == 2 and "--supersample" in capsys.readouterr().err
    assert not os.path.exists("x.png")


def test_box_resolve_by_hand():
    frame = np.array([[1, 3, 0, 0], [5, 7, 0, 8], [-2, -2, 1e-3, 0], [2, 2, 0, 0]], dtype=np.float32)
    frame = np.stack([frame, 2 * frame, np.zeros_like(frame), np.ones_like(frame)], axis=2)   # [4, 4, 4]
    out = box_resolve(frame, 2)
    assert out.dtype == np.float32 and out.shape == (2, 2, 4)
    expect = np.array([[4, 2], [0, np.float32(1e-3) / 4]], dtype=np.float32)
    assert (out[..., 0] == expect).all() and (out[..., 1] == 2 * expect).all() and (out[..., 2] == 0).all() and (out[..., 3] == 1).all()
    assert (box_resolve(frame, 1) == frame).all()
    whole = np.float32((24 + float(np.float32(1e-3))) / 16)   # (16 + 8 + 0 + 1e-3) / 16 in double, rounded once
    assert (box_resolve(frame, 4)[0, 0] == np.array([whole, 2 * whole, 0, 1], dtype=np.float32)).all()
    with pytest.raises(ValueError):
        box_resolve(frame, 3)


def test_the_kernel_is_built_into_the_setup_code_object_only(tmp_path, monkeypatch):
    """gr_resolve_supersampled is part of the set-up module (IEEE arithmetic, a compilation of its own), and the code object a fused frame
    launches - gr_trace_fused's - neither holds it nor was compiled with it"""
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.check(gra.lib.gr_program_precompile_frame_path(gra.Metric("kerr_boyer").argument_string().encode()))
    files = sorted(tmp_path.glob("*.hsaco"))
    setups = [f for f in files if f.name.endswith(".setup.hsaco")]
    frames = [f for f in files if f not in setups]
    assert len(setups) == 1 and len(frames) == 1
    setup, frame = setups[0].read_bytes(), frames[0].read_bytes()
    for blob in (setup, frame):
        assert blob[:4] == b"\x7fELF" and b"gfx950" in blob
    assert b"gr_trace_fused" in frame and b"gr_render" in frame
    assert b"gr_resolve_supersampled" in setup and b"gr_camera_setup" in setup
    assert b"gr_resolve_supersampled" not in frame and b"gr_trace_fused" not in setup
