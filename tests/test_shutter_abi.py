"""CPU tests of motion-blurred frames (include/geodesic_hip_internal.h, "Motion-blurred frames"): the four names, gr_accumulate_frame against
numpy float32 - whose `*` and `+` are single IEEE operations - bit for bit, a triple on which a fused multiply-add would give another bit,
the refusals that need no device, the kernel's place in the set-up module and its disassembly (a multiply and an add, no fma), the two pure
functions of the CLI (shutter_times, camera_path_at) and the CLI's refusals."""
import ctypes
import glob
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import geodesic_raytracing_amd as gra
from geodesic_raytracing_amd import render
from geodesic_raytracing_amd.pipeline import accumulate_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_accumulate_frame", "gr_shutter_accumulate", "gr_render_subframe", "gr_deliver_accumulated"]
CONTRACT_SHA256 = "8d085403df7f900e515ee2740ba562a30fdaee115bae2c6b4c608a80dad10245"   # include/geodesic_hip.h of the parent commit
INVALID, DEVICE = -1, -4   # GR_ERROR_INVALID_ARGUMENT, GR_ERROR_DEVICE
GUARD = 16


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(gr_[a-z0-9_]+)\s*\(", text))


def last_error_names(name):
    return name.encode() in (gra.lib.gr_last_error() or b"")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """bit patterns equal wherever the value is a number, and a NaN exactly where a NaN is wanted (which NaN an operation returns is the
    one thing IEEE 754 leaves open)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def step(accum, frame, weight, first):
    """the definition in numpy float32: one rounded multiply, one rounded add"""
    product = np.float32(weight) * np.asarray(frame, dtype=np.float32)
    assert product.dtype == np.float32
    return product if first else np.asarray(accum, dtype=np.float32) + product


def library_step(accum, frame, weight, first):
    """gr_accumulate_frame on a copy of accum that sits between guard words"""
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    buf = np.full(frame.size + 2 * GUARD, np.float32(123.5), dtype=np.float32)
    buf[GUARD:GUARD + frame.size] = np.asarray(accum, dtype=np.float32).reshape(-1)
    rc = gra.lib.gr_accumulate_frame(ctypes.c_void_p(buf.ctypes.data + 4 * GUARD), frame.ctypes.data_as(ctypes.c_void_p), frame.size, float(weight), int(first))
    assert rc == 0, gra.lib.gr_last_error()
    assert (buf[:GUARD] == np.float32(123.5)).all() and (buf[GUARD + frame.size:] == np.float32(123.5)).all(), "guard words were written"
    return buf[GUARD:GUARD + frame.size].reshape(frame.shape).copy()


def test_the_names_are_declared_exported_and_bound():
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    for name in NAMES:
        assert name in internal and name not in contract, name
        assert hasattr(gra.lib, name) and name in gra.EXPORTED_SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "geodesic_hip_internal.h")).read()
    assert "Motion-blurred frames" in header and header.index("Motion-blurred frames") < header.index("gr_accumulate_frame")
    assert "does NOT normalise" in header and "NEVER a fused multiply-add" in header
    assert re.search(r"enum \{ GR_FRAME_YUV420 = 2, GR_FRAME_YUV420P10 = 3 \};", header)
    assert (gra.FRAME_F32, gra.FRAME_RGBA8, gra.FRAME_YUV420, gra.FRAME_YUV420P10) == (0, 1, 2, 3)   # nothing renumbered


def test_both_headers_still_match_the_exports():
    """tests/test_abi.py's method: every name either header declares is exported and bound, the two do not overlap, and the contract header
    is the parent commit's file"""
    contract, internal = declared("geodesic_hip.h"), declared("geodesic_hip_internal.h")
    assert 40 <= len(contract) <= 80 and not contract & internal
    for name in contract | internal:
        assert hasattr(gra.lib, name), name
    assert contract | internal == set(gra.EXPORTED_SYMBOLS)
    blob = open(os.path.join(ROOT, "include", "geodesic_hip.h"), "rb").read()
    assert hashlib.sha256(blob).hexdigest() == CONTRACT_SHA256


def test_a_fused_multiply_add_would_differ():
    """a + w * r with w * r inexact: the two roundings of the definition and the one rounding of an fma give different floats (emulated
    in float64, which holds the product of two floats exactly and, for these, their sum with a too) - and the library gives the first"""
    a, w, r = np.float32(-(1.0 + 2.0 ** -11)), np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12)
    exact_product = np.float64(w) * np.float64(r)                 # 1 + 2^-11 + 2^-24: exact in float64, not a float32
    assert exact_product == 1.0 + 2.0 ** -11 + 2.0 ** -24 and np.float64(np.float32(exact_product)) != exact_product
    two_roundings = np.float32(a + np.float32(exact_product))     # the product rounds to 1 + 2^-11 (a tie, to even): the sum is 0
    exact_sum = np.float64(a) + exact_product                     # 2^-24, which an fma would deliver
    assert exact_sum == 2.0 ** -24
    one_rounding = np.float32(exact_sum)
    assert two_roundings == 0 and one_rounding == np.float32(2.0 ** -24) and bits(two_roundings) != bits(one_rounding)
    assert bits(step([a], [r], w, False))[0] == bits(two_roundings)
    got = library_step([a], [r], w, False)
    assert bits(got)[0] == bits(two_roundings) and bits(got)[0] != bits(one_rounding)
    # ... and over many random triples some of which differ under an fma: the library is with numpy on every one
    rs = np.random.RandomState(11)
    acc, frame = rs.uniform(0.5, 2.0, 100000).astype(np.float32), rs.uniform(0.5, 2.0, 100000).astype(np.float32)
    weight = np.float32(0.3)
    fused = (acc.astype(np.float64) + np.float64(weight) * frame.astype(np.float64)).astype(np.float32)
    want = step(acc, frame, weight, False)
    assert (bits(fused) != bits(want)).sum() > 1000
    assert same_bits(library_step(acc, frame, weight, False), want)


def test_accumulate_frame_against_numpy():
    rs = np.random.RandomState(5)
    n = 1000000
    frame = (rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))).astype(np.float32)
    accum = (rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))).astype(np.float32)
    for weight in (np.float32(1) / np.float32(3), np.float32(0.125), np.float32(-0.7), np.float32(1.0), np.float32(0.0)):
        assert same_bits(library_step(accum, frame, weight, True), step(accum, frame, weight, True)), weight
        assert same_bits(library_step(accum, frame, weight, False), step(accum, frame, weight, False)), weight
    picked = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1.0 + 2.0 ** -12, 3.4e38, 1e-38, 1e-45, -1e-45, 0.1], dtype=np.float32)
    frame, accum = [g.reshape(-1) for g in np.meshgrid(picked, picked)]
    with np.errstate(all="ignore"):
        for weight in (np.float32(1.0), np.float32(0.5), np.float32(1.0 + 2.0 ** -12), np.float32(0.0), np.float32(-0.0), np.float32(3.0)):
            assert same_bits(library_step(accum, frame, weight, True), step(accum, frame, weight, True)), weight
            assert same_bits(library_step(accum, frame, weight, False), step(accum, frame, weight, False)), weight
    # with `first` the accumulation is not read: a NaN in it is gone
    assert same_bits(library_step(np.full(4, np.nan, np.float32), np.arange(4, dtype=np.float32), 0.5, True), np.arange(4, dtype=np.float32) * np.float32(0.5))
    # ... and the Python wrapper is the same function, in place
    a = accum.copy()
    assert accumulate_frame(a, frame, 0.5, False) is a
    with np.errstate(all="ignore"):
        assert same_bits(a, step(accum, frame, 0.5, False))
    with pytest.raises(ValueError):
        accumulate_frame(np.zeros(3, np.float32), np.zeros(4, np.float32), 1.0, True)


def test_a_weight_of_one_on_the_first_subframe_is_the_identity():
    rs = np.random.RandomState(6)
    frame = rs.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every kind of float, NaNs included
    frame[:6] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], dtype=np.float32)
    got = library_step(np.zeros_like(frame), frame, 1.0, True)
    number = ~np.isnan(frame)
    assert np.array_equal(bits(got)[number], bits(frame)[number]) and np.isnan(got[~number]).all()
    assert bits(got)[1] == 0x80000000   # -0.0 stays -0.0: it is not 0 + 1 * -0


@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_box_weights_in_sequence(count):
    rs = np.random.RandomState(20 + count)
    frames = rs.uniform(0, 4, size=(count, 9, 7, 4)).astype(np.float32)
    frames[0, 0, 0] = [0.0, -0.0, np.inf, np.nan]
    weight = np.float32(1) / np.float32(count)
    want = got = None
    with np.errstate(all="ignore"):
        for j in range(count):
            want = step(want, frames[j], weight, j == 0)
            got = library_step(got if j else np.zeros_like(frames[0]), frames[j], weight, j == 0)
    assert same_bits(got, want)
    if count == 1:
        number = ~np.isnan(frames[0])
        assert np.array_equal(bits(got)[number], bits(frames[0])[number])


def test_refusals_that_need_no_device():
    src = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before any object is looked at
    ok = np.zeros(4, dtype=np.float32)
    p = ok.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, p, 4, 0.5, 1), (p, None, 4, 0.5, 0), (p, p, 4, float("nan"), 1), (p, p, 4, float("inf"), 0), (p, p, 4, float("-inf"), 1)):
        assert gra.lib.gr_accumulate_frame(*args) == INVALID, args
        assert last_error_names("gr_accumulate_frame")
    assert gra.lib.gr_accumulate_frame(p, p, 0, 0.5, 1) == 0 and (ok == 0).all()
    other = ctypes.c_void_p(8192)
    for program in (None, src):
        for args in ((None, other, 8, 8, 1, 0.5, 1), (src, None, 8, 8, 1, 0.5, 1), (src, src, 8, 8, 1, 0.5, 1), (src, other, 8, 8, 0, 0.5, 1),
                     (src, other, 8, 8, 5, 0.5, 0), (src, other, 0, 8, 1, 0.5, 1), (src, other, 8, -1, 1, 0.5, 1), (src, other, 30000, 20000, 2, 0.5, 1),
                     (src, other, 2, 300000, 1, 0.5, 1), (src, other, 8, 8, 1, float("nan"), 1), (src, other, 8, 8, 2, float("inf"), 0)):
            assert gra.lib.gr_shutter_accumulate(program, None, *args) == INVALID, args
            assert last_error_names("gr_shutter_accumulate")
    assert gra.lib.gr_shutter_accumulate(None, None, src, other, 8, 8, 1, 0.5, 1) == INVALID and b"null program" in gra.lib.gr_last_error()
    cam, feats, opts = gra.default_camera(), gra.default_features(), gra.frame_options()
    strips = gra.frame_options(mode=gra.MODE_FUSED, strip_count=2, strip_rank=0, block_rows=8)

    def subframe(state, program, metric, camera, bg, weight, first, options):
        return gra.lib.gr_render_subframe(state, program, metric, None, camera, ctypes.byref(feats), None, 0, bg, bg, 64, 32, 1, weight, first,
                                          ctypes.byref(options))

    c = ctypes.byref(cam)
    for args in ((None, src, src, c, src, 0.5, 1, opts), (src, None, src, c, src, 0.5, 1, opts), (src, src, None, c, src, 0.5, 1, opts),
                 (src, src, src, None, src, 0.5, 1, opts), (src, src, src, c, None, 0.5, 1, opts),                       # null arguments
                 (src, src, src, c, src, float("nan"), 1, opts), (src, src, src, c, src, float("inf"), 0, opts),          # a weight that is not finite
                 (src, src, src, c, src, 0.5, 1, strips), (src, src, src, c, src, 0.5, 0, strips)):                       # whole frames only
        assert subframe(*args) == INVALID, args
        assert last_error_names("gr_render_subframe")
    for args in ((None, src, None, 0, 0, src), (src, None, None, 0, 0, src), (src, src, None, 0, 0, None), (src, src, None, 4, 0, src),
                 (src, src, None, -1, 0, src), (src, src, None, gra.FRAME_YUV420, 2, src), (src, src, None, gra.FRAME_YUV420P10, -1, src),
                 (src, src, None, gra.FRAME_YUV420, 0, ctypes.c_void_p(4098))):
        assert gra.lib.gr_deliver_accumulated(*args) == INVALID, args
        assert last_error_names("gr_deliver_accumulated")
    # without a device a call that nothing is wrong with fails as every device entry point does (with one, these made-up objects must not
    # be used: tests/test_gpu_shutter.py calls it with real ones)
    n = ctypes.c_int(0)
    if not (gra.lib.gr_device_count(ctypes.byref(n)) == 0 and n.value > 0):
        assert subframe(src, src, src, c, src, 0.5, 1, opts) == DEVICE and gra.lib.gr_last_error()
        with pytest.raises(gra.GeodesicError):
            gra.RenderState(64, 64, 0)


def test_the_kernel_is_part_of_the_setup_module_only():
    here = os.path.join(os.path.dirname(gra.__file__), "csrc")
    capi = open(os.path.join(here, "capi.cpp")).read()
    program_build = open(os.path.join(here, "program_build.cpp")).read()
    lists = {name: re.findall(r'"([a-z_]+\.(?:hip|inc))"', body) for name, body in re.findall(r"const (\w*PARTS)\[\] = \{(.*?)\};", program_build, flags=re.S)}
    frame_files, setup_files = lists["KERNEL_PARTS"], lists["PARTS"]
    assert "shutter.hip" in setup_files and "shutter.hip" not in frame_files
    assert setup_files.index("resolve.hip") < setup_files.index("shutter.hip")   # box_average<F> itself, in the same compilation
    assert re.search(r"is_setup_kernel\(int k\) \{[^}]*K_SHUTTER_ACCUMULATE", capi)
    shutter = open(os.path.join(here, "kernels", "shutter.hip")).read()
    assert "gr_shutter_accumulate(" in shutter and shutter.count("box_average<") >= 4 and "template" not in shutter
    for other in frame_files:
        assert "shutter" not in open(os.path.join(here, "kernels", other)).read(), other


def test_the_compiled_kernel_multiplies_and_adds_and_does_not_fuse(tmp_path, monkeypatch):
    """the set-up module as it is cross-compiled for gfx950 (no GPU needed): gr_shutter_accumulate holds fp32 multiplies and adds - four
    of each for `first` = 0, scalar or packed - and no floating-point multiply-add instruction, fused or not, of any name; the frame path's code object
    does not hold the kernel"""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump in this image")
    monkeypatch.setenv("GR_CACHE_DIR", str(tmp_path))
    gra.Program.precompile(gra.Metric("minkowski").argument_string())
    files = glob.glob(os.path.join(str(tmp_path), "*.hsaco"))
    (setup,) = [f for f in files if f.endswith(".setup.hsaco")]
    for f in files:
        assert (b"gr_shutter_accumulate" in open(f, "rb").read()) == (f == setup), f
    text = subprocess.run([objdump, "-d", "--no-show-raw-insn", setup], capture_output=True, text=True, check=True).stdout
    ops, inside = [], False
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            inside = m.group(1) == "gr_shutter_accumulate"
        elif inside and line.startswith("\t"):
            ops.append(line.strip().split(" ")[0])
    assert len(ops) > 20
    # (v_mad_u64_u32 and its kin are the 64-bit indices' integer arithmetic: floating-point names end in a float type)
    assert not [op for op in ops if "fma" in op or (("mad" in op or "mac" in op) and re.search(r"_f(16|32|64)|legacy", op))], sorted(set(ops))
    multiplies = sum(2 if op.startswith("v_pk_mul_f32") else 1 for op in ops if op.startswith(("v_mul_f32", "v_pk_mul_f32")))
    adds = sum(2 if op.startswith("v_pk_add_f32") else 1 for op in ops if op.startswith(("v_add_f32", "v_pk_add_f32")))
    assert multiplies >= 4 and adds >= 4, sorted(set(ops))
    print("gr_shutter_accumulate:", len(ops), "instructions,", multiplies, "fp32 multiplies,", adds, "fp32 adds, no fma / mad / mac")


def test_shutter_times():
    for frames, shutter, samples in ((1, 0.5, 8), (3, 1.0, 2), (48, 0.5, 8), (5, 0.25, 3), (2, 1.0, 64), (4, 0.5, 1)):
        t = render.shutter_times(frames, shutter, samples)
        assert t.shape == (frames, samples) and t.dtype == np.float64
        flat = t.ravel()
        assert (np.diff(flat) > 0).all()                                  # monotone over the whole sequence
        for k in range(frames):
            assert (t[k] >= k).all() and (t[k] < k + shutter).all()       # inside the frame's own shutter interval
            edges = k + shutter * np.arange(samples + 1) / samples
            assert np.allclose(t[k], (edges[:-1] + edges[1:]) / 2, rtol=0, atol=1e-12)   # midpoints of equal parts
            assert t[k, 0] == k + shutter * 0.5 / samples
    assert np.float32(1) / np.float32(8) == np.float32(0.125)
    for bad in ((0, 0.5, 8), (2, 0.0, 8), (2, 1.5, 8), (2, -0.5, 8), (2, 0.5, 0), (2, float("nan"), 4)):
        with pytest.raises(ValueError):
            render.shutter_times(*bad)


def test_camera_path_at():
    start, end = ([0.0, 0.0, -8.0, 0.0], [0.1, 0.2, 0.3, 0.9]), ([0.0, 3.0, -6.0, 0.5], [-0.4, 0.1, 0.2, 0.7])
    for frames in (1, 2, 7, 48):
        for position_to, quat_to in ((end[0], end[1]), (end[0], None), (None, end[1]), (None, None), (end[0], [0.1, 0.2, 0.3, 0.9000001])):
            whole = render.camera_path(start[0], start[1], position_to, quat_to, frames)
            assert render.camera_path_at(start[0], start[1], position_to, quat_to, frames, range(frames)) == whole   # exactly
            assert render.camera_path_at(start[0], start[1], position_to, quat_to, frames, np.arange(frames, dtype=np.float64)) == whole
    # between and beyond the ends: unit quaternions, positions on the line
    times = render.shutter_times(6, 1.0, 4).ravel()
    poses = render.camera_path_at(start[0], start[1], end[0], end[1], 6, times)
    assert len(poses) == 24 and times.max() > 5
    p0, p1 = np.array(start[0]), np.array(end[0])
    for t, (position, quat) in zip(times, poses):
        assert abs(np.linalg.norm(quat) - 1) < 1e-12
        assert np.allclose(position, p0 + (p1 - p0) * t / 5, rtol=0, atol=1e-12)
    # the arc goes on at the same rate past the end: the turn from pose(5) to pose(5.5) is the turn from pose(4.5) to pose(5)
    q = [np.array(quat) for _, quat in render.camera_path_at(start[0], start[1], end[0], end[1], 6, [4.5, 5.0, 5.5])]
    assert abs(np.arccos(min(1.0, abs(q[0] @ q[1]))) - np.arccos(min(1.0, abs(q[1] @ q[2])))) < 1e-9
    assert render.camera_path_at(None, None, None, None, 1, [0.0, 0.4]) == render.camera_path(None, None, None, None, 1) * 2
    with pytest.raises(ValueError):
        render.camera_path_at([0, 0, 0], None, None, None, 4, [0.5])
    with pytest.raises(ValueError):
        render.camera_path_at(None, [0, 0, 0, 0], None, None, 4, [0.5])


def test_the_cli_refuses_a_shutter_it_cannot_render(capsys, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    moving = ["--camera-to", "0,3,-6,0", "--frames", "4"]
    for argv, names in ((["--shutter", "0.5", "--devices", "0,1"] + moving, "--devices"),
                        (["--shutter", "0.5", "--geodesic-speed", "0,0.3,0", "--devices", "0"], "--devices"),
                        (["--shutter", "0.5", "--adaptive"] + moving, "--adaptive"),
                        (["--shutter", "0.5", "--frames", "4"], "no motion"),
                        (["--shutter", "0.5", "--shutter-samples", "4"], "no motion"),
                        (["--shutter-samples", "4"] + moving, "--shutter-samples without --shutter"),
                        (["--shutter", "0"] + moving, "--shutter"), (["--shutter", "1.5"] + moving, "--shutter"),
                        (["--shutter", "0.5", "--shutter-samples", "1"] + moving, "--shutter-samples"),
                        (["--shutter", "0.5", "--shutter-samples", "65"] + moving, "--shutter-samples")):
        for out in ("x.png", "x.y4m"):
            with pytest.raises(SystemExit) as e:
                render.main(["--metric", "kerr_boyer", "--out", out] + argv)
            err = capsys.readouterr().err
            assert e.value.code == 2 and "--shutter" in err and names in err, (argv, err[-300:])
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError, match="shutter_samples"):
        render.render("kerr_boyer", 8, 8, shutter_samples=4)                                  # nothing moves
    with pytest.raises(ValueError, match="shutter_samples"):
        render.render("kerr_boyer", 8, 8, cameras=[([0, 0, -4, 0], [0, 0, 0, 1])] * 6, shutter_samples=4)   # 6 poses are not whole shutters of 4
    with pytest.raises(ValueError, match="shutter_samples"):
        render.render("kerr_boyer", 8, 8, cameras=[([0, 0, -4, 0], [0, 0, 0, 1])] * 4, shutter_samples=4, adaptive=True)
