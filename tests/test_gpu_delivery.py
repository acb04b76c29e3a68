"""GPU tests (-m gpu) of frame delivery as a whole (csrc/frame.cpp: a frame, then a sink): every sink gives the bytes of the same source.
On one state and with one camera the float frame F is rendered; the same state then delivers RGBA8, I420, NV12, yuv420p10le and P010,
each the host encode of F byte for byte (encode_srgb8, rgba8_to_yuv420, rgb10_to_yuv420p10(frame_to_rgb10(F))); and one sub-frame of
weight 1.0 with first = 1, delivered in all five formats and as float4, gives the same bytes again.  Eight states: 36 x 20 (a width that is
a multiple of 4: the 10-bit kernel's 8-byte stores) or 34 x 19 (its 2-byte stores, an odd chroma edge row), factor 1 or 2, the box or the
Mitchell filter.  Kerr, a = 0.45, the substituted program of tests/test_gpu_shutter.py, built once."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd.pipeline import encode_srgb8, frame_to_rgb10, rgb10_to_yuv420p10, rgba8_to_yuv420  # noqa: E402
from test_gpu_shutter import I420, NV12, every_delivery_is_the_encode_of, plain_frame as frame, same_bits, subframe  # noqa: E402

CAMERA = ([0.0, 0.25, -8.0, 0.1], None)


@pytest.mark.parametrize("filter", [gra.FILTER_BOX, gra.FILTER_MITCHELL], ids=["box", "mitchell"])
@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("w,h", [(36, 20), (34, 19)])
def test_every_sink_gives_the_bytes_of_the_same_source(w, h, factor, filter):
    camera = gra.default_camera(*CAMERA)
    state = gra.RenderState(w, h, 0, supersample=factor, filter=filter)
    F = frame(state, camera)
    assert np.isfinite(F).all() and len(np.unique(encode_srgb8(F))) > 32   # a picture, not a flat frame
    rgba8, codes = encode_srgb8(F), frame_to_rgb10(F)
    assert frame(state, camera, "rgba8").tobytes() == rgba8.tobytes()
    for layout in (I420, NV12):
        assert frame(state, camera, "yuv420", layout).tobytes() == rgba8_to_yuv420(rgba8, layout).tobytes(), layout
        assert frame(state, camera, "yuv420p10", layout).astype("<u2").tobytes() == rgb10_to_yuv420p10(codes, layout).astype("<u2").tobytes(), layout
    same_bits(frame(state, camera), F, "the float frame again, after the encoded ones")
    subframe(state, camera, 1.0, True)
    every_delivery_is_the_encode_of(state, F)
