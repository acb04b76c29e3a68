"""GPU test (-m gpu) of the core both device encoders sit on (csrc/device_encoders.cpp): a PNG literals encoder, a PNG runs encoder and a
JPEG encoder of one program alive together, encoding in turn - every file the host encoder's, every scratch intact, the launch timer each
encoder's own, and the three closed in either order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
from geodesic_raytracing_amd.pipeline import DeviceBuffer  # noqa: E402
from test_gpu_jpeg import kerr  # noqa: E402

WIDTH, HEIGHT, QUALITY = 33, 17, 90


def test_three_encoders_of_one_program_side_by_side():
    _, prog, _ = kerr()
    pixels = np.random.default_rng(3317).integers(0, 256, (HEIGHT, WIDTH, 4), dtype=np.uint8)
    frame = DeviceBuffer.from_numpy(0, pixels)
    expected = [gra.png_encode_host(pixels, "literals"), gra.png_encode_host(pixels, "runs"), gra.jpeg_encode_host(pixels, QUALITY)]
    for closing_order in (1, -1):   # in the order of creation, then in reverse
        encoders = [gra.PngEncoder(prog, WIDTH, HEIGHT, "literals"), gra.PngEncoder(prog, WIDTH, HEIGHT, "runs"), gra.JpegEncoder(prog, WIDTH, HEIGHT, QUALITY)]
        encoders[2].time_launches()
        for _round in range(2):
            for encoder, file in zip(encoders, expected):
                assert encoder.encode(frame.ptr) == file, (closing_order, _round, type(encoder).__name__, getattr(encoder, "stream_kind", None))
            assert [encoder.scratch_intact() for encoder in encoders] == [True, True, True]
        times = encoders[2].launch_ms()
        assert len(times) == 3 and all(ms > 0 for ms in times), times
        for png in encoders[:2]:   # (the JPEG encoder's timer is not theirs)
            with pytest.raises(gra.GeodesicError, match="no encode was timed"):
                png.launch_ms()
        for encoder in encoders[::closing_order]:
            encoder.close()
        assert all(encoder.handle is None for encoder in encoders)
