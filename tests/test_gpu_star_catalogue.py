"""GPU tests (-m gpu) of the star catalogue built on the device (kernels/stars.hip behind gr_star_catalogue_create) against the numpy
catalogue of tests/star_sky_model.py: cell_start and the order of the stars equal the model's exactly, the float64 summed-area table is
within 1e-12 relative, and a second build gives identical bytes - the scatter's atomics decide nothing."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import geodesic_raytracing_amd as gra  # noqa: E402
import star_sky_model as ssm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "geodesic_raytracing_amd", "scripts")
_shared = {}


def program():
    if "program" not in _shared:
        metric = gra.Metric("kerr_boyer", SCRIPTS)
        _shared["program"] = gra.Program(metric.argument_string(), 0)
    return _shared["program"]


def fields():
    rng = np.random.default_rng(11)
    one = (np.array([[0.7312, 0.2501]]), np.array([[1e-6, 2e-6, 3e-6]]))
    # 257 stars: a seam pair at u = 0 and u = 1 - 2^-24, stars at v = 0 and v = 1, two identical stars
    uv = rng.random((257, 2))
    uv[:7] = [(0.0, 0.4), (1 - 2.0 ** -24, 0.4), (0.3, 0.0), (0.6, 1.0), (0.123, 0.456), (0.123, 0.456), (1 - 2.0 ** -24, 1.0)]
    edge = (uv, rng.uniform(0, 1e-5, (257, 3)))
    # 300 stars all in one cell of either grid
    crowd = (np.stack([0.501 + rng.random(300) * 0.013, 0.2505 + rng.random(300) * 0.029], axis=1), rng.uniform(0, 1e-5, (300, 3)))
    random = ssm.star_field_random(3, 5000)
    return {"one": one, "edge_257": edge, "one_cell_300": crowd, "random_5000": random}


@pytest.mark.parametrize("cells", [(16, 16), (64, 32)])
@pytest.mark.parametrize("name", ["one", "edge_257", "one_cell_300", "random_5000"])
def test_the_device_builds_the_models_catalogue(name, cells):
    uv, flux = fields()[name]
    uv, flux = np.asarray(uv, dtype=np.float32), np.asarray(flux, dtype=np.float32)
    want = ssm.catalogue(uv, flux, *cells)
    if name == "one_cell_300":
        assert len(np.unique(want["cell"])) == 1
    built = gra.StarCatalogue(program(), uv, flux, *cells)
    assert (built.n, built.cells_u, built.cells_v) == (len(uv), *cells)
    cell_start, order, table = built.download()
    assert np.array_equal(cell_start, want["cell_start"])
    assert np.array_equal(order, want["order"])
    assert (table[:, 0, :] == 0).all() and (table[:, :, 0] == 0).all()
    scale = np.abs(want["table"]).max(axis=(1, 2), keepdims=True)
    assert (np.abs(table - want["table"]) <= 1e-12 * scale).all()
    assert np.allclose(table[:, -1, -1], flux.astype(np.float64).sum(axis=0), rtol=1e-12)
    again = gra.StarCatalogue(program(), uv, flux, *cells).download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (cell_start, order, table))), "two builds differ"


def test_the_default_cells_and_a_million_stars():
    """1024 x 512 cells, three chunks of the scan's second level and cells of several stars: the order is still the model's"""
    uv, flux = gra.star_field_random(5, 1 << 20)
    built = gra.StarCatalogue(program(), uv, flux)
    assert (built.cells_u, built.cells_v) == (1024, 512)
    want = ssm.catalogue(uv, flux, 1024, 512)
    cell_start, order, table = built.download()
    assert np.array_equal(cell_start, want["cell_start"]) and np.array_equal(order, want["order"])
    assert (np.abs(table - want["table"]) <= 1e-12 * np.abs(want["table"]).max(axis=(1, 2), keepdims=True)).all()
