"""The glare (include/geodesic_hip_internal.h, "Glare") restated from the header's text, for tests/test_glare_abi.py and
tests/test_gpu_glare.py: a float64 model with the standard bound on its running sums, a float32 restatement whose `*` and `+` are
single IEEE operations (numpy's), the inputs, and the tables that tell orders and directions apart.  Nothing here looks at the C code."""
import numpy as np

import geodesic_raytracing_amd as gra

# distinct, asymmetric, of both signs (the shape of tests/test_filter_abi.py's): a reversed order or the other axis' role gives other floats
UNEVEN15 = np.array([0.013 * (t + 2) * (-1 if t % 4 == 2 else 1) for t in range(15)], dtype=np.float32)
UNEVEN7 = np.array([0.07 * (t + 1) * (-1 if t % 3 == 1 else 1) for t in range(7)], dtype=np.float32)
UNEVEN129 = np.array([0.002 * (t + 3) * (-1 if t % 5 == 3 else 1) for t in range(129)], dtype=np.float32)


def make_glare(core, weights=(), tables=()):
    """a GlareStruct from a core, K weights and K tables of an odd number of taps; what the PSF does not use stays zero"""
    g = gra.GlareStruct()
    g.core, g.components = float(core), len(tables)
    for k, (weight, table) in enumerate(zip(weights, tables)):
        g.weight[k], g.taps[k] = float(weight), len(table)
        for t, value in enumerate(table):
            g.tap[k][t] = float(value)
    return g


def fields(g):
    """(core, weights, tables) of a GlareStruct as float32"""
    k = g.components
    return (np.float32(g.core), [np.float32(g.weight[i]) for i in range(k)], [np.array(g.tap[i][:g.taps[i]], dtype=np.float32) for i in range(k)])


def source(w, h, seed, planted=False):
    """float32 [h, w, 4]: normal-range values of both signs over several decades, as tests/test_gpu_filter.py::source makes them; planted:
    with +0, -0, both infinities and NaN in it, few enough that most footprints stay finite"""
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal((h, w, 4)) * np.exp(rs.uniform(-7, 7, (h, w, 4)))).astype(np.float32)
    v[np.abs(v) < 1e-20] = 1
    if planted:
        kind = rs.uniform(size=v.shape)
        for k, (value, share) in enumerate([(0.0, 0.01), (-0.0, 0.01), (np.inf, 0.0003), (-np.inf, 0.0003), (np.nan, 0.0003)]):
            v[(kind >= 0.01 * k) & (kind < 0.01 * k + share)] = value
    return v


def _passes(s, table, dtype):
    """g_k of the definition over the channels of s [H, W, C]: the rows pass, rounded to dtype, then the columns pass, in ascending t"""
    h, w = s.shape[:2]
    n = len(table)
    radius = (n - 1) // 2
    table = np.asarray(table, dtype=dtype)
    rows = None
    for t in range(n):
        cx = np.clip(np.arange(w) - radius + t, 0, w - 1)
        product = table[t] * s[:, cx, :]
        rows = product if t == 0 else rows + product
    out = None
    for t in range(n):
        cy = np.clip(np.arange(h) - radius + t, 0, h - 1)
        product = table[t] * rows[cy, :, :]
        out = product if t == 0 else out + product
    assert out.dtype == dtype
    return out


def model(src, g):
    """(the definition in float64 for r, g, b -> [H, W, 3]; A: the same expression with every tap, weight, core and sample replaced by
    its absolute value).  |gr_glare_frame - model| <= bound(g) * A is the standard bound on running sums of rounded products."""
    core, weights, tables = fields(g)
    s = np.asarray(src, dtype=np.float64)[..., :3]
    out, a = np.float64(core) * s, abs(np.float64(core)) * np.abs(s)
    for weight, table in zip(weights, tables):
        out = out + np.float64(weight) * _passes(s, table.astype(np.float64), np.float64)
        a = a + abs(np.float64(weight)) * _passes(np.abs(s), np.abs(table.astype(np.float64)), np.float64)
    return out, a


def bound(g):
    """(2 n_max + 2 K + 4) 2^-24: n_max products and n_max - 1 sums a pass, two passes, a product and a sum a component, the core's product"""
    n_max = max([g.taps[k] for k in range(g.components)] + [0])
    return (2 * n_max + 2 * g.components + 4) * 2.0 ** -24


def restated(src, g):
    """the definition in numpy float32, one rounded multiply and one rounded add at a time -> [H, W, 4]; alpha is the source's"""
    core, weights, tables = fields(g)
    src = np.asarray(src, dtype=np.float32)
    with np.errstate(all="ignore"):
        acc = core * src[..., :3]
        for weight, table in zip(weights, tables):
            product = weight * _passes(src[..., :3], table, np.float32)
            acc = acc + product
    assert acc.dtype == np.float32
    out = src.copy()
    out[..., :3] = acc
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """bit patterns equal wherever the value is a number, a NaN exactly where one is wanted (which NaN an operation returns is open)"""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
