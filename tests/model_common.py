"""What the float64 models of two stages share (tests/render_data_model.py, tests/setup_model.py): the polar helpers of cl.cl:103-204,
the tetrad's frame_basis_with_swap (cl.cl:1761-1850) and the central-difference Jacobian of a chart map with its step rule."""
import numpy as np

JACOBIAN_STEP = 1e-5


def _polar_to_cartesian(p):
    r, th, ph = p
    return np.array([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)])


def _cartesian_to_polar(c):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(c @ c)
        return np.array([r, np.arccos(c[2] / r), np.arctan2(c[1], c[0])])


def _spherical_velocity_to_cartesian(p, dp):
    r, x, y = p
    dr, dx, dy = dp
    sx, cx, sy, cy = np.sin(x), np.cos(x), np.sin(y), np.cos(y)
    return np.array([-r * sx * sy * dy + r * cx * cy * dx + sx * cy * dr, sx * sy * dr + r * sx * cy * dy + r * cx * sy * dx, cx * dr - r * sx * dx])


def _cartesian_velocity_to_polar_velocity(p, v):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt(p @ p)
        repeated_eq = r * np.sqrt(1 - (p[2] * p[2] / (r * r)))
        rdot = (p @ v) / r
        tdot = ((p[2] * rdot) / (r * repeated_eq)) - v[2] / repeated_eq
        pdot = (p[0] * v[1] - p[1] * v[0]) / (p[0] * p[0] + p[1] * p[1])
    return np.array([rdot, tdot, pdot])


def _rot_quat(point, q):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = q / np.sqrt(q @ q)
    t = 2 * np.cross(q[:3], point)
    return point + q[3] * t + np.cross(q[:3], t)


def _frame_basis_with_swap(g, index_swap, trace=None):
    """-> (the timelike slot found, the four legs); `trace` (a dict) receives first_nonzero"""
    arr = [np.eye(4)[i] for i in range(4)]
    lengths = [g[i, i] for i in range(4)]
    arr[0], arr[index_swap] = arr[index_swap], arr[0]
    lengths[0], lengths[index_swap] = lengths[index_swap], lengths[0]
    indices = [0, 1, 2, 3]
    first = next((i for i in range(4) if not abs(lengths[i]) <= 0.00001), 0)
    if trace is not None:
        trace["first_nonzero"] = first
    if first != 0:
        arr[0], arr[first] = arr[first], arr[0]
        indices[0], indices[first] = indices[first], indices[0]
    dot = lambda u, v: (g @ u) @ v
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        proj = lambda u, v: (dot(u, v) / dot(u, u)) * u
        u1 = arr[0]
        u2 = arr[1] - proj(u1, arr[1])
        u3 = arr[2] - proj(u1, arr[2])
        u3 = u3 - proj(u2, u3)
        u4 = arr[3] - proj(u1, arr[3])
        u4 = u4 - proj(u2, u4)
        u4 = u4 - proj(u3, u4)
        res = [u / np.sqrt(abs(dot(u, u))) for u in (u1, u2, u3, u4)]
    ordered = [None] * 4
    for i in range(4):
        ordered[indices[i]] = res[i]
    lowest, lowest_value = -1, 0.0
    for i in range(4):
        with np.errstate(invalid="ignore", over="ignore"):
            d = dot(ordered[i], ordered[i])
        if d < lowest_value:
            lowest, lowest_value = i, d
    which = lowest if lowest != -1 else 0
    if which > 0:
        ordered[0], ordered[which] = ordered[which], ordered[0]
    return which, ordered


def _jacobian_of(f, x, angles=(3,)):
    """d f_i / d x_k [i][k] of a chart map by central differences, step JACOBIAN_STEP * max(1, |x_k|) (the truncation and rounding
    errors: tests/render_data_model.py's docstring).  The difference of an output listed in `angles` is taken modulo 2 pi (atan2's
    cut) - a no-op on every difference smaller than pi."""
    x = np.asarray(x, dtype=np.float64)
    J = np.zeros((4, 4))
    for k in range(4):
        h = JACOBIAN_STEP * max(1.0, abs(x[k]))
        up, down = x.copy(), x.copy()
        up[k] += h
        down[k] -= h
        with np.errstate(invalid="ignore"):
            d = f(up) - f(down)
            for i in angles:
                d[i] = d[i] - 2 * np.pi * np.rint(d[i] / (2 * np.pi))
        J[:, k] = d / (2 * h)
    return J
