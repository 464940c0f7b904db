"""NumPy restatement of the geometry rules of the field evaluator (include/gmrf_hip.h, gmrf_eval_line_create / _tri_create): the
rows of E = evaluation_matrix(disc, points) on the project's lines and triangle meshes, the dof coordinates a test samples a
polynomial at, and the test points.  Every function takes the arithmetic's dtype (float64: the operations of the library in its
order; longdouble: the same rules carried further)."""
import numpy as np

LINES = [(nc, order, bc) for nc in (4, 5, 16) for order in (1, 2) for bc in ("periodic", "dirichlet")]
TRIANGLES = [(nx, ny, order) for nx, ny in ((3, 4), (5, 3), (17, 9)) for order in (1, 2)]


def line_length(bc):
    return 2.0 if bc == "dirichlet" else 1.0


def _sorted(idx, w):
    o = np.argsort(idx, axis=1, kind="stable")
    return np.take_along_axis(idx, o, axis=1), np.take_along_axis(w, o, axis=1)


def line_ns(nc, order, bc):
    return order * nc + (1 if bc == "dirichlet" else 0)


def line_rows(nc, order, bc, length, points, dtype=np.float64):
    """(idx (npts, order + 1) int64 ascending, w) of the points on the line of nc cells."""
    T = dtype
    x = np.asarray(points, dtype=T).reshape(-1)
    ns = line_ns(nc, order, bc)
    h = T(length) / T(nc)
    e = np.minimum(np.floor(x / h).astype(np.int64), nc - 1)
    xi = np.clip(T(2) * (x - e.astype(T) * h) / h - T(1), T(-1), T(1))
    if order == 1:
        idx = np.stack([e, (e + 1) % ns], axis=1)
        w = np.stack([(T(1) - xi) / T(2), (T(1) + xi) / T(2)], axis=1)
    else:
        idx = np.stack([2 * e, (2 * e + 2) % ns, 2 * e + 1], axis=1)
        w = np.stack([T(0.5) * xi * (xi - T(1)), T(0.5) * xi * (xi + T(1)), T(1) - xi * xi], axis=1)
    return _sorted(idx, w)


def tri_ns(nx, ny, order):
    return nx * ny if order == 1 else (2 * nx - 1) * (2 * ny - 1)


def tri_rows(nx, ny, order, xy, dtype=np.float64):
    """(idx (npts, 3 or 6) int64 ascending, w) of the points (npts, 2) on the nx x ny vertex mesh of the unit square."""
    T = dtype
    xy = np.asarray(xy, dtype=T).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    hx, hy = T(1) / T(nx - 1), T(1) / T(ny - 1)
    qx = np.minimum(np.floor(x / hx).astype(np.int64), nx - 2)
    qy = np.minimum(np.floor(y / hy).astype(np.int64), ny - 2)
    s = np.clip((x - qx.astype(T) * hx) / hx, T(0), T(1))
    t = np.clip((y - qy.astype(T) * hy) / hy, T(0), T(1))
    lower = t <= s
    one = T(1)
    # cell vertices (i, j) in local order: lower (n00, n10, n11), upper (n00, n11, n01)
    vi = np.stack([qx, qx + 1, np.where(lower, qx + 1, qx)], axis=1)
    vj = np.stack([qy, np.where(lower, qy, qy + 1), qy + 1], axis=1)
    lam = np.stack([np.where(lower, one - s, one - t), np.where(lower, s - t, s), np.where(lower, t, t - s)], axis=1)
    if order == 1:
        return _sorted(vi + nx * vj, lam)
    lx = 2 * nx - 1
    a, b = np.array([0, 1, 2]), np.array([1, 2, 0])
    idx = np.concatenate([2 * vi + lx * (2 * vj), (vi[:, a] + vi[:, b]) + lx * (vj[:, a] + vj[:, b])], axis=1)
    w = np.concatenate([lam * (T(2) * lam - one), T(4) * lam[:, a] * lam[:, b]], axis=1)
    return _sorted(idx, w)


def _vertex_coords(n, h, last, dtype):
    c = np.arange(n).astype(dtype) * dtype(h)
    c[-1] = dtype(last)
    return c


def line_dof_coords(nc, order, bc, length, dtype=np.float64):
    """Coordinates of the ns dofs numbered by position: vertices e h (the last one exactly `length`), midpoints between them."""
    T = dtype
    v = _vertex_coords(nc + 1, T(length) / T(nc), length, T)
    if order == 1:
        c = v
    else:
        c = np.empty(2 * nc + 1, dtype=T)
        c[0::2] = v
        c[1::2] = T(0.5) * (v[:-1] + v[1:])
    return c[:line_ns(nc, order, bc)]


def tri_dof_coords(nx, ny, order, dtype=np.float64):
    """(ns, 2) coordinates of the dofs, x fastest: vertices i (1 / (n - 1)) with the last one exactly 1.0; order 2: the lattice of
    vertices and edge midpoints."""
    T = dtype

    def axis(n):
        v = _vertex_coords(n, T(1) / T(n - 1), 1.0, T)
        if order == 1:
            return v
        c = np.empty(2 * n - 1, dtype=T)
        c[0::2] = v
        c[1::2] = T(0.5) * (v[:-1] + v[1:])
        return c
    X, Y = axis(nx), axis(ny)
    return np.stack([np.tile(X, Y.size), np.repeat(Y, X.size)], axis=1)


def line_points(nc, bc, length, seed=0, n_random=300):
    """300 uniform random points, then the corner cases: every vertex (both ends of every cell), the cell midpoints, and the end of
    the domain -- x = length on the interval, the largest double below `length` on the periodic line (LAST: its row holds dof 0)."""
    rng = np.random.default_rng(seed)
    h = length / nc
    verts = np.arange(nc) * h
    end = length if bc == "dirichlet" else np.nextafter(length, 0.0)
    return np.concatenate([rng.uniform(0.0, length, n_random), verts, verts + 0.5 * h, np.nextafter(verts[1:], 0.0), [end]])


def tri_points(nx, ny, seed=0, n_random=300):
    """300 uniform random points, then the corner cases, in this order: every vertex; points on the cut diagonal of the first quad
    with t == s exactly (0.5 and 0.25 of it) and of every quad approximately; points on x = 1 and on y = 1; (0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    vx, vy = np.arange(nx) * hx, np.arange(ny) * hy
    vx[-1] = vy[-1] = 1.0
    verts = np.stack([np.tile(vx, ny), np.repeat(vy, nx)], axis=1)
    diag0 = np.array([[0.5 * hx, 0.5 * hy], [0.25 * hx, 0.25 * hy]])
    a = rng.uniform(0.0, 1.0, (nx - 1) * (ny - 1))
    qx, qy = np.tile(np.arange(nx - 1), ny - 1), np.repeat(np.arange(ny - 1), nx - 1)
    diag = np.stack([(qx + a) * hx, (qy + a) * hy], axis=1)
    r = rng.uniform(0.0, 1.0, 8)
    sides = np.concatenate([np.stack([np.ones(8), r], axis=1), np.stack([r, np.ones(8)], axis=1), [[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]]])
    pts = np.concatenate([rng.uniform(0.0, 1.0, (n_random, 2)), verts, diag0, diag, sides, [[0.5, 0.5]]])
    return np.clip(pts, 0.0, 1.0)


def dot_rows(idx, w, fields):
    """sum_k w[c][k] fields[..., idx[c][k]] in longdouble, and sum_k |w| |f| beside it: (ref, mag), each (..., npts)."""
    wl, f = w.astype(np.longdouble), np.asarray(fields).astype(np.longdouble)[..., idx]
    return np.sum(wl * f, axis=-1), np.sum(np.abs(wl) * np.abs(f), axis=-1)
