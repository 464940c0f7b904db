"""What the tests of the pointwise predictive variance (gmrf_eval_pairs / _var_batch / _calibration_batch) share: geometries as
tuples ("line", nc, order, bc) / ("tri", nx, ny, order), the element connectivity of a geometry from tests/field_eval_oracle.py's
rows, the test matrix A on it, its inverse in longdouble, and the quadratic form diag(E Sigma E^T) in longdouble."""
import functools

import numpy as np
import scipy.sparse as sp

from tests import field_eval_oracle as FO

EPS = 2.0 ** -52


def ns_of(geom):
    return FO.line_ns(*geom[1:]) if geom[0] == "line" else FO.tri_ns(*geom[1:])


def width_of(geom):
    return geom[2] + 1 if geom[0] == "line" else (3 if geom[3] == 1 else 6)


def points_of(geom, n_random=300):
    if geom[0] == "line":
        return FO.line_points(geom[1], geom[3], FO.line_length(geom[3]), n_random=n_random)
    return FO.tri_points(geom[1], geom[2], n_random=n_random)


def evaluator(pkg, geom, pts, **kw):
    if geom[0] == "line":
        _, nc, order, bc = geom
        return pkg.FieldEvaluator.line(nc, pts, order=order, bc=bc, length=FO.line_length(bc), **kw)
    return pkg.FieldEvaluator.triangles(geom[1], geom[2], pts, order=geom[3], **kw)


def element_dofs(geom):
    """(cells, width) dofs of every element: the oracle's rows at the elements' midpoints / centroids."""
    if geom[0] == "line":
        _, nc, order, bc = geom
        length = FO.line_length(bc)
        return FO.line_rows(nc, order, bc, length, (np.arange(nc) + 0.5) * (length / nc))[0]
    _, nx, ny, order = geom
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    qx, qy = np.tile(np.arange(nx - 1), ny - 1), np.repeat(np.arange(ny - 1), nx - 1)
    lower = np.stack([(qx + 2.0 / 3.0) * hx, (qy + 1.0 / 3.0) * hy], axis=1)
    upper = np.stack([(qx + 1.0 / 3.0) * hx, (qy + 2.0 / 3.0) * hy], axis=1)
    return FO.tri_rows(nx, ny, order, np.concatenate([lower, upper]))[0]


def connectivity(geom):
    """Dense boolean (ns, ns): dofs that share an element (the diagonal included)."""
    ns = ns_of(geom)
    M = np.zeros((ns, ns), dtype=bool)
    for row in element_dofs(geom):
        M[np.ix_(row, row)] = True
    return M


@functools.lru_cache(maxsize=None)
def spd_matrix(geom, nt, batch, seed=0):
    """(pattern, values, dense): the CSC pattern (sorted, values 1.0) shared by `batch` strictly diagonally dominant -- so SPD --
    matrices of size nt ns, their values (batch, nnz) in its order, and the matrices dense (batch, n, n).  Off-diagonals -|u|, u
    seeded uniform in (-1, 1), on the full element connectivity of every slice (other values per slice and problem), -0.3 I between
    neighbouring slices, the diagonal the sum of the row's |off-diagonals| + 1."""
    ns, n = ns_of(geom), nt * ns_of(geom)
    conn = connectivity(geom)
    mask = np.kron(np.eye(nt, dtype=bool), conn)
    mask |= np.kron(np.eye(nt, k=1, dtype=bool) | np.eye(nt, k=-1, dtype=bool), np.eye(ns, dtype=bool))
    rng = np.random.default_rng(seed + 1000 * nt + batch)
    dense = np.zeros((batch, n, n))
    for p in range(batch):
        u = -np.abs(np.triu(rng.uniform(-1.0, 1.0, (n, n)), 1))
        off = np.where(np.kron(np.eye(nt, dtype=bool), conn), u + u.T, 0.0)
        np.fill_diagonal(off, 0.0)
        off -= 0.3 * (np.eye(n, k=ns) + np.eye(n, k=-ns))
        dense[p] = off + np.diag(np.abs(off).sum(axis=1) + 1.0)
    pattern = sp.csc_matrix(mask.astype(np.float64))
    pattern.sort_indices()
    cols = np.repeat(np.arange(n), np.diff(pattern.indptr))
    values = np.stack([d[pattern.indices, cols] for d in dense])
    return pattern, values, dense



def inverse_longdouble(A):
    """inv(A) of a dense well-conditioned matrix in longdouble: the double inverse, then two Newton-Schulz steps X += X (I - A X)
    carried in longdouble (each squares the residual, |I - A X| ~ 1e-15 -> the format's rounding)."""
    Al = np.asarray(A, dtype=np.longdouble)
    X = np.linalg.inv(np.asarray(A, dtype=np.float64)).astype(np.longdouble)
    eye = np.eye(A.shape[0], dtype=np.longdouble)
    for _ in range(2):
        X = X + X @ (eye - Al @ X)
    return 0.5 * (X + X.T)


def quadratic_form(idx, w, nt, ns, sigma, scale=None):
    """(v, mag), each (nt, npts): v = sum_ab w_a w_b Sigma[t ns + i_a, t ns + i_b] in longdouble over a dense Sigma (n, n), and
    mag = sum_ab |w_a w_b Sigma_ab| -- or, with scale = d (n,), sum_ab |w_a w_b| d_a d_b."""
    wl = w.astype(np.longdouble)
    S = np.asarray(sigma, dtype=np.longdouble)
    v, mag = [], []
    for t in range(nt):
        j = idx + t * ns
        blk = S[j[:, :, None], j[:, None, :]]
        ww = wl[:, :, None] * wl[:, None, :]
        v.append(np.sum(ww * blk, axis=(1, 2)))
        if scale is None:
            mag.append(np.sum(np.abs(ww * blk), axis=(1, 2)))
        else:
            d = np.asarray(scale, dtype=np.longdouble)[j]
            mag.append(np.sum(np.abs(ww) * d[:, :, None] * d[:, None, :], axis=(1, 2)))
    return np.stack(v), np.stack(mag)
