"""Host-side mirror of the reference's operator surface for the block-tridiagonal path.

Same names, argument meaning and error behaviour as
/root/reference/src/tridiagonal_cholesky.jl (`tridiagonal_cholesky` :65-82,
`forward_solve` :43-52, `backward_solve` :24-33, `ldiv!`/`ldiv` :54-63, `make_chunks`
:11-14, struct fields `N`, `chos`, `Cs` :5-9) and scripts/solve_burger.jl:182-254
(`extract_blocks`), with every numeric step done by libgmrf_hip.so on the GPU.  Julia is not
available in this image, so this Python layer stands where the Julia shim
(julia/DiffEqGMRFsHIP.jl) stands in a Julia session; both are thin wrappers over the same
C ABI (include/gmrf_hip.h).

Vectors / matrices may be NumPy arrays (host) or torch CUDA tensors (device resident; no
PCIe traffic).  Matrices of right-hand sides are n x k in column-major order (Julia
layout): pass `np.asfortranarray(B)` or a torch tensor of shape (k, n) via `.T`.
"""
from __future__ import annotations

import ctypes as C
import enum
from typing import List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from . import _cabi
from ._cabi import GmrfError, NotPositiveDefinite  # noqa: F401  (re-exported)


class Switch(enum.IntFlag):
    """The route switches of a factor handle (`TridiagonalCholeskyFactor.set_eager`): the GMRF_SW_* constants of
    include/gmrf_hip.h one for one, where each is described.  The values are ABI."""
    EAGER = 1 << 0
    BATCH_ROUTES = 1 << 1
    SWEEP_NO_GEMM = 1 << 2
    DENSE_COUPLING = 1 << 3
    FORK_GRAPH = 1 << 4
    NO_STAIRCASE = 1 << 5
    DOUBLING_INVERSE = 1 << 7
    NO_LOOKAHEAD = 1 << 8
    NO_XSPLIT = 1 << 12
    NO_PERSIST = 1 << 13
    NO_PERSIST_PANELS = 1 << 15
    NO_SWEEP_PERSIST = 1 << 16
    NO_SCATTER_FOLD = 1 << 17
    TWO_CALL_POSTERIOR = 1 << 18
    NO_FACTOR_FWD = 1 << 19
    NO_GROUPED_GEMM = 1 << 20
    NO_ENVELOPE = 1 << 21


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def _colmajor(b, n: int):
    """Return (array_or_tensor, k, ld, was_1d) with column-major n x k storage."""
    if _is_torch(b):
        import torch
        if b.dtype != torch.float64:
            raise TypeError("float64 required")
        if b.dim() == 1:
            if b.shape[0] != n:
                raise ValueError("dimension mismatch")
            return b.contiguous(), 1, n, True
        # a (n, k) tensor whose transpose is contiguous is column-major
        if b.shape[0] != n:
            raise ValueError("dimension mismatch")
        bt = b.t()
        if not bt.is_contiguous():
            bt = bt.contiguous()
        return bt, b.shape[1], n, False          # bt is (k, n) row-major == n x k column-major
    a = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        if a.shape[0] != n:
            raise ValueError("dimension mismatch")
        return np.ascontiguousarray(a), 1, n, True
    if a.shape[0] != n:
        raise ValueError("dimension mismatch")
    return np.asfortranarray(a), a.shape[1], n, False


def _alloc_like(ref, n: int, k: int, one_d: bool):
    if _is_torch(ref):
        import torch
        out = torch.empty((k, n), dtype=torch.float64, device=ref.device)
        return out, (out[0] if one_d else out.t())
    out = np.empty((n, k), dtype=np.float64, order="F")
    return out, (out[:, 0] if one_d else out)


class CsrMatrix:
    """Device-resident sparse matrix for `Q * x` (K6).  For a symmetric matrix the CSC arrays
    of a SparseMatrixCSC are the CSR arrays of the same matrix."""

    def __init__(self, A, device: int = 0, values_f32: bool = False, stream: int = 0):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.shape = A.shape
        self.nnz = int(A.nnz)
        self._h = C.c_void_p()
        rp = A.indptr.astype(np.int64)
        ci = A.indices.astype(np.int64)
        v = A.data.astype(np.float64)
        self.indptr, self.indices = rp, A.indices.astype(np.int32)       # the pattern (selected_inverse returns it)
        lib = _cabi.load()
        _cabi.check(lib.gmrf_csr_create(device, C.c_void_p(stream), A.shape[0], A.shape[1], _cabi.ptr(rp),
                                        _cabi.ptr(ci), _cabi.ptr(v), 0, int(values_f32), C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_csr_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def __matmul__(self, X):
        return self.matmul(X)

    def matmul_into(self, X, Y):
        """Stream-ordered Y = S X for torch CUDA tensors, written into `Y`, without synchronising (gmrf_spmm_async /
        gmrf_spmm_rows_async): X (n,) or C-contiguous (n, k) = node-major; Y of the matching shape."""
        if not (_is_torch(X) and _is_torch(Y) and X.is_cuda and Y.is_cuda and X.is_contiguous() and Y.is_contiguous()):
            raise TypeError("matmul_into takes contiguous torch CUDA tensors")
        lib = _cabi.load()
        if X.ndim == 1:
            _cabi.check(lib.gmrf_spmm_async(self._h, _cabi.ptr(X), _cabi.ptr(Y), 1, self.shape[1], self.shape[0]))
        else:
            k = X.shape[1]
            _cabi.check(lib.gmrf_spmm_rows_async(self._h, _cabi.ptr(X), _cabi.ptr(Y), k, k, k))
        return Y

    def matmul_rows(self, X):
        """Y = S X for X stored node-major: an (n, k) C-contiguous NumPy array or torch CUDA tensor (the k
        values of a node side by side).  This is the layout of the LDS-tiled SpMM kernel."""
        n = self.shape[1]
        if X.ndim != 2 or X.shape[0] != n:
            raise ValueError("dimension mismatch")
        k = X.shape[1]
        if _is_torch(X):
            import torch
            if X.dtype != torch.float64:
                raise TypeError("float64 required")
            X = X.contiguous()
            Y = torch.empty((self.shape[0], k), dtype=torch.float64, device=X.device)
        else:
            X = np.ascontiguousarray(X, dtype=np.float64)
            Y = np.empty((self.shape[0], k), dtype=np.float64)
        _cabi.check(_cabi.load().gmrf_spmm_rows(self._h, _cabi.ptr(X), _cabi.ptr(Y), k, k, k))
        return Y

    def matmul(self, X):
        n = self.shape[1]
        # a row-major (n, k) operand already is node-major: no copy, LDS-tiled kernel
        if getattr(X, "ndim", 0) == 2 and X.shape[1] > 1 and X.shape[0] == n:
            row_major = X.is_contiguous() if _is_torch(X) else (X.flags.c_contiguous and not X.flags.f_contiguous)
            if row_major and (not _is_torch(X) or X.dtype.is_floating_point):
                return self.matmul_rows(X)
        xa, k, ld, one_d = _colmajor(X, n)
        store, view = _alloc_like(xa, self.shape[0], k, one_d)
        _cabi.check(_cabi.load().gmrf_spmm(self._h, _cabi.ptr(xa), _cabi.ptr(store), k, ld, self.shape[0]))
        return view


class PosteriorAssembler:
    """Device assembly of the Gauss-Newton / conditioning system:

        A   = Q + noise * J' * J                        scripts/solve_burger.jl:145
        rhs = base + noise * J' * (J * x + obs_diff)    scripts/solve_burger.jl:146

    for fixed sparsity patterns of Q (n x n, symmetric, both triangles) and J (m x n).  The
    symbolic phase runs once here; `precision()` / `rhs()` take the current values as NumPy arrays
    or torch CUDA tensors and return the same kind.  `pattern` is the CSC matrix (values 1) whose
    `.data` order `precision()` fills -- factor it once with `TridiagonalCholeskyFactor.factor`,
    then `refactor(values)`.  device = -1: symbolic only (no GPU needed)."""

    def __init__(self, Q, J, device: int = 0, stream: int = 0):
        Q = sp.csc_matrix(Q); Q.sort_indices()
        J = sp.csr_matrix(J); J.sort_indices()
        if Q.shape[0] != Q.shape[1] or J.shape[1] != Q.shape[0]:
            raise ValueError("Q must be n x n and J m x n")
        self.n, self.m = Q.shape[0], J.shape[0]
        self.nnz_q, self.nnz_j = int(Q.nnz), int(J.nnz)
        self._h = C.c_void_p()
        lib = _cabi.load()
        qp, qi = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)
        jp, ji = J.indptr.astype(np.int64), J.indices.astype(np.int64)
        _cabi.check(lib.gmrf_assemble_create(device, C.c_void_p(stream), self.n, _cabi.ptr(qp), _cabi.ptr(qi), self.m,
                                             _cabi.ptr(jp), _cabi.ptr(ji), 0, C.byref(self._h)))
        nnz, nprod = C.c_int64(0), C.c_int64(0)
        _cabi.check(lib.gmrf_assemble_pattern(self._h, C.byref(nnz), C.byref(nprod), None, None, 0))
        self.nnz_out, self.n_products = int(nnz.value), int(nprod.value)
        cp, rv = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz_out, dtype=np.int64)
        _cabi.check(lib.gmrf_assemble_pattern(self._h, None, None, _cabi.ptr(cp), _cabi.ptr(rv), 0))
        self.pattern = sp.csc_matrix((np.ones(self.nnz_out), rv, cp), shape=(self.n, self.n))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_assemble_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def _like(ref, count):
        if _is_torch(ref):
            import torch
            return torch.empty(count, dtype=torch.float64, device=ref.device)
        return np.empty(count, dtype=np.float64)

    @staticmethod
    def _vec(v, count, name):
        if v is None:
            return None
        if _is_torch(v):
            v = v.contiguous()
        else:
            v = np.ascontiguousarray(v, dtype=np.float64)
        if (v.numel() if _is_torch(v) else v.size) != count:
            raise ValueError(f"{name}: expected {count} values")
        return v

    def precision(self, q_values, j_values, noise: float):
        q = self._vec(q_values, self.nnz_q, "q_values")
        j = self._vec(j_values, self.nnz_j, "j_values")
        out = self._like(j, self.nnz_out)
        _cabi.check(_cabi.load().gmrf_assemble_precision(self._h, _cabi.ptr(q), _cabi.ptr(j), float(noise), _cabi.ptr(out)))
        return out

    def rhs(self, base, j_values, x, obs_diff, noise: float):
        j = self._vec(j_values, self.nnz_j, "j_values")
        xv = self._vec(x, self.n, "x")
        b = self._vec(base, self.n, "base")
        o = self._vec(obs_diff, self.m, "obs_diff")
        out = self._like(j, self.n)
        _cabi.check(_cabi.load().gmrf_assemble_rhs(self._h, _cabi.ptr(b) if b is not None else None, _cabi.ptr(j),
                                                  _cabi.ptr(xv), _cabi.ptr(o) if o is not None else None, float(noise),
                                                  _cabi.ptr(out)))
        return out

    # -- a batch of problems on the same patterns: arrays (B, ...) C-contiguous, NumPy or torch CUDA in, the same kind out
    @staticmethod
    def _mat(v, B, count, name):
        if v is None:
            return None
        v = v.contiguous() if _is_torch(v) else np.ascontiguousarray(v, dtype=np.float64)
        if _is_torch(v):
            import torch
            if v.dtype != torch.float64:
                raise TypeError("float64 required")
        if v.ndim != 2 or v.shape[0] != B or v.shape[1] != count:
            raise ValueError(f"{name}: expected shape ({B}, {count})")
        return v

    def _q(self, q_values, B):
        """(values, stride): one (nnz_q,) array shared by the batch (stride 0) or (B, nnz_q) per problem."""
        if getattr(q_values, "ndim", 1) == 2:
            return self._mat(q_values, B, self.nnz_q, "q_values"), self.nnz_q
        return self._vec(q_values, self.nnz_q, "q_values"), 0

    @staticmethod
    def _like2(ref, shape):
        if _is_torch(ref):
            import torch
            return torch.empty(shape, dtype=torch.float64, device=ref.device)
        return np.empty(shape, dtype=np.float64)

    def precision_batch(self, q_values, j_values, noise: float):
        """j_values (B, nnz_j) -> (B, nnz_out): row p is `precision` of problem p, bit for bit.  q_values: (nnz_q,) shared or
        (B, nnz_q) per problem."""
        B = j_values.shape[0]
        j = self._mat(j_values, B, self.nnz_j, "j_values")
        q, stride = self._q(q_values, B)
        out = self._like2(j, (B, self.nnz_out))
        _cabi.check(_cabi.load().gmrf_assemble_precision_batch(self._h, B, _cabi.ptr(q), stride, _cabi.ptr(j), float(noise),
                                                               _cabi.ptr(out)))
        return out

    def rhs_batch(self, base, j_values, x, obs_diff, noise: float):
        """(B, n) right-hand sides: row p is `rhs` of problem p, bit for bit (base / obs_diff may be None)."""
        B = j_values.shape[0]
        j = self._mat(j_values, B, self.nnz_j, "j_values")
        xv, b, o = self._mat(x, B, self.n, "x"), self._mat(base, B, self.n, "base"), self._mat(obs_diff, B, self.m, "obs_diff")
        out = self._like2(j, (B, self.n))
        _cabi.check(_cabi.load().gmrf_assemble_rhs_batch(self._h, B, _cabi.ptr(b), _cabi.ptr(j), _cabi.ptr(xv), _cabi.ptr(o),
                                                         float(noise), _cabi.ptr(out)))
        return out

    def objective_batch(self, q_values, x_prior, x, obs_diff, noise: float):
        """(B,) objectives (x_prior - x)' Q (x_prior - x) + noise |obs_diff|^2 (scripts/solve_burger.jl:157): a fixed-shape
        sum, the same bits on every call and whatever batch a problem sits in."""
        B = x.shape[0]
        xv, xp, o = self._mat(x, B, self.n, "x"), self._mat(x_prior, B, self.n, "x_prior"), self._mat(obs_diff, B, self.m, "obs_diff")
        q, stride = self._q(q_values, B)
        out = self._like2(xv, (B,))
        _cabi.check(_cabi.load().gmrf_assemble_objective_batch(self._h, B, _cabi.ptr(q), stride, _cabi.ptr(xp), _cabi.ptr(xv),
                                                               _cabi.ptr(o), float(noise), _cabi.ptr(out)))
        return out

    def quadform_batch(self, a_values, x, z):
        """(B,) quadratic forms (z - x)' A (z - x), `sqmahal(x, z)` of scripts/burgers/solve_burgers_gmrf-collocation.jl:208-215:
        a_values (nnz_out,) shared or (B, nnz_out) per problem, the values on `pattern` as `precision_batch` returns them; x, z
        (B, n).  One pass over the values on the device, a fixed-shape sum: the same bits on every call and whatever batch a
        problem sits in (gmrf_assemble_quadform_batch)."""
        B = x.shape[0]
        xv, zv = self._mat(x, B, self.n, "x"), self._mat(z, B, self.n, "z")
        if getattr(a_values, "ndim", 1) == 2:
            a, stride = self._mat(a_values, B, self.nnz_out, "a_values"), self.nnz_out
        else:
            a, stride = self._vec(a_values, self.nnz_out, "a_values"), 0
        out = self._like2(xv, (B,))
        _cabi.check(_cabi.load().gmrf_assemble_quadform_batch(self._h, B, _cabi.ptr(a), stride, _cabi.ptr(xv), _cabi.ptr(zv),
                                                              _cabi.ptr(out)))
        return out


class DarcyP1Assembler:
    """Darcy stiffness matrix and load vector on the device (first piece):
    `assemble_darcy_diff_matrix` of /root/reference/src/problems/darcy.jl:5-63 on the structured P1 mesh
    (nx x ny nodes, x fastest, quads cut by the diagonal n00 - n11, one quadrature point per cell), the
    coefficient looked up by nearest grid point (src/datasets/darcy.jl:30-34), Dirichlet rows / columns
    applied.  `pattern` is the CSR matrix (values 1) whose `.data` order `assemble()` fills -- the `J`
    of `PosteriorAssembler`.  device = -1: pattern only (no GPU needed).
    order = 2: the reference's own element (src/utils.jl:32-33) -- Lagrange{RefTriangle,2} with the 4-point rule of degree 3
    on the same nx x ny vertex mesh; dofs = the (2 nx - 1) x (2 ny - 1) lattice of vertices and edge midpoints."""

    def __init__(self, nx: int, ny: int, device: int = 0, stream: int = 0, order: int = 1):
        if order not in (1, 2):
            raise ValueError("order must be 1 (P1) or 2 (quadratic triangles)")
        self.nx, self.ny, self.order = int(nx), int(ny), int(order)
        self.n = int(nx) * int(ny) if order == 1 else (2 * int(nx) - 1) * (2 * int(ny) - 1)
        self._h = C.c_void_p()
        lib = _cabi.load()
        create = lib.gmrf_darcy_p1_create if order == 1 else lib.gmrf_darcy_p2_create
        _cabi.check(create(device, C.c_void_p(stream), nx, ny, C.byref(self._h)))
        nnz = C.c_int64(0)
        _cabi.check(lib.gmrf_darcy_p1_pattern(self._h, C.byref(nnz), None, None, 0))
        self.nnz = int(nnz.value)
        rp, ci = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        _cabi.check(lib.gmrf_darcy_p1_pattern(self._h, None, _cabi.ptr(rp), _cabi.ptr(ci), 0))
        self.pattern = sp.csr_matrix((np.ones(self.nnz), ci, rp), shape=(self.n, self.n))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_darcy_p1_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def assemble(self, coeff_table, beta: float = 1.0):
        """coeff_table: (ng, ng) array a[x index, y index] on the grid linspace(0, 1, ng)^2 (NumPy array or
        torch CUDA tensor).  Returns (values in `pattern.data` order, load vector f), same kind as the input."""
        if _is_torch(coeff_table):
            import torch
            tab = coeff_table.contiguous()
            vals = torch.empty(self.nnz, dtype=torch.float64, device=tab.device)
            f = torch.empty(self.n, dtype=torch.float64, device=tab.device)
        else:
            tab = np.ascontiguousarray(coeff_table, dtype=np.float64)
            vals, f = np.empty(self.nnz), np.empty(self.n)
        if tab.ndim != 2 or tab.shape[0] != tab.shape[1]:
            raise ValueError("coeff_table must be square (ng x ng)")
        _cabi.check(_cabi.load().gmrf_darcy_p1_assemble(self._h, _cabi.ptr(tab), tab.shape[0], float(beta), _cabi.ptr(vals),
                                                        _cabi.ptr(f)))
        return vals, f


    def assemble_batch(self, tables, beta: float = 1.0):
        """tables: (B, ng, ng) coefficient tables (NumPy array or torch CUDA tensor) -> (values (B, nnz), load vectors (B, n)),
        same kind as the input; row p is `assemble(tables[p])`, bit for bit."""
        if _is_torch(tables):
            import torch
            tab = tables.contiguous()
            if tab.dtype != torch.float64:
                raise TypeError("float64 required")
        else:
            tab = np.ascontiguousarray(tables, dtype=np.float64)
        if tab.ndim != 3 or tab.shape[1] != tab.shape[2]:
            raise ValueError("tables must have shape (B, ng, ng)")
        B = tab.shape[0]
        vals, f = PosteriorAssembler._like2(tab, (B, self.nnz)), PosteriorAssembler._like2(tab, (B, self.n))
        _cabi.check(_cabi.load().gmrf_darcy_p1_assemble_batch(self._h, B, _cabi.ptr(tab), tab.shape[1], float(beta), _cabi.ptr(vals),
                                                              _cabi.ptr(f)))
        return vals, f


class BurgersP1Tangent:
    """Residual and tangent of the Burgers space-time system on the device (second
    piece): `f_and_J` of /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:118-149 with
    `assemble_burgers_advection_matrix` (src/problems/burgers.jl:5-59) per time slice and the static part of
    `assemble_burgers_mass_diffusion_matrices` (:60-98), on the periodic P1 line (ns nodes on [0,1), nt slices,
    time-major index) or, with order = 2, the quadratic periodic line.  `pattern` is the CSR matrix (values 1, (nt-1) ns x nt ns, 6 entries per row) whose `.data`
    order `tangent()` fills -- the `J` of `PosteriorAssembler`.  device = -1: pattern only (no GPU needed).

    scheme = "cn": Crank-Nicolson, `f_and_J_CN` of _research/burgers_chen24.jl:121-132, :195-226 (the same pattern).
    bc = "dirichlet": an interval of `length` with homogeneous Dirichlet ends (:101-108), ns = order * cells + 1 dofs numbered by
    position; the rows and columns of dofs 0 and ns - 1 hold stored zeros and f is 0 there (a prior pins them), and a row holds
    its in-range columns only.  All 8 combinations of (order, scheme, bc) are served (gmrf_burgers_line_create)."""

    SCHEMES = {"euler": 0, "cn": 1}
    BCS = {"periodic": 0, "dirichlet": 1}

    def __init__(self, ns: int, nt: int, dt: float, nu: float, device: int = 0, stream: int = 0, order: int = 1,
                 scheme: str = "euler", bc: str = "periodic", length: float = 1.0):
        """ns: the number of dofs.  order = 2: the quadratic line of the reference's scripts (src/utils.jl:42-49): dofs numbered by
        position, vertex rows of J with 10 entries, midpoint rows with 6; ns = 2 N_x (periodic) or 2 N_x + 1 (dirichlet)."""
        self.ns, self.nt, self.dt, self.nu, self.order = int(ns), int(nt), float(dt), float(nu), int(order)
        self.scheme, self.bc, self.length = scheme, bc, float(length)
        if scheme not in self.SCHEMES or bc not in self.BCS or self.order not in (1, 2):
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"BurgersP1Tangent: order {order!r} (1, 2), scheme {scheme!r} {tuple(self.SCHEMES)}, "
                                                 f"bc {bc!r} {tuple(self.BCS)}")
        ends = 1 if bc == "dirichlet" else 0
        if (self.ns - ends) % self.order:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"BurgersP1Tangent: ns = {ns} is not {self.order} * cells + {ends}, the dofs of the "
                                                 f"order-{self.order} {bc} line")
        self.cells = (self.ns - ends) // self.order
        self.rows, self.n = (self.nt - 1) * self.ns, self.nt * self.ns
        self._h = C.c_void_p()
        lib = _cabi.load()
        _cabi.check(lib.gmrf_burgers_line_create(device, C.c_void_p(stream), self.cells, nt, float(dt), float(nu), self.order,
                                                 self.SCHEMES[scheme], self.BCS[bc], self.length, C.byref(self._h)))
        self._read_pattern()

    def _read_pattern(self):
        """nnz and `pattern` of the created handle (rows and n are set)."""
        lib = _cabi.load()
        nnz = C.c_int64(0)
        _cabi.check(lib.gmrf_burgers_p1_pattern(self._h, C.byref(nnz), None, None, 0))
        self.nnz = int(nnz.value)
        rp, ci = np.empty(self.rows + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        _cabi.check(lib.gmrf_burgers_p1_pattern(self._h, None, _cabi.ptr(rp), _cabi.ptr(ci), 0))
        self.pattern = sp.csr_matrix((np.ones(self.nnz), ci, rp), shape=(self.rows, self.n))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_burgers_p1_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def tangent(self, w):
        """w: (nt ns,) linearisation point (NumPy array or torch CUDA tensor).  Returns (J values in `pattern.data`
        order, residual f(w)), same kind as the input."""
        if _is_torch(w):
            import torch
            wv = w.contiguous()
            vals = torch.empty(self.nnz, dtype=torch.float64, device=wv.device)
            f = torch.empty(self.rows, dtype=torch.float64, device=wv.device)
        else:
            wv = np.ascontiguousarray(w, dtype=np.float64)
            vals, f = np.empty(self.nnz), np.empty(self.rows)
        if wv.ndim != 1 or wv.shape[0] != self.n:
            raise ValueError(f"w must have {self.n} entries")
        _cabi.check(_cabi.load().gmrf_burgers_p1_tangent(self._h, _cabi.ptr(wv), _cabi.ptr(vals), _cabi.ptr(f)))
        return vals, f

    def tangent_batch(self, W):
        """W: (B, nt ns) linearisation points -> (J values (B, nnz), residuals (B, rows)), same kind as the input; row p is
        `tangent(W[p])`, bit for bit."""
        if _is_torch(W):
            import torch
            wv = W.contiguous()
            if wv.dtype != torch.float64:
                raise TypeError("float64 required")
        else:
            wv = np.ascontiguousarray(W, dtype=np.float64)
        if wv.ndim != 2 or wv.shape[1] != self.n:
            raise ValueError(f"W must have shape (B, {self.n})")
        B = wv.shape[0]
        vals, f = PosteriorAssembler._like2(wv, (B, self.nnz)), PosteriorAssembler._like2(wv, (B, self.rows))
        _cabi.check(_cabi.load().gmrf_burgers_p1_tangent_batch(self._h, B, _cabi.ptr(wv), _cabi.ptr(vals), _cabi.ptr(f)))
        return vals, f


class BurgersCollocationTangent(BurgersP1Tangent):
    """Residual and tangent of the implicit-Euler Burgers step evaluated at collocation points on the periodic quadratic line, on
    the device: `f_and_J` of the reference's scripts/burgers/solve_burgers_gmrf-collocation.jl:186-192 with `J_static` (:183) and
    the operators `A_coll`, du/dx, d2u/dx2 of :167-169.  nc cells of length / nc, ns = 2 nc dofs numbered by position; `points`
    are npts coordinates in [0, length), in any order.  Row (t-1) npts + c (t = 1 .. nt-1) is point c of the step t-1 -> t:
        f = u - u_prev + dt u u_x - dt nu u_xx,    J[., t-1] = -a,    J[., t] = a + dt (u_x a + u d) - dt nu s
    with a, d, s the values and derivatives of the three shape functions of the point's cell.  `pattern` is the CSR matrix (values 1,
    (nt-1) npts x nt ns, 6 entries per row, zeros stored) whose `.data` order `tangent()` / `tangent_batch()` fill.  A
    `BurgersP1Tangent` to `PosteriorAssembler` and `GaussNewtonBatch`.  device = -1: pattern only (no GPU needed).

    Gauss-Newton without damping on this residual -- the reference's algorithm -- does not converge on coarse meshes at the
    nu = 0.01 / pi and T = 1 of the FEM loop's tests."""

    def __init__(self, nc: int, nt: int, dt: float, nu: float, points, length: float = 1.0, device: int = 0, stream: int = 0):
        self.cells, self.nt, self.dt, self.nu, self.length = int(nc), int(nt), float(dt), float(nu), float(length)
        self.ns, self.order, self.scheme, self.bc = 2 * self.cells, 2, "collocation", "periodic"
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1).copy()
        self.npts = int(self.points.shape[0])
        self.rows, self.n = (self.nt - 1) * self.npts, self.nt * self.ns
        self._h = C.c_void_p()
        _cabi.check(_cabi.load().gmrf_burgers_colloc_create(device, C.c_void_p(stream), self.cells, self.nt, self.dt, self.nu,
                                                            self.length, self.npts, _cabi.ptr(self.points), C.byref(self._h)))
        self._read_pattern()


class BurgersP1Prior:
    """Prior of the Burgers space-time GMRF with the initial condition conditioned in, for a batch of problems on the device: the
    "Prior" stage (`form_prior`, /root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:86-107) and the information vector of
    the "Initial condition" stage (:161) of the data-set loop, as `workloads.burgers(ns, nt, ic_noise, 0.0, ic)` states them
    (`workloads.burgers_prior_from_bulk`).  Every problem has its own values through bulk = mean(ic), on ONE structural pattern:
    `pattern` is the CSC matrix (values 1; symmetric, nt blocks of ns, offsets 0, +-1, +-2 in the diagonal blocks and 0, +-1 beside
    them) whose `.data` order `values_batch` fills.  An entry whose value is 0.0 is stored, SciPy prunes such entries: compare
    matrices, not `.data` arrays.  The other lines of `BurgersP1Tangent` -- quadratic, dirichlet, any length -- have their prior in
    `BurgersLinePrior`.  device = -1: pattern only (no GPU needed)."""

    def __init__(self, ns: int, nt: int, dt: float, nu: float, ic_noise: float = 1e8, device: int = 0, stream: int = 0):
        self.ns, self.nt, self.dt, self.nu, self.ic_noise = int(ns), int(nt), float(dt), float(nu), float(ic_noise)
        self.n = self.ns * self.nt
        self._h = C.c_void_p()
        lib = _cabi.load()
        _cabi.check(lib.gmrf_burgers_prior_create(device, C.c_void_p(stream), ns, nt, float(dt), float(nu), float(ic_noise), C.byref(self._h)))
        nnz = C.c_int64(0)
        _cabi.check(lib.gmrf_burgers_prior_pattern(self._h, C.byref(nnz), None, None, 0))
        self.nnz = int(nnz.value)
        cp, rv = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        _cabi.check(lib.gmrf_burgers_prior_pattern(self._h, None, _cabi.ptr(cp), _cabi.ptr(rv), 0))
        self.pattern = sp.csc_matrix((np.ones(self.nnz), rv, cp), shape=(self.n, self.n))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_burgers_prior_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _ics(self, ics):
        if _is_torch(ics):
            import torch
            v = ics.contiguous()
            if v.dtype != torch.float64:
                raise TypeError("float64 required")
        else:
            v = np.ascontiguousarray(ics, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != self.ns:
            raise ValueError(f"ics must have shape (B, {self.ns})")
        return v

    def values_batch(self, ics):
        """ics (B, ns) initial conditions -> {"bulk": (B,), "q_values": (B, nnz), "Qx_prior": (B, n)}, same kind as the input
        (NumPy or torch CUDA).  Problem p's bits do not depend on B or on its place in the batch; the values are bitwise symmetric."""
        v = self._ics(ics)
        B = v.shape[0]
        like2 = PosteriorAssembler._like2
        out = {"bulk": like2(v, (B,)), "q_values": like2(v, (B, self.nnz)), "Qx_prior": like2(v, (B, self.n))}
        _cabi.check(_cabi.load().gmrf_burgers_prior_values_batch(self._h, B, _cabi.ptr(v), _cabi.ptr(out["bulk"]), _cabi.ptr(out["q_values"]),
                                                                 _cabi.ptr(out["Qx_prior"])))
        return out


class BurgersLinePrior(BurgersP1Prior):
    """`BurgersP1Prior` on every line `BurgersP1Tangent` serves: nc cells of length / nc, order 1 or 2, bc = "periodic" (ns =
    order nc dofs) or "dirichlet" (ns = order nc + 1, `pin` added on the diagonal of dofs 0 and ns - 1 of every slice) -- the
    periodic quadratic line the reference's `form_prior` runs on (/root/reference/scripts/burgers/solve_burgers_gmrf-fem.jl:71-72,
    :86-107) and the interval of _research/burgers_chen24.jl, as `workloads.burgers_line_prior_from_bulk` states the prior.
    ic_obs = "all": the initial condition is observed at every dof of slice 0 that is not pinned; "vertices" (order 2): at the even
    ones of them, one point per cell; bulk is the mean of ic over the observed dofs (ics stay (B, ns)).  `pattern` holds the offsets
    0 .. +-2 order in the diagonal blocks and 0 .. +-order beside them, wrapped (periodic) or clipped (dirichlet).  `.pattern`,
    `.values_batch` and `BurgersInitialConditionBatch` as for `BurgersP1Prior`; (order 1, periodic, length 1) is that prior
    evaluated by other kernels (gmrf_burgers_line_prior_create).  device = -1: pattern only."""

    IC_OBS = {"all": 0, "vertices": 1}

    def __init__(self, nc: int, nt: int, dt: float, nu: float, order: int = 2, bc: str = "periodic", length: float = 1.0,
                 ic_noise: float = 1e8, pin: float = 1e8, ic_obs: str = "all", device: int = 0, stream: int = 0):
        if bc not in BurgersP1Tangent.BCS or ic_obs not in self.IC_OBS:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"BurgersLinePrior: bc {bc!r} {tuple(BurgersP1Tangent.BCS)}, ic_obs {ic_obs!r} "
                                                 f"{tuple(self.IC_OBS)}")
        self.nc, self.nt, self.dt, self.nu, self.ic_noise = int(nc), int(nt), float(dt), float(nu), float(ic_noise)
        self.order, self.bc, self.length, self.pin, self.ic_obs = int(order), bc, float(length), float(pin), ic_obs
        self.ns = self.order * self.nc + (1 if bc == "dirichlet" else 0)
        self.n = self.ns * self.nt
        self._h = C.c_void_p()
        lib = _cabi.load()
        _cabi.check(lib.gmrf_burgers_line_prior_create(device, C.c_void_p(stream), self.nc, self.nt, self.dt, self.nu, self.ic_noise,
                                                       self.order, BurgersP1Tangent.BCS[bc], self.length, self.pin, self.IC_OBS[ic_obs],
                                                       C.byref(self._h)))
        nnz = C.c_int64(0)
        _cabi.check(lib.gmrf_burgers_prior_pattern(self._h, C.byref(nnz), None, None, 0))
        self.nnz = int(nnz.value)
        cp, rv = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        _cabi.check(lib.gmrf_burgers_prior_pattern(self._h, None, _cabi.ptr(cp), _cabi.ptr(rv), 0))
        self.pattern = sp.csc_matrix((np.ones(self.nnz), rv, cp), shape=(self.n, self.n))


class EllipticP1Tangent:
    """Tangent, residual and load of the nonlinear elliptic benchmark -Lap u + u^3 = f_src on the device:
    `f_and_J` of /root/reference/_research/elliptic_chen24.jl:280-285 with `assemble_J_cube` (:231-278) and the stiffness
    rows and load of `assemble_J_diff_and_f` (:179-228), on the structured P1 triangle mesh of `DarcyP1Assembler` (nx x ny
    nodes, x fastest, quads cut by the diagonal n00 - n11) with the symmetric 3-point rule.  The rows of the nodes on the four
    sides stay zero, columns are kept.  `pattern` is the CSR matrix (values 1) whose `.data` order `tangent()` fills --
    exactly `DarcyP1Assembler(nx, ny).pattern`, the `J` of `PosteriorAssembler`; `qpoints` (cells, 3, 2) are the quadrature
    points at which the caller evaluates its source.  The residual does not contain the load: `load(src_q)` goes to
    `GaussNewtonBatch.run` as `y`.  device = -1: pattern and quadrature points only (no GPU needed).

    order = 2: the reference's default element (`element_order = 2` of `gmrf_fem_solve`, :118-122), `Lagrange{RefTriangle,2}` under
    `QuadratureRule{RefTriangle}(3)` on the lattice of `DarcyP1Assembler(nx, ny, order=2)`: n = (2 nx - 1)(2 ny - 1) dofs (vertices
    and edge midpoints, x fastest), `pattern` exactly that assembler's, `nq` = 4 quadrature points per cell, `qpoints` (cells, 4, 2)
    and `load` of (cells, 4); prescribed rows are the lattice points on the four sides (gmrf_elliptic_p2_create)."""

    def __init__(self, nx: int, ny: int, device: int = 0, stream: int = 0, order: int = 1):
        if order not in (1, 2):
            raise ValueError("order must be 1 or 2")
        self.nx, self.ny, self.order = int(nx), int(ny), int(order)
        self.n = (2 * self.nx - 1) * (2 * self.ny - 1) if self.order == 2 else self.nx * self.ny
        self.nq = 4 if self.order == 2 else 3
        self.rows = self.n
        self.cells = 2 * (self.nx - 1) * (self.ny - 1)
        self._h = C.c_void_p()
        lib = _cabi.load()
        create = lib.gmrf_elliptic_p2_create if self.order == 2 else lib.gmrf_elliptic_p1_create
        _cabi.check(create(device, C.c_void_p(stream), nx, ny, C.byref(self._h)))
        nnz = C.c_int64(0)
        _cabi.check(lib.gmrf_elliptic_p1_pattern(self._h, C.byref(nnz), None, None, 0))
        self.nnz = int(nnz.value)
        rp, ci = np.empty(self.n + 1, dtype=np.int64), np.empty(self.nnz, dtype=np.int64)
        _cabi.check(lib.gmrf_elliptic_p1_pattern(self._h, None, _cabi.ptr(rp), _cabi.ptr(ci), 0))
        self.pattern = sp.csr_matrix((np.ones(self.nnz), ci, rp), shape=(self.n, self.n))
        self.qpoints = np.empty((self.cells, self.nq, 2), dtype=np.float64)
        _cabi.check(lib.gmrf_elliptic_p1_qpoints(self._h, _cabi.ptr(self.qpoints)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_elliptic_p1_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def _f64(a):
        if _is_torch(a):
            import torch
            if a.dtype != torch.float64:
                raise TypeError("float64 required")
            return a.contiguous()
        return np.ascontiguousarray(a, dtype=np.float64)

    def tangent(self, w):
        """w: (n,) linearisation point (NumPy array or torch CUDA tensor).  Returns (J values in `pattern.data`
        order, residual f(w) without the load), same kind as the input."""
        wv = self._f64(w)
        if wv.ndim != 1 or wv.shape[0] != self.n:
            raise ValueError(f"w must have {self.n} entries")
        vals, f = PosteriorAssembler._like2(wv, (self.nnz,)), PosteriorAssembler._like2(wv, (self.n,))
        _cabi.check(_cabi.load().gmrf_elliptic_p1_tangent(self._h, _cabi.ptr(wv), _cabi.ptr(vals), _cabi.ptr(f)))
        return vals, f

    def tangent_batch(self, W):
        """W: (B, n) linearisation points -> (J values (B, nnz), residuals (B, n)), same kind as the input; row p is
        `tangent(W[p])`, bit for bit."""
        wv = self._f64(W)
        if wv.ndim != 2 or wv.shape[1] != self.n:
            raise ValueError(f"W must have shape (B, {self.n})")
        B = wv.shape[0]
        vals, f = PosteriorAssembler._like2(wv, (B, self.nnz)), PosteriorAssembler._like2(wv, (B, self.n))
        _cabi.check(_cabi.load().gmrf_elliptic_p1_tangent_batch(self._h, B, _cabi.ptr(wv), _cabi.ptr(vals), _cabi.ptr(f)))
        return vals, f

    def load(self, src_q):
        """src_q: (cells, nq) or (B, cells, nq) values of the source at `qpoints` -> b (n,) or (B, n), b[i] = int phi_i f_src, same
        kind as the input; row p of a batch is `load(src_q[p])`, bit for bit."""
        sv = self._f64(src_q)
        if sv.ndim not in (2, 3) or tuple(sv.shape[-2:]) != (self.cells, self.nq):
            raise ValueError(f"src_q must have shape ({self.cells}, {self.nq}) or (B, {self.cells}, {self.nq})")
        B = sv.shape[0] if sv.ndim == 3 else 1
        b = PosteriorAssembler._like2(sv, (B, self.n) if sv.ndim == 3 else (self.n,))
        _cabi.check(_cabi.load().gmrf_elliptic_p1_load(self._h, B, _cabi.ptr(sv), _cabi.ptr(b)))
        return b


class ShallowWaterP1:
    """Element kernels of the linear shallow-water SPDE on the device (third piece):
    `assemble_system!` of /root/reference/src/spdes/shallow_water.jl:17-122 (coupling K, element-lumped mass M, stiffness S
    of the three fields h, u, v) and the per-step operators of `discretize` (:170-217), on the structured P1 triangle mesh
    (nx x ny nodes, x fastest, quads cut by the diagonal n00 - n11; dof = 3 * node + field; symmetric 3-point quadrature).
    `pattern_K` / `pattern_S` are CSR matrices (values 1) whose `.data` order `assemble()` / `operators()` fill;
    `qpoints` (cells, 3, 2) are the quadrature points at which the caller evaluates its H(x).  device = -1: patterns and
    quadrature points only (no GPU needed)."""

    def __init__(self, nx: int, ny: int, device: int = 0, stream: int = 0):
        self.nx, self.ny, self.nn, self.n = int(nx), int(ny), int(nx) * int(ny), 3 * int(nx) * int(ny)
        self.cells = 2 * (self.nx - 1) * (self.ny - 1)
        self._h = C.c_void_p()
        lib = _cabi.load()
        _cabi.check(lib.gmrf_shallow_water_p1_create(device, C.c_void_p(stream), nx, ny, C.byref(self._h)))
        pats = []
        for which in (0, 1):
            nnz = C.c_int64(0)
            _cabi.check(lib.gmrf_shallow_water_p1_pattern(self._h, which, C.byref(nnz), None, None, 0))
            rp, ci = np.empty(self.n + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int64)
            _cabi.check(lib.gmrf_shallow_water_p1_pattern(self._h, which, None, _cabi.ptr(rp), _cabi.ptr(ci), 0))
            pats.append(sp.csr_matrix((np.ones(nnz.value), ci, rp), shape=(self.n, self.n)))
        self.pattern_K, self.pattern_S = pats
        self.qpoints = np.empty((self.cells, 3, 2), dtype=np.float64)
        _cabi.check(lib.gmrf_shallow_water_p1_qpoints(self._h, _cabi.ptr(self.qpoints)))

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _cabi.load().gmrf_shallow_water_p1_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    @staticmethod
    def _mask(prescribed, n):
        if prescribed is None:
            return None
        if _is_torch(prescribed):
            import torch
            m = prescribed.to(torch.uint8).contiguous()
            if m.numel() != n:
                raise ValueError(f"prescribed: expected {n} entries")
            return m
        m = np.ascontiguousarray(np.asarray(prescribed) != 0, dtype=np.uint8)
        if m.size != n:
            raise ValueError(f"prescribed: expected {n} entries")
        return m

    def _out(self, ref, count):
        if _is_torch(ref):
            import torch
            return torch.empty(count, dtype=torch.float64, device=ref.device)
        return np.empty(count, dtype=np.float64)

    def assemble(self, H_q, k: float = 0.0, f: float = 0.0, g: float = 9.81, prescribed=None):
        """H_q: (cells, 3) values of H at `qpoints` (NumPy array or torch CUDA tensor).  Returns (K values, lumped M, S values),
        same kind as H_q, with `apply!` of the prescribed dofs done."""
        hq = H_q.contiguous() if _is_torch(H_q) else np.ascontiguousarray(H_q, dtype=np.float64)
        if (hq.numel() if _is_torch(hq) else hq.size) != self.cells * 3:
            raise ValueError(f"H_q must have {self.cells} x 3 entries")
        kv, ml, sv = self._out(hq, self.pattern_K.nnz), self._out(hq, self.n), self._out(hq, self.pattern_S.nnz)
        m = self._mask(prescribed, self.n)
        _cabi.check(_cabi.load().gmrf_shallow_water_p1_assemble(self._h, _cabi.ptr(hq), float(k), float(f), float(g), _cabi.ptr(m),
                                                                _cabi.ptr(kv), _cabi.ptr(ml), _cabi.ptr(sv)))
        return kv, ml, sv

    def operators(self, K_vals, M_lumped, S_vals, prescribed=None, kappa_matern: float = 1.0, tau: float = 1.0, dt: float = 1.0):
        """The operators of one time step (`discretize`, :170-217): dict with G_dt (values in pattern_K: M~ + dt K, constraints
        applied), J (values in pattern_S: sqrt(ratio) M~^-1/2 (kappa^2 M~ + G); Q_matern = J'J), M_tilde, beta."""
        g_v, j_v = self._out(K_vals, self.pattern_K.nnz), self._out(K_vals, self.pattern_S.nnz)
        mt, be = self._out(K_vals, self.n), self._out(K_vals, self.n)
        m = self._mask(prescribed, self.n)
        _cabi.check(_cabi.load().gmrf_shallow_water_p1_operators(self._h, _cabi.ptr(K_vals), _cabi.ptr(M_lumped), _cabi.ptr(S_vals),
                                                                 _cabi.ptr(m), float(kappa_matern), float(tau), float(dt),
                                                                 _cabi.ptr(g_v), _cabi.ptr(j_v), _cabi.ptr(mt), _cabi.ptr(be)))
        return {"G_dt": g_v, "J": j_v, "M_tilde": mt, "beta": be}


def gn_step(F: "TridiagonalCholeskyFactor", asm: PosteriorAssembler, q_values, Qx_prior, j_values, x, obs_diff,
            noise: float):
    """One Gauss-Newton step of scripts/solve_burger.jl:143-149 with everything resident on the
    device: assemble A = Q + noise J'J and the right-hand side, re-factor on the analysed pattern
    (`F` must have been factored once on `asm.pattern`), solve."""
    a_vals = asm.precision(q_values, j_values, noise)
    rhs = asm.rhs(Qx_prior, j_values, x, obs_diff, noise)
    F.refactor(a_vals)
    return ldiv(F, rhs)


class GaussNewtonBatch:
    """The Burgers data-set loop (scripts/burgers/solve_burgers_gmrf-fem.jl:154-233, loop body scripts/solve_burger.jl:143-180)
    for `F.batch` problems on one mesh in lock step, resident on the device (gmrf_gn_run): per iteration
    tangent -> A = Q + noise J'J, rhs -> refactor -> solve -> objective -> stop rule, and one status word crosses the bus.

    `F` (reference order, factored once on `asm.pattern`), `asm` and `tangent` must have been created on the same device with
    the same `stream` argument.  A problem is active while |last - cur| / |cur| > rtol and steps < max_steps; one that has
    stopped is frozen and stays in the batch.

    With an `EllipticP1Tangent` the same loop is the Gauss-Newton loop of _research/elliptic_chen24.jl:142-166: pass the load
    `tangent.load(src_q)` as `y` and noise = 3e13.  The stop rule stays the relative objective change (the reference's Newton
    decrement lives in a package that is not available).

    With a `BurgersP1Tangent(..., scheme="cn", bc="dirichlet")` it is the loop of _research/burgers_chen24.jl:139-152 on the
    problems of `workloads.burgers_chen24_batch` (zero observations; the same stop rule).

    With a `BurgersCollocationTangent` it is the loop of scripts/burgers/solve_burgers_gmrf-collocation.jl:236-246 on the problems
    of `workloads.burgers_collocation_batch` (zero observations, noise = 1e8; the same stop rule)."""

    def __init__(self, F: "TridiagonalCholeskyFactor", asm: PosteriorAssembler, tangent: "BurgersP1Tangent | EllipticP1Tangent"):
        self.F, self.asm, self.tangent = F, asm, tangent          # (kept alive: the library holds their handles)
        self._h = C.c_void_p()
        lib = _cabi.load()
        if isinstance(tangent, EllipticP1Tangent):
            create = lib.gmrf_gn_create_elliptic
        elif isinstance(tangent, BurgersP1Tangent):
            create = lib.gmrf_gn_create
        else:
            raise TypeError("tangent must be a BurgersP1Tangent or an EllipticP1Tangent")
        _cabi.check(create(F._h, asm._h, tangent._h, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _cabi.load().gmrf_gn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, q_values, Qx_prior, x_prior, x0, y=None, noise: float = 1e8, rtol: float = 1e-4, max_steps: int = 20):
        """q_values (nnz_q,) shared or (B, nnz_q); Qx_prior, x_prior, x0 (B, n); y (B, m) or None (zero observations).  NumPy
        arrays or torch CUDA tensors.  Returns (x (B, n), same kind as x0; steps (B,) int32 NumPy; objective history
        (B, max_steps + 1) NumPy, slot 0 at the start point, NaN in the slots no step reached).  The defaults are the
        reference's (scripts/solve_burger.jl:140, :171)."""
        B, a = self.F.batch, self.asm
        if x0.ndim != 2 or x0.shape[0] != B:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"x0: expected ({B}, {a.n}), the batch of the handle")
        q, stride = a._q(q_values, B)
        qx, xp, yv = a._mat(Qx_prior, B, a.n, "Qx_prior"), a._mat(x_prior, B, a.n, "x_prior"), a._mat(y, B, a.m, "y")
        x = a._mat(x0, B, a.n, "x0")
        x = x.clone() if _is_torch(x) else x.copy()
        steps = np.zeros(B, dtype=np.int32)
        hist = np.full((B, int(max_steps) + 1), np.nan)
        info = C.c_int32(0)
        st = _cabi.load().gmrf_gn_run(self._h, _cabi.ptr(q), stride, _cabi.ptr(qx), _cabi.ptr(xp), _cabi.ptr(x), _cabi.ptr(yv),
                                      float(noise), float(rtol), int(max_steps), _cabi.ptr(steps), _cabi.ptr(hist), C.byref(info))
        self.last = (x, steps, hist)                  # (after NotPositiveDefinite: the last complete iterates)
        _cabi.check(st, info.value)
        return x, steps, hist

    def finalize(self):
        """Tangent at the final x, assemble, re-factor: `F` then holds the factor of Q + noise J(x)' J(x) of every problem
        (x_final of solve_burgers_gmrf-fem.jl:184-193) for posterior_batch / sample_batch / marginal_var / logdet."""
        info = C.c_int32(0)
        _cabi.check(_cabi.load().gmrf_gn_finalize(self._h, C.byref(info)), info.value)
        return self.F

    _VAR = {None: -1, "none": -1, "exact": _cabi.VAR_EXACT, "rbmc": _cabi.VAR_RBMC, "mc": _cabi.VAR_MC}

    def posterior(self, z=None, first: int = 0, k_samples: int = 1, var="rbmc", k_var: int = 50, sample_seed: int = 0x5EED,
                  var_seed: int = 0x5EED, out=None):
        """Everything `solve_problem` returns for the final iterate of the last `run`, in ONE call on the device
        (gmrf_gn_posterior): `finalize()`, then k_samples samples x + L^-T z (ids of `sample_batch`), the marginal standard
        deviations by `var` ("rbmc" = the reference's RBMCStrategy(k_var), "mc", "exact" or None; problem p draws the ids
        p k_var + s) and their norms, logdet, and -- with z (B, n), the reference solution's dofs -- sqmahal(x, z), nll and
        (rel_err, rmse, max_err) of x against z over the elements [first, n) (first = ns: the scripts' [2:end, :]).  Each piece
        is bitwise the public call (`sample_batch`, `marginal_var`, `logdet_batch`, `quadform_batch`, `solution_errors_batch`).
        The result's arrays are torch tensors on the device when z -- or, without z, the last run's x -- is one, NumPy
        otherwise.  `out`: a GaussNewtonPosterior of arrays to fill instead of new ones (`x` is not written); after
        NotPositiveDefinite they are unchanged."""
        B, a = self.F.batch, self.asm
        if var not in self._VAR:
            raise ValueError('var must be "rbmc", "mc", "exact" or None')
        method = self._VAR[var]
        k_samples = int(k_samples)
        zv = a._mat(z, B, a.n, "z")
        x_last = self.last[0] if getattr(self, "last", None) is not None else None
        ref = zv if zv is not None else (x_last if x_last is not None else np.empty(0))
        shapes = (("samples", (B, k_samples, a.n) if k_samples > 0 else None), ("std", (B, a.n) if method >= 0 else None),
                  ("std_norm", (B,) if method >= 0 else None), ("logdet", (B,)), ("sqmahal", (B,) if zv is not None else None),
                  ("nll", (B,) if zv is not None else None), ("errors", (B, 3) if zv is not None else None))
        if out is None:
            like2 = PosteriorAssembler._like2
            out = GaussNewtonPosterior(x_last, **{name: (like2(ref, shape) if shape is not None else None) for name, shape in shapes})
        else:
            for name, shape in shapes:
                arr = getattr(out, name)
                if arr is None:
                    continue
                if shape is None:
                    raise ValueError(f"out.{name} given, but this call does not produce it")
                ok = tuple(arr.shape) == shape and (arr.is_contiguous() and str(arr.dtype) == "torch.float64" if _is_torch(arr)
                                                    else isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.dtype == np.float64)
                if not ok:
                    raise ValueError(f"out.{name} must be a contiguous float64 array of shape {shape}")
        info = C.c_int32(0)
        st = _cabi.load().gmrf_gn_posterior(self._h, _cabi.ptr(zv), int(first), k_samples, int(sample_seed), method, int(k_var),
                                            int(var_seed), _cabi.ptr(out.samples), _cabi.ptr(out.std), _cabi.ptr(out.std_norm),
                                            _cabi.ptr(out.logdet), _cabi.ptr(out.sqmahal), _cabi.ptr(out.nll), _cabi.ptr(out.errors),
                                            C.byref(info))
        _cabi.check(st, info.value)
        return out


class GaussNewtonPosterior:
    """What `GaussNewtonBatch.posterior` returns: x (B, n), the final iterate of the run; samples (B, k_samples, n) or None; std
    (B, n) and std_norm (B,) or None (var=None); logdet (B,); sqmahal (B,), nll (B,) and errors (B, 3) = (rel_err, rmse, max_err),
    or None without z."""
    __slots__ = ("x", "samples", "std", "std_norm", "logdet", "sqmahal", "nll", "errors")

    def __init__(self, x=None, samples=None, std=None, std_norm=None, logdet=None, sqmahal=None, nll=None, errors=None):
        self.x, self.samples, self.std, self.std_norm = x, samples, std, std_norm
        self.logdet, self.sqmahal, self.nll, self.errors = logdet, sqmahal, nll, errors


class DarcyConditioningResult:
    """What `DarcyConditioningBatch.run` returns: mean (B, n), samples (B, k_samples, n) or None, std (B, n) and std_norm (B,)
    or None (var=None)."""
    __slots__ = ("mean", "samples", "std", "std_norm")

    def __init__(self, mean, samples, std, std_norm):
        self.mean, self.samples, self.std, self.std_norm = mean, samples, std, std_norm


class DarcyConditioningBatch:
    """The Darcy data-set loop (scripts/darcy/solve_darcy_gmrf-fem.jl:176-198) for `F.batch` problems on one mesh in ONE call,
    resident on the device (gmrf_dc_run): coefficient tables -> A, y -> Q + q_eps A'A and the information vector -> refactor ->
    mean and samples -> marginal standard deviations and their norms.

    `F` (reference order, factored once on `asm.pattern`), `asm` (built on `darcy.pattern`) and `darcy` must have been created on
    the same device with the same `stream` argument."""

    _VAR = {None: -1, "none": -1, "exact": _cabi.VAR_EXACT, "rbmc": _cabi.VAR_RBMC, "mc": _cabi.VAR_MC}

    def __init__(self, F: "TridiagonalCholeskyFactor", asm: PosteriorAssembler, darcy: DarcyP1Assembler):
        self.F, self.asm, self.darcy = F, asm, darcy              # (kept alive: the library holds their handles)
        self._h = C.c_void_p()
        _cabi.check(_cabi.load().gmrf_dc_create(F._h, asm._h, darcy._h, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _cabi.load().gmrf_dc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, tables, q_values, Q_mu=None, q_eps: float = 1e8, beta: float = 1.0, k_samples: int = 1, var="rbmc",
            k_var: int = 50, sample_seed: int = 0x5EED, var_seed: int = 0x5EED, out=None):
        """tables (B, ng, ng); q_values (nnz_q,) shared or (B, nnz_q); Q_mu (B, n) = Q mu or None (zero prior mean).  NumPy arrays
        or torch CUDA tensors; the result's arrays are torch tensors on the device when `tables` is one, NumPy otherwise.
        var: "rbmc" (the reference's RBMCStrategy(k_var)), "mc", "exact" or None.  Problem p's samples carry the ids
        p k_samples + s (`posterior_batch`), its variance draws p k_var + s (`marginal_var` of a batch).  The defaults are the
        reference's (:163, :174).  `out`: a DarcyConditioningResult of arrays to fill instead of new ones; after
        NotPositiveDefinite they are unchanged."""
        B, a = self.F.batch, self.asm
        if var not in self._VAR:
            raise ValueError('var must be "rbmc", "mc", "exact" or None')
        method = self._VAR[var]
        if _is_torch(tables):
            import torch
            tab = tables.contiguous()
            if tab.dtype != torch.float64:
                raise TypeError("float64 required")
        else:
            tab = np.ascontiguousarray(tables, dtype=np.float64)
        if tab.ndim != 3 or tab.shape[0] != B or tab.shape[1] != tab.shape[2]:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"tables: expected ({B}, ng, ng), the batch of the handle")
        q, stride = a._q(q_values, B)
        qm = a._mat(Q_mu, B, a.n, "Q_mu")
        k_samples = int(k_samples)
        if out is None:
            like2 = PosteriorAssembler._like2
            out = DarcyConditioningResult(like2(tab, (B, a.n)), like2(tab, (B, k_samples, a.n)) if k_samples > 0 else None,
                                          like2(tab, (B, a.n)) if method >= 0 else None, like2(tab, (B,)) if method >= 0 else None)
        else:
            for name, arr, shape in (("mean", out.mean, (B, a.n)), ("samples", out.samples, (B, k_samples, a.n) if k_samples > 0 else None),
                                     ("std", out.std, (B, a.n) if method >= 0 else None), ("std_norm", out.std_norm, (B,) if method >= 0 else None)):
                if arr is None:
                    continue
                if shape is None:
                    raise ValueError(f"out.{name} given, but this run does not produce it")
                ok = tuple(arr.shape) == shape and (arr.is_contiguous() and str(arr.dtype) == "torch.float64" if _is_torch(arr)
                                                    else isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.dtype == np.float64)
                if not ok:
                    raise ValueError(f"out.{name} must be a contiguous float64 array of shape {shape}")
        info = C.c_int32(0)
        st = _cabi.load().gmrf_dc_run(self._h, _cabi.ptr(tab), tab.shape[1], float(beta), _cabi.ptr(q), stride, _cabi.ptr(qm),
                                      float(q_eps), k_samples, int(sample_seed), method, int(k_var), int(var_seed),
                                      _cabi.ptr(out.mean), _cabi.ptr(out.samples), _cabi.ptr(out.std), _cabi.ptr(out.std_norm),
                                      C.byref(info))
        _cabi.check(st, info.value)
        return out


class BurgersInitialConditionBatch:
    """The "Prior" and "Initial condition" stages of the Burgers data-set loop (scripts/burgers/solve_burgers_gmrf-fem.jl:154-179) for
    `F.batch` problems in ONE call, resident on the device (gmrf_bic_run): initial conditions -> bulk, the prior's values and
    information vector -> refactor -> x_ic = mean(x_ic), on the handle and the analysis `GaussNewtonBatch` uses afterwards:

        x_ic, q, qx, _ = ic_stage.run(ics)
        x, steps, hist = gn.run(q, qx, x_ic, x_ic)      # prior mean and start = mean(x_ic); Q_ic mean(x_ic) = qx
        post = gn.posterior(z=soln_dofs, first=ns)      # samples, std, logdet, sqmahal, nll, errors (or F = gn.finalize() and the calls)

    `F` (reference order, factored once on `asm.pattern`), `asm` (built on `prior.pattern` and the tangent's pattern) and `prior`
    (a `BurgersP1Prior` or a `BurgersLinePrior`, with the `BurgersP1Tangent` of the same line in `asm`) must have been created on the same device with the same `stream` argument."""

    def __init__(self, F: "TridiagonalCholeskyFactor", asm: PosteriorAssembler, prior: BurgersP1Prior):
        self.F, self.asm, self.prior = F, asm, prior              # (kept alive: the library holds their handles)
        self._h = C.c_void_p()
        _cabi.check(_cabi.load().gmrf_bic_create(F._h, asm._h, prior._h, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _cabi.load().gmrf_bic_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, ics):
        """ics (B, ns), NumPy or torch CUDA -> (x_ic (B, n), q_values (B, nnz_q), Qx_prior (B, n), bulk (B,)) of the same kind.
        NotPositiveDefinite carries the failing block in `.info`."""
        B, a = self.F.batch, self.asm
        v = self.prior._ics(ics)
        if v.shape[0] != B:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"ics: expected ({B}, {self.prior.ns}), the batch of the handle")
        like2 = PosteriorAssembler._like2
        x_ic, q, qx, bulk = like2(v, (B, a.n)), like2(v, (B, a.nnz_q)), like2(v, (B, a.n)), like2(v, (B,))
        info = C.c_int32(0)
        st = _cabi.load().gmrf_bic_run(self._h, _cabi.ptr(v), _cabi.ptr(x_ic), _cabi.ptr(q), _cabi.ptr(qx), _cabi.ptr(bulk), C.byref(info))
        _cabi.check(st, info.value)
        return x_ic, q, qx, bulk


def solution_errors_batch(pred, soln, first: int = 0, device: int = 0) -> np.ndarray:
    """(B, 3) NumPy array of (rel_err, rmse, max_err) per problem (/root/reference/src/metrics.jl:3-13; `workloads.solution_errors`
    on the host) of pred against soln, both (B, n) NumPy arrays or torch CUDA tensors, over the elements [first, n): first = ns
    leaves the first time slice out as the scripts' [2:end, :] does.  Computed on the device with fixed-shape sums: the same bits
    on every call and for every B."""
    def prep(a):
        if _is_torch(a):
            import torch
            if a.dtype != torch.float64:
                raise TypeError("float64 required")
            return a.contiguous()
        return np.ascontiguousarray(a, dtype=np.float64)
    p, s = prep(pred), prep(soln)
    if p.ndim != 2 or tuple(p.shape) != tuple(s.shape):
        raise ValueError("pred and soln must have one shape (B, n)")
    stream = 0
    for a in (p, s):
        if _is_torch(a) and a.is_cuda:
            import torch
            device, stream = a.device.index, torch.cuda.current_stream(a.device).cuda_stream
    out = np.empty((p.shape[0], 3), dtype=np.float64)
    _cabi.check(_cabi.load().gmrf_field_errors_batch(int(device), C.c_void_p(stream), p.shape[0], p.shape[1], int(first), _cabi.ptr(p),
                                                     _cabi.ptr(s), _cabi.ptr(out)))
    return out


class FieldEvaluator:
    """FEM fields at the points of a data grid, on the device: `E = evaluation_matrix(disc, pred_coords)` of the data-set loops
    (scripts/darcy/solve_darcy_gmrf-fem.jl:82-89, scripts/burgers/solve_burgers_gmrf-fem.jl:75-83), `pred = E * mean` and its
    `rel_err`, `rmse`, `max_err` against the data set's solution -- the last line of those loops:

        ev = FieldEvaluator.triangles(nx, ny, workloads.darcy_pred_coords(xs, ys), order=2)
        errors = ev.errors(DarcyConditioningBatch(F, asm, darcy).run(tables, q).mean, truth)              # (B, 3)
        ev = FieldEvaluator.line(nc, workloads.burgers_pred_coords(xs))
        errors = ev.errors(gn.posterior().x, truth, nt=nt, first_slice=1)                                # the scripts' [2:end, :]
        std = ev.variance(F, nt, std=True); cal = ev.calibration(F, mean, truth, nt)     # error bars and calibration at the points

    The rows of E are computed once at creation, on the host, in double precision (include/gmrf_hip.h states the rules); `points`
    are host coordinates in any order.  Every value is ONE rounding sequence, w0 f[i0] then fma(wk, f[ik], .) in ascending dof
    index: the same bits in every batch and on every call.  The calls run on the handle's stream (`stream`, or one of its own)
    and return synchronised; a tensor that torch is still writing on another stream must be complete before it is passed, as for
    the other handles.  device = -1: `rows()` and `matrix()` only (no GPU needed)."""

    def __init__(self, handle: C.c_void_p, npts: int):
        self._h, self.npts = handle, int(npts)
        ns, width = C.c_int64(0), C.c_int64(0)
        _cabi.check(_cabi.load().gmrf_eval_rows(self._h, C.byref(ns), C.byref(width), None, None))
        self.ns, self.width = int(ns.value), int(width.value)

    @classmethod
    def line(cls, nc: int, points, order: int = 2, bc: str = "periodic", length: float = 1.0, device: int = 0, stream: int = 0):
        """The lines of `BurgersP1Tangent`: nc cells of length / nc, order 1 or 2, bc "periodic" (points in [0, length)) or
        "dirichlet" (points in [0, length])."""
        if bc not in BurgersP1Tangent.BCS:
            raise GmrfError(_cabi.ERR_BAD_SHAPE, f"FieldEvaluator.line: bc {bc!r} {tuple(BurgersP1Tangent.BCS)}")
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        h = C.c_void_p()
        _cabi.check(_cabi.load().gmrf_eval_line_create(int(device), C.c_void_p(stream), int(nc), int(order), BurgersP1Tangent.BCS[bc],
                                                       float(length), pts.shape[0], _cabi.ptr(pts), C.byref(h)))
        return cls(h, pts.shape[0])

    @classmethod
    def triangles(cls, nx: int, ny: int, xy, order: int = 1, device: int = 0, stream: int = 0):
        """The triangle meshes of `DarcyP1Assembler` / `EllipticP1Tangent` / `ShallowWaterP1`: nx x ny vertices on the unit
        square, order 1 (vertex dofs) or 2 (the (2 nx - 1) x (2 ny - 1) lattice); xy (npts, 2) in [0, 1]^2."""
        pts = np.ascontiguousarray(xy, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("xy must have shape (npts, 2)")
        h = C.c_void_p()
        _cabi.check(_cabi.load().gmrf_eval_tri_create(int(device), C.c_void_p(stream), int(nx), int(ny), int(order), pts.shape[0],
                                                      _cabi.ptr(pts), C.byref(h)))
        return cls(h, pts.shape[0])

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _cabi.load().gmrf_eval_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self) -> Tuple[np.ndarray, np.ndarray]:
        """(idx (npts, width) int64, w (npts, width)): the dofs of every point, ascending, and their weights (zeros stored)."""
        idx, w = np.empty((self.npts, self.width), dtype=np.int64), np.empty((self.npts, self.width))
        _cabi.check(_cabi.load().gmrf_eval_rows(self._h, None, None, _cabi.ptr(idx), _cabi.ptr(w)))
        return idx, w

    def matrix(self, nt: int = 1, slice: Optional[int] = None) -> sp.csr_matrix:
        """E as a SciPy CSR matrix built on the host from `rows()`, explicit zeros kept.  nt = 1: (npts, ns), the reference's
        `evaluation_matrix`; nt > 1: the space-time form (nt npts, nt ns) of `spatial_to_spatiotemporal`, slice t's points on slice
        t's dofs; slice = t: those npts rows alone, (npts, nt ns) -- slice = 0 is `A_ic`."""
        nt = int(nt)
        if nt < 1 or (slice is not None and not 0 <= int(slice) < nt):
            raise ValueError("nt >= 1 and 0 <= slice < nt")
        idx, w = self.rows()
        slices = np.arange(nt) if slice is None else np.array([int(slice)])
        cols = (idx[None, :, :] + self.ns * slices[:, None, None]).reshape(-1)
        rp = self.width * np.arange(slices.size * self.npts + 1, dtype=np.int64)
        return sp.csr_matrix((np.tile(w.reshape(-1), slices.size), cols, rp), shape=(slices.size * self.npts, nt * self.ns))

    @staticmethod
    def _prep(a, name: str):
        if _is_torch(a):
            import torch
            if a.dtype != torch.float64:
                raise TypeError("float64 required")
            if not a.is_cuda:
                raise TypeError(f"{name}: a torch tensor must live on the device (pass NumPy for host data)")
            return a.contiguous()
        return np.ascontiguousarray(a, dtype=np.float64)

    def apply(self, fields):
        """fields (..., ns) -> (..., npts) of the same kind (NumPy array or torch CUDA tensor): every leading index is one spatial
        field -- means, samples, or the slices of space-time fields given as (..., nt, ns)."""
        f = self._prep(fields, "fields")
        if f.ndim < 1 or f.shape[-1] != self.ns:
            raise ValueError(f"fields must have a last axis of {self.ns} dofs")
        lead = tuple(f.shape[:-1])
        rows = int(np.prod(lead, dtype=np.int64))
        pred = PosteriorAssembler._like2(f, lead + (self.npts,))
        _cabi.check(_cabi.load().gmrf_eval_apply_batch(self._h, rows, _cabi.ptr(f), _cabi.ptr(pred)))
        return pred

    def errors(self, fields, truth, nt: int = 1, first_slice: int = 0, return_pred: bool = False):
        """(B, 3) NumPy array of (rel_err, rmse, max_err) per problem of E fields against truth over the slices [first_slice, nt):
        fields (B, nt ns) or (B, nt, ns), truth (B, nt npts) or (B, nt, npts), NumPy arrays or torch CUDA tensors.  Bitwise
        `solution_errors_batch(apply(fields), truth, first=first_slice * npts)`, in one pass that does not write pred.
        return_pred: also pred (B, nt npts), of the kind of `fields`, the bits of `apply`."""
        nt = int(nt)
        f, t = self._prep(fields, "fields"), self._prep(truth, "truth")
        if f.ndim < 2 or int(np.prod(f.shape[1:], dtype=np.int64)) != nt * self.ns:
            raise ValueError(f"fields must have shape (B, {nt} * {self.ns})")
        B = f.shape[0]
        if t.shape[0] != B or int(np.prod(t.shape[1:], dtype=np.int64)) != nt * self.npts:
            raise ValueError(f"truth must have shape ({B}, {nt} * {self.npts})")
        out = np.empty((B, 3), dtype=np.float64)
        pred = PosteriorAssembler._like2(f, (B, nt * self.npts)) if return_pred else None
        _cabi.check(_cabi.load().gmrf_eval_errors_batch(self._h, B, nt, int(first_slice), _cabi.ptr(f), _cabi.ptr(t), _cabi.ptr(out),
                                                        _cabi.ptr(pred)))
        return (out, pred) if return_pred else out

    def pairs(self) -> Tuple[sp.csr_matrix, np.ndarray]:
        """(P, pos): the pair table of the pointwise variance (gmrf_eval_pairs; no GPU needed).  P (ns, ns) is the pattern --
        symmetric, both triangles, sorted, values 1.0 -- of exactly the dof pairs some point uses, with the diagonal of every dof
        used; pos (width (width + 1) / 2, npts) int32 holds for point c and the pair a >= b of its row, at a (a + 1) / 2 + b, the
        place of the entry (idx[c, a], idx[c, b]) in P's CSR order."""
        lib, nnz = _cabi.load(), C.c_int64(0)
        _cabi.check(lib.gmrf_eval_pairs(self._h, C.byref(nnz), None, None, None))
        rp, ci = np.empty(self.ns + 1, dtype=np.int64), np.empty(int(nnz.value), dtype=np.int64)
        pos = np.empty((self.width * (self.width + 1) // 2, self.npts), dtype=np.int32)
        _cabi.check(lib.gmrf_eval_pairs(self._h, None, _cabi.ptr(rp), _cabi.ptr(ci), _cabi.ptr(pos)))
        return sp.csr_matrix((np.ones(ci.size), ci, rp), shape=(self.ns, self.ns)), pos

    def pair_pattern(self, nt: int = 1) -> sp.csr_matrix:
        """I_nt (x) P as a sorted SciPy CSR matrix (nt ns, nt ns): the entries of Sigma that `variance` reads for a field of nt
        slices, slice t on the dofs t ns .. (t + 1) ns - 1 as in `matrix(nt)`; the entry of `pairs()`'s pos sits at t nnz(P) + pos."""
        if int(nt) < 1:
            raise ValueError("nt >= 1")
        K = sp.kron(sp.identity(int(nt), format="csr"), self.pairs()[0], format="csr")
        K.sort_indices()
        return K

    def variance(self, F, nt: int = 1, out=None, std: bool = False):
        """The pointwise predictive variance diag(E Sigma E^T) at the points, (batch, nt, npts), for the batch that the
        `TridiagonalCholeskyFactor` F holds factored (F.N == nt * ns), exactly: the selected inverse on `pair_pattern(nt)` never
        leaves the device and every value is ONE rounding sequence (gmrf_eval_var_batch), the same bits in every batch and on
        every call.  `out`: a contiguous float64 array of that shape to fill -- NumPy, or a torch tensor on the device; default a
        new NumPy array.  std=True: sqrt(max(v, 0)) in place of v.  F's pattern rule applies to the pairs (`selected_inverse`):
        same or neighbouring block, the later index below rmax -- true for the pairs of the mesh F's matrix was assembled on."""
        out = TridiagonalCholeskyFactor._out_array(out, (F.batch, int(nt), self.npts))
        _cabi.check(_cabi.load().gmrf_eval_var_batch(self._h, F._h, int(nt), _cabi.ptr(out)))
        if std:
            if _is_torch(out):
                out.clamp_(min=0.0).sqrt_()
            else:
                np.sqrt(np.maximum(out, 0.0, out=out), out=out)
        return out

    def calibration(self, F, fields, truth, nt: int = 1, first_slice: int = 0, zcrit: float = 1.96, return_pred: bool = False,
                    return_var: bool = False):
        """(B, 4) NumPy array of (mean z^2, coverage, mean log predictive density, min variance) per problem over the slices
        [first_slice, nt): z = (E fields - truth) / sqrt(v) with v of `variance(F, nt)`, coverage the share of points with
        |z| <= zcrit, the density's term -(log(2 pi v) + z^2) / 2.  fields (B, nt ns) or (B, nt, ns) -- the prediction's dofs, e.g.
        the posterior means of the batch F factors -- and truth (B, nt npts) or (B, nt, npts): NumPy arrays or torch CUDA
        tensors.  The same bits on every call.  A point with v <= 0 makes the first three inf or nan and shows in the fourth: look
        at it first.  return_pred / return_var: also pred / the variances (B, nt npts), of the kind of `fields`, the bits of
        `apply` / `variance`."""
        nt = int(nt)
        f, t = self._prep(fields, "fields"), self._prep(truth, "truth")
        if f.ndim < 2 or int(np.prod(f.shape[1:], dtype=np.int64)) != nt * self.ns:
            raise ValueError(f"fields must have shape (B, {nt} * {self.ns})")
        B = f.shape[0]
        if t.shape[0] != B or int(np.prod(t.shape[1:], dtype=np.int64)) != nt * self.npts:
            raise ValueError(f"truth must have shape ({B}, {nt} * {self.npts})")
        out = np.empty((B, 4), dtype=np.float64)
        pred = PosteriorAssembler._like2(f, (B, nt * self.npts)) if return_pred else None
        var = PosteriorAssembler._like2(f, (B, nt * self.npts)) if return_var else None
        _cabi.check(_cabi.load().gmrf_eval_calibration_batch(self._h, F._h, B, nt, int(first_slice), float(zcrit), _cabi.ptr(f),
                                                             _cabi.ptr(t), _cabi.ptr(out), _cabi.ptr(pred), _cabi.ptr(var)))
        extra = tuple(a for a, want in ((pred, return_pred), (var, return_var)) if want)
        return (out,) + extra if extra else out


class ConditionedGMRF:
    """What `condition_on_observations(x, A, Q_eps, y; solver_blueprint)` returns in the reference's
    problem loop (scripts/darcy/solve_darcy_gmrf-fem.jl:176-192), served by the block-tridiagonal
    path: posterior precision Q + Q_eps A'A (assembled on the device), then `mean`, `rand`, `std`,
    `logdet`.  One object per sparsity pattern; `update(a_values, y)` re-conditions on a new
    observation matrix with the same pattern (the next problem of the data set) -- values only."""

    def __init__(self, Q, mu, A, q_eps: float, y, n_blocks: int, device: int = 0):
        Q = sp.csc_matrix(Q); Q.sort_indices()
        A = sp.csr_matrix(A); A.sort_indices()
        self.Q, self.q_eps, self.n_blocks = Q, float(q_eps), int(n_blocks)
        self.mu = np.zeros(Q.shape[0]) if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
        self._qmu = Q @ self.mu
        self.asm = PosteriorAssembler(Q, A, device=device)
        self.F = TridiagonalCholeskyFactor(device=device)
        self._analysed = False
        self.update(A.data, y)

    def update(self, a_values, y):
        """Re-condition with new values of A (same pattern) and new observations y."""
        self._vals = np.asarray(self.asm.precision(self.Q.data, a_values, self.q_eps))
        if not self._analysed:
            self.F.factor(self.precision_matrix(), self.n_blocks)      # symbolic analysis + first factor
            self._analysed = True
        else:
            self.F.refactor(self._vals)
        # information vector Q mu + Q_eps A' y  (gmrf_assemble_rhs with x = 0, obs_diff = y)
        self._rhs = self.asm.rhs(self._qmu, a_values, np.zeros(self.asm.n), y, self.q_eps)
        self._mean = None
        self._csr = None
        return self

    def precision_matrix(self):
        """Posterior precision as a SciPy CSC matrix (`to_matrix(precision_map(x_cond))`)."""
        P = self.asm.pattern.copy()
        P.data = self._vals.copy()
        return P

    def mean(self):
        if self._mean is None:
            self._mean = ldiv(self.F, self._rhs)
        return self._mean

    def rand(self, k: int = 1, seed: int = 0x5EED, first_id: int = 0):
        """n x k samples  mean + L^-T z  with device Philox normals (`rand(rng, x_cond)`)."""
        return self.F.sample(k, mean=self.mean(), seed=seed, first_id=first_id)

    def var(self, method: str = "exact", k: int = 50, seed: int = 0x5EED):
        """Marginal variances: "exact" selected inversion, or "rbmc" = the reference's RBMCStrategy(k)."""
        if method == "exact":
            return self.F.marginal_var("exact")
        if self._csr is None:
            self._csr = CsrMatrix(self.precision_matrix())
        return self.F.marginal_var(method, k=k, seed=seed, Q=self._csr)

    def std(self, method: str = "exact", k: int = 50, seed: int = 0x5EED):
        return np.sqrt(self.var(method, k, seed))

    def logdet(self) -> float:
        return self.F.logdet()

    def selected_inverse(self):
        """Q_post^-1 on the pattern of Q_post (scipy.sparse.csr_matrix): the covariances of every pair of coupled dofs, with
        the marginal variances on its diagonal."""
        if self._csr is None:
            self._csr = CsrMatrix(self.precision_matrix())
        return self.F.selected_inverse(self._csr)

    def sqmahal(self, z) -> float:
        """`sqmahal(x_cond, z)` = (z - mean)' Q_post (z - mean) (scripts/burgers/solve_burgers_gmrf-collocation.jl:262):
        one CSR SpMV of the posterior precision (K6) and a dot product."""
        if self._csr is None:
            self._csr = CsrMatrix(self.precision_matrix())
        d = np.ascontiguousarray(np.asarray(z, dtype=np.float64) - np.asarray(self.mean()))
        return float(d @ np.asarray(self._csr @ d))

    def nll(self, z) -> float:
        """Negative log-likelihood of z under the conditioned GMRF, `nll_soln` of the same script (:213-215):
        0.5 (n log 2 pi + sqmahal + logdet Sigma), logdet Sigma = -logdet Q_post = -2 sum log diag L (:208-211)."""
        n = self.asm.n
        return 0.5 * (n * np.log(2.0 * np.pi) + self.sqmahal(z) - self.logdet())


def condition_on_observations(Q, mu, A, q_eps: float, y, n_blocks: int, device: int = 0) -> ConditionedGMRF:
    """Python twin of the reference's `condition_on_observations(x, A, Q_eps, y)` for a GMRF
    N(mu, Q^-1) whose posterior precision is block tridiagonal with `n_blocks` blocks."""
    return ConditionedGMRF(Q, mu, A, q_eps, y, n_blocks, device)


class _LazyBlocks(Sequence):
    """`F.chos` / `F.Cs`: dense blocks copied from the device on access."""

    def __init__(self, owner: "TridiagonalCholeskyFactor", kind: int, count: int):
        self._o, self._kind, self._count = owner, kind, count

    def __len__(self):
        return self._count

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._count))]
        if i < 0:
            i += self._count
        if not 0 <= i < self._count:
            raise IndexError(i)
        return self._o.get_block(self._kind, i)


class TridiagonalCholeskyFactor:
    """Handle wrapper of the device-resident factor (struct at src/tridiagonal_cholesky.jl:5-9).

    `N` is the total size n (as in the reference, NOT the block count); `chos[i]` is the
    lower-triangular L_i, `Cs[i]` = L_{i+1,i}.

    order = "twisted" (one problem): Q = T T^T, two chains that run at the same time and meet in block `meet`
    (0-based; None = automatic).  `ldiv`, the marginal variances and `logdet` do not depend on the order; `chos[i]` is then
    L_i (i <= meet) or the upper-triangular U_i, `Cs[i]` is G_{i+1} (i < meet) or H_i = T[i, i+1], the half-solves are
    T^-1 b / T^-T b and a sample with a given z is mean + T^-T z (gmrf_bt_set_order).
    """

    def __init__(self, device: int = 0, stream: int = 0, batch: int = 1, order: str = "reference", meet: Optional[int] = None):
        self._h = C.c_void_p()
        self._lib = _cabi.load()
        _cabi.check(self._lib.gmrf_bt_create(device, C.c_void_p(stream), C.byref(self._h)))
        self.batch = 1
        if batch != 1:
            self.set_batch(batch)
        if order != "reference" or meet is not None:
            self.set_order(order, meet)
        self.N = 0
        self.n_blocks = 0
        self.block_size = 0
        self.device = device
        self._pattern = None

    # -- life cycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmrf_bt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- batch of independent problems on one sparsity pattern
    def set_batch(self, batch: int):
        _cabi.check(self._lib.gmrf_bt_set_batch(self._h, int(batch)))
        self.batch = int(batch)

    def set_order(self, order: str, meet: Optional[int] = None):
        """Elimination order "reference" or "twisted" (meeting block `meet`, None = automatic); drops the current factor."""
        o = {"reference": _cabi.ORDER_REFERENCE, "twisted": _cabi.ORDER_TWISTED}.get(order)
        if o is None:
            raise ValueError('order must be "reference" or "twisted"')
        _cabi.check(self._lib.gmrf_bt_set_order(self._h, o, -1 if meet is None else int(meet)))

    @property
    def order(self) -> str:
        o, m = C.c_int32(0), C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_get_order(self._h, C.byref(o), C.byref(m)))
        return "twisted" if o.value == _cabi.ORDER_TWISTED else "reference"

    @property
    def meet(self) -> int:
        """The meeting block (0-based): resolved by the last factorisation; n_blocks - 1 for the reference order."""
        o, m = C.c_int32(0), C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_get_order(self._h, C.byref(o), C.byref(m)))
        return m.value

    def half_stats(self, half: int) -> dict:
        """stats() of one half of a twisted factor (0: blocks 0 .. meet, 1: blocks N-1 .. meet+1)."""
        s = _cabi.Stats()
        _cabi.check(self._lib.gmrf_bt_half_stats(self._h, int(half), C.byref(s)))
        return {f: (list(getattr(s, f)) if hasattr(getattr(s, f), "__len__") else getattr(s, f)) for f, _ in s._fields_}

    def select_problem(self, p: int):
        _cabi.check(self._lib.gmrf_bt_select_problem(self._h, int(p)))

    def solve_batch(self, b, mode: int = _cabi.SOLVE_FULL):
        """b: (B, k, n) C-contiguous NumPy array / torch CUDA tensor (each right-hand side
        contiguous) -> same shape.  Problem p is solved with factor p."""
        B, k, n = b.shape
        if B != self.batch or n != self.N:
            raise ValueError("expected shape (batch, k, n)")
        if _is_torch(b):
            import torch
            b = b.contiguous()
            out = torch.empty_like(b)
        else:
            b = np.ascontiguousarray(b, dtype=np.float64)
            out = np.empty_like(b)
        _cabi.check(self._lib.gmrf_bt_solve(self._h, _cabi.ptr(b), _cabi.ptr(out), k, n, n, mode))
        return out

    def sample_batch(self, k: int, mean=None, seed: int = 0x5EED, first_id: int = 0, like=None):
        """(B, k, n) samples: problem p, sample s = mean[p] + L_p^-T z(id = first_id + p*k + s)."""
        B, n = self.batch, self.N
        ref = like if like is not None else mean
        if _is_torch(ref):
            import torch
            out = torch.empty((B, k, n), dtype=torch.float64, device=ref.device)
            if mean is not None:
                mean = mean.contiguous()
        else:
            out = np.empty((B, k, n), dtype=np.float64)
            if mean is not None:
                mean = np.ascontiguousarray(mean, dtype=np.float64)
        _cabi.check(self._lib.gmrf_bt_sample(self._h, seed, first_id, k, _cabi.ptr(mean), None, _cabi.ptr(out), n))
        return out

    # -- factorisation
    def factor(self, A, N_blocks: int, values=None):
        """`values`: (batch, nnz) array of CSC values for a batch of problems on the pattern of A."""
        A = sp.csc_matrix(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError("matrix must be square")
        if not A.has_sorted_indices:
            A = A.copy()
            A.sort_indices()
        n = A.shape[0]
        colptr = A.indptr.astype(np.int64)
        rowval = A.indices.astype(np.int64)
        nz = np.ascontiguousarray(A.data if values is None else values, dtype=np.float64)
        if nz.size != self.batch * A.nnz:
            raise ValueError("values must hold batch * nnz entries")
        info = C.c_int32(0)
        st = self._lib.gmrf_bt_factor_csc(self._h, n, int(N_blocks), _cabi.ptr(colptr), _cabi.ptr(rowval),
                                          _cabi.ptr(nz), 0, C.byref(info))
        _cabi.check(st, info.value)
        self._set_shape(n, int(N_blocks))
        self._pattern = (colptr, rowval)
        return self

    def factor_blocks(self, diag_blocks, off_diag_blocks):
        """Factor from the output of `extract_blocks` (lists of sparse bs x bs blocks)."""
        nb = len(diag_blocks)
        bs = diag_blocks[0].shape[0]
        keep = []

        def mk(blocks):
            arr = (_cabi.SparseBlock * max(len(blocks), 1))()
            for i, b in enumerate(blocks):
                b = sp.csc_matrix(b)
                b.sort_indices()
                p = b.indptr.astype(np.int64); ix = b.indices.astype(np.int64); v = b.data.astype(np.float64)
                keep.extend([p, ix, v])
                arr[i].nnz = b.nnz
                arr[i].ptr = p.ctypes.data; arr[i].idx = ix.ctypes.data; arr[i].val = v.ctypes.data
            return arr

        d = mk(diag_blocks)
        lo = mk(off_diag_blocks)
        info = C.c_int32(0)
        st = self._lib.gmrf_bt_factor_blocks(self._h, nb * bs, nb, C.cast(d, C.c_void_p), C.cast(lo, C.c_void_p),
                                             0, 1, C.byref(info))
        _cabi.check(st, info.value)
        self._set_shape(nb * bs, nb)
        return self

    def refactor(self, nzval):
        """New values on the sparsity pattern of the last `factor` (nzval in CSC order;
        NumPy array or torch CUDA tensor)."""
        info = C.c_int32(0)
        if not _is_torch(nzval):
            nzval = np.ascontiguousarray(nzval, dtype=np.float64)
        st = self._lib.gmrf_bt_refactor_values(self._h, _cabi.ptr(nzval), C.byref(info))
        _cabi.check(st, info.value)
        return self

    def _set_shape(self, n, nb):
        self.N = n
        self.n_blocks = nb
        self.block_size = n // nb
        self.chos = _LazyBlocks(self, _cabi.BLOCK_L, nb)
        self.Cs = _LazyBlocks(self, _cabi.BLOCK_C, nb - 1)
        self.inverses = _LazyBlocks(self, _cabi.BLOCK_LINV, nb)

    # -- solves
    def _solve(self, b, mode: int, out=None):
        xa, k, ld, one_d = _colmajor(b, self.N)
        if out is None:
            store, view = _alloc_like(xa, self.N, k, one_d)
        else:
            store, view = out, out
        _cabi.check(self._lib.gmrf_bt_solve(self._h, _cabi.ptr(xa), _cabi.ptr(store), k, ld, self.N, mode))
        return view

    def get_block(self, kind: int, i: int) -> np.ndarray:
        bs = self.block_size
        out = np.empty((bs, bs), dtype=np.float64, order="F")
        _cabi.check(self._lib.gmrf_bt_get_block(self._h, kind, i, _cabi.ptr(out), bs))
        return out

    def logdet(self) -> float:
        v = C.c_double(0.0)
        _cabi.check(self._lib.gmrf_bt_logdet(self._h, C.byref(v)))
        return v.value

    def logdet_batch(self, out=None):
        """(B,) logdet of every problem in one call (gmrf_bt_logdet_batch): entry p is bitwise `logdet()` after
        `select_problem(p)`.  `out`: a contiguous float64 array of B values to fill -- NumPy, or a torch tensor on the handle's
        device; default: a new NumPy array."""
        out = self._out_array(out, (self.batch,))
        _cabi.check(self._lib.gmrf_bt_logdet_batch(self._h, _cabi.ptr(out)))
        return out

    def normals(self, k: int, seed: int = 0x5EED, first_id: int = 0, like=None):
        if self.batch != 1:
            raise ValueError("a batched handle draws (batch, k, n) normals: normals_batch")
        store, view = _alloc_like(like if like is not None else np.empty(0), self.N, k, False)
        _cabi.check(self._lib.gmrf_bt_normals(self._h, seed, first_id, k, _cabi.ptr(store), self.N))
        return view

    def normals_batch(self, k: int, seed: int = 0x5EED, first_id: int = 0):
        """(B, k, n) host array of the N(0,1) draws `sample_batch(k, seed=, first_id=)` and the batched variance
        estimators use: problem p, draw s = Philox id first_id + p*k + s."""
        out = np.empty((self.batch, k, self.N), dtype=np.float64)
        _cabi.check(self._lib.gmrf_bt_normals(self._h, seed, first_id, k, _cabi.ptr(out), self.N))
        return out

    def sample(self, k: int, mean=None, z=None, seed: int = 0x5EED, first_id: int = 0, like=None):
        """k posterior samples mean + L^-T z as an n x k matrix (rand(rng, x_cond))."""
        ref = like if like is not None else (z if z is not None else (mean if mean is not None else np.empty(0)))
        za = None
        if z is not None:
            za, kz, _, _ = _colmajor(z, self.N)
            k = kz
        if mean is not None and not _is_torch(mean):
            mean = np.ascontiguousarray(mean, dtype=np.float64)
        store, view = _alloc_like(ref if _is_torch(ref) else np.empty(0), self.N, k, False)
        _cabi.check(self._lib.gmrf_bt_sample(self._h, seed, first_id, k, _cabi.ptr(mean), _cabi.ptr(za),
                                             _cabi.ptr(store), self.N))
        return view

    def posterior(self, b, k: int, seed: int = 0x5EED, first_id: int = 0):
        """(mean, samples) = (A^-1 b, mean + L^-T z) in ONE call (mean(x_cond) and rand(rng, x_cond) of the reference's script,
        scripts/darcy/solve_darcy_gmrf-fem.jl:190-191): bitwise `ldiv(F, b)` and `F.sample(k, mean=...)`; on device tensors the
        samples' sweep runs beside the mean's two where this handle's sweeps are persistent launches (gmrf_bt_posterior).
        One problem (batch == 1); b: n values; samples come back n x k like `sample`."""
        if self.batch != 1:
            raise ValueError("posterior(): one problem per handle (use solve_batch / sample_batch for batches)")
        xa, kb, ld, one_d = _colmajor(b, self.N)
        if kb != 1:
            raise ValueError("posterior(): one right-hand side")
        mstore, mview = _alloc_like(xa, self.N, 1, True)
        sstore, sview = _alloc_like(xa, self.N, k, False)
        _cabi.check(self._lib.gmrf_bt_posterior(self._h, _cabi.ptr(xa), seed, first_id, k, _cabi.ptr(mstore), _cabi.ptr(sstore),
                                                self.N))
        return mview, sview

    def posterior_batch(self, b, k: int, seed: int = 0x5EED, first_id: int = 0):
        """(mean, samples) of a batch in ONE call (gmrf_bt_posterior): b (B, 1, n) or (B, n) torch CUDA tensor -> mean (B, n),
        samples (B, k, n) with the sample ids of `sample_batch` (problem p, sample s: first_id + p*k + s).  Where the samples'
        sweep runs on the GEMM (k <= 128, padded to a multiple of 64, enough tiles) and no output overlaps an input, the mean's
        backward sweep is the tail row of the samples' (one pass over the factor; samples' L^-T z bitwise `sample_batch`, the mean
        at rounding level of `solve_batch`); else the call is `solve_batch` + `sample_batch`.  `set_eager(Switch.TWO_CALL_POSTERIOR)` keeps the latter."""
        import torch
        B, n = self.batch, self.N
        b = b.reshape(B, n).contiguous()
        mean = torch.empty((B, n), dtype=torch.float64, device=b.device)
        out = torch.empty((B, k, n), dtype=torch.float64, device=b.device)
        _cabi.check(self._lib.gmrf_bt_posterior(self._h, _cabi.ptr(b), seed, first_id, k, _cabi.ptr(mean), _cabi.ptr(out), n))
        return mean, out

    def set_factor_rhs(self, b):
        """Register the right-hand side of later `posterior_batch` calls (gmrf_bt_set_factor_rhs): b, a contiguous float64 torch
        CUDA tensor of B x n values, is READ AT FACTOR TIME -- a batch's factorisations then solve L y = b inside their own products,
        and `posterior_batch` with this same tensor skips its forward sweep.  None clears it."""
        if b is None:
            self._factor_rhs = None
            _cabi.check(self._lib.gmrf_bt_set_factor_rhs(self._h, None))
            return
        if not (_is_torch(b) and b.is_cuda and b.is_contiguous()) or (self.N and b.numel() != self.batch * self.N):
            raise ValueError("set_factor_rhs(): a contiguous device tensor of batch x n values")
        self._factor_rhs = b                     # (kept alive: the library holds its pointer)
        _cabi.check(self._lib.gmrf_bt_set_factor_rhs(self._h, _cabi.ptr(b)))

    def marginal_var(self, method: str = "exact", k: int = 50, seed: int = 0x5EED, Q: Optional[CsrMatrix] = None,
                     q_values=None, out=None):
        """diag(Q^-1).  "exact" (selected inversion), "rbmc" (the reference's RBMCStrategy(k); needs Q)
        or "mc".  A batch returns (batch, n); its sampled estimators take Q for the pattern and
        `q_values` (batch, nnz): every problem's values in Q's CSR order (for a symmetric matrix the
        nzval arrays the factor was given).  `out`: a contiguous float64 array of that shape to fill -- NumPy, or a
        torch tensor on the handle's device (the variances then never leave the device); default: a new NumPy array."""
        m = {"exact": _cabi.VAR_EXACT, "rbmc": _cabi.VAR_RBMC, "mc": _cabi.VAR_MC}[method]
        shape = (self.N,) if self.batch == 1 else (self.batch, self.N)
        if out is None:
            out = np.empty(shape, dtype=np.float64)
        else:
            ok = tuple(out.shape) == shape and (out.is_contiguous() and str(out.dtype) == "torch.float64" if _is_torch(out)
                                                else out.flags.c_contiguous and out.dtype == np.float64)
            if not ok:
                raise ValueError(f"out must be a contiguous float64 array of shape {shape}")
        if self.batch > 1 and m != _cabi.VAR_EXACT:
            qv = None
            if q_values is not None:
                qv = q_values.contiguous() if _is_torch(q_values) else np.ascontiguousarray(q_values, dtype=np.float64)
            _cabi.check(self._lib.gmrf_bt_marginal_var_batch(self._h, m, k, seed, Q._h if Q is not None else None,
                                                             _cabi.ptr(qv) if qv is not None else None, _cabi.ptr(out)))
            return out
        _cabi.check(self._lib.gmrf_bt_marginal_var(self._h, m, k, seed, Q._h if Q is not None else None,
                                                   _cabi.ptr(out)))
        return out

    def selected_inverse(self, S: CsrMatrix, out=None):
        """Entries of Sigma = Q^-1 at the stored positions of S (its values are ignored; gmrf_bt_selinv).  Every entry (r, c)
        lies in the same or a neighbouring block, and for a coupling entry the index in the later block is below the factored
        pattern's rmax: true for the factored matrix and any sub-pattern of it.  Batch 1: a scipy.sparse.csr_matrix with
        S's pattern; a batch: the (batch, nnz) values in S's CSR order.  `out`: a contiguous float64 array of that shape
        (batch 1: (nnz,)) to fill -- NumPy, or a torch tensor on the handle's device; it is then returned as it is."""
        shape = (S.nnz,) if self.batch == 1 else (self.batch, S.nnz)
        given = out is not None
        out = self._out_array(out, shape)
        _cabi.check(self._lib.gmrf_bt_selinv(self._h, S._h, _cabi.ptr(out)))
        if given or self.batch > 1:
            return out
        return sp.csr_matrix((out, S.indices.copy(), S.indptr.copy()), shape=S.shape)

    def trace_inv(self, S: CsrMatrix, dvals):
        """tr(Q^-1 dQ_j) = sum_e Sigma[e] dvals[j][e] for every row j of `dvals`, (m, nnz) or (batch, m, nnz): dQ_j on S's
        pattern, its values in S's CSR order (both triangles).  Returns (m,) or (batch, m), a NumPy array, or a device torch
        tensor when `dvals` is one.  Sigma stays on the device; the same call gives the same bits (gmrf_bt_trace_inv)."""
        nd = 2 if self.batch == 1 else 3
        if dvals.ndim != nd or dvals.shape[-1] != S.nnz or (nd == 3 and dvals.shape[0] != self.batch):
            want = "(m, nnz)" if nd == 2 else "(batch, m, nnz)"
            raise ValueError(f"dvals must be {want} with nnz = {S.nnz}")
        m = int(dvals.shape[-2])
        if _is_torch(dvals):
            import torch
            if dvals.dtype != torch.float64:
                raise TypeError("float64 required")
            dvals = dvals.contiguous()
            out = torch.empty(dvals.shape[:-1], dtype=torch.float64, device=dvals.device)
        else:
            dvals = np.ascontiguousarray(dvals, dtype=np.float64)
            out = np.empty(dvals.shape[:-1], dtype=np.float64)
        _cabi.check(self._lib.gmrf_bt_trace_inv(self._h, S._h, _cabi.ptr(dvals), m, _cabi.ptr(out)))
        return out

    @staticmethod
    def _out_array(out, shape):
        if out is None:
            return np.empty(shape, dtype=np.float64)
        ok = tuple(out.shape) == shape and (out.is_contiguous() and str(out.dtype) == "torch.float64" if _is_torch(out)
                                            else out.flags.c_contiguous and out.dtype == np.float64)
        if not ok:
            raise ValueError(f"out must be a contiguous float64 array of shape {shape}")
        return out

    def var_accumulate(self, acc, method: str, first_id: int, k: int, seed: int = 0x5EED,
                       Q: Optional[CsrMatrix] = None):
        m = {"rbmc": _cabi.VAR_RBMC, "mc": _cabi.VAR_MC}[method]
        _cabi.check(self._lib.gmrf_bt_var_accumulate(self._h, m, first_id, k, seed,
                                                     Q._h if Q is not None else None, _cabi.ptr(acc)))
        return acc

    def stats(self) -> dict:
        s = _cabi.Stats()
        _cabi.check(self._lib.gmrf_bt_stats(self._h, C.byref(s)))
        out = {}
        for f, _ in s._fields_:
            v = getattr(s, f)
            out[f] = list(v) if hasattr(v, "__len__") else v
        return out

    def gemm_shapes(self) -> list:
        """GEMM launches of the profiled steps by shape (test hook gmrf_test_gemm_shapes): list of dicts."""
        n = C.c_int64(0)
        _cabi.check(self._lib.gmrf_test_gemm_shapes(self._h, None, 0, C.byref(n)))
        buf = np.zeros((max(int(n.value), 1), 11))
        _cabi.check(self._lib.gmrf_test_gemm_shapes(self._h, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.shape[0], C.byref(n)))
        names = ("class", "M", "N", "K", "tri", "lower_only", "problems", "k_bounds")
        return [dict({k: int(r[i]) for i, k in enumerate(names)}, launches=int(r[8]), ms=float(r[9]), flops=float(r[10]))
                for r in buf[: int(n.value)]]

    def envelope(self):
        """The envelope bounds of the analysed pattern (test hook gmrf_test_envelope): (lo, hi, state), lo / hi int32 arrays
        [n_blocks][padded block size / 64] of in-block columns (None where the blocks are no multiple of 256), state 0 none,
        1 trivial for every panel, 2 in use."""
        n, state = C.c_int64(0), C.c_int32(0)
        _cabi.check(self._lib.gmrf_test_envelope(self._h, None, None, 0, C.byref(n), C.byref(state)))
        if n.value == 0:
            return None, None, int(state.value)
        lo, hi = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        _cabi.check(self._lib.gmrf_test_envelope(self._h, _cabi.ptr(lo), _cabi.ptr(hi), n.value, C.byref(n), C.byref(state)))
        return lo, hi, int(state.value)

    def set_profiling(self, level: int):
        _cabi.check(self._lib.gmrf_bt_set_profiling(self._h, level))

    def set_eager(self, switches: int = 0):
        """Select the handle's routes: the OR of any `Switch` members (0: every default route; True is `Switch.EAGER`)."""
        _cabi.check(self._lib.gmrf_bt_set_eager(self._h, int(switches)))

    def synchronize(self):
        _cabi.check(self._lib.gmrf_bt_synchronize(self._h))

    def factor_buffer(self, kind: int) -> Tuple[int, int]:
        p = C.c_void_p()
        nbytes = C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_factor_buffer(self._h, kind, C.byref(p), C.byref(nbytes)))
        return int(p.value or 0), int(nbytes.value)

    def export_factor(self) -> np.ndarray:
        """Flat host image (uint8) of the selected problem's factor: header + L, C, Linv blocks."""
        nbytes = C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_export_size(self._h, C.byref(nbytes)))
        buf = np.empty(nbytes.value, dtype=np.uint8)
        _cabi.check(self._lib.gmrf_bt_export_factor(self._h, _cabi.ptr(buf), nbytes.value))
        return buf

    def import_factor(self, image: np.ndarray):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        _cabi.check(self._lib.gmrf_bt_import_factor(self._h, _cabi.ptr(image), image.size))
        hdr = image[:64].view(np.int64)
        self._set_shape(int(hdr[2]), int(hdr[3]))
        return self

    def adopt_shape(self, n: int, n_blocks: int):
        _cabi.check(self._lib.gmrf_bt_adopt_shape(self._h, n, n_blocks))
        self._set_shape(n, n_blocks)

    def get_layout(self) -> np.ndarray:
        """Layout record of the stored factor: [cmin, rmax, n_row_tiles, kst..., split p of the block inverses (0: full)] (int64)."""
        cnt = C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_get_layout(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, dtype=np.int64)
        _cabi.check(self._lib.gmrf_bt_get_layout(self._h, _cabi.ptr(out), out.size, C.byref(cnt)))
        return out

    def adopt_layout(self, n: int, n_blocks: int, layout=None):
        """A rank that receives the factor: shape + the root's layout record, storage without factoring."""
        if layout is None:
            _cabi.check(self._lib.gmrf_bt_adopt_layout(self._h, n, n_blocks, None, 0))
        else:
            lay = np.ascontiguousarray(layout, dtype=np.int64)
            _cabi.check(self._lib.gmrf_bt_adopt_layout(self._h, n, n_blocks, _cabi.ptr(lay), lay.size))
        self._set_shape(n, n_blocks)

    def adopt_commit(self, l_blocks_valid: bool = False):
        _cabi.check(self._lib.gmrf_bt_adopt_commit(self._h, int(l_blocks_valid)))

    def set_keep_l(self, keep: bool):
        """keep = False: the blocks chos[i].L are not retained (sweeps, samples, variances and logdet do
        not need them): 1.6 -> 0.84 GB per darcy256 posterior; `F.chos` then raises."""
        _cabi.check(self._lib.gmrf_bt_set_keep_l(self._h, int(keep)))

    def block_range(self, kind: int, i0: int, i1: int):
        """(first element, element count, problem stride) of blocks [i0, i1) inside a factor buffer."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_block_range(self._h, kind, i0, i1, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def packed_size(self, i0: int, i1: int) -> int:
        """Doubles per problem of the packed transport image of blocks [i0, i1) (gmrf_bt_packed_size)."""
        v = C.c_int64(0)
        _cabi.check(self._lib.gmrf_bt_packed_size(self._h, i0, i1, C.byref(v)))
        return v.value

    def pack_blocks_async(self, i0: int, i1: int, dev_buf):
        """Blocks [i0, i1) of every problem -> dev_buf ((batch, packed_size) torch CUDA tensor), stream-ordered."""
        _cabi.check(self._lib.gmrf_bt_pack_blocks_async(self._h, i0, i1, _cabi.ptr(dev_buf)))

    def unpack_blocks_async(self, i0: int, i1: int, dev_buf):
        _cabi.check(self._lib.gmrf_bt_unpack_blocks_async(self._h, i0, i1, _cabi.ptr(dev_buf)))

    def factor_begin(self, A, N_blocks: int):
        A = sp.csc_matrix(A)
        n = A.shape[0]
        colptr = A.indptr.astype(np.int64); rowval = A.indices.astype(np.int64)
        nz = np.ascontiguousarray(A.data, dtype=np.float64)
        _cabi.check(self._lib.gmrf_bt_factor_begin_csc(self._h, n, int(N_blocks), _cabi.ptr(colptr),
                                                       _cabi.ptr(rowval), _cabi.ptr(nz), 0))
        self._set_shape(n, int(N_blocks))

    def factor_begin_values(self, nzval):
        """Start a pipelined re-factorisation on the analysed pattern (nzval host or device)."""
        if not _is_torch(nzval):
            nzval = np.ascontiguousarray(nzval, dtype=np.float64)
        _cabi.check(self._lib.gmrf_bt_factor_begin_csc(self._h, self.N, self.n_blocks, None, None,
                                                       _cabi.ptr(nzval), 0))

    def factor_step_async(self, i0: int, i1: int):
        _cabi.check(self._lib.gmrf_bt_factor_step_async(self._h, i0, i1))

    def factor_end(self):
        info = C.c_int32(0)
        st = self._lib.gmrf_bt_factor_end(self._h, C.byref(info))
        _cabi.check(st, info.value)


# ----------------------------------------------------------------------------- reference surface

def tridiagonal_cholesky(A, N_blocks: int, device: int = 0, stream: int = 0, order: str = "reference",
                         meet: Optional[int] = None) -> TridiagonalCholeskyFactor:
    """tridiagonal_cholesky(A::SparseMatrixCSC, N_blocks)  (src/tridiagonal_cholesky.jl:65-82).

    Raises NotPositiveDefinite (PosDefException) with the failing block index, ValueError
    when size(A,1) is not a multiple of N_blocks (the reference would silently mis-factor),
    GmrfError(ERR_BAND) when entries lie outside the block tri-band (the reference silently
    ignores them)."""
    n = A.shape[0]
    if N_blocks <= 0 or n % N_blocks != 0:
        raise ValueError("size(A,1) must be a positive multiple of N_blocks")
    return TridiagonalCholeskyFactor(device, stream, order=order, meet=meet).factor(A, N_blocks)


def forward_solve(L: TridiagonalCholeskyFactor, b):
    """y = L^-1 b  (src/tridiagonal_cholesky.jl:43-52); returns the flat vector/matrix."""
    return L._solve(b, _cabi.SOLVE_FORWARD)


def backward_solve(L: TridiagonalCholeskyFactor, b):
    """x = L^-T b  (src/tridiagonal_cholesky.jl:24-33)."""
    return L._solve(b, _cabi.SOLVE_BACKWARD)


def ldiv(L: TridiagonalCholeskyFactor, b):
    """ldiv(L, b) = A^-1 b  (src/tridiagonal_cholesky.jl:60-63)."""
    return L._solve(b, _cabi.SOLVE_FULL)


def ldiv_(y, L: TridiagonalCholeskyFactor, b):
    """ldiv!(y, L, b)  (src/tridiagonal_cholesky.jl:54-58): result written into y, which is
    returned.  y may alias b."""
    res = L._solve(b, _cabi.SOLVE_FULL)
    if _is_torch(y):
        y.copy_(res)
    else:
        y[...] = res
    return y


def make_chunks(X, n: int):
    """src/tridiagonal_cholesky.jl:11-14: n contiguous views, the last takes the remainder."""
    c = X.shape[0] // n
    return [X[c * k:(X.shape[0] if k == n - 1 else c * k + c)] for k in range(n)]


def extract_blocks(I, J, V, block_size: int):
    """scripts/solve_burger.jl:182-254 on 1-based COO triplets: (diag_blocks, off_diag_blocks),
    the lower off-diagonal convention, entries outside the tri-band dropped as the reference
    does.  Vectorised host code (no per-entry Python loop)."""
    I = np.asarray(I, dtype=np.int64) - 1
    J = np.asarray(J, dtype=np.int64) - 1
    V = np.asarray(V)
    if I.size == 0:
        return [], []
    bi, bj = I // block_size, J // block_size
    nb = int(bi.max()) + 1
    diag, off = [], []
    is_d = bi == bj
    is_o = bi == bj + 1
    order_d = np.flatnonzero(is_d)
    order_o = np.flatnonzero(is_o)
    for b in range(nb):
        sel = order_d[bi[order_d] == b]
        diag.append(sp.coo_matrix((V[sel], (I[sel] - b * block_size, J[sel] - b * block_size)),
                                  shape=(block_size, block_size)).tocsc())
        if b > 0:
            sel = order_o[bi[order_o] == b]
            off.append(sp.coo_matrix((V[sel], (I[sel] - b * block_size, J[sel] - (b - 1) * block_size)),
                                     shape=(block_size, block_size)).tocsc())
    return diag, off


def logdet(L: TridiagonalCholeskyFactor) -> float:
    return L.logdet()


class StreamSet:
    """n HIP streams on hardware queues of their own (gmrf_streams_create): one per handle that is driven side by side
    with others.  `.pointers` are hipStream_t values (pass as `stream=` to TridiagonalCholeskyFactor / CsrMatrix, or wrap
    with torch.cuda.ExternalStream); `.n_distinct` of them were measured to overlap pairwise."""

    def __init__(self, n: int, device: int = 0):
        import ctypes as C
        lib = _cabi.load()
        arr = (C.c_void_p * n)()
        nd = C.c_int32(0)
        _cabi.check(lib.gmrf_streams_create(device, n, arr, C.byref(nd)))
        self.device, self._arr, self._n = device, arr, n
        self.pointers = [int(arr[i] or 0) for i in range(n)]
        self.n_distinct = int(nd.value)

    def close(self):
        if self._arr is not None:
            _cabi.load().gmrf_streams_destroy(self.device, self._n, self._arr)
            self._arr, self.pointers = None, []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator of this process (one per GPU) through the C ABI -- what a Julia host uses to
    share a factor over xGMI (include/gmrf_hip.h, "multi-GPU").  `unique_id()` on rank 0, ship the
    128 bytes to the other ranks by any means, then `Comm(device, rank, world, id)` everywhere."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_char * 128)()
        _cabi.check(_cabi.load().gmrf_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    def __init__(self, device: int, rank: int, world: int, uid: bytes):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        self._lib = _cabi.load()
        buf = (C.c_char * 128).from_buffer_copy(uid)
        _cabi.check(self._lib.gmrf_comm_create(device, rank, world, C.cast(buf, C.c_void_p), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmrf_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bcast_host(self, arr: np.ndarray, root: int = 0) -> np.ndarray:
        """In-place broadcast of a small contiguous NumPy array."""
        _cabi.check(self._lib.gmrf_comm_bcast_host(self._h, _cabi.ptr(arr), arr.nbytes, root))
        return arr

    def bcast_blocks_async(self, F: TridiagonalCholeskyFactor, i0: int, i1: int, root: int = 0, with_l: bool = False):
        _cabi.check(self._lib.gmrf_bt_bcast_blocks_async(F._h, self._h, root, i0, i1, int(with_l)))

    def allgather_blocks_async(self, F_own: TridiagonalCholeskyFactor, F_all: TridiagonalCholeskyFactor, i0: int, i1: int):
        """Blocks [i0, i1) of every rank's share `F_own` (batch b) -> `F_all` (batch world * b) on every rank
        (gmrf_bt_allgather_blocks_async: pack, ncclAllGather, unpack on the communicator's stream)."""
        _cabi.check(self._lib.gmrf_bt_allgather_blocks_async(F_own._h, F_all._h, self._h, i0, i1))

    def wait(self, F: TridiagonalCholeskyFactor):
        _cabi.check(self._lib.gmrf_comm_wait(F._h, self._h))

    def bytes_moved(self, reset: bool = False) -> float:
        """Factor bytes broadcast through this communicator so far."""
        v = C.c_double(0.0)
        _cabi.check(self._lib.gmrf_comm_bytes(self._h, int(reset), C.byref(v)))
        return v.value

    def allreduce_sum(self, dev_tensor, F: Optional[TridiagonalCholeskyFactor] = None):
        _cabi.check(self._lib.gmrf_comm_allreduce_sum(self._h, F._h if F is not None else None, _cabi.ptr(dev_tensor),
                                                      dev_tensor.numel()))
        return dev_tensor
