"""Every kernel route of the sparse products Y = S X, each asserted through the route hook (gmrf_test_spmm_route: the route the
library would take for the call's geometry, and after the call the one it took) and checked cell by cell against a longdouble
reference with the row-wise bound of tests/spmm_ref.py.

Operands are torch device tensors with leading dimensions beyond the live extent: the pad of X and every row of X no entry reads
hold NaN, Y is prefilled with a sentinel that every cell outside the live columns must still hold.  Matrices have 100 rows (one
full 64-row tile + 36: every kernel meets a partial last tile) with rows 5 and 99 empty, unless stated."""
import ctypes as C

import numpy as np
import pytest

from tests import spmm_ref as R

pytestmark = pytest.mark.gpu

PLAIN, TILES, PAD = R.PLAIN, R.TILES, R.PAD
SENTINEL = -1.2345e300
TABLE = sorted(R.TABLE)


class Dev:
    """A device matrix created from raw CSR arrays on torch's current stream, with the hooks around it."""

    def __init__(self, pkg, A, f32=False, vals=None):
        import torch
        self.pkg, self.lib, self.A, self.f32 = pkg, pkg._cabi.load(), A, f32
        self.vals = A.vals if vals is None else np.ascontiguousarray(vals, np.float64)
        self.h = C.c_void_p()
        p = pkg._cabi.ptr
        pkg._cabi.check(self.lib.gmrf_csr_create(0, C.c_void_p(torch.cuda.current_stream().cuda_stream), A.shape[0], A.shape[1],
                                                 p(A.rowptr), p(A.colidx), p(self.vals), 0, int(f32), C.byref(self.h)))

    def __del__(self):
        try:
            if self.h.value:
                self.lib.gmrf_csr_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def route(self, k, ldx, ldy, X, Y, xs=0, ys=0, no_pad=False):
        geom = np.array([k, ldx, ldy, 0, 0, xs, ys, no_pad], np.int64)
        out = np.zeros(12, np.int64)
        self.pkg._cabi.check(self.lib.gmrf_test_spmm_route(self.h, self.pkg._cabi.ptr(geom), C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr()),
                                                           self.pkg._cabi.ptr(out)))
        o = [int(v) for v in out]
        return {"rows": (o[6], o[7], o[1] if o[6] != PLAIN else 0), "cols": o[8],
                "last_rows": (o[9], o[10], o[1] if o[9] > PLAIN else 0), "last_cols": o[11]}


def operand(rows, ld, live, fill, off=0, problems=1, stride=0):
    """A flat device buffer of `problems` node-major (rows, ld) operands `stride` apart, starting `off` doubles into the
    allocation, all cells = fill.  Returns (buffer, view of the operands' first cell on, mask of the live cells in the buffer)."""
    import torch
    stride = stride if problems > 1 else 0
    n = off + (problems - 1) * stride + rows * ld + 3
    buf = torch.full((n,), fill, dtype=torch.float64, device="cuda")
    mask = np.zeros(n, bool)
    for p in range(problems):
        m = mask[off + p * stride: off + p * stride + rows * ld].reshape(rows, ld)
        m[:, :live] = True
    return buf, buf[off:], mask


def live_x(A, k, seed, problems=1, p0=0):
    """Random right-hand sides (problems, n_cols, k) of the problems p0, p0 + 1, ... (problem p's do not depend on the batch it
    comes in); the rows no entry reads are NaN."""
    X = np.stack([np.random.default_rng([1000 + seed, p0 + p]).standard_normal((A.shape[1], k)) for p in range(problems)])
    X[:, A.unreferenced(), :] = np.nan
    return X


def put(buf, mask, values):
    import torch
    buf[torch.from_numpy(np.flatnonzero(mask)).cuda()] = torch.from_numpy(np.ascontiguousarray(values).ravel()).cuda()


def take(buf, mask, shape, what):
    """The live cells; everything else must still hold the sentinel."""
    h = buf.cpu().numpy()
    rest = h[~mask]
    assert np.all(rest == SENTINEL), f"{what}: {np.count_nonzero(rest != SENTINEL)} cells outside the live columns were written"
    return h[mask].reshape(shape)


def rows_call(S, k, ldx, ldy, expect, x_off=0, y_off=0, seed=0, p0=0, what=""):
    """One node-major product through the public stream-ordered entry; returns Y (n_rows, k)."""
    import torch
    A = S.A
    X = live_x(A, k, seed, 1, p0)[0]
    xb, xv, xm = operand(A.shape[1], ldx, k, float("nan"), x_off)
    yb, yv, ym = operand(A.shape[0], ldy, k, SENTINEL, y_off)
    put(xb, xm, X)
    assert xv.data_ptr() % 16 == 8 * (x_off % 2) and yv.data_ptr() % 16 == 8 * (y_off % 2)
    assert S.route(k, ldx, ldy, xv, yv)["rows"] == expect, (what, "would take", S.route(k, ldx, ldy, xv, yv), expect)
    torch.cuda.synchronize()                                # (the matrix may run on a stream of its own: the fills first)
    S.pkg._cabi.check(S.lib.gmrf_spmm_rows_async(S.h, C.c_void_p(xv.data_ptr()), C.c_void_p(yv.data_ptr()), k, ldx, ldy))
    torch.cuda.synchronize()
    assert S.route(k, ldx, ldy, xv, yv)["last_rows"] == expect, (what, "took", S.route(k, ldx, ldy, xv, yv), expect)
    Y = take(yb, ym, (A.shape[0], k), what)
    ratio = R.check(Y, A, X, f32=S.f32, vals=S.vals, what=what)
    print(f"{what}: route {expect}, k {k} ld ({ldx}, {ldy}) worst error / bound {ratio:.3f}")
    return Y


def batch_call(S, vals, k, ldx, ldy, expect, xs=None, ys=None, no_pad=False, seed=0, p0=0, what=""):
    """gmrf_test_spmm_rows_batch on B = len(vals) problems; returns Y (B, n_rows, k)."""
    import torch
    A = S.A
    vals = np.ascontiguousarray(vals, np.float64).reshape(-1, A.nnz)
    B = len(vals)
    xs = A.shape[1] * ldx if xs is None else xs
    ys = A.shape[0] * ldy if ys is None else ys
    X = live_x(A, k, seed, B, p0)
    xb, xv, xm = operand(A.shape[1], ldx, k, float("nan"), 0, B, xs)
    yb, yv, ym = operand(A.shape[0], ldy, k, SENTINEL, 0, B, ys)
    put(xb, xm, X)
    dv = torch.from_numpy(vals).cuda()
    geom = dict(xs=xs if B > 1 else 0, ys=ys if B > 1 else 0, no_pad=no_pad)
    assert S.route(k, ldx, ldy, xv, yv, **geom)["rows"] == expect, (what, "would take", S.route(k, ldx, ldy, xv, yv, **geom), expect)
    torch.cuda.synchronize()
    S.pkg._cabi.check(S.lib.gmrf_test_spmm_rows_batch(S.h, B, C.c_void_p(dv.data_ptr()), C.c_void_p(xv.data_ptr()), ldx, geom["xs"],
                                                      C.c_void_p(yv.data_ptr()), ldy, geom["ys"], k, int(no_pad)))
    torch.cuda.synchronize()
    assert S.route(k, ldx, ldy, xv, yv, **geom)["last_rows"] == expect, (what, "took", expect)
    Y = take(yb, ym, (B, A.shape[0], k), what)
    for p in range(B):
        ratio = R.check(Y[p], A, X[p], vals=vals[p], what=f"{what} problem {p}")
        print(f"{what} problem {p}: route {expect}, k {k} worst error / bound {ratio:.3f}")
    return Y


def cols_call(S, k, expect, seed=0, what=""):
    """One column-major product (gmrf_spmm_async) with ldx = n_cols + 3, ldy = n_rows + 5; returns Y (n_rows, k)."""
    import torch
    A = S.A
    ldx, ldy = A.shape[1] + 3, A.shape[0] + 5
    X = live_x(A, k, seed)[0]
    xb, xv, xm = operand(k, ldx, A.shape[1], float("nan"))
    yb, yv, ym = operand(k, ldy, A.shape[0], SENTINEL)
    put(xb, xm, X.T)
    assert S.route(k, k + (k & 1), k + (k & 1), xv, yv)["cols"] == expect, (what, "would take", S.route(k, k, k, xv, yv), expect)
    torch.cuda.synchronize()                                # (the matrix may run on a stream of its own: the fills first)
    S.pkg._cabi.check(S.lib.gmrf_spmm_async(S.h, C.c_void_p(xv.data_ptr()), C.c_void_p(yv.data_ptr()), k, ldx, ldy))
    torch.cuda.synchronize()
    assert S.route(k, k + (k & 1), k + (k & 1), xv, yv)["last_cols"] == expect, (what, "took", expect)
    Y = take(yb, ym, (k, A.shape[0]), what).T
    ratio = R.check(Y, A, X, f32=S.f32, vals=S.vals, what=what)
    print(f"{what}: lane group {expect}, k {k} worst error / bound {ratio:.3f}")
    return Y


@pytest.fixture(scope="module")
def table(pkg):
    """The six table matrices, device handles with fp64 and fp32 values, and each one's planned tile height."""
    out = {}
    for key in TABLE:
        A = R.generate(100, *R.TABLE[key])
        out[key] = (A, Dev(pkg, A), Dev(pkg, A, f32=True))
    return out


# ------------------------------------------------------------------------------------------ node-major, padded kernels
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("key", TABLE, ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_padded_kernels(table, key, f32):
    A, S64, S32 = table[key]
    rows_call(S32 if f32 else S64, 16, 18, 22, (PAD, key[1], key[0]), what=f"padded {key}")


@pytest.mark.parametrize("key", TABLE, ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_row_lengths_padded_and_unpadded(pkg, key):
    """Rows of 0, 1, 7, 8, 9, 15, 16, 17, 24 and 31 entries: the padded kernel's first-16 staging, its j >= 16 loop and rows
    padded by 0 .. 7 entries; the unpadded kernel's turns of 8, 4, 2 and 1."""
    w, per = R.TABLE[key]
    A = R.generate(100, w, per, lengths=R.ROW_LENGTHS)
    assert set(np.diff(A.rowptr)) == set(R.ROW_LENGTHS)
    # (short rows change the plan: the route comes from the restatement, which the CPU test holds against the library's plan)
    pl = R.plan(100, A.rowptr, A.colidx)
    kind, ng = R.rows_route(pl, w, 16, 16, 16)
    assert kind == PAD
    S = Dev(pkg, A)
    Y = rows_call(S, 16, 16, 16, (PAD, ng, pl["R"]), what="row lengths, padded")
    rows_call(Dev(pkg, A, f32=True), 16, 16, 16, (PAD, ng, pl["R"]), what="row lengths, padded, fp32")
    Yu = batch_call(S, A.vals, 16, 16, 16, (TILES, ng, pl["R"]), no_pad=True, what="row lengths, unpadded")
    assert np.array_equal(Yu[0], Y)


# ------------------------------------------------------------------------------------------ node-major, unpadded kernels
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_unpadded_kernel_reached_by_the_plan(pkg, f32):
    """width 96, per 57: 3591 entries per 64-row tile (ecap 3840) fit the unpadded image, their padding to 64 per row does not."""
    A = R.generate(100, *R.UNPADDED_64_7)
    S = Dev(pkg, A, f32=f32)
    for k, ldx, ldy in ((16, 16, 16), (14, 16, 20), (34, 36, 40)):
        rows_call(S, k, ldx, ldy, (TILES, 7, 64), what="unpadded R64 NG7")


@pytest.mark.parametrize("key", TABLE, ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_unpadded_kernels_with_the_padded_plan_withheld(table, key):
    A, S64, _ = table[key]
    batch_call(S64, A.vals, 16, 18, 22, (TILES, key[1], key[0]), no_pad=True, what=f"unpadded {key}")


# ------------------------------------------------------------------------------------------ k and ld on each tiled route
@pytest.mark.parametrize("no_pad", [False, True], ids=["padded", "unpadded"])
@pytest.mark.parametrize("key", TABLE, ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_k_and_leading_dimensions(table, key, no_pad):
    """k = 2, 4 (one partial chunk), 14 (k mod 16 = 14: the scalar tail store of the last lane group), 16, 18 (mod 16 = 2), 34 (three
    chunks); leading dimensions equal to k and beyond it by different amounts for X and Y."""
    A, S64, _ = table[key]
    for k in (2, 4, 14, 16, 18, 34):
        for ldx, ldy in ((k, k), (k + 2, k + 6)):
            if no_pad:
                batch_call(S64, A.vals, k, ldx, ldy, (TILES, key[1], key[0]), no_pad=True, seed=k, what=f"unpadded {key}")
            else:
                rows_call(S64, k, ldx, ldy, (PAD, key[1], key[0]), seed=k, what=f"padded {key}")


# ------------------------------------------------------------------------------------------ plain kernel, reason by reason
@pytest.mark.parametrize("reason,k,ldx,ldy,x_off,y_off", [
    ("k = 1", 1, 2, 2, 0, 0), ("k = 3", 3, 4, 4, 0, 0), ("k = 17", 17, 18, 18, 0, 0),
    ("ldx odd", 4, 5, 6, 0, 0), ("ldy odd", 4, 6, 7, 0, 0), ("X base at +8 bytes", 4, 6, 6, 1, 0), ("Y base at +8 bytes", 4, 6, 6, 0, 1),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else None)
def test_plain_kernel_by_alignment(table, reason, k, ldx, ldy, x_off, y_off):
    """A matrix WITH a padded plan (R 64, NG 10), so the one thing named is what sends the call to csr_spmm_rows; the same call
    with that thing mended takes the padded kernel."""
    A, S64, S32 = table[(64, 10)]
    for S in (S64, S32):
        rows_call(S, k, ldx, ldy, (PLAIN, 0, 0), x_off, y_off, what=f"plain: {reason}")
    rows_call(S64, k + (k & 1), ldx + (ldx & 1), ldy + (ldy & 1), (PAD, 10, 64), what=f"mended: {reason}")


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_plain_kernel_without_a_plan(pkg, f32):
    A = R.generate(100, *R.NO_PLAN)                          # 16-row tiles of ~290 distinct columns and 912 entries: beyond 52 KB
    assert R.plan(100, A.rowptr, A.colidx)["state"] == -1
    S = Dev(pkg, A, f32=f32)
    for k in (2, 16, 34):
        rows_call(S, k, k + 2, k + 6, (PLAIN, 0, 0), what="plain: no plan")
    A = R.generate(100, 300, 520, replace=True)              # 16 rows x 520 entries > 8192 (columns repeat within a row)
    pl = R.plan(100, A.rowptr, A.colidx)
    assert pl["state"] == -1 and set(pl["why"].values()) == {"entries"}
    rows_call(Dev(pkg, A, f32=f32), 16, 18, 22, (PLAIN, 0, 0), what="plain: entries")


# ------------------------------------------------------------------------------------------ one summation order everywhere
@pytest.mark.parametrize("key", TABLE, ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_all_node_major_routes_agree_bitwise(table, key):
    """Every node-major route adds a row's products in CSR order into one fused multiply-add chain: padded, unpadded (withheld),
    plain (odd ldy), one problem of a batch and the product with another problem's (equal) values are the same bits."""
    A, S64, _ = table[key]
    r, ng = key
    k = 16
    Y = rows_call(S64, k, k, k, (PAD, ng, r), what="bitwise: padded")
    assert np.array_equal(Y, rows_call(S64, k, k, k + 1, (PLAIN, 0, 0), what="bitwise: plain"))
    assert np.array_equal(Y, batch_call(S64, A.vals, k, k, k, (TILES, ng, r), no_pad=True, what="bitwise: unpadded")[0])
    assert np.array_equal(Y, batch_call(S64, A.vals, k, k, k, (PAD, ng, r), what="bitwise: other values, padded")[0])
    assert np.array_equal(Y, batch_call(S64, A.vals, k, k, k + 1, (PLAIN, 0, 0), what="bitwise: other values, plain")[0])
    other = np.random.default_rng(9).standard_normal((3, A.nnz))
    other[1] = A.vals
    Y1 = rows_call(S64, k, k, k, (PAD, ng, r), p0=1, what="bitwise: padded, the right-hand sides of problem 1")
    assert np.array_equal(Y1, batch_call(S64, other, k, k, k, (PAD, ng, r), what="bitwise: batch")[1])


# ------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("key", [(64, 7), (32, 10), (16, 7)], ids=lambda k: f"R{k[0]}-NG{k[1]}")
def test_batches_with_gaps_between_problems(pkg, table, key):
    """B = 3 value sets, problems further apart than one operand (the gaps keep their sentinels / NaN): every problem is bitwise the
    one-problem product of a matrix created with its values, on the padded, an unpadded and the plain route (an odd stride)."""
    A, _, _ = table[key]
    r, ng = key
    k, ldx, ldy = 16, 18, 22
    vals = np.random.default_rng(5).standard_normal((3, A.nnz))
    S = Dev(pkg, A)
    # the one-problem calls: a matrix created with problem p's values, through the public entry, on problem p's right-hand sides
    one = np.stack([rows_call(Dev(pkg, A, vals=vals[p]), k, ldx, ldy, (PAD, ng, r), p0=p, what=f"one problem {p}") for p in range(3)])
    xs, ys = A.shape[1] * ldx + 10, A.shape[0] * ldy + 14
    Yb = {"padded": batch_call(S, vals, k, ldx, ldy, (PAD, ng, r), xs, ys, what="batch, padded"),
          "unpadded": batch_call(S, vals, k, ldx, ldy, (TILES, ng, r), xs, ys, no_pad=True, what="batch, unpadded"),
          "plain, odd x stride": batch_call(S, vals, k, ldx, ldy, (PLAIN, 0, 0), xs + 1, ys, what="batch, plain (odd x stride)"),
          "plain, odd y stride": batch_call(S, vals, k, ldx, ldy, (PLAIN, 0, 0), xs, ys + 1, what="batch, plain (odd y stride)")}
    for name, Y in Yb.items():
        assert np.array_equal(Y, one), name


# ------------------------------------------------------------------------------------------ column-major
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("per,g", [(9, 8), (15, 16), (25, 32), (45, 64)])
def test_lane_group_kernel(pkg, per, g, f32):
    """csr_spmm<VT, G> at every G, every remainder of k mod 4 (k = 2, 3, 4, 5, 7, 9: turns of four right-hand sides and a last turn
    of 1, 2 or 3), leading dimensions beyond n_cols and n_rows."""
    A = R.generate(100, 120, per)
    S = Dev(pkg, A, f32=f32)
    for k in (2, 3, 4, 5, 7, 9):
        cols_call(S, k, g, seed=k, what=f"lane group per {per}")


@pytest.mark.parametrize("lengths,g", [((30, 1, 1, 1, 1, 1), 8), ((70, 3, 3, 3, 3, 3, 3), 16)], ids=["G8", "G16"])
def test_lane_group_rows_shorter_than_g_and_longer_than_2g(pkg, lengths, g):
    A = R.generate(100, 120, 0, lengths=lengths)
    L = np.diff(A.rowptr)
    assert 0 < L[L > 0].min() < g and L.max() > 2 * g
    S = Dev(pkg, A)
    for k in (2, 5, 7):
        cols_call(S, k, g, what=f"lane group rows {lengths}")


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_spmv_tiles_second_pass(pkg, f32):
    """per 25: a 64-row tile has 1550 entries, beyond the 1024 of the pipelined first pass."""
    A = R.generate(100, 120, 25)
    assert 1024 < A.rowptr[64] <= R.SPMV_CAP
    cols_call(Dev(pkg, A, f32=f32), 1, 0, what="spmv tiles, second pass")


@pytest.mark.parametrize("extra,expect", [(0, 0), (1, 32)], ids=["2304", "2305"])
def test_spmv_tiles_capacity(pkg, extra, expect):
    """A 64-row tile of exactly SPMV_CAP = 2304 entries fills csr_spmv_tiles' LDS image; one more and the matrix takes the lane-group
    kernel at k = 1."""
    A = R.generate(100, 120, 36, empty=(), lengths=[36 + extra] + [36] * 63 + [3] * 36)
    assert A.rowptr[64] == 2304 + extra
    cols_call(Dev(pkg, A), 1, expect, what=f"spmv tiles, {2304 + extra} entries")


def test_spmv_tiles_multi_tile_walk(pkg):
    """131072 + 3 * 64 + 5 rows: 2052 tiles on the 2048 workgroups the launcher caps the grid at, so four workgroups walk two tiles
    (the software pipeline's prefetched next tile) and the last tile is partial."""
    n = 131072 + 3 * 64 + 5
    A = R.tridiagonal(n)
    assert (n + 63) // 64 == 2048 + 4 and n % 64 == 5
    cols_call(Dev(pkg, A), 1, 0, what="spmv tiles, multi-tile walk")
