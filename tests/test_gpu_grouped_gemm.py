"""Two independent products in one launch (gemm_f64_dma_grouped): the diagonal chain of a batch's 256-column panels runs
S_BB -= L_BA L_BA^T and T = L_BA X_A as ONE launch in front of the second potrf_diag128 -- five launches per panel instead of six.
Checked: the route and the launch counts from the launch statistics, the factor bitwise against the same build with the grouping
switched off (set_eager bit 20) and against the oracle, and the kernel itself against two single launches."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O
from tests.test_gpu_parity import TOL_FACTOR

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch
TRI_B_LOWER = 4
GEMM_CLASSES = (0, 6, 7, 11, 12, 13, 14, 15, 18)


def chain(bs, nb, seed=0, corner=0):
    """A diagonally dominant block tridiagonal matrix of nb blocks of bs: tridiagonal diagonal blocks; coupling blocks with a
    diagonal and a subdiagonal, or (corner = w) entries only in their first w rows and last w columns."""
    rng = np.random.default_rng(seed)
    n = bs * nb
    T = sp.diags([-np.ones(bs - 1), np.zeros(bs), -np.ones(bs - 1)], [-1, 0, 1])
    D = sp.kron(sp.eye(nb), T)
    if corner:
        r = np.arange(corner)
        Bc = sp.coo_matrix((-(0.5 + 0.5 * rng.random(corner)), (r, bs - corner + r)), shape=(bs, bs))
        Bc = Bc + sp.coo_matrix((-0.3 * np.ones(corner - 1), (r[1:], bs - corner + r[:-1])), shape=(bs, bs))
    else:
        Bc = sp.diags([-(0.5 + 0.5 * rng.random(bs)), -0.3 * np.ones(bs - 1)], [0, -1])
    Lo = sp.kron(sp.eye(nb, k=-1), Bc)
    Q = D + Lo + Lo.T + sp.diags(6.0 + rng.random(n))
    Q = sp.csc_matrix(Q)
    Q.sort_indices()
    return Q


def _blocks(F, nb, probs):
    out = []
    for p in probs:
        F.select_problem(p)
        for i in range(nb):
            out.append(F.get_block(2, i))                  # Linv_i
            if i + 1 < nb:
                out.append(F.get_block(1, i))              # C_{i+1}
        out.append(np.array([F.logdet()]))
    F.select_problem(0)
    return out


def _profiled_refactor(F, vals):
    F.set_profiling(1)
    F.refactor(vals)
    st = F.stats()
    shapes = F.gemm_shapes()
    F.set_profiling(0)
    return st, shapes


BS, NB, B = 512, 3, 8
PANELS = NB * (BS // 256)


@pytest.fixture(scope="module")
def factored(pkg):
    Q = chain(BS, NB)
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.set_eager(Switch.NO_PERSIST_PANELS)
    F.factor(Q, NB, values=vals)
    probs = tuple(range(B))
    grouped = _blocks(F, NB, probs)
    st_g, shapes_g = _profiled_refactor(F, vals)
    F.set_eager(Switch.NO_PERSIST_PANELS | Switch.NO_GROUPED_GEMM)
    F.refactor(vals)
    plain = _blocks(F, NB, probs)
    st_p, shapes_p = _profiled_refactor(F, vals)
    F.close()                                              # (the results are host arrays: the handle and its claims go now)
    return Q, vals, grouped, plain, st_g, shapes_g, st_p, shapes_p


def test_route_and_one_launch_fewer_per_panel(factored):
    Q, vals, grouped, plain, st_g, shapes_g, st_p, shapes_p = factored
    for st in (st_g, st_p):
        # the launch-per-product route of the 256-column panels: two potrf_diag128 per panel, no persistent launch
        assert st["persist_route"] == 0
        assert st["kernel_launches"][17] == 0
        assert st["kernel_launches"][16] == 2 * PANELS
    n_g = sum(st_g["kernel_launches"][c] for c in GEMM_CLASSES)
    n_p = sum(st_p["kernel_launches"][c] for c in GEMM_CLASSES)
    print("GEMM launches per factorisation: grouped", n_g, "plain", n_p, "panels", PANELS)
    assert n_p - n_g == PANELS
    assert sum(st_p["kernel_launches"]) - sum(st_g["kernel_launches"]) == PANELS
    # the grouped launch is booked once per panel, with both products' flops
    rows = [g for g in shapes_g if g["class"] == 14 and (g["M"], g["N"], g["K"]) == (256, 128, 128)]
    assert len(rows) == 1 and rows[0]["launches"] == PANELS
    assert not [g for g in shapes_p if (g["M"], g["N"], g["K"]) == (256, 128, 128)]
    w_g = sum(st_g["kernel_work"][c] for c in GEMM_CLASSES)
    w_p = sum(st_p["kernel_work"][c] for c in GEMM_CLASSES)
    assert abs(w_g - w_p) <= 1e-12 * w_p
    t3 = 2.0 * 64.0 ** 3
    assert abs(rows[0]["flops"] - PANELS * B * (6.0 * t3 + 8.0 * t3 * 0.75)) <= 1e-9 * rows[0]["flops"]


def test_factor_bitwise_with_and_without_grouping(factored):
    Q, vals, grouped, plain, *_ = factored
    assert len(grouped) == len(plain) == B * (2 * NB)
    assert all(np.array_equal(a, c) for a, c in zip(grouped, plain))


def test_factor_against_the_oracle(factored):
    Q, vals, grouped, *_ = factored
    per = 2 * NB
    for p in (0, B - 1):
        Qp = Q.copy(); Qp.data = vals[p]
        Fo = O.tridiagonal_cholesky(Qp, NB)
        got = grouped[p * per:(p + 1) * per]
        for i in range(NB):
            Xo = np.linalg.inv(Fo.chos[i])
            assert np.max(np.abs(np.tril(got[2 * i]) - Xo)) / np.max(np.abs(Xo)) < TOL_FACTOR
            if i + 1 < NB:
                assert np.max(np.abs(got[2 * i + 1] - Fo.Cs[i])) / np.max(np.abs(Fo.Cs[i])) < TOL_FACTOR
        ld = O.logdet(Fo)
        assert abs(got[-1][0] - ld) <= TOL_FACTOR * abs(ld)


def _pair(pkg, lib, batch, grouped, desc, ab, ops):
    out = [ops[2].copy(), ops[5].copy()]
    d = np.asarray(desc, dtype=np.int64)
    a = np.asarray(ab, dtype=np.float64)
    pkg._cabi.check(lib.gmrf_test_gemm_pair(0, batch, int(grouped), pkg._cabi.ptr(d), pkg._cabi.ptr(a), pkg._cabi.ptr(ops[0]),
                                            pkg._cabi.ptr(ops[1]), pkg._cabi.ptr(out[0]), pkg._cabi.ptr(ops[3]), pkg._cabi.ptr(ops[4]),
                                            pkg._cabi.ptr(out[1])))
    return out


@pytest.mark.parametrize("batch", [1, 5, 8])
def test_grouped_launch_against_two_launches(pkg, lib, batch):
    """Descriptor 0: a rank-128 update of the lower tiles of a 128 x 128 block (B [n][k], triangular grid, alpha = -1, beta = 1);
    descriptor 1: 192 x 128 outputs through a lower triangular B stored [k][n] (alpha = 1, beta = 0).  3 and 6 workgroups per
    problem: with 5 problems neither count is a multiple of 8."""
    rng = np.random.default_rng(batch)
    M0 = N0 = K0 = 128
    M1, N1, K1 = 192, 128, 128
    A0 = rng.standard_normal((batch, M0, K0)); B0 = rng.standard_normal((batch, N0, K0)); C0 = rng.standard_normal((batch, M0, N0))
    A1 = rng.standard_normal((batch, M1, K1)); B1 = np.tril(rng.standard_normal((batch, K1, N1))); C1 = rng.standard_normal((batch, M1, N1))
    ops = [np.ascontiguousarray(x) for x in (A0, B0, C0, A1, B1, C1)]
    desc = [M0, N0, K0, 0, 0, 1, M1, N1, K1, 1, TRI_B_LOWER, 0]
    ab = [-1.0, 1.0, 1.0, 0.0]
    one = _pair(pkg, lib, batch, True, desc, ab, ops)
    two = _pair(pkg, lib, batch, False, desc, ab, ops)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    # and both are the products: the 64 x 64 tiles that touch the lower triangle of C0 (the others keep their input), all of C1
    ref0 = C0 - A0 @ B0.transpose(0, 2, 1)
    upper = np.zeros((M0, N0), dtype=bool); upper[:64, 64:] = True
    assert np.array_equal(one[0][:, upper], C0[:, upper])
    assert np.max(np.abs(one[0][:, ~upper] - ref0[:, ~upper])) < 1e-12 * K0
    assert np.max(np.abs(one[1] - A1 @ B1)) < 1e-12 * K1
