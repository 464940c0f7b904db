"""The references of tests/takahashi_ref.py without a GPU: every case is the geometry it is there for (on the restatement and
on the library's own symbolic analysis of the matrix), the matrices stay well conditioned, the float64 restatement of the
kernels' products stays inside Reference A's bound and the float64 recurrence of tests/selinv_oracle.py inside Reference B's
gate, and every planted defect is pushed over the bound by the checks tests/test_gpu_takahashi_windows.py applies."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import bt_oracle as O
from tests import bxt_ref as R
from tests import selinv_oracle as SI
from tests import takahashi_ref as T

DEFECT_CASES = ("window", "ragged", "padded64", "late")


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


_FACTORS = {}


def _oracle_factor(name, p=0):
    """(X_i, C_i) of problem p in float64 from the oracle's factor: shared, left unchanged."""
    if (name, p) not in _FACTORS:
        geo = T.geometry(name)
        F = O.tridiagonal_cholesky(T.matrix(name, p)[0], geo.N)
        eye = np.eye(geo.bs)
        _FACTORS[(name, p)] = (F, [O._chol_forward(L, eye) for L in F.chos], F.Cs)
    return _FACTORS[(name, p)]


def _values(name, Xs, Cs, defect=None):
    geo = T.geometry(name)
    diag, low, var = T.restate(geo, Xs, Cs, defect)
    return T.sel_pattern(name).fill(diag, [b[:geo.rme] for b in low]), var


@pytest.mark.parametrize("name", T.CASES)
def test_case_geometry(pkg, lib, name):
    """(bs, bsp, N, cmin, rmax, kst) of every case on the restatement, and the library's analysis of the matrix that is factored."""
    geo = T.geometry(name)
    assert geo.summary() == T.GEOMETRY[name], (name, geo.summary())
    assert name not in R.ALL_CASES or T.pattern(name) is R.case(name)
    Q = T.matrix(name, 0)[0]
    assert (abs(Q - Q.T)).nnz == 0 and Q.has_sorted_indices
    for p in (1, 8):                                        # another seed, the same pattern
        Qp = T.matrix(name, p)[0]
        assert np.array_equal(Qp.indptr, Q.indptr) and np.array_equal(Qp.indices, Q.indices) and not np.array_equal(Qp.data, Q.data)
    if geo.N > 1:
        class Pat:
            n, N, bsp, nnz = geo.n, geo.N, geo.bsp, Q.nnz
            colptr, rowval = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)
        P, _ = R.lib_plan(pkg._cabi, lib, Pat, True)
        assert (P["cmin"], P["rmax"], [int(v) for v in P["kst"]]) == (geo.cmin, geo.rmax, geo.kst), name
    # what the geometries are for
    if name == "late":
        assert geo.cmin > geo.rmax
    if name == "padded64":
        assert geo.rmax < geo.bs < geo.bsp
    if name == "padded100":
        assert geo.bs < geo.rmax
    if name == "split512":
        assert geo.bsp // 64 >= 8 and geo.cmin >= 256              # a batch keeps its block inverses split at 256
    if name == "window5rev":
        assert (geo.cmin, geo.rmax) == (256 - T.geometry("window5").rmax, 256 - T.geometry("window5").cmin)
    # the window's masks: the last column tile of the window is met by every row tile, so a planted K-bound defect there bites
    assert geo.N == 1 or geo.mend[(geo.bs - geo.cmin - 1) // 64] == geo.rmax
    rows = geo.rows(0)
    assert set(r for r in (0, 63, 64, geo.rmax - 1, geo.rmax, geo.bs - 1) if r < geo.bs) <= set(rows.tolist())
    assert set((rows // 64).tolist()) == set(range((geo.bs + 63) // 64)) and rows.max() < geo.bs


@pytest.mark.parametrize("name", T.CASES)
def test_condition_cap(name, capsys):
    conds = [T.matrix(name, p)[1] for p in range(9)]                  # every problem a batch of 9 factors
    _say(capsys, f"TAKAHASHI_COND {name}: cond_2 of problems 0 .. {len(conds) - 1}: {min(conds):.1f} .. {max(conds):.1f}")
    assert max(conds) <= T.COND_CAP, (name, conds)


@pytest.mark.parametrize("name", T.CASES)
def test_restatement_within_reference_a(name, capsys):
    """The kernels' products in float64 on the oracle's factor against the longdouble recurrence on the same factor."""
    geo = T.geometry(name)
    _, Xs, Cs = _oracle_factor(name)
    ref = T.ReferenceA(geo, Xs, Cs)
    vals, var = _values(name, Xs, Cs)
    worst, where, by_region = T.check_selinv(ref, T.sel_pattern(name), vals)
    wv, where_v = T.check_var(ref, var)
    _say(capsys, f"TAKAHASHI_REF_A {name}: restatement / bound, selected inverse {worst:.4f} at {where}, variances {wv:.4f} at {where_v}")
    assert 0.0 < worst <= 1.0 and 0.0 < wv <= 1.0, (name, worst, where, wv, where_v)
    assert all(v <= 1.0 for v in by_region.values())
    # the truth too, at the kernels' gate
    tr = T.truth(name, 0)
    assert tr.resid <= 1e-17, (name, tr.resid)
    assert T.truth_selinv(tr, T.sel_pattern(name), vals) <= T.TRUTH_FACTOR and T.truth_var(tr, var) <= T.TRUTH_FACTOR


@pytest.mark.parametrize("name", T.CASES)
def test_float64_recurrence_within_reference_b(name, capsys):
    """tests/selinv_oracle.pattern_values on the pattern of Q against the longdouble inverse: <= 1 cond 2^-52 on the correlation scale."""
    geo = T.geometry(name)
    Q, cond = T.matrix(name, 0)
    F = _oracle_factor(name)[0]
    S = sp.csr_matrix(Q)
    S.sort_indices()
    vals, mask, _ = SI.pattern_values(F, S)
    assert mask.all()
    tr = T.truth(name, 0)
    assert tr.resid <= 1e-17
    # every entry of Q's pattern that lies in a row the truth keeps (its own block and the block before it)
    d = np.sqrt(tr.diag)
    rows = np.repeat(np.arange(geo.n), np.diff(S.indptr))
    worst, count = 0.0, 0
    for i in range(geo.N):
        for r in tr.rows[i]:
            g = i * geo.bs + int(r)
            for blk, ref_rows, ref in ((i, tr.rows[i], tr.d_val[i]), (i - 1, tr.l_rows[i - 1], tr.l_val[i - 1] if i > 0 else None)):
                e = np.flatnonzero((rows == g) & (S.indices // geo.bs == blk))
                if blk < 0 or r not in ref_rows or not len(e):
                    continue
                want = ref[list(ref_rows).index(r), S.indices[e] - blk * geo.bs]
                worst = max(worst, float((np.abs(vals[e].astype(T.LD) - want) / (d[g] * d[S.indices[e]])).max()))
                count += len(e)
    assert count > 20 * geo.N
    # and the recurrence's whole blocks on the dense pattern
    diag, low = SI.selected_blocks(F)
    dense = T.truth_selinv(tr, T.sel_pattern(name), T.sel_pattern(name).fill([diag[i] for i in range(geo.N)], [low[i][:geo.rme] for i in range(geo.N - 1)]))
    _say(capsys, f"TAKAHASHI_REF_B {name}: float64 recurrence, error / (cond 2^-52): {worst / (cond * T.EPS):.3f} on the pattern of Q "
                 f"({count} entries), {dense:.3f} on the dense pattern")
    assert worst <= cond * T.EPS and dense <= 1.0, (name, worst / (cond * T.EPS), dense)


def test_gate_of_one_is_a_measured_one(capsys):
    """A fact, recorded: 1 cond 2^-52 is what the float64 recurrence meets on problem 0 of every case, not a bound it must meet.
    On another seed of padded100 (cond 5.4, where a single rounding of an entry is a fifth of the gate) it is past it, and still
    inside the factor 4 the kernels are given."""
    name, p = "padded100", 2
    geo, selpat = T.geometry(name), T.sel_pattern(name)
    diag, low = SI.selected_blocks(_oracle_factor(name, p)[0])
    ratio = T.truth_selinv(T.truth(name, p), selpat, selpat.fill([diag[i] for i in range(geo.N)], [low[i][:geo.rme] for i in range(geo.N - 1)]))
    _say(capsys, f"TAKAHASHI_FACT {name} problem {p}: float64 recurrence, error / (cond 2^-52) = {ratio:.3f}")
    assert ratio <= T.TRUTH_FACTOR


@pytest.mark.parametrize("name", DEFECT_CASES)
def test_planted_defects_are_caught(name, capsys):
    geo, selpat = T.geometry(name), T.sel_pattern(name)
    _, Xs, Cs = _oracle_factor(name)
    ref = T.ReferenceA(geo, Xs, Cs)
    good, good_var = _values(name, Xs, Cs)
    assert T.check_selinv(ref, selpat, good)[0] <= 1.0 and T.check_var(ref, good_var)[0] <= 1.0
    seen = {}
    # a K slice dropped from each product, the two K-bound arrays, the mirror, the split of the diagonal at rmax
    for defect in T.DEFECTS:
        vals, var = _values(name, Xs, Cs, defect)
        a, where, _ = T.check_selinv(ref, selpat, vals)
        v, _ = T.check_var(ref, var)
        seen[defect] = (a, v)
        if defect == "diag_without_y":
            assert v > 1.0, (name, defect, v)
        else:
            assert a > 1.0, (name, defect, a, where)
            assert where[1] in T.REGIONS
    # a coupling entry read transposed: Sigma_{i+1,i}[r, c] holds [c, r]
    i, bs = geo.N - 2, geo.bs
    lr = ref.l_rows[i]                                      # (the pair of checked rows whose two entries differ most)
    sub = np.abs(ref.l_val[i][:, lr] - ref.l_val[i][:, lr].T).astype(np.float64)
    r, c = (int(lr[k]) for k in np.unravel_index(np.argmax(sub), sub.shape))
    if name == "late":
        # rows and columns below rmax = 64 lie left of cmin = 192, where X[cmin:, :] is exactly zero: both entries are exact
        # zeros, a transposed read there changes nothing
        assert sub.max() == 0.0 and not ref.l_val[i][:, :geo.rme].any() and not ref.l_bnd[i][:, :geo.rme].any()
    else:
        assert r != c and r < geo.rme and c < geo.rme
        bad = good.copy()
        bad[selpat.pos((i + 1) * bs + r, i * bs + c)] = good[selpat.pos((i + 1) * bs + c, i * bs + r)]
        a, where, _ = T.check_selinv(ref, selpat, bad)
        seen["coupling transposed"] = (a, 0.0)
        assert a > 1.0 and where == (i, T.REGIONS[4], r, c), (name, a, where)
    # the two slots of a symmetric pair swapped with the neighbouring pair's
    r = int(ref.rows[1][3])
    step = np.abs(np.diff(ref.d_val[1][3])).astype(np.float64)
    step[max(r - 1, 0):r + 1] = 0.0                         # (not the diagonal entry's own pair)
    c = int(np.argmax(step))
    assert r not in (c, c + 1) and step[c] > 0.0
    bad = good.copy()
    for (a0, b0), (a1, b1) in (((r, c), (r, c + 1)), ((c, r), (c + 1, r))):
        p0, p1 = selpat.pos(bs + a0, bs + b0), selpat.pos(bs + a1, bs + b1)
        bad[p0], bad[p1] = good[p1], good[p0]
    a = T.check_selinv(ref, selpat, bad)[0]
    seen["pair swapped"] = (a, 0.0)
    assert a > 1.0, (name, a)
    # one problem of a batch given another problem's values
    _, X1, C1 = _oracle_factor(name, 1)
    other, other_var = _values(name, X1, C1)
    a, v = T.check_selinv(ref, selpat, other)[0], T.check_var(ref, other_var)[0]
    seen["another problem"] = (a, v)
    assert a > 1.0 and v > 1.0
    assert T.truth_selinv(T.truth(name, 0), selpat, other) > T.TRUTH_FACTOR and T.truth_var(T.truth(name, 0), other_var) > T.TRUTH_FACTOR
    _say(capsys, f"TAKAHASHI_DEFECTS {name}: " + ", ".join(f"{k} {max(v):.1e}" for k, v in seen.items()))


def test_ratios_can_fail():
    """A value where the bound is zero must be exactly zero, and a NaN never passes."""
    val, bnd = np.zeros(3, T.LD), np.array([0.0, 1e-16, 1e-16])
    assert T._ratios(np.array([0.0, 5e-17, -5e-17]), val, bnd).max() <= 1.0
    assert T._ratios(np.array([1e-300, 0.0, 0.0]), val, bnd).max() == np.inf
    assert T._ratios(np.array([0.0, np.nan, 0.0]), val, bnd).max() == np.inf
    assert T._ratios(np.array([0.0, 2e-16, 0.0]), val, bnd).max() > 1.0
