"""GPU pins of the Takahashi recurrence (marginal_var("exact"), selected_inverse, trace_inv, the twisted order's exact variances)
on every coupling-window geometry of tests/takahashi_ref.py, at batch 1, 3 and 9.

Reference A: the longdouble recurrence on the handle's own X_i (BLOCK_LINV) and C_i (BLOCK_C), read after the calls, with its
entrywise bound: every checked entry of every problem and block within it.  Reference B: Q^-1 in longdouble, on the correlation
scale, at 4 cond_2(Q) 2^-52: the float64 recurrence of tests/selinv_oracle.py meets 1 cond 2^-52 (tests/test_takahashi_ref_cpu.py);
the kernels get a factor 4 over it because they sum in another order and read X from another block algorithm.  The rows checked:
0, 63, 64, rmax - 1, rmax, bs - 1 and 16 seeded ones of every block, all their columns, and the whole diagonal.

Each run (case, batch) is made once and shared by the tests that look at it."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import takahashi_ref as T
from tests.potrf_ref import SLACK

pytestmark = pytest.mark.gpu

RUNS = [(name, B) for name in T.CASES for B in ((3, 9) if name == "split512" else (1, 3, 9))]
RUN_IDS = [f"{name}-b{B}" for name, B in RUNS]
TWISTED = [(name, meet) for name in T.TWISTED_CASES for meet in ("auto", "first", "last")]
_RUNS = {}


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _q_csr(name):
    S = sp.csr_matrix(T.matrix(name, 0)[0])
    S.sort_indices()
    return S


def _run(pkg, name, B):
    """Factor the case's B problems, run the calls with the GEMM classes recorded, read the factor back, measure everything."""
    if (name, B) in _RUNS:
        return _RUNS[(name, B)]
    cabi = pkg._cabi
    geo, selpat = T.geometry(name), T.sel_pattern(name)
    mats = [T.matrix(name, p) for p in range(B)]
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.factor(mats[0][0], geo.N, values=np.stack([M.data for M, _ in mats]) if B > 1 else None)
    rec = dict(layout_before=F.get_layout().copy())
    Sd, Sq = pkg.CsrMatrix(selpat.csr()), _q_csr(name)
    Sqd = pkg.CsrMatrix(Sq)
    F.set_profiling(1)
    vals = F.selected_inverse(Sd)
    vals = (vals.data if B == 1 else vals).reshape(B, selpat.nnz)
    var = F.marginal_var("exact").reshape(B, geo.n)
    rec["classes"] = sorted({s["class"] for s in F.gemm_shapes()})
    F.set_profiling(0)
    rec["layout_after"] = F.get_layout().copy()
    # the sub-pattern of Q itself, and traces on it
    sub = F.selected_inverse(Sqd)
    sub = (sub.data if B == 1 else sub).reshape(B, Sq.nnz)
    qr = np.repeat(np.arange(geo.n), np.diff(Sq.indptr))
    rec["sub_same"] = bool(np.array_equal(sub, vals[:, selpat.pos(qr, Sq.indices)]))
    dv = np.random.default_rng([5, B, geo.n]).standard_normal((B, 3, Sq.nnz))
    tr = np.asarray(F.trace_inv(Sqd, dv if B > 1 else dv[0])).reshape(B, 3)
    want = np.einsum("pe,pje->pj", sub.astype(T.LD), dv.astype(T.LD))
    mag = np.einsum("pe,pje->pj", np.abs(sub), np.abs(dv))
    g_nnz = Sq.nnz * T.U / (1.0 - Sq.nnz * T.U)
    rec["trace"] = float((np.abs(tr.astype(T.LD) - want).astype(np.float64) / (g_nnz * mag * SLACK)).max())
    # the factor as the calls read it (a split handle holds full inverses by now), problem by problem
    rec.update(a_sel=[], a_var=[], b_sel=[], b_var=[], upper_zero=True, regions=dict.fromkeys(T.REGIONS, 0.0))
    for p in range(B):
        F.select_problem(p)
        Xs = [F.get_block(cabi.BLOCK_LINV, i) for i in range(geo.N)]
        Cs = [F.get_block(cabi.BLOCK_C, i) for i in range(geo.N - 1)]
        rec["upper_zero"] &= all(not np.triu(X, 1).any() for X in Xs)
        ref = T.ReferenceA(geo, Xs, Cs)
        worst, where, by_region = T.check_selinv(ref, selpat, vals[p])
        rec["a_sel"].append((worst, where))
        for k, v in by_region.items():
            rec["regions"][k] = max(rec["regions"][k], v)
        rec["a_var"].append(T.check_var(ref, var[p]))
        tru = T.truth(name, p)
        assert tru.resid <= 1e-17, (name, p, tru.resid)
        rec["b_sel"].append(T.truth_selinv(tru, selpat, vals[p]))
        rec["b_var"].append(T.truth_var(tru, var[p]))
    F.close()
    _RUNS[(name, B)] = rec
    return rec


@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_selected_inverse_within_reference_a(pkg, name, B, capsys):
    rec = _run(pkg, name, B)
    worst = max(rec["a_sel"], key=lambda t: t[0])
    _say(capsys, f"TAKAHASHI_A selinv {name} batch {B}: worst error / bound {worst[0]:.4f} at (step, region, row, column) {worst[1]}; "
                 "by region " + ", ".join(f"{k} {v:.4f}" for k, v in rec["regions"].items()))
    assert len(rec["a_sel"]) == B and rec["upper_zero"]
    for p, (ratio, where) in enumerate(rec["a_sel"]):
        assert ratio <= 1.0, (name, B, "problem", p, ratio, where)


@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_exact_variances_within_reference_a(pkg, name, B, capsys):
    rec = _run(pkg, name, B)
    worst = max(rec["a_var"], key=lambda t: t[0])
    _say(capsys, f"TAKAHASHI_A var {name} batch {B}: worst error / bound {worst[0]:.4f} at (step, region, index) {worst[1]}; "
                 f"trace_inv error / bound {rec['trace']:.4f}")
    for p, (ratio, where) in enumerate(rec["a_var"]):
        assert ratio <= 1.0, (name, B, "problem", p, ratio, where)
    assert rec["sub_same"], (name, B, "the pattern of Q gives other bits than the dense pattern at the shared entries")
    assert rec["trace"] <= 1.0, (name, B, rec["trace"])


@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_against_the_inverse(pkg, name, B, capsys):
    rec = _run(pkg, name, B)
    _say(capsys, f"TAKAHASHI_B {name} batch {B}: error / (cond 2^-52), selected inverse {max(rec['b_sel']):.3f}, variances {max(rec['b_var']):.3f}")
    for p in range(B):
        assert rec["b_sel"][p] <= T.TRUTH_FACTOR and rec["b_var"][p] <= T.TRUTH_FACTOR, (name, B, "problem", p, rec["b_sel"][p], rec["b_var"][p])


@pytest.mark.parametrize("name,B", RUNS, ids=RUN_IDS)
def test_kernel_families_and_layout(pkg, name, B, capsys):
    """Batch 1 runs the recurrence's products on the 32 x 32-tile kernel (class 13), batch 9 is past its limit of 8 problems and
    runs them on the LDS-DMA kernels (14, 15, 18); split512's batches hold their inverses split at 256 until the first call."""
    rec = _run(pkg, name, B)
    geo = T.geometry(name)
    _say(capsys, f"TAKAHASHI_CLASSES {name} batch {B}: GEMM classes {rec['classes']}, split before / after {rec['layout_before'][-1]} / {rec['layout_after'][-1]}")
    lay = rec["layout_after"]
    if geo.N > 1:
        assert (int(lay[0]), int(lay[1])) == (geo.cmin, geo.rmax) and [int(v) for v in lay[3:3 + int(lay[2])]] == geo.kst[:geo.rmax // 64]
    if name == "split512":
        assert rec["layout_before"][-1] == 256 and rec["layout_after"][-1] == 0
    else:
        assert rec["layout_before"][-1] == 0 and rec["layout_after"][-1] == 0
    if B == 1:
        assert 13 in rec["classes"]
    if B == 9:
        assert 13 not in rec["classes"] and set(rec["classes"]) & {14, 15, 18}


@pytest.mark.parametrize("name,meet", TWISTED, ids=[f"{n}-{m}" for n, m in TWISTED])
def test_twisted_exact_variances_against_the_inverse(pkg, name, meet, capsys):
    """Two chains that meet in a block: each half runs the recurrence on its own window (window5rev: the top half sees the
    mirrored one), the bottom half seeded by the meeting block."""
    geo = T.geometry(name)
    Q, _ = T.matrix(name, 0)
    m = {"auto": None, "first": 0, "last": geo.N - 1}[meet]
    F = pkg.TridiagonalCholeskyFactor(order="twisted", meet=m)
    F.factor(Q, geo.N)
    assert F.order == "twisted" and (m is None or F.meet == m)
    var = F.marginal_var("exact")
    ratio = T.truth_var(T.truth(name, 0), var)
    _say(capsys, f"TAKAHASHI_B twisted {name} meet {meet} ({F.meet}): variances, error / (cond 2^-52) {ratio:.3f}")
    F.close()
    assert ratio <= T.TRUTH_FACTOR, (name, meet, ratio)
