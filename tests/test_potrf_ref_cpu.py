"""CPU checks of the in-block Cholesky reference (tests/potrf_ref.py) on every case the GPU tests run
(tests/test_gpu_potrf_routes.py registers them): float64 restatements of each route's arithmetic meet the derived bounds, five
mutations of their outputs break them, the inputs are positive definite by a margin, and the sampled rows cover every 16-row
group.  This is what keeps the bounds honest: they were derived, not fitted, and a bound no mutation can break checks nothing."""
from dataclasses import replace

import numpy as np
import pytest

from tests import potrf_ref as R
from tests import test_gpu_potrf_routes as G


def _all_cases():
    out = []
    for name, fn, test in G.CASES:
        for n, ps in enumerate(G.param_sets(test)):
            for i, c in enumerate(fn(**ps)):
                out.append((f"{name}-{n}-{i}", c))
    return out


ALL = _all_cases()


def _problems():
    """Every distinct (form, problem) of the GPU cases, with the problem next to it in its batch (or the one a batch would
    put there) as the neighbour."""
    seen = {}
    for cid, c in ALL:
        probs = c.probs if c.batch > 1 else R.problems(c.family, c.n, c.seed, 2)
        form = replace(c.form, persist=0)          # (the persistent launches do the arithmetic of the launches they replace)
        for p in range(c.batch):
            seen.setdefault((form, probs[p]), (f"{cid}-p{p}", form, probs[p], probs[(p + 1) % len(probs)]))
    return list(seen.values())


PROBLEMS = _problems()
# the mutations: once per form, input family and size (not per seed and scale of a batch's problems)
MUTATED = list({(f, pr[0], pr[1]): (cid, f, pr, nb) for cid, f, pr, nb in reversed(PROBLEMS)}.values())[::-1]
_OUT = {}


def restated(form, prob):
    key = (form, prob)
    if key not in _OUT:
        L, X = R.restate(form, R.matrix(prob))
        L.setflags(write=False)
        X.setflags(write=False)
        _OUT[key] = (L, X)
    return _OUT[key]


def test_every_gpu_test_registers_its_cases():
    registered = {name for name, _, _ in G.CASES}
    tests = {n for n in dir(G) if n.startswith("test_")}
    assert tests - registered == {"test_bad_arguments_launch_nothing"}
    assert len(ALL) > 150 and len(PROBLEMS) > 60
    routes = {(c.form.route, c.form.persist, c.form.inv) for _, c in ALL}
    assert {r for r, _, _ in routes} == {1, 2, 3, 4} and {p for _, p, _ in routes} == {0, 1, 2, 3}
    assert {(3, 3, "panel_persist"), (3, 0, "panel_diag128")} <= routes
    assert {c.form.xsplit for _, c in ALL} == {0, 256, 512} and any(c.form.in_slot for _, c in ALL)
    assert {c.form.kmax for _, c in ALL if c.form.route == R.ROUTE_STEPS and c.n >= 512} == {128, 512}


def test_plan_is_the_host_code_on_its_landmarks():
    """The route predicate as csrc/gmrf_hip.hip states it (potrf_route, planned_xsplit, persist_demand)."""
    assert R.persist_tiles(16, 0, 16, 1) + 1 == 135 and R.persist_tiles(4, 0, 4, 2) + 1 == 7 and R.persist_tiles(32, 0, 4, 0) + 1 == 90
    assert R.plan(1024).route == R.ROUTE_FUSED and R.plan(2048).route == R.ROUTE_BIG_ONE
    assert R.plan(256, 36).persist == 3 and R.plan(256, 37).persist == 0
    assert R.plan(1024, 2, cmin=768).xsplit == 512 and R.plan(512, 2, cmin=192).xsplit == 0 and R.plan(256, 2, cmin=192).xsplit == 0
    assert R.plan(512, 2, cmin=256, keep_l=0).in_slot and not R.plan(1024, 2, cmin=512, keep_l=0).in_slot


@pytest.mark.parametrize("n", sorted({c.n for _, c in ALL if c.n >= 512}))
def test_row_set_covers_every_16_row_group(n):
    for seed in range(5):
        rows = R.row_set(n, seed)
        assert len(rows) == n // 16 and np.array_equal(rows // 16, np.arange(n // 16))
    assert not np.array_equal(R.row_set(n, 0), R.row_set(n, 1))


@pytest.mark.parametrize("prob", sorted({p for _, _, p, _ in PROBLEMS}), ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}-{p[3]:g}")
def test_inputs_are_positive_definite_by_a_margin(prob):
    """Every float64 pivot stays above 1e3 n u a_ii: info == 0 is the reference's own verdict on these inputs."""
    A = R.matrix(prob)
    n = A.shape[0]
    piv = np.diag(np.linalg.cholesky(A)) ** 2
    assert np.all(piv > 1e3 * n * R.U * np.diag(A)), float(np.min(piv / np.diag(A)))
    assert np.array_equal(A, A.T)


@pytest.mark.parametrize("cid, form, prob, neighbour", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_restatement_meets_the_bounds(cid, form, prob, neighbour):
    L, X = restated(form, prob)
    S0, L0, X0 = R.build_buffers([R.matrix(prob)])
    up, _ = R.tile_masks(form.n)
    Lb, Xb = np.where(up, -0.0, L), np.where(up, -0.0, X)
    assert not R.structure_errors(form, L0[0], X0[0], Lb, Xb)
    r = R.check(form, R.matrix(prob), L, X)
    assert all(v <= 1.0 for v in r.values()), r
    assert set(r) == ({"L", "X"} if form.n <= 256 else {"L", "X", "L_rows", "X_rows"})


def _fails(form, prob, L, X):
    r = R.check(form, R.matrix(prob), L, X, full=False)
    return any(not v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("cid, form, prob, neighbour", MUTATED, ids=[p[0] for p in MUTATED])
def test_mutations_break_the_bounds(cid, form, prob, neighbour):
    n, nt = form.n, form.nt
    rng = np.random.default_rng([n, form.route, form.kmax])
    L, X = restated(form, prob)
    p = form.xsplit
    # one tile of X left at its input value (NaN): the diagonal tile of a seeded tile row
    t = int(rng.integers(0, nt))
    Xm = X.copy()
    Xm[64 * t:64 * t + 64, 64 * t:64 * t + 64] = np.tril(np.full((64, 64), np.nan))
    assert _fails(form, prob, L, Xm)[0]
    # one 16 x 16 block of X transposed: a block strictly below the diagonal of an inverted part, next to the diagonal
    i = 16 * int(rng.integers(1, n // 16))
    while (p and i == p) or np.array_equal(X[i:i + 16, i - 16:i], X[i:i + 16, i - 16:i].T):     # (a sparse input's block can be symmetric)
        i = 16 + (i % (n - 16))
    Xm = X.copy()
    Xm[i:i + 16, i - 16:i] = X[i:i + 16, i - 16:i].T
    bad, r = _fails(form, prob, L, Xm)
    assert bad, ("transposed block", i, r)
    # one element of L scaled by 1 + 2^-36: the largest of a row of the sampled set (bs >= 512: where longdouble looks)
    rows = R.row_set(n) if n >= 512 else np.arange(n)
    i = int(rows[len(rows) // 2])
    Leff = R.clean(form, L, X)[0]
    j = int(np.argmax(np.abs(Leff[i, :i + 1])))
    Lm, Xm = L.copy(), X.copy()
    (Xm if (p and i >= p and j < p) else Lm)[i, j] *= 1.0 + 2.0 ** -36
    if p and i >= p and j < p and not form.in_slot:
        Lm[i, j] = Xm[i, j]
    bad, r = _fails(form, prob, Lm, Xm)
    assert bad, ("2^-36", i, j, r)
    if nt < 2:
        return
    # one tile of L taken from the neighbouring problem
    Ln = restated(R.plan(n), neighbour)[0] if form.in_slot else restated(form, neighbour)[0]
    r_, c_ = nt - 1, int(rng.integers(0, nt - 1))
    if form.in_slot and r_ >= 4 and c_ < 4:
        c_ = 4 if nt > 5 else c_
    Lm, Xm = L.copy(), X.copy()
    tgt = Xm if (form.in_slot and 64 * c_ < p) else Lm
    tgt[64 * r_:64 * r_ + 64, 64 * c_:64 * c_ + 64] = Ln[64 * r_:64 * r_ + 64, 64 * c_:64 * c_ + 64]
    if p and not form.in_slot and 64 * r_ >= p and 64 * c_ < p:
        Xm[64 * r_:64 * r_ + 64, 64 * c_:64 * c_ + 64] = Lm[64 * r_:64 * r_ + 64, 64 * c_:64 * c_ + 64]
    bad, r = _fails(form, prob, Lm, Xm)
    assert bad, ("neighbour's tile", r_, c_, r)
    # one rank-4 slice (one MFMA k-step) dropped from one trailing update of the last diagonal tile: the k-step that carries
    # the most there (the lattice inputs have k-steps of exact zeros, whose loss nothing can notice)
    w = (Leff[64 * (nt - 1):, :64 * (nt - 1)] ** 2).sum(axis=0).reshape(-1, 4).sum(axis=1)
    k = 4 * int(np.argmax(w))
    Ld, Xd = R.restate(form, R.matrix(prob), drop=(nt - 1, nt - 1, k // 64, k % 64))
    bad, r = _fails(form, prob, Ld, Xd)
    assert bad, ("dropped k-step", r)
