"""Envelope K bounds of the batched factorisation (round 19): the panel products and rank-256 updates of the 256-column panels,
and the backward sweep's L_ba^T product, skip the 64-wide K units in which the rows that S = D_i - C C^T left as D_i's are still
exact zeros (GemmArgs::ke_m beside kb_m / kb_n / ke_n).  set_eager bit 21 switches the bounds off.

Checked: the kernel with the bounds against the same kernel without them on zeroed operands (bitwise) and against NumPy; the
bounds the handle computed against tests/envelope_ref.py; factor, forward solve and fused posterior bitwise with and without
bit 21 and against the oracle; the K units booked; a workload without such structure.

The bounds are hints for the LDS-DMA kernels: launches of at most 128 tiles of a batch of at most 8 run on the 32 x 32 kernel,
which gets none and carries no tail row either.  darcy128 at batch 4 and darcy256 at batch 2 are such batches for most of their
launches, so the leading blocks of both at batch 9 are checked as well: there every launch takes the bounds and the tails ride."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O
from tests import envelope_ref as E
from tests import gemm_desc_ref as R
from tests.test_gpu_parity import TOL_FACTOR

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch
T3 = 2.0 * 64.0 ** 3


# ------------------------------------------------------------------------------------------------ kernel level
def _env_call(lib, pkg, d, route, buf, kb_m=None, ke_m=None, grouped=0):
    def pn(a):
        return (pkg._cabi.ptr(a), 0 if a is None else a.size)
    desc = d.desc_array()
    abt = np.array([d.alpha, d.beta, d.tbeta])
    fam = C.c_int32(-1)
    kb = None if kb_m is None else np.asarray(kb_m, np.int32)
    ke = None if ke_m is None else np.asarray(ke_m, np.int32)
    args = []
    for a in (buf["A"], buf["B"], buf["C"], None, buf.get("tA"), buf.get("tC"), None, kb, None, None, ke):
        args += list(pn(a))
    pkg._cabi.check(lib.gmrf_test_gemm_env(0, route, pkg._cabi.ptr(desc), pkg._cabi.ptr(abt), *args, grouped, C.byref(fam)))
    return fam.value


def _buffers(d, A, B, C0, tA, tC0):
    """Flat buffers of the descriptor's layout from per-problem logical operands (gaps hold zeros)."""
    sz, ix = R.need(d), R.index_maps(d)
    buf = {k: np.zeros(sz[k]) for k in ("A", "B", "C")}
    for z in range(d.batch):
        buf["A"][ix["A"][z]] = A[z]
        buf["B"][ix["B"][z]] = B[z]
        buf["C"][ix["C"][z]] = C0[z]
    if d.tail == 2:
        buf["tA"], buf["tC"] = np.zeros(sz["tA"]), np.zeros(sz["tC"])
        for z in range(d.batch):
            buf["tA"][ix["tA"][z]] = tA[z]
            buf["tC"][ix["tC"][z]] = tC0[z]
    return buf


M_, N_, K_, BATCH = 128, 64, 128, 3
KB_M, KE_M = (0, 64), (64, 128)


@pytest.mark.parametrize("tail,grouped", [(0, 0), (2, 0), (0, 1), (0, 2)], ids=["plain", "tail", "grouped_first", "grouped_second"])
@pytest.mark.parametrize("b_n", [0, 1])
def test_kernel_skips_what_the_bounds_exclude(lib, pkg, b_n, tail, grouped):
    """64 x 64 tile, M = 128, N = 64, K = 128, batch 3, kb_m = [0, 64], ke_m = [64, 128]: A holds 1e30 outside the bounded ranges.
    The tail row (operands of its own) rides in the last row tile, whose K range [64, 128) is then the tail's; a grouped launch
    (gemm_f64_dma_grouped, the descriptor as its first / second product) carries none."""
    d = R.make(M_, N_, K_, "stack", b_n=b_n, batch=BATCH, alpha=-1.0, beta=1.0, tbeta=1.0, tail=tail)
    rng = np.random.default_rng(190 + 2 * b_n + tail)
    A = rng.standard_normal((BATCH, M_, K_)); B = rng.standard_normal((BATCH, K_, N_)); C0 = rng.standard_normal((BATCH, M_, N_))
    tA = rng.standard_normal((BATCH, K_)); tC0 = rng.standard_normal((BATCH, N_))
    inside = np.zeros((M_, K_), bool)
    for t in range(M_ // 64):
        inside[64 * t:64 * t + 64, KB_M[t]:KE_M[t]] = True
    t_inside = np.zeros(K_, bool); t_inside[KB_M[-1]:KE_M[-1]] = True
    A_zero, A_big = np.where(inside, A, 0.0), np.where(inside, A, 1e30)
    tA_zero, tA_big = np.where(t_inside, tA, 0.0), np.where(t_inside, tA, -1e30)
    route, fam = (R.TAIL, R.FAM_TAIL) if tail else (R.DMA64, R.FAM_DMA64)
    bounded = _buffers(d, A_big, B, C0, tA_big, tC0)
    plain = _buffers(d, A_zero, B, C0, tA_zero, tC0)
    assert _env_call(lib, pkg, d, route, bounded, KB_M, KE_M, grouped) == fam
    assert _env_call(lib, pkg, d, route, plain, None, None, grouped) == fam
    outs = ("C", "tC") if tail else ("C",)
    for nm in outs:
        assert np.array_equal(bounded[nm].view(np.uint64), plain[nm].view(np.uint64)), nm
    # NumPy, to the tolerance of tests/test_gpu_gemm_desc.py (gemm_desc_ref.within)
    L = np.longdouble
    ix = R.index_maps(d)
    for z in range(BATCH):
        ref = C0[z].astype(L) - A_zero[z].astype(L) @ B[z].astype(L)
        mag = (np.abs(A_zero[z]) @ np.abs(B[z]) + np.abs(C0[z])) * (1.0 + 2.0 ** -40)
        got = bounded["C"][ix["C"][z]]
        print(f"z={z} worst error / bound: {R.worst(got, ref, mag, K_):.3f}")
        assert R.within(got, ref, mag, K_), z
        if tail:
            tref = tC0[z].astype(L) - tA_zero[z].astype(L) @ B[z].astype(L)
            tmag = (np.abs(tA_zero[z]) @ np.abs(B[z]) + np.abs(tC0[z])) * (1.0 + 2.0 ** -40)
            assert R.within(bounded["tC"][ix["tC"][z]], tref, tmag, K_), z


# ------------------------------------------------------------------------------------------------ factor
def _leading(w, nb):
    m = nb * w.block_size
    Q = sp.csc_matrix(w.Q[:m, :m])
    Q.sort_indices()
    return Q, np.ascontiguousarray(w.rhs[:m]), nb


def _fwd_state(pkg, F):
    st = C.c_int32(-1)
    y = np.empty((F.batch, F.N), dtype=np.float64)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_factor_fwd(F._h, C.byref(st), pkg._cabi.ptr(y)))
    return int(st.value), y


def _blocks(F, idx, probs):
    out = []
    for p in probs:
        F.select_problem(p)
        for i in idx:
            out.append(F.get_block(2, i))                  # Linv_i
            if i > 0:
                out.append(F.get_block(1, i - 1))          # C_i
        out.append(np.array([F.logdet()]))
    F.select_problem(0)
    return out


# (workload, leading blocks or None, batch, blocks read back, must the tails ride?)
FCASES = {"darcy128_b4": ("darcy128", None, 4, (0, 1, 31), False), "darcy256_b2": ("darcy256", None, 2, (0, 1, 63), False),
          "darcy128_leading3_b9": ("darcy128", 3, 9, (0, 1, 2), True), "darcy256_leading3_b9": ("darcy256", 3, 9, (0, 1, 2), True)}
_W = {}


def _workload(pkg, name):
    if name not in _W:
        _W[name] = pkg.workloads.darcy(int(name[5:]))
    return _W[name]


@pytest.fixture(scope="module", params=list(FCASES))
def fcase(request, pkg):
    """One handle per case, factored with and without a registered right-hand side, with and without bit 21: host copies only."""
    import torch
    name, nb, B, idx, tails = FCASES[request.param]
    w = _workload(pkg, name)
    Q, rhs, nb = _leading(w, nb) if nb else (w.Q, np.ascontiguousarray(w.rhs), w.n_blocks)
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
    probs = (0, B - 1)
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    got = {}
    F.factor(Q, nb, values=vals)
    env = F.envelope()
    for with_rhs in (False, True):
        F.set_factor_rhs(b if with_rhs else None)
        for bits in (0, Switch.NO_ENVELOPE):
            F.set_eager(bits)
            F.refactor(vals)
            st, y = _fwd_state(pkg, F)
            ld = F.logdet_batch()
            ld = ld.cpu().numpy() if hasattr(ld, "cpu") else np.asarray(ld)
            got[(with_rhs, bits)] = (_blocks(F, idx, probs), st, y, ld.copy())
    F.set_eager(0)
    F.close()
    return w, Q, nb, B, idx, tails, vals, env, got, probs


def test_bounds_are_the_patterns(fcase):
    w, Q, nb, B, idx, tails, vals, (lo, hi, state), got, probs = fcase
    lo_py, hi_py = E.envelope(Q, nb)
    assert state == 2
    assert np.array_equal(lo.reshape(lo_py.shape), lo_py) and np.array_equal(hi.reshape(hi_py.shape), hi_py)


def test_factor_and_forward_solve_bitwise_with_and_without_the_bounds(fcase):
    w, Q, nb, B, idx, tails, vals, env, got, probs = fcase
    for with_rhs in (False, True):
        blocks_on, st_on, y_on, ld_on = got[(with_rhs, 0)]
        blocks_off, st_off, y_off, ld_off = got[(with_rhs, Switch.NO_ENVELOPE)]
        assert st_on == st_off == (1 if (with_rhs and tails) else st_on)
        if not with_rhs:
            assert st_on == 0
        assert len(blocks_on) == len(blocks_off)
        assert all(np.array_equal(a.view(np.uint64), c.view(np.uint64)) for a, c in zip(blocks_on, blocks_off))
        assert np.array_equal(ld_on.view(np.uint64), ld_off.view(np.uint64))
        if st_on == 1:
            assert np.array_equal(y_on.view(np.uint64), y_off.view(np.uint64))
    # and a registered right-hand side changes no bit of the factor
    assert all(np.array_equal(a, c) for a, c in zip(got[(False, 0)][0], got[(True, 0)][0]))


def test_factor_against_the_oracle(fcase):
    """As tests/test_gpu_grouped_gemm.py compares them; the oracle factors the leading blocks, which are the chain's own."""
    w, Q, nb, B, idx, tails, vals, env, got, probs = fcase
    lead = [i for i in idx if i < 3]
    m = 3 * w.block_size
    per = len(got[(True, 0)][0]) // len(probs)
    for k, p in enumerate(probs):
        Qp = sp.csc_matrix(Q.copy()); Qp.data = vals[p].copy()
        Fo = O.tridiagonal_cholesky(sp.csc_matrix(Qp[:m, :m]), 3)
        blocks = got[(True, 0)][0][k * per:(k + 1) * per]
        at = 0
        for i in idx:
            X = blocks[at]; at += 1
            Ci = None
            if i > 0:
                Ci = blocks[at]; at += 1
            if i not in lead:
                continue
            Xo = np.linalg.inv(Fo.chos[i])
            assert np.max(np.abs(np.tril(X) - Xo)) / np.max(np.abs(Xo)) < TOL_FACTOR
            if Ci is not None:
                assert np.max(np.abs(Ci - Fo.Cs[i - 1])) / np.max(np.abs(Fo.Cs[i - 1])) < TOL_FACTOR
        if nb == 3:
            ld = O.logdet(Fo)
            assert abs(blocks[-1][0] - ld) <= TOL_FACTOR * abs(ld)


# ------------------------------------------------------------------------------------------------ fused posterior
@pytest.mark.parametrize("name,nb,B", [("darcy128", None, 32), ("darcy256", 3, 9)], ids=["darcy128_b32", "darcy256_leading3_b9"])
def test_fused_posterior_bitwise(pkg, name, nb, B):
    """k = 64: mean and samples with and without bit 21.  darcy256's factor is kept in the split form (p = 256), whose backward
    sweep multiplies with L[256:, 0:256]: the product that takes ke_n from the envelope."""
    import torch
    w = _workload(pkg, name)
    Q, rhs, nb = _leading(w, nb) if nb else (w.Q, np.ascontiguousarray(w.rhs), w.n_blocks)
    vals = np.stack([Q.data * (1.0 + 0.01 * p) for p in range(B)])
    b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.set_keep_l(False)
    F.set_factor_rhs(b)
    out = {}
    F.factor(Q, nb, values=vals)
    for bits in (0, Switch.NO_ENVELOPE):
        F.set_eager(bits)
        F.refactor(vals)
        mu, X = F.posterior_batch(b, 64, seed=19, first_id=7)
        assert F.stats()["sample_ms"] == 0.0               # the fused pass
        out[bits] = (mu.cpu().numpy().copy(), X.cpu().numpy().copy())
    F.close()
    assert np.array_equal(out[0][0].view(np.uint64), out[Switch.NO_ENVELOPE][0].view(np.uint64))
    assert np.array_equal(out[0][1].view(np.uint64), out[Switch.NO_ENVELOPE][1].view(np.uint64))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()


# ------------------------------------------------------------------------------------------------ work
def _profiled(F, vals):
    F.set_profiling(1)
    F.refactor(vals)
    shapes = F.gemm_shapes()
    F.set_profiling(0)
    return shapes


def _row(shapes, M, N, K, lower):
    rows = [g for g in shapes if (g["M"], g["N"], g["K"], g["lower_only"]) == (M, N, K, lower)]
    assert len(rows) == 1, rows
    return rows[0]


@pytest.mark.parametrize("with_rhs", [False, True], ids=["no_tail", "tail_riding"])
def test_k_units_booked(pkg, with_rhs):
    """darcy256, three leading blocks, batch 9: the first panel's product (768 x 256 x 256) and update (768^2 lower, K = 256) book
    the K units the bounds leave -- per block behind the first 120 -> 90 (99 with the tail riding) and 312 -> 244."""
    import torch
    nb, B = 3, 9
    w = _workload(pkg, "darcy256")
    Q, rhs, nb = _leading(w, nb)
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    if with_rhs:
        F.set_factor_rhs(torch.from_numpy(np.stack([rhs] * B)).cuda())
    F.factor(Q, nb, values=vals)
    on = _profiled(F, vals)
    F.set_eager(Switch.NO_ENVELOPE)
    off = _profiled(F, vals)
    F.close()
    lo, hi = E.envelope(Q, nb)
    assert E.units(lo, hi, 1, 0, with_rhs) == E.units(lo, hi, 2, 0, with_rhs) == ((99 if with_rhs else 90), 244)
    rows = 769 if with_rhs else 768                        # (a launch with a tail row is booked with its M + 1 rows)
    scale = T3 * B * rows / 768.0
    want_pp = sum(E.units(lo, hi, i, 0, with_rhs)[0] for i in range(nb))
    want_upd = sum(E.units(lo, hi, i, 0, with_rhs)[1] for i in range(nb))
    for shapes, pp, upd, flag in ((on, want_pp, want_upd, 1), (off, 120 * nb, 312 * nb, 0)):
        r_pp, r_upd = _row(shapes, rows, 256, 256, 0), _row(shapes, rows, 768, 256, 1)
        print("panel product", r_pp, "update", r_upd)
        assert r_pp["launches"] == r_upd["launches"] == nb and r_pp["k_bounds"] == r_upd["k_bounds"] == flag
        assert abs(r_pp["flops"] - scale * pp) <= 1e-9 * scale * pp
        assert abs(r_upd["flops"] - scale * upd) <= 1e-9 * scale * upd
    # the later panels have no such rows below them: the same launches either way
    later_on = sorted((g["M"], g["N"], g["K"], g["launches"], g["flops"], g["k_bounds"]) for g in on if g["M"] not in (768, 769))
    later_off = sorted((g["M"], g["N"], g["K"], g["launches"], g["flops"], g["k_bounds"]) for g in off if g["M"] not in (768, 769))
    assert later_on == later_off


# ------------------------------------------------------------------------------------------------ no structure
def test_trivial_bounds_launch_as_before(pkg):
    Q = E.no_structure_chain()
    nb, B = 3, 9
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    F = pkg.TridiagonalCholeskyFactor(batch=B)
    F.factor(Q, nb, values=vals)
    lo, hi, state = F.envelope()
    lo_py, hi_py = E.envelope(Q, nb)
    assert state == 1 and np.array_equal(lo.reshape(lo_py.shape), lo_py) and np.array_equal(hi.reshape(hi_py.shape), hi_py)
    on_blocks = _blocks(F, range(nb), (0, B - 1))
    on = _profiled(F, vals)
    F.set_eager(Switch.NO_ENVELOPE)
    F.refactor(vals)
    off_blocks = _blocks(F, range(nb), (0, B - 1))
    off = _profiled(F, vals)
    F.close()

    def key(shapes):
        return sorted((g["class"], g["M"], g["N"], g["K"], g["tri"], g["lower_only"], g["problems"], g["k_bounds"], g["launches"], g["flops"])
                      for g in shapes)
    assert key(on) == key(off)
    assert all(np.array_equal(a.view(np.uint64), c.view(np.uint64)) for a, c in zip(on_blocks, off_blocks))
