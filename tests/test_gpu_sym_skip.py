"""Strict-lower mode of the symmetric products (round 29, GemmArgs::strict_lower): on a diagonal tile of a triangular grid the
64 x 64 LDS-DMA kernels leave what lies strictly above the tile's block diagonal as C held it -- the six upper 16 x 16 MFMA blocks
with B stored [n][k] (the factor's symmetric products; the ten other blocks are dealt over the four waves), the quadrant rows
0 .. 31 x columns 32 .. 63 with B stored [k][n].

Kernel level, through gmrf_test_gemm_sym: the launch with the bit against the same launch without it, bit by bit, on a C that
holds a finite sentinel of its own in every element ("unchanged" cannot be mistaken for "rewritten with the same value").
Factor level: the batched factor with the process-wide hook gmrf_test_strict_lower on and off in fresh handles (the hook is
read when a factor graph is captured), against the oracle, and after a factorisation of other values in the same handle
(nothing a factorisation leaves above the diagonal of S reaches an output of the next).  tests/sym_skip_ref.py states the masks."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import __graft_entry__
from oracle import bt_oracle as O
from tests import gemm_desc_ref as R
from tests import sym_skip_ref as S
from tests.test_gpu_parity import TOL_FACTOR

pytestmark = pytest.mark.gpu

Switch = __graft_entry__.load_package().Switch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ kernel level
def _sym_call(lib, pkg, d, route, buf, strict, kb=None, grouped=0):
    def pn(a):
        return (pkg._cabi.ptr(a), 0 if a is None else a.size)
    desc = d.desc_array()
    abt = np.array([d.alpha, d.beta, d.tbeta])
    fam = C.c_int32(-1)
    kbv = None if kb is None else np.asarray(kb, np.int32)
    args = []
    for a in (buf["A"], buf["B"], buf["C"], None, buf.get("tA"), buf.get("tC"), None, kbv, kbv, None, None):
        args += list(pn(a))
    pkg._cabi.check(lib.gmrf_test_gemm_sym(0, route, pkg._cabi.ptr(desc), pkg._cabi.ptr(abt), *args, grouped, int(strict), C.byref(fam)))
    return fam.value


def _operands(d, seed, kb=None):
    """Flat buffers of the descriptor's layout: random A (real zeros left of kb per row tile), B = the same operand (a symmetric
    product), C = a finite sentinel per element, gaps included; the tail's operands of its own."""
    rng = np.random.default_rng(seed)
    sz, ix = R.need(d), R.index_maps(d)
    buf = {"A": np.zeros(sz["A"]), "B": np.zeros(sz["B"]), "C": 1000.0 + 0.25 * np.arange(sz["C"], dtype=np.float64)}
    for z in range(d.batch):
        a = rng.standard_normal((d.M, d.K))
        if kb is not None:
            for t in range(d.M // 64):
                a[64 * t:64 * t + 64, :kb[t]] = 0.0
        buf["A"][ix["A"][z]] = a
        buf["B"][ix["B"][z]] = a.T                               # op(B) = A^T (either storage: the index map is [k][n])
    if d.tail == 2:
        buf["tA"] = np.zeros(sz["tA"]); buf["tC"] = 500.0 + 0.5 * np.arange(sz["tC"], dtype=np.float64)
        for z in range(d.batch):
            buf["tA"][ix["tA"][z]] = rng.standard_normal(d.K)
    return buf


def _check_launch(lib, pkg, d, seed, kb=None, grouped=0):
    route, fam = (R.TAIL, R.FAM_TAIL) if d.tail else (R.DMA64, R.FAM_DMA64)
    M = d.M
    ix = R.index_maps(d)
    start = _operands(d, seed, kb)
    off = {k: v.copy() for k, v in start.items()}
    on = {k: v.copy() for k, v in start.items()}
    assert _sym_call(lib, pkg, d, route, off, 0, kb, grouped) == fam
    assert _sym_call(lib, pkg, d, route, on, 1, kb, grouped) == fam
    must, above, skip = S.must_write(M), ~S.may_write(M), S.skipped(M, d.b_n)
    rest = S.may_write(M) & ~must & ~skip
    for z in range(d.batch):
        c0, c_off, c_on = (_bits(b["C"][ix["C"][z]]) for b in (start, off, on))
        tag = (M, d.K, d.batch, d.beta, d.tail, d.b_n, z)
        assert np.array_equal(c_on[must], c_off[must]), tag                  # every element with row >= col keeps its bits
        assert np.array_equal(c_on[above], c0[above]), tag                   # tiles above the block diagonal: untouched
        assert np.array_equal(c_on[skip], c0[skip]), tag                     # the skipped blocks / quadrant: untouched
        assert np.array_equal(c_on[rest], c_off[rest]), tag                  # the rest of a diagonal tile: the no-bit result
        # and the launch without the bit did write that quadrant: the comparison above can tell
        assert not np.any(c_off[skip] == c0[skip]), tag
        assert np.isfinite(off["C"][ix["C"][z]]).all()
    # everything else in the buffer (the gaps between rows and problems) is as it was, in both
    expect = off["C"].copy()
    for z in range(d.batch):
        e = expect[ix["C"][z]]
        e[skip] = start["C"][ix["C"][z]][skip]
        expect[ix["C"][z]] = e
    assert np.array_equal(_bits(on["C"]), _bits(expect))
    if d.tail:
        assert np.array_equal(_bits(on["tC"]), _bits(off["tC"]))             # the tail row: the same eight partial sums
        for z in range(d.batch):
            assert not np.any(_bits(on["tC"][ix["tC"][z]]) == _bits(start["tC"][ix["tC"][z]]))


@pytest.mark.parametrize("tail", [0, 2], ids=["plain", "tail"])
@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
@pytest.mark.parametrize("batch", [1, 9], ids=["b1", "b9"])
@pytest.mark.parametrize("b_n", [0, 1], ids=["B_nk", "B_kn"])
def test_kernel_leaves_the_upper_part_and_keeps_every_lower_bit(lib, pkg, b_n, batch, beta, tail):
    """B stored [n][k] (the symmetric products' layout) and [k][n], M = N in {64, 128, 192}, K in {16, 64, 256}; nine problems
    walk the nz % 8 != 0 tile order.  The tail rides on operands of its own, as the factor's forward solve does on triangular grids."""
    for M in (64, 128, 192):
        for K in (16, 64, 256):
            d = R.make(M, M, K, "stack", b_n=b_n, lower_only=1, batch=batch, alpha=-1.0, beta=beta, tbeta=1.0, tail=tail)
            _check_launch(lib, pkg, d, seed=2900 + M + K + batch)


@pytest.mark.parametrize("tail", [0, 2], ids=["plain", "tail"])
@pytest.mark.parametrize("batch", [9, 8], ids=["b9", "b8_xcd_groups"])
def test_kernel_with_staircase_bounds(lib, pkg, batch, tail):
    """kb_m = kb_n = (0, 64, 128), K = 256 -- G2's staircase: rows ascending, tile (b, b) starts at 64 b, as the tail's column does."""
    d = R.make(192, 192, 256, "stack", b_n=0, lower_only=1, batch=batch, alpha=-1.0, beta=1.0, tbeta=1.0, tail=tail)
    _check_launch(lib, pkg, d, seed=2950 + batch, kb=(0, 64, 128))


@pytest.mark.parametrize("grouped", [1, 2], ids=["first", "second"])
def test_kernel_as_a_product_of_the_grouped_launch(lib, pkg, grouped):
    """128^2, K = 128, batch 9, beta = 1: the S_BB update as descriptor 0 (and 1) of gemm_f64_dma_grouped."""
    d = R.make(128, 128, 128, "stack", b_n=0, lower_only=1, batch=9, alpha=-1.0, beta=1.0)
    _check_launch(lib, pkg, d, seed=2970, grouped=grouped)


def test_other_kernels_take_the_bit_and_write_whole_tiles(lib, pkg):
    """The register-staged 64 x 64 kernel and the 32 x 32 one: the bit is allowed and changes nothing."""
    d = R.make(128, 128, 64, "stack", b_n=0, lower_only=1, batch=1, alpha=-1.0, beta=1.0)
    for route, fams in ((R.REG, (R.FAM_REG16, R.FAM_REG32)), (R.LL, (R.FAM_LL,))):
        start = _operands(d, 2980)
        off = {k: v.copy() for k, v in start.items()}
        on = {k: v.copy() for k, v in start.items()}
        assert (_sym_call(lib, pkg, d, route, off, 0) & 255) in fams
        assert (_sym_call(lib, pkg, d, route, on, 1) & 255) in fams
        assert np.array_equal(_bits(on["C"]), _bits(off["C"]))


# ------------------------------------------------------------------------------------------------ factor level
# (workload, leading blocks or None, batch, blocks read back, keep L blocks?, switches)
FCASES = {"darcy128_leading3_b9": ("darcy128", 3, 9, (0, 1, 2), False, 0),
          "darcy128_leading3_b9_diag128": ("darcy128", 3, 9, (0, 1, 2), False, int(Switch.NO_PERSIST_PANELS)),
          "darcy64_b9": ("darcy64", None, 9, (0, 1, 15), True, 0)}
K_SAMPLES = 64


def _fwd_state(pkg, F):
    st = C.c_int32(-1)
    y = np.empty((F.batch, F.N), dtype=np.float64)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_factor_fwd(F._h, C.byref(st), pkg._cabi.ptr(y)))
    return int(st.value)


def _run(pkg, lib, Q, nb, B, idx, keep_l, bits, b, first, then=None, strict=1):
    """A fresh handle: factor `first`, then (stale-data case) refactor `then`; posterior, blocks of problems 0 and B - 1, logdet."""
    pkg._cabi.check(lib.gmrf_test_strict_lower(strict))
    try:
        F = pkg.TridiagonalCholeskyFactor(batch=B)
        F.set_keep_l(keep_l)
        F.set_eager(bits)
        F.set_factor_rhs(b)
        F.factor(Q, nb, values=first)
        if then is not None:
            F.refactor(then)
        fwd = _fwd_state(pkg, F)
        mu, X = F.posterior_batch(b, K_SAMPLES, seed=29, first_id=3)
        out = {"mean": mu.cpu().numpy().copy(), "samples": X.cpu().numpy().copy(), "fwd": fwd}
        ld = F.logdet_batch()
        out["logdet"] = (ld.cpu().numpy() if hasattr(ld, "cpu") else np.asarray(ld)).copy()
        blocks = []
        for p in (0, B - 1):
            F.select_problem(p)
            for i in idx:
                blocks.append(F.get_block(2, i))                   # Linv_i
                if i > 0:
                    blocks.append(F.get_block(1, i - 1))           # C_i
        F.select_problem(0)
        out["blocks"] = blocks
        F.close()
        return out
    finally:
        pkg._cabi.check(lib.gmrf_test_strict_lower(1))


@pytest.fixture(scope="module", params=list(FCASES))
def fcase(request, pkg, lib):
    import torch
    name, nb, B, idx, keep_l, bits = FCASES[request.param]
    w = pkg.workloads.darcy(int(name[5:]))
    if nb:
        m = nb * w.block_size
        Q = sp.csc_matrix(w.Q[:m, :m]); Q.sort_indices()
        rhs = np.ascontiguousarray(w.rhs[:m])
    else:
        Q, rhs, nb = w.Q, np.ascontiguousarray(w.rhs), w.n_blocks
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    other = np.stack([Q.data * (3.7 - 0.2 * p) for p in range(B)])            # the factorisation that came before
    b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
    got = {"on": _run(pkg, lib, Q, nb, B, idx, keep_l, bits, b, vals),
           "off": _run(pkg, lib, Q, nb, B, idx, keep_l, bits, b, vals, strict=0),
           "stale": _run(pkg, lib, Q, nb, B, idx, keep_l, bits, b, other, then=vals)}
    return request.param, w, Q, nb, B, idx, vals, got


def _same(a, c):
    assert a["fwd"] == c["fwd"]
    for nm in ("mean", "samples", "logdet"):
        assert np.array_equal(_bits(a[nm]), _bits(c[nm])), nm
    assert len(a["blocks"]) == len(c["blocks"])
    for k, (x, y) in enumerate(zip(a["blocks"], c["blocks"])):
        assert np.array_equal(_bits(x), _bits(y)), k


def test_factor_and_posterior_bitwise_with_the_hook_on_and_off(fcase):
    name, w, Q, nb, B, idx, vals, got = fcase
    if name.startswith("darcy128"):
        assert got["on"]["fwd"] == 1                       # every launch on the 64 x 64 tile: the forward solve rides
    assert np.isfinite(got["on"]["mean"]).all() and np.isfinite(got["on"]["samples"]).all()
    _same(got["on"], got["off"])


def test_nothing_an_earlier_factorisation_left_reaches_an_output(fcase):
    name, w, Q, nb, B, idx, vals, got = fcase
    _same(got["stale"], got["on"])


def test_factor_against_the_oracle(fcase):
    """As tests/test_gpu_envelope_bounds.py compares them."""
    name, w, Q, nb, B, idx, vals, got = fcase
    per = len(got["on"]["blocks"]) // 2
    for k, p in enumerate((0, B - 1)):
        Qp = sp.csc_matrix(Q.copy()); Qp.data = vals[p].copy()
        Fo = O.tridiagonal_cholesky(Qp, nb)
        blocks = got["on"]["blocks"][k * per:(k + 1) * per]
        at = 0
        for i in idx:
            X = blocks[at]; at += 1
            Xo = np.linalg.inv(Fo.chos[i])
            err = np.max(np.abs(np.tril(X) - Xo)) / np.max(np.abs(Xo))
            print(f"{name} problem {p} block {i}: Linv error {err:.2e}")
            assert err < TOL_FACTOR
            if i > 0:
                Ci = blocks[at]; at += 1
                assert np.max(np.abs(Ci - Fo.Cs[i - 1])) / np.max(np.abs(Fo.Cs[i - 1])) < TOL_FACTOR
        ld = O.logdet(Fo)
        assert abs(got["on"]["logdet"][p] - ld) <= TOL_FACTOR * abs(ld)
