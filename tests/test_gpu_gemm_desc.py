"""Every fp64 GEMM kernel family driven directly through a general GemmArgs (gmrf_test_gemm_desc): batches with inner and
outer strides, interleaved and padded operands, a separate addend, per-tile K bounds, early-exit and triangular grids, the
single-stage form, the launcher's own choice, the tail row and the direct output.  Every result is compared element by element
with the longdouble reference of tests/gemm_desc_ref.py under its derived bound; outputs are compared as bits outside the
writable set; every case asserts the kernel family the hook reports."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from tests import gemm_desc_ref as R

pytestmark = pytest.mark.gpu

BAD_SHAPE = -2
OUTS = ("C", "tC", "samples", "mean")


def call(lib, pkg, d, route, buf):
    """One hook call on the buffers of R.build (outputs are overwritten in place).  Returns (status, family)."""
    def pn(name):
        a = buf.get(name)
        return (pkg._cabi.ptr(a), 0 if a is None else a.size)
    desc = d.desc_array()
    abt = np.array([d.alpha, d.beta, d.tbeta])
    fam = C.c_int32(-1)
    args = []
    for nm in ("A", "B", "C", "D", "tA", "tC", "tD", "kb_m", "kb_n", "ke_n", "samples", "mean"):
        args += list(pn(nm))
    st = lib.gmrf_test_gemm_desc(0, route, pkg._cabi.ptr(desc), pkg._cabi.ptr(abt), *args, C.byref(fam))
    return st, fam.value


def run(lib, pkg, d, route, data, fam_expected):
    """Build (poisoned at the granularity of the expected family's tile), launch, assert the family.  Returns (buf, init)."""
    buf = R.build(d, data, R.FAM_TILE[fam_expected & 255])
    init = {k: buf[k].copy() for k in OUTS if k in buf}
    st, fam = call(lib, pkg, d, route, buf)
    pkg._cabi.check(st)
    assert fam == fam_expected, (fam, fam_expected)
    return buf, init


def check(d, fam, buf, init, data, seed):
    """C (and the tail) against the reference inside the written set, bit-unchanged outside the writable set, exact where a
    tile's K range is empty."""
    refs = R.reference(d, data, seed)
    ix = R.index_maps(d)
    wm, may, em = R.written_mask(d, fam), R.may_write_mask(d, fam), R.empty_mask(d, fam)
    touched = np.zeros(buf["C"].size, bool)
    t_touched = np.zeros(buf["tC"].size, bool) if d.tail == 2 else None
    for z in range(d.batch):
        zp = z // d.nb1
        got = buf["C"][ix["C"][z]]
        r = refs[z]
        g = got[:d.M]
        print(f"z={z} worst error / bound: {R.worst(g[wm], r['ref'][wm], r['mag'][wm], d.K):.3f}")
        assert R.within(g[wm], r["ref"][wm], r["mag"][wm], d.K), f"problem {z}"
        sel = em & wm
        if sel.any():
            addend = (data["D"][zp] if d.has_D else data["C"][z])[:d.M]
            if d.beta != 0.0:
                assert np.array_equal(g[sel], (d.beta * addend)[sel]), f"problem {z}: empty K range"
            else:
                assert d.alpha > 0 and np.all(g[sel].view(np.uint64) == 0), f"problem {z}: empty K range is not +0.0"
        touched[ix["C"][z][:d.M][may]] = True
        if d.tail == 1:
            print(f"z={z} tail worst / bound: {R.worst(got[d.M], r['tref'], r['tmag'], d.K):.3f}")
            assert R.within(got[d.M], r["tref"], r["tmag"], d.K), f"problem {z}: tail row"
            touched[ix["C"][z][d.M]] = True
        if d.tail == 2:
            tg = buf["tC"][ix["tC"][zp]]
            print(f"z={z} tail worst / bound: {R.worst(tg, r['tref'], r['tmag'], d.K):.3f}")
            assert R.within(tg, r["tref"], r["tmag"], d.K), f"problem {z}: tail"
            t_touched[ix["tC"][zp]] = True
    assert np.array_equal(buf["C"].view(np.uint64)[~touched], init["C"].view(np.uint64)[~touched]), "C written outside the writable set"
    if d.tail == 2:
        assert np.array_equal(buf["tC"].view(np.uint64)[~t_touched], init["tC"].view(np.uint64)[~t_touched]), "tC written outside"
    return refs


def logical_C(d, buf, z, rows=None):
    return buf["C"][R.index_maps(d)["C"][z]][:rows or d.M]


def assert_batch_invariant(lib, pkg, d, route, fam, data, buf, zs=None, fam_alone=None):
    """Problem z of the batch == the same problem launched alone on the same family, bit for bit."""
    wm = R.written_mask(d, fam)
    for z in (range(d.batch) if zs is None else zs):
        d1, dat1 = R.pick(d, data, z)
        b1, _ = run(lib, pkg, d1, route, dat1, fam_alone or fam)
        a, b = logical_C(d, buf, z, d.rows), logical_C(d1, b1, 0, d.rows)
        wr = np.vstack([wm, np.ones((d.rows - d.M, d.N), bool)])
        assert np.array_equal(a[wr].view(np.uint64), b[wr].view(np.uint64)), f"problem {z} differs from its launch alone"
        if d.tail == 2:
            ix, ix1 = R.index_maps(d), R.index_maps(d1)
            assert np.array_equal(buf["tC"][ix["tC"][z // d.nb1]].view(np.uint64), b1["tC"][ix1["tC"][0]].view(np.uint64))


# Every test below takes its descriptors from a function of its own parameters and registers it, so that the CPU half
# (tests/test_gemm_desc_cpu.py) checks the reference, the masks and the size formulas on exactly the descriptors used here.
CASES = []          # (test name, function(**parameters) -> [(descriptor, family whose tile poisons the buffers)], test)


def described_by(fn):
    """Outermost decorator of a test: registers the descriptor function with the test's own parametrisation."""
    def deco(test):
        CASES.append((test.__name__, fn, test))
        return test
    return deco


def param_sets(test):
    """The parameter dicts of a test, from its parametrize marks."""
    sets = [{}]
    for m in getattr(test, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")]
        grown = []
        for st in sets:
            for v in m.args[1]:
                v = getattr(v, "values", v)
                grown.append({**st, **dict(zip(names, (v,) if len(names) == 1 else v))})
        sets = grown
    return sets


# (name, route, family, M, N, K, transA): the smallest shapes that reach each family, more than one tile each
FAMILIES = [
    ("reg16_k48", R.REG, R.FAM_REG16, 128, 192, 48, 0),
    ("reg16_k208", R.REG, R.FAM_REG16, 64, 128, 208, 0),
    ("reg32", R.REG, R.FAM_REG32, 128, 192, 96, 0),
    ("reg32_at", R.REG, R.FAM_REG32, 128, 64, 64, 1),
    ("big", R.BIG, R.FAM_BIG, 128, 256, 48, 0),
    ("ll", R.LL, R.FAM_LL, 128, 64, 96, 0),
    ("dma64", R.DMA64, R.FAM_DMA64, 128, 192, 48, 0),
    ("dma128x64", R.DMA128x64, R.FAM_DMA128x64, 256, 64, 48, 0),
    ("dma64x128", R.DMA64x128, R.FAM_DMA64x128, 64, 256, 48, 0),
    ("dma64_at", R.DMA64, R.FAM_DMA64, 128, 192, 48, 1),
]
FAM_IDS = [f[0] for f in FAMILIES]
BATCHES = [(3, 1), (8, 1), (6, 3), (16, 2)]


def descs_batches(fam, b_n, batch, nb1):
    name, route, family, M, N, K, ta = fam
    return [(R.make(M, N, K, "inter", transA=ta, b_n=b_n, batch=batch, nb1=nb1, alpha=alpha, beta=beta), family)
            for beta, alpha in ((1.0, -0.75), (0.0, 1.25))]


@described_by(descs_batches)
@pytest.mark.parametrize("batch,nb1", BATCHES)
@pytest.mark.parametrize("b_n", [0, 1])
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_batches_and_strides(lib, pkg, fam, b_n, batch, nb1):
    name, route, family, M, N, K, ta = fam
    seed = 1000 + batch
    for d, _ in descs_batches(fam, b_n, batch, nb1):
        assert d.ldc != N and d.lda % 2 == 0 and d.lda % 64 and d.ldb % 64
        data = R.logical(d, seed)
        if route == R.LL and batch > 8:
            # the 32 x 32 kernel is chosen by launch size (a handful of problems): a batch of 16 does not qualify and must be refused
            st, _ = call(lib, pkg, d, route, R.build(d, data, (32, 32)))
            assert st == BAD_SHAPE
            continue
        buf, init = run(lib, pkg, d, route, data, family)
        check(d, family, buf, init, data, seed)
        assert_batch_invariant(lib, pkg, d, route, family, data, buf)


def descs_bitwise(fam, b_n):
    name, route, family, M, N, K, ta = fam
    d = R.make(M, N, K, "inter", transA=ta, b_n=b_n, batch=6, nb1=3, alpha=-0.75, beta=1.0)
    return [(d, family), (d, R.FAM_REG32 if K % 32 == 0 else R.FAM_REG16)]


@described_by(descs_bitwise)
@pytest.mark.parametrize("b_n", [0, 1])
@pytest.mark.parametrize("fam", [f for f in FAMILIES if f[1] != R.REG], ids=[f[0] for f in FAMILIES if f[1] != R.REG])
def test_batch_matches_register_kernel_bitwise(lib, pkg, fam, b_n):
    """The LDS-DMA, 128 x 128 and 32 x 32 kernels sum every element in the register-staged kernel's order: the same bits, per
    problem of a batch."""
    name, route, family, M, N, K, ta = fam
    (d, _), (_, reg_family) = descs_bitwise(fam, b_n)
    data = R.logical(d, 1006)
    buf, _ = run(lib, pkg, d, route, data, family)
    ref, _ = run(lib, pkg, d, R.REG, data, reg_family)
    assert np.array_equal(buf["C"].view(np.uint64), ref["C"].view(np.uint64))


def descs_addend(fam, b_n, layout, batch, nb1, beta):
    name, route, family, M, N, K, ta = fam
    return [(R.make(M, N, K, layout, transA=ta, b_n=b_n, batch=batch, nb1=nb1, alpha=0.5, beta=beta, has_D=True), family)]


@described_by(descs_addend)
@pytest.mark.parametrize("beta", [1.0, -0.5])
@pytest.mark.parametrize("layout,batch,nb1", [("inter", 6, 3), ("stack", 3, 1)])
@pytest.mark.parametrize("b_n", [0, 1])
@pytest.mark.parametrize("fam", FAMILIES, ids=FAM_IDS)
def test_separate_addend(lib, pkg, fam, b_n, layout, batch, nb1, beta):
    """D of its own (ldd != ldc, pD != pC, shared by the inner items of a problem), C NaN everywhere: C is never read."""
    name, route, family, M, N, K, ta = fam
    (d, _), = descs_addend(fam, b_n, layout, batch, nb1, beta)
    assert d.ldd != d.ldc and d.pD != d.pC
    data = R.logical(d, 2000 + batch)
    buf, init = run(lib, pkg, d, route, data, family)
    check(d, family, buf, init, data, 2000 + batch)


# K bounds: the staircase at 256^3 and 384 x 256 x 256.  (route, family) of every kernel that takes bounds at these shapes
BOUND_FAMS = [("reg32", R.REG, R.FAM_REG32), ("big", R.BIG, R.FAM_BIG), ("ll", R.LL, R.FAM_LL), ("dma64", R.DMA64, R.FAM_DMA64),
              ("dma128x64", R.DMA128x64, R.FAM_DMA128x64), ("dma64x128", R.DMA64x128, R.FAM_DMA64x128)]


def _bounds(M, N, K, which):
    kb_m, kb_n, ke_n = R.staircase(M, N, K)
    return {"all": dict(kb_m=kb_m, kb_n=kb_n, ke_n=ke_n), "ke": dict(ke_n=ke_n), "kb": dict(kb_m=kb_m, kb_n=tuple(kb_m[:N // 64]))}[which]


def descs_k_bounds(fam, M, tri, which):
    b_n = (tri >> 2) & 1 ^ (1 if which == "ke" else 0)
    d = R.make(M, 256, 256, "stack", b_n=b_n, tri=tri, alpha=0.75, beta=0.0, **_bounds(M, 256, 256, which))
    return [(d, fam[2]), (replace(d, beta=-0.5), fam[2])]


@described_by(descs_k_bounds)
@pytest.mark.parametrize("which", ["all", "ke", "kb"])
@pytest.mark.parametrize("tri", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("M", [256, 384])
@pytest.mark.parametrize("fam", BOUND_FAMS, ids=[f[0] for f in BOUND_FAMS])
def test_k_bounds(lib, pkg, fam, M, tri, which):
    name, route, family = fam
    (d, _), (d_in_place, _) = descs_k_bounds(fam, M, tri, which)
    data = R.logical(d, 3000 + M)
    buf, init = run(lib, pkg, d, route, data, family)
    check(d, family, buf, init, data, 3000 + M)
    if which == "all":
        assert R.empty_mask(d, R.FAM_REG32).any()
    d = d_in_place
    buf, init = run(lib, pkg, d, route, data, family)
    check(d, family, buf, init, data, 3000 + M)


def descs_k_bounds_lower(fam, which):
    return [(R.make(256, 256, 256, "stack", b_n=0, lower_only=1, alpha=1.0, beta=1.0, **_bounds(256, 256, 256, which)), fam[2])]


@described_by(descs_k_bounds_lower)
@pytest.mark.parametrize("which", ["all", "kb"])
@pytest.mark.parametrize("fam", [f for f in BOUND_FAMS if f[1] != R.DMA64x128], ids=[f[0] for f in BOUND_FAMS if f[1] != R.DMA64x128])
def test_k_bounds_lower_only(lib, pkg, fam, which):
    """The square staircase on a triangular grid (the LDS-DMA kernel then walks its rows in ascending order)."""
    name, route, family = fam
    (d, _), = descs_k_bounds_lower(fam, which)
    data = R.logical(d, 3100)
    buf, init = run(lib, pkg, d, route, data, family)
    check(d, family, buf, init, data, 3100)


def descs_k_bounds_batch8(fam, lower):
    d = R.make(256, 256, 256, "inter", b_n=0, lower_only=lower, batch=8, alpha=0.75, beta=0.0, **_bounds(256, 256, 256, "all"))
    return [(d, fam[2]), (R.pick(d, R.logical(d, 3200), 0)[0], fam[2])]


@described_by(descs_k_bounds_batch8)
@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("fam", BOUND_FAMS[:1] + BOUND_FAMS[3:4] + BOUND_FAMS[1:2], ids=["reg32", "dma64", "big"])
def test_k_bounds_batch_of_8(lib, pkg, fam, lower):
    name, route, family = fam
    d = descs_k_bounds_batch8(fam, lower)[0][0]
    data = R.logical(d, 3200)
    buf, init = run(lib, pkg, d, route, data, family)
    check(d, family, buf, init, data, 3200)
    assert_batch_invariant(lib, pkg, d, route, family, data, buf, zs=[0, 5])


def descs_early_exit(fam, b_n):
    return [(R.make(384, 256, 64, "inter", b_n=b_n, lower_only=1, batch=batch, alpha=-1.0, beta=1.0), fam[2]) for batch in (1, 8)]


@described_by(descs_early_exit)
@pytest.mark.parametrize("b_n", [0, 1])
@pytest.mark.parametrize("fam", [("reg32", R.REG, R.FAM_REG32), ("dma64", R.DMA64, R.FAM_DMA64)], ids=["reg32", "dma64"])
def test_early_exit_grid(lib, pkg, fam, b_n):
    """lower_only with M != N: a rectangular grid whose tiles above the diagonal exit; they stay bit-unchanged."""
    name, route, family = fam
    for d, _ in descs_early_exit(fam, b_n):
        batch = d.batch
        data = R.logical(d, 4000 + batch)
        buf, init = run(lib, pkg, d, route, data, family)
        check(d, family, buf, init, data, 4000 + batch)
        assert not R.written_mask(d, family).all()


def descs_single_stage():
    d = R.make(256, 256, 64, "stack", b_n=0, batch=56, alpha=1.0, beta=0.0, lda=64 + 7)
    return [(d, R.FAM_REG32), (replace(d, batch=8), R.FAM_REG32)]


@described_by(descs_single_stage)
def test_single_stage(lib, pkg):
    """256 x 256 x 64 at batch 56: 896 workgroups, more than 768: the launcher's own choice is the register-staged kernel's
    single-stage form (odd lda keeps the LDS-DMA kernel out); bitwise the double-stage result of the same problems at batch 8."""
    (d, _), (d8, _) = descs_single_stage()
    data = R.logical(d, 5000)
    buf, init = run(lib, pkg, d, R.AUTO, data, R.FAM_REG32 | R.FAM_SINGLE)
    check(d, R.FAM_REG32, buf, init, data, 5000)
    ix = R.index_maps(d)
    for z0 in range(0, 56, 8):
        dat8 = {k: v[z0:z0 + 8] for k, v in data.items()}
        b8, _ = run(lib, pkg, d8, R.REG, dat8, R.FAM_REG32)
        ix8 = R.index_maps(d8)
        for z in range(8):
            assert np.array_equal(buf["C"][ix["C"][z0 + z]].view(np.uint64), b8["C"][ix8["C"][z]].view(np.uint64)), z0 + z


# the launcher's own choice, each side of each gate: (id, expected family, make() arguments)
AUTO_CASES = [
    ("ll_at_128_tiles", R.FAM_LL, dict(M=256, N=256, K=64, batch=8)),                       # 16 tiles x 8 = 128: the 32 x 32 kernel
    ("dma_above_ll_gate", R.FAM_DMA64, dict(M=256, N=320, K=64, batch=8)),                  # 160 tiles: past the gate, LDS-DMA default
    ("dma_batch_9", R.FAM_DMA64, dict(M=128, N=128, K=64, batch=9)),                        # 36 tiles but more than 8 problems
    ("ll_batch_1", R.FAM_LL, dict(M=128, N=128, K=64, batch=1)),
    ("dma_k48", R.FAM_DMA64, dict(M=128, N=128, K=48, batch=1)),                            # K % 32: not the 32 x 32 kernel
    ("reg16_odd_lda", R.FAM_REG16, dict(M=128, N=128, K=48, batch=2, lda=48 + 9)),          # the LDS-DMA kernel declines an odd lda
    ("reg32_odd_lda", R.FAM_REG32, dict(M=128, N=192, K=64, batch=9, lda=64 + 9)),
    ("ll_odd_lda", R.FAM_LL, dict(M=128, N=192, K=64, batch=2, lda=64 + 9)),
    # the 128 x 128 kernel: a launch the LDS-DMA kernel does not take (odd lda) of at least 64 of its tiles, and then where the
    # makespan model (fixed constants: a function of the descriptor alone) predicts it faster than the 64 x 64 kernel
    ("big_below_gate", R.FAM_REG32, dict(M=256, N=384, K=64, batch=10, lda=64 + 9)),        # 6 x 10 = 60 big tiles < 64
    # 66 big tiles, 4 K steps of 2.5 us + 1 = 11 us in one round, against 264 small tiles, 2 steps of 2.2 us + 1 = 5.4 us in one round
    ("big_past_gate_model_says_64", R.FAM_REG32, dict(M=256, N=384, K=64, batch=11, lda=64 + 9)),
    # 132 big tiles, 3 steps of 2.5 us + 1 = 8.5 us in one round, against 528 small tiles on 512 slots: two rounds of 4.75 us = 9.5 us
    ("big_past_gate_model_says_128", R.FAM_BIG, dict(M=256, N=384, K=48, batch=22, lda=48 + 9)),
    # the wide LDS-DMA tile: full products of at least 2048 tiles of 64 x 64
    ("dma128x64_at_2048_tiles", R.FAM_DMA128x64, dict(M=128, N=128, K=16, batch=512)),
    ("dma64_below_2048_tiles", R.FAM_DMA64, dict(M=128, N=128, K=16, batch=504)),
]


def descs_auto(case, b_n):
    name, family, kw = case
    kw = dict(kw)
    return [(R.make(kw.pop("M"), kw.pop("N"), kw.pop("K"), "stack", b_n=b_n, alpha=-0.75, beta=1.0, **kw), family)]


@described_by(descs_auto)
@pytest.mark.parametrize("case", AUTO_CASES, ids=[c[0] for c in AUTO_CASES])
@pytest.mark.parametrize("b_n", [0, 1])
def test_launchers_own_choice(lib, pkg, case, b_n):
    name, family, kw = case
    (d, _), = descs_auto(case, b_n)
    data = R.logical(d, 6000)
    buf, init = run(lib, pkg, d, R.AUTO, data, family)
    check(d, family, buf, init, data, 6000)


# ------------------------------------------------------------------------------------------------ tail row
def _tail_vs_plain(lib, pkg, d, data, seed):
    """Run the tail product, check it, and compare rows 0 .. M-1 bitwise with the 64 x 64 LDS-DMA kernel without the tail."""
    buf, init = run(lib, pkg, d, R.TAIL, data, R.FAM_DOUT if d.dout else R.FAM_TAIL)
    check(d, R.FAM_TAIL, buf, init, data, seed)
    dp = _plain(d)
    bp, _ = run(lib, pkg, dp, R.DMA64, data, R.FAM_DMA64)
    wm = R.written_mask(d, R.FAM_TAIL)
    for z in range(d.batch):
        a, b = logical_C(d, buf, z), logical_C(dp, bp, z)
        assert np.array_equal(a[wm].view(np.uint64), b[wm].view(np.uint64)), f"problem {z}: rows differ from the kernel without the tail"
    return buf, init


def _plain(d):
    """The same product without its tail, as the 64 x 64 LDS-DMA kernel runs it."""
    return replace(d, tail=0, has_tD=False, dout=False, ptA=0, ptC=0, ptD=0, o_j0=0, o_n=0, o_cols=0, o_ld=0, o_k=0)


def descs_tail_own(b_n, lower, tri, tbeta, has_tD, batch):
    d = R.make(192, 192, 64 if lower else 192, "inter" if batch > 1 else "stack", b_n=b_n, lower_only=lower, tri=tri, batch=batch,
               alpha=-1.0, beta=1.0, tbeta=tbeta, tail=2, has_tD=has_tD)
    return [(d, R.FAM_TAIL), (_plain(d), R.FAM_DMA64)]


@described_by(descs_tail_own)
@pytest.mark.parametrize("batch", [1, 3, 8])
@pytest.mark.parametrize("tbeta,has_tD", [(0.0, False), (1.0, False), (1.0, True)])
@pytest.mark.parametrize("b_n,lower,tri", [(0, 1, 0), (0, 0, 8), (1, 0, 4), (1, 0, 0)],
                         ids=["nk_triangular_grid", "nk_tri_b_upper", "kn_tri_b_lower", "kn_full"])
def test_tail_with_operands_of_its_own(lib, pkg, b_n, lower, tri, tbeta, has_tD, batch):
    d = descs_tail_own(b_n, lower, tri, tbeta, has_tD, batch)[0][0]
    _tail_vs_plain(lib, pkg, d, R.logical(d, 7000 + batch), 7000 + batch)


def descs_tail_row_m(beta, batch, nb1):
    d = R.make(128, 192, 48, "inter" if batch > 1 else "stack", b_n=1, batch=batch, nb1=nb1, alpha=0.5, beta=beta, has_D=True, tail=1)
    return [(d, R.FAM_TAIL), (_plain(d), R.FAM_DMA64)]


@described_by(descs_tail_row_m)
@pytest.mark.parametrize("batch,nb1", [(1, 1), (3, 1), (8, 1), (6, 3)])
@pytest.mark.parametrize("beta", [1.0, -0.5])
def test_tail_in_row_m_with_separate_addend(lib, pkg, beta, batch, nb1):
    d = descs_tail_row_m(beta, batch, nb1)[0][0]
    _tail_vs_plain(lib, pkg, d, R.logical(d, 7100 + batch), 7100 + batch)


def descs_tail_staircase(b_n, lower, batch):
    which = "kb" if lower else "all"
    d = R.make(256, 256, 256, "inter" if batch > 1 else "stack", b_n=b_n, lower_only=lower, batch=batch, alpha=1.0, beta=0.0,
               tbeta=1.0, tail=2, **_bounds(256, 256, 256, which))
    return [(d, R.FAM_TAIL), (_plain(d), R.FAM_DMA64)]


@described_by(descs_tail_staircase)
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("b_n,lower", [(0, 1), (0, 0), (1, 0)], ids=["nk_triangular_grid", "nk_full", "kn_full"])
def test_tail_with_staircase_bounds(lib, pkg, b_n, lower, batch):
    """The tail's K range is its carrying tile's: the diagonal tile (bn, bn) of a triangular grid, else the last row tile."""
    d = descs_tail_staircase(b_n, lower, batch)[0][0]
    _tail_vs_plain(lib, pkg, d, R.logical(d, 7200 + batch), 7200 + batch)


def descs_dout(k, o_cols, o_j0, tri, batch):
    M, N, K = 64 if k == 1 else 128, 128, 128
    o_n = o_j0 + N + 5
    d = R.make(M, N, K, "inter" if batch > 1 else "stack", b_n=1, tri=tri, batch=batch, alpha=1.0, beta=0.0, tail=1, dout=True,
               o_j0=o_j0, o_n=o_n, o_cols=o_cols, o_ld=o_n + 3, o_k=k)
    return [(d, R.FAM_DOUT), (_plain(d), R.FAM_DMA64)]


@described_by(descs_dout)
@pytest.mark.parametrize("batch", [1, 8])
@pytest.mark.parametrize("tri", [0, 4, 8])
@pytest.mark.parametrize("k,o_cols,o_j0", [(1, 100, 3), (16, 128, 64), (63, 127, 1)])
def test_direct_output(lib, pkg, k, o_cols, o_j0, tri, batch):
    """samples[(p k + r) ld + j0 + c] = C[r][c] + tail[c] for r < k, c < o_cols; mean[p n + j0 + c] = tail[c]; nothing else."""
    d = descs_dout(k, o_cols, o_j0, tri, batch)[0][0]
    M, K, o_n = d.M, d.K, d.o_n
    seed = 7300 + batch
    data = R.logical(d, seed)
    buf, init = _tail_vs_plain(lib, pkg, d, data, seed)
    refs = R.reference(d, data, seed)
    s_touched = np.zeros(buf["samples"].size, bool)
    m_touched = np.zeros(buf["mean"].size, bool)
    L = np.longdouble
    for p in range(batch):
        r = refs[p]
        si = (p * k + np.arange(k))[:, None] * d.o_ld + o_j0 + np.arange(o_cols)[None, :]
        mi = p * o_n + o_j0 + np.arange(o_cols)
        # a sample is the rounded sum of the two rounded values: both bounds and one more rounding of a sum no larger than the two magnitudes
        sref = r["ref"][:k, :o_cols] + r["tref"][None, :o_cols]
        smag = r["mag"][:k, :o_cols] + r["tmag"][None, :o_cols]
        assert R.within(buf["samples"][si], sref.astype(L), smag, K, extra=1), f"problem {p}: samples"
        assert R.within(buf["mean"][mi], r["tref"][:o_cols], r["tmag"][:o_cols], K), f"problem {p}: mean"
        # and exactly the sum of what the launch left in C
        got = buf["C"][R.index_maps(d)["C"][p]]
        assert np.array_equal(buf["samples"][si], got[:k, :o_cols] + got[M][None, :o_cols])
        assert np.array_equal(buf["mean"][mi], got[M][:o_cols])
        s_touched[si] = True
        m_touched[mi] = True
    for nm, t in (("samples", s_touched), ("mean", m_touched)):
        assert np.array_equal(buf[nm].view(np.uint64)[~t], init[nm].view(np.uint64)[~t]), f"{nm} written outside its part"


def _good_product(lib, pkg):
    d = R.make(64, 64, 16, "tight", b_n=1)
    data = R.logical(d, 1)
    buf, init = run(lib, pkg, d, R.DMA64, data, R.FAM_DMA64)
    check(d, R.FAM_DMA64, buf, init, data, 1)


DOUT_BASE = dict(b_n=1, batch=2, alpha=1.0, beta=0.0, tail=1, dout=True, o_j0=0, o_n=140, o_cols=128, o_ld=150, o_k=16)


@pytest.mark.parametrize("change", [dict(beta=1.0), dict(kb_m=(0, 64)), dict(ke_n=(64, 128)), dict(batch=4, nb1=2), dict(tri=1), dict(tri=2),
                                    dict(b_n=0)], ids=["beta", "kb_m", "ke_n", "nb1", "tri_a_lower", "tri_a_upper", "b_nk"])
def test_direct_output_refusals(lib, pkg, change):
    """What gemm_tail_ok must refuse for a direct output (every row tile sums the tail row over its own K range, and the tail
    must not read C): decided on the host, nothing launched, outputs untouched."""
    d = R.make(128, 128, 128, "stack", **dict(DOUT_BASE, **change))
    data = R.logical(d, 8000)
    buf = R.build(d, data, (64, 64))
    init = {k: buf[k].copy() for k in ("C", "samples", "mean")}
    st, fam = call(lib, pkg, d, R.TAIL, buf)
    assert st == BAD_SHAPE and fam == 0
    for k in init:
        assert np.array_equal(buf[k].view(np.uint64), init[k].view(np.uint64))
    _good_product(lib, pkg)


def _refusal_cases():
    """(id, descriptor the buffers are built for, descriptor of the call, route, buffers to cut short)"""
    base = R.make(128, 128, 64, "stack", b_n=0, batch=4, nb1=2, beta=1.0, has_D=True)
    dout = R.make(128, 128, 128, "stack", **DOUT_BASE)
    own = R.make(128, 128, 64, "stack", b_n=1, batch=2, tail=2)

    def same(d):
        return d, d

    yield ("short_A", *same(base), R.REG, dict(A=-1))
    yield ("short_B", *same(base), R.REG, dict(B=-1))
    yield ("short_C", *same(base), R.DMA64, dict(C=-1))
    yield ("short_D", *same(base), R.DMA64, dict(D=-1))
    yield ("batch_not_multiple_of_nb1", replace(base, batch=6), replace(base, batch=5), R.REG, {})
    yield ("ld_below_width", base, replace(base, ldc=64), R.REG, {})
    yield ("big_on_192_rows", *same(R.make(192, 128, 64, "stack")), R.BIG, {})
    yield ("big_transposed_A", *same(R.make(128, 128, 64, "stack", transA=1)), R.BIG, {})
    yield ("ll_k48", *same(R.make(128, 128, 48, "stack")), R.LL, {})
    yield ("ll_above_gate", *same(R.make(256, 320, 64, "stack", batch=8)), R.LL, {})
    yield ("dma_odd_lda", *same(R.make(128, 128, 64, "stack", lda=71)), R.DMA64, {})
    yield ("dma128x64_on_192_rows", *same(R.make(192, 128, 64, "stack")), R.DMA128x64, {})
    yield ("dma64x128_lower_only", *same(R.make(256, 256, 64, "stack", lower_only=1)), R.DMA64x128, {})
    yield ("tail_transposed_A", *same(R.make(128, 128, 64, "stack", transA=1, b_n=1, tail=2)), R.TAIL, {})
    yield ("tail_row_m_on_nk", *same(R.make(128, 128, 64, "stack", b_n=0, tail=1)), R.TAIL, {})
    yield ("tail_early_exit_grid", *same(R.make(256, 128, 64, "stack", lower_only=1, tail=2)), R.TAIL, {})
    yield ("own_tail_nb1", *same(R.make(128, 128, 64, "stack", b_n=1, batch=4, nb1=2, tail=2)), R.TAIL, {})
    yield ("short_tA", *same(own), R.TAIL, dict(tA=-1))
    yield ("short_tC", *same(own), R.TAIL, dict(tC=-1))
    yield ("short_kb_m", *same(R.make(128, 128, 64, "stack", kb_m=(0, 64))), R.REG, dict(kb_m=-1))
    yield ("bound_not_multiple_of_64", *same(R.make(128, 128, 64, "stack", kb_m=(0, 32))), R.REG, {})
    yield ("short_samples", *same(dout), R.TAIL, dict(samples=-8))
    yield ("short_mean", *same(dout), R.TAIL, dict(mean=-8))


_REFUSALS = list(_refusal_cases())


@pytest.mark.parametrize("case", _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_refusals(lib, pkg, case):
    """Undersized buffers, batch % nb1 != 0 and forced routes the descriptor does not qualify for: bad_shape from the host-side
    checks, the outputs untouched, and the library good for a product afterwards."""
    name, d_build, d_call, route, cut = case
    buf = R.build(d_build, R.logical(d_build, 9000), (64, 64))
    for nm, by in cut.items():
        buf[nm] = buf[nm][:by].copy()
    init = {k: buf[k].copy() for k in OUTS if k in buf}
    st, fam = call(lib, pkg, d_call, route, buf)
    assert st == BAD_SHAPE and fam == 0
    for k in init:
        assert np.array_equal(buf[k].view(np.uint64), init[k].view(np.uint64))
    _good_product(lib, pkg)
