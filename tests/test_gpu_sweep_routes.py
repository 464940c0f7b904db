"""Every kernel instantiation of the block sweep products (csrc/sweep.hpp), driven through gmrf_test_sweep_product at the smallest
shapes that reach each loop of each kernel.  Every case asserts its route before the call (gmrf_test_sweep_route and the
restatement of tests/sweep_ref.py) and after it (the id the hook says ran), checks every output cell against the longdouble
reference with the derived bound (L + 3) 2^-53 (|b| + sum |a||x|), and every other cell of the panel -- sentinels, NaN pads,
inputs, addends that are not outputs -- bit for bit against what was uploaded.  The block holds NaN wherever the contract says
nobody reads (pads, left of a staircase start, from a staircase end on, the 64 x 64 tiles above a triangular block's diagonal)
and exact zeros where the factor leaves zeros (the strict upper triangles of the diagonal tiles): an output that met a NaN is
not finite.  A problem of a batch is bitwise that problem alone on the same kernel."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import sweep_ref as R

pytestmark = pytest.mark.gpu

SUBS = ("none", "apart", "inplace")


def hook_route(pkg, lib, case):
    out = np.full(4, -1, np.int64)
    pkg._cabi.check(lib.gmrf_test_sweep_route(pkg._cabi.ptr(case.desc()), pkg._cabi.ptr(out)))
    return tuple(int(v) for v in out)


def run(pkg, lib, case, expect, force=0, what=""):
    """One product: the route asserted before and after, the whole panel checked.  Returns the outputs (nprob, kp, rows)."""
    what = f"{what} [{R.NAMES[expect]}{', forced' if force else ''}; kp {case.kp} rows {case.rows} kdim {case.kdim} nprob {case.nprob} sub {case.sub}]"
    own = hook_route(pkg, lib, case)
    assert own == case.route(), (what, "library", own, "restatement", case.route())
    if force:
        assert force == expect and case.forced(force)[0] == force, (what, "the forced kernel's preconditions refuse the shape")
    else:
        assert own[0] == expect, (what, "would take", own)
    Mat, before = case.mat_buffer(), case.panel()
    after = before.copy()
    ran = C.c_int32(-1)
    p = pkg._cabi.ptr
    pkg._cabi.check(lib.gmrf_test_sweep_product(0, force, p(case.desc()), p(Mat), len(Mat), p(after), len(after), case.x_off, case.b_off, case.o_off,
                                                p(case.kst), 0 if case.kst is None else len(case.kst),
                                                p(case.mend), 0 if case.mend is None else len(case.mend), C.byref(ran)))
    assert ran.value == expect, (what, "ran", ran.value)
    out, ratio = case.check_panel(before, after, what)
    print("SWEEP_RATIO " + json.dumps({"case": what, "kernel": R.NAMES[expect], "products": case.nprob * case.kp, "ratio": round(ratio, 4)}))
    return out


def run_with_ties(pkg, lib, expect, what, problems=None, **kw):
    """The case on launch_sweep's own choice; then, for a batch, the problems `problems` (default: all) alone on the same kernel:
    the same bits."""
    case = R.Case(**kw)
    out = run(pkg, lib, case, expect, what=what)
    if case.nprob > 1:
        for q in (range(case.nprob) if problems is None else problems):
            alone = R.Case(**{**kw, "nprob": 1, "p0": kw.get("p0", 0) + q})
            one = run(pkg, lib, alone, expect, force=expect, what=f"{what}, problem {q} alone")
            assert np.array_equal(one[0], out[q]), f"{what}: problem {q} of the batch is not the problem alone"
    return out


# ------------------------------------------------------------------------------------------ sweep_mm
@pytest.mark.parametrize("trans", [False, True], ids=["n", "t"])
@pytest.mark.parametrize("kdim", [8, 40, 264])
def test_mm_dense(pkg, lib, trans, kdim):
    """rows 32; kdim 8: one group, three idle waves; 40: chunks of 16 -- the third wave takes the rest, the last starts past the
    end; 264: 72 per wave = one 8-group chunk and a single group, the last wave 48 = six single groups."""
    i = 0
    for kp in (16, 32):
        for nprob in (1, 3):
            run_with_ties(pkg, lib, R.mm_id(trans, False), "sweep_mm dense", trans=trans, tri=False, kp=kp, rows=32, kdim=kdim, nprob=nprob,
                          sub=SUBS[(i + kdim // 8) % 3], seed=kdim + i)
            i += 1


@pytest.mark.parametrize("stair", [("kst", [0, 64]), ("kst", [64, 64]), ("mend", [64, 128])], ids=["kst0-64", "kst64-64", "mend64-128"])
def test_mm_staircase(pkg, lib, stair):
    trans = stair[0] == "mend"
    for i, (kp, nprob) in enumerate(((16, 1), (32, 3), (16, 3), (32, 1))):
        run_with_ties(pkg, lib, R.mm_id(trans, False), f"sweep_mm {stair[0]} {stair[1]}", trans=trans, tri=False, kp=kp, rows=128, kdim=128,
                      nprob=nprob, sub=SUBS[(i + 1) % 3], seed=i, **{stair[0]: stair[1]})


@pytest.mark.parametrize("trans", [False, True], ids=["n", "t"])
@pytest.mark.parametrize("n", [16, 48, 272])
def test_mm_triangular(pkg, lib, trans, n):
    """One tile; three tiles (ranges of 16, 32, 48); 272: a range of 272 = 72 per wave, and every shorter one."""
    for i, (kp, nprob) in enumerate(((16, 1), (32, 3), (16, 3), (32, 1))):
        run_with_ties(pkg, lib, R.mm_id(trans, True), "sweep_mm triangular", trans=trans, tri=True, kp=kp, rows=n, kdim=n, nprob=nprob,
                      sub=SUBS[(i + n // 16) % 3], seed=n + i)


# ------------------------------------------------------------------------------------------ sweep_gemv_n
@pytest.mark.parametrize("n", [1, 2, 3, 1603])
def test_gemv_n_triangular(pkg, lib, n):
    """Rows of 1 (the odd tail alone), 2, 3 elements; 1603 rows: a ragged last workgroup, rows whose lane 0 passes the 8-stride
    loop (1024 elements and more), the 4-stride loop, single strides and the odd tail."""
    for i, sub in enumerate(SUBS):
        run_with_ties(pkg, lib, 6, "sweep_gemv_n triangular", trans=False, tri=True, kp=1, rows=n, kdim=n, sub=sub, seed=n + i)
        if n > 3:
            break
    if n == 3:
        run_with_ties(pkg, lib, 6, "sweep_gemv_n triangular, batch", trans=False, tri=True, kp=1, rows=n, kdim=n, nprob=2, sub="inplace", seed=9)


def test_gemv_n_dense_long_odd_rows(pkg, lib):
    """rows 7 (a ragged last workgroup), kdim 1601: lane 0 goes through the 8-stride loop once (k = 0 .. 896), the 4-stride loop
    once (1024 .. 1408), one single stride (1536) and the odd tail (1600)."""
    for i, sub in enumerate(SUBS):
        run_with_ties(pkg, lib, 5, "sweep_gemv_n dense 7 x 1601", trans=False, tri=False, kp=1, rows=7, kdim=1601, sub=sub, seed=i)


def test_gemv_n_staircase_and_fall_through(pkg, lib):
    run_with_ties(pkg, lib, 5, "sweep_gemv_n staircase", trans=False, tri=False, kp=1, rows=130, kdim=300, kst=[0, 64, 128], sub="inplace")
    # rows % 16 != 0 with kdim <= 256 (the short form's length) falls through, one problem and a batch of nine
    run_with_ties(pkg, lib, 5, "sweep_gemv_n fall-through", trans=False, tri=False, kp=1, rows=50, kdim=130, sub="apart", seed=1)
    run_with_ties(pkg, lib, 5, "sweep_gemv_n fall-through, batch", trans=False, tri=False, kp=1, rows=50, kdim=130, nprob=9, sub="none", seed=2)


# ------------------------------------------------------------------------------------------ sweep_gemv_n_short
@pytest.mark.parametrize("nprob", [1, 9])
def test_gemv_n_short(pkg, lib, nprob):
    """Triangular 16 (one workgroup, every second piece skipped), 144 (a second piece per lane from row 128 on), 256; dense rows
    48 with 2 (one lane), 130 (the second piece in one lane) and 256 elements (both pieces in every lane)."""
    for i, n in enumerate((16, 144, 256)):
        run_with_ties(pkg, lib, 8, "sweep_gemv_n_short triangular", trans=False, tri=True, kp=1, rows=n, kdim=n, nprob=nprob, sub=SUBS[i], seed=n)
    for i, kdim in enumerate((2, 130, 256)):
        run_with_ties(pkg, lib, 7, "sweep_gemv_n_short dense", trans=False, tri=False, kp=1, rows=48, kdim=kdim, nprob=nprob, sub=SUBS[(i + 1) % 3], seed=kdim)


# ------------------------------------------------------------------------------------------ sweep_gemv_n4
def test_gemv_n4_triangular(pkg, lib):
    """272 (the paired loop once for the last rows), 400, 768 (three turns of the paired loop)."""
    for i, n in enumerate((272, 400, 768)):
        run_with_ties(pkg, lib, 10, "sweep_gemv_n4 triangular", problems=(0, 7), trans=False, tri=True, kp=1, rows=n, kdim=n, nprob=8, sub=SUBS[i], seed=n)


def test_gemv_n4_dense_and_staircase(pkg, lib):
    """kdim 258 (paired loop for lane 0 only, then nothing), 384 (paired loop, then the single loop), 768; the staircase keeps a
    256-long product off the short kernel."""
    for i, kdim in enumerate((258, 384, 768)):
        run_with_ties(pkg, lib, 9, "sweep_gemv_n4 dense", problems=(0, 7), trans=False, tri=False, kp=1, rows=64, kdim=kdim, nprob=8, sub=SUBS[(i + 2) % 3], seed=kdim)
    run_with_ties(pkg, lib, 9, "sweep_gemv_n4 staircase", problems=(1, 6), trans=False, tri=False, kp=1, rows=128, kdim=256, nprob=8, kst=[0, 64], sub="inplace")


# ------------------------------------------------------------------------------------------ sweep_gemv_t
def test_gemv_t16(pkg, lib):
    """Triangular 16 (one block), 48 (three blocks: the middle one once), 288 (rows enough for the eight-load loop: 32 row groups
    x 8 = 256); dense rows 64 with 5 rows to sum (most row groups idle) and 300; a staircase end per output tile."""
    for i, n in enumerate((16, 48, 288)):
        run_with_ties(pkg, lib, 14, "sweep_gemv_t<16> triangular", trans=True, tri=True, kp=1, rows=n, kdim=n, sub=SUBS[i], seed=n)
    for i, kdim in enumerate((5, 300)):
        run_with_ties(pkg, lib, 13, "sweep_gemv_t<16> dense", trans=True, tri=False, kp=1, rows=64, kdim=kdim, sub=SUBS[i + 1], seed=kdim)
    run_with_ties(pkg, lib, 13, "sweep_gemv_t<16> mend", trans=True, tri=False, kp=1, rows=128, kdim=128, mend=[64, 128], sub="none", seed=3)
    run_with_ties(pkg, lib, 14, "sweep_gemv_t<16> triangular, batch", trans=True, tri=True, kp=1, rows=48, kdim=48, nprob=3, sub="apart", seed=4)
    run_with_ties(pkg, lib, 13, "sweep_gemv_t<16> mend, batch", trans=True, tri=False, kp=1, rows=128, kdim=128, nprob=3, mend=[64, 128], sub="inplace", seed=5)


def test_gemv_t8(pkg, lib):
    """narrow = 1.  Triangular 8 (one block) and 520 (65 blocks: 33 workgroups, the middle block once; 64 row groups x 8 = 512 rows
    for the eight-load loop); dense rows 72, kdim 520."""
    for i, n in enumerate((8, 520)):
        run_with_ties(pkg, lib, 12, "sweep_gemv_t<8> triangular", trans=True, tri=True, kp=1, rows=n, kdim=n, narrow=1, sub=SUBS[i], seed=n)
    run_with_ties(pkg, lib, 12, "sweep_gemv_t<8> triangular, batch", trans=True, tri=True, kp=1, rows=24, kdim=24, nprob=3, narrow=1, sub="inplace", seed=1)
    for i, sub in enumerate(SUBS):
        run_with_ties(pkg, lib, 11, "sweep_gemv_t<8> dense", trans=True, tri=False, kp=1, rows=72, kdim=520, nprob=1 + 2 * (i == 2), narrow=1, sub=sub, seed=i)


def test_gemv_t32_triangular(pkg, lib):
    """64 problems x 480 rows: 15 blocks = 8 workgroups per problem = 512; 128 problems x 224 rows: 7 blocks = 4 workgroups."""
    run_with_ties(pkg, lib, 16, "sweep_gemv_t<32> triangular 480", problems=(0, 63), trans=True, tri=True, kp=1, rows=480, kdim=480, nprob=64, sub="none")
    run_with_ties(pkg, lib, 16, "sweep_gemv_t<32> triangular 224", problems=(1, 127), trans=True, tri=True, kp=1, rows=224, kdim=224, nprob=128, sub="inplace", seed=1)
    run_with_ties(pkg, lib, 16, "sweep_gemv_t<32> triangular 224", problems=(64,), trans=True, tri=True, kp=1, rows=224, kdim=224, nprob=128, sub="apart", seed=2)


@pytest.mark.parametrize("mend", [None, [64, 128, 130, 130]], ids=["dense", "mend"])
def test_gemv_t32_dense(pkg, lib, mend):
    for i, sub in enumerate(SUBS if mend is None else ("inplace",)):
        run_with_ties(pkg, lib, 15, "sweep_gemv_t<32> 256 x 130", problems=(0, 63), trans=True, tri=False, kp=1, rows=256, kdim=130, nprob=64, mend=mend,
                      sub=sub, seed=i)


# ------------------------------------------------------------------------------------------ the three one-row / four-row forms on one operand
@pytest.mark.parametrize("kdim", [130, 256])
def test_non_transposed_gemv_kernels_agree_bitwise_dense(pkg, lib, kdim):
    """sweep_gemv_n, sweep_gemv_n_short and sweep_gemv_n4 forced on one operand: even elements into one chain per lane, odd into
    another, ascending k, the two added, then the wave's butterfly -- the same bits."""
    kw = dict(trans=False, tri=False, kp=1, rows=48, kdim=kdim, nprob=2, sub="apart", seed=kdim)
    outs = [run(pkg, lib, R.Case(**kw), kid, force=kid, what="tie, dense") for kid in (5, 7, 9)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("n", [144, 256])
def test_non_transposed_gemv_kernels_triangular_tie(pkg, lib, n):
    """Triangular: the two four-row kernels agree on every row.  sweep_gemv_n agrees with them on the odd rows (an even number of
    elements: whole pieces) and on the rows that are multiples of 128 (the last element's piece is lane 0's own last); on the other
    even rows it adds the last element to lane 0's chain while the four-row kernels keep it in lane (row / 2) % 64's, which is
    another order of the same sum: each stays within the bound (checked by every call), the bits may differ."""
    kw = dict(trans=False, tri=True, kp=1, rows=n, kdim=n, nprob=2, sub="inplace", seed=n)
    one, short, four = (run(pkg, lib, R.Case(**kw), kid, force=kid, what="tie, triangular") for kid in (6, 8, 10))
    assert np.array_equal(short, four)
    row = np.arange(n)
    same_order = (row % 2 == 1) | (row % 128 == 0)
    assert np.array_equal(one[..., same_order], short[..., same_order])
    differ = np.flatnonzero(np.any(one != short, axis=(0, 1)))
    print(f"SWEEP_TIE triangular {n}: sweep_gemv_n and the four-row kernels differ on {len(differ)} of {np.count_nonzero(~same_order)} "
          f"even rows that are no multiple of 128, on no other row; first {differ[:6].tolist()}")
    assert len(differ) > 0 and not np.any(same_order[differ])
