"""The block sweep products' route (csrc/sweep.hpp: sweep_route), host only: gmrf_test_sweep_route against its restatement
(tests/sweep_ref.py) on both sides of every boundary and on every refusal; every product sweep_launches issues today is accepted;
the refusals of gmrf_test_sweep_product, which all come before its upload; and the reference with its bound against fp64
emulations of the product, sound and defective."""
import ctypes as C

import numpy as np
import pytest

from tests import sweep_ref as R


def hook_route(pkg, lib, trans, tri, kp, rows, kdim, nprob, narrow=0, has_kst=False, has_mend=False):
    desc = np.array([trans, tri, kp, rows, kdim, nprob, narrow, has_kst, has_mend, 0, 0, 0, 0, 0, 0, 0, 0], np.int64)
    out = np.full(4, -1, np.int64)
    pkg._cabi.check(lib.gmrf_test_sweep_route(pkg._cabi.ptr(desc), pkg._cabi.ptr(out)))
    return tuple(int(v) for v in out)


def both(pkg, lib, *a, **k):
    got, want = hook_route(pkg, lib, *a, **k), R.route(*a, **k)
    assert got == want, (a, k, "library", got, "restatement", want)
    if got[0] == 0:
        assert got == R.REFUSED
    return got


def test_route_boundaries_non_transposed(pkg, lib):
    """kdim 256 / 258 (short | four-row), 768 / 770 (four-row | one row per wave), nprob 7 / 8, rows % 16, kst, odd kdim."""
    seen = set()
    for tri in (False, True):
        for nprob in (1, 7, 8, 9):
            for rows in (16, 48, 50, 52, 256, 272, 768, 784):
                for kdim in ([rows] if tri else [2, 255, 256, 257, 258, 767, 768, 769, 770, 1601]):
                    for kst in ((False,) if tri else (False, True)):
                        for narrow in (0, 1):
                            seen.add(both(pkg, lib, False, tri, 1, rows, kdim, nprob, narrow, kst, False)[0])
    assert seen == {5, 6, 7, 8, 9, 10}
    # one by one, the four conditions of the short form and the four of the four-row form
    assert both(pkg, lib, False, False, 1, 48, 256, 1)[0] == 7 and both(pkg, lib, False, False, 1, 48, 258, 1)[0] == 5
    assert both(pkg, lib, False, False, 1, 48, 258, 8)[0] == 9 and both(pkg, lib, False, False, 1, 48, 258, 7)[0] == 5
    assert both(pkg, lib, False, False, 1, 48, 768, 8)[0] == 9 and both(pkg, lib, False, False, 1, 48, 770, 8)[0] == 5
    assert both(pkg, lib, False, False, 1, 48, 256, 1, 0, True)[0] == 5 and both(pkg, lib, False, False, 1, 48, 256, 8, 0, True)[0] == 9
    assert both(pkg, lib, False, False, 1, 50, 256, 8)[0] == 5 and both(pkg, lib, False, False, 1, 48, 255, 8)[0] == 5
    assert both(pkg, lib, False, True, 1, 256, 256, 64)[0] == 8 and both(pkg, lib, False, True, 1, 272, 272, 64)[0] == 10
    assert both(pkg, lib, False, True, 1, 272, 272, 7)[0] == 6 and both(pkg, lib, False, True, 1, 784, 784, 64)[0] == 6
    assert both(pkg, lib, False, False, 1, 7, 1601, 1) == (5, 2, 1, 1)


def test_route_boundaries_transposed(pkg, lib):
    """rows % 32 / % 16 / % 8, narrow on and off, nprob 7 / 8, and 511 / 512 workgroups of the wide form, triangular and not."""
    seen = set()
    for tri in (False, True):
        for nprob in (1, 7, 8, 63, 64, 128):
            for rows in (8, 16, 24, 32, 48, 64, 72, 224, 256, 480, 512, 520, 2016, 2048, 4064, 4096):
                for narrow in (0, 1):
                    for mend in ((False,) if tri else (False, True)):
                        seen.add(both(pkg, lib, True, tri, 1, rows, rows if tri else 130, nprob, narrow, False, mend)[0])
    assert seen == {0, 11, 12, 13, 14, 15, 16}
    # 512 workgroups: 64 problems x 8 blocks of 32 columns (256 rows); 63 x 8 = 504 and 64 x 7 (224 rows) = 448 stay narrow
    assert both(pkg, lib, True, False, 1, 256, 130, 64) == (15, 8, 1, 64)
    assert both(pkg, lib, True, False, 1, 256, 130, 63) == (13, 16, 1, 63)
    assert both(pkg, lib, True, False, 1, 224, 130, 64) == (13, 14, 1, 64)
    assert both(pkg, lib, True, False, 1, 16352, 130, 1)[0] == 13                    # 511 blocks, one problem: nprob >= 8 is asked too
    assert both(pkg, lib, True, False, 1, 2048, 130, 8) == (15, 64, 1, 8) and both(pkg, lib, True, False, 1, 2016, 130, 8) == (13, 126, 1, 8)
    assert both(pkg, lib, True, False, 1, 2048, 130, 7, 1) == (11, 256, 1, 7)
    # triangular: paired blocks, (ncb + 1) / 2 workgroups per problem -- 480 rows = 15 blocks = 8 workgroups x 64 = 512; 63: 504
    assert both(pkg, lib, True, True, 1, 480, 480, 64) == (16, 8, 1, 64)
    assert both(pkg, lib, True, True, 1, 480, 480, 63) == (14, 15, 1, 63)
    assert both(pkg, lib, True, True, 1, 448, 448, 64) == (14, 14, 1, 64)             # 14 blocks = 7 workgroups x 64 = 448
    assert both(pkg, lib, True, True, 1, 224, 224, 128) == (16, 4, 1, 128) and both(pkg, lib, True, True, 1, 224, 224, 127) == (14, 7, 1, 127)
    # narrow: asked for and rows % 8 == 0, but never instead of the wide form
    assert both(pkg, lib, True, True, 1, 520, 520, 1, 1) == (12, 33, 1, 1) and both(pkg, lib, True, True, 1, 520, 520, 1, 0)[0] == 0
    assert both(pkg, lib, True, False, 1, 72, 520, 1, 1) == (11, 9, 1, 1) and both(pkg, lib, True, False, 1, 256, 130, 64, 1)[0] == 15
    assert both(pkg, lib, True, True, 1, 8, 8, 1, 1) == (12, 1, 1, 1)


def test_route_panels(pkg, lib):
    for trans in (False, True):
        for tri in (False, True):
            for kp in (16, 32, 48, 64, 512):
                for rows, kdim in ((16, 16), (32, 8), (32, 40), (32, 264), (128, 128), (272, 272), (4096, 4096)):
                    if tri and rows != kdim:
                        continue
                    assert both(pkg, lib, trans, tri, kp, rows, kdim, 3) == (R.mm_id(trans, tri), rows // 16, kp // 16, 3)


def test_every_refusal(pkg, lib):
    """Exactly the shapes a kernel cannot compute: its grid would not cover them or its loops would not reach their end."""
    lib.gmrf_last_error.restype = C.c_char_p
    for trans in (False, True):
        for tri in (False, True):
            sq = lambda rows, kdim: (rows, rows) if tri else (rows, kdim)            # noqa: E731
            for kp in (2, 15, 17, 24, 40):                                           # right-hand sides beyond the last 16 would be lost
                assert both(pkg, lib, trans, tri, kp, *sq(32, 32), 1) == R.REFUSED
            for rows in (8, 24, 40, 50):                                             # rows beyond the last 16 would be lost
                assert both(pkg, lib, trans, tri, 16, *sq(rows, 32), 1) == R.REFUSED
            assert b"multiple of 16" in lib.gmrf_last_error()
            if not tri:
                for kdim in (1, 4, 12, 20, 257):                                     # the K remainder beyond the last 8 would be lost
                    assert both(pkg, lib, trans, tri, 16, 32, kdim, 1) == R.REFUSED
                assert b"multiple of 8" in lib.gmrf_last_error()
            for rows, kdim in ((0, 16), (16, 0), (-16, 16), (16, -8)):
                for kp in (1, 16):
                    assert both(pkg, lib, trans, tri, kp, rows, kdim, 1) == R.REFUSED
            assert both(pkg, lib, trans, tri, 1, *sq(32, 32), 0) == R.REFUSED and both(pkg, lib, trans, tri, 0, *sq(32, 32), 1) == R.REFUSED
    # triangular is square
    for trans in (False, True):
        for kp in (1, 16):
            assert both(pkg, lib, trans, True, kp, 32, 64, 1) == R.REFUSED and both(pkg, lib, trans, True, kp, 64, 32, 1) == R.REFUSED
    # one right-hand side, transposed: rows no multiple of the chosen column block, or fewer than one block
    for tri in (False, True):
        for rows in (4, 8, 12, 24, 40, 100, 520):
            assert both(pkg, lib, True, tri, 1, rows, rows, 1, 0) == R.REFUSED
        for rows in (4, 12, 20, 100):
            assert both(pkg, lib, True, tri, 1, rows, rows, 1, 1) == R.REFUSED       # (narrow falls back to 16 when rows % 8 != 0)
        for rows in (8, 24, 40, 520):
            assert both(pkg, lib, True, tri, 1, rows, rows, 1, 1)[0] == R.fam(R.GEMV_T8, tri)
    # one right-hand side, not transposed: sweep_gemv_n takes every positive shape
    for tri in (False, True):
        for rows in (1, 2, 3, 5, 1603):
            assert both(pkg, lib, False, tri, 1, rows, rows, 1) == (R.fam(R.GEMV_N, tri), (rows + 3) // 4, 1, 1)


def test_kernel_preconditions_of_the_restatement():
    """kernel_route(id, ...) accepts exactly what route() can send to id, plus the shapes only a forced call reaches."""
    for trans in (False, True):
        for tri in (False, True):
            for kp in (1, 16):
                for rows in (8, 16, 32, 48, 50, 256, 272):
                    for kdim in ([rows] if tri else [2, 8, 255, 256, 258, 770]):
                        for nprob in (1, 8, 64):
                            for narrow in (0, 1):
                                for st in ((False,) if tri else (False, True)):
                                    r = R.route(trans, tri, kp, rows, kdim, nprob, narrow, st and not trans, st and trans)
                                    if r[0]:
                                        assert R.kernel_route(r[0], trans, tri, kp, rows, kdim, nprob, st and not trans, st and trans) == r
    assert R.kernel_route(7, False, False, 1, 48, 258, 1) == R.REFUSED and R.kernel_route(7, False, False, 1, 48, 256, 1, True) == R.REFUSED
    assert R.kernel_route(9, False, False, 1, 48, 256, 1) == (9, 3, 1, 1) and R.kernel_route(9, False, False, 1, 48, 2048, 1) == (9, 3, 1, 1)
    assert R.kernel_route(9, False, False, 1, 50, 256, 1) == R.REFUSED and R.kernel_route(10, False, False, 1, 48, 256, 1) == R.REFUSED
    assert R.kernel_route(15, True, False, 1, 48, 16, 1) == R.REFUSED and R.kernel_route(15, True, False, 1, 64, 16, 1) == (15, 2, 1, 1)
    assert R.kernel_route(13, False, False, 1, 64, 16, 1) == R.REFUSED and R.kernel_route(1, False, False, 1, 64, 16, 1) == R.REFUSED


KEYS = ("trans", "tri", "kp", "rows", "kdim", "nprob", "narrow", "has_kst", "has_mend")


def _layouts():
    for bsp in range(64, 4096 + 1, 64):
        for cmin in range(0, bsp, 64):
            yield bsp, cmin


def test_no_product_of_todays_handles_is_refused(pkg, lib):
    """Every launch_sweep call of sweep_launches over bsp = 64 .. 4096, every (cmin, rmax) set_layout accepts, the split point
    planned_xsplit gives, kp in 1, 16, 48, 64 and 1, 7, 8, 64 problems, both directions -- and the factorisation's forward product --
    is accepted by the restatement; the library agrees on every distinct argument tuple.  So the truncation launch_sweep now
    refuses was never reached."""
    distinct = {}
    n_products = 0
    for nprob in (1, 7, 8, 64):
        for kp in (1, 16, 48, 64):
            for backward in (False, True):
                widest = {}
                for bsp, cmin in _layouts():
                    if R.via_gemm(bsp, kp, nprob):
                        assert R.products(bsp, cmin, 64, 0, kp, nprob, backward) == []
                        continue
                    xs = R.planned_xsplit(bsp, cmin, nprob)
                    assert xs == 0 or (xs % 64 == 0 and 256 <= xs < bsp and xs <= cmin)
                    blocks = R.block_products(bsp, xs, kp, nprob, backward)
                    assert len(blocks) == (3 if xs else 1) and R.products(bsp, cmin, 64, xs, kp, nprob, backward)[1:] == blocks
                    n_products += (len(blocks) + 1) * (bsp // 64)
                    for pr in blocks:
                        distinct.setdefault(tuple(pr[k] for k in KEYS), pr["name"])
                    key = (bsp - cmin, R.coupling_product(bsp, cmin, 64, kp, nprob, backward)["narrow"])
                    widest[key] = max(widest.get(key, 0), bsp)
                # the coupling product depends on (bsp, cmin, rmax) through bsp - cmin, rmax and `narrow` alone, and rmax runs up
                # to bsp: the widest block of each (bsp - cmin, narrow) has them all
                for (wc, narrow), bsp in widest.items():
                    for rmax in range(64, bsp + 1, 64):
                        pr = R.coupling_product(bsp, bsp - wc, rmax, kp, nprob, backward)
                        assert pr["narrow"] == narrow
                        distinct.setdefault(tuple(pr[k] for k in KEYS), pr["name"])
    for nprob in (1, 7, 8, 64):
        pr = R.factor_forward_product(nprob)
        distinct.setdefault(tuple(pr[k] for k in KEYS), pr["name"])
    reached = set()
    for args, name in distinct.items():
        r = R.route(*args)
        assert r[0] != 0, ("refused", name, args)
        assert R.kernel_route(r[0], *args[:6], *args[7:]) == r
        assert hook_route(pkg, lib, *args) == r, (name, args)
        reached.add(r[0])
    print(f"{n_products} products over the grid, {len(distinct)} distinct argument tuples, kernels reached: {sorted(reached)}")
    assert reached == set(range(1, 17))


# ------------------------------------------------------------------------------------------ the product hook's refusals
def product_status(pkg, lib, case, force=0, **over):
    """gmrf_test_sweep_product's status for a case with fields of its description or call overridden (never reaches a device
    when it refuses: the refusals come before the upload)."""
    d = case.desc()
    names = ("trans", "tri", "kp", "rows", "kdim", "nprob", "narrow", "has_kst", "has_mend", "ld", "ldx", "ldb", "ldo", "pMat", "pXin", "pBin", "pOut")
    for k, v in over.items():
        if k in names:
            d[names.index(k)] = v
    Mat, P = np.zeros(over.get("nMat", case.nMat)), np.zeros(over.get("nP", case.nP))
    kst, mend = over.get("kst", case.kst), over.get("mend", case.mend)
    kst = None if kst is None else np.asarray(kst, np.int32)
    mend = None if mend is None else np.asarray(mend, np.int32)
    ran = C.c_int32(-1)
    p = pkg._cabi.ptr
    st = lib.gmrf_test_sweep_product(0, force, p(d), p(Mat), len(Mat), p(P), len(P), over.get("x_off", case.x_off), over.get("b_off", case.b_off),
                                     over.get("o_off", case.o_off), p(kst), 0 if kst is None else len(kst), p(mend), 0 if mend is None else len(mend),
                                     C.byref(ran))
    return st, ran.value


def test_product_hook_refuses_before_it_uploads(pkg, lib):
    BAD = pkg._cabi.ERR_BAD_SHAPE
    ref = lambda case, force=0, **over: product_status(pkg, lib, case, force, **over) == (BAD, 0)        # noqa: E731
    gn = R.Case(False, False, 1, 48, 130, sub="apart")
    # a forced kernel whose preconditions the shape does not meet
    assert ref(gn, 7 + 1) and ref(gn, 13) and ref(gn, 1) and ref(gn, 17) and ref(gn, -1)
    assert ref(R.Case(False, False, 1, 48, 258), 7) and ref(R.Case(False, False, 1, 50, 130), 9) and ref(R.Case(True, False, 1, 48, 130), 15)
    assert ref(R.Case(False, False, 1, 128, 256, kst=[0, 64]), 7)
    # a refused route
    assert ref(R.Case(False, False, 16, 24, 32)) and ref(R.Case(False, False, 16, 32, 20)) and ref(R.Case(True, True, 1, 24, 24))
    # extents
    assert ref(gn, nMat=gn.pMat - 6 - 3) and ref(gn, nP=gn.nP - 3 - 1 - 5 - gn.ldb + gn.rows)
    assert ref(gn, ld=128) and ref(gn, nprob=2) and ref(gn, x_off=-2) and ref(gn, o_off=gn.nP - 40)
    mm = R.Case(True, False, 16, 32, 40, nprob=3, sub="inplace")
    assert ref(mm, nMat=mm.nMat - 6 - 3) and ref(mm, ldx=38) and ref(mm, ldo=30) and ref(mm, nprob=4)
    # alignment under 16-byte loads
    assert ref(gn, ld=133) and ref(gn, x_off=3) and ref(R.Case(False, False, 1, 48, 130, nprob=2), pMat=48 * 132 + 7)
    assert ref(R.Case(False, False, 1, 48, 130, nprob=2), pXin=133) and ref(R.Case(False, False, 16, 32, 40), ldx=43)
    assert ref(R.Case(True, False, 1, 64, 300), ld=67)
    # staircases
    st = R.Case(False, False, 1, 130, 300, kst=[0, 64, 128])
    assert ref(st, kst=[0, 64]) and ref(st, kst=[0, 63, 128]) and ref(st, kst=[0, 64, 302]) and ref(st, kst=[0, -2, 128]) and ref(st, has_kst=0)
    assert ref(R.Case(False, False, 16, 128, 128, kst=[0, 64]), kst=[0, 60]) and ref(R.Case(True, False, 16, 128, 128, mend=[64, 128]), mend=[64, 124])
    assert ref(R.Case(True, False, 1, 128, 128, mend=[64, 128]), mend=[64, 130]) and ref(R.Case(True, False, 1, 128, 128, mend=[64, 128]), mend=[63, 128])
    assert ref(R.Case(False, True, 1, 128, 128), kst=[0, 64], has_kst=1) and ref(R.Case(False, False, 1, 128, 128), mend=[64, 128], has_mend=1)
    # overlaps: the input with the output, two problems' outputs, an addend with another output
    assert ref(gn, x_off=gn.o_off - 2) and ref(gn, o_off=gn.x_off + 128) and ref(gn, b_off=gn.o_off + 2)
    two = R.Case(False, False, 1, 48, 130, nprob=2, sub="inplace")
    assert ref(two, pOut=40, pBin=40) and ref(two, pBin=two.pOut + 2)


# ------------------------------------------------------------------------------------------ the reference and its bound
EMULATED = {
    "dense gemv": dict(trans=False, tri=False, kp=1, rows=48, kdim=130, sub="apart"),
    "triangular gemv": dict(trans=False, tri=True, kp=1, rows=144, kdim=144, sub="none"),
    "triangular transposed": dict(trans=True, tri=True, kp=1, rows=48, kdim=48, sub="inplace"),
    "staircase": dict(trans=False, tri=False, kp=1, rows=128, kdim=256, kst=[0, 64], nprob=2, sub="inplace"),
    "mend panel": dict(trans=True, tri=False, kp=16, rows=128, kdim=128, mend=[64, 128], sub="apart"),
    "long": dict(trans=False, tri=False, kp=1, rows=7, kdim=1601, sub="apart"),
}


@pytest.fixture(scope="module")
def emulated():
    return {k: R.Case(**v) for k, v in EMULATED.items()}


@pytest.mark.parametrize("name", sorted(EMULATED))
def test_fp64_emulations_stay_within_the_bound(emulated, name):
    case = emulated[name]
    for order in ("ascending", "pairwise"):
        ratio = case.check(R.emulate(case, order), f"{name}, {order}")
        print(f"{name}, {order}: worst error / bound {ratio:.3f}")
        assert 0 < ratio <= 1


@pytest.mark.parametrize("name,mutation", [
    ("dense gemv", "last term"), ("dense gemv", "k group"), ("dense gemv", "float32"), ("dense gemv", "added"),
    ("triangular gemv", "last term"), ("triangular gemv", "tri short"), ("triangular gemv", "float32"),
    ("triangular transposed", "tri short"), ("triangular transposed", "added"),
    ("staircase", "stair 64"), ("staircase", "k group"), ("staircase", "added"),
    ("mend panel", "stair 64"), ("mend panel", "last term"), ("mend panel", "float32"), ("long", "last term"), ("long", "float32"),
])
def test_the_reference_catches_each_defect(emulated, name, mutation):
    case = emulated[name]
    for order in ("ascending", "pairwise"):
        with pytest.raises(AssertionError, match="beyond the bound"):
            case.check(R.emulate(case, order, mutation), f"{name}, {mutation}")


def test_a_read_outside_the_contract_is_not_finite(emulated):
    """The generator's NaN: a staircase bound moved the other way, a triangular row read one tile too far."""
    case = emulated["staircase"]
    B = case.blocks()
    assert np.all(np.isnan(B[:, 64:128, :64])) and np.all(np.isfinite(B[:, 64:128, 64:256])) and np.all(np.isnan(B[:, :, 256:]))
    tri = emulated["triangular gemv"]
    T = tri.blocks()[0]
    assert np.all(T[:64, :64][np.triu_indices(64, 1)] == 0.0) and np.all(np.isnan(T[:64, 64:])) and np.all(np.isnan(T[64:128, 128:]))
    assert np.all(np.isfinite(T[:, :144][np.tril_indices(144)]))
    out = R.emulate(tri)
    out[0, 0, 5] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        tri.check(out)


def test_panel_check_sees_a_stray_write(emulated):
    case = emulated["staircase"]
    before = case.panel()
    after = before.copy()
    after[case.out_cells()] = R.emulate(case)
    out, ratio = case.check_panel(before, after)
    assert ratio <= 1
    for cell in (0, case.x_off + 3, case.o_off + case.rows, case.nP - 1, case.x_off + case.kdim):
        stray = after.copy()
        stray[cell] = 1.0
        with pytest.raises(AssertionError, match="outside the outputs"):
            case.check_panel(before, stray)
