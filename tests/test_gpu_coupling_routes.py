"""Every route of the coupling step C_i = B_i Linv_{i-1}^T (spmm_bxt<8|16|32>, spmm_bxt_tiles with its product, zero and scatter
roles, the dense GEMM), one launch at a time through gmrf_test_coupling_product on handles that gmrf_bt_factor_begin_csc has
prepared, at the smallest shapes at which each mechanism exists (tests/bxt_ref.py has the patterns, the restatement of plan and
route, the longdouble reference and the derived bound).  Every call: the route it reports against the restatement; every cell of
the whole image of the coupling blocks -- inside block i's window within (L_r + 1) 2^-53 sum |b||x| of the reference or, left of
its tile's staircase start only, still the sentinel; everywhere else the sentinel, bit for bit -- and the Schur work block
exactly.  Linv holds NaN wherever the route may not read.  All launches of a case agree bit for bit on the cells both wrote, and
a problem of a batch is bitwise that problem alone.

Two limits of the contract, by construction of the routes: the dense GEMM multiplies the structural zeros of B's image with every
column >= cm of Linv, so for it only rows and columns < cm hold NaN; blocks of 320 are padded to 512, so there the scatter role
is refused and the zero role is the library's own choice (the fold is pinned at 128 and 256)."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import bxt_ref as R

pytestmark = pytest.mark.gpu

BAD_SHAPE = -2


class Handle:
    """A solver handle through the C ABI: batch, switches, tile grouping, then gmrf_bt_factor_begin_csc (analysis, storage, values
    of the problems p0 .. p0 + B - 1) and no step."""

    def __init__(self, pkg, lib, name, B=1, p0=0, switches=0, group=None):
        self.cabi, self.lib, self.name, self.B, self.p0, self.switches = pkg._cabi, lib, name, B, p0, switches
        self.pat = R.case(name)
        self.group = (B >= 8) if group is None else group
        self.P = R.case_plan(name, self.group)
        self.h = C.c_void_p()
        chk, p = self.cabi.check, self.cabi.ptr
        chk(lib.gmrf_bt_create(0, None, C.byref(self.h)))
        try:
            chk(lib.gmrf_bt_set_batch(self.h, B))
            chk(lib.gmrf_bt_set_eager(self.h, switches))
            if group is not None:
                chk(lib.gmrf_test_coupling_group_tiles(self.h, int(group)))
            self.vals = [R.case_refs(name, 1, p0 + q)[0] for q in range(B)]
            nz = np.ascontiguousarray(np.stack(self.vals))
            chk(lib.gmrf_bt_factor_begin_csc(self.h, self.pat.n, self.pat.N, p(self.pat.colptr), p(self.pat.rowval), p(nz), 0))
            chk(lib.gmrf_bt_synchronize(self.h))
            import torch
            self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        except Exception:
            self.close()
            raise

    def close(self):
        if self.h:
            self.lib.gmrf_bt_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def own_route(self, i):
        return R.route(self.pat, self.P, self.B, self.cus, i, self.switches)

    def call(self, i, force, over, X, Cimg, S):
        r = np.full(10, -1, np.int64)
        p = self.cabi.ptr
        ov = None if over is None else np.array(over, np.int32)
        st = self.lib.gmrf_test_coupling_product(self.h, i, force, p(ov), p(X), X.size, p(Cimg), Cimg.size, p(S), S.size, p(r))
        return st, tuple(int(v) for v in r)

    def product(self, i, force=0, cw=0, nch=0, skip_dead=0, fill=0, what=""):
        """One launch on sentinels; everything checked.  Returns (route, outputs [B][rm][W], written masks, worst ratio, cells)."""
        pat, P, B = self.pat, self.P, self.B
        own = self.own_route(i)
        kind = own[0] if force == 0 else {1: R.BXT, 2: R.TILES, 3: R.DENSE}[force]
        base = own if force == 0 else R.route_of(pat, P, kind, B, self.cus, i, self.switches)
        want = R.with_overrides(pat, P, base, B, cw, nch, skip_dead, fill)
        what = f"{self.name} block {i} B {B} p0 {self.p0} {'grouped' if self.group else 'alone'} force {force} cw {cw} nch {nch} skip {skip_dead} fill {fill} {what}"
        refs, Xs = [], []
        for q in range(B):
            _, _, X, ref, bound = R.case_refs(self.name, i, self.p0 + q)
            refs.append((ref, bound))
            Xs.append(R.poison_x(pat, P, i, X, kind))
        X = np.ascontiguousarray(np.stack(Xs))
        Cimg = R.sentinel(int(np.prod(R.c_image_shape(pat, P, B))))
        S = R.sentinel(B * pat.bsp * pat.bsp)
        st, ran = self.call(i, force, (cw, nch, skip_dead, fill), X, Cimg, S)
        assert st == 0, (what, st, self.lib.gmrf_last_error())
        assert ran == want, (what, "ran", ran, "restatement", want)
        written, worst, cells = R.check_c(pat, P, i, B, Cimg, refs, what)
        R.check_s(pat, P, i, B, S, ran[7], self.vals, what)
        out = Cimg.reshape(R.c_image_shape(pat, P, B))[:, i - 1].copy()
        return ran, out, written, worst, cells

    def refused(self, i, force, over, what):
        pat, P, B = self.pat, self.P, self.B
        X = np.zeros(B * pat.bsp * pat.bsp)
        Cimg = R.sentinel(int(np.prod(R.c_image_shape(pat, P, B))))
        S = R.sentinel(B * pat.bsp * pat.bsp)
        st, _ = self.call(i, force, over, X, Cimg, S)
        assert st == BAD_SHAPE, (self.name, what, st)
        assert (R.bits(Cimg) == R.SENT).all() and (R.bits(S) == R.SENT).all(), (self.name, what, "touched a buffer")


class Tally:
    def __init__(self, case):
        self.case, self.by = case, {}

    def add(self, ran, worst, cells):
        k = R.ROUTE_NAMES[ran[0]]
        c, w, n = self.by.get(k, (0, 0.0, 0))
        self.by[k] = (c + cells, max(w, worst), n + 1)

    def report(self):
        for k, (cells, worst, calls) in self.by.items():
            assert worst <= 1.0
            print("COUPLING_RATIO " + json.dumps({"case": self.case, "route": k, "calls": calls, "cells": cells, "ratio": round(worst, 4)}))


def sweep(H, tally, routes=(0, 1, 2, 3), cws=(16, 32, 64), nchs=(1, 3, 8, 16)):
    """Blocks 1 and 2 on every admitted route and override of the handle; all outputs of a block tied bitwise (the dense GEMM, which
    sums in another order, within the bound only).  Returns {block: (output, written)} of the own choice."""
    pat, P, B = H.pat, H.P, H.B
    W, rm = pat.bsp - P["cmin"], P["rmax"]
    plan_ok = P["bxt_ok"]
    res = {}
    for i in (1, 2):
        runs = []

        def go(**kw):
            ran, out, written, worst, cells = H.product(i, **kw)
            tally.add(ran, worst, cells)
            if ran[0] != R.DENSE:
                runs.append((kw, out, written))
            return ran, out, written

        ran, out, written = go(force=0)
        assert ran == H.own_route(i)
        res[i] = (out, written)
        if 1 in routes and P["sparse_b"]:
            for cw in cws:
                if W % cw == 0:
                    go(force=1, cw=cw, fill=1 if cw == 32 else 0)
        if 2 in routes and plan_ok:
            for k, nch in enumerate(n for n in nchs if n <= W // 16):
                for sd in (1, 2):
                    f = (0, 2 if rm < pat.bsp else 1, 3 if (B == 1 and pat.bsp == pat.bs) else 1, 1)[(2 * k + sd - 1) % 4]
                    go(force=2, nch=nch, skip_dead=sd, fill=f)
        if 3 in routes:
            go(force=3)
        for kw, o, w in runs[1:]:
            for q in range(B):
                R.tie(runs[0][1][q], runs[0][2][q], o[q], w[q], f"{H.name} block {i} problem {q}: {runs[0][0]} against {kw}")
    return res


def batches_are_their_problems(pkg, lib, name, tally, sizes=(3, 8, 16), forces=(0, 1)):
    """Problem p of a batch is bitwise the problem alone on the same kernel (8 and 16: the % 8 == 0 workgroup mapping)."""
    alone = {}
    for B in sizes:
        with Handle(pkg, lib, name, B=B) as H:
            for i in (1, 2):
                for force in forces:
                    if force == 2 and not H.P["bxt_ok"]:
                        continue
                    ran, out, written, worst, cells = H.product(i, force=force)
                    tally.add(ran, worst, cells)
                    for q in (0, 1, B // 2, B - 1):
                        if (q, i, ran[0]) not in alone:
                            # the same kernel family; tiles: the same grouping as the batch's plan
                            with Handle(pkg, lib, name, B=1, p0=q, group=H.group) as A:
                                f1 = {R.DENSE: 3, R.BXT: 1, R.TILES: 2}[ran[0]]
                                r1, o1, w1, worst1, cells1 = A.product(i, force=f1, fill=1)
                                tally.add(r1, worst1, cells1)
                                alone[(q, i, ran[0])] = (o1[0], w1[0])
                        R.tie(out[q], written[q], *alone[(q, i, ran[0])], f"{name} block {i}: problem {q} of {B} against alone")


# ------------------------------------------------------------------------------------------------ the cases
def test_band(pkg, lib):
    """bs 128, tridiagonal band: the base case, every route, B in {1, 3, 8, 16}."""
    t = Tally("band")
    for B in (1, 3, 8, 16):
        with Handle(pkg, lib, "band", B=B) as H:
            assert H.own_route(1)[0] == R.TILES
            sweep(H, t)
    batches_are_their_problems(pkg, lib, "band", t)
    t.report()


def test_window(pkg, lib):
    """bs 256, cm 64, rm 128 < bsp, kst [0, 128]: cells left of the staircase, the zero fill by zero_rows and by the zero role,
    the scatter role over a block whose lower rows the product does not write."""
    t = Tally("window")
    for B in (1, 3, 8):
        with Handle(pkg, lib, "window", B=B) as H:
            own = H.own_route(1)
            assert own[7] == (R.FILL_SCATTER_ROLE if B == 1 else R.FILL_ZERO_ROLE)
            res = sweep(H, t)
            # tile 1 left of its staircase start: the tile kernel leaves the sentinel, nobody writes a value that is not an exact zero
            assert not res[1][1][0][64:128, :128].any()
        with Handle(pkg, lib, "window", B=B, switches=R.SW_DENSE_COUPLING) as H:
            assert H.own_route(2)[0] == R.DENSE and H.own_route(2)[7] == R.FILL_ZERO_ROWS
            sweep(H, t, routes=(0,))
    batches_are_their_problems(pkg, lib, "window", t, sizes=(3, 8))
    t.report()


def test_ragged(pkg, lib):
    """bs 320 (bsp 512), cm 192, W 320 = 20 chunks, rm 320: the second 256-row chunk of spmm_bxt has 64 live rows; nch 3, 8, 16 leave
    partial last column groups and, with kst [0, 0, 0, 64, 64], column groups that begin left of a tile group's first chunk; cw 64
    gives five column chunks; a 3-tile group beside single tiles, grouped against every tile alone."""
    t = Tally("ragged")
    outs = {}
    for group in (True, False):
        with Handle(pkg, lib, "ragged", B=1, group=group) as H:
            assert H.own_route(1)[5] == (3 if group else 5) and H.own_route(1)[7] == R.FILL_ZERO_ROLE       # padded blocks: no scatter role
            outs[group] = sweep(H, t)
            H.refused(1, 2, (0, 24, 0, 0), "nch above W / 16")
            H.refused(1, 2, (0, 5, 0, 0), "nch outside the launcher's list")
            H.refused(1, 1, (48, 0, 0, 0), "cw 48")
            H.refused(1, 2, (0, 0, 0, 3), "scatter role on padded blocks")
            H.refused(1, 1, (0, 0, 0, 2), "zero role outside the tile route")
            H.refused(0, 0, None, "block 0")
    for i in (1, 2):
        R.tie(outs[True][i][0][0], outs[True][i][1][0], outs[False][i][0][0], outs[False][i][1][0], f"ragged block {i}: grouped against alone")
    with Handle(pkg, lib, "ragged", B=8) as H:
        sweep(H, t, nchs=(3, 16))
    t.report()


@pytest.mark.parametrize("km", [8, 16, 32])
def test_rows(pkg, lib, km):
    """Rows of 0, 1, 3, 4, 5, 8 (9, 16 (17, 32)) entries mixed, an empty tile in block 2: spmm_bxt<8|16|32>, the 4-entry padding."""
    t = Tally(f"rows{km}")
    for B in (1, 3):
        with Handle(pkg, lib, f"rows{km}", B=B) as H:
            assert R.route_of(H.pat, H.P, R.BXT, B, H.cus, 1)[1] == km
            sweep(H, t)
    t.report()


def test_rows_of_33_go_dense(pkg, lib):
    t = Tally("rows33")
    with Handle(pkg, lib, "rows33", B=1) as H:
        assert H.own_route(1)[0] == R.DENSE
        sweep(H, t, routes=(0, 3))
        H.refused(1, 1, None, "spmm_bxt with a row of 33")
        H.refused(1, 2, None, "tiles without a plan")
    t.report()


def test_ucap(pkg, lib):
    """bs 512: a tile group on exactly 256 distinct columns (every thread gathers one); 257 refuse the plan and the library's own
    choice falls back to spmm_bxt (tied bitwise to the tile route on 256, held to the same bound on 257)."""
    t = Tally("ucap")
    with Handle(pkg, lib, "ucap256", B=1) as H:
        assert H.own_route(1)[0] == R.TILES and (np.diff(H.P["uptr"][1]) == 256).any()
        sweep(H, t, nchs=(1, 8))
    with Handle(pkg, lib, "ucap257", B=1) as H:
        assert H.own_route(1)[0] == R.BXT
        sweep(H, t, routes=(0, 1, 3), cws=(16, 64))
        H.refused(1, 2, None, "tiles without a plan")
    t.report()


def test_lds_gate(pkg, lib):
    """bs 256: a group of 1536 padded entries fills the plan's LDS capacity to the last slot; 1540 refuse the plan."""
    t = Tally("lds")
    with Handle(pkg, lib, "lds1536", B=1) as H:
        assert H.P["ecap"] == 1536 and H.own_route(1)[0] == R.TILES
        sweep(H, t, nchs=(1, 16))
    with Handle(pkg, lib, "lds1540", B=1) as H:
        assert H.own_route(1) == R.route_of(H.pat, H.P, R.BXT, 1, H.cus, 1) and H.own_route(1)[1] == 32
        sweep(H, t, routes=(0, 3))
        H.refused(1, 2, None, "tiles without a plan")
    t.report()


def test_padded_blocks(pkg, lib):
    """bs 100 (bsp 128): pad rows and columns empty; the scatter role is refused; with rows < 64 only the zero role is the own choice."""
    t = Tally("padded")
    with Handle(pkg, lib, "padded100", B=1) as H:
        assert H.own_route(1)[7] == R.FILL_NONE and H.P["rmax"] == 128
        sweep(H, t)
        H.refused(1, 2, (0, 0, 0, 3), "scatter role on padded blocks")
        H.refused(1, 2, (0, 0, 0, 2), "zero role without rows below rmax")
    for B in (1, 3):
        with Handle(pkg, lib, "padded64", B=B) as H:
            assert H.own_route(1)[0] == R.TILES and H.own_route(1)[7] == R.FILL_ZERO_ROLE
            sweep(H, t)
            H.refused(2, 0, (0, 0, 0, 3), "scatter role on padded blocks")
    t.report()


def test_scatter_fold(pkg, lib):
    """One problem, unpadded blocks: the scatter role is the library's own choice (bs 128: the whole block, rm = bsp; bs 256 with
    rm 128), and off under NO_SCATTER_FOLD; bs 320 is padded to 512: the zero role."""
    t = Tally("fold")
    for name, folded, unfolded in (("band", R.FILL_SCATTER_ROLE, R.FILL_NONE), ("window", R.FILL_SCATTER_ROLE, R.FILL_ZERO_ROLE),
                                   ("ragged", R.FILL_ZERO_ROLE, R.FILL_ZERO_ROLE)):
        for sw, fill in ((0, folded), (R.SW_NO_SCATTER_FOLD, unfolded)):
            with Handle(pkg, lib, name, B=1, switches=sw) as H:
                for i in (1, 2):
                    ran, out, written, worst, cells = H.product(i)
                    assert ran[0] == R.TILES and ran[7] == fill, (name, sw, ran)
                    t.add(ran, worst, cells)
        with Handle(pkg, lib, name, B=3) as H:
            H.refused(1, 2, (0, 0, 0, 3), "scatter role on a batch")
    t.report()


def test_wrong_buffers_are_refused(pkg, lib):
    with Handle(pkg, lib, "band", B=3) as H:
        pat, P = H.pat, H.P
        nC = int(np.prod(R.c_image_shape(pat, P, 3)))
        X, Cimg, S = np.zeros(3 * 128 * 128), R.sentinel(nC), R.sentinel(3 * 128 * 128)
        for a, b, c in ((X[:-1], Cimg, S), (X, Cimg[:-1], S), (X, Cimg, S[:-1]), (X[:128 * 128], Cimg, S)):
            st, _ = H.call(1, 0, None, np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))
            assert st == BAD_SHAPE
        st, _ = H.call(3, 0, None, X, Cimg, S)
        assert st == BAD_SHAPE
        st, _ = H.call(1, 4, None, X, Cimg, S)
        assert st == BAD_SHAPE


# ------------------------------------------------------------------------------------------------ handle level
def test_new_pattern_on_a_used_handle_rezeroes_c(pkg):
    """A handle that factored pattern P1 then factors P2 -- the same n, blocks, cmin and rmax, the staircase further right -- and
    gives C_i and the solve of a fresh handle bit for bit: the cells of C that P1's products wrote and P2's kernels skip (left of
    the new staircase start) are cleared by the new analysis (c_dirty)."""
    import scipy.sparse as sp
    bs, N = 256, 3

    def matrix(start):
        lo = [(r, 64 + r % 64) for r in range(64)] + [(r, c) for r in range(64, 128) for c in (start + (r - 64) // 2, 192 + r - 64)]
        pat = R.Pattern(bs, [None, lo, lo + [(3, 70)]])
        v = pat.values(0)
        L = sp.csc_matrix((v, pat.rowval, pat.colptr), shape=(pat.n, pat.n))
        low = sp.tril(L, -1)
        Q = sp.csc_matrix(sp.tril(L) + low.T)
        Q.sort_indices()
        return pat, Q

    (p1, Q1), (p2, Q2) = matrix(70), matrix(200)
    P1, P2 = R.plan(p1, False), R.plan(p2, False)
    assert (P1["cmin"], P1["rmax"]) == (P2["cmin"], P2["rmax"]) == (64, 128) and list(P1["kst"][:2]) == [0, 0] and list(P2["kst"][:2]) == [0, 128]
    rhs = np.random.default_rng(3).standard_normal(p1.n)
    used = pkg.tridiagonal_cholesky(Q1, N)
    fresh = None
    try:
        first = [used.get_block(1, i) for i in range(N - 1)]
        assert np.abs(first[0][64:128, 64:192]).max() > 0            # P1 wrote where P2's staircase starts later
        used.factor(Q2, N)
        fresh = pkg.tridiagonal_cholesky(Q2, N)
        for i in range(N - 1):
            a, b = used.get_block(1, i), fresh.get_block(1, i)
            assert np.array_equal(a, b), ("C", i, np.argwhere(a != b)[:1])
            assert not a[64:128, 64:192].any()
        assert np.array_equal(pkg.ldiv(used, rhs), pkg.ldiv(fresh, rhs))
    finally:
        # (the handles hold CUs of the device's budget for persistent launches until they are destroyed: not left to the collector)
        used.close()
        if fresh is not None:
            fresh.close()
