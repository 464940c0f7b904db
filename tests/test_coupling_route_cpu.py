"""The coupling step's host side without a GPU: the plan build_symbolic makes for a pattern (gmrf_test_coupling_plan) against the
NumPy restatement of tests/bxt_ref.py array by array, every boundary and refusal of the plan, the route rule's fields, and
planted defects that the checks of tests/test_gpu_coupling_routes.py must catch."""
import numpy as np
import pytest

from tests import bxt_ref as R


def _same_plan(lib_p, ref_p, what):
    for k in ("cmin", "rmax", "max_row", "sparse_b", "bxt_ok", "ecap", "nrt"):
        assert lib_p[k] == ref_p[k], (what, k, lib_p[k], ref_p[k])
    for k in ("kst", "rowptr"):
        assert np.array_equal(lib_p[k], ref_p[k]), (what, k)
    if ref_p["bxt_ok"]:
        for k in ("ng", "gtiles", "uptr", "ucols", "lidx"):
            assert np.array_equal(lib_p[k], ref_p[k]), (what, k, lib_p[k], ref_p[k])


@pytest.mark.parametrize("group_tiles", [True, False], ids=["grouped", "alone"])
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_library_plan_is_the_restatement(pkg, lib, name, group_tiles):
    pat = R.case(name)
    got, _ = R.lib_plan(pkg._cabi, lib, pat, group_tiles)
    _same_plan(got, R.case_plan(name, group_tiles), (name, group_tiles))


def test_case_geometry():
    """What the cases of the GPU file are there for, stated on the restatement (which the test above ties to the library)."""
    P = R.case_plan("window", True)
    assert (P["cmin"], P["rmax"], list(P["kst"])) == (64, 128, [0, 128, 192, 192])
    P = R.case_plan("ragged", True)
    assert (R.case("ragged").bsp, P["cmin"], P["rmax"], list(P["kst"][:5])) == (512, 192, 320, [0, 0, 0, 64, 64])
    for i in (1, 2):
        assert P["ng"][i] == 3 and P["gtiles"][i].tolist()[:3] == [[0, 1, 2], [3, -1, -1], [4, -1, -1]]
    A = R.case_plan("ragged", False)
    assert A["ng"][1] == 5 and (A["gtiles"][1][:, 1:] == -1).all()
    # per-block offsets matter: the two lower blocks differ in pattern in every case
    for name in R.ALL_CASES:
        pat = R.case(name)
        assert not np.array_equal(pat.lower[1], pat.lower[2]), name
    # an empty tile leads a group of its own; a row of 3 entries is padded to 4, of 5 to 8
    P = R.case_plan("rows32", True)
    assert P["gtiles"][2].tolist()[0] == [0, -1, -1] and P["uptr"][2][1] == P["uptr"][2][0]
    assert R.case_plan("padded100", True)["rmax"] == 128 and R.case_plan("padded64", True)["rmax"] == 64


def test_boundaries_and_refusals(pkg, lib):
    km = {n: R.route(R.case(n), R.case_plan(n, True), 1, 256, 1) for n in ("rows8", "rows16", "rows32", "rows33")}
    assert [R.case_plan(n, True)["max_row"] for n in ("rows8", "rows16", "rows32", "rows33")] == [8, 16, 32, 33]
    assert km["rows33"][0] == R.DENSE and not R.case_plan("rows33", True)["sparse_b"]
    for n, want in (("rows8", 8), ("rows16", 16), ("rows32", 32)):
        r = R.route_of(R.case(n), R.case_plan(n, True), R.BXT, 1, 256, 1)
        assert r[1] == want and km[n][0] == R.TILES
    # 8|9 and 16|17: one more entry in one row moves KM
    for base, top in ((8, 16), (16, 32)):
        pat = R.case(f"rows{base}")
        r0 = next(r for r in range(128) if (pat.lower[1][:, 0] == r).sum() == base)
        free = next(c for c in range(128) if c not in set(pat.lower[1][pat.lower[1][:, 0] == r0][:, 1]))
        more = R.Pattern(128, [None, [tuple(e) for e in pat.lower[1]] + [(r0, free)], [tuple(e) for e in pat.lower[2]]])
        got, r = R.lib_plan(pkg._cabi, lib, more, True, query=(1, 256, 1, 0))
        assert got["max_row"] == base + 1
        P = R.plan(more, True)
        _same_plan(got, P, ("rows", base + 1))
        assert R.route_of(more, P, R.BXT, 1, 256, 1)[1] == top
    # 256 | 257 distinct columns in a tile
    assert R.case_plan("ucap256", True)["bxt_ok"] and not R.case_plan("ucap257", True)["bxt_ok"]
    assert R.route(R.case("ucap256"), R.case_plan("ucap256", True), 1, 256, 1)[0] == R.TILES
    assert R.route(R.case("ucap257"), R.case_plan("ucap257", True), 1, 256, 1)[0] == R.BXT
    # 1536 padded entries fit the LDS gate, 1537 .. 1600 (here 1540) do not
    for g in (True, False):
        a, b = R.case_plan("lds1536", g), R.case_plan("lds1540", g)
        assert (a["pmax"], a["ecap"], a["bxt_ok"]) == (1536, 1536, True), a["pmax"]
        assert (b["pmax"], b["bxt_ok"]) == (1540, False)
    # bsp = 64: one tile, sparse, a plan
    small = R.Pattern(64, [None, [(r, c) for r in range(64) for c in (r, (r + 9) % 64)], [(r, r) for r in range(64)]])
    got, r = R.lib_plan(pkg._cabi, lib, small, True, query=(1, 256, 2, 0))
    P = R.plan(small, True)
    _same_plan(got, P, "bsp 64")
    assert P["bxt_ok"] and r == R.route(small, P, 1, 256, 2) and r[0] == R.TILES and r[7] == R.FILL_SCATTER_ROLE


def test_greedy_join_ignores_the_lds_gate(pkg, lib, capsys):
    """A fact, recorded: the greedy grouping looks at the distinct columns only.  Three tiles of 64 x 12 entries on the same columns
    are joined (2304 padded entries), the LDS gate then refuses the whole plan, though every tile alone (768) fits."""
    g, _ = R.lib_plan(pkg._cabi, lib, R.case("greedy"), True)
    a, _ = R.lib_plan(pkg._cabi, lib, R.case("greedy"), False)
    with capsys.disabled():
        print(f"\nCOUPLING_FACT greedy join: grouped pmax {R.case_plan('greedy', True)['pmax']} -> bxt_ok {g['bxt_ok']}; "
              f"alone pmax {R.case_plan('greedy', False)['pmax']} -> bxt_ok {a['bxt_ok']}, ecap {a['ecap']}")
    assert not g["bxt_ok"] and a["bxt_ok"] and a["ecap"] == 768


@pytest.mark.parametrize("cus", [1, 256])
@pytest.mark.parametrize("B", [1, 3, 8, 64])
def test_route_fields(pkg, lib, B, cus):
    for name in R.ALL_CASES:
        pat = R.case(name)
        for sw in (0, R.SW_DENSE_COUPLING, R.SW_NO_SCATTER_FOLD):
            for i in (1, 2):
                g = B >= 8
                _, got = R.lib_plan(pkg._cabi, lib, pat, g, query=(B, cus, i, sw))
                assert got == R.route(pat, R.case_plan(name, g), B, cus, i, sw), (name, B, cus, i, sw, got)


def test_route_fields_of_the_measured_shape(pkg, lib):
    """darcy256 x 64 on 256 CUs, the benchmark's launch: the tile route with 16 chunks per workgroup (4 groups x 3 column groups
    x 64 problems = 768 workgroups, one round), the zero role clearing the rows below rmax."""
    w = pkg.workloads.make("darcy256")
    Q = w.Q.tocsc()
    Q.sort_indices()

    class Pat:
        n, N, bsp, nnz = w.n, w.n_blocks, 1024, Q.nnz
        colptr, rowval = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)
    P, r = R.lib_plan(pkg._cabi, lib, Pat, True, query=(64, 256, 1, 0))
    assert (P["cmin"], P["bxt_ok"], int(P["ng"][1])) == (256, True, 4)
    kind, km, cw, nch, ncg, ng, grid, fill, zwgs, sd = r
    assert (kind, nch, ncg, ng, fill, sd) == (R.TILES, 16, 3, 4, R.FILL_ZERO_ROLE, 0), r
    assert grid == (3 * 4 + zwgs) * 64 and zwgs == R.zero_wgs(1024, P["rmax"])
    _, r1 = R.lib_plan(pkg._cabi, lib, Pat, False, query=(1, 256, 1, 0))
    assert r1[0] == R.TILES and r1[7] == R.FILL_SCATTER_ROLE and r1[3] == 1


# ------------------------------------------------------------------------------------------------ the checks can fail
def _image(pat, P, B, i, outs):
    """A whole C image of sentinels with `outs[p]` in block i's window, the cells left of the staircase unwritten."""
    img = R.sentinel(int(np.prod(R.c_image_shape(pat, P, B)))).reshape(R.c_image_shape(pat, P, B)).copy()
    for p in range(B):
        img[p, i - 1] = outs[p]
        left = np.arange(pat.bsp - P["cmin"])[None, :] < P["kst"][np.arange(P["rmax"]) // 64][:, None]
        img[p, i - 1][left] = R.sentinel(int(left.sum()))
    return img


@pytest.mark.parametrize("name", ["window", "ragged"])
def test_planted_defects_are_caught(name):
    pat, P, i = R.case(name), R.case_plan(name, True), 2
    vals, bv, X, ref, bound = R.case_refs(name, i, 0)
    refs = [(ref, bound)]
    good = R.emulate(pat, P, i, bv, X)
    img = _image(pat, P, 1, i, [good])
    written, worst, cells = R.check_c(pat, P, i, 1, img, refs, "clean")            # the clean emulation passes
    assert worst <= 1.0 and cells > 0
    e = pat.lower[i]

    def fails(outs, what):
        with pytest.raises(AssertionError):
            R.check_c(pat, P, i, 1, outs, refs, what)

    # a row's last entry dropped
    r0 = int(e[len(e) // 2, 0])
    last = np.flatnonzero(e[:, 0] == r0)[-1]
    keep = np.ones(len(e), bool)
    keep[last] = False
    fails(_image(pat, P, 1, i, [R.emulate(pat, P, i, bv[keep], X, e[keep])]), "last entry dropped")
    # a column index off by one
    e2 = e.copy()
    e2[last, 1] -= 1
    fails(_image(pat, P, 1, i, [R.emulate(pat, P, i, bv, X, e2)]), "column off by one")
    # another problem's values
    fails(_image(pat, P, 1, i, [R.emulate(pat, P, i, R.case_refs(name, i, 1)[1], X)]), "another problem's values")
    # a staircase start 16 too far right: the 16 columns from the start of the last staircase tile are left unwritten
    t = P["rmax"] // 64 - 1
    bad = img.copy()
    bad[0, i - 1, 64 * t:64 * t + 64, P["kst"][t]:P["kst"][t] + 16] = R.sentinel(64 * 16).reshape(64, 16)
    fails(bad, "staircase 16 too far right")
    # one 16-column chunk not written
    bad = img.copy()
    W = pat.bsp - P["cmin"]
    bad[0, i - 1, 0:64, W - 16:W] = R.sentinel(64 * 16).reshape(64, 16)
    fails(bad, "a chunk not written")
    # a write into another block's window / another problem
    bad = img.copy()
    bad[0, i - 2, 3, 5] = 0.0
    fails(bad, "stray write")
    # the Schur block: a D_i entry scattered before its zero (the zero lands on it), a zero fill that misses a row
    S = R.sentinel(pat.bsp ** 2).reshape(pat.bsp, pat.bsp).copy()
    for r in range(pat.bsp):
        S[r, :64 * (r // 64 + 1)] = 0.0
    de, dv = pat.diag_lower(i, vals)
    S[de[:, 0], de[:, 1]] = dv
    R.check_s(pat, P, i, 1, S, R.FILL_SCATTER_ROLE, [vals], "clean scatter")
    lost = S.copy()
    lost[de[5, 0], de[5, 1]] = 0.0
    with pytest.raises(AssertionError):
        R.check_s(pat, P, i, 1, lost, R.FILL_SCATTER_ROLE, [vals], "entry under its zero")
    Z = R.sentinel(pat.bsp ** 2).reshape(pat.bsp, pat.bsp).copy()
    Z[P["rmax"]:, :] = 0.0
    R.check_s(pat, P, i, 1, Z, R.FILL_ZERO_ROWS, [vals], "clean zero fill")
    Z[P["rmax"] - 1, 0] = 0.0
    with pytest.raises(AssertionError):
        R.check_s(pat, P, i, 1, Z, R.FILL_ZERO_ROWS, [vals], "zero fill one row too many")


def test_ties_can_fail():
    a = np.array([[1.0, 2.0], [0.0, 4.0]])
    w = np.ones((2, 2), bool)
    R.tie(a, w, a.copy(), w)
    b = a.copy()
    b[1, 0] = -0.0
    R.tie(a, w, b, w)                       # +0 and -0: the same exact zero
    b[0, 1] = np.nextafter(2.0, 3.0)
    with pytest.raises(AssertionError):
        R.tie(a, w, b, w)
