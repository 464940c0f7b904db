"""Every in-block Cholesky route (potrf_block: csrc/potrf_step.hpp, csrc/potrf_persist.hpp, the routing in csrc/gmrf_hip.hip)
driven directly through gmrf_test_potrf_route at the smallest shapes each form exists at.  Every output is held to the contract
and to the derived componentwise bounds of tests/potrf_ref.py (A - L L^T and Linv L - I, in longdouble); every case asserts the
route, the persistent form and the split the hook reports; the bitwise ties the code claims are asserted as bits.

The forms read once per process from the environment run in child processes (tests/potrf_route_child.py).  Two of the cases
set for them, GMRF_PANEL_TILES = 2 / 8 with set_eager bit 1 at bs 512, run and pass but do not reach a panel width other than 4:
bit 1 at 8 tiles is the 256-column panel route, which has no panel width.  The width is read by the big one-problem route (32
tiles and more) and by the step route at 8 tiles and more, which bit 4 selects outside a capture; the children run that too.

GMRF_POTRF_RATIOS_OUT=<file>: the worst residual / bound per route form and input family of the run, as JSON."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import potrf_ref as R
from tests.potrf_ref import Case

pytestmark = pytest.mark.gpu

BAD_SHAPE = -2
WORST = {}          # "<route>/<persist form>/<inverse>" -> family -> {criterion: worst ratio}


def form_name(form):
    inv = "split%d%s" % (form.xsplit, "_in_slot" if form.in_slot else "") if form.xsplit else ("rows" if form.rows_upto == form.n else "doubling")
    return f"{R.ROUTE_NAMES[form.route]}/persist{form.persist}/{form.inv}/{inv}"


def record(case, worst, name=None):
    d = WORST.setdefault(name or form_name(case.form), {}).setdefault(case.family if case.batch == 1 else "batch", {})
    for k, v in worst.items():
        d[k] = max(d.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _ratios_file():
    yield
    path = os.environ.get("GMRF_POTRF_RATIOS_OUT")
    if path:
        with open(path, "w") as fh:
            json.dump(WORST, fh, indent=1, sort_keys=True)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_verified(lib, pkg, case):
    out = R.run_hook(lib, pkg, case)
    assert out[4] == 0, f"info {out[4]}"
    record(case, R.verify(case, out))
    return out


# Every test takes its cases from a function of its own parameters and registers it: tests/test_potrf_ref_cpu.py holds the
# restatements to the bounds, and shows that mutations break them, on exactly these cases.
CASES = []          # (test name, function(**parameters) -> [Case], test)


def cases_from(fn):
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


# ------------------------------------------------------------------------------------------------ one problem
def fused_cases(bs, family):
    return [Case(bs, bits=b, family=family, seed=bs // 64) for b in (0, R.BIT_NO_PERSIST, R.BIT_NO_LOOKAHEAD, R.BIT_DOUBLING)]


@cases_from(lambda family: [Case(64, family=family)])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_tile_only(lib, pkg, family):
    (case,) = [Case(64, family=family)]
    assert case.form.route == R.ROUTE_FUSED and case.form.persist == 0
    run_verified(lib, pkg, case)


@cases_from(fused_cases)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("bs", [128, 256, 512, 1024])
def test_fused_route_and_its_ties(lib, pkg, bs, family):
    """ROUTE_FUSED: the persistent launch (bits 0), the look-ahead chain of launches (bit 13), every step re-factoring its tile
    (bit 8) and the inverse by doubling (bit 7).  potrf_persist.hpp claims the factor and the inverse of the persistent form
    bitwise those of the launch-per-step form, the parity tests claim the same of bit 8, and of bit 7 for L."""
    base, chain, refactor, doubling = fused_cases(bs, family)
    assert [c.form.route for c in (base, chain, refactor, doubling)] == [R.ROUTE_FUSED] * 4
    assert (base.form.persist, chain.form.persist, refactor.form.persist, doubling.form.persist) == (1, 0, 0, 0)
    o0 = run_verified(lib, pkg, base)
    for c in (chain, refactor):
        o = R.run_hook(lib, pkg, c)
        assert o[4] == 0 and o[5][:3] == (c.form.route, 0, 0) and o[5][3] == 0, (c, o[4], o[5])
        assert same_bits(o[2], o0[2]) and same_bits(o[3], o0[3]), f"{c}: not the bits of the persistent launch"
    od = run_verified(lib, pkg, doubling)
    assert same_bits(od[2], o0[2]), "bit 7 changed L"


def big_cases(family):
    return [Case(2048, bits=b, family=family, seed=32) for b in (0, R.BIT_NO_PERSIST, R.BIT_NO_LOOKAHEAD)]


@cases_from(big_cases)
@pytest.mark.parametrize("family", ["dominant", "graded"])
def test_big_one_problem_route_and_its_ties(lib, pkg, family):
    """ROUTE_BIG_ONE at 32 tiles: a persistent launch per 256-column panel; fused steps inside the panel (bits 13 and 8), which
    potrf_persist.hpp claims bitwise equal."""
    base, steps, refactor = big_cases(family)
    assert [c.form.route for c in (base, steps, refactor)] == [R.ROUTE_BIG_ONE] * 3
    assert (base.form.persist, steps.form.persist, refactor.form.persist) == (2, 0, 0)
    o0 = run_verified(lib, pkg, base)
    for c in (steps, refactor):
        o = R.run_hook(lib, pkg, c)
        assert o[4] == 0 and o[5][:3] == (R.ROUTE_BIG_ONE, 0, 0) and o[5][3] == 0, (c, o[4], o[5])
        assert same_bits(o[2], o0[2]) and same_bits(o[3], o0[3]), f"{c}: not the bits of the persistent panels"


@cases_from(lambda bs, family: [Case(bs, bits=R.BIT_BATCH_ROUTES, family=family, seed=bs // 64 + 3)])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("bs", [64, 128, 256, 512, 1024])
def test_batch_routes_at_batch_one(lib, pkg, bs, family):
    case = Case(bs, bits=R.BIT_BATCH_ROUTES, family=family, seed=bs // 64 + 3)
    assert case.form.route == (R.ROUTE_PANELS256 if bs >= 256 else R.ROUTE_STEPS)
    assert case.form.persist == (3 if bs >= 256 else 0)
    run_verified(lib, pkg, case)


# ------------------------------------------------------------------------------------------------ batches
def batch_case(bs, B, slim):
    return Case(bs, B, R.BIT_NO_PERSIST_PANELS if slim else 0, family=R.FAMILIES[(B + bs // 256) % 4], seed=7 + B)


def check_invariance(lib, pkg, case, out):
    """Problem p of the batch is the same problem run alone on the same route, bit for bit (p = 0 and the last)."""
    for p in sorted({0, case.batch - 1}):
        alone, prob = case.alone(p)
        assert (alone.form.route, alone.form.persist, alone.form.xsplit) == (case.form.route, case.form.persist, case.form.xsplit)
        o = R.run_hook(lib, pkg, alone, mats=[R.matrix(prob)])
        assert o[4] == 0 and o[5][:3] == out[5][:3], (o[4], o[5])
        assert same_bits(o[2][0], out[2][p]) and same_bits(o[3][0], out[3][p]), f"problem {p} differs from its call alone"


@cases_from(lambda bs, B, slim: [batch_case(bs, B, slim)])
@pytest.mark.parametrize("slim", [0, 1])
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("bs", [256, 512])
def test_batches_on_the_panel_route(lib, pkg, bs, B, slim):
    """One persistent launch per 256 x 256 diagonal block (route[1] = 3), or potrf_diag128_slim and three GEMM launches (bit 15)."""
    case = batch_case(bs, B, slim)
    assert (case.form.route, case.form.persist) == (R.ROUTE_PANELS256, 0 if slim else 3)
    out = run_verified(lib, pkg, case)
    check_invariance(lib, pkg, case, out)


@cases_from(lambda B: [Case(256, B, family="graded", seed=40)])
@pytest.mark.parametrize("B", [36, 37])
def test_either_side_of_the_persistent_panel_gate(lib, pkg, B):
    """7 workgroups per problem: 36 problems fit the 256 compute units, 37 do not and take the one-workgroup kernels."""
    case = Case(256, B, family="graded", seed=40)
    assert (case.form.route, case.form.persist, case.form.inv) == (R.ROUTE_PANELS256, 3 if B == 36 else 0, "panel_persist" if B == 36 else "panel_diag128")
    run_verified(lib, pkg, case)


@cases_from(lambda bs: [Case(bs, 3, family="lattice", seed=50)])
@pytest.mark.parametrize("bs", [64, 128])
def test_batches_on_the_step_route(lib, pkg, bs):
    case = Case(bs, 3, family="lattice", seed=50)
    assert (case.form.route, case.form.persist) == (R.ROUTE_STEPS, 0)
    out = run_verified(lib, pkg, case)
    check_invariance(lib, pkg, case, out)


SPLITS = [(512, 256, 256), (1024, 256, 256), (1024, 512, 512)]          # bs, cmin, the split it gives


def split_case(bs, cmin, keep_l, control):
    return Case(bs, 2, R.BIT_NO_XSPLIT if control else 0, cmin, keep_l, family="spectrum" if keep_l else "graded", seed=60 + keep_l)


@cases_from(lambda bs, cmin, p, keep_l, control: [split_case(bs, cmin, keep_l, control)])
@pytest.mark.parametrize("control", [0, 1])
@pytest.mark.parametrize("keep_l", [1, 0])
@pytest.mark.parametrize("bs, cmin, p", SPLITS)
def test_split_inverse(lib, pkg, bs, cmin, p, keep_l, control):
    """A coupling window that starts at cmin >= 256 leaves the first block column of the inverse unassembled: X[b, a] holds
    L[b, a], copied or (p = 256, no kept L) formed there.  Bit 12 keeps the full inverse."""
    case = split_case(bs, cmin, keep_l, control)
    assert case.form.xsplit == (0 if control else p) and case.form.in_slot == (not control and p == 256 and not keep_l)
    out = run_verified(lib, pkg, case)
    assert out[5][2] == (0 if control else p)
    check_invariance(lib, pkg, case, out)


# ------------------------------------------------------------------------------------------------ non-SPD
# (name, case, tiles that get a -1 on their diagonal): each route's smallest multi-tile size; tile 0, a middle one, the last;
# potrf_diag128: the second tile of each 128-block too
def _positions(case, diag128=False):
    nt = case.n // 64
    return sorted({0, nt // 2, nt - 1} | ({1, 3} if diag128 else set()))


NON_SPD = [
    ("fused_persist", Case(128)), ("fused_chain", Case(128, bits=R.BIT_NO_PERSIST)), ("fused_refactor", Case(128, bits=R.BIT_NO_LOOKAHEAD)),
    ("fused_doubling", Case(128, bits=R.BIT_DOUBLING)),
    ("big_persist", Case(2048, seed=32)), ("big_steps", Case(2048, bits=R.BIT_NO_PERSIST, seed=32)),
    ("big_refactor", Case(2048, bits=R.BIT_NO_LOOKAHEAD, seed=32)),
    ("panels_persist_1", Case(256, bits=R.BIT_BATCH_ROUTES)), ("panels_slim_1", Case(256, bits=R.BIT_BATCH_ROUTES | R.BIT_NO_PERSIST_PANELS)),
    ("steps_1", Case(128, bits=R.BIT_BATCH_ROUTES)),
    ("panels_persist_3", Case(256, 3)), ("panels_slim_3", Case(256, 3, R.BIT_NO_PERSIST_PANELS)), ("steps_3", Case(128, 3)),
    ("panels_persist_512", Case(512, 2)),
]
NON_SPD_RUNS = [(nm, c, t) for nm, c in NON_SPD for t in _positions(c, "slim" in nm)]


@cases_from(lambda name, case, tile: [case])
@pytest.mark.parametrize("name, case, tile", NON_SPD_RUNS, ids=[f"{nm}-tile{t}" for nm, _, t in NON_SPD_RUNS])
def test_non_spd_is_reported_with_the_block_id(lib, pkg, name, case, tile):
    """A -1 on the diagonal inside one tile of the LAST problem: info is that problem's block id (1 + p: one block per problem),
    no persistent wait gives up, and every other problem of the batch still meets both bounds.  One run per case."""
    mats = [R.matrix(p) for p in case.probs]
    bad = case.batch - 1
    A = mats[bad].copy()
    i = 64 * tile + 5
    A[i, i] = -1.0
    mats[bad] = A
    out = R.run_hook(lib, pkg, case, mats=mats)
    assert out[4] == 1 + bad, (out[4], out[5])
    assert out[5][3] == 0
    if case.batch > 1:
        R.verify(case, out, mats=mats, skip={bad})


@cases_from(lambda bits: [Case(256, 3, bits, family="graded", seed=70)])
@pytest.mark.parametrize("bits", [0, R.BIT_NO_PERSIST_PANELS])
def test_two_non_spd_problems_report_one_of_them(lib, pkg, bits):
    """atomicCAS lets the first writer win: info is one of the two ids; the problem between them is untouched by either."""
    case = Case(256, 3, bits, family="graded", seed=70)
    mats = [R.matrix(p) for p in case.probs]
    for p, i in ((0, 130), (2, 7)):
        A = mats[p].copy()
        A[i, i] = -1.0
        mats[p] = A
    out = R.run_hook(lib, pkg, case, mats=mats)
    assert out[4] in (1, 3), out[4]
    assert out[5][3] == 0
    R.verify(case, out, mats=mats, skip={0, 2})


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_launch_nothing(lib, pkg):
    S, L, X = R.build_buffers([R.spd("dominant", 128, 1)])
    keep = (S.copy(), L.copy(), X.copy())
    info = C.c_int32(-7)
    route = (C.c_int32 * 4)(-1, -1, -1, -1)
    for bs, batch, cmin in ((128, 0, 0), (128, -1, 0), (128, 1, 32), (128, 1, 128), (128, 1, -64), (192, 1, 0), (96, 1, 0)):
        st = lib.gmrf_test_potrf_route(0, bs, batch, 0, cmin, 1, pkg._cabi.ptr(S), pkg._cabi.ptr(L), pkg._cabi.ptr(X), C.byref(info), route)
        assert st == BAD_SHAPE, (bs, batch, cmin, st)
    assert info.value == -7 and tuple(route) == (-1, -1, -1, -1)
    for a, b in zip((S, L, X), keep):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------ forms chosen by the environment
ENV_FORMS = [
    ("fat", {"GMRF_DIAG128_FAT": "1"}, [Case(256, 2, R.BIT_NO_PERSIST_PANELS, family="graded", seed=80),
                                        Case(512, 2, R.BIT_NO_PERSIST_PANELS, family="spectrum", seed=81)]),
    ("panel2", {"GMRF_PANEL_TILES": "2"}, [Case(512, bits=R.BIT_BATCH_ROUTES, family="graded", seed=82, panel_tiles=2),
                                           Case(512, bits=R.BIT_BATCH_ROUTES | R.BIT_FORK, family="graded", seed=82, panel_tiles=2),
                                           Case(512, 2, R.BIT_FORK, family="lattice", seed=83, panel_tiles=2)]),
    ("panel8", {"GMRF_PANEL_TILES": "8"}, [Case(512, bits=R.BIT_BATCH_ROUTES, family="spectrum", seed=84, panel_tiles=8),
                                           Case(1024, bits=R.BIT_BATCH_ROUTES | R.BIT_FORK, family="spectrum", seed=84, panel_tiles=8),
                                           Case(1024, 2, R.BIT_FORK, family="dominant", seed=85, panel_tiles=8)]),
]


def digest(out):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(out[2]).tobytes() + np.ascontiguousarray(out[3]).tobytes()).hexdigest()


_CHILD_FAILED = []          # names of the forms whose child failed: no later child is started


@cases_from(lambda form: [c for name, _, cs in ENV_FORMS if name == form for c in cs])
@pytest.mark.parametrize("form", [name for name, _, _ in ENV_FORMS])
def test_forms_read_from_the_environment(lib, pkg, form):
    """potrf_diag128 (the three-tile form, GMRF_DIAG128_FAT=1) and the panel widths 2 and 8 (GMRF_PANEL_TILES) are chosen once per
    process: one fresh child per form, one after the other under a time limit, and none is started once one has failed.  The
    child holds its outputs to the bounds and prints the worst ratios; potrf_step.hpp claims potrf_diag128 bitwise equal to
    potrf_diag128_slim, which this process runs."""
    assert not _CHILD_FAILED, f"not started: the child of {_CHILD_FAILED[0]} failed"
    (env, cases), = [(e, cs) for name, e, cs in ENV_FORMS if name == form]
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "potrf_route_child.py")
    r = subprocess.run([sys.executable, child, form], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        _CHILD_FAILED.append(form)
    assert r.returncode == 0, (form, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"potrf child {form}: {res}")
    assert len(res["cases"]) == len(cases)
    for case, got in zip(cases, res["cases"]):
        f = case.form
        assert tuple(got["route"]) == (f.route, f.persist, f.xsplit, 0), (form, case, got)
        assert got["info"] == 0 and not got["errors"], (form, case, got)
        assert got["ratios"] and all(v <= 1.0 for v in got["ratios"].values()), (form, case, got)
        record(case, got["ratios"], name=f"env_{form}/" + form_name(f))
        if form == "fat":
            assert got["digest"] == digest(R.run_hook(lib, pkg, case)), "potrf_diag128 is not potrf_diag128_slim bit for bit"
