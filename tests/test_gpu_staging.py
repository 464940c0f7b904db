"""Host-or-device arguments of the workload handles, straight through the C ABI.

Every entry point of the posterior assembler and of the Burgers, Darcy and shallow-water element handles takes each of its
arrays from host or device memory.  Host arrays pass through the handle's one staging arena; device arrays are used where they
lie.  The kernels are the same either way, so for every entry point the results of

  (a) all arguments on the host,  (b) all on the device,  (c) inputs on one side and outputs on the other (both ways)

are compared BITWISE, with the optional arguments (base, obs_diff, prescribed) once given and once null.  The cases of one handle
run in order of growing size (larger batch, larger coefficient table), so the arena grows between calls, and every case is also
compared with the same call on a fresh handle.  (api.py returns "the same kind as the input", so it never reaches case (c).)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

NS, NT = 16, 6              # Burgers line: n = 96 unknowns, 80 rows of J
NX, NY = 7, 5               # Darcy / shallow-water mesh
PLACEMENTS = ((False, False), (True, True), (False, True), (True, False))      # (inputs on the device, outputs on the device)


def _run(cabi, call, ins, out_counts, in_dev, out_dev):
    """call(*pointers of the inputs, *pointers of the outputs) with the arrays placed as asked; the outputs as host arrays."""
    import torch

    def place(a, dev):
        if a is None:
            return None
        return torch.from_numpy(a).cuda() if dev else a.copy()

    pin = [place(a, in_dev) for a in ins]
    pout = [place(np.full(c, np.nan), out_dev) for c in out_counts]
    torch.cuda.synchronize()                # the handles' streams do not wait for torch's
    cabi.check(call(*[cabi.ptr(a) for a in pin + pout]))
    res = [o.cpu().numpy() if out_dev else o for o in pout]
    for a, a0 in zip(pin, ins):             # inputs are read only
        if a is not None:
            assert np.array_equal(a.cpu().numpy() if in_dev else a, a0)
    return res


def _assert_bitwise(what, ref, got):
    assert len(ref) == len(got)
    for i, (r, g) in enumerate(zip(ref, got)):
        assert r.shape == g.shape and r.tobytes() == g.tobytes(), (what, "output", i, float(np.nanmax(np.abs(r - g))))


def _check(cabi, name, make, destroy, cases):
    """cases: (label, bind, inputs, output counts), smallest first; bind(handle) is the call."""
    shared = make()
    try:
        for label, bind, ins, outs in cases:
            ref = _run(cabi, bind(shared), ins, outs, False, False)
            for r in ref:
                assert np.all(np.isfinite(r)), (name, label)
            for in_dev, out_dev in PLACEMENTS[1:]:
                _assert_bitwise((name, label, in_dev, out_dev), ref, _run(cabi, bind(shared), ins, outs, in_dev, out_dev))
            _assert_bitwise((name, label, "host again"), ref, _run(cabi, bind(shared), ins, outs, False, False))
            fresh = make()
            try:
                _assert_bitwise((name, label, "fresh handle"), ref, _run(cabi, bind(fresh), ins, outs, False, False))
            finally:
                destroy(fresh)
    finally:
        destroy(shared)


def _burgers(lib, order=1):
    def make():
        h = C.c_void_p()
        create = lib.gmrf_burgers_p2_create if order == 2 else lib.gmrf_burgers_p1_create
        assert create(0, None, NS, NT, 0.05, 0.01, C.byref(h)) == 0
        return h
    return make, lib.gmrf_burgers_p1_destroy


def _burgers_pattern(cabi, lib):
    h = C.c_void_p()
    assert lib.gmrf_burgers_p1_create(-1, None, NS, NT, 0.05, 0.01, C.byref(h)) == 0
    nnz = C.c_int64(0)
    lib.gmrf_burgers_p1_pattern(h, C.byref(nnz), None, None, 0)
    rp, ci = np.zeros((NT - 1) * NS + 1, dtype=np.int64), np.zeros(nnz.value, dtype=np.int64)
    assert lib.gmrf_burgers_p1_pattern(h, None, cabi.ptr(rp), cabi.ptr(ci), 0) == 0
    lib.gmrf_burgers_p1_destroy(h)
    return rp, ci


def _assembler(cabi, lib):
    """Q: a symmetric band pattern on the Burgers unknowns; J: the Burgers tangent's pattern."""
    n, m = NS * NT, (NT - 1) * NS
    jp, ji = _burgers_pattern(cabi, lib)
    Q = sp.diags([np.ones(n - abs(k)) for k in (-NS, -1, 0, 1, NS)], (-NS, -1, 0, 1, NS), format="csc")
    Q.sort_indices()
    qp, qi = Q.indptr.astype(np.int64), Q.indices.astype(np.int64)

    def make():
        h = C.c_void_p()
        assert lib.gmrf_assemble_create(0, None, n, cabi.ptr(qp), cabi.ptr(qi), m, cabi.ptr(jp), cabi.ptr(ji), 0, C.byref(h)) == 0
        return h

    h = make()
    nnz_out = C.c_int64(0)
    assert lib.gmrf_assemble_pattern(h, C.byref(nnz_out), None, None, None, 0) == 0
    lib.gmrf_assemble_destroy(h)
    return make, lib.gmrf_assemble_destroy, dict(n=n, m=m, nnz_q=int(qp[-1]), nnz_j=int(jp[-1]), nnz_out=nnz_out.value)


def test_assemble_precision(pkg, lib):
    cabi, rng = pkg._cabi, np.random.default_rng(1)
    make, destroy, d = _assembler(cabi, lib)
    ins = [rng.standard_normal(d["nnz_q"]), rng.standard_normal(d["nnz_j"])]
    bind = lambda h: lambda q, jv, out: lib.gmrf_assemble_precision(h, q, jv, 0.7, out)      # noqa: E731
    _check(cabi, "precision", make, destroy, [("one problem", bind, ins, [d["nnz_out"]])])


def test_assemble_rhs(pkg, lib):
    cabi, rng = pkg._cabi, np.random.default_rng(2)
    make, destroy, d = _assembler(cabi, lib)
    base, jv, x, od = (rng.standard_normal(d[k]) for k in ("n", "nnz_j", "n", "m"))
    bind = lambda h: lambda base, jv, x, od, out: lib.gmrf_assemble_rhs(h, base, jv, x, od, 0.7, out)      # noqa: E731
    _check(cabi, "rhs", make, destroy, [(f"base {b is not None}, obs_diff {o is not None}", bind, [b, jv, x, o], [d["n"]])
                                        for b in (None, base) for o in (None, od)])


@pytest.mark.parametrize("q_shared", [False, True])
def test_assemble_precision_batch(pkg, lib, q_shared):
    cabi, rng = pkg._cabi, np.random.default_rng(3)
    make, destroy, d = _assembler(cabi, lib)
    cases = []
    for batch in (2, 9):
        ins = [rng.standard_normal(d["nnz_q"] * (1 if q_shared else batch)), rng.standard_normal(batch * d["nnz_j"])]
        bind = lambda h, batch=batch: lambda q, jv, out: lib.gmrf_assemble_precision_batch(      # noqa: E731
            h, batch, q, 0 if q_shared else d["nnz_q"], jv, 0.7, out)
        cases.append((f"batch {batch}", bind, ins, [batch * d["nnz_out"]]))
    _check(cabi, "precision_batch", make, destroy, cases)


def test_assemble_rhs_batch(pkg, lib):
    cabi, rng = pkg._cabi, np.random.default_rng(4)
    make, destroy, d = _assembler(cabi, lib)
    cases = []
    for batch in (2, 9):
        base, jv, x, od = (rng.standard_normal(batch * d[k]) for k in ("n", "nnz_j", "n", "m"))
        bind = lambda h, batch=batch: lambda base, jv, x, od, out: lib.gmrf_assemble_rhs_batch(h, batch, base, jv, x, od, 0.7, out)      # noqa: E731
        cases += [(f"batch {batch}, base {b is not None}, obs_diff {o is not None}", bind, [b, jv, x, o], [batch * d["n"]])
                  for b in (None, base) for o in (None, od)]
    _check(cabi, "rhs_batch", make, destroy, cases)


@pytest.mark.parametrize("q_shared", [False, True])
def test_assemble_objective_batch(pkg, lib, q_shared):
    cabi, rng = pkg._cabi, np.random.default_rng(5)
    make, destroy, d = _assembler(cabi, lib)
    cases = []
    for batch in (2, 9):
        ins = [rng.standard_normal(d["nnz_q"] * (1 if q_shared else batch))] + [rng.standard_normal(batch * d[k]) for k in ("n", "n", "m")]
        bind = lambda h, batch=batch: lambda q, xp, x, od, out: lib.gmrf_assemble_objective_batch(      # noqa: E731
            h, batch, q, 0 if q_shared else d["nnz_q"], xp, x, od, 0.7, out)
        cases.append((f"batch {batch}", bind, ins, [batch]))
    _check(cabi, "objective_batch", make, destroy, cases)


def test_one_assembler_serves_every_call_in_turn(pkg, lib):
    """The calls of one assembler share its arena: a small call after a large one, and the other way round."""
    cabi, rng = pkg._cabi, np.random.default_rng(6)
    make, destroy, d = _assembler(cabi, lib)
    q, jv, x, od = (rng.standard_normal(d[k]) for k in ("nnz_q", "nnz_j", "n", "m"))
    B = 5
    qb, jvb, xb, odb = (rng.standard_normal(B * d[k]) for k in ("nnz_q", "nnz_j", "n", "m"))
    prec = lambda h: lambda q, jv, out: lib.gmrf_assemble_precision(h, q, jv, 0.7, out)      # noqa: E731
    rhs = lambda h: lambda jv, x, od, out: lib.gmrf_assemble_rhs(h, None, jv, x, od, 0.7, out)      # noqa: E731
    precb = lambda h: lambda q, jv, out: lib.gmrf_assemble_precision_batch(h, B, q, d["nnz_q"], jv, 0.7, out)      # noqa: E731
    rhsb = lambda h: lambda jv, x, od, out: lib.gmrf_assemble_rhs_batch(h, B, None, jv, x, od, 0.7, out)      # noqa: E731
    _check(cabi, "assembler in turn", make, destroy, [
        ("rhs", rhs, [jv, x, od], [d["n"]]), ("precision", prec, [q, jv], [d["nnz_out"]]),
        ("rhs batch", rhsb, [jvb, xb, odb], [B * d["n"]]), ("precision batch", precb, [qb, jvb], [B * d["nnz_out"]]),
        ("rhs after the batches", rhs, [jv, x, od], [d["n"]]), ("precision after the batches", prec, [q, jv], [d["nnz_out"]])])


@pytest.mark.parametrize("order", [1, 2])
def test_burgers_tangent_and_batch(pkg, lib, order):
    cabi, rng = pkg._cabi, np.random.default_rng(7)
    make, destroy = _burgers(lib, order)
    n, rows = NS * NT, (NT - 1) * NS
    nnz = rows * (8 if order == 2 else 6)
    cases = [("one problem", lambda h: lambda w, vals, f: lib.gmrf_burgers_p1_tangent(h, w, vals, f), [rng.standard_normal(n)], [nnz, rows])]
    for batch in (3, 11):
        bind = lambda h, batch=batch: lambda w, vals, f: lib.gmrf_burgers_p1_tangent_batch(h, batch, w, vals, f)      # noqa: E731
        cases.append((f"batch {batch}", bind, [rng.standard_normal(batch * n)], [batch * nnz, batch * rows]))
    cases.append(cases[0])          # the one-problem call again, in the grown arena
    _check(cabi, f"burgers tangent order {order}", make, destroy, cases)


@pytest.mark.parametrize("order", [1, 2])
def test_darcy_assemble(pkg, lib, order):
    cabi, rng = pkg._cabi, np.random.default_rng(8)

    def make():
        h = C.c_void_p()
        create = lib.gmrf_darcy_p2_create if order == 2 else lib.gmrf_darcy_p1_create
        assert create(0, None, NX, NY, C.byref(h)) == 0
        return h

    h = make()
    nnz = C.c_int64(0)
    assert lib.gmrf_darcy_p1_pattern(h, C.byref(nnz), None, None, 0) == 0
    lib.gmrf_darcy_p1_destroy(h)
    n = NX * NY if order == 1 else (2 * NX - 1) * (2 * NY - 1)
    cases = []
    for ng in (4, 33, 8):           # the coefficient table grows, then shrinks again
        bind = lambda h, ng=ng: lambda tab, vals, f: lib.gmrf_darcy_p1_assemble(h, tab, ng, 1.5, vals, f)      # noqa: E731
        cases.append((f"ng {ng}", bind, [np.exp(0.3 * rng.standard_normal(ng * ng))], [nnz.value, n]))
    _check(cabi, f"darcy order {order}", make, lib.gmrf_darcy_p1_destroy, cases)


def test_shallow_water_assemble_and_operators(pkg, lib):
    cabi, rng = pkg._cabi, np.random.default_rng(9)

    def make():
        h = C.c_void_p()
        assert lib.gmrf_shallow_water_p1_create(0, None, NX, NY, C.byref(h)) == 0
        return h

    h = make()
    nnz_k, nnz_s = C.c_int64(0), C.c_int64(0)
    assert lib.gmrf_shallow_water_p1_pattern(h, 0, C.byref(nnz_k), None, None, 0) == 0
    assert lib.gmrf_shallow_water_p1_pattern(h, 1, C.byref(nnz_s), None, None, 0) == 0
    nn, n, cells = NX * NY, 3 * NX * NY, 2 * (NX - 1) * (NY - 1)
    Hq = 1.0 + rng.random(cells * 3)
    pres = np.zeros(n, dtype=np.uint8)
    ix, iy = np.arange(nn) % NX, np.arange(nn) // NX
    pres[3 * np.flatnonzero((ix == 0) | (iy == 0) | (ix == NX - 1) | (iy == NY - 1))] = 1        # the first field on the boundary
    asm = lambda h: lambda Hq, pres, K, M, S: lib.gmrf_shallow_water_p1_assemble(h, Hq, 0.1, 0.2, 9.81, pres, K, M, S)      # noqa: E731
    ops = lambda h: lambda K, M, S, pres, G, J, Mt, beta: lib.gmrf_shallow_water_p1_operators(      # noqa: E731
        h, K, M, S, pres, 2.0, 0.5, 0.01, G, J, Mt, beta)
    # operators of what the assemble call gives (host arrays; with and without the constraints)
    mats = {}
    for p in (None, pres):
        K, M, S = _run(cabi, asm(h), [Hq, p], [nnz_k.value, n, nnz_s.value], False, False)
        mats[p is not None] = (K, S, M)
    lib.gmrf_shallow_water_p1_destroy(h)
    cases = []
    for p in (None, pres):
        K, S, M = mats[p is not None]
        cases.append((f"assemble, prescribed {p is not None}", asm, [Hq, p], [nnz_k.value, n, nnz_s.value]))
        cases.append((f"operators, prescribed {p is not None}", ops, [K, M, S, p], [nnz_k.value, nnz_s.value, n, n]))
    _check(cabi, "shallow water", make, lib.gmrf_shallow_water_p1_destroy, cases)
