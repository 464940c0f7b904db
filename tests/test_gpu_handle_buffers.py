"""The device buffers of the solver handle (csrc/host_util.hpp: DevArr, reserve_group, the borrowed state): a handle whose
grow-on-demand buffers have all grown, shrunk and been re-created computes the bits of a fresh handle; the forward solve inside
a batch's factorisation survives a change of batch; caller-owned storage outlives the handle untouched; and handles that come
and go leave no device memory behind."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def _arrays(x):
    """Whatever a call returned, as a list of NumPy arrays."""
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _arrays(y)]
    if sp.issparse(x):
        return [np.asarray(x.data)]
    if hasattr(x, "cpu"):
        return [x.cpu().numpy()]
    return [np.asarray(x)]


class _State:
    """What a step needs of the handle before its call: the matrix, the batch and whether L is kept."""

    def __init__(self, w, batch=1, keep_l=True):
        self.w, self.batch, self.keep_l = w, batch, keep_l

    def values(self):
        return np.stack([self.w.Q.data * (1.0 + 0.25 * p) for p in range(self.batch)]) if self.batch > 1 else None

    def key(self):
        return (id(self.w), self.batch, self.keep_l)

    def enter(self, F, current):
        """Brings F from state `current` (None: a fresh handle) to this one."""
        if current is not None and current.key() == self.key():
            return
        if (current.keep_l if current else True) != self.keep_l:
            F.set_keep_l(self.keep_l)
        if (current.batch if current else 1) != self.batch:
            F.set_batch(self.batch)
        F.factor(self.w.Q, self.w.n_blocks, values=self.values())


def _steps(pkg):
    """(name, state, call) in the order the long-lived handle runs them.  Shapes 4 x 64 (bsp 64), 3 x 130 (bsp 256) and 2 x 512
    (one problem with blocks of 512: its sweeps are persistent launches, so the posterior reaches the samples' own panels and
    the sweeps' intermediate panel); batch 1 -> 2 -> 1; right-hand-side counts 1, 3, 64, 200, 2 (a batch: 128 for 200)."""
    import torch
    wa = pkg.workloads.random_block_tridiagonal(4, 64, seed=1)
    wb = pkg.workloads.random_block_tridiagonal(3, 130, seed=6)
    wc = pkg.workloads.random_block_tridiagonal(2, 512, seed=3, density=0.02)
    rng = np.random.default_rng(7)
    A1, B1, C1 = _State(wa), _State(wb), _State(wc)
    A2, A1n = _State(wa, batch=2), _State(wa, keep_l=False)
    csr = {}

    def pattern(w, diag_only):
        key = (id(w), diag_only)
        if key not in csr:
            S = sp.csr_matrix(sp.diags(w.Q.diagonal())) if diag_only else sp.csr_matrix(w.Q)
            csr[key] = pkg.CsrMatrix(S)
        return csr[key]

    steps = []

    def add(name, state, call):
        steps.append((name, state, call))

    def one_problem(tag, st, ks):
        w = st.w
        for k in ks:
            Bk = rng.standard_normal((w.n, k)) if k > 1 else w.rhs.copy()
            add(f"{tag} ldiv k={k}", st, lambda F, Bk=Bk: pkg.ldiv(F, Bk))
        add(f"{tag} sample 3", st, lambda F: F.sample(3, seed=11))
        add(f"{tag} sample 70 + mean", st, lambda F, w=w: F.sample(70, mean=w.rhs, seed=12, first_id=5))
        for k in (2, 40):                                  # (the samples' panels grow between the two)
            add(f"{tag} posterior k={k}", st,
                lambda F, w=w, k=k: F.posterior(torch.from_numpy(w.rhs).cuda(), k, seed=13, first_id=2))
        add(f"{tag} var exact", st, lambda F: F.marginal_var("exact"))
        add(f"{tag} var rbmc", st, lambda F, w=w: F.marginal_var("rbmc", k=20, seed=14, Q=pattern(w, False)))
        for diag_only in (True, False, True):              # two patterns of different nnz: smaller, larger, smaller
            S = pattern(w, diag_only)
            dv = rng.standard_normal((3, S.nnz))
            add(f"{tag} selinv diag={diag_only}", st, lambda F, S=S: F.selected_inverse(S))
            add(f"{tag} trace_inv diag={diag_only}", st, lambda F, S=S, dv=dv: F.trace_inv(S, dv))

    one_problem("4x64", A1, (1, 3, 64, 200, 2))
    one_problem("3x130", B1, (1, 3, 64, 200, 2))
    one_problem("4x64 again", A1, (2, 200))
    one_problem("2x512", C1, (1, 3, 2))
    rb = np.stack([wa.rhs, 2.0 * wa.rhs])
    for k in (1, 3, 64, 128, 2):                           # (a batch takes at most 128 right-hand sides per call)
        Bk = np.ascontiguousarray(np.broadcast_to(rb[:, None, :], (2, k, wa.n))) * np.arange(1, k + 1)[None, :, None]
        add(f"batch 2 solve k={k}", A2, lambda F, Bk=Bk: F.solve_batch(Bk))
    add("batch 2 sample", A2, lambda F: F.sample_batch(5, seed=15))
    add("batch 2 var exact", A2, lambda F: F.marginal_var("exact"))
    add("batch 2 posterior", A2, lambda F: F.posterior_batch(torch.from_numpy(rb).cuda(), 4, seed=16))
    add("batch 1 again: ldiv", A1, lambda F: pkg.ldiv(F, wa.rhs))
    add("batch 1 again: sample", A1, lambda F: F.sample(3, seed=11))
    add("no L: ldiv", A1n, lambda F: pkg.ldiv(F, wa.rhs))
    add("no L: sample", A1n, lambda F: F.sample(9, seed=17))
    add("no L: var exact", A1n, lambda F: F.marginal_var("exact"))
    add("L again: ldiv", A1, lambda F: pkg.ldiv(F, wa.rhs))
    add("L again: blocks", A1, lambda F: [F.get_block(0, 1), F.get_block(1, 0), F.get_block(2, 3)])
    add("3x130 again: ldiv", B1, lambda F: pkg.ldiv(F, wb.rhs))
    return steps, csr


def test_a_used_handle_computes_the_bits_of_a_fresh_one(pkg):
    steps, csr = _steps(pkg)
    refs = []
    for name, state, call in steps:                        # one fresh handle per step, closed before the next is created:
        F = pkg.TridiagonalCholeskyFactor()                # the persistent-launch budget is every handle's alone
        try:
            state.enter(F, None)
            refs.append(_arrays(call(F)))
        finally:
            F.close()
    F = pkg.TridiagonalCholeskyFactor()
    current = None
    try:
        for (name, state, call), ref in zip(steps, refs):
            state.enter(F, current)
            current = state
            got = _arrays(call(F))
            assert len(got) == len(ref), name
            for g, r in zip(got, ref):
                assert g.shape == r.shape and np.array_equal(g, r), name
    finally:
        F.close()


def _fwd_state(pkg, F):
    st = C.c_int32(-1)
    pkg._cabi.check(pkg._cabi.load().gmrf_test_factor_fwd(F._h, C.byref(st), None))
    return int(st.value)


FWD_BLOCKS, FWD_BATCH = 2, 12      # darcy256's leading blocks: the factorisation leaves y = L^-1 b (asserted below)


def test_forward_solve_in_the_factor_survives_a_change_of_batch(pkg):
    import torch
    w = pkg.workloads.make("darcy256")
    nb, B = FWD_BLOCKS, FWD_BATCH
    m = nb * w.block_size
    Q = sp.csc_matrix(w.Q[:m, :m])
    Q.sort_indices()
    vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
    b = torch.from_numpy(np.stack([w.rhs[:m] * (1.0 + 0.5 * p) for p in range(B)])).cuda()

    def fresh():
        F = pkg.TridiagonalCholeskyFactor(batch=B)
        F.set_factor_rhs(b)
        F.factor(Q, nb, values=vals)
        return F

    G = fresh()
    try:
        assert _fwd_state(pkg, G) == 1
        mu_ref, X_ref = [t.cpu().numpy() for t in G.posterior_batch(b, 8, seed=21, first_id=3)]
    finally:
        G.close()
    F = fresh()
    try:
        assert _fwd_state(pkg, F) == 1
        for small in (B // 2, 1):
            F.set_factor_rhs(None)
            F.set_batch(small)
            F.factor(Q, nb, values=vals[:small] if small > 1 else None)
            F.set_batch(B)
            F.set_factor_rhs(b)
            F.factor(Q, nb, values=vals)
            assert _fwd_state(pkg, F) == 1
            mu, X = [t.cpu().numpy() for t in F.posterior_batch(b, 8, seed=21, first_id=3)]
            assert np.array_equal(mu, mu_ref) and np.array_equal(X, X_ref)
    finally:
        F.close()


def test_caller_owned_storage_outlives_the_handle(pkg, lib):
    import torch
    w = pkg.workloads.make("darcy32")
    bl, bc, bi = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    pkg._cabi.check(lib.gmrf_bt_storage_bytes(w.n, w.n_blocks, 1, C.byref(bl), C.byref(bc), C.byref(bi)))

    def tensors():
        return [torch.full((nb.value // 8,), 777.0, dtype=torch.float64, device="cuda") for nb in (bl, bc, bi)]

    def run(F, bufs, keep_l):
        """set_storage, factor, solve; what the handle shows of its factor."""
        ptrs = [pkg._cabi.ptr(t) for t in bufs]
        pkg._cabi.check(lib.gmrf_bt_set_storage(F._h, w.n, w.n_blocks, 1, ptrs[0] if keep_l else None, ptrs[1], ptrs[2]))
        F.factor(w.Q, w.n_blocks)
        x = pkg.ldiv(F, w.rhs)
        for kind in (0, 1, 2) if keep_l else (1, 2):
            p, nbytes = F.factor_buffer(kind)
            assert p == bufs[kind].data_ptr() and nbytes == bufs[kind].numel() * 8
        blocks = [F.get_block(kind, 1) for kind in ((0, 1, 2) if keep_l else (1, 2))]
        return x, blocks

    first, second = tensors(), tensors()
    F = pkg.TridiagonalCholeskyFactor()
    x1, blocks1 = run(F, first, True)
    images1 = [t.clone() for t in first]
    pkg._cabi.check(lib.gmrf_bt_set_storage(F._h, w.n, w.n_blocks, 1, *[pkg._cabi.ptr(t) for t in second]))   # the first set is let go of
    F.factor(w.Q, w.n_blocks)
    assert np.array_equal(pkg.ldiv(F, w.rhs), x1)
    images2 = [t.clone() for t in second]
    F.close()
    torch.cuda.synchronize()
    for t, image in zip(first + second, images1 + images2):            # still the caller's, still readable, untouched by the close
        assert bool((t == image).all())
    for a, c in zip(images1, images2):
        assert bool((a == c).all())
    # keep_l off on a fresh handle (the API's order: set_keep_l before set_storage): L's tensor is not used, the work block is the handle's
    third = tensors()
    G = pkg.TridiagonalCholeskyFactor()
    G.set_keep_l(False)
    x3, blocks3 = run(G, third, False)
    assert np.array_equal(x3, x1)
    images3 = [t.clone() for t in third]
    G.close()
    torch.cuda.synchronize()
    for t, image in zip(third, images3):
        assert bool((t == image).all())
    assert bool((third[0] == 777.0).all())
    for kind in (1, 2):
        assert bool((images3[kind] == images1[kind]).all())
        assert np.array_equal(blocks3[kind - 1], blocks1[kind])
    # a second handle given the same tensors factors to the same bits
    H = pkg.TridiagonalCholeskyFactor()
    try:
        x4, blocks4 = run(H, first, True)
        assert np.array_equal(x4, x1) and all(np.array_equal(a, c) for a, c in zip(blocks4, blocks1))
        for t, image in zip(first, images1):
            assert bool((t == image).all())
    finally:
        H.close()


def test_handles_that_come_and_go_leave_no_device_memory(pkg):
    import torch
    w = pkg.workloads.random_block_tridiagonal(4, 64, seed=1)
    used = []
    for it in range(20):
        for order in ("reference", "twisted"):
            F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks, order=order)
            pkg.ldiv(F, w.rhs); F.sample(3, seed=1); F.marginal_var("exact")
            F.close()
        free_b, total_b = torch.cuda.mem_get_info(0)
        used.append(total_b - free_b)
    assert max(used[2:]) - min(used[2:]) < 64 << 20


@pytest.mark.parametrize("batch,bs,route,switch", [(1, 128, 1, "NO_PERSIST"), (2, 256, 3, "NO_PERSIST_PANELS")])
def test_a_changed_switch_reaches_a_handle_with_captured_graphs(pkg, batch, bs, route, switch):
    """Graphs on: a handle that has captured its factor graph on the persistent route (stats persist_route: 1 the fused block
    launch of one problem at block size 128, 3 a batch's launch per panel diagonal block at 256 -- the smallest shapes that take
    them) drops it when the switch comes, takes the launch-per-step form (0), and takes the persistent one again when the switch
    goes.  Each factor solves to the first one's solution within the bound of solves across routes (test_gpu_parity.solve_tol)."""
    from tests.test_gpu_parity import rel, solve_tol
    w = pkg.workloads.random_block_tridiagonal(3, bs, seed=5)
    vals = np.stack([w.Q.data * (1.0 + 0.25 * p) for p in range(batch)]) if batch > 1 else w.Q.data
    rhs = np.stack([w.rhs * (p + 1.0) for p in range(batch)])
    F = pkg.TridiagonalCholeskyFactor(batch=batch)         # (the only handle alive: the CU budget is its alone)
    try:
        def solve():
            return F.solve_batch(rhs[:, None, :])[:, 0, :] if batch > 1 else pkg.ldiv(F, rhs[0])[None, :]

        F.factor(w.Q, w.n_blocks, values=vals if batch > 1 else None)
        assert F.stats()["persist_route"] == route
        x0 = solve()
        for switches, want in ((getattr(pkg.Switch, switch), 0), (0, route)):
            F.set_eager(switches)
            F.refactor(vals)
            assert F.stats()["persist_route"] == want, (switches, F.stats()["persist_route"])
            x = solve()
            for p in range(batch):
                assert rel(x[p], x0[p]) < solve_tol(w), (switches, p)
    finally:
        F.close()
