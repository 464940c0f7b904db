"""Child process of test_persistent_sweep_abort_falls_back (GMRF_SWEEP_SPIN_MS=0 in its environment: the first look at an input
panel inside a persistent sweep that finds a sentinel gives up at once and raises the abort words; the factorisation's persistent
launches keep their own bound).  Prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import __graft_entry__ as g

pkg = g.load_package()
out = {}
w = pkg.workloads.make("burgers512x64")
rhs = torch.from_numpy(w.rhs).cuda()
F = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
keys = ("persist_aborts", "persist_cus", "sweep_persist")
out["after_factor"] = {k: F.stats()[k] for k in keys}
mu = pkg.ldiv(F, rhs)                                   # the forward sweep gives up; the solve is repeated with a launch per product
out["after_solve"] = {k: F.stats()[k] for k in keys}
X = F.sample(16, mean=mu, seed=11, like=rhs)            # the handle has left the persistent forms: no second abort
out["after_sample"] = {k: F.stats()[k] for k in keys}
F.refactor(w.Q.data)                                    # ... and its factorisations take the launch-per-step route from now on
out["route_after_refactor"] = int(F.stats()["persist_route"])
mu2 = pkg.ldiv(F, rhs)
G = pkg.TridiagonalCholeskyFactor()
G.set_eager(pkg.Switch.NO_SWEEP_PERSIST)                                      # a launch per product up front
G.factor(w.Q, w.n_blocks)
mu_g = pkg.ldiv(G, rhs)
X_g = G.sample(16, mean=mu_g, seed=11, like=rhs)
out["solve_equal"] = bool(torch.equal(mu, mu_g) and torch.equal(mu2, mu_g))
out["sample_equal"] = bool(torch.equal(X, X_g))
out["aborts_of_the_per_product_form"] = int(G.stats()["persist_aborts"])
# a fresh handle whose FIRST persistent sweep is a sample's (the abort is seen behind the sample's own synchronisation)
del F, G                                                # (the chip is theirs until they let go of it)
import gc; gc.collect()
H = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
Xh = H.sample(16, mean=mu_g, seed=11, like=rhs)
out["sample_first"] = {k: H.stats()[k] for k in keys}
out["sample_first_equal"] = bool(torch.equal(Xh, X_g))
# the sampled variances, a sharded accumulation, the batch entry point on a batch of one, and two aliased calls: each on a fresh
# handle whose FIRST persistent sweep is the call under test; each result bitwise that of the per-product handle
del H
gc.collect()
import scipy.sparse as sp
cabi = pkg._cabi
lib = cabi.load()
Q = pkg.CsrMatrix(w.Q)
q_csr = sp.csr_matrix(w.Q)
q_csr.sort_indices()
q_vals = np.ascontiguousarray(q_csr.data, dtype=np.float64)
mu_h = mu_g.cpu().numpy()


def var_batch(F):
    v = np.empty(w.n)
    cabi.check(lib.gmrf_bt_marginal_var_batch(F._h, cabi.VAR_RBMC, 65, 13, Q._h, cabi.ptr(q_vals), cabi.ptr(v)))
    return v


def var_accumulate(F, on_dev, method):
    acc = torch.ones(w.n, dtype=torch.float64, device="cuda") if on_dev else np.ones(w.n)       # (what was in it stays)
    torch.cuda.synchronize()                            # (the handle's stream is its own: it does not wait for torch's)
    F.var_accumulate(acc, method, 0, 70, seed=13, Q=Q if method == "rbmc" else None)
    F.var_accumulate(acc, method, 70, 60, seed=13, Q=Q if method == "rbmc" else None)
    return acc.cpu().numpy() if on_dev else acc


def sample_mean_is_out(F):
    buf = torch.from_numpy(mu_h.copy()).cuda()
    cabi.check(lib.gmrf_bt_sample(F._h, 17, 0, 1, cabi.ptr(buf), None, cabi.ptr(buf), w.n))
    return buf.cpu().numpy()


def posterior_b_in_samples(F):
    samples = torch.zeros((16, w.n), dtype=torch.float64, device="cuda")
    samples[0] = rhs
    torch.cuda.synchronize()                            # (the handle's stream is its own: it does not wait for torch's)
    mean = torch.empty(w.n, dtype=torch.float64, device="cuda")
    cabi.check(lib.gmrf_bt_posterior(F._h, cabi.ptr(samples[0]), 19, 0, 16, cabi.ptr(mean), cabi.ptr(samples), w.n))
    return torch.cat([mean[None], samples]).cpu().numpy()


cases = {
    "var_mc_65": lambda F: F.marginal_var("mc", k=65, seed=13),
    "var_rbmc_50": lambda F: F.marginal_var("rbmc", k=50, seed=13, Q=Q),
    "var_accumulate_mc_dev": lambda F: var_accumulate(F, True, "mc"),
    "var_accumulate_rbmc_host": lambda F: var_accumulate(F, False, "rbmc"),
    "var_batch_rbmc_65": var_batch,
    "sample_mean_is_out": sample_mean_is_out,
    "posterior_b_in_samples": posterior_b_in_samples,
}
G = pkg.TridiagonalCholeskyFactor()
G.set_eager(pkg.Switch.NO_SWEEP_PERSIST)
G.factor(w.Q, w.n_blocks)
refs = {name: f(G) for name, f in cases.items()}
out["aborts_of_the_per_product_form"] += int(G.stats()["persist_aborts"])
del G
gc.collect()
for name, f in cases.items():
    H = pkg.tridiagonal_cholesky(w.Q, w.n_blocks)
    cus_before = int(H.stats()["persist_cus"])
    r = f(H)
    st = H.stats()
    out[name] = {"persist_cus_before": cus_before, "persist_aborts": int(st["persist_aborts"]), "persist_cus": int(st["persist_cus"]),
                 "launches": int(st["sweep_persist_launches"]), "equal": bool(np.array_equal(r, refs[name]))}
    H.close()
    del H
    gc.collect()
print(json.dumps(out))
