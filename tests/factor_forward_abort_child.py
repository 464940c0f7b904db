"""Child process of test_persistent_panel_abort_recomputes_y (GMRF_PERSIST_SPIN_MS=0 in its environment: the first wait inside a
persistent panel launch that has to wait gives up at once, and the factorisation is repeated launch-per-step).  A batch with a
registered right-hand side: the repeat must recompute y.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import torch

import __graft_entry__ as g

pkg = g.load_package()
lib = pkg._cabi.load()

w = pkg.workloads.make("darcy256")
nb, B = 8, 12
m = nb * w.block_size
Q = sp.csc_matrix(w.Q[:m, :m]); Q.sort_indices()
rhs = np.ascontiguousarray(w.rhs[:m])
vals = np.stack([Q.data * (1.0 + 0.05 * p) for p in range(B)])
b = torch.from_numpy(np.stack([rhs * (1.0 + 0.5 * p) for p in range(B)])).cuda()
F = pkg.TridiagonalCholeskyFactor(batch=B)
F.set_factor_rhs(b)
F.factor(Q, nb, values=vals)
n_ab = C.c_int32(-1)
pkg._cabi.check(lib.gmrf_test_persist_aborts(F._h, C.byref(n_ab)))
st = C.c_int32(-1)
y = np.empty((B, m), dtype=np.float64)
pkg._cabi.check(lib.gmrf_test_factor_fwd(F._h, C.byref(st), pkg._cabi.ptr(y)))
ysw = F.solve_batch(b[:, None, :], mode=1)[:, 0, :].cpu().numpy()
mu_f, _ = F.posterior_batch(b, 64, seed=3, first_id=0)
mu_s = F.solve_batch(b[:, None, :])[:, 0, :]
rel = lambda a, c: float(np.linalg.norm(a - c) / np.linalg.norm(c))
out = {"aborts": int(n_ab.value), "fwd": int(st.value),
       "y_rel": max(rel(y[p], ysw[p]) for p in range(B)),
       "mean_rel": max(rel(mu_f[p].cpu().numpy(), mu_s[p].cpu().numpy()) for p in range(B))}
print(json.dumps(out))
