"""Child process of test_forms_read_from_the_environment: the cases of one form that the environment chooses once per process
(GMRF_DIAG128_FAT, GMRF_PANEL_TILES; argv[1] names the entry of ENV_FORMS).  Every output is held to the contract and the bounds
of tests/potrf_ref.py here; prints one JSON line: per case the route the hook reported, info, contract violations, the worst
residual / bound ratios and a digest of L and Linv."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as g
from tests import potrf_ref as R
from tests.test_gpu_potrf_routes import ENV_FORMS, digest

pkg = g.load_package()
lib = pkg._cabi.load()
(cases,) = [cs for name, _, cs in ENV_FORMS if name == sys.argv[1]]
res = []
for case in cases:
    out = R.run_hook(lib, pkg, case)
    L0, X0, L, X, info, route = out
    form, errors, ratios = case.form, [], {}
    for p, prob in enumerate(case.probs):
        errors += [f"problem {p}: {e}" for e in R.structure_errors(form, L0[p], X0[p], L[p], X[p])]
        for k, v in R.check(form, R.matrix(prob), L[p], X[p], rows_seed=case.seed + p).items():
            ratios[k] = max(ratios.get(k, 0.0), v)
    res.append({"route": list(route), "info": info, "errors": errors, "ratios": ratios, "digest": digest(out)})
print(json.dumps({"cases": res}))
