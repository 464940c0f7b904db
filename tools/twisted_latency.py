"""One-problem latency of the reference and the twisted elimination order (gmrf_bt_set_order), in the same process.

For darcy256, elliptic512 and burgers512x64: factor (gmrf_bt_refactor_values), mean (ldiv), 64 samples and the one-call
posterior (mean + 64 samples), device-resident right-hand sides, median of --reps after --warmup; the twisted order with the
automatic meeting block, its resolved m and each half's persist_route / persist_aborts.  darcy256 is also factored in the
reference order with set_eager(Switch.NO_PERSIST) (bit 13, the launch-per-step in-block form: the ratio behind the automatic meeting block).
Handles are closed before the next one is made (a one-problem handle with persistent sweeps claims the whole chip).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warmup, dev_ms=None):
    for _ in range(warmup):
        fn()
    host, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
        if dev_ms is not None:
            dev.append(dev_ms())
    out = {"ms": statistics.median(host)}
    if dev:
        out["device_ms"] = statistics.median(dev)
    return out


def measure(pkg, w, order, reps, warmup, legs=("factor", "mean", "samples", "posterior"), switches=0):
    import torch
    F = pkg.TridiagonalCholeskyFactor(order=order)
    if switches:
        F.set_eager(switches)
    F.factor(w.Q, w.n_blocks)
    nz = w.Q.tocsc()
    nz.sort_indices()
    vals = torch.from_numpy(nz.data.copy()).cuda()
    b = torch.from_numpy(w.rhs).cuda()
    torch.cuda.synchronize()
    r = {}
    if "factor" in legs:
        r["factor"] = _median_ms(lambda: F.refactor(vals), reps, warmup, lambda: F.stats()["factor_ms"])
    mu = pkg.ldiv(F, b)
    if "mean" in legs:
        r["mean"] = _median_ms(lambda: pkg.ldiv(F, b), reps, warmup)
    if "samples" in legs:
        r["samples64"] = _median_ms(lambda: F.sample(64, mean=mu, seed=7, like=b), reps, warmup)
    if "posterior" in legs:
        r["posterior64"] = _median_ms(lambda: F.posterior(b, 64, seed=7), reps, warmup)
    st = F.stats()
    r["persist_aborts"] = st["persist_aborts"]
    r["meet"] = F.meet
    if order == "twisted":
        for half in (0, 1):
            hs = F.half_stats(half)
            r[f"half{half}"] = {"persist_route": hs["persist_route"], "persist_aborts": hs["persist_aborts"],
                                "persist_cus": hs["persist_cus"], "persist_refused": hs["persist_refused"]}
    else:
        r["persist_route"] = st["persist_route"]
    F.close()
    torch.cuda.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="darcy256,elliptic512,burgers512x64")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    out = {"tool": "twisted_latency", "reps": args.reps, "warmup": args.warmup, "cases": {}}
    for name in args.cases.split(","):
        w = pkg.workloads.make(name)
        c = {"n": w.n, "n_blocks": w.n_blocks, "block_size": w.n // w.n_blocks}
        c["reference"] = measure(pkg, w, "reference", args.reps, args.warmup)
        c["twisted"] = measure(pkg, w, "twisted", args.reps, args.warmup)
        if name == "darcy256":
            c["reference_launch_per_step"] = measure(pkg, w, "reference", args.reps, args.warmup, legs=("factor",), switches=pkg.Switch.NO_PERSIST)
            c["step_over_persist_per_block"] = (c["reference_launch_per_step"]["factor"]["device_ms"] /
                                                c["reference"]["factor"]["device_ms"])
        c["twisted_over_reference_factor"] = c["twisted"]["factor"]["device_ms"] / c["reference"]["factor"]["device_ms"]
        out["cases"][name] = c
        print(json.dumps({name: c}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
