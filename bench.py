#!/usr/bin/env python3
"""bench.py -- GMRF posterior solves/sec (mean + samples) on the 256x256 Darcy posterior.

N = 1 (the BASELINE metric config C3).  One step = one pass of the hot path over one batch of
synthetic input: T x B independent 256^2 Darcy posteriors (same mesh and sparsity pattern, different
coefficient fields -- the per-problem loop of scripts/darcy/solve_darcy_gmrf-fem.jl:176-198), each
one: numeric factorisation of Q_post (values already in HBM; the pattern is analysed once before
the timed region, like the reference re-uses its permutation, :166-174), the posterior mean (forward
+ backward sweep) and 64 posterior samples (backward sweep of 64 right-hand sides).  B problems
advance in lock step on one handle (problem = one more grid dimension of every kernel); T handles
run on T HIP streams driven by T host threads (the latency-bound launches of one chain leave CUs to
the others).  value = T * B * (1 + 64) * steps / time.

N > 1 (launched by torch.distributed.run, one rank per GPU).  Headline = the north-star split:
ONE factor shared by all ranks -- rank 0 factors a batch of posteriors block-range by block-range,
every finished range of Linv / C blocks is broadcast over RCCL (the library's own communicator,
gmrf_comm_*; torch.distributed if that cannot be set up) while the next range is being factored --
and the samples sharded: every rank takes the means and draws ITS OWN 64 samples per posterior.
value = B_shared * (1 + 64 N) * steps / time (B_shared = 32 posteriors per step: the root factors them as one
batch, 2.6 ms per posterior, and 0.83 GB per posterior cross xGMI).  With --full, beside it in the same run: the
independent-problems mode of the N = 1 line (no data-path collective) and BASELINE config C4 (elliptic 512^2, 256 samples
sharded over the ranks).

A plain run does what the headline needs and nothing more: set-up, --warmup steps, --steps timed steps, the outputs of
the last one if --dump-outputs is given, the result line.  --full adds everything else the benchmark measures and checks,
after the timed steps: at N = 1 one instrumented step (per-kernel times, roofline figures, GEMM launches by shape), the
phase times, the batch-1 latency, the reference's whole per-problem loop, the K6 SpMM roofline, the CPU baselines and the
oracle parity of the timed route (--no-single-problem, --no-full-loop, --no-spmm and --no-cpu-baseline leave legs out);
at N > 1 the side legs (--no-side-legs).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR     # + what the last timed step returned, as .npy
    python bench.py --gpus 1 --steps 20 --warmup 3 --full                 # + every other leg
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_MFMA_TFLOPS = 78.6     # MI355X datasheet fp64 matrix peak; 77.7 measured (tools/mb2.hip)
PEAK_HBM_GBPS = 8000.0           # MI355X_MICROARCH.md: 8 TB/s spec (6.3-6.5 TB/s achievable)

KERNEL_CLASSES = {      # one class per kernel symbol (include/gmrf_hip.h, gmrf_stats)
    0: ("gemm_f64_mfma<false,false>", "mfma"),   # 64 x 64 tile GEMM, B stored [n][k]
    11: ("gemm_f64_mfma<false,true>", "mfma"),   # 64 x 64 tile GEMM, B stored [k][n]
    13: ("gemm_f64_ll", "mfma"),                 # 32 x 32 tile GEMM of launches with <= 128 tiles of 64 x 64
    14: ("gemm_f64_dma<B[n][k]>", "mfma"),       # LDS-DMA staged GEMM (gemm_f64_dma.hpp), B stored [n][k]
    15: ("gemm_f64_dma<B[k][n]>", "mfma"),       # LDS-DMA staged GEMM, B stored [k][n]
    12: ("gemm_f64_mfma<true,*>", "mfma"),       # A stored [k][m] (selected inversion only)
    16: ("potrf_diag128", "mfma"),               # 128 x 128 diagonal block of a batch (two tile Choleskys + its inverse)
    18: ("gemm_f64_dma<A[k][m]>", "mfma"),       # LDS-DMA staged GEMM, A stored [k][m] (selected inversion, round 4)
    17: ("potrf_persist", "mfma"),               # persistent in-block Cholesky (one problem: a block / a 256-column panel per launch; small batches: a panel's diagonal block)
    6: ("gemm_f64_big<false>", "mfma"),     # 128 x 128 tile GEMM, B stored [n][k]
    7: ("gemm_f64_big<true>", "mfma"),      # 128 x 128 tile GEMM, B stored [k][n]
    1: ("potrf_step<false>", "mfma"),       # tile Cholesky + inverse (latency-bound, B workgroups)
    8: ("potrf_panel", "mfma"),
    9: ("potrf_update", "mfma"),
    2: ("sweep_mm", "mfma"),
    3: ("sweep_gemv", "hbm"),
    19: ("sweep_persist<k=1>", "hbm"),      # one problem: a whole k = 1 sweep as ONE persistent launch (round 5)
    20: ("sweep_persist<k>=16>", "mfma"),   # ... a whole sweep of 16 .. 128 right-hand sides
    10: ("spmm_bxt", "hbm"),
    4: ("csr_spmm", "hbm"),
}


def git_head():
    """Commit of the tree: from git, or (on a GPU box, whose snapshot has no .git) from .build_head, which
    __graft_entry__.build() / the profile scripts write beside the built library."""
    try:
        h = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True, timeout=5).stdout.strip()
        if h:
            return h
    except Exception:
        pass
    try:
        return open(os.path.join(ROOT, ".build_head")).read().strip() or None
    except OSError:
        return None


def pmc_traffic(file_stem: str, symbol_prefixes, batch=None):
    """HBM bytes per launch of kernel symbols from the committed rocprofv3 --pmc snapshot profiles/<round>_<file_stem>.json
    (newest round present; FETCH_SIZE x2 + WRITE_SIZE, tools/pmc_summary.py).  A snapshot, not a live counter read: the
    source string names the commit it was taken at.  Returns ({symbol: bytes}, source) or (None, None)."""
    for rnd in ("r05", "r04", "r03", "r02"):
        path = os.path.join(ROOT, "profiles", f"{rnd}_{file_stem}.json")
        try:
            prof = json.load(open(path))
        except Exception:
            continue
        if batch is not None and prof.get("batch", batch) != batch:
            continue
        got = {}
        for pre in symbol_prefixes:
            key = next((k for k in prof["kernels"] if k.replace(" ", "").startswith(pre.replace(" ", ""))), None)
            if key:
                got[key] = prof["kernels"][key]["read_bytes_per_launch"] + prof["kernels"][key]["write_bytes_per_launch"]
        if got:
            return got, (f"snapshot: profiles/{rnd}_{file_stem}.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes, taken at "
                         f"commit {prof.get('head', '?')}; this run is {git_head()})")
    return None, None


def pmc_traffic_weighted(file_stem: str, prefix: str, batch=None):
    """Launch-weighted HBM bytes per launch over every kernel symbol that starts with `prefix` in the newest committed
    snapshot (see pmc_traffic).  Returns (bytes, source) or (None, None)."""
    for rnd in ("r05", "r04", "r03", "r02"):
        try:
            prof = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_{file_stem}.json")))
        except Exception:
            continue
        if batch is not None and prof.get("batch", batch) != batch:
            continue
        rows = [v for k, v in prof["kernels"].items() if k.startswith(prefix)]
        n = sum(r["launches"] for r in rows)
        if n:
            tot = sum(r["launches"] * (r["read_bytes_per_launch"] + r["write_bytes_per_launch"]) for r in rows)
            return tot / n, (f"snapshot: profiles/{rnd}_{file_stem}.json ({len(rows)} symbols {prefix}*, launch-weighted; rocprofv3 --pmc FETCH_SIZE x2 + "
                             f"WRITE_SIZE, separate passes, taken at commit {prof.get('head', '?')}; this run is {git_head()})")
    return None, None


def cpu_sparse_direct(w, k_samples: int):
    """Secondary CPU comparator: a general sparse direct solver on the same posterior
    precision -- what the reference's scripts really call (CHOLMOD there; SuperLU via SciPy here,
    CHOLMOD bindings are not installed).  1 factorisation + (1 + k) solves, single thread, single shot."""
    import numpy as np
    import scipy.sparse.linalg as spla
    Z = np.random.default_rng(0).standard_normal((w.n, k_samples))
    t0 = time.perf_counter()
    lu = spla.splu(w.Q.tocsc(), permc_spec="MMD_AT_PLUS_A", options={"SymmetricMode": True})
    t1 = time.perf_counter()
    lu.solve(w.rhs)
    lu.solve(Z)
    t2 = time.perf_counter()
    return {"value": (1 + k_samples) / (t2 - t0), "unit": "solves/s", "cores": 1,
            "kind": "scipy.sparse.linalg.splu (SuperLU, MMD_AT_PLUS_A, symmetric mode), single shot",
            "sample": f"1 factorisation {t1 - t0:.2f} s + {1 + k_samples} solves {t2 - t1:.2f} s"}


def cpu_baseline(w, k_samples: int, sample_blocks: int = 8):
    """The oracle (LAPACK-backed NumPy/SciPy restatement of the reference algorithm) timed on this box's
    host cores on a BOUNDED sample of the workload: the leading `sample_blocks` blocks of the chain
    (same block size, same arithmetic per block: factor + mean + k samples), scaled to the full chain by
    n_blocks / sample_blocks.  Protocol of SURVEY 8d: thread-count sweep (1 warm-up + 2 timed runs each),
    then 1 warm-up + median of 5 at the best count."""
    import numpy as np
    from oracle import bt_oracle as O
    from threadpoolctl import threadpool_info, threadpool_limits
    nb = min(sample_blocks, w.n_blocks)
    ns = nb * w.block_size
    Qs = w.Q.tocsr()[:ns, :ns].tocsc()
    rhs = w.rhs[:ns]
    Z = np.random.default_rng(0).standard_normal((ns, k_samples))

    def job():
        t0 = time.perf_counter()
        F = O.tridiagonal_cholesky(Qs, nb)
        t1 = time.perf_counter()
        mu = O.ldiv(F, rhs)
        X = O.sample(F, mu, Z)
        return time.perf_counter() - t0, t1 - t0, (mu, X)

    # the sweep stays within the cores this process may run on and within the BLAS thread pools as they were sized at load time
    # (OMP_NUM_THREADS / OPENBLAS_NUM_THREADS, else every core): OpenBLAS crashes when it is asked for more threads than that
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    ncpu = min([ncpu] + [p["num_threads"] for p in threadpool_info() if p.get("user_api") == "blas"])
    counts = sorted({c for c in (4, 8, 16, 32, 64, 128, ncpu) if c <= ncpu})
    sweep = {}
    for c in counts:
        with threadpool_limits(limits=c):
            job()
            sweep[c] = min(job()[0] for _ in range(2))
    best = min(sweep, key=sweep.get)
    with threadpool_limits(limits=best):
        job()
        runs = [job() for _ in range(5)]
    runs.sort(key=lambda r: r[0])
    t_med, t_fac, res = runs[2]
    scale = w.n_blocks / nb
    extrapolated = (1 + k_samples) / (t_med * scale)
    # Round 4: the WHOLE chain once at the best thread count -- 1 warm-up + median of 3 of factor + mean +
    # k samples on the full matrix -- is the reported value; the bounded sample above picks the thread count and stays as a
    # cross-check.  Bounded: skipped (value = the extrapolation, and the line says so) if one full run would exceed ~15 s.
    full = None
    if t_med * scale <= 15.0 and nb < w.n_blocks:
        Qf = w.Q.tocsc()
        Zf = np.random.default_rng(0).standard_normal((w.n, k_samples))

        def job_full():
            t0 = time.perf_counter()
            F = O.tridiagonal_cholesky(Qf, w.n_blocks)
            t1 = time.perf_counter()
            mu = O.ldiv(F, w.rhs)
            O.sample(F, mu, Zf)
            return time.perf_counter() - t0, t1 - t0

        with threadpool_limits(limits=best):
            job_full()
            fr = sorted(job_full() for _ in range(3))
        full = fr[1]
    value = (1 + k_samples) / full[0] if full else extrapolated
    if full:
        sample = (f"the whole chain of {w.name} (n={w.n}, {w.n_blocks} blocks of {w.block_size}): factor + mean + {k_samples} samples, "
                  f"median of 3 after a warm-up = {full[0]:.3f} s (factor {full[1]:.3f} s); ")
    elif nb == w.n_blocks:
        sample = "the sample below IS the whole chain; "
    else:
        sample = "the whole chain was NOT timed (one run would exceed 15 s): the value is the extrapolation below; "
    timed_whole = bool(full) or nb == w.n_blocks
    sample += (f"cross-check on the leading {nb} blocks (n={ns}), median of 5 after a warm-up = {t_med:.3f} s (factor {t_fac:.3f} s), "
               f"x{scale:g} = {extrapolated:.1f} solves/s; SciPy/OpenBLAS with {best} threads (sweep on the leading blocks, best of 2: "
               + ", ".join(f"{c}: {v:.3f} s" for c, v in sweep.items()) + ")")
    return {"value": value, "unit": "solves/s", "cores": int(best), "kind": "port", "sample": sample,
            "extrapolated_from_leading_blocks": extrapolated, "timed_whole_chain": timed_whole}, (Qs, nb, rhs, Z, res)


def full_loop(pkg, torch, n_xy: int, batch: int, local: int, with_cpu: bool, sample_blocks: int = 8):
    """The reference's WHOLE per-problem loop (scripts/darcy/solve_darcy_gmrf-fem.jl:176-198) for a batch of data-set
    problems, everything after the coefficient table on the device, under its four timers:
      "PDE Discretization"  coefficient table -> gmrf_darcy_p1_assemble (A, y)                      (:179-187)
      "Conditioning"        gmrf_assemble_precision (Q + Q_eps A'A) + information vector, re-factorisation on the
                            analysed pattern, posterior mean                                         (:188-190)
      "Sampling"            one posterior sample                                                     (:191)
      "Std dev"             RBMCStrategy(50) as the reference configures it (:174), and block-tridiagonal selected
                            inversion beside it                                                      (:192)
    Device times (events on the stream) of one pass over the batch, median of 3, per problem = / batch."""
    import numpy as np
    W = pkg.workloads
    q_eps = 1e8
    Q0, _, N = W.darcy_conditioning(n_xy)
    n = n_xy * n_xy
    gq = np.linspace(0.0, 1.0, 241)
    GX, GY = np.meshgrid(gq, gq, indexing="ij")
    tabs = [W.darcy_coefficient(523802340 + p)(GX.ravel(), GY.ravel()).reshape(241, 241) for p in range(min(8, batch))]
    dev = torch.device("cuda", local)
    st = torch.cuda.current_stream(dev)
    tables = torch.from_numpy(np.stack([tabs[p % len(tabs)] for p in range(batch)])).to(dev)
    d = pkg.DarcyP1Assembler(n_xy, n_xy, device=local, stream=st.cuda_stream)
    asm = pkg.PosteriorAssembler(Q0, d.pattern, device=local, stream=st.cuda_stream)
    qd = torch.from_numpy(Q0.data).to(dev)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    nz = torch.empty((batch, asm.nnz_out), dtype=torch.float64, device=dev)
    rhs = torch.empty((batch, 1, n), dtype=torch.float64, device=dev)
    F = pkg.TridiagonalCholeskyFactor(device=local, stream=st.cuda_stream, batch=batch)
    F.set_keep_l(False)
    Qc = None
    v_rb_d = torch.empty((batch, n), dtype=torch.float64, device=dev)
    v_ex_d = torch.empty((batch, n), dtype=torch.float64, device=dev)

    def one_pass(first):
        nonlocal Qc
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record(st)
        av, yv = [], []
        for p in range(batch):                               # "PDE Discretization"
            a, y = d.assemble(tables[p])
            av.append(a); yv.append(y)
        ev[1].record(st)
        for p in range(batch):                               # "Conditioning"
            nz[p] = asm.precision(qd, av[p], q_eps)
            rhs[p, 0] = asm.rhs(None, av[p], zero, yv[p], q_eps)
        if first:
            P = asm.pattern.copy()
            P.data = nz[0].cpu().numpy()
            F.factor(P, N, values=nz.cpu().numpy())           # symbolic analysis once (the reference's permutation, :166-174)
            Qc = pkg.CsrMatrix(P, device=local, stream=st.cuda_stream)
        else:
            F.refactor(nz)
        mu = F.solve_batch(rhs)[:, 0, :]
        ev[2].record(st)
        F.sample_batch(1, mean=mu, seed=7, like=rhs)          # "Sampling"
        ev[3].record(st)
        F.marginal_var("rbmc", k=50, seed=9, Q=Qc, q_values=nz, out=v_rb_d)     # "Std dev", the reference's estimator
        ev[4].record(st)
        F.marginal_var("exact", out=v_ex_d)                   # the deterministic alternative
        ev[5].record(st)
        ev[5].synchronize()
        # (the variances stay on the device like everything else of the loop: a fresh pageable host array per call cost
        #  0.4 ms per problem of page faults and copy inside the "Std dev" timers; copied out after the clock stops)
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(5)], mu, v_rb_d.cpu().numpy(), v_ex_d.cpu().numpy()

    one_pass(True)
    runs = [one_pass(False) for _ in range(3)]
    ms = np.median(np.array([r[0] for r in runs]), axis=0)
    _, mu, v_rb, v_ex = runs[-1]
    names = ["pde_discretization", "conditioning_incl_mean", "sampling_1", "std_rbmc50", "std_selected_inversion"]
    out = {"workload": f"darcy{n_xy}: batch of {batch} data-set problems (8 coefficient fields), prior + pattern fixed",
           "ms_per_batch": {k: float(v) for k, v in zip(names, ms)},
           "ms_per_problem": {k: float(v) / batch for k, v in zip(names, ms)},
           "problems_per_s_reference_loop": batch / (1e-3 * float(ms[0] + ms[1] + ms[2] + ms[3])),
           "std_rbmc_vs_selected_inversion_median_rel": float(np.median(np.abs(np.sqrt(v_rb[0]) - np.sqrt(v_ex[0])) / np.sqrt(v_ex[0])))}
    # the K6 product inside the RBMC estimator: Q x on 50 node-major right-hand sides, posterior pattern of this workload
    X = torch.randn(n, 50, dtype=torch.float64, device=dev)
    Y = torch.empty_like(X)
    for _ in range(20):
        Qc.matmul_into(X, Y)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(50):
        Qc.matmul_into(X, Y)
    e1.record(st); e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    b = asm.nnz_out * 12 + 8 * (n + 1) + 16 * n * 50
    out["rbmc_k6"] = {"kernel": "csr_spmm_tiles_pad (k = 50 node-major)", "us": us, "algorithmic_bytes": b, "achieved": b / us / 1e3,
                      "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": b / us / 1e3 / PEAK_HBM_GBPS,
                      "note": "11 MB of matrix + 52 MB of operands per call: L2 / Infinity-Cache resident at this size, "
                              "roofline_spmm has the HBM-sized case"}
    F.close()
    if with_cpu:
        # the oracle's same loop on the host: discretisation and assembly at full size (one problem), factor / mean /
        # sample / RBMC(50) on the leading blocks scaled by n_blocks / sample_blocks (as cpu_baseline does)
        from oracle import bt_oracle as O
        t0 = time.perf_counter()
        A_o, y_o = O.assemble_darcy_diff_matrix(n_xy, n_xy, gq, gq, tabs[0], 1.0)
        t1 = time.perf_counter()
        Qp = (Q0 + q_eps * (A_o.T @ A_o)).tocsc()
        b_o = q_eps * (A_o.T @ y_o)
        t2 = time.perf_counter()
        nb = min(sample_blocks, N)
        ns = nb * (n // N)
        Qs = Qp.tocsr()[:ns, :ns].tocsc()
        scale = N / nb
        t3 = time.perf_counter()
        Fo = O.tridiagonal_cholesky(Qs, nb)
        mu_o = O.ldiv(Fo, b_o[:ns])
        t4 = time.perf_counter()
        rng = np.random.default_rng(0)
        O.sample(Fo, mu_o, rng.standard_normal((ns, 1)))
        t5 = time.perf_counter()
        Xs = O.backward_solve(Fo, rng.standard_normal((ns, 50)))
        O.marginal_variances_rbmc(Qs, Xs)
        t6 = time.perf_counter()
        out["cpu_oracle_ms_per_problem"] = {
            "pde_discretization": 1e3 * (t1 - t0), "conditioning_incl_mean": 1e3 * ((t2 - t1) + (t4 - t3) * scale),
            "sampling_1": 1e3 * (t5 - t4) * scale, "std_rbmc50": 1e3 * (t6 - t5) * scale,
            "note": f"oracle (NumPy / SciPy, {os.cpu_count()} host cores available): discretisation and assembly at full size, "
                    f"factor + mean / sample / RBMC(50) on the leading {nb} of {N} blocks scaled x{scale:g}; single shot"}
    return out



def fit_batch(torch, w, local, batch, n_streams, samples, keep_l):
    """Largest batch <= `batch` (a multiple of 8) whose T x B posteriors fit the free HBM: per posterior the block inverses,
    the coupling blocks (dense bound), five work blocks, three right-hand-side panels, the sample output (darcy256: 1.03 GB per posterior estimated, 1.01 measured).
    The default (4 x 64 darcy256 = 260 GB) is sized for the 288 GB of an MI355X; a card with less free memory gets a
    smaller batch instead of an out-of-memory error, and the line says so."""
    free_b, _ = torch.cuda.mem_get_info(local)
    bsp = 64
    while bsp < w.block_size:
        bsp *= 2
    N = w.n_blocks
    per = 8.0 * bsp * bsp * (N * (2 if keep_l else 1) + 0.6 * max(N - 1, 0) + 5) + 8.0 * N * bsp * (3 * max(samples, 16) + samples + 4)
    b = batch
    fits = lambda x: n_streams * x * per * 1.01 <= free_b
    while b > 1 and not fits(b):
        b = (b - 1) // 8 * 8 if b > 8 else b - 1   # the next lower multiple of 8 first (XCD grouping: 12 -> 8, 64 -> 56), then one by one
    return b                                     # (b == 1 may still not fit: the handles' allocation then reports it)


class ProblemsJob:
    """T handles x batch B of independent posteriors on T streams / host threads (no collective)."""

    def __init__(self, pkg, post, w, torch, local, config, batch, n_streams, samples, rank, keep_l, eager_flags=0):
        import numpy as np
        self.torch, self.samples, self.batch, self.n_streams = torch, samples, batch, n_streams
        total = batch * n_streams
        vals, rhss = [w.Q.data], [w.rhs]
        n_distinct = 1 if os.environ.get("GMRF_BENCH_SAME_VALUES") == "1" else 8      # (diagnostic: one coefficient field for all)
        for p in range(1, min(total, n_distinct)):   # coefficient fields on the same mesh: same pattern, different values
            same = False
            if config.startswith("darcy"):
                wp = pkg.workloads.darcy(int(config[5:]), seed=523802340 + 1000 * rank + p)
                same = wp.Q.nnz == w.Q.nnz and np.array_equal(wp.Q.indices, w.Q.indices)
            if same:
                vals.append(wp.Q.data); rhss.append(wp.rhs)
            else:
                vals.append(w.Q.data * (1.0 + 0.01 * p)); rhss.append(w.rhs)
        self.jobs = []
        # one stream per handle, each on a hardware queue of its own (two streams that share a queue serialise: 27.3 k
        # instead of 32.2 k solves/s with 4 handles -- gmrf_streams_create probes which streams overlap)
        self.stream_set = pkg.StreamSet(n_streams, device=local) if n_streams > 1 else None
        self.streams_on_own_queue = self.stream_set.n_distinct if self.stream_set else 1
        for t in range(n_streams):
            st_t = (torch.cuda.current_stream() if n_streams == 1
                    else torch.cuda.ExternalStream(self.stream_set.pointers[t], device=torch.device("cuda", local)))
            idx = [(t * batch + p) % len(vals) for p in range(batch)]
            with torch.cuda.stream(st_t):
                e_t = post.HipEngine(pkg, w, device_index=local, batch=batch, values=np.stack([vals[i] for i in idx]),
                                     rhs=np.stack([rhss[i] for i in idx]), keep_l=keep_l)
                if eager_flags:
                    e_t.F.set_eager(eager_flags)
                j_t = post.ShardedPosterior(e_t, k_samples=samples, replicate_factor=True)
                j_t.prepare()
                j_t.step(1 << 20)     # set-up, untimed: captures the sweep / sample graphs too, whatever --warmup is
            self.jobs.append((st_t, e_t, j_t))
        self.eng, self.job = self.jobs[0][1], self.jobs[0][2]
        # keep_last: run() keeps what the LAST step of each handle returned, (means, samples), in self.last[t] (--dump-outputs);
        # the other steps' outputs are dropped as they come, as without it
        self.keep_last = False
        self.last = [None] * n_streams

    def solves_per_step(self):
        return self.n_streams * self.batch * (1 + self.samples)

    def run(self, first, count):
        torch = self.torch

        def worker(t, st_t, j_t):
            with torch.cuda.stream(st_t):
                for s in range(count):
                    if self.keep_last and s == count - 1:
                        self.last[t] = j_t.step(first + s)
                    else:
                        j_t.step(first + s)
                st_t.synchronize()
        if len(self.jobs) == 1:
            worker(0, self.jobs[0][0], self.jobs[0][2])
            return
        ths = [threading.Thread(target=worker, args=(t, st_t, j_t)) for t, (st_t, _, j_t) in enumerate(self.jobs)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()

    def persist_state(self):
        """What gmrf_stats says about the persistent launches (potrf_persist) of the handles: a wait that gives up inside one is
        repeated launch-per-step and would otherwise only look like a slow box."""
        st = [e.F.stats() for _, e, _ in self.jobs]
        return {"persist_aborts": int(sum(x["persist_aborts"] for x in st)),
                "persist_route_per_handle": [int(x["persist_route"]) for x in st],
                "persist_cus_per_handle": [int(x["persist_cus"]) for x in st],
                "persist_refused": int(sum(x["persist_refused"] for x in st))}

    def close(self):
        self.last = [None] * len(self.jobs)
        for _, e, _ in self.jobs:
            e.F.close()
        self.jobs = []
        if self.stream_set is not None:
            self.torch.cuda.synchronize()
            self.stream_set.close()
            self.stream_set = None
        self.torch.cuda.empty_cache()


def timed(run, sync, dist, torch, first, steps):
    sync()
    t0 = time.perf_counter()
    run(first, steps)
    sync()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    return elapsed


DUMP_BYTES = {"mean": 16_000_000, "samples": 48_000_000}      # --dump-outputs: float64 bytes per array, 64 MB in all


def dump_outputs(path, arrays):
    """--dump-outputs: write what the timed path returned in its last step as path/<name>.npy, float64.  `arrays` maps a name
    to the per-handle device tensors whose concatenation along dimension 0 is the array (handle t's problems follow handle
    t - 1's).  An array that fits its share of DUMP_BYTES is written whole, in its shape; a larger one as a fixed sample of its
    entries in row-major order: the flat range is cut into m equal strata and stratum i gives the entry at a uniform offset
    drawn by numpy.random.default_rng(<array's position in DUMP_BYTES>) -- the same entries for the same shape in every run.
    Returns what the result line says about the files."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    rec = {}
    for pos, (name, parts) in enumerate(arrays.items()):
        shape = [sum(int(p.shape[0]) for p in parts)] + [int(d) for d in parts[0].shape[1:]]
        total = int(np.prod(shape))
        m = DUMP_BYTES[name] // 8
        if total <= m:
            vals = torch.cat([p.reshape(p.shape[0], -1) for p in parts]).cpu().numpy().reshape(shape)
            rec[name] = {"shape": shape, "written": "whole"}
        else:
            i = np.arange(m, dtype=np.int64)
            lo, hi = i * total // m, (i + 1) * total // m
            idx = lo + (np.random.default_rng(pos).random(m) * (hi - lo)).astype(np.int64)
            vals, off = np.empty(m, dtype=np.float64), 0
            for p in parts:                      # each handle's tensor gives the entries of its flat range
                sel = (idx >= off) & (idx < off + p.numel())
                if sel.any():
                    vals[sel] = torch.take(p.contiguous(), torch.from_numpy(idx[sel] - off).to(p.device)).cpu().numpy()
                off += p.numel()
            rec[name] = {"shape": shape, "written": f"sample of {m} entries (row-major order, one per stratum of {total // m}+ entries, "
                                                    f"offsets from numpy.random.default_rng({pos}).random)"}
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(vals, dtype=np.float64))
    return rec


def spmm_roofline(pkg, torch):
    """K6 on the 31 M-entry precision matrix of BASELINE config C5 (burgers 4096 x 512): k = 1 (LDS-staged row
    tiles) and k = 64 node-major (LDS-tiled SpMM), fp64 and fp32 values; device-resident operands, HIP events on
    the stream the kernels run on.  bytes = nnz (vbytes + 4) + 8 (n + 1) + 16 n k."""
    w = pkg.workloads.make("burgers4096x512")
    out = {"matrix": f"{w.name}: n={w.n}, nnz={w.Q.nnz}", "bound": "hbm", "peak": PEAK_HBM_GBPS, "unit": "GB/s", "cases": {}}
    st = torch.cuda.Stream()          # an explicit stream: the null stream's handle is 0 = "make your own" for gmrf_csr_create,
    torch.cuda.set_stream(st)         # and the async products below must run on the stream the events are recorded on
    for f32 in (False, True):
        S = pkg.CsrMatrix(w.Q, values_f32=f32, stream=st.cuda_stream)
        for k in (1, 64):
            X = torch.randn(w.n, dtype=torch.float64, device="cuda") if k == 1 else torch.randn(w.n, k, dtype=torch.float64, device="cuda")
            # warm up to steady clocks: the matrix was just built on the host (GPU idle for seconds), and the first
            # ~30 ms of launches after an idle period run 15-20 % slower (tools/spmm_clock_probe.py)
            Y = torch.empty_like(X)
            # (uninterrupted queues of launches: a warm-up that synchronises every few launches leaves the first timed
            #  batch 8 % slow -- tools/spmm_mem_probe.py: 627 us, then 577 us for the following batches)
            for _ in range(2):
                for _ in range(60):
                    S.matmul_into(X, Y)
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 30
            e0.record(st)
            for _ in range(reps):
                S.matmul_into(X, Y)          # stream-ordered (gmrf_spmm*_async): launches back to back, no host sync in between
            e1.record(st)
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            b = w.Q.nnz * ((4 if f32 else 8) + 4) + 8 * (w.n + 1) + 16 * w.n * k
            rec = {"us": us, "achieved": b / us / 1e3, "frac": b / us / 1e3 / PEAK_HBM_GBPS, "algorithmic_bytes": b}
            if not f32:
                got, src = pmc_traffic("spmm_hbm_traffic", ["csr_spmv_tiles<double" if k == 1 else "csr_spmm_tiles_pad<double"])
                if got:
                    rec["traffic"], rec["traffic_source"] = next(iter(got.values())), src
            out["cases"][f"{'fp32' if f32 else 'fp64'}_k{k}"] = rec
        del S
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="darcy256")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64, help="independent problems per handle and step (4 x 64 darcy256 posteriors = 260 GB of the 288 GB)")
    ap.add_argument("--streams", type=int, default=4,
                    help="independent batched handles per GPU, each on its own HIP stream and host thread")
    ap.add_argument("--mode", choices=["auto", "problems", "shared-factor"], default="auto",
                    help="headline workload.  auto = problems: independent posteriors per rank at every N (the shared-factor job "
                         "then runs as side legs at N > 1 with --full); shared-factor: rank 0 factors, broadcast, samples sharded")
    ap.add_argument("--shared-batch", type=int, default=32, help="posteriors per step whose factor is shared (N > 1)")
    ap.add_argument("--group", type=int, default=8, help="blocks per broadcast range (shared-factor)")
    ap.add_argument("--share", choices=["broadcast", "allgather"], default="allgather",
                    help="shared-factor job: rank 0 factors the batch and broadcasts it, or every rank factors batch / N posteriors and "
                         "the block ranges are all-gathered (round 4; both run as side legs at N > 1)")
    ap.add_argument("--keep-l", action="store_true", help="retain the L blocks (F.chos); default: only Linv and C are stored")
    ap.add_argument("--transport", choices=["auto", "cabi", "torch"], default="auto")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, every other leg of the benchmark (N = 1: instrumented step, roofline, phase times, "
                         "batch-1 latency, whole-loop, K6 SpMM, CPU baselines, oracle parity; N > 1: the side legs).  Off: the "
                         "headline alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines and the oracle parity leg")
    ap.add_argument("--no-single-problem", action="store_true",
                    help="--full: skip the batch-1 latency probe (profile runs: keeps one launch shape per kernel)")
    ap.add_argument("--no-spmm", action="store_true", help="--full: skip the K6 roofline leg (burgers4096x512 matrix)")
    ap.add_argument("--no-full-loop", action="store_true", help="--full: skip the leg that times the reference's whole per-problem loop")
    ap.add_argument("--no-side-legs", action="store_true", help="--full, N > 1: skip the side legs")
    ap.add_argument("--side-leg-limit", type=float, default=360.0, help="N > 1: seconds after which the side legs are abandoned")
    ap.add_argument("--eager-flags", type=int, default=0, help="gmrf_bt_set_eager bits for every handle (experiments)")
    ap.add_argument("--force-shared", action="store_true",
                    help="rehearsal: run the shared-factor code (process group, communicator, broadcasts) with a world of one rank")
    ap.add_argument("--regimes", default="256,1024",
                    help="N > 1: further samples-per-rank-and-posterior regimes of the shared-factor job (side leg)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (means, samples of the independent-problems "
                         "headline; rank 0) as DIR/mean.npy and DIR/samples.npy, float64, 64 MB at most (dump_outputs())")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if args.dump_outputs and (args.mode == "shared-factor" or args.force_shared):
        ap.error("--dump-outputs writes the outputs of the independent-problems headline (not of --mode shared-factor / --force-shared)")

    # `python bench.py --gpus N` without a launcher: start the N ranks here (a torch.distributed.run child, spawned
    # before this process makes any GPU call) and relay their output and exit code.
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)
    if int(world_env or "1") != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world_env or 1}: start one rank per GPU "
              f"(python -m torch.distributed.run --nproc-per-node {args.gpus} ... bench.py --gpus {args.gpus}), or "
              f"run `python bench.py --gpus {args.gpus}` without a launcher", file=sys.stderr)
        sys.exit(2)

    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    from importlib import import_module
    post = import_module(g.PKG_NAME + ".posterior")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # Rehearsal of the N > 1 control flow on a one-GPU box: GMRF_BENCH_BACKEND=gloo with
    # GMRF_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 (gloo moves CUDA tensors through the host).
    backend = os.environ.get("GMRF_BENCH_BACKEND", "nccl")
    one_device = os.environ.get("GMRF_BENCH_ONE_DEVICE") == "1" and backend == "gloo"
    if one_device:
        local = 0
    if world > 1 or args.force_shared:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    torch.cuda.set_device(local)
    # Headline at every N: independent posteriors per rank (the BASELINE single-GPU config on every GPU, no data-path
    # collective: ONE weak-scaling series).  The shared-factor job of north_star (rank 0 factors, the factor crosses xGMI,
    # samples sharded) runs in the same invocation as side legs at N > 1 with --full; --mode shared-factor makes it the headline.
    mode = args.mode if args.mode != "auto" else ("shared-factor" if args.force_shared else "problems")
    shared = mode == "shared-factor" and (world > 1 or args.force_shared)
    shared_legs = (world > 1 or args.force_shared) and args.full and not args.no_side_legs       # the shared-factor job runs somewhere
    keep_l = bool(args.keep_l)

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    w = pkg.workloads.make(args.config)
    out = None
    extra = {}

    # ------------------------------------------------------------------ transport of a shared factor
    comm, transport = None, "torch"
    if shared or shared_legs:
        want = args.transport
        if want in ("auto", "cabi") and not one_device:
            # Every rank takes part in every collective of the negotiation whatever fails where: rank 0 always
            # broadcasts the box (None when librccl could not be opened), every rank then says whether it can open
            # the library (all-reduce MIN), and only if all can does any rank enter ncclCommInitRank.
            box = [None]
            if rank == 0:
                try:
                    box = [pkg.api.Comm.unique_id()]
                except Exception as e:      # noqa: BLE001
                    extra["cabi_comm_error"] = repr(e)[:300]
            dist.broadcast_object_list(box, src=0)
            can = 0
            if box[0] is not None:
                try:
                    pkg.api.Comm.unique_id()          # opens librccl in this process (the id itself is discarded)
                    can = 1
                except Exception as e:      # noqa: BLE001
                    extra["cabi_comm_error"] = repr(e)[:300]
            ok = torch.tensor([can], device="cuda")
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok.item()) == 1:
                comm = pkg.api.Comm(local, rank, world, box[0])   # a failure here is fatal on this rank (raises): the
                transport = "cabi"                                # others sit in ncclCommInitRank until the launcher ends the job

    def shared_job(wl, batch, k_per_rank, values=None, rhs=None, share="broadcast"):
        if share == "allgather":
            # every rank factors batch / world posteriors, block ranges are all-gathered (posterior.HipGatherEngine)
            va = values if values is not None else np.tile(np.ascontiguousarray(wl.Q.data), (batch, 1))
            ra = rhs if rhs is not None else np.tile(np.ascontiguousarray(wl.rhs), (batch, 1))
            eng = post.HipGatherEngine(pkg, wl, device_index=local, batch_total=batch, world=world, rank=rank, values_all=va, rhs_all=ra,
                                       keep_l=False, transport=transport, comm=comm)
        else:
            eng = post.HipEngine(pkg, wl, device_index=local, batch=batch, values=values, rhs=rhs, keep_l=keep_l,
                                 transport=transport, comm=comm)
        job = post.ShardedPosterior(eng, dist=dist, rank=rank, world=world, k_samples=k_per_rank, group=args.group,
                                    force_shared=args.force_shared, keep_samples=False, timing=True, share=share)
        job.prepare()
        job.step(1 << 20)             # set-up, untimed (every rank): graph captures, first broadcasts
        return eng, job

    def gather_phases(j):
        """Per-rank device phase times of the last step: the root's, and the slowest receiver's."""
        torch.cuda.synchronize()
        ph = j.phase_ms()
        box = [None] * world
        dist.all_gather_object(box, ph)
        if rank != 0:
            return None
        recv = [b for b in box[1:] if b]
        res = {"root": {k: round(v, 3) for k, v in box[0].items()}}
        if recv:
            res["receivers_max"] = {k: round(max(b[k] for b in recv), 3) for k in recv[0]}
        return res

    def run_shared(steps, warmup, share="broadcast"):
        """The shared-factor job (north_star's split): per step B posteriors are factored -- all by rank 0 and broadcast
        (share = "broadcast"), or B / N by every rank and all-gathered (share = "allgather", round 4) --, ranges of blocks
        cross xGMI as packed images beside the factorisation, every rank takes the means and draws its own samples.  Returns
        the engine (the regimes reuse it), seconds for `steps` steps (max over ranks), solves per step and what the line says."""
        B = max(1, args.shared_batch)
        if share == "allgather" and B % world:
            B = (B // world + 1) * world
        vals = np.stack([w.Q.data * (1.0 + 0.01 * p) for p in range(B)])
        rhs = np.stack([w.rhs] * B)
        eng_s, job_s = shared_job(w, B, args.samples, vals, rhs, share)

        def run(first, count):
            for s in range(count):
                job_s.step(first + s)
        run(0, warmup)
        eng_s.transport_bytes(reset=True)
        el = timed(run, sync, dist, torch, warmup, steps)
        moved = eng_s.transport_bytes(reset=True) / max(steps, 1)
        phases = gather_phases(job_s)
        # (no scaling curve has been measured on real multi-GPU hardware before the driver's SCALE run; these fields say
        # which regime a record is in)
        # what a ring algorithm puts on every busy link per step: the whole image for a broadcast (each link out of the root
        # and onwards carries all of it), (N - 1) / N of all images for an all-gather (= what came INTO this rank, `moved`)
        rec = {"bytes_broadcast_per_step": moved, "bytes_broadcast_per_posterior": moved / B,
               "form": share, "bytes_per_link_per_step": moved, "posteriors_factored_per_rank": (B // world if share == "allgather" else B),
               "transport": transport, "phase_ms_last_step": phases,
               "reading": "root-bound when root.factor_ms dominates ms_per_step; broadcast-bound when transfer_wait_ms does; "
                          "the samples-per-factor regimes of side_legs.regimes show where sharing the factor pays"}
        how = (f"{B // world} by every rank, Linv / C ranges of {args.group} blocks all-gathered" if share == "allgather" else
               f"all by rank 0, Linv / C ranges of {args.group} blocks broadcast")
        wl = (f"{w.name}: n={w.n}, {w.n_blocks} blocks x {w.block_size}, nnz={w.Q.nnz}; per step {B} posterior(s) factored, {how} "
              f"(packed lower-triangular tiles) over {world} ranks beside the factorisation, every rank: {B} mean(s) + {args.samples} "
              f"samples per posterior")
        sh = (f"one shared factor per posterior, RCCL {'all-gather' if share == 'allgather' else 'broadcast'} "
              f"({'library communicator gmrf_comm_*' if transport == 'cabi' else 'torch.distributed ' + backend}), samples sharded by Philox sample id")
        return eng_s, el, job_s.solves_per_step(), rec, wl, sh

    pj = None
    if shared:
        eng, elapsed, per_step, rec_s, workload, sharding = run_shared(args.steps, args.warmup, args.share)
        extra["shared_factor"] = rec_s
    else:
        fit = fit_batch(torch, w, local, args.batch, max(1, args.streams), args.samples, keep_l)
        if dist is not None:            # every rank runs the same batch
            box = [None] * world
            dist.all_gather_object(box, fit)
            fit = min(box)
        if fit != args.batch:
            extra["batch_reduced"] = {"from": args.batch, "to": fit, "why": "free HBM on the card"}
            args.batch = fit
        pj = ProblemsJob(pkg, post, w, torch, local, args.config, args.batch, max(1, args.streams), args.samples, rank, keep_l,
                         args.eager_flags)
        eng, job = pj.eng, pj.job
        pj.run(0, args.warmup)
        pj.keep_last = bool(args.dump_outputs)
        elapsed = timed(pj.run, sync, dist, torch, args.warmup, args.steps)
        pj.keep_last = False
        if args.dump_outputs and rank == 0:
            extra["dump_outputs"] = dict(dir=args.dump_outputs, step=args.warmup + args.steps - 1, arrays=dump_outputs(
                args.dump_outputs, {"mean": [r[0] for r in pj.last], "samples": [r[1] for r in pj.last]}))
        pj.last = [None] * len(pj.jobs)
        per_step = world * pj.solves_per_step()
        workload = (f"{w.name}: n={w.n}, {w.n_blocks} blocks x {w.block_size}, nnz={w.Q.nnz}; {pj.n_streams * pj.batch} independent "
                    f"posterior(s) per GPU and step ({pj.n_streams} stream(s) x batch {pj.batch}), each factor + mean + {args.samples} samples")
        sharding = ("independent problems per rank, no data-path collective (weak scaling; north_star's split -- ONE factor shared, samples "
                    "sharded by Philox id over RCCL -- is measured at n_gpus > 1 in side_legs.shared_factor_allgather / side_legs.shared_factor "
                    "(root broadcast) / side_legs.c4_elliptic512 of this line)")
        extra["streams_on_own_hardware_queue"] = pj.streams_on_own_queue

    if rank == 0:
        out = {
            "metric": "GMRF posterior solves/sec (mean+samples), 256^2 Darcy",
            "value": per_step * args.steps / elapsed, "unit": "solves/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload, "mode": mode, "samples_per_problem_per_rank": args.samples, "sharding": sharding,
                       "l_blocks_kept": keep_l},
        }
        free_b, total_b = torch.cuda.mem_get_info(local)
        out["hbm_used_gb"] = round((total_b - free_b) / 1e9, 1)
        out.update(extra)

    # ------------------------------------------------------------------ N > 1: the other legs, same run
    leg_state = {}
    watchdog = None
    if shared_legs:
        # The side legs never cost the headline: if they overrun (a rank stuck in a collective), every rank leaves
        # after --side-leg-limit seconds and rank 0 prints the line it already has.
        import threading

        leg = leg_state
        leg["name"] = "set-up"

        def give_up():
            # a rank that is still in a side leg after the limit is stuck (a collective that never completes = a GPU
            # hang): rank 0 prints the headline line it already has, every rank leaves with a NON-ZERO code so that
            # the launcher and the driver see the failure.  Nothing is restarted from here.
            if rank == 0:
                out["side_legs"] = dict(side, error=f"side legs exceeded {args.side_leg_limit} s and were abandoned "
                                                    f"in leg '{leg['name']}'; exit code 3")
                print(json.dumps(out), flush=True)
            sys.stderr.write(f"bench.py rank {rank}: side-leg watchdog fired in leg '{leg['name']}'\n")
            sys.stderr.flush()
            os._exit(3)
        side = {}
        watchdog = threading.Timer(args.side_leg_limit, give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            if not shared:
                # (s) north_star's split beside the headline: the shared-factor job at the headline's samples per posterior
                leg["name"] = "shared_factor"
                pj.close()                    # the headline's posteriors (streams x batch of them) leave the HBM first
                pj = None
                steps_s = max(2, args.steps // 4)
                # (s') the all-gather form first (every rank factors its share): its engine leaves the HBM again before the
                # broadcast form, whose engine the regimes below reuse
                leg["name"] = "shared_factor_allgather"
                eng_g, el_g, per_g, rec_g, wl_g, sh_g = run_shared(steps_s, 1, "allgather")
                if rank == 0:
                    side["shared_factor_allgather"] = dict({"value": per_g * steps_s / el_g, "unit": "solves/s", "ms_per_step": 1e3 * el_g / steps_s,
                                                            "steps": steps_s, "workload": wl_g, "sharding": sh_g}, **rec_g)
                eng_g.F.close(); eng_g.F_all.close()
                del eng_g
                sync()
                leg["name"] = "shared_factor"
                eng, el_s, per_s, rec_s, wl_s, sh_s = run_shared(steps_s, 1, "broadcast")
                if rank == 0:
                    side["shared_factor"] = dict({"value": per_s * steps_s / el_s, "unit": "solves/s", "ms_per_step": 1e3 * el_s / steps_s,
                                                  "steps": steps_s, "workload": wl_s, "sharding": sh_s}, **rec_s)
            elif args.share == "allgather":
                # the headline was the all-gather form: the regimes below run on the broadcast form's engine
                leg["name"] = "shared_factor"
                eng.F.close(); eng.F_all.close()
                sync()
                steps_s = max(2, args.steps // 4)
                eng, el_s, per_s, rec_s, wl_s, sh_s = run_shared(steps_s, 1, "broadcast")
                if rank == 0:
                    side["shared_factor"] = dict({"value": per_s * steps_s / el_s, "unit": "solves/s", "ms_per_step": 1e3 * el_s / steps_s,
                                                  "steps": steps_s, "workload": wl_s, "sharding": sh_s}, **rec_s)
                    side["shared_factor_allgather"] = dict(extra.get("shared_factor", {}), value=out["value"], ms_per_step=out["ms_per_step"])
            # (r) the same shared-factor job at more samples per factor and rank: the factor (and its broadcast) is paid once
            # per posterior, the sample sweeps scale with the ranks -- which regime reaches what multiple of one rank
            leg["name"] = "regimes"
            regimes = [int(x) for x in args.regimes.split(",") if x.strip()]
            reg = {}
            for kr in regimes:
                jr = post.ShardedPosterior(eng, dist=dist, rank=rank, world=world, k_samples=kr, group=args.group,
                                           force_shared=args.force_shared, keep_samples=False, timing=True)
                jr.step(1 << 21)

                def run_r(first, count, jr=jr):
                    for s in range(count):
                        jr.step(first + s)
                el = timed(run_r, sync, dist, torch, 0, 3)
                ph = gather_phases(jr)
                if rank == 0:
                    reg[str(kr)] = {"value": jr.solves_per_step() * 3 / el, "unit": "solves/s", "ms_per_step": 1e3 * el / 3,
                                    "samples_per_posterior_and_rank": kr, "phase_ms_last_step": ph}
            # (a) the same jobs on ONE rank (no broadcast): what sharing the factor is compared with
            leg["name"] = "one_rank_same_job"
            if rank == 0:
                e1 = post.HipEngine(pkg, w, device_index=local, batch=eng.batch, values=eng.values_host, rhs=eng.rhs[:, 0, :].cpu().numpy(), keep_l=keep_l)
                for kr in [args.samples] + regimes:
                    j1 = post.ShardedPosterior(e1, k_samples=kr, replicate_factor=True, keep_samples=False)
                    if kr == args.samples:
                        j1.prepare()
                    j1.step(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for s in range(3):
                        j1.step(1 + s)
                    torch.cuda.synchronize()
                    t1 = (time.perf_counter() - t0) / 3
                    rec = {"ms_per_step": 1e3 * t1, "value": e1.batch * (1 + kr) / t1,
                           "note": f"rank 0 alone: factor + mean + {kr} samples per posterior, no broadcast"}
                    if kr == args.samples:
                        side["one_rank_same_job"] = rec
                        rec["n_rank_over_one_rank"] = (out["value"] if shared else side["shared_factor"]["value"]) / rec["value"]
                    else:
                        reg[str(kr)]["one_rank"] = rec
                        reg[str(kr)]["n_rank_over_one_rank"] = reg[str(kr)]["value"] / rec["value"]
                side["regimes"] = reg
                e1.F.close()
            eng.F.close()
            sync()
            # (b) C4: elliptic 512^2, 256 samples sharded over the ranks, one shared factor
            leg["name"] = "c4_elliptic512"
            try:
                w4 = pkg.workloads.make("elliptic512")
                k4 = max(1, 256 // world)
                e4, j4 = shared_job(w4, 1, k4)

                def run4(first, count):
                    for s in range(count):
                        j4.step(first + s)
                run4(0, 1)
                el4 = timed(run4, sync, dist, torch, 1, 3)
                ph4 = gather_phases(j4)
                if rank == 0:
                    side["c4_elliptic512"] = {"ms_per_job": 1e3 * el4 / 3, "value": (1 + k4 * world) * 3 / el4, "unit": "solves/s",
                                              "samples_total": k4 * world, "samples_per_rank": k4,
                                              "root_factor_ms": (ph4 or {}).get("root", {}).get("factor_ms"), "phase_ms_last_step": ph4,
                                              "workload": f"{w4.name}: n={w4.n}, {w4.n_blocks} blocks x {w4.block_size}"}
                e4.F.close()
            except Exception as e:      # noqa: BLE001
                if rank == 0:
                    side["c4_elliptic512"] = {"error": repr(e)[:300]}
            sync()
            if shared:
                # (c) independent problems per rank (the default headline's mode): no data-path collective
                leg["name"] = "problems_mode"
                pj = ProblemsJob(pkg, post, w, torch, local, args.config, args.batch, max(1, args.streams), args.samples, rank, keep_l)
                pj.run(0, 1)
                steps_p = max(2, args.steps // 4)
                elp = timed(pj.run, sync, dist, torch, 1, steps_p)
                if rank == 0:
                    side["problems_mode"] = {"value": world * pj.solves_per_step() * steps_p / elp, "unit": "solves/s",
                                             "ms_per_step": 1e3 * elp / steps_p, "steps": steps_p,
                                             "note": f"{pj.n_streams} streams x batch {pj.batch} independent posteriors per rank, no data-path collective"}
                pj.close()
                pj = None
        except Exception as e:      # noqa: BLE001
            # a leg that fails the same way on every rank (an API error, memory) must not cost the headline: record it and go on
            # to the end; a failure on ONE rank leaves the others in a collective, which the watchdog above ends
            side["error"] = f"leg '{leg['name']}' raised on rank {rank}: {repr(e)[:300]}; exit code 4"
            sys.stderr.write(f"bench.py rank {rank}: {side['error']}\n")
            leg["failed"] = True
        if rank == 0:
            out["side_legs"] = side
            # what a SCALE record is read for, at the top level: north_star's job in both forms, what it
            # puts on a link, how many ranks RCCL saw, and for C4 the serial root factorisation beside the whole job
            sg = side.get("shared_factor_allgather") or {}
            sb = side.get("shared_factor") or ({} if not shared else dict(extra.get("shared_factor", {}), value=out["value"]))
            out["shared_factor_solves_per_s"] = sg.get("value") if sg else sb.get("value")
            out["shared_factor_form"] = "allgather" if sg else sb.get("form")
            out["shared_factor_broadcast_solves_per_s"] = sb.get("value")
            out["bytes_per_link_per_step"] = {"allgather": sg.get("bytes_per_link_per_step"), "broadcast": sb.get("bytes_per_link_per_step")}
            out["rccl_ranks"] = world if (transport == "cabi" or backend == "nccl") else 0
            c4 = side.get("c4_elliptic512") or {}
            out["c4_elliptic512"] = {k: c4.get(k) for k in ("ms_per_job", "root_factor_ms", "value", "samples_total") if k in c4}
        watchdog.cancel()
    elif pj is not None and world > 1:
        pj.close()
        pj = None

    # ------------------------------------------------------------------ N = 1, plain run: what the timed handles' persistent
    # launches did (a counter read, no further launch), then their HBM back
    if rank == 0 and world == 1 and not shared and not args.full:
        ps = pj.persist_state()
        out["persist_aborts"] = ps["persist_aborts"]
        out["persist"] = ps
        pj.close()
        pj = None

    # ------------------------------------------------------------------ N = 1, --full: per-kernel roofline + parity + CPU baseline
    if rank == 0 and world == 1 and not shared and args.full:
        eng.F.set_profiling(1)
        with torch.cuda.stream(pj.jobs[0][0]):
            job.step(10_000)
        torch.cuda.synchronize()
        st = eng.F.stats()
        shapes = eng.F.gemm_shapes()
        eng.F.set_profiling(0)
        ms, work, cnt = st["kernel_ms"], st["kernel_work"], st["kernel_launches"]
        # dominant kernel = the class with the largest time in one instrumented step of one handle (HIP events on the
        # handle's stream around every launch); both symbols of the 64 x 64 GEMM kernel are also reported together
        dom = max(KERNEL_CLASSES, key=lambda c: ms[c])
        name, bound = KERNEL_CLASSES[dom]
        if bound == "mfma":
            achieved, peak, unit = work[dom] / (ms[dom] * 1e-3) / 1e12, PEAK_FP64_MFMA_TFLOPS, "TFLOP/s"
        else:
            achieved, peak, unit = work[dom] / (ms[dom] * 1e-3) / 1e9, PEAK_HBM_GBPS, "GB/s"
        traffic, traffic_src = None, None
        if w.name == "darcy256":
            # kernel symbol of the class as a rocprofv3 trace spells it
            sym = {14: "gemm_f64_dma<64,64,false", 15: "gemm_f64_dma<64,64,true", 0: "gemm_f64_mfma<false,false", 11: "gemm_f64_mfma<false,true",
                   16: "potrf_diag128", 10: "spmm_bxt_tiles", 13: "gemm_f64_ll"}.get(dom, name)
            got, traffic_src = pmc_traffic("hbm_traffic", [sym], batch=eng.batch)
            if got:
                traffic = next(iter(got.values()))
        gemm_cls = [c for c in (0, 11, 12, 13, 14, 15, 18, 6, 7) if ms[c] > 0]
        tw = sum(work[c] for c in gemm_cls) / max(sum(ms[c] for c in gemm_cls), 1e-9) / 1e9 if gemm_cls else 0.0
        out["roofline"] = {"bound": bound, "achieved": achieved, "peak": peak, "unit": unit,
                           "frac": achieved / peak, "traffic": traffic, "traffic_source": traffic_src, "kernel": name,
                           "launches_per_step": int(cnt[dom]), "avg_launch_us": 1e3 * ms[dom] / max(cnt[dom], 1),
                           "work": "executed flops (structurally skipped K ranges not counted)",
                           "timing": "one instrumented step of one handle; GEMM launches carry the dispatch's own begin / end time "
                                     "stamps (hipExtLaunchKernelGGL start / stop events) = the duration a rocprofv3 kernel trace reports",
                           "all_gemm_symbols_time_weighted": {"achieved": tw, "frac": tw / PEAK_FP64_MFMA_TFLOPS,
                                                              "ms_per_step": sum(ms[c] for c in gemm_cls),
                                                              "symbols": [KERNEL_CLASSES[c][0] for c in gemm_cls]}}
        # the HBM-bound leg of the path (north_star: sweep HBM GB/s against the 8 TB/s roofline): the k = 1 GEMV
        # sweep kernels of the same instrumented step, on the bytes they stream (Linv triangles + C inside its staircase)
        out["kernels"] = {KERNEL_CLASSES[c][0]: {"ms_per_step": ms[c], "launches": int(cnt[c]),
                                                  ("tflops" if KERNEL_CLASSES[c][1] == "mfma" else "gbps"):
                                                  (work[c] / (ms[c] * 1e-3) / (1e12 if KERNEL_CLASSES[c][1] == "mfma" else 1e9)) if ms[c] > 0 else 0.0}
                          for c in KERNEL_CLASSES}
        # the GEMM launches of that step by shape (where the time-weighted figure comes from): M x N outputs per problem, K, flags
        # (tri: triangular K range, lower: lower tiles only, kb: per-tile staircase bounds), flops as booked = executed
        gsum = max(sum(g["ms"] for g in shapes), 1e-9)
        out["gemm_by_shape"] = [{"kernel": KERNEL_CLASSES.get(g["class"], (str(g["class"]),))[0], "MxNxK": [g["M"], g["N"], g["K"]],
                                 "tri": g["tri"], "lower": g["lower_only"], "kb": g["k_bounds"], "problems": g["problems"],
                                 "launches": g["launches"], "ms": round(g["ms"], 3), "share": round(g["ms"] / gsum, 4),
                                 "tflops": round(g["flops"] / max(g["ms"], 1e-9) / 1e9, 2)}
                                for g in sorted(shapes, key=lambda g: -g["ms"]) if g["launches"] > 0]
        # the same symbols restricted to the launches that fill the chip (>= 1024 workgroups of 64 x 64 outputs = every
        # workgroup slot of the 256 CUs): what the kernel does when the launch is not the limit
        def wgs(g):
            tm, tn = g["M"] // 64, g["N"] // 64
            return (tm * (tm + 1) // 2 if g["lower_only"] and g["M"] == g["N"] else tm * tn) * g["problems"]
        big = [g for g in shapes if g["launches"] > 0 and wgs(g) >= 1024 and g["class"] in (0, 11, 14, 15)]
        if big:
            bms, bfl = sum(g["ms"] for g in big), sum(g["flops"] for g in big)
            out["roofline"]["chip_filling_launches"] = {"achieved": bfl / bms / 1e9, "frac": bfl / bms / 1e9 / PEAK_FP64_MFMA_TFLOPS,
                                                        "ms_per_step": bms, "share_of_gemm_time": bms / gsum,
                                                        "launches_per_step": sum(g["launches"] for g in big),
                                                        "note": "GEMM launches of >= 1024 workgroups; the symbol-level figures above also average "
                                                                "over the short products of the diagonal chain and the 64-row sweep panels"}
        executed = sum(work[c] for c in KERNEL_CLASSES if KERNEL_CLASSES[c][1] == "mfma")
        # phase times of the un-instrumented path (whole batch of one handle)
        eng.F.refactor(eng.nz)
        mu = eng.mean()
        s1 = eng.F.stats()
        eng.sample(args.samples, mu, 0x5EED, 0)
        s2 = eng.F.stats()
        out["phases_ms"] = {"factor": s1["factor_ms"], "mean_2_sweeps": s1["solve_ms"], "samples_1_sweep": s2["sample_ms"]}
        out["factor_tflops_lapack_count"] = st["factor_flops"] / (s1["factor_ms"] * 1e-3) / 1e12
        out["whole_job_executed_tflops"] = executed * pj.n_streams / (1e-3 * out["ms_per_step"]) / 1e12
        out["sweep_k1_gbps"] = {"reference_dense_blocks": s1["sweep_bytes"] / (0.5 * s1["solve_ms"] * 1e-3) / 1e9,
                                "streamed": s1["sweep_bytes_streamed"] / (0.5 * s1["solve_ms"] * 1e-3) / 1e9}
        out["factor_bytes_per_posterior_gb"] = s1["factor_bytes"] / eng.batch / 1e9
        if ms[3] > 0:
            # achieved = the mean solve as the product runs it: both sweeps replayed from their HIP graph, HIP events on the
            # handle's stream around the replay (pack / unpack of the right-hand side included), over the bytes the 254
            # GEMV launches stream.  Beside it the same launches timed one by one in eager mode (an event pair per
            # launch adds the dispatch gap: 28.7 us against 23.9 us per launch in the rocprofv3 trace).
            g_graph = 2.0 * s1["sweep_bytes_streamed"] / (s1["solve_ms"] * 1e-3) / 1e9      # (stats: bytes of ONE sweep)
            # PMC traffic per launch, launch-weighted over every sweep_gemv* symbol of the profiled step (coupling window, X_aa /
            # L_ba / X_bb parts, forward / backward)
            sweep_traffic, sweep_traffic_src = None, None
            if w.name == "darcy256":
                sweep_traffic, sweep_traffic_src = pmc_traffic_weighted("hbm_traffic", "sweep_gemv", batch=eng.batch)
            g3 = work[3] / (ms[3] * 1e-3) / 1e9
            out["roofline_sweep"] = {"bound": "hbm", "achieved": g_graph, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                     "frac": g_graph / PEAK_HBM_GBPS, "kernel": "sweep_gemv_n / sweep_gemv_t",
                                     "launches_per_step": int(cnt[3]), "avg_launch_us": 1e3 * s1["solve_ms"] / max(cnt[3], 1),
                                     "timing": "graph replay of the k = 1 forward + backward sweep (events around the replay)",
                                     "bytes": "streamed: lower triangle of Linv_i, C_i inside its staircase window",
                                     "traffic": sweep_traffic, "traffic_source": sweep_traffic_src,
                                     "algorithmic_bytes_per_launch": 2.0 * s1["sweep_bytes_streamed"] / max(cnt[3], 1),
                                     "eager_per_launch_events": {"achieved": g3, "frac": g3 / PEAK_HBM_GBPS,
                                                                 "avg_launch_us": 1e3 * ms[3] / max(cnt[3], 1)}}
        # persistent launches of the timed handles: aborts (0 = none gave a wait up), route (0 none, 1 block, 2 panel, 3 panel
        # diagonal block of a small batch) and the CUs each handle holds of the device's budget
        ps = pj.persist_state()
        out["persist_aborts"] = ps["persist_aborts"]
        out["persist"] = ps
        pj.close()
        if not args.no_single_problem:
            # latency of ONE problem (batch 1) on the same GPU: what tridiagonal_cholesky(A, N) as the reference
            # defines it (one matrix) delivers
            F1 = pkg.TridiagonalCholeskyFactor(device=local, stream=torch.cuda.current_stream().cuda_stream).factor(w.Q, w.n_blocks)
            nz1 = torch.from_numpy(w.Q.data).cuda(); rhs1 = torch.from_numpy(w.rhs).cuda()
            lat, fms = [], []
            # factor, then mean + samples in ONE call (gmrf_bt_posterior: where the sweeps are persistent launches the samples' sweep
            # runs beside the mean's two; bitwise the two calls) -- and, for the record, the same job as the three separate calls
            lat_sep, sol_sep, sam_sep = [], [], []
            for _ in range(4):
                torch.cuda.synchronize(); t1 = time.perf_counter()
                F1.refactor(nz1); mu1 = pkg.ldiv(F1, rhs1); sol_sep.append(F1.stats()["solve_ms"])
                F1.sample(args.samples, mean=mu1, seed=1, like=rhs1)
                torch.cuda.synchronize(); lat_sep.append(time.perf_counter() - t1)
                sam_sep.append(F1.stats()["sample_ms"])
            post_ms = []
            for _ in range(4):
                torch.cuda.synchronize(); t1 = time.perf_counter()
                F1.refactor(nz1); fms.append(F1.stats()["factor_ms"])
                F1.posterior(rhs1, args.samples, seed=1)
                torch.cuda.synchronize(); lat.append(time.perf_counter() - t1)
                post_ms.append(F1.stats()["solve_ms"] + F1.stats()["sample_ms"])      # (beside: the whole call is in solve_ms, sample_ms = 0)
            lat1, f1 = min(lat[1:]), min(fms[1:])
            s1p = F1.stats()
            out["single_problem"] = {"latency_ms": 1e3 * lat1, "solves_per_s": (1 + args.samples) / lat1, "factor_ms": f1,
                                     "factor_tflops_lapack_count": s1p["factor_flops"] / (f1 * 1e-3) / 1e12,
                                     "persist_route": int(s1p["persist_route"]), "persist_aborts": int(s1p["persist_aborts"]),
                                     "persist_cus": int(s1p["persist_cus"]), "persist_refused": int(s1p["persist_refused"]),
                                     "sweep_persist": int(s1p["sweep_persist"]), "mean_and_samples_ms": min(post_ms[1:]),
                                     "call": "refactor + posterior (mean and samples in one call)",
                                     "separate_calls": {"latency_ms": 1e3 * min(lat_sep[1:]), "solve_ms": min(sol_sep[1:]),
                                                        "sample_ms": min(sam_sep[1:])}}
            # (top level too, so that the driver's record keeps them: VERDICT r4 item 1)
            out["single_problem_latency_ms"] = 1e3 * lat1
            out["single_problem_factor_ms"] = f1
            out["persist_aborts"] = out.get("persist_aborts", 0) + int(s1p["persist_aborts"])
            F1.close()
        if not args.no_full_loop and args.config.startswith("darcy"):
            try:
                out["full_loop"] = full_loop(pkg, torch, int(args.config[5:]), args.batch, local, not args.no_cpu_baseline)
            except Exception as e:      # noqa: BLE001
                out["full_loop"] = {"error": repr(e)[:300]}
        if not args.no_spmm:
            try:
                out["roofline_spmm"] = spmm_roofline(pkg, torch)
            except Exception as e:      # noqa: BLE001
                out["roofline_spmm"] = {"error": repr(e)[:300]}
        if not args.no_cpu_baseline:
            base, (Qs, nbs, rhs_s, Z, (mu_o, X_o)) = cpu_baseline(w, args.samples)
            out["cpu_baseline"] = base
            out["speedup_vs_cpu"] = out["value"] / base["value"]
            out["cpu_sparse_direct"] = cpu_sparse_direct(w, args.samples)
            # parity of the TIMED route against the oracle (the full-size comparison of the same route lives in
            # tests/test_gpu_parity.py::test_measured_path_darcy256_batch_against_oracle): a batch of 8 coefficient fields
            # on the leading blocks of the workload, keep_l = 0, on a StreamSet stream, ShardedPosterior.step replayed
            # from its graphs -- mean, 64 device-drawn samples, logdet, exact and RBMC(50) variances of one problem
            from tests import measured_path as MP
            from oracle import bt_oracle as O
            fields = [w]
            for p in range(1, 8):
                wp = pkg.workloads.darcy(int(args.config[5:]), seed=523802340 + p) if args.config.startswith("darcy") else None
                fields.append(wp if wp is not None and wp.Q.nnz == w.Q.nnz and np.array_equal(wp.Q.indices, w.Q.indices) else None)
            ns_p = nbs * w.block_size
            Qp0 = w.Q.tocsr()[:ns_p, :ns_p].tocsc(); Qp0.sort_indices()
            vals_p, rhs_p = [], []
            for p, f in enumerate(fields):
                if f is None:
                    vals_p.append(Qp0.data * (1.0 + 0.01 * p)); rhs_p.append(w.rhs[:ns_p])
                else:
                    Qf = f.Q.tocsr()[:ns_p, :ns_p].tocsc(); Qf.sort_indices()
                    vals_p.append(Qf.data); rhs_p.append(f.rhs[:ns_p])
            pb = max(8, args.batch // 8 * 8)              # the timed batch size: same grids and kernel symbols per launch
            mp = MP.run(pkg, post, O, Qp0, nbs, np.stack([vals_p[p % 8] for p in range(pb)]),
                        np.stack([rhs_p[p % 8] for p in range(pb)]), k_samples=args.samples, check=(5,),
                        last_blocks=min(4, nbs), rbmc_k=50)
            out["parity"] = {"on": f"problem 5 of a batch of {pb} (8 coefficient fields) on the leading {nbs} blocks of {w.name}, driven like the "
                                   f"timed region (HipEngine / ShardedPosterior.step on a StreamSet stream, keep_l = 0, graph replay), "
                                   f"against the oracle", **mp[5], "kernel_classes_launched": mp["route"]}
    if rank == 0:
        print(json.dumps(out))
    if comm is not None:
        comm.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if leg_state.get("failed"):
        sys.exit(4)             # the line is out; a side leg raised on this rank


if __name__ == "__main__":
    main()
