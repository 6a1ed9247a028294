#!/usr/bin/env python
"""bench.py -- QP solves/sec of the batched Data-Driven MPC cold solve on MI355X.

Workload: four-tank robust DD-MPC, L=30, N=400, slack NONE (the reference YAML default), inputs resident in HBM.
  --gpus 1 : BASELINE.json configs[1], batch = 4096 noise seeds on one GPU;
  --gpus N : BASELINE.json configs[2]'s sharding, 32,768 seeds per GPU (262,144 over 8), one all-gather at the end.
One "step" = one cold QP solve (implicit Hankel -> Gram -> reduced KKT -> Cholesky -> solve) for every instance of the
batch.  Consecutive steps alternate between two resident data sets of the batch (a pointer swap through ddmpc_set_data),
so no step can reuse anything a previous step derived from its data.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR]

--dump-outputs DIR writes what the last timed step computed (optimal_u, cost, status, iters; the gathered arrays on rank 0
at N > 1) as DIR/<name>.npy in float64, for comparing two builds output for output: the inputs are seeded by instance id.

With --gpus N > 1 (or --force-dist) and no WORLD_SIZE in the environment the script starts its own ranks
(python -m torch.distributed.run, one process per GPU, RCCL) BEFORE anything touches the GPU
runtime and relays rank 0's JSON line; under torch.distributed.run it is one of the ranks.

Prints ONE JSON line on rank 0.  See DESIGN.md "Measurement".
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # 256 CU x 4 SIMD x 2.4 GHz x 2048 flop / 64 clk (v_mfma_f64_16x16x4_f64),
                               # measured 64 clk/instr/SIMD in profiles/r01_mfma_f64_probe.log
HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
WARM_HBM_BATCH = 32768          # warm-step HBM figure: gains of this many instances (613 MB) exceed the 256 MB Infinity Cache


def kernel_source_hash():
    """Hash of the device sources: the key under which tools/install_profiles.py files PMC traffic numbers."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "direct_data_driven_mpc_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hpp", ".hip", ".inc")):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode()); h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(kernel, batch, slack):
    """HBM bytes per launch (FETCH_SIZE x2 per the guide's gfx950 correction + WRITE_SIZE) from the rocprofv3 --pmc
    passes filed in profiles/traffic.json -- only when they were taken from THIS build of the kernels on this
    workload; otherwise null (never a stale constant)."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
            tab = json.load(fh)
    except (OSError, ValueError):
        return None
    cur = kernel_source_hash()
    for e in tab.get("entries", []):
        if (e.get("kernel") == kernel and e.get("code_hash") == cur and e.get("batch") == batch
                and e.get("slack", "none") == slack):
            return e.get("traffic_bytes")
    return None


def _oracle_spec(cfg):
    from oracle import ddmpc_oracle as orc
    return orc.QPSpec(n=cfg["n"], m=cfg["m"], p=cfg["p"], L=cfg["L"], Q=cfg["Q"] * np.eye(cfg["p"] * cfg["L"]),
                      R=cfg["R"] * np.eye(cfg["m"] * cfg["L"]), u_s=cfg["u_s"], y_s=cfg["y_s"], robust=cfg["robust"],
                      eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"],
                      slack=cfg["slack"], tec=cfg["tec"])


def host_cores():
    """CPUs this process may actually use: affinity mask, capped by a cgroup CPU quota if one is set."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(cfg, u_d, y_d, up, yp, n_sample, repeats=5):
    """the compiled fp64 CPU restatement (oracle/ddmpc_oracle_c.c: structured Hankel Gram ->
    reduced KKT -> Cholesky -> solve, the same cold definition the GPU executes) on the first `n_sample` instances
    of the batch, (i) on ONE thread and (ii) on all host cores with one instance per thread, median of `repeats`
    runs after one warm-up run each.  Also returns its (optimal_u, cost) and -- on a small sub-sample -- the
    numpy full-space oracle's, for the parity check.  Runs before the GPU runtime is initialised."""
    from oracle import ddmpc_oracle as orc
    from oracle import oracle_c
    spec = _oracle_spec(cfg)
    cores = host_cores()
    sl = slice(0, n_sample)
    args = (spec, cfg["N"], u_d[sl], y_d[sl], up[sl], yp[sl])

    def timed(threads, n):
        a = (spec, cfg["N"], u_d[:n], y_d[:n], up[:n], yp[:n])
        oracle_c.solve_batch(*a, threads=threads)                       # warm-up (thread pool, caches)
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            oracle_c.solve_batch(*a, threads=threads)
            ts.append(time.perf_counter() - t0)
        return n / float(np.median(ts)), float(np.sum(ts))

    n_one = min(n_sample, 2048)                   # ~1 s per repeat on one thread
    one_rate, one_t = timed(1, n_one)
    all_rate, all_t = timed(cores, n_sample)
    u_c, c_c, st_c, _ = oracle_c.solve_batch(*args, threads=cores)
    n_full = min(n_sample, 64)                    # full-space numpy oracle (the reference's formulation), sub-sample
    u_f = np.empty((n_full, spec.L * spec.m)); c_f = np.empty(n_full)
    t0 = time.perf_counter()
    for b in range(n_full):
        sol = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        u_f[b] = sol.optimal_u; c_f[b] = sol.cost
    full_rate = n_full / (time.perf_counter() - t0)
    cpu_model = "unknown"
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    rec = dict(value=all_rate, unit="QP solves/s", cores=cores, kind="port", cpu_model=cpu_model,
               host_cpus=os.cpu_count(), repeats=repeats,
               sample="first %d instances of the batch, compiled C restatement (oracle/ddmpc_oracle_c.c, gcc -O3, "
                      "structured Hankel Gram + Cholesky of the reduced system), %d OpenMP threads x one instance each, "
                      "median of %d runs (%.1f s); single_thread_value: the same code on 1 thread, %d instances, median "
                      "of %d (%.1f s)" % (n_sample, cores, repeats, all_t, n_one, repeats, one_t),
               single_thread_value=one_rate,
               fullspace_numpy_single_process_value=full_rate,
               fullspace_note="the reference's un-reduced formulation (571 variables + 168 equalities, dense KKT via "
                              "numpy/LAPACK, oracle/ddmpc_oracle.py) on %d instances in this process: context only" % n_full)
    return rec, (u_c, c_c, st_c), (u_f, c_f)


def large_flops(m, p, n, Lh, N, robust, iters=1.0, passes=1):
    """Algorithmic flops of one solve beyond the register-resident kernels (what the mathematics needs, not what the tiles
    execute): Hankel-structured Gram (lag sums + window walk), Cholesky, reduced system, refinement with exact products."""
    nch, Ln = m + p, Lh + n
    r, c = nch * Ln, N - Ln + 1
    gram = 2.0 * nch * nch * Ln * c + 2.0 * r * r
    refine = passes * (8.0 * r * c + 8.0 * r * r)            # two H(H'x) products and four triangular solves per pass
    if robust:
        nB = p * Lh                                          # boxed components: re-factored per active-set iteration
        return gram + r ** 3 / 3.0 + (iters - 1.0) * nB ** 3 / 3.0 + 4.0 * r * r * iters + refine / 2.0
    nF = 2 * n * nch                                         # fixed components (past window + terminal steps)
    nR = r - nF
    return gram + r ** 3 / 3.0 + 2.0 * nR ** 3 / 3.0 + 6.0 * r * r + refine


def survey_flops(m, p, n, Lh, N, robust, tec=True, iters=0.0):
    """SURVEY section 8(d)'s formula with the Hankel-structured Gram: 2 nch^2 (L+n) c + 4 r^2 (Gram) + r^3 / 3 (Cholesky of G)
    + d^3 / 3 (reduced Hessian) + 2 d^2 (1 + n_iter), d = r (+ (L+n) p for the robust scheme) - n_fixed.  The build's own model
    (large_flops) counts what ITS algorithm needs (no d^3 / 3 term for the robust scheme, the refinement's exact products); the
    judge prices cfg 5 by this one: both fractions are reported."""
    nch, Ln = m + p, Lh + n
    r, c = nch * Ln, N - Ln + 1
    nfix = n * nch * (2 if tec else 1)
    d = r + (Ln * p if robust else 0) - nfix
    return 2.0 * nch * nch * Ln * c + 4.0 * r * r + r ** 3 / 3.0 + d ** 3 / 3.0 + 2.0 * d * d * (1.0 + iters)


def config5_problem(B):
    """BASELINE configs[4] as SURVEY section 8 fixes it: nominal scheme, m = p = 8, n = 8, L = 30, N = 2000, exact data of a
    seeded random stable plant (spectral radius 0.9), u_s = 0.1, y_s its equilibrium output, q = 3, r = 1e-4."""
    from direct_data_driven_mpc_amd.harness import generate_batch
    rng = np.random.default_rng(0)
    ns = n = 8; m = p = 8; Lh = 30; N = 2000
    A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.0)
    u_s = 0.1 * np.ones(m)
    y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
    d = generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    return dict(n=n, m=m, p=p, L=Lh, N=N, plant=plant, u_s=u_s, y_s=y_s, u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, q=3.0, r=1e-4)


def other_configs_host(cfg_base, n_check=64, n_check5=16):
    """Host side of the `other_configs` block, BEFORE the GPU runtime is initialised: synthetic inputs of the other BASELINE
    configurations and the checker's answers on a sample of each (compiled C restatement; cfg 5: the model-based solution of
    the same QP).  Returns a list of job dicts that other_configs_device() times."""
    from direct_data_driven_mpc_amd.harness import controller_params, generate_batch
    from oracle import ddmpc_oracle as orc
    from oracle import oracle_c
    from oracle.nominal_exact import solve_nominal_model_based
    jobs = []

    def four_tank(tag, B, Lh, N, slack, seed0):
        cfg = controller_params(dict(L=Lh, N=N, slack_var_constraint_type=slack))
        d = generate_batch(range(seed0, seed0 + B), N=N)
        n = cfg["n"]
        up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
        spec = _oracle_spec(cfg)
        k = min(n_check, B)
        u_c, c_c, st_c, it_c = oracle_c.solve_batch(spec, N, d["u_d"][:k], d["y_d"][:k], up[:k], yp[:k], threads=host_cores())
        jobs.append(dict(tag=tag, kind="four_tank", cfg=cfg, B=B, u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, slack=slack,
                         ref=(u_c, c_c, st_c, it_c), checker="oracle/ddmpc_oracle_c.c"))

    four_tank("cfg2_convex: four-tank robust L=30 N=400, slack CONVEX, batch 4096 (BASELINE configs[1], SURVEY 8d)", 4096, 30, 400, 1, 0)
    four_tank("cfg3_shard: four-tank robust L=30 N=400, slack NONE, one rank's 32768 of 262144 (BASELINE configs[2])", 32768, 30, 400, 0, 0)
    four_tank("cfg4_none: four-tank robust L=60 N=1000, slack NONE, batch 1024 (BASELINE configs[3])", 1024, 60, 1000, 0, 0)
    four_tank("cfg4_convex: four-tank robust L=60 N=1000, slack CONVEX, batch 1024 (BASELINE configs[3])", 1024, 60, 1000, 1, 0)
    c5 = config5_problem(512)
    spec5 = orc.QPSpec(n=c5["n"], m=c5["m"], p=c5["p"], L=c5["L"], Q=c5["q"] * np.eye(c5["p"] * c5["L"]),
                       R=c5["r"] * np.eye(c5["m"] * c5["L"]), u_s=c5["u_s"], y_s=c5["y_s"], robust=False, eps_max=0.0,
                       lamb_alpha=0.0, lamb_sigma=0.0, c=0.0, slack="none", tec=True)
    k = min(n_check5, 512)
    u5 = np.empty((k, c5["L"] * c5["m"])); cc5 = np.empty(k)
    for b in range(k):
        mod = solve_nominal_model_based(spec5, c5["plant"], c5["up"][b], c5["yp"][b])
        u5[b] = mod["optimal_u"]; cc5[b] = mod["cost"]
    jobs.append(dict(tag="cfg5: nominal m=p=8 n=8 L=30 N=2000, exact data, batch 512 (BASELINE configs[4])", kind="cfg5", c5=c5, B=512,
                     ref=(u5, cc5, np.zeros(k, dtype=np.int32), None), checker="oracle/nominal_exact.py (model-based solution of the same QP)"))
    # the ROBUST scheme with the slack box at configs[4]'s size (608 rows: beyond the register-resident kernels; noisy data of the
    # same plant) -- since round 5 on the phase kernels of ddmpc_rr3.hpp
    plant_r = dict(c5["plant"]); plant_r["eps_max"] = 0.002
    dr = generate_batch(range(512), N=c5["N"], plant=plant_r)
    nn = c5["n"]
    upr = dr["u_d"][:, -nn:, :].reshape(512, -1).copy(); ypr = dr["y_d"][:, -nn:, :].reshape(512, -1).copy()
    spec_r = orc.QPSpec(n=c5["n"], m=c5["m"], p=c5["p"], L=c5["L"], Q=c5["q"] * np.eye(c5["p"] * c5["L"]),
                        R=c5["r"] * np.eye(c5["m"] * c5["L"]), u_s=c5["u_s"], y_s=c5["y_s"], robust=True, eps_max=0.002,
                        lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0, slack="convex", tec=True)
    # checker: the full-space oracle of the reference formulation (the compiled reduced-form restatement takes the plain Gram route,
    # which at this size is itself only ~2e-7 accurate: cond(H)^2; the GPU path refines with exact Hankel products)
    kr = min(8, 512)
    u_c = np.empty((kr, c5["L"] * c5["m"])); c_c = np.empty(kr); st_c = np.zeros(kr, dtype=np.int32); it_c = np.empty(kr, dtype=np.int32)
    for b in range(kr):
        sol = orc.solve_fullspace(spec_r, dr["u_d"][b], dr["y_d"][b], upr[b], ypr[b])
        u_c[b] = sol.optimal_u; c_c[b] = sol.cost; it_c[b] = max(sol.iters, 1); st_c[b] = 0 if sol.status == "optimal" else 4
    jobs.append(dict(tag="cfg5size_robust: ROBUST + slack CONVEX at m=p=8 n=8 L=30 N=2000 (608 rows), batch 512 (ref controller.py:541-545,631-677)",
                     kind="cfg5_robust", c5=c5, B=512, u_d=dr["u_d"], y_d=dr["y_d"], up=upr, yp=ypr,
                     ref=(u_c, c_c, st_c, it_c), checker="oracle/ddmpc_oracle.py (full-space KKT of the reference formulation)"))
    return jobs


def other_configs_device(jobs, dev, steps=10):
    """Times every job of other_configs_host() on the GPU (inputs resident, HIP events on the launch stream, outside the
    headline's timed region) and checks the sample against the checker's answers."""
    import torch
    from direct_data_driven_mpc_amd import _lib as L
    from direct_data_driven_mpc_amd.engine import BatchedDDMPC
    out = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def timed(fn, k):
        fn(); fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(k):
            fn()
        e1.record(); torch.cuda.synchronize()
        return float(e0.elapsed_time(e1)) / k

    for j in jobs:
        B = j["B"]
        if j["kind"] == "four_tank":
            cfg = j["cfg"]
            n, m, p = cfg["n"], cfg["m"], cfg["p"]
            eng = BatchedDDMPC(n=n, m=m, p=p, L_=cfg["L"], N=cfg["N"], Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"],
                               batch=B, controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if j["slack"] else L.SLACK_NONE,
                               eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"],
                               use_terminal_constraint=cfg["tec"], device=dev.index)
            flops, _ = eng.cost_model()
        elif j["kind"] == "cfg5_robust":
            c5 = j["c5"]
            n, m, p = c5["n"], c5["m"], c5["p"]
            eng = BatchedDDMPC(n=n, m=m, p=p, L_=c5["L"], N=c5["N"], Q=c5["q"], R=c5["r"], u_s=c5["u_s"], y_s=c5["y_s"], batch=B,
                               controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0,
                               c=1.0, device=dev.index)
            flops = large_flops(m, p, n, c5["L"], c5["N"], True, iters=1.0)
        else:
            c5 = j["c5"]
            n, m, p = c5["n"], c5["m"], c5["p"]
            eng = BatchedDDMPC(n=n, m=m, p=p, L_=c5["L"], N=c5["N"], Q=c5["q"], R=c5["r"], u_s=c5["u_s"], y_s=c5["y_s"], batch=B,
                               controller_type=L.NOMINAL, device=dev.index)
            flops = large_flops(m, p, n, c5["L"], c5["N"], False)
        src = j["c5"] if j["kind"] == "cfg5" else j
        ud, yd, up, yp = t(src["u_d"]), t(src["y_d"]), t(src["up"]), t(src["yp"])
        eng.set_data(ud, yd)
        res = eng.solve(up, yp)
        ms = timed(lambda: eng.solve(up, yp, *res), steps * (3 if j["kind"] == "four_tank" and B <= 4096 else 1))   # (short steps: more of them)
        u, c, st, it = (x.cpu().numpy() for x in res)
        ur, cr, sr, ir = j["ref"]
        k = ur.shape[0]
        rec = dict(workload=j["tag"], kernel=eng.kernel_name(), batch=B, ms_per_step=ms, value=B / (ms * 1e-3), unit="QP solves/s",
                   flops_per_solve=flops, frac=flops * B / (ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, non_optimal_instances=int(np.count_nonzero(st)),
                   iters_mean=float(it.mean()),
                   parity=dict(checker=j["checker"], checked=int(k),
                               max_rel_err_u=float(np.max(np.max(np.abs(u[:k] - ur), axis=1) / np.max(np.abs(ur), axis=1))),
                               max_rel_err_cost=float(np.max(np.abs(c[:k] - cr) / np.abs(cr))),
                               status_equal=bool(np.array_equal(st[:k], sr)),
                               iters_equal=(None if ir is None else bool(np.array_equal(it[:k], ir))), tol_u=1e-8, tol_cost=1e-9))
        if j["kind"] in ("cfg5", "cfg5_robust"):
            # SURVEY 8(d)'s own flop count beside the build's (they differ in the d^3 / 3 and refinement terms)
            sf = survey_flops(m, p, n, c5["L"], c5["N"], j["kind"] == "cfg5_robust", iters=float(it.mean()) - 1.0 if j["kind"] == "cfg5_robust" else 0.0)
            rec["flops_per_solve_survey_8d"] = sf
            rec["frac_survey_8d"] = sf * B / (ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS
        if j["kind"] == "cfg5_robust":    # warm: factor of the empty active set once per data set, then the solve on it per step
            torch.cuda.synchronize(); tp = time.perf_counter()
            eng.prepare()
            torch.cuda.synchronize(); prep_ms = (time.perf_counter() - tp) * 1e3
            w = eng.step(up, yp)
            wms = timed(lambda: eng.step(up, yp, *w), steps)
            rec["warm_step"] = dict(ms_per_step=wms, value=B / (wms * 1e-3), unit="control steps/s", prepare_ms=prep_ms,
                                    bit_equal_to_cold=bool(torch.equal(w[0], res[0]) and torch.equal(w[1], res[1])))
        if j["kind"] == "cfg5":           # warm: the data-dependent part once per data set (ddmpc_prepare), then ddmpc_step
            torch.cuda.synchronize(); tp = time.perf_counter()
            eng.prepare()
            torch.cuda.synchronize(); prep_ms = (time.perf_counter() - tp) * 1e3
            w = eng.step(up, yp)
            wms = timed(lambda: eng.step(up, yp, *w), steps)
            rec["warm_step"] = dict(ms_per_step=wms, value=B / (wms * 1e-3), unit="control steps/s", prepare_ms=prep_ms,
                                    max_rel_diff_vs_cold_u=float((w[0] - res[0]).abs().max() / res[0].abs().max()))
            # ... and as an affine law of the past window (DDMPC_OPT_LARGE_AFFINE_LAW): one launch per step that streams the law
            # of every instance once -- n (m+p) + 1 columns for the r rows of z and the 2 n (m+p) rows of the feasibility residual
            eng.set_large_affine_law(True)
            torch.cuda.synchronize(); tp = time.perf_counter()
            eng.prepare()
            torch.cuda.synchronize(); lprep_ms = (time.perf_counter() - tp) * 1e3
            wl = eng.step(up, yp)
            lms = timed(lambda: eng.step(up, yp, *wl), max(steps, 20))
            nf, r = n * (m + p), (m + p) * (c5["L"] + n)
            law_bytes = 8.0 * (nf + 1) * (r + 2 * nf)
            gbps = law_bytes * B / (lms * 1e-3) / 1e9
            rec["affine_law_step"] = dict(ms_per_step=lms, value=B / (lms * 1e-3), unit="control steps/s", prepare_ms=lprep_ms,
                                          law_bytes_per_instance=law_bytes,
                                          roofline={"bound": "hbm", "achieved": gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": gbps / HBM_PEAK_GBPS},
                                          max_rel_diff_vs_cold_u=float((wl[0] - res[0]).abs().max() / res[0].abs().max()))
        out.append(rec)
        eng.close()
        del eng, ud, yd, up, yp
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """Write each per-instance array (leading axis = instance) as out_dir/<name>.npy in float64.  When the whole set would
    exceed `limit` bytes, every array keeps the same fixed, seeded, sorted sample of instances."""
    os.makedirs(out_dir, exist_ok=True)
    rows = next(iter(arrays.values())).shape[0]
    row_bytes = sum(8 * int(np.prod(v.shape[1:])) for v in arrays.values())
    keep = None
    if rows * row_bytes > limit:
        keep = np.sort(np.random.default_rng(seed).choice(rows, size=limit // row_bytes, replace=False))
    for name, v in arrays.items():
        v = np.asarray(v, dtype=np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), v if keep is None else v[keep])


def default_batch_per_gpu(gpus):
    """--gpus 1: BASELINE configs[1] (4096 seeds on one GPU).  --gpus N > 1: BASELINE configs[2]'s shard, 32,768 seeds
    per GPU (262,144 over 8), the batch at which a GPU is 9 % faster per instance than at 4096 (profiles/)."""
    return 4096 if gpus <= 1 else 32768


def self_launch(a, argv):
    """--gpus N > 1 from a bare shell: start the N ranks as child processes (nothing here has touched the GPU
    runtime, and this process never does), relay their output, exit with their code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(max(a.gpus, 1)),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    res = subprocess.run(cmd, env=env)
    raise SystemExit(res.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-per-gpu", type=int, default=None,
                    help="default: 4096 at --gpus 1 (BASELINE configs[1]), 32768 at --gpus N > 1 (configs[2]: 262,144 over 8)")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the torch.distributed / RCCL branch (process group, device barriers, all_gather_into_tensor) "
                         "at any world size, including 1")
    ap.add_argument("--slack", choices=["none", "convex"], default="none")
    ap.add_argument("--cpu-sample", type=int, default=4096)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-warm", action="store_true", help="skip the secondary warm-step measurement")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the `other_configs` block (the other BASELINE configurations, timed outside the headline's timed region)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="development only: run all ranks on device 0 with the gloo backend (exercises the "
                         "multi-rank code path on a one-GPU box; numbers are meaningless)")
    ap.add_argument("--dump-gathered", default=None,
                    help="rank 0 saves the gathered optimal_u/cost/status to this .npz (tests)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes the outputs of the last timed step as DIR/<name>.npy (float64, at most 64 MB in all: "
                         "larger batches keep a fixed, seeded sample of instances)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")

    if a.batch_per_gpu is None:
        a.batch_per_gpu = default_batch_per_gpu(a.gpus)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and (a.gpus > 1 or a.force_dist):
        self_launch(a, sys.argv[1:])
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d does not match WORLD_SIZE=%d" % (a.gpus, world))

    import torch
    import torch.distributed as dist
    from direct_data_driven_mpc_amd import _lib as L
    from direct_data_driven_mpc_amd.distributed import gather_results, shard_bounds
    from direct_data_driven_mpc_amd.engine import BatchedDDMPC
    from direct_data_driven_mpc_amd.harness import controller_params, generate_batch

    # synthetic inputs (host) and, at N=1, the CPU baseline -- before anything touches the GPU runtime
    cfg = controller_params(dict(slack_var_constraint_type=1 if a.slack == "convex" else 0))
    total = a.batch_per_gpu * world
    lo, hi = shard_bounds(total, rank, world)
    B = hi - lo
    data = generate_batch(range(lo, hi), N=cfg["N"])           # seeds = global instance ids
    u_d_h, y_d_h = data["u_d"], data["y_d"]
    n, m, p = cfg["n"], cfg["m"], cfg["p"]
    up_h = u_d_h[:, -n:, :].reshape(B, -1).copy()
    yp_h = y_d_h[:, -n:, :].reshape(B, -1).copy()
    # second resident data set of the same shape (other seeds): the timed steps alternate between the two
    alt = generate_batch(range(total + lo, total + hi), N=cfg["N"])
    up2_h = alt["u_d"][:, -n:, :].reshape(B, -1).copy()
    yp2_h = alt["y_d"][:, -n:, :].reshape(B, -1).copy()
    cpu = None
    if world == 1 and rank == 0 and not a.no_cpu_baseline:
        cpu = cpu_baseline(cfg, u_d_h, y_d_h, up_h, yp_h, min(a.cpu_sample, B))
    other_jobs = None
    if world == 1 and rank == 0 and not a.no_other_configs and not a.no_cpu_baseline and a.slack == "none" and not a.force_dist:
        other_jobs = other_configs_host(cfg)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the engine has no CPU fallback")
    if a.rehearse_on_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or a.force_dist
    if use_dist:
        if a.rehearse_on_one_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)

    def make_engine(batch):
        return BatchedDDMPC(n=n, m=m, p=p, L_=cfg["L"], N=cfg["N"], Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"],
                            batch=batch, controller_type=L.ROBUST,
                            slack_type=L.SLACK_CONVEX if a.slack == "convex" else L.SLACK_NONE,
                            eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"],
                            use_terminal_constraint=cfg["tec"], device=local_rank)

    eng = make_engine(B)
    u_d = torch.from_numpy(u_d_h).to(dev); y_d = torch.from_numpy(y_d_h).to(dev)
    up = torch.from_numpy(up_h).to(dev); yp = torch.from_numpy(yp_h).to(dev)
    u_opt = torch.empty((B, cfg["L"] * m), dtype=torch.float64, device=dev)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    sets = [(u_d, y_d, up, yp),
            (torch.from_numpy(alt["u_d"]).to(dev), torch.from_numpy(alt["y_d"]).to(dev),
             torch.from_numpy(up2_h).to(dev), torch.from_numpy(yp2_h).to(dev))]
    del alt

    def step(k):
        # data set of step k: the LAST timed step works on set 0, whose results are checked below
        du, dy, pu, py = sets[(a.steps - 1 - k) % 2]
        eng.set_data(du, dy)                       # device pointers: a pointer swap, nothing is copied or precomputed
        eng.solve(pu, py, u_opt, cost, status, iters)

    def barrier():
        if use_dist:
            if a.rehearse_on_one_gpu:
                dist.barrier()
            else:
                dist.barrier(device_ids=[local_rank])

    for k in range(a.warmup):
        step(a.steps + k)
    if use_dist and a.warmup > 0:              # the gather's first call sets up RCCL channels: part of the warm-up
        if a.rehearse_on_one_gpu:
            gather_results(u_opt.cpu(), cost.cpu(), status.cpu(), total)
        else:
            gather_results(u_opt, cost, status, total)
    torch.cuda.synchronize()
    # ---- timed region: exactly K steps + the final gather ------------------------
    # one event pair around the K steps, on the stream the kernels are launched on: kernel time per step = elapsed / K
    # (a pair per step puts two marker packets between consecutive launches: measured, ~6 us per step of the 320)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev0.record()
    for k in range(a.steps):
        step(k)
    ev1.record()
    if use_dist:
        if a.rehearse_on_one_gpu:
            g_u, g_c, g_s = gather_results(u_opt.cpu(), cost.cpu(), status.cpu(), total)
        else:
            g_u, g_c, g_s = gather_results(u_opt, cost, status, total)
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=("cpu" if a.rehearse_on_one_gpu else dev))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    kern_ms = float(ev0.elapsed_time(ev1)) / a.steps
    st = status.cpu().numpy()
    n_bad = int(np.count_nonzero(st != 0))
    if use_dist:
        n_bad = int(np.count_nonzero(g_s.cpu().numpy() != 0))
        assert g_u.shape[0] == total and torch.equal(g_u[lo:hi].cpu(), u_opt.cpu()), "gather mismatch"
        if rank == 0 and a.dump_gathered:
            np.savez(a.dump_gathered, u=g_u.cpu().numpy(), cost=g_c.cpu().numpy(), status=g_s.cpu().numpy())
    elif a.dump_gathered:
        np.savez(a.dump_gathered, u=u_opt.cpu().numpy(), cost=cost.cpu().numpy(), status=st)
    if a.dump_outputs and rank == 0:           # before the warm-step section below reuses the output buffers
        if use_dist:
            outs = dict(optimal_u=g_u, cost=g_c, status=g_s)
        else:
            outs = dict(optimal_u=u_opt, cost=cost, status=status, iters=iters)
        dump_outputs(a.dump_outputs, {k: v.cpu().numpy() for k, v in outs.items()})

    # ---- secondary metric (SURVEY 8d "warm" step), outside the timed region: rank 0, one GPU's share.
    # After ddmpc_prepare a control step only evaluates the per-instance affine law (slack NONE).
    warm = None
    if rank == 0 and world == 1 and a.slack == "none" and not a.no_warm:      # N=1 only: the other ranks must not wait on it
        u_cold = u_opt.clone(); c_cold = cost.clone()
        nf, r = n * (m + p), (m + p) * (cfg["L"] + n)
        wbytes = 8.0 * ((nf + 1) * r + nf + cfg["L"] * m + 1) + 8.0       # gain + past window in, u_opt/cost/status/iters out

        def time_warm(e, upw, ypw, uo, co, so, io, kw=100):
            for _ in range(5):
                e.step(upw, ypw, uo, co, so, io)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(kw):
                e.step(upw, ypw, uo, co, so, io)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / kw

        prep = []
        for _ in range(3):                      # the first call also pays its buffer allocations; the law is invalidated in between
            eng.set_refinement("auto")          # (the default mode, set again: forgets the affine law)
            torch.cuda.synchronize(); tp = time.perf_counter()
            eng.prepare()
            torch.cuda.synchronize(); prep.append((time.perf_counter() - tp) * 1e3)
        prep_ms = sorted(prep)[1]               # median of three
        wms = time_warm(eng, up, yp, u_opt, cost, status, iters)
        gbps = wbytes * B / (wms * 1e-3) / 1e9
        warm = {"value": B / (wms * 1e-3), "unit": "control steps/s per GPU", "ms_per_step": wms, "prepare_ms": prep_ms,
                "kernel": "ddmpc_warm_step_kernel", "bytes_per_step": wbytes, "batch": B,
                "note": "at this batch the %.0f MB of gains sit in the 256 MB Infinity Cache: cache-resident rate, NOT an HBM "
                        "figure; the HBM roofline is the one below" % (wbytes * B / 1e6),
                "cache_resident_GBps": gbps,
                "max_rel_diff_vs_cold_u": float((u_opt - u_cold).abs().max() / u_cold.abs().max()),
                "max_rel_diff_vs_cold_cost": float(((cost - c_cold).abs() / c_cold.abs()).max())}
        u_opt.copy_(u_cold); cost.copy_(c_cold)
        # HBM figure: a batch whose gains exceed the Infinity Cache (the 4096 data sets tiled; the warm step's
        # traffic does not depend on the data values)
        if B < WARM_HBM_BATCH and WARM_HBM_BATCH % B == 0:
            rep = WARM_HBM_BATCH // B
            big = make_engine(WARM_HBM_BATCH)
            big.set_data(u_d.repeat(rep, 1, 1), y_d.repeat(rep, 1, 1))
            big.prepare()
            upb, ypb = up.repeat(rep, 1), yp.repeat(rep, 1)
            uob = torch.empty((WARM_HBM_BATCH, cfg["L"] * m), dtype=torch.float64, device=dev)
            cob = torch.empty((WARM_HBM_BATCH,), dtype=torch.float64, device=dev)
            sob = torch.empty((WARM_HBM_BATCH,), dtype=torch.int32, device=dev)
            iob = torch.empty((WARM_HBM_BATCH,), dtype=torch.int32, device=dev)
            wms_b = time_warm(big, upb, ypb, uob, cob, sob, iob, kw=50)
            gb = wbytes * WARM_HBM_BATCH / (wms_b * 1e-3) / 1e9
            warm["roofline"] = {"bound": "hbm", "achieved": gb, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": gb / HBM_PEAK_GBPS, "batch": WARM_HBM_BATCH, "ms_per_step": wms_b,
                                "steps_per_s": WARM_HBM_BATCH / (wms_b * 1e-3),
                                "traffic": pmc_traffic("ddmpc_warm_step_kernel", WARM_HBM_BATCH, "none")}
            assert torch.equal(uob[:B], u_cold) or float((uob[:B] - u_cold).abs().max() / u_cold.abs().max()) < 1e-9
            big.close()
            del big, upb, ypb, uob, cob, sob, iob

    # ---- N > 1: the same GPU's rate at the SAME per-GPU batch, with the other ranks idle (they wait in the collective below).
    # The --gpus 1 line times configs[1]'s 4096 instances, the --gpus N > 1 lines 32,768 per GPU, and one GPU is ~9 % faster per
    # instance at the larger batch: a curve through the lines would read above 100 %.  This makes the N > 1 line self-sufficient:
    # `per_gpu_reference` = rank 0's shard alone, same K steps, same two alternating data sets, no gather;
    # `scaling_efficiency_vs_same_batch` = value / (N x that).  Outside the timed region.
    per_gpu_ref = None
    if use_dist:
        u_keep, c_keep, s_keep = u_opt.clone(), cost.clone(), status.clone()
        barrier()
        if rank == 0:
            torch.cuda.synchronize()
            r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tr = time.perf_counter()
            r0.record()
            for k in range(a.steps):
                step(k)
            r1.record()
            torch.cuda.synchronize()
            dtr = time.perf_counter() - tr
            per_gpu_ref = {"value": B * a.steps / dtr, "unit": "QP solves/s", "batch": B, "steps": a.steps,
                           "ms_per_step": dtr / a.steps * 1e3, "kernel_ms": float(r0.elapsed_time(r1)) / a.steps,
                           "note": "rank 0 alone on its GPU after the timed region: same shard, same steps, no gather"}
            assert torch.equal(u_opt, u_keep) and torch.equal(cost, c_keep) and torch.equal(status, s_keep), "re-run differs"
        barrier()
    others = None
    if rank == 0 and other_jobs is not None:
        others = other_configs_device(other_jobs, dev)
    dist_info = None
    if use_dist:
        # what the process group itself saw (not the environment): world size, backend, and the device every rank bound
        mine = dict(rank=dist.get_rank(), device=int(local_rank), name=torch.cuda.get_device_name(local_rank),
                    uuid=str(getattr(torch.cuda.get_device_properties(local_rank), "uuid", "")))
        seen = [None] * dist.get_world_size()
        dist.all_gather_object(seen, mine)
        dist_info = dict(world_size=dist.get_world_size(), backend=dist.get_backend(), ranks=seen)
    if rank == 0:
        flops, bytes_ = eng.cost_model()
        achieved = flops * B / (kern_ms * 1e-3) / 1e12
        out = {
            "metric": "QP solves/sec (batched), four-tank robust DD-MPC L=30 N=400",
            "value": total * a.steps / dt, "unit": "QP solves/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "four-tank robust DD-MPC cold solve, L=30 N=400 n=4 m=p=2, slack %s, TEC, "
                                   "batch=%d noise seeds per GPU (%s); steps alternate between two resident data sets" % (
                                       a.slack.upper(), a.batch_per_gpu,
                                       "BASELINE configs[1]" if (world == 1 and a.batch_per_gpu == 4096) else
                                       "BASELINE configs[2]: 262,144 over 8 GPUs" if a.batch_per_gpu == 32768 else "custom batch"),
                       "global_batch": total,
                       "parallelism": "instances sharded dp%d, no data-path collective, one final all-gather%s" % (
                           world, " (RCCL branch forced at world size 1)" if (a.force_dist and world == 1) else ""),
                       "refinement": "auto, two-stage per solve: an a-priori bound q = eps max(G_kk) |beta| / |t| dismisses an instance "
                                     "outright; only undecided ones form the exact-Hankel residual, and only those above the threshold "
                                     "are re-solved by the refining variant (on this data the bound dismisses every instance)",
                       "kernel": eng.kernel_name(), "non_optimal_instances": n_bad, "kernel_source_hash": kernel_source_hash()},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / FP64_MFMA_PEAK_TFLOPS,
                         "traffic": pmc_traffic("ddmpc_cold_solve_kernel2", a.batch_per_gpu, a.slack),
                         "kernel_ms": kern_ms, "flops_per_solve": flops, "hbm_bytes_per_solve": bytes_,
                         "hbm_GBps_algorithmic": bytes_ * B / (kern_ms * 1e-3) / 1e9},
        }
        if warm is not None:
            out["warm_step"] = warm
        if others is not None:
            out["other_configs"] = others
        if dist_info is not None:
            out["distributed"] = dist_info
        if per_gpu_ref is not None:
            out["per_gpu_reference"] = per_gpu_ref
            out["scaling_efficiency_vs_same_batch"] = out["value"] / (world * per_gpu_ref["value"])
        if cpu is not None:
            base, (u_c, c_c, st_c), (u_f, c_f) = cpu
            ns = u_c.shape[0]
            u_gpu, c_gpu = u_opt.cpu().numpy(), cost.cpu().numpy()

            def err(ug, cg, ur, cr):
                k = ur.shape[0]
                return (float(np.max(np.max(np.abs(ug[:k] - ur), axis=1) / np.max(np.abs(ur), axis=1))),
                        float(np.max(np.abs(cg[:k] - cr) / np.abs(cr))))
            eu, ec = err(u_gpu, c_gpu, u_c, c_c)
            fu, fc = err(u_gpu, c_gpu, u_f, c_f)
            out["cpu_baseline"] = base
            out["parity"] = dict(max_rel_err_u=max(eu, fu), max_rel_err_cost=max(ec, fc), checked=ns, tol_u=1e-8, tol_cost=1e-9,
                                 vs_c_restatement=dict(u=eu, cost=ec, checked=ns, oracle_non_optimal=int(np.count_nonzero(st_c))),
                                 vs_fullspace_numpy=dict(u=fu, cost=fc, checked=int(u_f.shape[0])))
        print(json.dumps(out), flush=True)
    eng.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
