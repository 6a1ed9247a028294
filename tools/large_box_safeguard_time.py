"""Dev timing (GPU): DDMPC_OPT_LARGE_BOX_SAFEGUARD 0 against 1 on bounded ROBUST controllers beyond 271 rows
(rr3_box_safeguard_kernel, ddmpc_rr3_box_safe.hpp), batch 512 at the data tail, capacity 128, max_iter 50:

  cfg5:none:input, cfg5:convex:input   the cfg-5-size input box of tools/large_bounds_time.py (608 rows; per channel the 0.5 % /
                                       99.5 % quantiles of the unbounded solution's free inputs over the batch)
  tank70:convex:input02                four-tank, L = 70, 296 rows, u in [0, 2]

Per case and option: ddmpc_solve and ddmpc_step in ms by HIP events (median of --reps repeats after a warm-up call), the
instances that are not optimal split into "at the cap" (iters >= max_iter) and "beyond the capacity" (their peak exceeds it, or
the safeguard's working set did), the distribution of `iters`, and from the record of the last solve (ddmpc_debug_workspace)
  * the wide kernel's own cost per primal-dual iteration: ticks / iterations of an instance that converged below max_iter,
  * the cost per safeguard solve: rr3_box_safeguard_kernel's ticks of a finished instance / its solves (iters - max_iter),
both as the median per bucket of 32 of the peak number of active components, in us.

    python tools/large_box_safeguard_time.py [--batch 512] [--reps 5] [--capacity 128] [--only rows] [--json out.json]
"""
import argparse, ctypes as C, json, sys
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--capacity", type=int, default=128)
ap.add_argument("--only", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("large_box_safeguard_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B, MAX_ITER = a.batch, 50
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                        # warm-up: allocations, LDS attributes
    out = []
    for _ in range(a.reps):
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def record(eng, r):
    """[k, state, iterations, peak k, ticks] of every instance of the last solve."""
    rv = (r + 1) & ~1
    na, nm = C.c_int64(), C.c_int64()
    L.check(lib.ddmpc_debug_workspace(eng._h, 0, C.c_void_p(), 0, C.c_void_p(), 0, C.addressof(na), C.addressof(nm)))
    n = int(nm.value)
    cap = n - 4 - rv - 4
    meta = np.zeros(n, np.int32)
    out = np.zeros((B, 5), np.int64)
    for b in range(B):
        L.check(lib.ddmpc_debug_workspace(eng._h, b, C.c_void_p(), 0, C.c_void_p(meta.ctypes.data), n, C.c_void_p(), C.c_void_p()))
        out[b] = (meta[0], meta[1], meta[2], meta[4 + cap + rv + 2], meta[4 + cap + rv + 1])
    return out


def problem(name):
    if name == "cfg5":
        rng = np.random.default_rng(0)
        ns = n = 8; m = p = 8; Lh = 30; N = 2000
        A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
        plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.002)
        u_s = 0.1 * np.ones(m)
        y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
        return dict(n=n, m=m, p=p, L=Lh, N=N, u_s=u_s, y_s=y_s, d=generate_batch(range(B), N=N, plant=plant), box=None)
    cfg = controller_params()
    return dict(n=4, m=2, p=2, L=70, N=700, u_s=cfg["u_s"].reshape(-1), y_s=cfg["y_s"].reshape(-1), d=generate_batch(range(B), N=700),
                box=([0.0, 0.0], [2.0, 2.0]))


def buckets(us, sel, peak):
    return {"%d-%d" % (lo, lo + 31): round(float(np.median(us[sel & (peak >= lo) & (peak < lo + 32)])), 1)
            for lo in range(0, 256, 32) if np.any(sel & (peak >= lo) & (peak < lo + 32))}


ROWS = [("cfg5", "none", "input"), ("cfg5", "convex", "input"), ("tank70", "convex", "input02")]
only = [tuple(s.split(":")) for s in a.only.split(",") if s]
res = {"batch": B, "reps": a.reps, "capacity": a.capacity, "max_iter": MAX_ITER, "cases": []}
for name in ("cfg5", "tank70"):
    rows = [row for row in ROWS if row[0] == name and (not only or row in only)]
    if not rows:
        continue
    pb = problem(name)
    n, m, p, Lh, N = pb["n"], pb["m"], pb["p"], pb["L"], pb["N"]
    r = (m + p) * (Lh + n)
    ud, yd = t(pb["d"]["u_d"]), t(pb["d"]["y_d"])
    up, yp = t(pb["d"]["u_d"][:, -n:, :].reshape(B, -1)), t(pb["d"]["y_d"][:, -n:, :].reshape(B, -1))
    for _, slack, kind in rows:
        eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=3.0, R=1e-4, u_s=pb["u_s"], y_s=pb["y_s"], batch=B, controller_type=L.ROBUST,
                           slack_type=L.SLACK_CONVEX if slack == "convex" else L.SLACK_NONE, eps_max=0.002, lamb_alpha=50.0,
                           lamb_sigma=1000.0, c=1.0, device=0, max_iter=MAX_ITER)
        eng.set_large_bounds(True)
        eng.set_large_box_capacity(a.capacity)
        eng.set_data(ud, yd)
        box = pb["box"]
        if box is None:                         # from the unbounded solution (free steps: the terminal ones sit at the setpoint)
            eng.solve(up, yp)
            ub = eng.get_solution("ubar").reshape(B, Lh + n, m)[:, n:Lh]
            box = (np.minimum(np.quantile(ub, 0.005, axis=(0, 1)), pb["u_s"] - 1e-3), np.maximum(np.quantile(ub, 0.995, axis=(0, 1)), pb["u_s"] + 1e-3))
        eng.set_input_bounds(*box)
        for opt in (0, 1):
            eng.set_large_box_safeguard(bool(opt))
            o = eng.solve(up, yp)
            rec = dict(problem=name, rows=r, slack=slack, box=kind, capacity=a.capacity, option=opt,
                       bounds=[np.asarray(v, float).tolist() for v in box])
            rec["solve_ms"] = ev_ms(lambda: eng.solve(up, yp, *o))
            eng.prepare()
            o = eng.step(up, yp)
            rec["step_ms"] = ev_ms(lambda: eng.step(up, yp, *o))
            st, it = o[2].cpu().numpy(), o[3].cpu().numpy()
            kq = record(eng, r)
            peak = kq[:, 3]
            bad = st != 0
            over = bad & ((peak > a.capacity) | ((it > MAX_ITER) & (opt == 1)))
            rec["not_optimal"] = int(np.count_nonzero(bad))
            rec["beyond_capacity"] = int(np.count_nonzero(over))
            rec["at_max_iter"] = int(np.count_nonzero(bad & ~over))
            safe = ~bad & (it > MAX_ITER)
            rec["iters_below_cap"] = [int(v) for v in np.quantile(it[it < MAX_ITER], [0, 0.5, 0.9, 1.0])] if np.any(it < MAX_ITER) else []
            rec["iters_safeguarded"] = [int(v) for v in np.quantile(it[safe], [0, 0.5, 0.9, 1.0])] if np.any(safe) else []
            rec["safeguarded"] = int(np.count_nonzero(safe))
            rec["peak_active"] = [int(peak.min()), float(np.median(peak)), int(peak.max())]
            pd = ~bad & (it > 1) & (it < MAX_ITER)
            rec["us_per_primal_dual_iteration_by_peak"] = buckets(0.01 * kq[:, 4] / np.maximum(it, 1), pd, peak)
            rec["us_per_safeguard_solve_by_peak"] = buckets(0.01 * kq[:, 4] / np.maximum(it - MAX_ITER, 1), safe, peak)
            res["cases"].append(rec)
            print(json.dumps(rec), flush=True)
        eng.close()

if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
