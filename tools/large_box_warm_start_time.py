"""Dev timing (GPU): DDMPC_OPT_LARGE_BOX_WARM_START 0 against 1 on bounded ROBUST controllers beyond 271 rows (the seeded
instantiation of rr3_solve_box_wide_kernel, ddmpc_rr3_box_wide.hpp, DESIGN 5.5.2 "Warm start"), batch 512, max_iter 50, both
option values on one handle in one process:

  tank70:convex:0:2:128:0       four-tank, L = 70, 296 rows, u in [0, 2], CONVEX, capacity 128
  tank70:none:0.9:1.1:192:0/1   u in [0.9, 1.1], slack NONE, capacity 192, without / with DDMPC_OPT_LARGE_BOX_SAFEGUARD
  tank70:convex:-4:6:128:0      the wide box
  cfg5:none/convex:q:q:128:1    the cfg-5-size input box of tools/large_bounds_time.py (608 rows), with the safeguard

Per configuration and option value:
  * ddmpc_step at the SECOND of two consecutive windows (the data tail, then the window behind one plant step with the first
    optimal input and noise eps_max U(-1, 1)): every repeat runs the step at the first window untimed -- it leaves the seed --
    and times the step at the second by HIP events; median of --reps repeats with min - max, `iters` mean / max and the
    instances that are not optimal at that step;
  * a per-step ddmpc_closed_loop of --steps steps (host arrays in and out, the same for both values), HIP events likewise,
    with the instances that stopped.

    python tools/large_box_warm_start_time.py [--batch 512] [--reps 5] [--steps 20] [--only rows] [--json out.json]
"""
import argparse, json, sys
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch
from oracle import ddmpc_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--json", default="")
ap.add_argument("--only", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("large_box_warm_start_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B, MAX_ITER = a.batch, 50
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def ev_ms(before, fn):
    """[median, min, max] ms of fn by HIP events over the repeats; `before` runs untimed ahead of every call of fn."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    before(); fn()                               # warm-up: allocations, LDS attributes
    out = []
    for _ in range(a.reps):
        before()
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return [round(float(np.median(out)), 4), round(float(np.min(out)), 4), round(float(np.max(out)), 4)]


def problem(name):
    if name == "cfg5":
        rng = np.random.default_rng(0)
        ns = n = 8; m = p = 8; Lh = 30; N = 2000
        A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
        plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.002)
        u_s = 0.1 * np.ones(m)
        y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
        return dict(n=n, m=m, p=p, L=Lh, N=N, u_s=u_s, y_s=y_s, d=generate_batch(range(B), N=N, plant=plant), plant=plant)
    cfg = controller_params()
    return dict(n=4, m=2, p=2, L=70, N=700, u_s=cfg["u_s"].reshape(-1), y_s=cfg["y_s"].reshape(-1), d=generate_batch(range(B), N=700),
                plant=orc.FOUR_TANK)


# (problem, slack, lower, upper, capacity, DDMPC_OPT_LARGE_BOX_SAFEGUARD); "q": the quantile box of the unbounded solution
ROWS = [("tank70", "convex", "0", "2", 128, 0), ("tank70", "none", "0.9", "1.1", 192, 0), ("tank70", "none", "0.9", "1.1", 192, 1),
        ("tank70", "convex", "-4", "6", 128, 0), ("cfg5", "none", "q", "q", 128, 1), ("cfg5", "convex", "q", "q", 128, 1)]
only = [s for s in a.only.split(",") if s]
res = {"batch": B, "reps": a.reps, "steps": a.steps, "max_iter": MAX_ITER, "cases": []}
for name in ("tank70", "cfg5"):
    rows = [row for row in ROWS if row[0] == name and (not only or ":".join(str(v) for v in row) in only)]
    if not rows:
        continue
    pb = problem(name)
    n, m, p, Lh, N, P = pb["n"], pb["m"], pb["p"], pb["L"], pb["N"], pb["plant"]
    r = (m + p) * (Lh + n)
    d = pb["d"]
    ud, yd = t(d["u_d"]), t(d["y_d"])
    up0, yp0 = d["u_d"][:, -n:, :].reshape(B, -1).copy(), d["y_d"][:, -n:, :].reshape(B, -1).copy()
    rng = np.random.default_rng(77)
    w = P["eps_max"] * rng.uniform(-1.0, 1.0, (B, a.steps, p))
    for _, slack, lo, hi, cap, safe in rows:
        eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=3.0, R=1e-4, u_s=pb["u_s"], y_s=pb["y_s"], batch=B, controller_type=L.ROBUST,
                           slack_type=L.SLACK_CONVEX if slack == "convex" else L.SLACK_NONE, eps_max=0.002, lamb_alpha=50.0,
                           lamb_sigma=1000.0, c=1.0, device=0, max_iter=MAX_ITER)
        eng.set_large_bounds(True)
        eng.set_large_box_capacity(cap)
        eng.set_large_box_safeguard(bool(safe))
        eng.set_data(ud, yd)
        if lo == "q":                           # from the unbounded solution (free steps: the terminal ones sit at the setpoint)
            eng.solve(t(up0), t(yp0))
            ub = eng.get_solution("ubar").reshape(B, Lh + n, m)[:, n:Lh]
            box = (np.minimum(np.quantile(ub, 0.005, axis=(0, 1)), pb["u_s"] - 1e-3), np.maximum(np.quantile(ub, 0.995, axis=(0, 1)), pb["u_s"] + 1e-3))
        else:
            box = (np.full(m, float(lo)), np.full(m, float(hi)))
        eng.set_input_bounds(*box)
        eng.prepare()
        # the second window: one plant step with the first optimal input (the option off; an instance that is not optimal
        # there keeps its first window)
        o = eng.step(t(up0), t(yp0))
        u0, st0 = o[0].cpu().numpy()[:, :m], o[2].cpu().numpy()
        ok0 = st0 == 0
        u0 = np.where(ok0[:, None], u0, up0[:, -m:])
        y0 = np.einsum("ij,bj->bi", P["C"], d["x_end"]) + np.einsum("ij,bj->bi", P["D"], u0) + w[:, 0]
        up1 = np.where(ok0[:, None], np.concatenate([up0[:, m:], u0], axis=1), up0)
        yp1 = np.where(ok0[:, None], np.concatenate([yp0[:, p:], y0], axis=1), yp0)
        W0, W1 = (t(up0), t(yp0)), (t(up1), t(yp1))
        for opt in (0, 1):
            eng.set_large_box_warm_start(bool(opt))
            rec = dict(problem=name, rows=r, slack=slack, box=[lo, hi], capacity=cap, safeguard=safe, option=opt,
                       bounds=[np.asarray(v, float).tolist() for v in box], not_optimal_first_window=int(np.count_nonzero(~ok0)))
            o = eng.step(*W0)
            o = eng.step(*W1)
            rec["step_ms"] = ev_ms(lambda: eng.step(*W0, *o), lambda: eng.step(*W1, *o))
            st, it = o[2].cpu().numpy(), o[3].cpu().numpy()
            rec["iters_mean"], rec["iters_max"] = round(float(np.mean(it)), 2), int(np.max(it))
            rec["not_optimal"] = int(np.count_nonzero(st != 0))
            out = []
            # (setting the option again drops the seed: every repeat of the loop starts its first step from the empty set)
            rec["loop_ms"] = ev_ms(lambda: eng.set_large_box_warm_start(bool(opt)), lambda: out.append(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up0, yp0, w)))
            rec["loop_stopped"] = int(np.count_nonzero(out[-1][2] != 0))
            res["cases"].append(rec)
            print(json.dumps(rec), flush=True)
        eng.close()

if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
