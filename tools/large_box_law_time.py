"""Dev timing (GPU): DDMPC_OPT_LARGE_BOX_LAW 0 against 1 on bounded ROBUST controllers beyond 271 rows (rr3_law_box_step_kernel,
ddmpc_rr3_box_law.hpp, DESIGN 5.5.2 "Law inside the box"), batch 512, both values on one handle:

  tank70  four-tank, L = 70, N = 700: 296 rows, CONVEX slack.  Inputs in [0, 2] (capacity 128) and in [-4, 6] (capacity 64).
  cfg5    m = p = 8, n = 8, L = 30, N = 2000: 608 rows, CONVEX slack, capacity 64.  The input box and the output box of
          tools/large_bounds_time.py: per channel the 0.5 % / 99.5 % quantiles of the unbounded solution's free inputs (outputs)
          over the batch at the data tail, widened to contain the setpoint.  Under DDMPC_REFINE_AUTO no law of this size reaches the
          refinement threshold: every instance is "no law" and every step the filtered re-solve, so the rows of this
          problem are timed under DDMPC_REFINE_OFF too, where the law serves.

Windows: four families with 0, 1/8, 1/2 and all of the instances on the data tail (the first ones of the batch), the others near
the setpoint (offsets 1e-3, seed 0).  Per row and family, for the option 0 and 1: ddmpc_step in ms, the instances with
iters = 1, the mean of iters and the instances that are not optimal; the instances the law served (their inputs differ from
the option 0's in some bit: a re-solved instance is bit-equal to it) and the largest relative difference of the inputs.  Per row:
ddmpc_prepare with 0 and 1, the law's memory, and a per-step closed loop of --steps steps from the data tail.  HIP events,
[median, min, max] over --reps repeats after a warm-up call.

    python tools/large_box_law_time.py [--batch 512] [--reps 5] [--steps 20] [--only rows] [--json out.json]
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
    raise SystemExit("large_box_law_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B, INF = a.batch, np.inf
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


# (problem, box, capacity, refinement); "q": the quantile box of the unbounded solution
ROWS = [("tank70", "input02", 128, "auto"), ("tank70", "input", 64, "auto"), ("cfg5", "input", 64, "auto"), ("cfg5", "output", 64, "auto"),
        ("cfg5", "input", 64, "off"), ("cfg5", "output", 64, "off")]
FAMILIES = (("none", 0), ("eighth", B // 8), ("half", B // 2), ("all", B))     # instances on the data tail
only = [s for s in a.only.split(",") if s]
res = {"batch": B, "reps": a.reps, "steps": a.steps, "cases": []}
for name in ("tank70", "cfg5"):
    rows = [row for row in ROWS if row[0] == name and (not only or ":".join(str(v) for v in row) in only)]
    if not rows:
        continue
    pb = problem(name)
    n, m, p, Lh, N, P = pb["n"], pb["m"], pb["p"], pb["L"], pb["N"], pb["plant"]
    r, nf = (m + p) * (Lh + n), n * (m + p)
    d = pb["d"]
    ud, yd = t(d["u_d"]), t(d["y_d"])
    up0, yp0 = d["u_d"][:, -n:, :].reshape(B, -1).copy(), d["y_d"][:, -n:, :].reshape(B, -1).copy()
    rng = np.random.default_rng(0)
    ups = np.tile(pb["u_s"], n)[None, :] + 1e-3 * rng.standard_normal((B, n * m))
    yps = np.tile(pb["y_s"], n)[None, :] + 1e-3 * rng.standard_normal((B, n * p))
    w = P["eps_max"] * np.random.default_rng(77).uniform(-1.0, 1.0, (B, a.steps, p))
    for _, kind, cap, refine in rows:
        eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=3.0, R=1e-4, u_s=pb["u_s"], y_s=pb["y_s"], batch=B, controller_type=L.ROBUST,
                           slack_type=L.SLACK_CONVEX, eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0, device=0)
        eng.set_large_bounds(True)
        eng.set_refinement(refine)
        if cap != 64:
            eng.set_large_box_capacity(cap)
        eng.set_data(ud, yd)
        if name == "cfg5":                      # from the unbounded solution (free steps: the terminal ones sit at the setpoint)
            eng.solve(t(up0), t(yp0))
            sel = "ubar" if kind == "input" else "ybar"
            v = eng.get_solution(sel).reshape(B, Lh + n, -1)[:, n:Lh]
            c = pb["u_s"] if kind == "input" else pb["y_s"]
            box = (np.minimum(np.quantile(v, 0.005, axis=(0, 1)), c - 1e-3), np.maximum(np.quantile(v, 0.995, axis=(0, 1)), c + 1e-3))
        else:
            box = dict(input=([-4.0, -4.0], [6.0, 6.0]), input02=([0.0, 0.0], [2.0, 2.0]))[kind]
        (eng.set_output_bounds if kind == "output" else eng.set_input_bounds)(*box)
        rec = dict(problem=name, rows=r, box=kind, capacity=cap, refine=refine, bounds=[np.asarray(v, float).tolist() for v in box],
                   law_bytes_per_instance=8 * (nf + 1) * r, families={})
        for opt in (0, 1):
            rec["prepare_ms_%d" % opt] = ev_ms(lambda: eng.set_large_box_law(bool(opt)), lambda: eng.prepare())
        for fam, ntail in FAMILIES:
            up, yp = ups.copy(), yps.copy()
            up[:ntail], yp[:ntail] = up0[:ntail], yp0[:ntail]
            W = (t(up), t(yp))
            f = {"on_the_tail": ntail}
            for opt in (0, 1):
                eng.set_large_box_law(bool(opt))
                eng.prepare()
                o = eng.step(*W)
                f["step_ms_%d" % opt] = ev_ms(lambda: None, lambda: eng.step(*W, *o))
                st, it = o[2].cpu().numpy(), o[3].cpu().numpy()
                f["iters_1_%d" % opt] = int(np.count_nonzero((it == 1) & (st == 0)))
                f["iters_mean_%d" % opt] = round(float(np.mean(it)), 2)
                f["not_optimal_%d" % opt] = int(np.count_nonzero(st != 0))
                f["u_%d" % opt] = o[0].cpu().numpy().copy()
            same = np.all(f["u_0"] == f["u_1"], axis=1) | np.all(np.isnan(f["u_0"]) & np.isnan(f["u_1"]), axis=1)
            f["served_by_the_law"] = int(np.count_nonzero(~same))          # (a re-solved instance is bit-equal to the option 0)
            ok = np.isfinite(f["u_0"]).all(axis=1) & np.isfinite(f["u_1"]).all(axis=1)
            f["max_rel_diff"] = float(np.max(np.abs(f["u_1"][ok] - f["u_0"][ok])) / np.max(np.abs(f["u_0"][ok]))) if ok.any() else None
            del f["u_0"], f["u_1"]
            rec["families"][fam] = f
        for opt in (0, 1):
            out = []
            eng.set_large_box_law(bool(opt))
            eng.prepare()
            rec["loop_ms_%d" % opt] = ev_ms(lambda: None, lambda: out.append(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up0, yp0, w)))
            rec["loop_stopped_%d" % opt] = int(np.count_nonzero(out[-1][2] != 0))
        res["cases"].append(rec)
        print(json.dumps(rec), flush=True)
        eng.close()

if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
