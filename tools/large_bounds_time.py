"""Dev timing (GPU): input and output bounds on ROBUST controllers beyond 271 rows (ddmpc_rr3_box.hpp) -- an
unbounded handle against a mild input box and a mild output box, same process, same data, batch 512 at the data tail:

  cfg5    m = p = 8, n = 8, L = 30, N = 2000: 608 rows (the cfg5size_robust problem of bench.py).  The boxes are taken from the
          unbounded solution: per channel the 0.5 % / 99.5 % quantiles of its free inputs (outputs) over the batch, widened to
          contain the setpoint -- about one boxed value in a hundred starts outside.
  tank70  four-tank, L = 70, N = 700: 296 rows.  Inputs in [-4, 6]; outputs y <= (0.66, 0.775).

Per case and slack type: ddmpc_prepare, ddmpc_solve and ddmpc_step in ms by HIP events (median of --reps repeats after a warm-up
call), solves per step (min / median / max of `iters`), the peak number of active components per instance (min / median / max,
from ddmpc_debug_workspace), the position n0 where the trailing block starts, and the instances that are not optimal -- with the
reason: beyond the capacity (their peak exceeds it) or at the max_iter cap -- and the kernel's own time per iteration against the
peak number of active components (the record's ticks / iterations, median per bucket of 32 components, in us).

--capacity K sets DDMPC_OPT_LARGE_BOX_CAPACITY (64, 128, 192, 256) on every bounded handle.  --only takes a comma-separated list
of problem:slack:box rows (e.g. cfg5:convex:output,tank70:convex:input02) and runs nothing else; the box `input02` of tank70 is
u in [0, 2].

    python tools/large_bounds_time.py [--batch 512] [--reps 5] [--capacity 64] [--only rows] [--json out.json]
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
ap.add_argument("--capacity", type=int, default=64)
ap.add_argument("--only", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("large_bounds_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B = a.batch
INF = np.inf
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
    """[k, state, iterations, peak k, ticks] of every instance of the last solve (the record's stride comes from the library:
    it depends on the capacity of the kernel that wrote it)."""
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
        d = generate_batch(range(B), N=N, plant=plant)
        return dict(n=n, m=m, p=p, L=Lh, N=N, u_s=u_s, y_s=y_s, d=d, boxes=None)
    cfg = controller_params()
    d = generate_batch(range(B), N=700)
    return dict(n=4, m=2, p=2, L=70, N=700, u_s=cfg["u_s"].reshape(-1), y_s=cfg["y_s"].reshape(-1), d=d,
                boxes=dict(input=([-4.0, -4.0], [6.0, 6.0]), output=([-INF, -INF], [0.66, 0.775]), input02=([0.0, 0.0], [2.0, 2.0])))


only = [tuple(s.split(":")) for s in a.only.split(",") if s]
want = lambda *row: not only or row in only
res = {"batch": B, "reps": a.reps, "capacity": a.capacity, "cases": []}
for name in ("cfg5", "tank70"):
    if not any(want(name, s, k) for s in ("none", "convex") for k in ("unbounded", "input", "output", "input02")):
        continue
    pb = problem(name)
    n, m, p, Lh, N = pb["n"], pb["m"], pb["p"], pb["L"], pb["N"]
    r = (m + p) * (Lh + n)
    ud, yd = t(pb["d"]["u_d"]), t(pb["d"]["y_d"])
    up, yp = t(pb["d"]["u_d"][:, -n:, :].reshape(B, -1)), t(pb["d"]["y_d"][:, -n:, :].reshape(B, -1))
    for slack in ("none", "convex"):
        kinds = [k for k in ("unbounded", "input", "output") + (("input02",) if name == "tank70" else ()) if want(name, slack, k)]
        if not kinds:
            continue
        eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=3.0, R=1e-4, u_s=pb["u_s"], y_s=pb["y_s"], batch=B, controller_type=L.ROBUST,
                           slack_type=L.SLACK_CONVEX if slack == "convex" else L.SLACK_NONE, eps_max=0.002, lamb_alpha=50.0,
                           lamb_sigma=1000.0, c=1.0, device=0)
        eng.set_large_bounds(True)
        if a.capacity != 64:
            eng.set_large_box_capacity(a.capacity)
        eng.set_data(ud, yd)
        boxes = pb["boxes"]
        if boxes is None:                       # from the unbounded solution (free steps: the terminal ones sit at the setpoint)
            eng.solve(up, yp)
            ub = eng.get_solution("ubar").reshape(B, Lh + n, m)[:, n:Lh]
            yb = eng.get_solution("ybar").reshape(B, Lh + n, p)[:, n:Lh]
            q = lambda v, s, c: (np.minimum(np.quantile(v, 0.005, axis=(0, 1)), c - s), np.maximum(np.quantile(v, 0.995, axis=(0, 1)), c + s))
            boxes = dict(input=q(ub, 1e-3, pb["u_s"]), output=q(yb, 1e-3, pb["y_s"]))
        for kind in kinds:
            eng.set_input_bounds(None, None)
            eng.set_output_bounds(None, None)
            if kind in ("input", "input02"):
                eng.set_input_bounds(*boxes[kind])
            if kind == "output":
                eng.set_output_bounds(*boxes["output"])
            o = eng.solve(up, yp)
            rec = dict(problem=name, rows=r, slack=slack, box=kind, capacity=a.capacity)
            if kind != "unbounded":
                rec["bounds"] = [np.asarray(v, float).tolist() for v in boxes[kind]]
            rec["prepare_ms"] = ev_ms(lambda: (eng.set_data(ud, yd), eng.prepare()))
            rec["solve_ms"] = ev_ms(lambda: eng.solve(up, yp, *o))
            eng.prepare()
            o = eng.step(up, yp)
            rec["step_ms"] = ev_ms(lambda: eng.step(up, yp, *o))
            st, it = o[2].cpu().numpy(), o[3].cpu().numpy()
            rec["not_optimal"] = int(np.count_nonzero(st))
            rec["solves_per_step"] = [int(it.min()), float(np.median(it)), int(it.max())]
            kq = record(eng, r)
            peak = kq[:, 3] if kind != "unbounded" else kq[:, 0]
            rec["active_components"] = [int(peak.min()), float(np.median(peak)), int(peak.max())]
            if kind != "unbounded":
                bad = st != 0
                rec["beyond_capacity"] = int(np.count_nonzero(bad & (peak > a.capacity)))
                rec["at_max_iter"] = int(np.count_nonzero(bad & (peak <= a.capacity) & (it >= 50)))
                ok = ~bad & (kq[:, 2] > 1)      # (the first "iteration" of the count is the solve on the empty set)
                us = 0.01 * kq[:, 4] / np.maximum(kq[:, 2], 1)
                rec["us_per_iteration_by_peak"] = {"%d-%d" % (lo, lo + 31): round(float(np.median(us[ok & (peak >= lo) & (peak < lo + 32)])), 1)
                                                   for lo in range(0, 256, 32) if np.any(ok & (peak >= lo) & (peak < lo + 32))}
            res["cases"].append(rec)
            print(json.dumps(rec), flush=True)
        eng.close()

if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
