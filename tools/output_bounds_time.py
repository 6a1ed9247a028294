"""Dev timing (GPU): ROBUST controllers with output bounds (ddmpc_set_output_bounds) -- ddmpc_prepare, ddmpc_step, ddmpc_solve
and the fused closed loop at 4096 four-tank controllers (L = 30, 136 rows, CONVEX slack box with the terminal constraint: 112
boxed components on 60 columns of M) with the boxes `mild-upper` (y <= 0.66, 0.775: few active components, the k x k system stays
in LDS) and `two-sided` ([0.60, 0.70] x [0.72, 0.82]: k > 16, the instance's global slice), data-tail windows, with the histogram
of active-set solves.  HIP-event timing, median of repeats after warm-up.  The closed loop runs the box along 101 steps of a
noisy plant; instances on which it becomes infeasible there end non-optimal and are counted (loop_status_ok).

    python tools/output_bounds_time.py [--batch 4096] [--reps 5] [--json out.json]
"""
import argparse, ctypes as C, json, sys, time
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch, FOUR_TANK as P

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=10, help="steps per timed repeat")
ap.add_argument("--loop-steps", type=int, default=101)
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("output_bounds_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

cfg = controller_params(dict(slack_var_constraint_type=1))
n, m, p, Lh, N = cfg["n"], cfg["m"], cfg["p"], cfg["L"], cfg["N"]
B = a.batch
dev = torch.device("cuda", 0)
res = {"batch": B}
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def median_ms(fn, reps, inner):
    fn()                                        # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ts))


d = generate_batch(range(500, 500 + B), N=N)
ud, yd = t(d["u_d"]), t(d["y_d"])
up, yp = t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
w = t(0.002 * np.random.default_rng(1).uniform(-1, 1, (B, a.loop_steps, p)))
lib = L.load()
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
INF = float("inf")
for key, lo, hi in (("mild-upper", [-INF, -INF], [0.66, 0.775]), ("two-sided", [0.60, 0.72], [0.70, 0.82])):
    with BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                      controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
                      lamb_sigma=cfg["lamb_sigma"], c=cfg["c"]) as eng:
        eng.set_output_bounds(lo, hi)
        ts = []
        for _ in range(3):                      # prepare: host-synchronous; the law is dropped by set_data
            eng.set_data(ud, yd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.prepare()
            ts.append((time.perf_counter() - t0) * 1e3)
        out = eng.step(up, yp)
        step_ms = median_ms(lambda: eng.step(up, yp, *out), a.reps, a.inner)
        it, st = out[3].cpu().numpy(), out[2].cpu().numpy()
        solve_ms = median_ms(lambda: eng.solve(up, yp, *out), max(2, a.reps // 2), 1)
        eng._use_torch_stream()
        usys = torch.empty((B, a.loop_steps, m), dtype=torch.float64, device=dev)
        ysys = torch.empty((B, a.loop_steps, p), dtype=torch.float64, device=dev)
        stl = torch.empty((B,), dtype=torch.int32, device=dev)
        x0 = t(d["x_end"])

        def loop():
            x, u, y = x0.clone(), up.clone(), yp.clone()
            vp = lambda z: C.c_void_p(z.data_ptr())
            L.check(lib.ddmpc_closed_loop(eng._h, C.byref(pl), a.loop_steps, 1, vp(x), vp(u), vp(y), vp(w), vp(usys), vp(ysys),
                                          vp(stl), L.MEM_DEVICE))
        loop_ms = median_ms(loop, max(2, a.reps // 2), 1)
        hist = {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))}
        res[key] = dict(prepare_ms=float(np.median(ts)), step_ms=step_ms, steps_per_s=B / step_ms * 1e3, solve_ms=solve_ms,
                        solves_per_s=B / solve_ms * 1e3, loop_ms=loop_ms, loop_steps_per_s=B * a.loop_steps / loop_ms * 1e3,
                        loop_kernel=eng.closed_loop_kernel_name(), loop_status_ok=int((stl == 0).sum().item()),
                        non_optimal=int((st != 0).sum()), iters_hist=hist)
        print(key, json.dumps(res[key]), flush=True)
    torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
