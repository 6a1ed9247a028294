"""Dev timing (GPU): DDMPC_OPT_BOX_SAFEGUARD off / on for ROBUST controllers with input bounds -- ddmpc_step and the fused closed
loop at 4096 four-tank controllers (L = 30, 136 rows, CONVEX slack box), data-tail windows, with the bounds [-4, 6] (few active
components), [0, 2] (k > 16) and [0.8, 1.2] (the primal-dual rule cycles on some instances: solver_error at the cap with the
option 0, the primal active set with 1), and the histogram of `iters` (max_iter + the safeguard's solves where it ran).  One
handle per box, the option toggled on it (the preparation is kept).  HIP-event timing, median and spread of repeats after warm-up.

    python tools/box_safeguard_time.py [--batch 4096] [--reps 5] [--json out.json]
"""
import argparse, ctypes as C, json, sys
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
ap.add_argument("--boxes", default="-4:6,0:2,0.8:1.2")
ap.add_argument("--options", default="0,1")
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("box_safeguard_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

cfg = controller_params(dict(slack_var_constraint_type=1))
n, m, p, Lh, N = cfg["n"], cfg["m"], cfg["p"], cfg["L"], cfg["N"]
B = a.batch
dev = torch.device("cuda", 0)
res = {"batch": B}
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def timed_ms(fn, reps, inner):
    """(median, min, max) ms per call over `reps` repeats of `inner` calls."""
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


d = generate_batch(range(500, 500 + B), N=N)
ud, yd = t(d["u_d"]), t(d["y_d"])
up, yp = t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
w = t(0.002 * np.random.default_rng(1).uniform(-1, 1, (B, a.loop_steps, p)))
lib = L.load()
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
for box in a.boxes.split(","):
    lo, hi = (float(v) for v in box.split(":"))
    with BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                      controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
                      lamb_sigma=cfg["lamb_sigma"], c=cfg["c"]) as eng:
        eng.set_input_bounds(lo, hi)
        eng.set_data(ud, yd)
        eng.prepare()
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

        for opt in (int(v) for v in a.options.split(",")):
            if hasattr(eng, "set_box_safeguard"):
                eng.set_box_safeguard(bool(opt))
            elif opt:                           # (run from a checkout without the option, to compare its option-0 rates)
                continue
            key = "[%g,%g] option %d" % (lo, hi, opt)
            out = eng.step(up, yp)
            step = timed_ms(lambda: eng.step(up, yp, *out), a.reps, a.inner)
            it, st = out[3].cpu().numpy(), out[2].cpu().numpy()
            lp = timed_ms(loop, a.reps, 1)
            hist = {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))}
            res[key] = dict(step_ms=step[0], step_ms_min=step[1], step_ms_max=step[2], steps_per_s=B / step[0] * 1e3,
                            loop_ms=lp[0], loop_ms_min=lp[1], loop_ms_max=lp[2], loop_steps_per_s=B * a.loop_steps / lp[0] * 1e3,
                            loop_kernel=eng.closed_loop_kernel_name(), loop_status_ok=int((stl == 0).sum().item()),
                            non_optimal=int((st != 0).sum()), iters_hist=hist)
            print(key, json.dumps(res[key]), flush=True)
    torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
