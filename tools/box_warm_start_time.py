"""Dev timing (GPU): DDMPC_OPT_BOX_WARM_START off / on for ROBUST controllers with input bounds -- 4096 four-tank controllers
(L = 30, 136 rows, CONVEX slack box) from the data tail, with the bounds [-4, 6], [0, 2] and [0.8, 1.2], each with
DDMPC_OPT_BOX_SAFEGUARD 0 and 1.  One handle per box, both options toggled on it (the preparation is kept), option 0 against 1
in one process.  HIP-event timing, median and spread of repeats after a warm-up.

  * ddmpc_step at the SECOND of two consecutive windows: every repeat steps at the data-tail window first (not timed; with the
    option 1 it leaves the seed), then the timed step at the window one plant step later.  That window is the same for both
    options: the plant is stepped with the inputs of the option-0 step (u_s for an instance that ended in solver_error).  Mean
    and maximum of `iters` and the instances at solver_error of that second step (`prev_window_iters_*`: of the step ahead of
    it, which with the option 1 starts from the set of the timed step of the repeat before).
  * the fused 101-step loop from the data tail; the seed is dropped before every repeat (the option is set again), so its first
    solve starts from the empty set and the set is carried from solve to solve inside the launch only.

    python tools/box_warm_start_time.py [--batch 4096] [--reps 5] [--boxes -4:6,0:2,0.8:1.2] [--json out.json]

Run with `--options 0` from a checkout of another commit's package to compare the default path.
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
ap.add_argument("--loop-steps", type=int, default=101)
ap.add_argument("--boxes", default="-4:6,0:2,0.8:1.2")
ap.add_argument("--options", default="0,1")
ap.add_argument("--safeguard", default="0,1")
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("box_warm_start_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

cfg = controller_params(dict(slack_var_constraint_type=1))
n, m, p, Lh, N = cfg["n"], cfg["m"], cfg["p"], cfg["L"], cfg["N"]
B = a.batch
dev = torch.device("cuda", 0)
res = {"batch": B}
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)


def timed_ms(fn, reps, before=lambda: None):
    """(median, min, max) ms of `fn` over `reps` repeats, `before` run ahead of each and not timed."""
    before()
    fn()                                        # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


d = generate_batch(range(500, 500 + B), N=N)
ud, yd = t(d["u_d"]), t(d["y_d"])
up1_h, yp1_h = d["u_d"][:, -n:, :].reshape(B, -1), d["y_d"][:, -n:, :].reshape(B, -1)
up1, yp1 = t(up1_h), t(yp1_h)
w_h = 0.002 * np.random.default_rng(1).uniform(-1, 1, (B, a.loop_steps, p))
w = t(w_h)
lib = L.load()
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
has_option = hasattr(BatchedDDMPC, "set_box_warm_start")
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
            x, u, y = x0.clone(), up1.clone(), yp1.clone()
            vp = lambda z: C.c_void_p(z.data_ptr())
            L.check(lib.ddmpc_closed_loop(eng._h, C.byref(pl), a.loop_steps, 1, vp(x), vp(u), vp(y), vp(w), vp(usys), vp(ysys),
                                          vp(stl), L.MEM_DEVICE))

        for safe in (int(v) for v in a.safeguard.split(",")):
            eng.set_box_safeguard(bool(safe))
            # the second window, from the option-0 step at the first
            if has_option:
                eng.set_box_warm_start(False)
            out = eng.step(up1, yp1)
            u1, st1 = out[0].cpu().numpy()[:, :m], out[2].cpu().numpy()
            u1 = np.where((st1 > 1)[:, None], np.asarray(cfg["u_s"], dtype=np.float64).reshape(1, m), u1)
            y1 = d["x_end"] @ C_.T + u1 @ D_.T + w_h[:, 0]
            up2 = t(np.concatenate([up1_h[:, m:], u1], axis=1))
            yp2 = t(np.concatenate([yp1_h[:, p:], y1], axis=1))
            out2 = [torch.empty_like(z) for z in out]
            for opt in (int(v) for v in a.options.split(",")):
                if has_option:
                    eng.set_box_warm_start(bool(opt))
                elif opt:                       # (run from a checkout without the option, to compare its option-0 rates)
                    continue
                key = "[%g,%g] safeguard %d warm_start %d" % (lo, hi, safe, opt)
                drop = (lambda: eng.set_box_warm_start(bool(opt))) if has_option else (lambda: None)
                step = timed_ms(lambda: eng.step(up2, yp2, *out2), a.reps, before=lambda: eng.step(up1, yp1, *out))
                it1, it, st = out[3].cpu().numpy(), out2[3].cpu().numpy(), out2[2].cpu().numpy()
                lp = timed_ms(loop, a.reps, before=drop)
                res[key] = dict(step_ms=step[0], step_ms_min=step[1], step_ms_max=step[2], steps_per_s=B / step[0] * 1e3,
                                prev_window_iters_mean=float(np.mean(it1)), prev_window_iters_max=int(np.max(it1)),
                                iters_mean=float(np.mean(it)), iters_max=int(np.max(it)), solver_error=int((st > 1).sum()),
                                loop_ms=lp[0], loop_ms_min=lp[1], loop_ms_max=lp[2],
                                loop_steps_per_s=B * a.loop_steps / lp[0] * 1e3, loop_kernel=eng.closed_loop_kernel_name(),
                                loop_status_ok=int((stl == 0).sum().item()), loop_solver_error=int((stl > 1).sum().item()))
                print(key, json.dumps(res[key]), flush=True)
    torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
