"""Dev timing (GPU): DDMPC_OPT_SETPOINT_CONVEX_LAW on four-tank controllers with the CONVEX slack box (L = 30, N = 400, 136 rows;
the setpoint calls run the SLACK instantiations of ddmpc_setpoint_box_step_kernel / ddmpc_closed_loop_setpoint_box_kernel), HIP events, median of `--reps` repeats, the compared versions alternating in one process after a warm-up of every version.
Per case (slack-only; u in [-4, 6]: few active inputs; u in [0, 2]: 30 .. 50 of them) and batch:

  * ddmpc_step with the option 0 -- twice, as two entries of the alternation: their difference is the run-to-run spread -- and
    with the option 1 (the unchanged path), against ddmpc_step_setpoints at the handle's own setpoints (the same problems, the
    same active sets) and at per-instance setpoints.  DDMPC_OPT_CONVEX_WARM_LAW is on on every handle: on the slack-only one
    ddmpc_step then iterates on the law and M as the new step does; a bounded handle always does;
  * the sequence the new step replaces, ddmpc_set_setpoints + ddmpc_prepare + ddmpc_step, against ddmpc_step_setpoints;
  * ddmpc_prepare with the option 0 and 1 (the preparation is forgotten before every call);
  * the 101-step fused loops, ddmpc_closed_loop against ddmpc_closed_loop_setpoints.

    python tools/setpoint_convex_law_time.py [--batches 4096] [--reps 5] [--json out.json]
"""
import argparse, ctypes as C, json, sys
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch, FOUR_TANK as P

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=20, help="steps per timed repeat")
ap.add_argument("--json", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("setpoint_convex_law_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

cfg = controller_params(dict(slack_var_constraint_type=1))
n, m, p, Lh, N = cfg["n"], cfg["m"], cfg["p"], cfg["L"], cfg["N"]
nch, n_steps = m + p, 101
res = {"r": nch * (Lh + n), "nf": n * nch}
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
vp = lambda z: C.c_void_p(z.data_ptr())
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
BOXES = {"slack-only": None, "[-4,6]": (-4.0, 6.0), "[0,2]": (0.0, 2.0)}
REFINE_RES_DEFAULT = 107                       # (DDMPC_REFINE_RES_DEFAULT: setting it changes nothing but forgets the preparation)


def engine(B, option, box):
    eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                       controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
                       lamb_sigma=cfg["lamb_sigma"], c=cfg["c"])
    eng.set_convex_warm_law(True)
    eng.set_setpoint_convex_law(option)
    if box is not None:
        eng.set_input_bounds(*box)
    return eng


def alternate(fns, reps, inner):
    """{name: (median, min, max) ms per call}: every version once for warm-up, then `reps` rounds that time each version in turn."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def report(B, tag, out):
    for k, (med, lo, hi) in out.items():
        res["B%d_%s_%s" % (B, tag, k)] = dict(ms=med, min_ms=lo, max_ms=hi)
        print("B%-6d %-20s %-36s %10.1f us   (min %.1f, max %.1f)" % (B, tag, k, med * 1e3, lo * 1e3, hi * 1e3), flush=True)


for B in [int(x) for x in a.batches.split(",")]:
    d = generate_batch(range(B), N=N)
    ud, yd = t(d["u_d"]), t(d["y_d"])
    up, yp = t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
    rng = np.random.default_rng(4)
    us = t(np.asarray(cfg["u_s"]) + rng.uniform(-0.5, 0.5, (B, m)))
    ys = t(np.asarray(cfg["y_s"]) + rng.uniform(-0.2, 0.2, (B, p)))
    us2, ys2 = np.asarray(cfg["u_s"]) + 0.1, np.asarray(cfg["y_s"]) + 0.05
    us_own, ys_own = t(np.tile(cfg["u_s"], (B, 1))), t(np.tile(cfg["y_s"], (B, 1)))      # the handle's setpoints: ddmpc_step's problem
    for name, box in BOXES.items():
        with engine(B, False, box) as e0, engine(B, True, box) as e1:
            for e in (e0, e1):
                e.set_data(ud, yd)
                e.prepare()
            out0, out1 = e0.step(up, yp), e1.step(up, yp)
            for tag, (s_u, s_y) in (("handle's s", (us_own, ys_own)), ("per-instance s", (us, ys))):
                _, _, st, its = e1.step_setpoints(up, yp, s_u, s_y)
                torch.cuda.synchronize()
                its, st = torch.as_tensor(its), torch.as_tensor(st)
                res["B%d_%s_iters_%s" % (B, name, tag)] = dict(mean=float(its.double().mean()), max=int(its.max()), not_optimal=int((st > 1).sum()))
                print("B%-6d %-20s iters of ddmpc_step_setpoints (%s): mean %.2f max %d, not optimal: %d" %
                      (B, name, tag, float(its.double().mean()), int(its.max()), int((st > 1).sum())))
            flip = [0]

            def reprepare():                    # without the option: new tables, new factor, new law and M, then the step
                flip[0] ^= 1
                e0.set_setpoints(us2 if flip[0] else cfg["u_s"], ys2 if flip[0] else cfg["y_s"])
                e0.step(up, yp, *out0)

            def prepare(e):                     # ddmpc_prepare alone: the preparation forgotten by an option write that changes nothing
                L.check(lib.ddmpc_set_option(e._h, L.OPT_REFINE_RES_LOG10, REFINE_RES_DEFAULT))
                e.prepare()

            report(B, "step " + name, alternate({
                "ddmpc_step opt 0": lambda: e0.step(up, yp, *out0),
                "ddmpc_step opt 0 (again)": lambda: e0.step(up, yp, *out0),
                "ddmpc_step opt 1": lambda: e1.step(up, yp, *out1),
                "ddmpc_step_setpoints (handle's s)": lambda: e1.step_setpoints(up, yp, us_own, ys_own, *out1),
                "ddmpc_step_setpoints": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
            }, a.reps, a.inner))
            report(B, "change " + name, alternate({
                "set_setpoints + prepare + step": reprepare,
                "ddmpc_step_setpoints": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
            }, a.reps, 1))
            if flip[0]:
                e0.set_setpoints(cfg["u_s"], cfg["y_s"])
            report(B, "prepare " + name, alternate({
                "ddmpc_prepare opt 0": lambda: prepare(e0),
                "ddmpc_prepare opt 1": lambda: prepare(e1),
            }, a.reps, 1))
            # the 101-step fused loops on device buffers
            w = t(cfg["eps_max"] * np.random.default_rng(1).uniform(-1, 1, (B, n_steps, p)))
            x0 = t(d["x_end"])
            uref, yref = us[:, None, :].repeat(1, n_steps, 1).contiguous(), ys[:, None, :].repeat(1, n_steps, 1).contiguous()
            uown, yown = us_own[:, None, :].repeat(1, n_steps, 1).contiguous(), ys_own[:, None, :].repeat(1, n_steps, 1).contiguous()
            usys = torch.empty((B, n_steps, m), dtype=torch.float64, device=dev)
            ysys = torch.empty((B, n_steps, p), dtype=torch.float64, device=dev)
            st = torch.empty((B,), dtype=torch.int32, device=dev)

            def loop(e, ref):
                x, u, y = x0.clone(), up.clone(), yp.clone()
                e._use_torch_stream()
                if ref:
                    L.check(lib.ddmpc_closed_loop_setpoints(e._h, C.byref(pl), n_steps, 1, vp(x), vp(u), vp(y), vp(w), vp(ref[0]),
                                                            vp(ref[1]), vp(usys), vp(ysys), vp(st), L.MEM_DEVICE))
                else:
                    L.check(lib.ddmpc_closed_loop(e._h, C.byref(pl), n_steps, 1, vp(x), vp(u), vp(y), vp(w), vp(usys), vp(ysys),
                                                  vp(st), L.MEM_DEVICE))

            report(B, "loop101 " + name, alternate({
                "ddmpc_closed_loop opt 0": lambda: loop(e0, False),
                "ddmpc_closed_loop opt 1": lambda: loop(e1, False),
                "closed_loop_setpoints (handle's s)": lambda: loop(e1, (uown, yown)),
                "ddmpc_closed_loop_setpoints": lambda: loop(e1, (uref, yref)),
            }, a.reps, 1))
            res["B%d_%s_loop_kernels" % (B, name)] = []
            for tag, ref in (("closed_loop", None), ("closed_loop_setpoints (handle's s)", (uown, yown)), ("closed_loop_setpoints", (uref, yref))):
                loop(e1, ref)                   # (a stopped instance makes no further solves in the setpoint loop: count them)
                torch.cuda.synchronize()
                res["B%d_%s_stopped_%s" % (B, name, tag)] = int((st > 1).sum())
                res["B%d_%s_loop_kernels" % (B, name)].append(e1.closed_loop_kernel_name())
                print("B%-6d %-20s %-36s %s, stopped instances: %d" % (B, name, tag, e1.closed_loop_kernel_name(), int((st > 1).sum())), flush=True)
    del ud, yd
    torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
