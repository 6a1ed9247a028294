"""Dev timing (GPU): what per-instance bounds cost on the setpoint calls -- ddmpc_step_setpoints and the fused 101-step
ddmpc_closed_loop_setpoints at 4096 four-tank controllers (L = 30, N = 400, 136 rows, data-tail windows), slack NONE
(DDMPC_OPT_SETPOINT_BOX_LAW) and the CONVEX slack box (DDMPC_OPT_SETPOINT_CONVEX_LAW), with the input boxes [-4, 6] (few active
components) and [0, 2] (k > 16), every instance at the handle's own setpoint
  * on a handle with the bounds shared by the batch (ddmpc_set_input_bounds: ddmpc_setpoint_box_step_kernel /
    ddmpc_closed_loop_setpoint_box_kernel),
  * on a handle given the same box in every row (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1, ddmpc_set_instance_input_bounds: the
    channel-table (BoxChannels) instantiations of the same two kernels, whose only extra work is the fill of two LDS arrays),
in one process, the two handles timed alternately.  ddmpc_step of the shared handle is timed next to them.  HIP-event timing
after warm-up; median with min / max over the repeats, and the per-instance / shared ratio of the medians.  The outputs of the
two handles are compared bit for bit.

    python tools/instance_setpoint_bounds_time.py [--batch 4096] [--reps 7] [--shared-only] [--json out.json]

--shared-only times the shared handle alone and uses no call newer than DDMPC_OPT_SETPOINT_CONVEX_LAW, so the same file run from
the root of a checkout of an earlier commit (its package is imported from the working directory) gives that build's figures.
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20, help="steps per timed repeat")
ap.add_argument("--loop-steps", type=int, default=101)
ap.add_argument("--shared-only", action="store_true")
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("instance_setpoint_bounds_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B = a.batch
dev = torch.device("cuda", 0)
res = {"batch": B, "reps": a.reps, "inner": a.inner, "loop_steps": a.loop_steps}
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
vp = lambda z: C.c_void_p(z.data_ptr())


def timed_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(fns, reps, inner):
    """Every function warmed up once, then timed in turn `reps` times: {name: [ms per call]}."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed_ms(fn, inner))
    return ts


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


cfg0 = controller_params()
n, m, p, Lh, N = cfg0["n"], cfg0["m"], cfg0["p"], cfg0["L"], cfg0["N"]
d = generate_batch(range(500, 500 + B), N=N)
ud, yd = t(d["u_d"]), t(d["y_d"])
up, yp = t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
w = t(0.002 * np.random.default_rng(1).uniform(-1, 1, (B, a.loop_steps, p)))
x0 = t(d["x_end"])
us, ys = t(np.tile(cfg0["u_s"], (B, 1))), t(np.tile(cfg0["y_s"], (B, 1)))                    # every row at the handle's own setpoint
uref, yref = t(np.tile(cfg0["u_s"], (B, a.loop_steps, 1))), t(np.tile(cfg0["y_s"], (B, a.loop_steps, 1)))
lib = L.load()
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
kinds = ("shared",) if a.shared_only else ("shared", "instance")


def engine(cfg, convex):
    return BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                        controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if convex else L.SLACK_NONE, eps_max=cfg["eps_max"],
                        lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"])


for convex in (False, True):
    cfg = controller_params(dict(slack_var_constraint_type=1 if convex else 0))
    for lo, hi in ((-4.0, 6.0), (0.0, 2.0)):
        key = "%s [%g,%g]" % ("convex" if convex else "none", lo, hi)
        engs, outs, souts, loops, bufs = {}, {}, {}, {}, {}
        try:
            for kind in kinds:
                eng = engs[kind] = engine(cfg, convex)
                if kind == "shared":
                    eng.set_input_bounds(lo, hi)
                else:
                    eng.set_instance_setpoint_bounds(True)
                    eng.set_instance_input_bounds(np.full((B, m), lo), np.full((B, m), hi))
                (eng.set_setpoint_convex_law if convex else eng.set_setpoint_box_law)(True)
                eng.set_data(ud, yd)
                eng.prepare()
                souts[kind] = eng.step(up, yp)
                outs[kind] = eng.step_setpoints(up, yp, us, ys)
                eng._use_torch_stream()
                bufs[kind] = (torch.empty((B, a.loop_steps, m), dtype=torch.float64, device=dev),
                              torch.empty((B, a.loop_steps, p), dtype=torch.float64, device=dev),
                              torch.empty((B,), dtype=torch.int32, device=dev))

                def loop(eng=eng, buf=bufs[kind]):
                    x, u, y = x0.clone(), up.clone(), yp.clone()
                    L.check(lib.ddmpc_closed_loop_setpoints(eng._h, C.byref(pl), a.loop_steps, 1, vp(x), vp(u), vp(y), vp(w), vp(uref),
                                                            vp(yref), vp(buf[0]), vp(buf[1]), vp(buf[2]), L.MEM_DEVICE))
                loops[kind] = loop
            fns = {k: (lambda k=k: engs[k].step_setpoints(up, yp, us, ys, *outs[k])) for k in kinds}
            fns["shared ddmpc_step"] = lambda: engs["shared"].step(up, yp, *souts["shared"])
            step_ts = alternate(fns, a.reps, a.inner)
            loop_ts = alternate(loops, a.reps, 1)
            r = {"ddmpc_step_shared": stats(step_ts["shared ddmpc_step"])}
            for kind in kinds:
                it, st = outs[kind][3].cpu().numpy(), outs[kind][2].cpu().numpy()
                r[kind] = dict(step=stats(step_ts[kind]), loop=stats(loop_ts[kind]), loop_kernel=engs[kind].closed_loop_kernel_name(),
                               non_optimal=int((st != 0).sum()), loop_status_ok=int((bufs[kind][2] == 0).sum().item()),
                               iters_hist={int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))})
            if len(kinds) == 2:
                r["step_ratio"] = r["instance"]["step"]["median_ms"] / r["shared"]["step"]["median_ms"]
                r["loop_ratio"] = r["instance"]["loop"]["median_ms"] / r["shared"]["loop"]["median_ms"]
                r["bit_equal"] = bool(all(torch.equal(x, y) for x, y in zip(outs["shared"], outs["instance"])) and
                                      all(torch.equal(x.nan_to_num(nan=-1.0), y.nan_to_num(nan=-1.0)) for x, y in
                                          zip(bufs["shared"][:2], bufs["instance"][:2])))
            res[key] = r
            print(key, json.dumps(r), flush=True)
        finally:
            for eng in engs.values():
                eng.close()
        torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
