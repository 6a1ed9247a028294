"""Dev timing (GPU): warm control steps under the CONVEX slack box with DDMPC_OPT_CONVEX_WARM_LAW off (affine iterate + filtered
cold re-solve) and on (active-set iteration on the law and M), same process, same data.  HIP-event timing, median of repeats
after warm-up.  Records ddmpc_step at 4096 and 32768 four-tank controllers (L = 30, 136 rows) on data-tail and near-setpoint
windows with the fraction that leaves the box and the mean / max number k of switched components, ddmpc_prepare, and the
4096 x 401 closed loop (1-step and 3-step); the algorithmic bytes of a warm step, 8 [(nf + 1) r + k r + nf + L m + 1], are
formed from the shapes here.

    python tools/convex_warm_time.py [--batches 4096,32768] [--reps 7]
"""
import argparse, ctypes as C, json, sys, time
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch, FOUR_TANK as P

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="4096,32768")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20, help="steps per timed repeat")
ap.add_argument("--closed-loop-batch", type=int, default=4096, help="0: no closed loop")
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("convex_warm_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

cfg = controller_params(dict(slack_var_constraint_type=1))
n, m, p, Lh, N = cfg["n"], cfg["m"], cfg["p"], cfg["L"], cfg["N"]
nch = m + p
r, nf, nbox = nch * (Lh + n), n * nch, p * Lh
dev = torch.device("cuda", 0)
res = {"r": r, "nf": nf, "nbox": nbox}


def engine(B):
    return BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                        controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=cfg["eps_max"],
                        lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"])


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


def step_bytes(k_mean):
    return 8.0 * ((nf + 1) * r + k_mean * r + nf + Lh * m + 1)


for B in [int(x) for x in a.batches.split(",")]:
    d = generate_batch(range(B), N=N)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ud, yd = t(d["u_d"]), t(d["y_d"])
    rng = np.random.default_rng(3)
    wins = {"tail": (d["u_d"][:, -n:, :].reshape(B, -1), d["y_d"][:, -n:, :].reshape(B, -1)),
            "setpoint": (np.tile(cfg["u_s"], n)[None] + 0.01 * rng.uniform(-1, 1, (B, n * m)),
                         np.tile(cfg["y_s"], n)[None] + 0.002 * rng.uniform(-1, 1, (B, n * p)))}
    for on in (False, True):
        with engine(B) as eng:
            eng.set_convex_warm_law(on)
            eng.set_data(ud, yd)
            ts = []
            for _ in range(3):                  # prepare: host-synchronous; the law is dropped by set_data
                eng.set_data(ud, yd)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.prepare()
                ts.append((time.perf_counter() - t0) * 1e3)
            res["B%d_prepare_ms_%s" % (B, "on" if on else "off")] = float(np.median(ts))
            for fam, (up, yp) in wins.items():
                upt, ypt = t(up), t(yp)
                out = eng.step(upt, ypt)
                ms = median_ms(lambda: eng.step(upt, ypt, *out), a.reps, a.inner)
                it = out[3].cpu().numpy()
                sg = eng.get_solution("sigma")[:, n * p:]
                bound = cfg["c"] * cfg["eps_max"]
                k = np.sum(np.abs(np.abs(sg) - bound) <= 1e-9 * bound, axis=1)
                key = "B%d_%s_%s" % (B, fam, "on" if on else "off")
                res[key] = dict(ms=ms, steps_per_s=B / ms * 1e3, left_box=float(np.mean(it >= 2)), iters_max=int(it.max()),
                                k_mean=float(k.mean()), k_max=int(k.max()), non_optimal=int((out[2] != 0).sum().item()),
                                GBps=B * step_bytes(float(k.mean())) / ms * 1e-6)
                print("%-22s %8.1f us  %.3e steps/s  left box %.3f  iters max %d  k mean %.2f max %d  %.0f GB/s (algorithmic)"
                      % (key, ms * 1e3, B / ms * 1e3, res[key]["left_box"], it.max(), k.mean(), k.max(), res[key]["GBps"]), flush=True)
        torch.cuda.empty_cache()
    for on in (False, True):
        print("B%d prepare %s: %.1f ms" % (B, "on " if on else "off", res["B%d_prepare_ms_%s" % (B, "on" if on else "off")]), flush=True)

# closed loop, device buffers (no host copies inside the timed region)
B, n_steps = a.closed_loop_batch, 401
d = generate_batch(range(max(B, 1)), N=N)
w = 0.002 * np.random.default_rng(1).uniform(-1, 1, (B, n_steps, p))
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
lib = L.load()
A_, B_, C_, D_ = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
pl = L.Plant(A_.shape[0], A_.ctypes.data_as(L.c_double_p), B_.ctypes.data_as(L.c_double_p), C_.ctypes.data_as(L.c_double_p),
             D_.ctypes.data_as(L.c_double_p))
for step in ((1, 3) if B > 0 else ()):
    ys = {}
    for on in (False, True):
        with engine(B) as eng:
            eng.set_convex_warm_law(on)
            eng.set_data(t(d["u_d"]), t(d["y_d"]))
            eng.prepare()
            eng._use_torch_stream()
            x0, up0, yp0 = t(d["x_end"]), t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
            wt = t(w)
            usys = torch.empty((B, n_steps, m), dtype=torch.float64, device=dev)
            ysys = torch.empty((B, n_steps, p), dtype=torch.float64, device=dev)
            st = torch.empty((B,), dtype=torch.int32, device=dev)
            bufs = {}

            def run():
                bufs["x"], bufs["u"], bufs["y"] = x0.clone(), up0.clone(), yp0.clone()
                vp = lambda z: C.c_void_p(z.data_ptr())
                L.check(lib.ddmpc_closed_loop(eng._h, C.byref(pl), n_steps, step, vp(bufs["x"]), vp(bufs["u"]), vp(bufs["y"]),
                                              vp(wt), vp(usys), vp(ysys), vp(st), L.MEM_DEVICE))
            ms = median_ms(run, max(3, a.reps // 2), 1)
            ys[on] = ysys.cpu().numpy()
            key = "closed_loop_B%d_x%d_step%d_%s" % (B, n_steps, step, "on" if on else "off")
            res[key] = dict(ms=ms, status_ok=int((st == 0).sum().item()))
            print("%-34s %8.2f ms  status ok %d / %d" % (key, ms, res[key]["status_ok"], B), flush=True)
    print("   step %d: max |y_sys(on) - y_sys(off)| = %.2e" % (step, float(np.nanmax(np.abs(ys[True] - ys[False])))), flush=True)
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
