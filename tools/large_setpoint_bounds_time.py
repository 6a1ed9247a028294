"""Dev timing (GPU): DDMPC_OPT_LARGE_SETPOINT_BOUNDS -- per-instance setpoints on bounded handles beyond 271 rows.
The four-tank plant at L = 70, N = 700 (296 rows) and the 8 x 8-channel size (608 rows, N = 2000), batch 512, slack NONE and
CONVEX.  HIP events, median / min / max of `--reps` repeats, the compared versions alternating in one process after a warm-up
of every version.  Boxes: u in [-4, 6] (default capacity), u in [0, 2] at capacity 128, one output box (y_s +- 0.2 per channel).
Per size, slack and box:

  * ddmpc_step with the option 0 -- twice, as two entries of the alternation: their difference is the run-to-run spread, the
    margin for every comparison below -- and with the option 1;
  * ddmpc_step_setpoints at the handle's own setpoints (the same problems as ddmpc_step) and at per-instance setpoints;
  * the sequence the new call replaces: ddmpc_set_setpoints + ddmpc_prepare + ddmpc_step;
  * ddmpc_solve with the option 0 (twice) and 1.

`--only-existing` times ddmpc_step / ddmpc_solve with the option 0 alone and takes no option-22 call: that part also runs on a
build of the parent commit, and two such runs (`--json` each) are the comparison of the existing calls across the two builds.

Per-instance setpoints: u_s +- 0.5, y_s +- 0.2 with rng(11) on the four-tank under slack NONE; elsewhere the equilibria
a_b (u_s, y_s), a_b in [0.5, 1.5] (any other setpoint binds the terminal slacks under CONVEX).  Statuses and iteration counts of
every timed setpoint step are reported next to its time: an instance beyond the capacity ends early and costs less.

    python tools/large_setpoint_bounds_time.py [--batch 512] [--reps 5] [--sizes 296,608] [--only-existing] [--json out.json]
"""
import argparse, json, sys
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=5, help="calls per timed repeat")
ap.add_argument("--sizes", default="296,608")
ap.add_argument("--only-existing", action="store_true")
ap.add_argument("--json", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("large_setpoint_bounds_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
res = {}


def case(size, slack, B):
    if size == 296:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=70)
        if slack == "convex":
            spec.c = 0.05
        N, plant = 700, None
    else:
        rng = np.random.default_rng(0)
        ns = n = 8; m = p = 8
        A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
        plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.002)
        u_s = 0.1 * np.ones(m)
        y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
        spec = orc.QPSpec(n=n, m=m, p=p, L=30, Q=3.0 * np.eye(p * 30), R=1e-4 * np.eye(m * 30), u_s=u_s, y_s=y_s, robust=True,
                          eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0, slack=slack, tec=True)
        N = 2000
    d = harness.generate_batch(range(B), N=N) if plant is None else harness.generate_batch(range(B), N=N, plant=plant)
    return spec, N, d


def engine(spec, N, B, option, box, cap):
    eng = BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                       controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if spec.slack == "convex" else L.SLACK_NONE,
                       eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c,
                       use_terminal_constraint=spec.tec)
    eng.set_large_bounds(True)
    eng.set_large_box_capacity(cap)
    if option:
        eng.set_large_setpoint_bounds(True)
    kind, lo, hi = box
    (eng.set_input_bounds if kind == "u" else eng.set_output_bounds)(lo, hi)
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


def report(tag, out):
    for k, (med, lo, hi) in out.items():
        res["%s | %s" % (tag, k)] = dict(ms=med, min_ms=lo, max_ms=hi)
        print("%-30s %-44s %9.1f us   (min %.1f, max %.1f)" % (tag, k, med * 1e3, lo * 1e3, hi * 1e3), flush=True)


def counts(tag, what, out):
    st, it = torch.as_tensor(out[2]), torch.as_tensor(out[3])
    e = dict(iters_mean=float(it.double().mean()), iters_max=int(it.max()), not_optimal=int((st > 1).sum()))
    res["%s | %s counts" % (tag, what)] = e
    print("%-30s %-44s iters mean %.2f max %d, not optimal %d of %d" % (tag, what, e["iters_mean"], e["iters_max"], e["not_optimal"], st.numel()),
          flush=True)


B = a.batch
for size in [int(x) for x in a.sizes.split(",")]:
    for slack in ("none", "convex"):
        spec, N, d = case(size, slack, B)
        n, m, p = spec.n, spec.m, spec.p
        ud, yd = t(d["u_d"]), t(d["y_d"])
        up, yp = t(d["u_d"][:, -n:, :].reshape(B, -1)), t(d["y_d"][:, -n:, :].reshape(B, -1))
        rng = np.random.default_rng(11)
        if size == 296 and slack == "none":
            us_h, ys_h = spec.u_s + rng.uniform(-0.5, 0.5, (B, m)), spec.y_s + rng.uniform(-0.2, 0.2, (B, p))
        else:
            ab = rng.uniform(0.5, 1.5, B)
            us_h, ys_h = ab[:, None] * np.asarray(spec.u_s)[None, :], ab[:, None] * np.asarray(spec.y_s)[None, :]
        us, ys = t(us_h), t(ys_h)
        us_own, ys_own = t(np.tile(spec.u_s, (B, 1))), t(np.tile(spec.y_s, (B, 1)))
        us2, ys2 = 1.1 * np.asarray(spec.u_s), 1.1 * np.asarray(spec.y_s)
        ys_np = np.asarray(spec.y_s, float)
        boxes = [("u[-4,6]", ("u", -4.0, 6.0), 64), ("u[0,2]/128", ("u", 0.0, 2.0), 128),
                 ("y+-0.2", ("y", np.minimum(ys_h.min(axis=0), ys_np) - 0.2, np.maximum(ys_h.max(axis=0), ys_np) + 0.2), 64)]
        for bname, box, cap in boxes:
            tag0 = "%d/%s/%s" % (size, slack, bname)
            with engine(spec, N, B, False, box, cap) as e0, engine(spec, N, B, not a.only_existing, box, cap) as e1:
                for e in (e0, e1):
                    e.set_data(ud, yd)
                    e.prepare()
                out0, out1 = e0.step(up, yp), e1.step(up, yp)
                counts(tag0, "ddmpc_step", out0)
                outs = e0.solve(up, yp)
                solves = {"ddmpc_solve opt 0": lambda: e0.solve(up, yp, *outs), "ddmpc_solve opt 0 (again)": lambda: e0.solve(up, yp, *outs)}
                if not a.only_existing:
                    solves["ddmpc_solve opt 1"] = lambda: e1.solve(up, yp, *out1)
                report(tag0 + " solve", alternate(solves, a.reps, 1))
                for e in (e0, e1):
                    e.prepare()
                steps = {"ddmpc_step opt 0": lambda: e0.step(up, yp, *out0), "ddmpc_step opt 0 (again)": lambda: e0.step(up, yp, *out0)}
                if not a.only_existing:
                    counts(tag0, "ddmpc_step_setpoints (handle's s)", e1.step_setpoints(up, yp, us_own, ys_own, *out1))
                    counts(tag0, "ddmpc_step_setpoints", e1.step_setpoints(up, yp, us, ys, *out1))
                    steps["ddmpc_step opt 1"] = lambda: e1.step(up, yp, *out1)
                    steps["ddmpc_step_setpoints (handle's s)"] = lambda: e1.step_setpoints(up, yp, us_own, ys_own, *out1)
                    steps["ddmpc_step_setpoints"] = lambda: e1.step_setpoints(up, yp, us, ys, *out1)
                report(tag0 + " step", alternate(steps, a.reps, a.inner))
                if a.only_existing:
                    continue
                flip = [0]

                def reprepare():                # without the option: new tables, new factors, then the step
                    flip[0] ^= 1
                    e0.set_setpoints(us2 if flip[0] else spec.u_s, ys2 if flip[0] else spec.y_s)
                    e0.step(up, yp, *out0)

                report(tag0 + " change", alternate({
                    "set_setpoints + prepare + step": reprepare,
                    "ddmpc_step_setpoints": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
                }, a.reps, 1))
        del ud, yd
        torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
