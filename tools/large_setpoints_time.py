"""Dev timing (GPU): DDMPC_OPT_LARGE_SETPOINTS beyond 271 rows -- the four-tank plant at L = 70, N = 700 (296 rows) and the
8 x 8-channel size (608 rows, N = 2000), slack NONE and CONVEX, batch 512.  HIP events, median / min / max of `--reps` repeats,
the compared versions alternating in one process after a warm-up of every version.  Per size and slack type:

  * kept factors: ddmpc_step with the option 0 -- twice, as two entries of the alternation: their difference is the run-to-run
    spread -- and with the option 1, against ddmpc_step_setpoints at the handle's own setpoints (the same problems) and at
    per-instance setpoints;
  * the law, under DDMPC_REFINE_OFF and AUTO: ddmpc_step against ddmpc_step_setpoints, with the bytes each streams
    ((nf + 1) r 8 against (nf + m + p) r 8 per instance) and the rate that makes; the fraction of instances the law step
    served (outputs that differ in some bit from the kept-factor setpoint step);
  * the sequence the new step replaces, ddmpc_set_setpoints + ddmpc_prepare + ddmpc_step, against both routes;
  * ddmpc_prepare without the law, with the law, with the law and S (the preparation is forgotten before every call);
  * ddmpc_solve with the option 0 (twice) and 1.

What this tool does not do.  "Option off against the parent commit" is measured here as option 0 against option 1 in one
process of ONE build (with the spread of the doubled option-0 entry); a build of the parent is not timed, the resource table of
DESIGN.md 9e says its kernels are the same.  The served fraction is inferred from the outputs -- an instance counts as served
when its law step differs in some bit from the kept-factor setpoint step -- not read from the nolaw / nosp counts.

Per-instance setpoints: the handle's (u_s, y_s) scaled by a_b in [0.5, 1.5] (equilibria of the plant at the 608-row size, where
any other setpoint binds the 64 terminal slacks under CONVEX); u_s +- 0.5, y_s +- 0.2 on the four-tank with slack NONE.

    python tools/large_setpoints_time.py [--batch 512] [--reps 5] [--sizes 296,608] [--json out.json]
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
ap.add_argument("--inner", type=int, default=10, help="steps per timed repeat")
ap.add_argument("--sizes", default="296,608")
ap.add_argument("--json", default="")
a = ap.parse_args()

lib = L.load()
if lib.ddmpc_device_count() <= 0:
    raise SystemExit("large_setpoints_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
REFINE_RES_DEFAULT = 107                       # (DDMPC_REFINE_RES_DEFAULT: setting it changes nothing but forgets the preparation)
res = {}


def case(size, slack, B):
    if size == 296:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=70)
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


def engine(spec, N, B, option, law, refine):
    eng = BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                       controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if spec.slack == "convex" else L.SLACK_NONE,
                       eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c,
                       use_terminal_constraint=spec.tec)
    eng.set_refinement(refine)
    eng.set_large_affine_law(law)
    eng.set_large_setpoints(option)
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


def report(tag, out, nbytes=None):
    for k, (med, lo, hi) in out.items():
        e = dict(ms=med, min_ms=lo, max_ms=hi)
        extra = ""
        if nbytes and k in nbytes:
            e["TBps"] = nbytes[k] / (med * 1e-3) / 1e12
            extra = "   %.2f TB/s of %.0f MB" % (e["TBps"], nbytes[k] / 1e6)
        res["%s | %s" % (tag, k)] = e
        print("%-28s %-44s %9.1f us   (min %.1f, max %.1f)%s" % (tag, k, med * 1e3, lo * 1e3, hi * 1e3, extra), flush=True)


B = a.batch
for size in [int(x) for x in a.sizes.split(",")]:
    for slack in ("none", "convex"):
        spec, N, d = case(size, slack, B)
        n, m, p = spec.n, spec.m, spec.p
        r, nf, nch = (m + p) * (spec.L + n), n * (m + p), m + p
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
        tag0 = "%d/%s" % (size, slack)

        def prepare(e):                         # ddmpc_prepare alone: the preparation forgotten by an option write that changes nothing
            L.check(lib.ddmpc_set_option(e._h, L.OPT_REFINE_RES_LOG10, REFINE_RES_DEFAULT))
            e.prepare()

        # ---- kept factors
        with engine(spec, N, B, False, False, "auto") as e0, engine(spec, N, B, True, False, "auto") as e1:
            for e in (e0, e1):
                e.set_data(ud, yd)
                e.prepare()
            out0, out1 = e0.step(up, yp), e1.step(up, yp)
            kept = tuple(torch.as_tensor(x).clone() for x in e1.step_setpoints(up, yp, us, ys))
            torch.cuda.synchronize()
            res["%s | kept-factor setpoint step" % tag0] = dict(iters_mean=float(kept[3].double().mean()), iters_max=int(kept[3].max()),
                                                              not_optimal=int((kept[2] > 1).sum()))
            print("%-28s kept-factor ddmpc_step_setpoints: iters mean %.2f max %d, not optimal %d" %
                  (tag0, float(kept[3].double().mean()), int(kept[3].max()), int((kept[2] > 1).sum())), flush=True)
            outs = e0.solve(up, yp)
            report(tag0 + " solve", alternate({
                "ddmpc_solve opt 0": lambda: e0.solve(up, yp, *outs),
                "ddmpc_solve opt 0 (again)": lambda: e0.solve(up, yp, *outs),
                "ddmpc_solve opt 1": lambda: e1.solve(up, yp, *out1),
            }, a.reps, a.inner))
            for e in (e0, e1):
                e.prepare()
            report(tag0 + " factors", alternate({
                "ddmpc_step opt 0": lambda: e0.step(up, yp, *out0),
                "ddmpc_step opt 0 (again)": lambda: e0.step(up, yp, *out0),
                "ddmpc_step opt 1": lambda: e1.step(up, yp, *out1),
                "ddmpc_step_setpoints (handle's s)": lambda: e1.step_setpoints(up, yp, us_own, ys_own, *out1),
                "ddmpc_step_setpoints": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
            }, a.reps, a.inner))
            flip = [0]

            def reprepare():                    # without the option: new tables, new factors, then the step
                flip[0] ^= 1
                e0.set_setpoints(us2 if flip[0] else spec.u_s, ys2 if flip[0] else spec.y_s)
                e0.step(up, yp, *out0)

            report(tag0 + " change", alternate({
                "set_setpoints + prepare + step (no law)": reprepare,
                "ddmpc_step_setpoints (factors)": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
            }, a.reps, 1))
            report(tag0 + " prepare", alternate({"ddmpc_prepare, no law": lambda: prepare(e0)}, a.reps, 1))
        # ---- the law
        for refine in ("off", "auto"):
            with engine(spec, N, B, False, True, refine) as e0, engine(spec, N, B, True, True, refine) as e1:
                for e in (e0, e1):
                    e.set_data(ud, yd)
                    e.prepare()
                out0, out1 = e0.step(up, yp), e1.step(up, yp)
                law = tuple(torch.as_tensor(x).clone() for x in e1.step_setpoints(up, yp, us, ys))
                torch.cuda.synchronize()
                if refine == "auto":
                    served = (law[0] != kept[0]).any(dim=1).double().mean().item()
                    res["%s | law served under AUTO" % tag0] = served
                    print("%-28s fraction of instances the setpoint law step served under AUTO: %.3f" % (tag0, served), flush=True)
                nb = {"ddmpc_step on the law": B * (nf + 1) * r * 8.0, "ddmpc_step_setpoints on the law": B * (nf + nch) * r * 8.0}
                report("%s law/%s" % (tag0, refine), alternate({
                    "ddmpc_step on the law": lambda: e0.step(up, yp, *out0),
                    "ddmpc_step on the law, opt 1": lambda: e1.step(up, yp, *out1),
                    "ddmpc_step_setpoints on the law": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
                }, a.reps, a.inner), nb)
                flip = [0]

                def reprepare_law():
                    flip[0] ^= 1
                    e0.set_setpoints(us2 if flip[0] else spec.u_s, ys2 if flip[0] else spec.y_s)
                    e0.step(up, yp, *out0)

                report("%s change/%s" % (tag0, refine), alternate({
                    "set_setpoints + prepare + step (law)": reprepare_law,
                    "ddmpc_step_setpoints (law)": lambda: e1.step_setpoints(up, yp, us, ys, *out1),
                }, a.reps, 1))
                report("%s prepare/%s" % (tag0, refine), alternate({
                    "ddmpc_prepare, law": lambda: prepare(e0),
                    "ddmpc_prepare, law and S": lambda: prepare(e1),
                }, a.reps, 1))
        del ud, yd
        torch.cuda.empty_cache()
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
