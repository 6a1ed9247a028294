"""Dev timing (GPU): DDMPC_OPT_LARGE_AFFINE_LAW on ROBUST controllers at the cfg-5 size (m = p = 8, n = 8, L = 30, N = 2000:
608 rows, the cfg5size_robust problem of bench.py), option off (the solve on the kept factors) and on (the law step), same process,
same data.  Slack NONE and CONVEX, data-tail and near-setpoint windows.  HIP-event timing, median of repeats after warm-up.

Records per case: ddmpc_prepare ms with and without the law, step ms of both, law bytes per instance 8 (nf + 1) r and the
achieved GB/s of the law step, the fraction of instances the step leaves to the re-solve (iters >= 2 under the box), the
fraction the law served (differs from the cold solve in some bit; the re-solve is bit-equal), the max relative difference of the
law step against the cold solve, and the break-even number of steps (prepare_law - prepare_factors) / (step_factors - step_law).

    python tools/large_robust_law_time.py [--batch 512] [--reps 7] [--refine auto] [--json out.json]
"""
import argparse, json, sys
import numpy as np
import torch                                   # (before the library: torch initialises the HIP runtime itself)
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=10, help="steps per timed repeat")
ap.add_argument("--refine", default="auto", choices=["off", "auto", "always"], help="DDMPC_OPT_REFINE of both handles")
ap.add_argument("--json", default="")
a = ap.parse_args()

if L.load().ddmpc_device_count() <= 0:
    raise SystemExit("large_robust_law_time: no HIP device visible -- the engine has no CPU fallback, nothing to time")

B = a.batch
rng = np.random.default_rng(0)
ns = n = 8; m = p = 8; Lh = 30; N = 2000
A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.002)
u_s = 0.1 * np.ones(m)
y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
d = generate_batch(range(B), N=N, plant=plant)
r, nf = (m + p) * (Lh + n), n * (m + p)
dev = torch.device("cuda", 0)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
ud, yd = t(d["u_d"]), t(d["y_d"])
wins = {"tail": (d["u_d"][:, -n:, :].reshape(B, -1), d["y_d"][:, -n:, :].reshape(B, -1))}
wins["setpoint"] = (np.tile(u_s, n)[None, :] + 1e-3 * rng.standard_normal((B, n * m)),
                    np.tile(y_s, n)[None, :] + 1e-3 * rng.standard_normal((B, n * p)))
law_bytes = 8.0 * (nf + 1) * r
res = {"refine": a.refine, "batch": B, "r": r, "nf": nf, "law_bytes_per_instance": law_bytes, "cases": []}


def ev_ms(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(a.reps):
        e0.record()
        for _ in range(k):
            fn()
        e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) / k)
    return float(np.median(out))


for slack in ("none", "convex"):
    eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=3.0, R=1e-4, u_s=u_s, y_s=y_s, batch=B, controller_type=L.ROBUST,
                       slack_type=L.SLACK_CONVEX if slack == "convex" else L.SLACK_NONE, eps_max=0.002, lamb_alpha=50.0,
                       lamb_sigma=1000.0, c=1.0, device=0)
    eng.set_refinement(a.refine)
    eng.set_data(ud, yd)
    prep = {}
    for law in (False, True, False, True):                      # alternated, the second of each kept (first: allocations)
        eng.set_large_affine_law(law)
        prep[law] = ev_ms(lambda: (eng.set_data(ud, yd), eng.prepare()), 1)
    for kind, (up_h, yp_h) in wins.items():
        up, yp = t(up_h), t(yp_h)
        cold = [x.clone() for x in eng.solve(up, yp)]
        rec = {"slack": slack, "windows": kind, "prepare_ms_factors": prep[False], "prepare_ms_law": prep[True]}
        for law in (False, True, False, True):
            eng.set_large_affine_law(law)
            eng.prepare()
            o = eng.step(up, yp)
            ms = ev_ms(lambda: eng.step(up, yp, *o), a.inner)
            rec["step_ms_law" if law else "step_ms_factors"] = ms
            if law:
                rec["max_rel_diff_u_vs_cold"] = float((o[0] - cold[0]).abs().max() / cold[0].abs().max())
                rec["status_equal"] = bool(torch.equal(o[2], cold[2]))
                rec["iters_equal"] = bool(torch.equal(o[3], cold[3]))
                rec["frac_resolved"] = float((o[3] >= 2).double().mean()) if slack == "convex" else 0.0
                # served by the law = differs from the cold solve in some bit (the re-solve of "no law" instances is bit-equal)
                rec["frac_law_served"] = float((o[0] != cold[0]).any(dim=1).double().mean())
        rec["speedup"] = rec["step_ms_factors"] / rec["step_ms_law"]
        rec["law_step_GBps"] = law_bytes * B / (rec["step_ms_law"] * 1e-3) / 1e9
        rec["frac_of_8TBps"] = rec["law_step_GBps"] / 8000.0
        gain = rec["step_ms_factors"] - rec["step_ms_law"]
        rec["break_even_steps"] = (rec["prepare_ms_law"] - rec["prepare_ms_factors"]) / gain if gain > 0 else None
        res["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    eng.close()

if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
