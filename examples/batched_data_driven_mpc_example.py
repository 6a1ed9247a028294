"""Batched Direct Data-Driven MPC example on an MI355X.

The flow of the reference's example script (examples/direct_data_driven_mpc_example.py:169-425) --
load the model and controller YAML files, randomise the initial state, generate a persistently
exciting trajectory, create the controller, close the loop for `t_sim` steps -- for `--batch`
independent noise realisations (seeds `seed .. seed+batch-1`) at once, with the whole control loop
on the device (ddmpc_closed_loop).  Instance `i` is the problem the reference example builds with
`--seed <seed+i>`.  No plots / animation: the closed-loop data are optionally written to an .npz.

    python examples/batched_data_driven_mpc_example.py --batch 4096 --t_sim 400 --verbose 1
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from direct_data_driven_mpc_amd import _lib as L                                  # noqa: E402
from direct_data_driven_mpc_amd.engine import BatchedDDMPC                        # noqa: E402
from direct_data_driven_mpc_amd.harness import (controller_params_from_yaml, generate_batch,   # noqa: E402
                                                plant_from_yaml, step_report_line)

CFG = os.path.join(ROOT, "examples", "config")


def parse_args():
    ap = argparse.ArgumentParser(description="Batched Direct Data-Driven MPC example (MI355X)")
    ap.add_argument("--model_config_path", default=os.path.join(CFG, "models", "four_tank_system_params.yaml"))
    ap.add_argument("--model_key_value", default="FourTankSystem")
    ap.add_argument("--controller_config_path",
                    default=os.path.join(CFG, "controllers", "data_driven_mpc_example_params.yaml"))
    ap.add_argument("--controller_key_value", default="data_driven_mpc_params")
    ap.add_argument("--n_mpc_step", type=int, default=None, help="n-step scheme: inputs applied per solve")
    ap.add_argument("--controller_type", choices=["Nominal", "Robust"], default=None)
    ap.add_argument("--slack_var_const_type", choices=["None", "Convex", "NonConvex"], default=None)
    ap.add_argument("--t_sim", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0, help="seed of instance 0; instance i uses seed+i")
    ap.add_argument("--batch", type=int, default=1024, help="number of independent controller instances")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="write u_sys / y_sys / status of all instances to this .npz")
    ap.add_argument("--plot", default=None, help="write a PNG of the closed-loop inputs/outputs (median, band, instance 0)")
    ap.add_argument("--u_min", type=float, nargs="+", default=None, help="lower input bounds (m values, or one for all channels)")
    ap.add_argument("--u_max", type=float, nargs="+", default=None, help="upper input bounds; give both or neither")
    ap.add_argument("--y_min", type=float, nargs="+", default=None, help="lower output bounds (p values, or one for all channels)")
    ap.add_argument("--y_max", type=float, nargs="+", default=None, help="upper output bounds; give both or neither")
    ap.add_argument("--box_safeguard", action="store_true",
                    help="with input bounds: finish solves on which the active-set iteration cycles by a primal active-set method")
    ap.add_argument("--box_warm_start", action="store_true",
                    help="with bounds up to 271 rows: start each solve's active-set iteration from the previous solve's set")
    ap.add_argument("--large_box_capacity", type=int, choices=[64, 128, 192, 256], default=None,
                    help="with bounds beyond 271 rows: how many boxed components may be active at once (default 64)")
    ap.add_argument("--large_box_safeguard", action="store_true",
                    help="with bounds beyond 271 rows: finish solves that end at the iteration cap by a primal active-set method")
    ap.add_argument("--large_box_warm_start", action="store_true",
                    help="with bounds beyond 271 rows: start each step's active-set iteration from the previous solve's set")
    ap.add_argument("--large_box_law", action="store_true",
                    help="with bounds beyond 271 rows: serve the steps that stay inside the box from the affine law, solve only the others")
    ap.add_argument("--setpoint_spread", type=float, default=None,
                    help="instance b tracks its own equilibrium: u_s + S * uniform(-1, 1) (generator seeded with --seed) and the "
                         "output the plant settles at under it (robust scheme, slack None; closed_loop_setpoints).  Together with "
                         "--u_min/--u_max or --y_min/--y_max every instance tracks its setpoint inside the box "
                         "(set_setpoint_box_law; --box_safeguard applies).  With slack Convex, bounded or not: "
                         "set_setpoint_convex_law.  With bounds and a long horizon, beyond 271 rows: "
                         "set_large_setpoint_bounds (--large_box_capacity / --large_box_safeguard apply)")
    ap.add_argument("--bound_spread", type=float, default=None,
                    help="a fleet with different limits: with --u_min/--u_max and / or --y_min/--y_max, the finite bounds of "
                         "instance b are widened by S * b / (batch - 1) on both sides and set per instance "
                         "(set_instance_input_bounds / set_instance_output_bounds; up to 271 rows).  Together with --setpoint_spread every "
                         "instance tracks its own setpoint inside its own box (set_instance_setpoint_bounds; up to 271 rows)")
    ap.add_argument("--verbose", type=int, choices=[0, 1, 2], default=1)
    return ap.parse_args()


def main():
    a = parse_args()
    plant = plant_from_yaml(a.model_config_path, a.model_key_value)
    m, p = plant["B"].shape[1], plant["C"].shape[0]
    over = {}
    if a.controller_type is not None:
        over["controller_type"] = {"Nominal": 0, "Robust": 1}[a.controller_type]
    if a.slack_var_const_type is not None:
        over["slack_var_constraint_type"] = {"None": 0, "Convex": 1, "NonConvex": 2}[a.slack_var_const_type]
    cfg = controller_params_from_yaml(a.controller_config_path, a.controller_key_value, m=m, p=p, overrides=over)
    n_mpc_step = a.n_mpc_step if a.n_mpc_step is not None else cfg["n_mpc_step"]   # controller_creation.py: n_mpc_step = n
    n, Lh, N, B = cfg["n"], cfg["L"], cfg["N"], a.batch
    if cfg["slack"] == "non_convex":
        raise NotImplementedError("Robust Data-Driven MPC with a non-convex constraint for the slack variable "
                                  "is not currently implemented.")            # controller.py:664-670
    if a.verbose:
        print(f"Data-Driven MPC: {'robust' if cfg['robust'] else 'nominal'} scheme, slack {cfg['slack']}, "
              f"n={n} L={Lh} N={N}, n_mpc_step={n_mpc_step}, batch={B}, seeds {a.seed}..{a.seed + B - 1}")

    t0 = time.perf_counter()
    data = generate_batch(range(a.seed, a.seed + B), N=N, plant=plant, u_range=cfg["u_range"])
    n_steps = a.t_sim + 1                                                        # controller_operation.py:263
    w = np.stack([plant["eps_max"] * rng.uniform(-1.0, 1.0, (n_steps, p)) for rng in data["rngs"]])
    t_gen = time.perf_counter() - t0

    eng = BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                       controller_type=L.ROBUST if cfg["robust"] else L.NOMINAL,
                       slack_type=L.SLACK_CONVEX if cfg["slack"] == "convex" else L.SLACK_NONE,
                       eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"],
                       use_terminal_constraint=cfg["tec"], device=a.device)
    ok, rank = eng.persistent_excitation_guard(data["u_d"])                      # controller.py:275-296
    if not np.all(ok):
        bad = int(np.nonzero(~ok)[0][0])
        raise ValueError(f"Initial input trajectory data is not persistently exciting of order (L + 2 * n) "
                         f"(instance {bad}: rank {int(rank[bad])}).")
    if (a.u_min is None) != (a.u_max is None):
        raise ValueError("--u_min and --u_max go together (use inf / -inf for a side without a bound)")
    eng.set_large_bounds(True)                   # (bounds with a long horizon, beyond 271 rows: the phase kernels)
    if (a.y_min is None) != (a.y_max is None):
        raise ValueError("--y_min and --y_max go together (use inf / -inf for a side without a bound)")
    if a.bound_spread is not None:
        if a.u_min is None and a.y_min is None:
            raise ValueError("--bound_spread widens the bounds of --u_min/--u_max and / or --y_min/--y_max: give at least one pair")
        if a.setpoint_spread is not None:        # per-instance bounds with per-instance setpoints: DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS
            if (m + p) * (Lh + n) > 271:
                raise ValueError("--bound_spread together with --setpoint_spread is limited to 271 rows: (m+p)(L+n) = "
                                 f"{(m + p) * (Lh + n)} (beyond that the bounds stay shared by the batch)")
            eng.set_instance_setpoint_bounds(True)

        def rows(lo, hi, nc):                    # instance b: [lo - S b / (B - 1), hi + S b / (B - 1)] on the finite sides
            grow = a.bound_spread * np.arange(B)[:, None] / max(B - 1, 1)
            return np.broadcast_to(np.asarray(lo, float), (nc,)) - grow, np.broadcast_to(np.asarray(hi, float), (nc,)) + grow

        if a.u_min is not None:
            eng.set_instance_input_bounds(*rows(a.u_min, a.u_max, m))
        if a.y_min is not None:
            eng.set_instance_output_bounds(*rows(a.y_min, a.y_max, p))
    else:
        if a.u_min is not None:
            eng.set_input_bounds(a.u_min if len(a.u_min) > 1 else a.u_min[0], a.u_max if len(a.u_max) > 1 else a.u_max[0])
        if a.y_min is not None:
            eng.set_output_bounds(a.y_min if len(a.y_min) > 1 else a.y_min[0], a.y_max if len(a.y_max) > 1 else a.y_max[0])
    if a.box_safeguard:
        eng.set_box_safeguard(True)
    if a.box_warm_start:
        eng.set_box_warm_start(True)
    if a.large_box_capacity is not None:
        eng.set_large_box_capacity(a.large_box_capacity)
    if a.large_box_safeguard:
        eng.set_large_box_safeguard(True)
    if a.large_box_warm_start:
        eng.set_large_box_warm_start(True)
    if a.large_box_law:
        eng.set_large_box_law(True)
    us_b = ys_b = None                           # --setpoint_spread: the setpoints of every instance, [B, m] and [B, p]
    bounded = a.u_min is not None or a.y_min is not None
    if a.setpoint_spread is not None:
        if bounded and (m + p) * (Lh + n) > 271: # bounds beyond 271 rows, slack NONE or CONVEX: DDMPC_OPT_LARGE_SETPOINT_BOUNDS
            eng.set_large_setpoint_bounds(True)
        elif cfg["slack"] == "convex":           # under the CONVEX slack box, bounded or not: DDMPC_OPT_SETPOINT_CONVEX_LAW
            eng.set_setpoint_convex_law(True)
        elif bounded:                            # setpoints per instance inside the box: DDMPC_OPT_SETPOINT_BOX_LAW
            eng.set_setpoint_box_law(True)
        else:
            eng.set_setpoint_law(True)
        gain_dc = plant["C"] @ np.linalg.inv(np.eye(plant["A"].shape[0]) - plant["A"]) @ plant["B"] + plant["D"]
        us_b = np.asarray(cfg["u_s"], float) + a.setpoint_spread * np.random.default_rng(a.seed).uniform(-1.0, 1.0, (B, m))
        ys_b = us_b @ gain_dc.T                  # y_s = (C (I - A)^-1 B + D) u_s: an equilibrium of the plant
    eng.set_data(data["u_d"], data["y_d"])
    up = data["u_d"][:, -n:, :].reshape(B, -1)                                   # controller.py:184-185
    yp = data["y_d"][:, -n:, :].reshape(B, -1)
    u0, cost0, status0, _ = eng.solve(up, yp)                                    # the construction-time solve
    if np.any(status0 > 1):
        raise ValueError("Failed to get the optimal control input: the first solve is not optimal for "
                         f"{int(np.count_nonzero(status0 > 1))} instance(s)")
    t1 = time.perf_counter()
    if us_b is not None:                         # every step of an instance tracks that instance's own setpoint
        u_sys, y_sys, status, x_end, up_end, yp_end = eng.closed_loop_setpoints(
            plant["A"], plant["B"], plant["C"], plant["D"], data["x_end"], up, yp, w,
            np.repeat(us_b[:, None, :], n_steps, axis=1), np.repeat(ys_b[:, None, :], n_steps, axis=1), n_mpc_step=n_mpc_step)
    else:
        u_sys, y_sys, status, x_end, up_end, yp_end = eng.closed_loop(plant["A"], plant["B"], plant["C"], plant["D"],
                                                                      data["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
    t_loop = time.perf_counter() - t1

    if a.verbose > 1:                                                            # per-step report of instance 0
        with BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=1,
                          controller_type=L.ROBUST if cfg["robust"] else L.NOMINAL,
                          slack_type=L.SLACK_CONVEX if cfg["slack"] == "convex" else L.SLACK_NONE,
                          eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"],
                          c=cfg["c"], use_terminal_constraint=cfg["tec"], device=a.device) as one:
            if us_b is not None and (bounded or cfg["slack"] == "convex"):
                if bounded and (m + p) * (Lh + n) > 271:
                    one.set_large_bounds(True)
                    one.set_large_setpoint_bounds(True)
                    if a.large_box_capacity is not None:
                        one.set_large_box_capacity(a.large_box_capacity)
                    one.set_large_box_safeguard(a.large_box_safeguard)
                elif cfg["slack"] == "convex":
                    one.set_setpoint_convex_law(True)
                else:
                    one.set_setpoint_box_law(True)
                if a.u_min is not None:
                    one.set_input_bounds(a.u_min if len(a.u_min) > 1 else a.u_min[0], a.u_max if len(a.u_max) > 1 else a.u_max[0])
                if a.y_min is not None:
                    one.set_output_bounds(a.y_min if len(a.y_min) > 1 else a.y_min[0], a.y_max if len(a.y_max) > 1 else a.y_max[0])
                one.set_box_safeguard(a.box_safeguard)
            elif us_b is not None:
                one.set_setpoint_law(True)
            one.set_data(data["u_d"][:1], data["y_d"][:1])
            U = np.concatenate([data["u_d"][0, -n:], u_sys[0]]); Y = np.concatenate([data["y_d"][0, -n:], y_sys[0]])
            for t in range(0, n_steps, n_mpc_step):                              # one line per solve, controller_operation.py:310-329
                if us_b is not None:
                    _, cst, _, _ = one.step_setpoints(U[t:t + n].reshape(1, -1), Y[t:t + n].reshape(1, -1), us_b[:1], ys_b[:1])
                else:
                    _, cst, _, _ = one.step(U[t:t + n].reshape(1, -1), Y[t:t + n].reshape(1, -1))
                k = min(t + n_mpc_step, n_steps) - 1                             # errors of the last applied step
                print(step_report_line(t, float(cst[0]), cfg["u_s"] if us_b is None else us_b[0],
                                       cfg["y_s"] if ys_b is None else ys_b[0], u_sys[0, k], y_sys[0, k]))
    if a.verbose:
        n_bad = int(np.count_nonzero(status > 1))
        err_y = np.abs(y_sys[:, -1, :] - (cfg["y_s"] if ys_b is None else ys_b))
        err_u = np.abs(u_sys[:, -1, :] - (cfg["u_s"] if us_b is None else us_b))
        solves = B * ((n_steps + n_mpc_step - 1) // n_mpc_step)
        print(f"data generation (host) {t_gen:.2f} s; closed loop of {B} controllers x {n_steps} steps "
              f"({solves} QP solves) in {t_loop * 1e3:.1f} ms incl. host<->device copies")
        print(f"non-optimal instances: {n_bad}; final |y - y_s| mean {err_y.mean(axis=0)}, max {err_y.max(axis=0)}; "
              f"final |u - u_s| mean {err_u.mean(axis=0)}")
        print(f"instance 0: y[-1] = {y_sys[0, -1]}, u[-1] = {u_sys[0, -1]}")
        if a.bound_spread is not None:
            print(f"per-instance bounds (spread {a.bound_spread}): {eng.closed_loop_kernel_name()}")
        if us_b is not None:
            print(f"per-instance setpoints (spread {a.setpoint_spread}): instance 0 tracks y_s = {ys_b[0]}, u_s = {us_b[0]}; "
                  f"{eng.closed_loop_kernel_name()}")
    if a.out:
        np.savez_compressed(a.out, u_sys=u_sys, y_sys=y_sys, status=status, u_s=cfg["u_s"] if us_b is None else us_b,
                            y_s=cfg["y_s"] if ys_b is None else ys_b)
    if a.plot:
        from _plot import plot_closed_loops
        if us_b is not None:                     # every instance as its deviation from its own setpoint, around the configured one
            u_sys = u_sys - us_b[:, None, :] + np.asarray(cfg["u_s"], float)
            y_sys = y_sys - ys_b[:, None, :] + np.asarray(cfg["y_s"], float)
        plot_closed_loops(a.plot, {"closed loop": (u_sys, y_sys)}, cfg["u_s"], cfg["y_s"],
                          title=f"{B} controllers, {'robust' if cfg['robust'] else 'nominal'} scheme, slack {cfg['slack']}")
    eng.close()


if __name__ == "__main__":
    main()
