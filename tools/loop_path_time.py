"""Dev timing (GPU) of the host-launch-bound paths, one JSON line: the 4096 x 401 one-step per-step loop (CONVEX, auto) with direct launches and with
graph replay, and ddmpc_prepare + first ddmpc_step at 4096 instances on a CONVEX handle with the warm law on and on a
bounded handle ([-4, 6]).  Host clock around calls that end in a device synchronise; per figure the median of the repeats
after the first.  Run it from a checkout of another commit as well to compare host code.

    python tools/loop_path_time.py
"""
import json, sys, time
import numpy as np
sys.path.insert(0, ".")
from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import FOUR_TANK as P, controller_params, generate_batch

B, n_steps = 4096, 401
d = generate_batch(range(B))
w = 0.002 * np.random.default_rng(1).uniform(-1, 1, (B, n_steps, 2))
up = d["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
cfg = controller_params()
res = {}


def engine():
    return BatchedDDMPC(n=4, m=2, p=2, L_=30, N=400, Q=cfg["Q"], R=cfg["R"], u_s=cfg["u_s"], y_s=cfg["y_s"], batch=B,
                        controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX, eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
                        lamb_sigma=cfg["lamb_sigma"], c=cfg["c"])


with engine() as eng:
    eng.set_data(d["u_d"], d["y_d"]); eng.set_closed_loop_path("auto")
    for graph in (False, True, False, True, False, True):
        eng.set_closed_loop_graph(graph)
        t = time.perf_counter()
        eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=1)
        ms = (time.perf_counter() - t) * 1e3
        res.setdefault("loop_graph_ms" if graph else "loop_direct_ms", []).append(round(ms, 3))
    assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
for key, opt in (("prep_step_cwl_ms", lambda e: e.set_convex_warm_law(True)), ("prep_step_box_ms", lambda e: e.set_input_bounds(-4.0, 6.0))):
    with engine() as eng:
        opt(eng)
        for _ in range(4):
            eng.set_data(d["u_d"], d["y_d"])
            eng.synchronize()
            t = time.perf_counter()
            eng.prepare()
            eng.step(up, yp)
            res.setdefault(key, []).append(round((time.perf_counter() - t) * 1e3, 3))
# first entries include one-time work (code objects, allocations): the figure of a run is the median of the rest
out = {k: float(np.median(v[1:])) for k, v in res.items()}
out["all"] = res
print(json.dumps(out), flush=True)
