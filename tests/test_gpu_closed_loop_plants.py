"""The device closed loop (ddmpc_closed_loop) on plants other than the four-tank, against the CPU oracle's loop.

Three kernels carry a copy of the plant step and the FIFO push: ddmpc_plant_kernel (every per-step path),
ddmpc_closed_loop_warm_kernel (fused loop on the affine law) and ddmpc_closed_loop_convex_warm_kernel (fused loop under
the slack box).  The four-tank has m = p, ns = n and D = 0, which hides a swap of m and p, of ns and n, and the whole
D u term; the plants here have none of these coincidences.  The reference of every comparison is
oracle.ddmpc_oracle.closed_loop (full-space QP by numpy at every solve, oracle.Plant stepped in place) on identical
data, noise, initial state and windows.  Bars (those of test_device_closed_loop_matches_oracle, fp64): u_sys 1e-8 of
max|u_ref|, y_sys and x_end 1e-9 of max(1, max|y_ref|), status optimal everywhere.

Every number below (plant and data seeds, c, max_iter, stop indices) was chosen from the oracle alone on a CPU; the
note next to it says how to see it again.  Nothing was tuned on what the device returns.
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

pytestmark = pytest.mark.gpu

TOL_U, TOL_Y = 1e-8, 1e-9
EPS = 0.002


# ------------------------------------------------------------------------------------------------ problem construction
def random_plant(m, p, ns, feedthrough=True):
    """Random stable LTI plant as in test_structured_gram_for_any_channel_count: A scaled to spectral radius 0.8, normal B
    and C, D = 0.3 * normal (or zero).  The generator is seeded by the shape alone."""
    rng = np.random.default_rng(9000 + 400 * m + 20 * p + ns)
    A = rng.normal(size=(ns, ns))
    A *= 0.8 / max(abs(np.linalg.eigvals(A)))
    Bm = rng.normal(size=(ns, m))
    C = rng.normal(size=(p, ns))
    D = 0.3 * rng.normal(size=(p, m))
    if not feedthrough:
        D = np.zeros((p, m))
    u_s = rng.uniform(-0.5, 0.5, m)
    y_s = (C @ np.linalg.inv(np.eye(ns) - A) @ Bm + D) @ u_s            # the output the plant settles at under u_s
    return dict(A=A, B=Bm, C=C, D=D, eps_max=EPS), u_s, y_s


def make_case(m, p, ns, n, Lh, slack, c=1.0, feedthrough=True, B=3, n_steps=10, seed0=0):
    """Controller (ROBUST, Q = 2, R = 0.05, lamb_alpha = 20, lamb_sigma = 500), data of `B` seeds, and the loop's inputs:
    the plant state after the data run, the data tail as the past windows, uniform noise of the plant's own bound."""
    plant, u_s, y_s = random_plant(m, p, ns, feedthrough)
    N = (m + 1) * (Lh + 2 * n) + 120
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=u_s, y_s=y_s, robust=True,
                      eps_max=EPS, lamb_alpha=20.0, lamb_sigma=500.0, c=c, slack=slack, tec=True)
    d = generate_batch(range(seed0, seed0 + B), N=N, plant=plant)
    w = EPS * np.random.default_rng(77 + seed0).uniform(-1.0, 1.0, (B, n_steps, p))
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy()
    yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    return dict(plant=plant, spec=spec, N=N, B=B, u_d=d["u_d"], y_d=d["y_d"], x0=d["x_end"].copy(), up=up, yp=yp, w=w)


def engine(case, **kw):
    s = case["spec"]
    return BatchedDDMPC(n=s.n, m=s.m, p=s.p, L_=s.L, N=case["N"], Q=2.0, R=0.05, u_s=s.u_s, y_s=s.y_s, batch=case["B"],
                        controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if s.slack == "convex" else L.SLACK_NONE,
                        eps_max=EPS, lamb_alpha=20.0, lamb_sigma=500.0, c=s.c, **kw)


def oracle_loop(case, b, n_mpc_step, n_steps=None):
    """orc.closed_loop for instance b -> (u_ref, y_ref, x_end of the oracle's plant)."""
    pl = case["plant"]
    plant = orc.Plant(pl["A"], pl["B"], pl["C"], pl["D"], pl["eps_max"])
    plant.x = case["x0"][b].copy()
    w = case["w"][b] if n_steps is None else case["w"][b, :n_steps]
    u_ref, y_ref = orc.closed_loop(case["spec"], case["u_d"][b], case["y_d"][b], plant, w, n_mpc_step=n_mpc_step,
                                   u_past=case["up"][b], y_past=case["yp"][b])
    return u_ref, y_ref, plant.x


def window_at(first, traj, t, n):
    """The past window (last n rows) after t steps of `traj` [T, ch] were pushed into the window `first` [n*ch]."""
    ch = traj.shape[1]
    return np.concatenate([first.reshape(n, ch), traj[:t]])[t:t + n].reshape(-1)


def oracle_iterations(case, n_mpc_step):
    """Active-set solves of the oracle at every solve of every instance's loop (CPU only)."""
    s = case["spec"]
    out = []
    for b in range(case["B"]):
        u_ref, y_ref, _ = oracle_loop(case, b, n_mpc_step)
        out.append([orc.solve_fullspace(s, case["u_d"][b], case["y_d"][b], window_at(case["up"][b], u_ref, t, s.n),
                                        window_at(case["yp"][b], y_ref, t, s.n)).iters
                    for t in range(0, u_ref.shape[0], n_mpc_step)])
    return out


PLANT, FUSED, FUSED_BOX = "ddmpc_plant_kernel", "ddmpc_closed_loop_warm_kernel", "ddmpc_closed_loop_convex_warm_kernel"


def paths_of(slack):
    """(name, closed-loop path, fused convex law, the kernel that must step the plant) of every path that serves a small handle
    of this slack type."""
    if slack == "none":
        return [("cold", "cold", False, PLANT),           # cold solve + ddmpc_plant_kernel per step
                ("fused", "warm", False, FUSED)]
    return [("cold", "cold", False, PLANT),
            ("filtered", "auto", False, PLANT),           # affine iterate + filtered cold launch + ddmpc_plant_kernel per step
            ("fused", "warm", True, FUSED_BOX)]


def run_loop(eng, case, path, cwl, kernel, n_mpc_step):
    """One closed loop on `path`; the leg fails unless `kernel` is what stepped the plant (a fused leg that quietly ran per
    step would test ddmpc_plant_kernel once more under another name).  Fused convex legs turn refinement off: a law that
    ddmpc_prepare took from refining solves sends the loop to the per-step path, and with DDMPC_REFINE_OFF there is none by
    construction (the p = 17 box row is such a handle under the default AUTO).  The bars stay the same."""
    pl = case["plant"]
    if cwl:
        eng.set_convex_warm_law(True)
        eng.set_refinement("off")
    eng.set_data(case["u_d"], case["y_d"])
    eng.set_closed_loop_path(path)
    out = eng.closed_loop(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"],
                          n_mpc_step=n_mpc_step)
    assert eng.closed_loop_kernel_name() == kernel, (path, cwl, eng.closed_loop_kernel_name())
    return out


def check_against_oracle(case, out, n_mpc_step, tag, refs=None):
    """Every instance, every step: the assertions of the module docstring; prints each figure before it is asserted."""
    u_sys, y_sys, status, x_end, up_end, yp_end = out
    s = case["spec"]
    n = s.n
    n_steps = u_sys.shape[1]
    assert [int(v) for v in status] == [0] * case["B"], (tag, status)
    for b in range(case["B"]):
        u_ref, y_ref, x_ref = refs[b] if refs is not None else oracle_loop(case, b, n_mpc_step, n_steps)
        ysc = max(1.0, np.max(np.abs(y_ref)))
        eu = np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref))
        ey = np.max(np.abs(y_sys[b] - y_ref)) / ysc
        ex = np.max(np.abs(x_end[b] - x_ref)) / ysc
        print("%s instance %d: u %.2e  y %.2e  x_end %.2e" % (tag, b, eu, ey, ex))
        assert eu < TOL_U, (tag, b, eu)
        assert ey < TOL_Y, (tag, b, ey)
        assert ex < TOL_Y, (tag, b, ex)
        # the returned windows are the tail of the returned trajectories, bit for bit (the head of the window that came in,
        # where the loop is shorter than the window)
        assert np.array_equal(up_end[b], window_at(case["up"][b], u_sys[b], n_steps, n)), (tag, b)
        assert np.array_equal(yp_end[b], window_at(case["yp"][b], y_sys[b], n_steps, n)), (tag, b)


def check_solution_record(case, eng, out, n_mpc_step, tag):
    """ddmpc_get_solution after the loop is the loop's last solve, at the window that solve saw -- the `.value`s the
    reference holds after its loop: equal to a ddmpc_solve at that window, and to the oracle's solve there."""
    u_sys, y_sys = out[0], out[1]
    s = case["spec"]
    Bn, n_steps = case["B"], u_sys.shape[1]
    t_last = n_mpc_step * ((n_steps - 1) // n_mpc_step)
    got = {k: eng.get_solution(k) for k in ("ubar", "ybar", "sigma", "alpha")}
    wu = np.stack([window_at(case["up"][b], u_sys[b], t_last, s.n) for b in range(Bn)])
    wy = np.stack([window_at(case["yp"][b], y_sys[b], t_last, s.n) for b in range(Bn)])
    eng.solve(wu, wy)
    for k, v in got.items():
        ref = eng.get_solution(k)
        err = np.max(np.abs(v - ref)) / max(1.0, np.max(np.abs(ref)))
        print("%s get_solution(%s) vs a solve at the last solve's window: %.2e" % (tag, k, err))
        assert err < 1e-9, (tag, k, err)
    for b in range(Bn):
        sol = orc.solve_fullspace(s, case["u_d"][b], case["y_d"][b], wu[b], wy[b])
        for k, ref in (("ubar", sol.ubar), ("ybar", sol.ybar)):
            err = np.max(np.abs(got[k][b] - ref)) / max(1.0, np.max(np.abs(ref)))
            assert err < 1e-8, (tag, k, b, err)


# ------------------------------------------------------------------------------------------------------------ the table
# (m, p, ns, n, L, n_mpc_step, n_steps, D != 0, slack, c) -- rows = (m + p)(L + n).  `c` scales the slack box (bound = c *
# eps_max); it is 1 unless lowered so that the ORACLE needs two or more active-set solves somewhere in the row's loops.
# The oracle's counts are in ORACLE_ITERS below.
CASES = {
    "siso-ns<n":         (1, 1, 2, 3, 8, 1, 13, True, "none", 1.0),       # 22 rows
    "siso-nstep=L":      (1, 1, 2, 3, 8, 8, 21, True, "convex", 1.0),     # 22 rows; n_mpc_step == L > n, ragged last block
    "m<p-nstep>n":       (1, 2, 3, 3, 10, 4, 14, True, "convex", 1.0),    # 39 rows
    "m>p-ns>n":          (3, 2, 5, 3, 9, 2, 11, True, "none", 1.0),       # 60 rows; five channels: Gram pre-launch
    "ns=1":              (2, 3, 1, 2, 7, 3, 10, False, "convex", 1.0),    # 45 rows; D = 0
    "ns=16":             (4, 4, 16, 4, 12, 5, 17, True, "none", 1.0),     # 128 rows; ns at its cap
    "p=17":              (1, 17, 4, 2, 10, 3, 10, True, "none", 1.0),     # 216 rows; more outputs than the fused loops once copied
    "p=17-box":          (2, 17, 4, 2, 10, 1, 7, True, "convex", 1.0),    # 228 rows
    "m=17":              (17, 1, 4, 4, 9, 2, 7, True, "none", 1.0),       # 234 rows
}
# ("p=17-box": under the default refinement mode ddmpc_prepare takes some of this row's laws from refining solves, and such a
#  handle's WARM loop runs per step; run_loop turns refinement off on the fused convex legs and asserts the kernel.)
# oracle_iterations() of the convex rows with the c above, per instance and solve: no row needed a smaller box
# (asserted on a CPU by tests/test_oracle.py::test_premises_of_the_closed_loop_plant_tests)
ORACLE_ITERS = {
    "siso-nstep=L": [[2, 1, 1], [1, 1, 1], [1, 1, 1]],
    "m<p-nstep>n":  [[2, 1, 1, 1], [2, 1, 1, 1], [2, 1, 1, 1]],
    "ns=1":         [[2, 1, 1, 1], [2, 1, 1, 1], [2, 1, 1, 1]],
    "p=17-box":     [[3, 3, 2, 2, 2, 1, 1], [2, 2, 2, 2, 1, 1, 1], [2, 1, 1, 1, 1, 1, 1]],
}


def _table_case(name):
    m, p, ns, n, Lh, nms, n_steps, feed, slack, c = CASES[name]
    return make_case(m, p, ns, n, Lh, slack, c=c, feedthrough=feed, B=3, n_steps=n_steps), nms


@pytest.mark.parametrize("name", list(CASES))
def test_closed_loop_on_other_plants_matches_oracle(gpu, name):
    case, nms = _table_case(name)
    s = case["spec"]
    assert (s.m + s.p) * (s.L + s.n) <= 271                     # register-resident kernels: the fused loops serve these
    refs = [oracle_loop(case, b, nms) for b in range(case["B"])]
    for tag, path, cwl, kernel in paths_of(s.slack):
        with engine(case) as eng:
            out = run_loop(eng, case, path, cwl, kernel, nms)
            check_against_oracle(case, out, nms, "%s/%s" % (name, tag), refs)
            check_solution_record(case, eng, out, nms, "%s/%s" % (name, tag))


def test_loop_shorter_than_the_window(gpu):
    # n_steps = 2 < n = 3: the returned window keeps the last row of the one that came in (m < p, D != 0, n_mpc_step > n_steps
    # on the second call)
    m, p, ns, n, Lh, _, _, feed, slack, c = CASES["m<p-nstep>n"]
    case = make_case(m, p, ns, n, Lh, slack, c=c, feedthrough=feed, B=3, n_steps=2)
    for nms in (1, 4):
        for tag, path, cwl, kernel in paths_of(slack):
            with engine(case) as eng:
                out = run_loop(eng, case, path, cwl, kernel, nms)
                check_against_oracle(case, out, nms, "short/%s/nstep%d" % (tag, nms))
                assert np.array_equal(out[4][:, :(n - 2) * m], case["up"][:, 2 * m:])
                assert np.array_equal(out[5][:, :(n - 2) * p], case["yp"][:, 2 * p:])


# ------------------------------------------------------------------------------------------------- beyond 271 rows
LARGE = dict(m=2, p=3, ns=4, n=2, Lh=58, nms=2, n_steps=6, B=2, seed0=0, oracle_iters=[[3, 2, 2], [2, 2, 1]])     # (2 + 3)(58 + 2) = 300 rows


def _large_case():
    g = LARGE
    return make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], "convex", B=g["B"], n_steps=g["n_steps"], seed0=g["seed0"])


@pytest.mark.parametrize("law", [False, True], ids=["factors", "affine-law"])
def test_closed_loop_beyond_the_register_resident_kernels_on_another_plant(gpu, law):
    # step_on_route (phase kernels) + ddmpc_plant_kernel with m != p and D != 0, DDMPC_OPT_LARGE_AFFINE_LAW off and on; the
    # oracle stays optimal on seeds 0 and 1 (on a CPU: orc.closed_loop raises otherwise; its iteration counts are
    # [[3, 2, 2], [2, 2, 1]])
    case = _large_case()
    s = case["spec"]
    assert (s.m + s.p) * (s.L + s.n) == 300
    pl = case["plant"]
    with engine(case) as eng:
        eng.set_large_affine_law(law)
        eng.set_data(case["u_d"], case["y_d"])
        out = eng.closed_loop(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"],
                              n_mpc_step=LARGE["nms"])
        assert eng.closed_loop_kernel_name() == PLANT
        check_against_oracle(case, out, LARGE["nms"], "300rows/%s" % ("law" if law else "factors"))
        # the record of the loop: ubar / ybar of its last solve, against the oracle's solve at that window
        t_last = LARGE["nms"] * ((LARGE["n_steps"] - 1) // LARGE["nms"])
        got = {k: eng.get_solution(k) for k in ("ubar", "ybar")}
    for b in range(case["B"]):
        sol = orc.solve_fullspace(s, case["u_d"][b], case["y_d"][b], window_at(case["up"][b], out[0][b], t_last, s.n),
                                  window_at(case["yp"][b], out[1][b], t_last, s.n))
        for k, ref in (("ubar", sol.ubar), ("ybar", sol.ybar)):
            assert np.max(np.abs(got[k][b] - ref)) / max(1.0, np.max(np.abs(ref))) < 1e-8, (k, b)


# ------------------------------------------------------------------------------------------ an instance that stops
def _four_tank(B, seed0, n_steps, **kw):
    spec = orc.spec_from_params(**kw)
    d = generate_batch(range(seed0, seed0 + B))
    w = np.stack([EPS * np.random.default_rng(500 + s).uniform(-1.0, 1.0, (n_steps, 2)) for s in range(seed0, seed0 + B)])
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy()
    yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    return spec, d, up, yp, w


def _spec_engine(spec, B, **kw):
    return BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=400, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                        controller_type=L.ROBUST if spec.robust else L.NOMINAL,
                        slack_type=L.SLACK_CONVEX if (spec.robust and spec.slack == "convex") else L.SLACK_NONE,
                        eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c, **kw)


def test_instance_stopped_at_the_first_solve(gpu):
    """include/ddmpc.h: "an instance whose solve is not optimal stops evolving ... the rest of its trajectory is NaN".
    NOMINAL four-tank, instance 2 with a constant trajectory (infeasible, as in test_bad_instance_gets_status_not_exception):
    per-step path.  Its rows are NaN from step 0, its x / windows come back as they went in, and its neighbours are
    bit-equal to the same loop on a batch without it."""
    B, n_steps, nms = 4, 9, 2
    spec, d, up, yp, w = _four_tank(B, 0, n_steps, controller_type=0)
    u_d, y_d = d["u_d"].copy(), d["y_d"].copy()
    u_d[2] = 1.0
    y_d[2] = 0.5
    P = orc.FOUR_TANK
    x0 = d["x_end"]
    with _spec_engine(spec, B) as eng:
        eng.set_data(u_d, y_d)
        u_sys, y_sys, status, x_end, up_end, yp_end = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, up, yp, w, n_mpc_step=nms)
    assert L.STATUS_STRINGS[int(status[2])] == "infeasible"
    assert [int(v) for v in status[[0, 1, 3]]] == [0, 0, 0]
    assert np.all(np.isnan(u_sys[2])) and np.all(np.isnan(y_sys[2]))
    assert np.array_equal(x_end[2], x0[2]) and np.array_equal(up_end[2], up[2]) and np.array_equal(yp_end[2], yp[2])
    keep = [0, 1, 3]
    with _spec_engine(spec, 3) as eng:
        eng.set_data(d["u_d"][keep], d["y_d"][keep])
        ref = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0[keep], up[keep], yp[keep], w[keep], n_mpc_step=nms)
    for a, r in zip((u_sys, y_sys, status, x_end, up_end, yp_end), ref):
        assert np.array_equal(a[keep], r)
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))


# Stopped mid-loop by the iteration cap: ROBUST + CONVEX four-tank, max_iter = 1, one solve per step.  With the cap at one
# the oracle reports solver_error at the first solve whose empty-active-set iterate leaves the slack box.  From the data
# tail that is solve 0 for 58 of seeds 0..63 and, with noise inside eps_max, never again: the uncapped oracle takes
# [2, 1, 1, 1, 1, 1, 1, 1, 1] solves on those and all ones on the other six.  So (i) the loops start one step later: `lead`
# steps of the uncapped oracle loop are applied first, and the state and windows they leave are what the capped loops
# (oracle and device) start from; (ii) two instances get one measurement outlier each, `spike` = {instance: (step,
# size)} added to the noise of output 0 (0.1 is absorbed by the unboxed slack of the window rows; 0.5 and 2.0 give the same
# stops): the solve after it sees a window the data cannot explain within the box.
# stop_at: the index of the first solve that reports solver_error per instance (None: never), as oracle_capped_loop()
# gives it on a CPU.
STOP = dict(seed0=0, B=4, lead=1, n_steps=8, max_iter=1, spike={1: (4, 0.5), 3: (1, 0.5)}, stop_at=[None, 5, None, 2])


def _stop_case():
    """Four-tank CONVEX batch and the start of the capped loops: (spec, d, x0, up, yp, w) after the lead steps."""
    g = STOP
    spec, d, up, yp, w = _four_tank(g["B"], g["seed0"], g["lead"] + g["n_steps"], slack_var_constraint_type=1)
    for b, (k, size) in g["spike"].items():
        w[b, g["lead"] + k, 0] += size
    x0 = np.empty_like(d["x_end"])
    for b in range(g["B"]):
        _, _, stop, x0[b], up[b], yp[b] = oracle_capped_loop(spec, d["u_d"][b], d["y_d"][b], d["x_end"][b], up[b], yp[b],
                                                             w[b, :g["lead"]], 1, 100)
        assert stop is None
    return spec, d, x0, up, yp, np.ascontiguousarray(w[:, g["lead"]:])


def oracle_capped_loop(spec, u_d, y_d, x0, up, yp, w, n_mpc_step, max_iter):
    """The loop of orc.closed_loop around orc.solve_fullspace(..., max_iter): an instance stops at the first solve that is
    not optimal.  Returns (u_sys, y_sys with NaN from the stop on, stop step or None, x, u_past, y_past at the stop)."""
    P = orc.FOUR_TANK
    plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
    plant.x = np.array(x0, float)
    up, yp = up.copy(), yp.copy()
    n_steps, m, p = w.shape[0], spec.m, spec.p
    u_sys = np.full((n_steps, m), np.nan)
    y_sys = np.full((n_steps, p), np.nan)
    for t in range(0, n_steps, n_mpc_step):
        sol = orc.solve_fullspace(spec, u_d, y_d, up, yp, max_iter=max_iter)
        if sol.status != orc.OPTIMAL:
            assert sol.status == orc.SOLVER_ERROR
            return u_sys, y_sys, t, plant.x, up, yp
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = sol.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys, None, plant.x, up, yp


@pytest.mark.parametrize("tag,path,cwl,kernel", [("per-step", "cold", False, PLANT), ("fused", "warm", True, FUSED_BOX)])
def test_instance_stopped_mid_loop_by_the_iteration_cap(gpu, tag, path, cwl, kernel):
    """Rows before an instance's stop match the oracle at the module's bars, rows from the stop on are NaN, status is
    solver_error (4) for the stopped instances and 0 for the others, and x / windows of a stopped instance are the oracle's
    at the stop.  Both device paths must stop where the oracle does."""
    g = STOP
    B, n_steps = g["B"], g["n_steps"]
    spec, d, x0, up, yp, w = _stop_case()
    refs = [oracle_capped_loop(spec, d["u_d"][b], d["y_d"][b], x0[b], up[b], yp[b], w[b], 1, g["max_iter"])
            for b in range(B)]
    stops = [r[2] for r in refs]
    assert stops == g["stop_at"]                                  # (the oracle's own figures, as recorded above)
    assert any(s is not None and s >= 1 for s in stops) and any(s is None for s in stops)
    P = orc.FOUR_TANK
    with _spec_engine(spec, B, max_iter=g["max_iter"]) as eng:
        if cwl:
            eng.set_convex_warm_law(True)
            eng.set_refinement("off")                             # (no refined law: the fused kernel serves the handle, see run_loop)
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_closed_loop_path(path)
        u_sys, y_sys, status, x_end, up_end, yp_end = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, up, yp, w,
                                                                      n_mpc_step=1)
        assert eng.closed_loop_kernel_name() == kernel
    assert [int(v) for v in status] == [0 if s is None else 4 for s in stops], (tag, status)
    for b in range(B):
        u_ref, y_ref, stop, x_ref, up_ref, yp_ref = refs[b]
        k = n_steps if stop is None else stop
        assert np.all(np.isnan(u_sys[b, k:])) and np.all(np.isnan(y_sys[b, k:])), (tag, b)
        assert np.all(np.isfinite(u_sys[b, :k])) and np.all(np.isfinite(y_sys[b, :k])), (tag, b)
        if k:
            eu = np.max(np.abs(u_sys[b, :k] - u_ref[:k])) / np.max(np.abs(u_ref[:k]))
            ey = np.max(np.abs(y_sys[b, :k] - y_ref[:k])) / max(1.0, np.max(np.abs(y_ref[:k])))
            print("%s instance %d (stop %s): u %.2e  y %.2e" % (tag, b, stop, eu, ey))
            assert eu < TOL_U and ey < TOL_Y, (tag, b, eu, ey)
        ysc = max(1.0, np.max(np.abs(y_ref[:k]))) if k else 1.0
        assert np.max(np.abs(x_end[b] - x_ref)) / ysc < TOL_Y, (tag, b)
        assert np.max(np.abs(up_end[b] - up_ref)) / np.max(np.abs(up_ref)) < TOL_U, (tag, b)
        assert np.max(np.abs(yp_end[b] - yp_ref)) / ysc < TOL_Y, (tag, b)
        # ... and bit for bit the tail of what the device itself applied before the stop
        assert np.array_equal(up_end[b], window_at(up[b], u_sys[b], k, 4)), (tag, b)
        assert np.array_equal(yp_end[b], window_at(yp[b], y_sys[b], k, 4)), (tag, b)
