"""DDMPC_WEIGHT_DIAG beyond 271 rows: diagonal weighting matrices whose entries differ from step to step and from channel to
channel, and positive SEMI-definite ones, on every route that serves such controllers, each against an independent reference
(oracle.ddmpc_oracle.solve_fullspace for ROBUST controllers, oracle.nominal_exact.solve_nominal_model_based for NOMINAL ones on
exact data).

A multiple of the identity cannot show an indexing mistake: every index reads the same number.  The profiles below change with
the step and with the channel (no two steps of a channel and no two channels of a step share a value), so a reader of the weight
tables (ddmpc_api.hip `upload_params`: tabd[0], tabd[1], tabd[3], the position-order copy `wz`) that maps component -> step /
channel -> entry wrongly is percents away from the reference.
tests/test_oracle.py::test_premises_of_the_large_weight_tests shows on the CPU, for every (shape, scheme, slack) used here, that
each of five typical mistakes (MUTATIONS) moves optimal_u or the cost by at least 1000 bars.

Bars: the project's (test_gpu_parity.py): optimal_u 1e-8 of max|u_ref|, cost 1e-9 relative, status equal
to the reference's, under the slack box iters equal to the oracle's; variables as in
test_robust_scheme_beyond_the_register_resident_kernels (sigma 1e-9, ybar 1e-9, alpha 1e-8 relative; ubar holds optimal_u and
takes its bar).  Every instance of every batch is compared.  Every figure is printed before it is asserted.

Which kernel reads the weights in which case (the route is asserted in the case: `_robust_route` reads the route record of
ddmpc_debug_workspace; the NOMINAL pipelines are told apart by DDMPC_OPT_LARGE_PIPELINE being accepted and their results
differing in some bit):
  test_robust_solve_step_and_variables[phases]        rr3_shift_kernel, rr3_solve_kernel (Woodbury data under CONVEX), rr3_outputs,
                                                      rr3_refine_kernel where AUTO refines
  test_robust_solve_step_and_variables[one_workgroup] ddmpc_large_solve_kernel
  test_robust_crowded_active_set_...                  rr3_solve_kernel -> ddmpc_large_solve_kernel (hand-over)
  test_robust_affine_law (296 rows)                   ddmpc_rr3_law.hpp: the law step is asserted per instance (it differs from the
                                                      solve in some bit); the filtered re-solve for the instances that leave the box
  test_robust_affine_law_at_the_cfg5_size             AUTO: the step is the re-solve, gain() exercises the law; REFINE_OFF: the law step
  test_nominal_solve_and_step[phases]                 `wz` in ddmpc_rr2_solve.hpp / ddmpc_rr2.hpp
  test_nominal_solve_and_step[one_workgroup]          `wv` in ddmpc_nominal_rr_kernel
  test_nominal_affine_law                             the step kernel's cost from tabd[3] (ddmpc_rr2_solve.hpp)
  test_*_beyond_1024_rows                             the 1024-thread instances of the two one-workgroup kernels
  test_closed_loop_per_step                           prepare / step on the phase kernels with a moving window + ddmpc_plant_kernel
  (the bounded kernels, up to 271 rows and beyond: tests/test_gpu_bounded_weights.py -- the per-component box table)

Zero weights.  ROBUST: an unweighted output under the slack box has D0 = 1e25 + 1/lamb_sigma == D1 = 1e25 in fp64; its
multiplier is ~1e-25, its slack 0, it never reaches the bound and so never enters the switched set whose Woodbury data divide
by lam (D0 - D1) (test_robust_unweighted_boxed_outputs_never_switch).  NOMINAL: zeros on output entries only, every input
weighted, so the solution stays unique (premise: the weighted reduced matrix has full column rank).

Measured on an MI355X (worst relative error over every instance, pipeline, profile and slack type of a test; for information
-- the assertions use the bars above; u = optimal_u, c = cost):
  robust solve, 296 rows     u 5.6e-13  c 8.4e-14  sigma 1.1e-14  ybar 3.4e-13  alpha 1.1e-12
  robust solve, 300 rows     u 8.5e-13  c 1.4e-13  sigma 9.3e-14  ybar 6.0e-13  alpha 1.1e-11
  crowded active set         u 1.0e-13  c 7.1e-14  (75 .. 97 slacks at the bound per instance, the oracle's counts)
  unweighted boxed outputs   their slacks: 0 in the oracle, 8e-29 on the device (bound 1e-4)
  robust law step, 296 rows  u 3.3e-12  c 1.1e-12  gain 1.6e-11  (served by the law: every instance at NONE, the instances inside
                             the box at CONVEX -- two of three at the setpoint window, none at the data windows)
  robust, 608 rows, AUTO     the step is the re-solve on every instance: u 2.3e-9  c 2.3e-11;  gain 9.0e-10
  robust, 608 rows, OFF      the law serves every instance: step 5.3e-6 (u), 3.2e-6 (c) from the oracle, the unrefined cold solve
                             the same to three digits
  nominal solve              u 6.1e-13 / 1.1e-11 / 7.7e-10 (ramp), 7.3e-11 / 1.1e-11 / 5.7e-10 (zeros) at 315 / 296 / 405 rows  c 5.2e-14
  nominal law step, 608 rows u 1.1e-9   c 5.3e-14
  1100 rows (robust)         u 1.6e-13  c 9.4e-14      1029 rows (nominal)  u 7.7e-15  c 4.0e-15
  closed loop, 300 rows      u 1.8e-13  y 6.5e-14  x_end 2.1e-14
Sensitivity on the real code (scratch builds of rr3_outputs, not committed).  `tabd[3 * RPs + rho]` read as the weight of the
same channel at prediction step 0 (`tabd[3 * RPs + n (m + p) + rho % (m + p)]`): 15 of the 27 tests of this file fail (every ROBUST solve
and law case on the phase kernels, cost off by 2e-4 and more), and of the 144 earlier GPU tests beyond 271 rows only
test_global_workspace_kernels_with_channel_counts_that_do_not_fill_a_tile[m3p2-convex] notices.  Read as `tabd[3 * RPs]` the
same 15 fail, but so do 20 earlier tests: entry 0 belongs to a fixed component of the past window and holds 0, not a weight.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import engine as E
from direct_data_driven_mpc_amd import harness
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc
from oracle.nominal_exact import solve_nominal_model_based
import test_gpu_closed_loop_plants as CLP
from test_gpu_large_robust_law import REL_OFF, TOL_OFF, _cfg5_robust, _windows
from test_gpu_round3 import _config5
from test_gpu_round4 import _exact_plant_case
from test_gpu_round5 import _four_tank_long

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
TOL_SIGMA, TOL_YBAR, TOL_ALPHA = 1e-9, 1e-9, 1e-8


# ------------------------------------------------------------------------------------------------------ weight profiles
def ramp(spec):
    """q[kp*p+cy] = q0 (1 + 0.5 cy + kp/L), r[kp*m+ch] = r0 (1 + 0.5 ch + kp/L): strictly increasing along both axes,
    within a factor of about 4 of the scalar q0 = Q[0, 0], r0 = R[0, 0] the spec came with.  Returns (q [L, p], r [L, m])."""
    kp = np.arange(spec.L)[:, None] / spec.L
    q = float(spec.Q[0, 0]) * (1.0 + 0.5 * np.arange(spec.p)[None, :] + kp)
    r = float(spec.R[0, 0]) * (1.0 + 0.5 * np.arange(spec.m)[None, :] + kp)
    return q, r


def zeros(spec):
    """The ramp with entries set to 0.  ROBUST: one output channel unweighted at every third step and every third input step
    unweighted (the pattern of test_positive_semidefinite_diagonal_weights; lamb_alpha keeps the problem strictly convex).
    NOMINAL: output entries only, (step + channel) % 3 == 0 -- y is determined by x0 and u and all of u is penalised."""
    q, r = ramp(spec)
    if spec.robust:
        q[0::3, min(1, spec.p - 1)] = 0.0
        r[2::3, :] = 0.0
    else:
        kp, cy = np.meshgrid(np.arange(spec.L), np.arange(spec.p), indexing="ij")
        q[(kp + cy) % 3 == 0] = 0.0
    return q, r


PROFILES = {"ramp": ramp, "zeros": zeros}

# five typical indexing mistakes of a reader of a step-major weight table w [L, channels] (n: the steps of the past window)
MUTATIONS = {
    "entry 0 used everywhere": lambda w, n: np.full_like(w, w[0, 0]),
    "index shifted by n steps": lambda w, n: np.roll(w, -n, axis=0),
    "channel-major instead of step-major": lambda w, n: w.reshape(-1).reshape(w.shape[1], w.shape[0]).T.copy(),
    "channels swapped": lambda w, n: w[:, ::-1].copy(),
    "time reversed": lambda w, n: w[::-1].copy(),
}


def with_weights(spec, q, r):
    return dataclasses.replace(spec, Q=np.diag(np.asarray(q, float).reshape(-1)), R=np.diag(np.asarray(r, float).reshape(-1)))


def weighted(spec, profile):
    return with_weights(spec, *PROFILES[profile](spec))


# --------------------------------------------------------------------------------------------------------------- cases
def robust_case(shape, slack, B):
    """(spec with its scalar weights, N, u_d, y_d, u_past, y_past) of the ROBUST shapes used below."""
    if shape == "296":                                    # four-tank, L = 70; c = 0.05: the box binds (test_gpu_large_robust_law.py)
        spec, d, up, yp = _four_tank_long(B, 70, 700, slack, c_box=0.05)
        return spec, 700, d["u_d"], d["y_d"], up, yp
    if shape == "296-crowded":                            # c = 0.01: more than 64 slacks at the bound (test_gpu_round5.py)
        spec, d, up, yp = _four_tank_long(B, 70, 700, slack, c_box=0.01)
        return spec, 700, d["u_d"], d["y_d"], up, yp
    if shape == "300":                                    # (m, p, n, L) = (2, 3, 2, 58): m != p, five channels do not fill a tile
        g = CLP.LARGE
        case = CLP.make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], slack, B=B, n_steps=g["n_steps"], seed0=g["seed0"])
        return case["spec"], case["N"], case["u_d"], case["y_d"], case["up"], case["yp"]
    if shape == "608":                                    # the cfg-5 size
        spec, N, d, up, yp = _cfg5_robust(B, slack)
        return spec, N, d["u_d"], d["y_d"], up, yp
    assert shape == "1100"                                # four-tank, L = 271 (test_robust_scheme_beyond_1024_rows)
    N = 1400
    spec = orc.spec_from_params(L=271, N=N, slack_var_constraint_type=1 if slack == "convex" else 0)
    d = harness.generate_batch(range(B), N=N)
    up = d["u_d"][:, -spec.n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -spec.n:, :].reshape(B, -1).copy()
    return spec, N, d["u_d"], d["y_d"], up, yp


NOMINAL_SHAPES = {"5ch-315rows": (2, 3, 3, 60, 900), "4ch-296rows": (2, 2, 4, 70, 700), "9ch-405rows": (5, 4, 5, 40, 1200),
                  "3ch-1029rows": (1, 2, 3, 340, 1100)}
NOMINAL_SEED = {"5ch-315rows": 125, "4ch-296rows": 142, "9ch-405rows": 4, "3ch-1029rows": 31}


def nominal_case(shape, B):
    """(spec, plant, N, u_d, y_d, u_past, y_past): exact data of the seeded plants of test_large_nominal_pipelines_agree and
    test_nominal_scheme_beyond_1024_rows; "cfg5" is the shape of test_large_nominal_affine_law."""
    if shape == "cfg5":
        spec, plant, N, d, up, yp = _config5(B)
    else:
        m, p, n, Lh, N = NOMINAL_SHAPES[shape]
        spec, plant, d, up, yp = _exact_plant_case(NOMINAL_SEED[shape], m, p, n, Lh, N, B)
    return spec, plant, N, d["u_d"], d["y_d"], up, yp


# every (shape, scheme, slack) of the GPU cases below, for the premises test
ROBUST_USED = [("296", "none"), ("296", "convex"), ("296-crowded", "convex"), ("300", "none"), ("300", "convex"),
               ("608", "none"), ("608", "convex"), ("1100", "convex")]
NOMINAL_USED = ["5ch-315rows", "4ch-296rows", "9ch-405rows", "cfg5", "3ch-1029rows"]


def nominal_reduced_matrix(spec, plant, up, yp):
    """sqrt(W) * (Qb[R] @ Nn) of solve_nominal_model_based: the matrix whose least-squares problem fixes the solution."""
    one = solve_nominal_model_based(spec, plant, up, yp, _parts=True)
    return np.sqrt(one["W"])[:, None] * (one["Qb"][one["R"]] @ one["Vft"][one["kf"]:].T)


# --------------------------------------------------------------------------------------------------------------- engine
def _engine(spec, N, B, **kw):
    """A handle with the weights of `spec` handed over as 1-D arrays: DDMPC_WEIGHT_DIAG (asserted)."""
    q, r = np.diag(spec.Q).copy(), np.diag(spec.R).copy()
    assert np.array_equal(spec.Q, np.diag(q)) and np.array_equal(spec.R, np.diag(r))
    assert E._weights(q, spec.p * spec.L, "Q")[0] == L.WEIGHT_DIAG and E._weights(r, spec.m * spec.L, "R")[0] == L.WEIGHT_DIAG
    eng = BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=q, R=r, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                       controller_type=L.ROBUST if spec.robust else L.NOMINAL,
                       slack_type=L.SLACK_CONVEX if (spec.robust and spec.slack == "convex") else L.SLACK_NONE, eps_max=spec.eps_max,
                       lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec, **kw)
    assert eng.weight_kind == L.WEIGHT_DIAG               # what ddmpc_create was handed
    return eng


def _robust_route(eng):
    """The route of the last solve of a ROBUST handle beyond 271 rows, from ddmpc_debug_workspace's route record
    (test_debug_workspace_reads_the_route_of_the_last_solve): the phase kernels leave the rr3 record, the one-workgroup kernel
    leaves nothing this call reads."""
    na, nm = C.c_int64(-1), C.c_int64(-1)
    rc = L.load().ddmpc_debug_workspace(eng._h, 0, None, 0, None, 0, C.byref(na), C.byref(nm))
    if rc == L.ERR_NOT_READY:
        return "one_workgroup"
    L.check(rc)
    assert na.value == 0
    return "phases"


def _rel(a, b, floor=1e-300):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), floor))


def _oracle_batch(spec, u_d, y_d, up, yp):
    sols = [orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b]) for b in range(up.shape[0])]
    for s in sols:
        assert s.status == "optimal"
    return sols


def _check_robust(tag, spec, res, sols):
    """status, iters (slack box), optimal_u and cost of every instance against the full-space oracle."""
    u, cost, status, iters = res
    worst = [0.0, 0.0]
    for b, sol in enumerate(sols):
        eu, ec = _rel(u[b], sol.optimal_u), abs(cost[b] - sol.cost) / abs(sol.cost)
        worst = [max(worst[0], eu), max(worst[1], ec)]
        print("%s instance %d: status %d iters %d (oracle %d)  u %.2e  cost %.2e" % (tag, b, status[b], iters[b], sol.iters, eu, ec))
    print("%s worst: u %.2e  cost %.2e" % (tag, worst[0], worst[1]))
    for b, sol in enumerate(sols):
        assert L.STATUS_STRINGS[int(status[b])] == sol.status, (tag, b)
        if spec.slack == "convex":
            assert int(iters[b]) == sol.iters, (tag, b, int(iters[b]), sol.iters)
        assert _rel(u[b], sol.optimal_u) < TOL_U, (tag, b)
        assert abs(cost[b] - sol.cost) <= TOL_COST * abs(sol.cost), (tag, b)


def _check_robust_variables(tag, got, sols):
    err = {k: 0.0 for k in ("sigma", "ybar", "ubar", "alpha")}
    for b, sol in enumerate(sols):
        err["sigma"] = max(err["sigma"], np.max(np.abs(got["sigma"][b] - sol.sigma.ravel())) / max(1.0, np.max(np.abs(sol.sigma))))
        err["ybar"] = max(err["ybar"], np.max(np.abs(got["ybar"][b] - sol.ybar.ravel())))
        err["ubar"] = max(err["ubar"], _rel(got["ubar"][b], sol.ubar.ravel()))
        err["alpha"] = max(err["alpha"], np.max(np.abs(got["alpha"][b] - sol.alpha.ravel())) / max(1e-3, np.max(np.abs(sol.alpha))))
    print("%s variables: %s" % (tag, "  ".join("%s %.2e" % kv for kv in err.items())))
    assert err["sigma"] <= TOL_SIGMA and err["ybar"] <= TOL_YBAR and err["ubar"] < TOL_U and err["alpha"] <= TOL_ALPHA, (tag, err)


def _copy(res):
    return tuple(x.copy() for x in res)


def _bit_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. ROBUST, 272 .. 1024 rows, both pipelines
@pytest.mark.parametrize("profile", ["ramp", "zeros"])
@pytest.mark.parametrize("slack", ["none", "convex"])
@pytest.mark.parametrize("shape,B", [("296", 5), ("300", 3)])
def test_robust_solve_step_and_variables(gpu, shape, B, slack, profile):
    """ddmpc_solve, ddmpc_step after ddmpc_set_data (the solve on the kept factors: bit-equal, include/ddmpc.h) and
    ddmpc_get_solution on the phase kernels and on ddmpc_large_solve_kernel.  The zeros profile under CONVEX is the case of
    unweighted boxed outputs (D0 == D1 in fp64)."""
    spec0, N, u_d, y_d, up, yp = robust_case(shape, slack, B)
    spec = weighted(spec0, profile)
    assert (spec.m + spec.p) * (spec.L + spec.n) == int(shape)
    sols = _oracle_batch(spec, u_d, y_d, up, yp)
    if slack == "convex":
        assert max(s.iters for s in sols) >= 2            # the box binds: the Woodbury path of the phase kernels runs
    res = {}
    for pipe in ("phases", "one_workgroup"):
        tag = "%s/%s/%s/%s" % (shape, slack, profile, pipe)
        with _engine(spec, N, B) as eng:
            assert eng.kernel_name() == "ddmpc_large_solve_kernel"
            eng.set_large_pipeline(pipe)
            eng.set_data(u_d, y_d)
            res[pipe] = _copy(eng.solve(up, yp))
            assert _robust_route(eng) == pipe
            got = {k: eng.get_solution(k) for k in ("sigma", "ybar", "ubar", "alpha")}
            eng.set_data(u_d, y_d)
            w = _copy(eng.step(up, yp))
            assert _robust_route(eng) == pipe
        _check_robust(tag, spec, res[pipe], sols)
        assert _bit_equal(w, res[pipe]), tag
        _check_robust_variables(tag, got, sols)
    assert np.array_equal(res["phases"][2], res["one_workgroup"][2])
    if slack == "convex":
        assert np.array_equal(res["phases"][3], res["one_workgroup"][3])


# ---------------------------------------------------------------- 2. ROBUST, crowded active set: the hand-over carries the weights
def test_robust_crowded_active_set_hands_the_weights_to_the_fall_back(gpu):
    """c = 0.01 at 296 rows with the ramp profile: more than 64 slacks reach their bound on some instance, the phase solve marks
    it and ddmpc_large_solve_kernel finishes it (test_large_robust_phase_kernels_hand_crowded_active_sets_to_the_fall_back)."""
    B = 6
    spec0, N, u_d, y_d, up, yp = robust_case("296-crowded", "convex", B)
    spec = weighted(spec0, "ramp")
    sols = _oracle_batch(spec, u_d, y_d, up, yp)
    with _engine(spec, N, B) as eng:
        eng.set_data(u_d, y_d)
        res = _copy(eng.solve(up, yp))
        assert _robust_route(eng) == "phases"
        sg = eng.get_solution("sigma")
    nact = np.sum(np.abs(sg[:, spec.n * spec.p:]) >= spec.c * spec.eps_max * (1 - 1e-12), axis=1)
    print("slacks at the bound per instance:", nact, " oracle:", [int(np.count_nonzero(s.active)) for s in sols])
    assert nact.max() > 64, nact                          # the fall-back did serve at least one instance
    _check_robust("296-crowded/ramp", spec, res, sols)


# ---------------------------------------------------------------- 3. ROBUST, unweighted boxed outputs under CONVEX
@pytest.mark.parametrize("pipe", ["phases", "one_workgroup"])
def test_robust_unweighted_boxed_outputs_never_switch(gpu, pipe):
    """An output with Q entry 0 is free: ybar absorbs it and its slack is 0 in the reference's solution.  On the device its
    multiplier is ~1e-25 (1/w = 1e25), so its slack never reaches c * eps_max and it never joins the switched set of
    rr3_solve_kernel, whose Woodbury data divide by lam (D0 - D1) = 0 for such a component.  Parity with the oracle on both
    pipelines, and the slacks of the unweighted components at 0 within the sigma bar in the oracle and on the device."""
    B = 5
    spec0, N, u_d, y_d, up, yp = robust_case("296", "convex", B)
    spec = weighted(spec0, "zeros")
    q = np.diag(spec.Q).reshape(spec.L, spec.p)
    free = np.concatenate([np.zeros((spec.n, spec.p), bool), q == 0.0]).reshape(-1)          # sigma's order: step-major, all L + n steps
    free[spec.L * spec.p:] = False                        # the terminal window: ybar is fixed there, Q is not read, the slack is live
    assert spec.tec and free.sum() == len(range(0, spec.L - spec.n, 3))
    sols = _oracle_batch(spec, u_d, y_d, up, yp)
    assert max(s.iters for s in sols) >= 2
    with _engine(spec, N, B) as eng:
        eng.set_large_pipeline(pipe)
        eng.set_data(u_d, y_d)
        res = _copy(eng.solve(up, yp))
        assert _robust_route(eng) == pipe
        sg = eng.get_solution("sigma")
    _check_robust("296/convex/zeros/%s" % pipe, spec, res, sols)
    for b, sol in enumerate(sols):
        so, sd = np.max(np.abs(sol.sigma.ravel()[free])), np.max(np.abs(sg[b][free]))
        print("instance %d: largest slack of an unweighted output: oracle %.2e  device %.2e  (bound %.1e)"
              % (b, so, sd, spec.c * spec.eps_max))
        assert so <= TOL_SIGMA and sd <= TOL_SIGMA
    assert np.max(np.abs(sg[:, spec.n * spec.p:])) <= spec.c * spec.eps_max * (1 + 1e-12)


# ---------------------------------------------------------------- 4. ROBUST affine law
def _data_windows(u_d, y_d, n, offsets):
    """Past windows taken from the data trajectories themselves at `offsets` [B]: windows the plant does produce."""
    B = u_d.shape[0]
    return (np.stack([u_d[b, o:o + n].reshape(-1) for b, o in enumerate(offsets)]),
            np.stack([y_d[b, o:o + n].reshape(-1) for b, o in enumerate(offsets)]))


def _gain_against_oracle(tag, spec, u_d, y_d, g, w1, w2):
    """ddmpc_get_gain against the oracle: beta is affine in the window w, so the oracle's solutions at two windows fix it on the
    line through them; H'(g0 + G'w) must be the oracle's alpha at both and at a third window of that line (worst relative error)."""
    B, n = u_d.shape[0], spec.n
    assert g.shape == (B, n * (spec.m + spec.p) + 1, (spec.m + spec.p) * (spec.L + n))
    (u1, y1), (u2, y2) = w1, w2
    w3 = (u1 + 1.7 * (u2 - u1), y1 + 1.7 * (y2 - y1))
    worst = 0.0
    for b in range(B):
        H = orc.hankel_matrix(np.concatenate([u_d[b], y_d[b]], axis=1), spec.L + n)
        a = [orc.solve_fullspace(spec, u_d[b], y_d[b], u_[b], y_[b]).alpha.ravel() for u_, y_ in (w1, w2, w3)]
        sc = max(1e-3, max(np.max(np.abs(x)) for x in a))
        assert np.max(np.abs(a[2] - (a[0] + 1.7 * (a[1] - a[0])))) <= 1e-9 * sc      # the oracle's own law is affine
        for (u_, y_), al in zip((w1, w2, w3), a):
            w = np.concatenate([u_[b], y_[b]])
            worst = max(worst, np.max(np.abs(H.T @ (g[b, 0] + g[b, 1:].T @ w) - al)) / max(1e-3, np.max(np.abs(al))))
    print("%s gain: H'(g0 + G'w) against the oracle's alpha, worst %.2e" % (tag, worst))
    return worst


def _law_windows(spec, N, u_d, y_d, up, yp):
    """The data tail, two windows taken at random places of the data, and one near the setpoint (inside the slack box)."""
    rng = np.random.default_rng(41)
    B = up.shape[0]
    return ([(up, yp)] + [_data_windows(u_d, y_d, spec.n, rng.integers(0, N - spec.n, B)) for _ in range(2)]
            + [_windows(None, up, yp, spec, "setpoint")])


def _law_steps(eng, wins):
    out = []
    for u_, y_ in wins:
        t = _copy(eng.step(u_, y_))
        assert _robust_route(eng) == "phases"
        out.append((_copy(eng.solve(u_, y_)), t))
    return out


def _differs(s, t):
    """Per instance: the step differs from the solve at the same window in some bit of optimal_u or the cost.  The filtered
    re-solve of a law step is the solve on the kept factors, bit-equal to ddmpc_solve; a step served by the law
    (rr3_law_step_kernel) is another computation and is not."""
    return np.any(t[0] != s[0], axis=1) | (t[1] != s[1])


@pytest.mark.parametrize("profile", ["ramp", "zeros"])
@pytest.mark.parametrize("slack", ["none", "convex"])
def test_robust_affine_law(gpu, profile, slack):
    """DDMPC_OPT_LARGE_AFFINE_LAW on the phase kernels at 296 rows: ddmpc_prepare, then ddmpc_step at the data tail, at two windows
    taken at random places of the data and at one near the setpoint, against the oracle.  Which computation served an instance
    is asserted per window.  NONE: every instance is on the law -- its step differs from ddmpc_solve in some bit
    (test_slack_none_step_at_296_rows).  CONVEX: the instances the oracle solves in one iteration stay in the box and are on the
    law; the others are re-solved on the kept factors, bit-equal to ddmpc_solve with its status and iteration count; both kinds
    occur.  NONE: ddmpc_get_gain against the oracle."""
    B = 3
    spec0, N, u_d, y_d, up, yp = robust_case("296", slack, B)
    spec = weighted(spec0, profile)
    wins = _law_windows(spec, N, u_d, y_d, up, yp)
    with _engine(spec, N, B) as eng:
        eng.set_large_affine_law(True)                    # (refused for dense weights: this handle is DDMPC_WEIGHT_DIAG)
        eng.set_data(u_d, y_d)
        eng.prepare()
        g = eng.gain()
        out = _law_steps(eng, wins)
    n_law = n_resolve = 0
    for k, ((u_, y_), (s, t)) in enumerate(zip(wins, out)):
        tag = "296/%s/%s/law window %d" % (slack, profile, k)
        sols = _oracle_batch(spec, u_d, y_d, u_, y_)
        _check_robust(tag + " step", spec, t, sols)
        _check_robust(tag + " solve", spec, s, sols)
        assert np.array_equal(s[2], t[2]) and np.array_equal(s[3], t[3]), tag
        on_law = np.array([max(so.iters, 1) == 1 for so in sols])
        diff = _differs(s, t)
        print("%s: on the law by the oracle's iteration counts %s, step differs from the solve %s" % (tag, on_law, diff))
        assert np.array_equal(diff, on_law), tag           # the law served exactly the instances inside the box
        n_law += int(on_law.sum()); n_resolve += int((~on_law).sum())
    assert n_law > 0 and (slack == "none" or n_resolve > 0)
    if slack == "none":
        assert n_resolve == 0
        assert _gain_against_oracle("296/" + profile, spec, u_d, y_d, g, wins[0], wins[1]) <= TOL_ALPHA


@pytest.mark.parametrize("slack", ["none", "convex"])
def test_robust_affine_law_at_the_cfg5_size(gpu, slack):
    """608 rows, ramp.  Under the default refinement (AUTO) no law of this size reaches the residual threshold
    (test_slack_none_step_at_the_cfg5_size), so a step there is the re-solve on the kept factors: that leg checks the step at the
    project's bars whatever served it (the fraction is printed) and, at NONE, ddmpc_get_gain -- the law itself, whose refinement
    reads lam * tabd[0] -- against the oracle.  With DDMPC_REFINE_OFF the law serves every instance inside the box (the second leg,
    as test_cfg5_size_refinement_off_law_serves and with its bars: step and cold solve both on the unrefined factor, REL_OFF
    apart; the step no further from the oracle than that solve plus REL_OFF, or TOL_OFF).  Those bars are 1e-7 .. 1e-5: three
    orders and more below what an indexing mistake moves (tests/test_oracle.py)."""
    B = 3
    spec0, N, u_d, y_d, up, yp = robust_case("608", slack, B)
    spec = weighted(spec0, "ramp")
    wins = _law_windows(spec, N, u_d, y_d, up, yp)
    with _engine(spec, N, B) as eng:
        eng.set_large_affine_law(True)
        eng.set_data(u_d, y_d)
        eng.prepare()
        g = eng.gain()
        out = _law_steps(eng, wins[:3])
    for k, ((u_, y_), (s, t)) in enumerate(zip(wins, out)):
        tag = "608/%s/ramp/auto window %d" % (slack, k)
        sols = _oracle_batch(spec, u_d, y_d, u_, y_)
        _check_robust(tag + " step", spec, t, sols)
        assert np.array_equal(s[2], t[2]) and np.array_equal(s[3], t[3]), tag
        print("%s: step differs from the solve (served by the law) %s" % (tag, _differs(s, t)))
    if slack == "none":
        assert _gain_against_oracle("608/ramp/auto", spec, u_d, y_d, g, wins[0], wins[1]) <= TOL_ALPHA
    # refinement off: the law serves
    off_wins = wins[:3] if slack == "none" else wins[3:]  # (CONVEX: the data windows all leave the box at this size)
    with _engine(spec, N, B) as eng:
        eng.set_refinement("off")
        eng.set_large_affine_law(True)
        eng.set_data(u_d, y_d)
        eng.prepare()
        out = _law_steps(eng, off_wins)
    for k, ((u_, y_), (s, t)) in enumerate(zip(off_wins, out)):
        tag = "608/%s/ramp/off window %d" % (slack, k)
        assert np.all(s[2] == 0) and np.array_equal(s[2], t[2]) and np.array_equal(s[3], t[3]), tag
        sel = t[3] == 1
        diff = _differs(s, t)
        print("%s: iters %s, step differs from the solve %s" % (tag, t[3], diff))
        assert sel.all() and diff.all(), tag               # every instance inside the box, every one served by the law
        assert _rel(t[0], s[0]) <= REL_OFF and np.max(np.abs(t[1] - s[1]) / np.abs(s[1])) <= REL_OFF, tag
        for b in range(B):
            sol = orc.solve_fullspace(spec, u_d[b], y_d[b], u_[b], y_[b])
            assert sol.status == "optimal" and max(sol.iters, 1) == 1
            eu, ec = _rel(s[0][b], sol.optimal_u), abs(s[1][b] - sol.cost) / abs(sol.cost)
            tu, tc = _rel(t[0][b], sol.optimal_u), abs(t[1][b] - sol.cost) / abs(sol.cost)
            print("%s instance %d: unrefined solve u %.2e cost %.2e   law step u %.2e cost %.2e" % (tag, b, eu, ec, tu, tc))
            assert eu < 1e-4 and ec < 1e-4, (tag, b)       # (the unrefined cold solve itself)
            assert tu <= max(TOL_OFF, eu + REL_OFF) and tc <= max(TOL_OFF, ec + REL_OFF), (tag, b)


# ---------------------------------------------------------------- 5. NOMINAL, 272 .. 1024 rows, both pipelines
def _check_nominal(tag, spec, plant, up, yp, res):
    u, cost, status, _ = res
    worst = [0.0, 0.0]
    refs = [solve_nominal_model_based(spec, plant, up[b], yp[b]) for b in range(up.shape[0])]
    for b, mod in enumerate(refs):
        eu, ec = _rel(u[b], mod["optimal_u"]), abs(cost[b] - mod["cost"]) / abs(mod["cost"])
        worst = [max(worst[0], eu), max(worst[1], ec)]
        print("%s instance %d: status %d  u %.2e  cost %.2e" % (tag, b, status[b], eu, ec))
    print("%s worst: u %.2e  cost %.2e" % (tag, worst[0], worst[1]))
    for b, mod in enumerate(refs):
        assert mod["feas_residual"] < 1e-10
        assert L.STATUS_STRINGS[int(status[b])] == "optimal", (tag, b, status)
        assert _rel(u[b], mod["optimal_u"]) < TOL_U, (tag, b)
        assert abs(cost[b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), (tag, b)


@pytest.mark.parametrize("profile", ["ramp", "zeros"])
@pytest.mark.parametrize("shape,B", [("5ch-315rows", 5), ("4ch-296rows", 3), ("9ch-405rows", 3)])
def test_nominal_solve_and_step(gpu, shape, B, profile):
    """Exact data of the seeded plants of test_large_nominal_pipelines_agree: ddmpc_solve against the model-based solution, the
    step on the kept factors bit-equal, ubar[n*m:] == optimal_u, and the two pipelines against each other at that test's bars."""
    spec0, plant, N, u_d, y_d, up, yp = nominal_case(shape, B)
    spec = weighted(spec0, profile)
    n, m = spec.n, spec.m
    res = {}
    for pipe in ("phases", "one_workgroup"):
        tag = "%s/%s/%s" % (shape, profile, pipe)
        with _engine(spec, N, B) as eng:
            assert (m + spec.p) * (spec.L + n) > 271 and "nominal_rr" in eng.kernel_name()
            eng.set_large_pipeline(pipe)                  # (one_workgroup refuses dense weights: this handle is DDMPC_WEIGHT_DIAG)
            eng.set_data(u_d, y_d)
            res[pipe] = _copy(eng.solve(up, yp))
            ub = eng.get_solution("ubar")
            eng.set_data(u_d, y_d)
            w = _copy(eng.step(up, yp))
        _check_nominal(tag, spec, plant, up, yp, res[pipe])
        assert _bit_equal(w, res[pipe]), tag
        assert np.array_equal(ub[:, n * m:], res[pipe][0]), tag
    a, b_ = res["phases"], res["one_workgroup"]
    eu, ec = _rel(a[0], b_[0]), np.max(np.abs(a[1] - b_[1]) / np.abs(b_[1]))
    print("%s/%s pipelines against each other: u %.2e  cost %.2e" % (shape, profile, eu, ec))
    assert eu < 1e-8 and ec < 1e-10
    # NOMINAL handles leave no route record: that the option selected another implementation is shown by proxy -- the two round
    # differently, so their results differ in some bit (should they ever agree to the bit, this line needs another witness)
    assert not np.array_equal(a[0], b_[0])


# ---------------------------------------------------------------- 6. NOMINAL affine law
def test_nominal_affine_law(gpu):
    """DDMPC_OPT_LARGE_AFFINE_LAW on the cfg-5 shape with the ramp profile: ddmpc_step (the law of z, its cost summed from the weight
    table per free component) at two consistent windows against the model-based solution; ddmpc_get_gain reproduces z =
    [ubar; ybar] of a step at a third window, whose optimal_u meets the reference."""
    B = 3
    spec0, plant, N, u_d, y_d, up, yp = nominal_case("cfg5", B)
    spec = weighted(spec0, "ramp")
    n, m, p = spec.n, spec.m, spec.p
    wins = [(up, yp), _data_windows(u_d, y_d, n, [100] * B), _data_windows(u_d, y_d, n, [731, 17, 1205])]
    with _engine(spec, N, B) as eng:
        eng.set_large_affine_law(True)
        eng.set_data(u_d, y_d)
        eng.prepare()
        g = eng.gain()
        out = []
        for u_, y_ in wins:
            t = _copy(eng.step(u_, y_))
            out.append((t, eng.get_solution("ubar"), eng.get_solution("ybar")))
        cold = _copy(eng.solve(*wins[0]))
    for k, ((u_, y_), (t, ub, yb)) in enumerate(zip(wins, out)):
        _check_nominal("cfg5/ramp/law window %d" % k, spec, plant, u_, y_, t)
        assert np.array_equal(ub[:, n * m:], t[0])
    assert not np.array_equal(cold[0], out[0][0][0])      # the step ran on the law, not on the kept factors
    (u3, y3), (t3, ub3, yb3) = wins[2], out[2]
    z = g[:, 0, :] + np.einsum("bjr,bj->br", g[:, 1:, :], np.concatenate([u3, y3], axis=1))
    zz = z.reshape(B, spec.L + n, m + p)
    eu, ey = _rel(zz[:, :, :m].reshape(B, -1), ub3), _rel(zz[:, :, m:].reshape(B, -1), yb3)
    print("cfg5/ramp gain against the step at the third window: ubar %.2e  ybar %.2e" % (eu, ey))
    assert eu < 1e-9 and ey < 1e-9                        # (the bars of test_large_nominal_affine_law)
    for b in range(B):
        mod = solve_nominal_model_based(spec, plant, u3[b], y3[b])
        assert _rel(zz[b, n:, :m].reshape(-1), mod["optimal_u"]) < TOL_U, b


# ---------------------------------------------------------------- 7. beyond 1024 rows
def test_robust_beyond_1024_rows(gpu):
    """Four-tank, L = 271 (1100 rows), CONVEX, ramp: the 1024-thread instance of ddmpc_large_solve_kernel.  Both instances."""
    B = 2
    spec0, N, u_d, y_d, up, yp = robust_case("1100", "convex", B)
    spec = weighted(spec0, "ramp")
    sols = _oracle_batch(spec, u_d, y_d, up, yp)
    with _engine(spec, N, B) as eng:
        assert (spec.m + spec.p) * (spec.L + spec.n) == 1100 and "large_solve" in eng.kernel_name()
        eng.set_data(u_d, y_d)
        res = _copy(eng.solve(up, yp))
        assert _robust_route(eng) == "one_workgroup"
        sg = eng.get_solution("sigma")
        eng.set_data(u_d, y_d)
        w = _copy(eng.step(up, yp))
    _check_robust("1100/convex/ramp", spec, res, sols)
    assert _bit_equal(w, res)
    for b, sol in enumerate(sols):
        assert np.max(np.abs(sg[b] - sol.sigma.ravel())) <= TOL_SIGMA * max(1.0, np.max(np.abs(sol.sigma)))


def test_nominal_beyond_1024_rows(gpu):
    """The 1024-thread instance of ddmpc_nominal_rr_kernel against the model-based solution, ramp, both instances.  Not the SISO
    plant of test_nominal_scheme_beyond_1024_rows: with one input and one output the ramp scales q and r of a step by the same
    factor, q[k] / r[k] stays q0 / r0 and a wrong index moves optimal_u by 5e-8 only (the premises test refused it).  The
    three-channel plant of test_nominal_phase_pipeline_gram_with_several_lags_per_tile (seed 31) with L = 340: 1029 rows."""
    B = 2
    spec0, plant, N, u_d, y_d, up, yp = nominal_case("3ch-1029rows", B)
    spec = weighted(spec0, "ramp")
    with _engine(spec, N, B) as eng:
        assert (spec.m + spec.p) * (spec.L + spec.n) == 1029 and "nominal_rr" in eng.kernel_name()
        eng.set_data(u_d, y_d)
        res = _copy(eng.solve(up, yp))
        eng.set_data(u_d, y_d)
        w = _copy(eng.step(up, yp))
    _check_nominal("3ch-1029rows/ramp", spec, plant, up, yp, res)
    assert np.array_equal(w[2], res[2]) and _rel(w[0], res[0]) <= 1e-9      # (as in test_nominal_scheme_beyond_1024_rows)


# ---------------------------------------------------------------- 8. per-step closed loop beyond 271 rows
def closed_loop_case():
    """The LARGE case of test_gpu_closed_loop_plants.py (300 rows, CONVEX, n_mpc_step = 2, 6 steps) with the ramp profile."""
    case = CLP._large_case()
    case["spec"] = weighted(case["spec"], "ramp")
    return case


def test_closed_loop_per_step(gpu):
    """ddmpc_closed_loop at 300 rows with m != p and D != 0: prepare / step on the phase kernels with a moving window and
    ddmpc_plant_kernel, against orc.closed_loop with the bars of test_gpu_closed_loop_plants.py."""
    case = closed_loop_case()
    s, pl, nms = case["spec"], case["plant"], CLP.LARGE["nms"]
    assert (s.m + s.p) * (s.L + s.n) == 300
    with _engine(s, case["N"], case["B"]) as eng:
        eng.set_data(case["u_d"], case["y_d"])
        out = eng.closed_loop(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"], n_mpc_step=nms)
        assert eng.closed_loop_kernel_name() == CLP.PLANT
        assert _robust_route(eng) == "phases"
    CLP.check_against_oracle(case, out, nms, "300rows/ramp")
