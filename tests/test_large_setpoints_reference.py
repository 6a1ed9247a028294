"""CPU premises of DDMPC_OPT_LARGE_SETPOINTS (tests/test_gpu_large_setpoints.py), from the oracle alone.

1. The setpoint-parametric law with the multi-hot S of tests/_setpoint_law_ref.py reproduces the full-space oracle at
   per-instance setpoints beyond 271 rows too, at the project bars (measured: 272 rows <= 8e-14 inputs / 6e-13 cost, 300 rows
   <= 6.4e-12 / 2.2e-10 with the law formed by QR, see _law_qr).
2. The crowded case of the limit test: four-tank L = 70, c = 0.01, setpoints rng(11 + b) -- every one of the six oracle solutions
   ends with more than 64 slack components at the bound (measured 77 .. 103).
"""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc

import _setpoint_law_ref as ref
import test_gpu_closed_loop_plants as plants                     # (the case constructors of the GPU tests: importing needs no GPU)
from test_gpu_round5 import _four_tank_long as _gpu_four_tank_long

TOL_U, TOL_COST = 1e-8, 1e-9


def _four_tank_long(B, L_, N, slack, c_box=1.0):
    spec, d, up, yp = _gpu_four_tank_long(B, L_, N, slack, c_box)
    return spec, d["u_d"], d["y_d"], up, yp


def _five_channel(B):
    # the 300-row plant of test_gpu_closed_loop_plants.LARGE, (m, p, ns, n, L) = (2, 3, 4, 2, 58), as the GPU tests build it
    g = plants.LARGE
    c = plants.make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], "none", B=B, n_steps=6)
    return c["spec"], c["u_d"], c["y_d"], c["up"], c["yp"]


def _setpoints(spec, B, du, dy, seed=11):
    rng = np.random.default_rng(seed)
    return spec.u_s + rng.uniform(-du, du, (B, spec.m)), spec.y_s + rng.uniform(-dy, dy, (B, spec.p))


def _law_qr(spec, u_d, y_d):
    """(P, S) of ref.law without squaring the condition number: K0 = A A' with A = [H, sqrt(lam D)], A' = Q R, so
    K0^-1 = R^-1 R^-T.  ref.law solves with the explicit Gram matrix; on the five-channel plant (cond K0 = 1e8) that puts the cost
    of ref.law_step at 4e-11 .. 9.6e-10 of the oracle's, the bar itself; this route measures <= 2.2e-10 there."""
    nat = ref.natural_of_internal(spec)
    _, _, lamD = ref.reduced_matrix(spec, u_d, y_d)
    H = np.vstack([orc.hankel_matrix(u_d, spec.Ln), orc.hankel_matrix(y_d, spec.Ln)])[nat]
    R = np.linalg.qr(np.hstack([H, np.diag(np.sqrt(lamD))]).T, mode="r")
    inv = lambda rhs: np.linalg.solve(R, np.linalg.solve(R.T, rhs))
    return inv(ref.past_hot(spec).T).T, inv(ref.multi_hot(spec).T).T


@pytest.mark.parametrize("rows", [272, 300])
def test_law_with_multi_hot_s_matches_oracle_beyond_271_rows(rows):
    B = 3
    if rows == 272:
        spec, u_d, y_d, up, yp = _four_tank_long(B, 64, 700, "none")
        us, ys = _setpoints(spec, B, 0.5, 0.2)
    else:
        spec, u_d, y_d, up, yp = _five_channel(B)
        us, ys = _setpoints(spec, B, 0.3, 0.3)
    assert (spec.m + spec.p) * (spec.L + spec.n) == rows
    hot = ref.multi_hot(spec)
    assert hot.shape == (spec.m + spec.p, rows) and np.all(hot.sum(axis=0) <= 1.0)
    for b in range(B):
        P, S = _law_qr(spec, u_d[b], y_d[b])
        u, cost = ref.law_step(spec, u_d[b], y_d[b], P, S, up[b], yp[b], us[b], ys[b])
        sol = orc.solve_fullspace(ref.with_setpoints(spec, us[b], ys[b]), u_d[b], y_d[b], up[b], yp[b])
        shared = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        assert sol.status == "optimal"
        eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(cost - sol.cost) / abs(sol.cost)
        moved = np.max(np.abs(sol.optimal_u - shared.optimal_u))
        print("rows %d b=%d eu %.2e ec %.2e, inputs move by %.2f against the shared setpoint" % (rows, b, eu, ec, moved))
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        assert moved > 1e-3                      # a wrong setpoint row cannot hide under the bars


def test_crowded_case_exceeds_64_switched_components():
    B = 6
    spec, u_d, y_d, up, yp = _four_tank_long(B, 70, 700, "convex", c_box=0.01)
    counts = []
    for b in range(B):
        us, ys = _setpoints(spec, 1, 0.5, 0.2, seed=11 + b)
        sol = orc.solve_fullspace(ref.with_setpoints(spec, us[0], ys[0]), u_d[b], y_d[b], up[b], yp[b])
        assert sol.status == "optimal"
        counts.append(int(np.sum(sol.active != 0)))
    print("slack components at the bound:", counts)
    assert min(counts) > 64, counts
