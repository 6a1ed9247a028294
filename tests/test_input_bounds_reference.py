"""The yardstick of the input-bound tests (tests/_input_bounds_ref.py), on the CPU: without finite bounds it is the oracle's
own solve, and on bounded four-tank problems its solution passes a solver-independent KKT certificate."""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc

import _input_bounds_ref as ref


def _instance(seed, n=4):
    d = orc.generate_instance(seed)
    return d["u_d"], d["y_d"], d["u_d"][-n:].reshape(-1), d["y_d"][-n:].reshape(-1)


@pytest.mark.parametrize("slack", [0, 1])
def test_infinite_bounds_are_the_oracle_solve(slack):
    spec = orc.spec_from_params(slack_var_constraint_type=slack)
    u_d, y_d, up, yp = _instance(500)
    sol = orc.solve_fullspace(spec, u_d, y_d, up, yp)
    got = ref.solve_bounded(spec, u_d, y_d, up, yp, -np.inf, np.inf)
    assert np.array_equal(got.x, sol.x) and got.cost == sol.cost and got.iters == sol.iters and got.status == sol.status
    assert np.array_equal(got.active, sol.active)


@pytest.mark.parametrize("slack,tec", [(1, True), (0, False)])
@pytest.mark.parametrize("seed", [500, 501, 502, 503])
def test_bounded_solution_passes_the_kkt_certificate(seed, slack, tec):
    spec = orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)
    u_d, y_d, up, yp = _instance(seed)
    sol = ref.solve_bounded(spec, u_d, y_d, up, yp, 0.0, 2.0)
    assert sol.status == "optimal" and sol.iters >= 2 and np.count_nonzero(sol.active) > 16
    pred = sol.optimal_u[:(spec.L - spec.n if tec else spec.L) * spec.m]
    assert pred.min() >= 0.0 and pred.max() <= 2.0
    cert = ref.kkt_certificate(spec, u_d, y_d, up, yp, 0.0, 2.0, sol.x)
    tol = 1e-9 * cert["grad_scale"]
    assert cert["res_eq"] < tol and cert["res_box"] < tol and cert["res_stat"] < tol and cert["dual_sign"] < tol, cert
