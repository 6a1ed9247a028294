"""The yardstick of the safeguard tests (tests/_box_safeguard_ref.py), on the CPU: four-tank, L = 30, n = 4, N = 400, CONVEX
slack, terminal constraint, seeds 500 .. 531 at the data tail, box [0.8, 1.2] on both channels.  On the four instances where
the primal-dual rule of tests/_input_bounds_ref.py ends at a cap of 50, the primal active set converges and passes the
solver-independent KKT certificate; where the primal-dual rule converges, both give the same solution."""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc

import _box_safeguard_ref as sg
import _input_bounds_ref as ref

CONVERGING = (0, 1, 2, 3)


@pytest.mark.parametrize("b", sg.CYCLING)
def test_safeguarded_reference_solves_what_the_primal_dual_rule_cycles_on(b):
    pdas = sg.cached("pdas", 1, True, b, *sg.TIGHT, max_iter=50)
    assert pdas.status == orc.SOLVER_ERROR and pdas.iters == 50
    sol = sg.cached("safe", 1, True, b, *sg.TIGHT)
    nbox = sol.idx.size
    print("b=%d solves %d kmax %d k %d" % (b, sol.iters, sol.kmax, np.count_nonzero(sol.active)))
    assert sol.status == orc.OPTIMAL and sol.iters <= 4 * nbox + 16 and sol.kmax > 16
    spec = orc.spec_from_params(slack_var_constraint_type=1, tec=True)
    cert = ref.kkt_certificate(spec, *sg.instance(b), *sg.TIGHT, sol.x)
    tol = 1e-10 * cert["grad_scale"]
    assert cert["res_eq"] < tol and cert["res_box"] < tol and cert["res_stat"] < tol and cert["dual_sign"] < tol, cert


@pytest.mark.parametrize("b", CONVERGING)
def test_safeguarded_reference_agrees_with_the_primal_dual_rule_where_it_converges(b):
    pdas = sg.cached("pdas", 1, True, b, *sg.TIGHT, max_iter=50)
    assert pdas.status == orc.OPTIMAL and pdas.iters < 50
    sol = sg.cached("safe", 1, True, b, *sg.TIGHT)
    assert sol.status == orc.OPTIMAL and np.array_equal(sol.active, pdas.active)
    assert np.max(np.abs(sol.x - pdas.x)) <= 1e-9 * np.max(np.abs(pdas.x))
    assert abs(sol.cost - pdas.cost) <= 1e-9 * abs(pdas.cost)


def test_without_a_violated_bound_it_is_the_oracle_solve():
    spec = orc.spec_from_params(slack_var_constraint_type=0, tec=False)
    u_d, y_d, up, yp = sg.instance(0)
    got = sg.solve_safeguarded(spec, u_d, y_d, up, yp, -np.inf, np.inf)
    sol = orc.solve_fullspace(spec, u_d, y_d, up, yp)
    assert got.status == orc.OPTIMAL and got.iters == 1 and np.array_equal(got.x, sol.x)
