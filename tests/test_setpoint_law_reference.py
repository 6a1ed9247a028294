"""CPU checks of the algebra behind DDMPC_OPT_SETPOINT_LAW (tests/_setpoint_law_ref.py) against the full-space oracle, and of
the premise of the 128-row GPU case.  No device.

Bars are the project's: inputs 1e-8 of max|u_ref|, cost 1e-9 (TOL_U / TOL_COST of test_gpu_parity.py)."""
import numpy as np
import pytest

import _setpoint_law_ref as ref
from oracle import ddmpc_oracle as orc
from oracle import reduced_form as rf

TOL_U, TOL_COST = 1e-8, 1e-9


def test_multi_hot_columns_are_the_setpoint_rows_of_their_channel():
    for tec in (True, False):
        spec = orc.spec_from_params(slack_var_constraint_type=0, tec=tec)
        n, m, p, Ln = spec.n, spec.m, spec.p, spec.Ln
        hot, past = ref.multi_hot(spec), ref.past_hot(spec)
        assert hot.shape == (m + p, (m + p) * Ln) and past.shape == (n * (m + p), (m + p) * Ln)
        rho = np.arange((m + p) * Ln)
        for c in range(m + p):          # every prediction step (free or terminal) of channel c, no internal step
            assert np.array_equal(hot[c], ((rho % (m + p) == c) & (rho // (m + p) >= n)).astype(float))
        # every row takes its target from exactly one source: a past entry or a setpoint
        assert np.array_equal(hot.sum(axis=0) + past.sum(axis=0), np.ones((m + p) * Ln))


@pytest.mark.parametrize("tec", [True, False], ids=["terminal", "no-terminal"])
def test_law_matches_fullspace_oracle_at_per_instance_setpoints(tec):
    spec = orc.spec_from_params(slack_var_constraint_type=0, tec=tec)
    n = spec.n
    for seed in range(3):
        inst = orc.generate_instance(seed, N=400)
        u_d, y_d = inst["u_d"], inst["y_d"]
        up, yp = u_d[-n:].reshape(-1), y_d[-n:].reshape(-1)
        rng = np.random.default_rng(seed)
        us = spec.u_s + rng.uniform(-0.5, 0.5, spec.m)
        ys = spec.y_s + rng.uniform(-0.2, 0.2, spec.p)
        P, S = ref.law(spec, u_d, y_d)
        u, cost = ref.law_step(spec, u_d, y_d, P, S, up, yp, us, ys)
        sol = orc.solve_fullspace(ref.with_setpoints(spec, us, ys), u_d, y_d, up, yp)
        assert sol.status == orc.OPTIMAL
        eu = np.max(np.abs(u - sol.optimal_u.reshape(-1))) / np.max(np.abs(sol.optimal_u))
        ec = abs(cost - sol.cost) / abs(sol.cost)
        print("tec %s seed %d: u %.2e  cost %.2e" % (tec, seed, eu, ec))
        assert eu < TOL_U, (tec, seed, eu)
        assert ec < TOL_COST, (tec, seed, ec)


def test_schedule_loop_with_a_constant_schedule_is_the_oracle_loop():
    spec = orc.spec_from_params(slack_var_constraint_type=0)
    inst = orc.generate_instance(1, N=400)
    u_d, y_d = inst["u_d"], inst["y_d"]
    n_steps = 5
    w = spec.eps_max * np.random.default_rng(3).uniform(-1.0, 1.0, (n_steps, spec.p))
    x0 = inst["plant"].x.copy()
    for nms in (1, 2):
        pa, pb = orc.Plant(**orc.FOUR_TANK), orc.Plant(**orc.FOUR_TANK)
        pa.x, pb.x = x0.copy(), x0.copy()
        u_a, y_a = orc.closed_loop(spec, u_d, y_d, pa, w, n_mpc_step=nms)
        u_b, y_b, up, yp = ref.schedule_loop(spec, u_d, y_d, pb, w, np.tile(spec.u_s, (n_steps, 1)), np.tile(spec.y_s, (n_steps, 1)),
                                             n_mpc_step=nms)
        assert np.array_equal(u_a, u_b) and np.array_equal(y_a, y_b) and np.array_equal(pa.x, pb.x)
        assert np.array_equal(up, np.concatenate([u_d[-spec.n:], u_a])[-spec.n:].reshape(-1))
        assert np.array_equal(yp, np.concatenate([y_d[-spec.n:], y_a])[-spec.n:].reshape(-1))


def test_premise_of_the_128_row_gpu_case_unrefined_gram_route_misses_the_bar():
    # "ns=16" of tests/test_gpu_closed_loop_plants.py: K0 has a condition number of 5e10 .. 7e10 there, and the reduced form
    # solved through the explicit Gram matrix without refinement is more than 1e-8 from the oracle.  So an S taken from the
    # unrefined factor cannot meet TOL_U on this case: its GPU test runs under DDMPC_REFINE_ALWAYS and fails without refined
    # columns.  (Setpoints: the case's own and the schedule generator of the GPU test, rng(5), within +-0.3.)
    import test_gpu_closed_loop_plants as plants
    case, _ = plants._table_case("ns=16")
    s = case["spec"]
    rng = np.random.default_rng(5)
    for amp in (0.0, 0.3):
        for b in range(case["B"]):
            sp = ref.with_setpoints(s, s.u_s + amp * rng.uniform(-1, 1, s.m), s.y_s + amp * rng.uniform(-1, 1, s.p))
            sol = orc.solve_fullspace(sp, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b])
            red = rf.solve_reduced(sp, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b])
            err = np.max(np.abs(red["optimal_u"] - sol.optimal_u.reshape(-1))) / np.max(np.abs(sol.optimal_u))
            print("ns=16 amp %.1f instance %d: unrefined reduced form vs oracle %.2e" % (amp, b, err))
            # (at the case's own setpoints the three instances are at 6.4e-9, 1.2e-9, 1.4e-9: printed, not part of the premise;
            #  moved by up to 0.3 they are at 1.6e-8, 1.6e-8, 2.0e-8)
            if amp > 0.0:
                assert err > 1e-8, (amp, b, err)
