"""The yardstick of the warm-start tests (tests/_box_warm_ref.py), on the CPU: four-tank, L = 30, n = 4, N = 400, CONVEX slack,
terminal constraint, box [0, 2] on both channels, seeds 500 and 501 from the data tail.  With an empty seed the helper is
`solve_bounded`; seeded with the optimal set it takes the law and one solve; over six closed-loop steps that carry the set it
takes the solve counts DESIGN 5.5 tabulates, converges at every step and applies the inputs of the empty start."""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc

import _box_warm_ref as wref
import _input_bounds_ref as ref

LO, HI = 0.0, 2.0
N_STEPS = 6
# solves per step (1 = the law, + 1 per solve of a non-empty set), cap 50: DESIGN 5.5, "Warm start"
SEEDED = {500: [10, 3, 4, 4, 4, 3], 501: [11, 4, 3, 4, 4, 3]}
EMPTY = {500: [10, 9, 10, 9, 9, 8], 501: [11, 11, 11, 11, 9, 8]}

_LOOPS = {}


def _spec():
    return orc.spec_from_params(slack_var_constraint_type=1, tec=True)


def _loop(seed, carry):
    """Six closed-loop steps of instance `seed` from the data tail, computed once."""
    if (seed, carry) not in _LOOPS:
        d = orc.generate_instance(seed)
        w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (10, 2))[:N_STEPS]
        _LOOPS[(seed, carry)] = (d, wref.closed_loop_seeded(_spec(), d["u_d"], d["y_d"], d["plant"], w, LO, HI, max_iter=50,
                                                             carry=carry))
    return _LOOPS[(seed, carry)]


def test_an_empty_seed_is_solve_bounded():
    d = orc.generate_instance(500)
    up, yp = d["u_d"][-4:].reshape(-1), d["y_d"][-4:].reshape(-1)
    sol = ref.solve_bounded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI)
    for seed in (None, np.zeros(sol.idx.size, dtype=int)):
        got = wref.solve_seeded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI, seed)
        assert not got.seeded and not got.fell_back
        assert got.status == sol.status == orc.OPTIMAL and got.iters == sol.iters and got.margin == sol.margin
        assert np.array_equal(got.x, sol.x) and np.array_equal(got.active, sol.active)


def test_seeded_with_the_optimal_set_it_takes_the_law_and_one_solve():
    d = orc.generate_instance(500)
    up, yp = d["u_d"][-4:].reshape(-1), d["y_d"][-4:].reshape(-1)
    sol = ref.solve_bounded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI)
    assert sol.iters > 2 and np.any(sol.active)
    got = wref.solve_seeded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI, sol.active)
    assert got.seeded and not got.fell_back and got.status == orc.OPTIMAL and got.iters == 2
    assert np.array_equal(got.active, sol.active)
    assert np.max(np.abs(got.x - sol.x)) <= 1e-12 * np.max(np.abs(sol.x))
    assert 0.0 < got.margin < np.inf


def test_a_seed_that_does_not_converge_within_the_cap_falls_back_to_the_empty_start():
    d = orc.generate_instance(500)
    up, yp = d["u_d"][-4:].reshape(-1), d["y_d"][-4:].reshape(-1)
    sol = ref.solve_bounded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI)
    bad = -sol.active                                   # every active component at the wrong bound
    bad[sol.active == 0] = 1                            # ... and every other one at its upper bound
    cap = sol.iters
    got = wref.solve_seeded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI, bad, max_iter=cap)
    cold = ref.solve_bounded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI, max_iter=cap)
    assert cold.status == orc.OPTIMAL
    if got.fell_back:                                   # the seeded run spent cap - 1 solves, then the empty start its own
        assert got.iters == cap - 1 + cold.iters and np.array_equal(got.x, cold.x)
    assert got.seeded and got.status == orc.OPTIMAL and np.array_equal(got.active, sol.active)
    assert got.margin <= cold.margin or not got.fell_back
    # a seed of another box list is refused, not read
    with pytest.raises(ValueError):
        wref.solve_seeded(_spec(), d["u_d"], d["y_d"], up, yp, LO, HI, np.ones(3, dtype=int))


@pytest.mark.parametrize("seed", sorted(SEEDED))
def test_closed_loop_that_carries_the_set(seed):
    d, (u_w, y_w, sols_w) = _loop(seed, True)
    _, (u_c, y_c, sols_c) = _loop(seed, False)
    print("seed %d seeded %s empty %s margins %s" % (seed, [s.iters for s in sols_w], [s.iters for s in sols_c],
                                                     ["%.1e" % s.margin for s in sols_w]))
    assert len(sols_w) == len(sols_c) == N_STEPS
    assert all(s.status == orc.OPTIMAL and not s.fell_back for s in sols_w)
    assert all(s.status == orc.OPTIMAL for s in sols_c)
    assert [s.iters for s in sols_w] == SEEDED[seed]
    assert [s.iters for s in sols_c] == EMPTY[seed]
    assert not sols_w[0].seeded and all(s.seeded for s in sols_w[1:])
    assert np.max(np.abs(u_w - u_c)) <= 1e-12 and np.max(np.abs(y_w - y_c)) <= 1e-12
    for s in sols_w:                                    # the margin of every solve made
        assert 0.0 < s.margin < np.inf
    # the loop with carry = False is closed_loop_bounded
    plant = orc.generate_instance(seed)["plant"]        # (its state: the end of the data)
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (10, 2))[:N_STEPS]
    u_r, y_r = ref.closed_loop_bounded(_spec(), d["u_d"], d["y_d"], plant, w, LO, HI)
    assert np.array_equal(u_r, u_c) and np.array_equal(y_r, y_c)
