"""The yardstick of the warm-start tests beyond 271 rows (tests/_large_box_warm_ref.py), on the CPU.

Fixture of tests/test_gpu_large_box_capacity.py: four-tank, L = 70, N = 700, 296 rows, the closed loop of instance b from the
data tail on the plant orc.FOUR_TANK with the noise eps_max U(-1, 1) of np.random.default_rng(1000 + b), one solve per step.
Solves per window (1 = the empty set's), empty start / seeded with the previous window's final set, as the helper gives them:

  A  u in [0, 2] CONVEX          0: 9 8 8 8 / 9 3 4 3      1: 10 10 10 9 / 10 5 4 3    2: 8 7 7 8 / 8 4 4 3
  B  u in [0.9, 1.1] NONE        0: 21 18 16 18 / 21 4 4 5 1: 29 27 22 22 / 29 6 3 4   2: 18 21 18 19 / 18 4 4 5
  W  u in [-4, 6] CONVEX         0: 4 3 3 2 1 / 4 3 3 4 1  (a wide box can lose solves: window 3)
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _box_warm_ref as fref
import _large_box_ref as lref
import _large_box_warm_ref as wref

B8, LH, N, MAX_ITER = 8, 70, 700, 50
CASES = dict(lref.CASES)
CASES["W"] = dict(box=dict(u=([-4.0, -4.0], [6.0, 6.0]), y=None), slack="convex")
SEEDED = {("A", 0): [9, 3, 4, 3], ("A", 1): [10, 5, 4, 3], ("A", 2): [8, 4, 4, 3],
          ("B", 0): [21, 4, 4, 5], ("B", 1): [29, 6, 3, 4], ("B", 2): [18, 4, 4, 5]}
EMPTY = {("A", 0): [9, 8, 8, 8], ("A", 1): [10, 10, 10, 9], ("A", 2): [8, 7, 7, 8],
         ("B", 0): [21, 18, 16, 18], ("B", 1): [29, 27, 22, 22], ("B", 2): [18, 21, 18, 19]}

_DATA, _PROB, _LOOP = {}, {}, {}


def data():
    if not _DATA:
        _DATA["d"] = harness.generate_batch(range(B8), N=N)
    return _DATA["d"]


def spec_of(case):
    return orc.spec_from_params(slack_var_constraint_type=1 if CASES[case]["slack"] == "convex" else 0, L=LH)


def problem(case, b):
    """The reduced problem of instance b of a case, formed once."""
    if (case, b) not in _PROB:
        d = data()
        _PROB[(case, b)] = wref.Reduced(spec_of(case), d["u_d"][b], d["y_d"][b], CASES[case]["box"])
    return _PROB[(case, b)]


def noise(b, n_steps):
    return orc.FOUR_TANK["eps_max"] * np.random.default_rng(1000 + b).uniform(-1.0, 1.0, (n_steps, 2))


def plant_of(b):
    P = orc.FOUR_TANK
    pl = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
    pl.x = data()["x_end"][b].copy()
    return pl


def loop(case, b, n_win=4, first=None):
    """The seeded closed loop of instance b over n_win windows, computed once: the solution of every window (with `window`)."""
    key = (case, b, n_win, first is not None)
    if key not in _LOOP:
        d = data()
        _LOOP[key] = wref.closed_loop_seeded(spec_of(case), d["u_d"][b], d["y_d"][b], plant_of(b), noise(b, n_win), CASES[case]["box"],
                                             max_iter=MAX_ITER, carry=True, problem=problem(case, b), first=first)[2]
    return _LOOP[key]


def _tail(b, spec):
    d = data()
    return d["u_d"][b][-spec.n:].reshape(-1).copy(), d["y_d"][b][-spec.n:].reshape(-1).copy()


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "W"])
def test_without_a_seed_the_helper_is_solve_reduced(case):
    d, spec = data(), spec_of(case)
    up, yp = _tail(0, spec)
    old = lref.solve_reduced(spec, d["u_d"][0], d["y_d"][0], up, yp, CASES[case]["box"], max_iter=MAX_ITER)
    for seed in (None, np.zeros(problem(case, 0).nbox, dtype=int)):
        got = problem(case, 0).solve(up, yp, seed, max_iter=MAX_ITER)
        print("case %s: %s iters %d/%d peak %d margin %.1e" % (case, got.status, got.iters, old.iters, got.peak, got.margin))
        assert not got.seeded and not got.fell_back
        assert got.status == old.status == "optimal" and got.iters == old.iters and got.sizes == old.sizes
        assert got.margin == old.margin and got.signed == old.signed and got.both == old.both
        assert np.array_equal(got.idx, old.idx) and np.array_equal(got.active, old.active)
        assert np.array_equal(got.optimal_u, old.optimal_u) and got.cost == old.cost
        assert np.array_equal(problem(case, 0).table_set(old), got.set)


def test_the_cap_without_a_seed_is_solve_reduced_too():
    d, spec = data(), spec_of("B")
    up, yp = _tail(3, spec)
    old = lref.solve_reduced(spec, d["u_d"][3], d["y_d"][3], up, yp, CASES["B"]["box"], max_iter=MAX_ITER)
    got = problem("B", 3).solve(up, yp, None, max_iter=MAX_ITER)
    assert got.status == old.status == "solver_error" and got.iters == old.iters == MAX_ITER and got.sizes == old.sizes
    assert got.at_cap and not np.any(got.set)


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_seeded_with_its_own_optimal_set_a_window_takes_two_solves(case):
    spec = spec_of(case)
    up, yp = _tail(0, spec)
    cold = problem(case, 0).solve(up, yp, None, max_iter=MAX_ITER)
    assert cold.iters > 2 and np.any(cold.set)
    got = problem(case, 0).solve(up, yp, cold.set, max_iter=MAX_ITER)
    assert got.seeded and not got.fell_back and got.status == "optimal" and got.iters == 2
    assert np.array_equal(got.set, cold.set) and got.sizes == [np.count_nonzero(cold.set)]
    assert np.array_equal(got.optimal_u, cold.optimal_u) and got.cost == cold.cost       # (both from the direct solve of the final system)


@pytest.mark.parametrize("case,b", sorted(SEEDED))
def test_four_windows_seeded_and_empty_end_with_the_same_set(case, b):
    sols = loop(case, b)
    prob = problem(case, b)
    empty = [prob.solve(*s.window, None, max_iter=MAX_ITER) for s in sols]
    print("case %s b=%d empty %s seeded %s margin %.1e / %.1e" % (case, b, [e.iters for e in empty], [s.iters for s in sols],
                                                                min(s.margin for s in sols), min(e.margin for e in empty)))
    assert [s.iters for s in sols] == SEEDED[(case, b)] and [e.iters for e in empty] == EMPTY[(case, b)]
    assert not sols[0].seeded and all(s.seeded and not s.fell_back for s in sols[1:])
    for s, e in zip(sols, empty):
        assert s.status == e.status == "optimal" and min(s.margin, e.margin) >= 1e-7
        assert np.array_equal(s.set, e.set) and np.array_equal(s.active, e.active)
        assert np.max(np.abs(s.optimal_u - e.optimal_u)) <= 1e-10 * np.max(np.abs(e.optimal_u))
        assert abs(s.cost - e.cost) <= 1e-10 * abs(e.cost)


def test_a_seeded_run_at_the_cap_starts_again_from_the_empty_set():
    """[-4, 6] CONVEX, instance 0: window 3 takes 2 solves from the empty set and 4 from window 2's set.  With max_iter = 3 the
    seeded run makes its three solves, ends at the cap and is given up; the empty start repeats none but the empty set's solve:
    3 - 1 + 2 = 4 solves in all, optimal.  With the safeguard the seeded run's cap is final."""
    sols = loop("W", 0, n_win=5)
    prob = problem("W", 0)
    assert [s.iters for s in sols] == [4, 3, 3, 4, 1]
    cold2 = prob.solve(*sols[2].window, None, max_iter=3)
    assert cold2.status == "optimal" and cold2.iters == 3 and np.array_equal(cold2.set, sols[2].set)   # window 2 inside the cap
    cold3 = prob.solve(*sols[3].window, None, max_iter=3)
    assert cold3.status == "optimal" and cold3.iters == 2
    got = prob.solve(*sols[3].window, sols[2].set, max_iter=3)
    print("restart: iters %d sizes %s margin %.1e" % (got.iters, got.sizes, got.margin))
    assert got.seeded and got.fell_back and got.status == "optimal" and got.iters == 4 and not got.at_cap
    assert np.array_equal(got.set, cold3.set) and np.array_equal(got.optimal_u, cold3.optimal_u) and got.cost == cold3.cost
    safe = prob.solve(*sols[3].window, sols[2].set, max_iter=3, safeguard=True)
    assert safe.status == "solver_error" and safe.iters == 3 and safe.at_cap and not np.any(safe.set)


def test_a_seeded_run_beyond_the_capacity_starts_again_from_the_empty_set():
    """The branch for the capacity, on the helper alone (no GPU input is known to reach it): a seed with more components than
    the capacity is given up before its solve, which counts as attempted."""
    sols = loop("W", 0, n_win=5)
    prob = problem("W", 0)
    k = np.count_nonzero(sols[0].set)
    cold = prob.solve(*sols[1].window, None, max_iter=MAX_ITER)
    got = prob.solve(*sols[1].window, sols[0].set, max_iter=MAX_ITER, capacity=k - 1)
    assert cold.peak <= k - 1 and got.fell_back and got.status == "optimal" and got.iters == 1 + cold.iters
    assert np.array_equal(got.set, cold.set)


def test_against_the_full_space_seeded_iteration():
    """[-4, 6] CONVEX, instance 0, windows 1 .. 3 against tests/_box_warm_ref.py::solve_seeded on the full-space problem (3 to 4
    solves of 0.2 s each): equal solve counts and signed sets."""
    sols = loop("W", 0, n_win=5)
    d, spec = data(), spec_of("W")
    lo, hi = CASES["W"]["box"]["u"]
    for prev, s in zip(sols[:3], sols[1:4]):
        full = fref.solve_seeded(spec, d["u_d"][0], d["y_d"][0], *s.window, lo, hi, prev.active, max_iter=MAX_ITER)
        print("full space: iters %d/%d margin %.1e / %.1e" % (s.iters, full.iters, s.margin, full.margin))
        assert full.seeded and not full.fell_back and full.status == orc.OPTIMAL
        assert np.array_equal(full.idx, s.idx) and full.iters == s.iters and np.array_equal(full.active, s.active)
        assert np.max(np.abs(full.optimal_u - s.optimal_u)) <= 1e-8 * np.max(np.abs(s.optimal_u))
