"""The reduced-space helper of the safeguard tests (tests/_large_box_safeguard_ref.py), pinned on the CPU in three ways.

Fixture: four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7 at the data tail, c = 1 (that of tests/test_gpu_large_box_capacity.py).

1. Against the full-space primal method tests/_box_safeguard_ref.py::solve_safeguarded on the instances 0 .. 3 of the box
   u in [-4, 6], slack NONE and CONVEX (4 - 8 solves each): equal solves and signed sets, inputs to 1e-8, cost to 1e-9 relative.
2. Against the primal-dual helper tests/_large_box_ref.py::solve_reduced on instance 0 of the cases A and B: the same final
   signed set, inputs and cost at those bars -- the QP is strictly convex, so both methods end at its one optimum.
3. On the instance that cycles: case B instance 3, where solve_reduced reports solver_error at 50, is optimal after 124 solves
   with a largest working set of 132 (= nbox; the set of the first solve has 115, the 129th component joins at solve 15) and a
   final set of 126.
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _box_safeguard_ref as fref
import _large_box_ref as lref
import _large_box_safeguard_ref as sref
from test_large_bounds_reference import L_LONG, N_LONG

TOL_U, TOL_COST = 1e-8, 1e-9
WIDE = dict(u=([-4.0, -4.0], [6.0, 6.0]), y=None)
_DATA = {}


def _four_tank(slack):
    if slack not in _DATA:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=L_LONG)
        d = harness.generate_batch(range(4), N=N_LONG)
        n = spec.n
        _DATA[slack] = (spec, d, d["u_d"][:, -n:, :].reshape(4, -1).copy(), d["y_d"][:, -n:, :].reshape(4, -1).copy())
    return _DATA[slack]


def _errors(a, b):
    return np.max(np.abs(a.optimal_u - b.optimal_u)) / np.max(np.abs(b.optimal_u)), abs(a.cost - b.cost) / abs(b.cost)


@pytest.mark.parametrize("slack", ["none", "convex"])
def test_helper_against_the_full_space_primal_method(slack):
    spec, d, up, yp = _four_tank(slack)
    for b in range(4):
        red = sref.solve_primal(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], WIDE)
        sol = fref.solve_safeguarded(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], *WIDE["u"])
        eu, ec = _errors(red, sol)
        print("%s b=%d: %s solves %d/%d set %d largest %d/%d margin %.1e err_u %.1e err_cost %.1e" %
              (slack, b, sol.status, red.iters, sol.iters, np.count_nonzero(sol.active), red.peak, sol.kmax, red.margin, eu, ec))
        assert red.status == sol.status == "optimal" and red.margin >= 1e-7
        assert 4 <= sol.iters <= 8 and red.iters == sol.iters and red.peak == sol.kmax
        assert np.array_equal(red.idx, sol.idx) and np.array_equal(red.active, sol.active)
        assert np.array_equal(red.lo, sol.lo) and np.array_equal(red.hi, sol.hi)
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)


@pytest.mark.parametrize("case", ["A", "B"])
def test_helper_ends_at_the_optimum_of_the_primal_dual_helper(case):
    c = lref.CASES[case]
    spec, d, up, yp = _four_tank(c["slack"])
    red = sref.solve_primal(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], c["box"])
    pd = lref.solve_reduced(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], c["box"], max_iter=50)
    eu, ec = _errors(red, pd)
    print("case %s: primal %s %d solves (%d releases), largest %d, final %d, margin %.1e; primal-dual %s %d; err_u %.1e err_cost %.1e" %
          (case, red.status, red.iters, red.releases, red.peak, np.count_nonzero(red.active), red.margin, pd.status, pd.iters, eu, ec))
    assert red.status == pd.status == "optimal" and red.margin >= 1e-7
    assert red.signed == pd.signed
    assert np.array_equal(red.idx, pd.idx) and np.array_equal(red.active, pd.active)
    assert eu < TOL_U and ec < TOL_COST, (eu, ec)
    assert len(red.sizes) == red.iters <= 4 * 272 + 16


def test_helper_solves_the_instance_that_cycles():
    c = lref.CASES["B"]
    spec, d, up, yp = _four_tank(c["slack"])
    pd = lref.solve_reduced(spec, d["u_d"][3], d["y_d"][3], up[3], yp[3], c["box"], max_iter=50)
    red = sref.solve_primal(spec, d["u_d"][3], d["y_d"][3], up[3], yp[3], c["box"])
    print("case B b=3: primal-dual %s at %d; primal %s, %d solves, largest %d, final %d, margin %.1e" %
          (pd.status, pd.iters, red.status, red.iters, red.peak, np.count_nonzero(red.active), red.margin))
    assert pd.status == "solver_error" and pd.iters == 50
    assert red.status == "optimal" and red.margin >= 1e-7
    assert (red.iters, red.peak, np.count_nonzero(red.active)) == (124, 132, 126)
    assert red.idx.size == 132 and red.sizes[0] == 115 and red.first_over(128) == 15 and red.first_over(192) is None
    assert np.all(np.abs(np.diff(red.sizes)) == 1)                           # one component joins or leaves per solve
    assert np.all(np.isfinite(red.optimal_u)) and np.all((red.optimal_u >= 0.9) & (red.optimal_u <= 1.1))
