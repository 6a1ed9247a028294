"""The reduced-space helper of the capacity tests (tests/_large_box_ref.py), pinned on the CPU:

1. against tests/test_large_bounds_reference.py::solve_trailing_block, whose iteration it holds: equal solve counts, signed
   sets and peaks, on instance 0 of the five cases of tests/test_gpu_large_box_capacity.py;
2. against the full-space helper tests/_output_bounds_ref.py::solve_bounded on instance 0 of the cases C and D (the output box
   y in [0.645, 0.655] x [0.765, 0.775], slack NONE and CONVEX; 123 and 131 components at the peak): inputs to 1e-8, cost to
   1e-9 relative, equal solve counts and signed sets.  The full-space helper costs about 0.2 s per solve at this size, which is
   why the GPU tests use the reduced one and why case E (21 - 46 solves) is not pinned in full space.
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _large_box_ref as lref
import _output_bounds_ref as yref
from test_large_bounds_reference import L_LONG, N_LONG, solve_trailing_block

INF = np.inf
_DATA = {}


def _four_tank(slack):
    if slack not in _DATA:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=L_LONG)
        d = harness.generate_batch(range(1), N=N_LONG)
        n = spec.n
        _DATA[slack] = (spec, d, d["u_d"][:, -n:, :].reshape(1, -1).copy(), d["y_d"][:, -n:, :].reshape(1, -1).copy())
    return _DATA[slack]


@pytest.mark.parametrize("case", sorted(lref.CASES))
def test_helper_is_the_trailing_block_iteration(case):
    c = lref.CASES[case]
    spec, d, up, yp = _four_tank(c["slack"])
    red = lref.solve_reduced(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], c["box"], max_iter=50)
    old = solve_trailing_block(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], c["box"], max_iter=50)
    print("case %s: %s iters %d/%d peak %d/%d margin %.1e sizes %s" % (case, red.status, red.iters, old["iters"], red.peak,
                                                                      old["peak"], red.margin, red.sizes))
    assert red.status == old["status"] == "optimal"
    assert red.iters == old["iters"] and red.peak == old["peak"] and red.both == old["both"]
    assert red.signed == old["signed"]
    assert len(red.sizes) == red.iters - 1
    # (inputs and cost: printed, not held to a bar here -- the helper takes them from a direct solve of the final system, the
    # older statement from the Woodbury update of its last iteration)
    print("   inputs %.1e cost %.1e apart" % (np.max(np.abs(red.optimal_u - old["optimal_u"])) / np.max(np.abs(old["optimal_u"])),
                                            abs(red.cost - old["cost"]) / abs(old["cost"])))
    assert red.first_over(red.peak) is None and red.sizes[red.first_over(red.peak - 1) - 1] == red.peak


@pytest.mark.parametrize("case", ["C", "D"])
def test_helper_against_the_full_space_iteration(case):
    c = lref.CASES[case]
    spec, d, up, yp = _four_tank(c["slack"])
    red = lref.solve_reduced(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], c["box"], max_iter=50)
    sol = yref.solve_bounded(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0], *c["box"]["y"])
    eu = np.max(np.abs(red.optimal_u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(red.cost - sol.cost) / abs(sol.cost)
    print("case %s: %s iters %d/%d k %d peak %d margin %.1e / %.1e err_u %.1e err_cost %.1e" %
          (case, sol.status, red.iters, sol.iters, np.count_nonzero(sol.active), red.peak, red.margin, sol.margin, eu, ec))
    assert red.status == sol.status == "optimal" and sol.margin >= 1e-7 and red.margin >= 1e-7
    assert red.iters == sol.iters
    assert np.array_equal(red.idx, sol.idx) and np.array_equal(red.active, sol.active)
    assert np.array_equal(red.lo, sol.lo) and np.array_equal(red.hi, sol.hi)
    assert eu < 1e-8 and ec < 1e-9, (eu, ec)
