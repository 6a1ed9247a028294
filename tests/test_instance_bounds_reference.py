"""The three per-instance boxes of tests/_instance_bounds_cases.py in the full-space reference alone (no GPU): what the GPU test
of ddmpc_set_instance_input_bounds / _output_bounds relies on when it compares every instance against its own reference.

For A, B and C in both modes (slack NONE without the terminal constraint, CONVEX with it):
  * every instance ends `optimal` within max_iter = 100;
  * at most 4 of the 32 have margin < 1e-6 -- the class the GPU test compares without iteration count and active set (two
    correct implementations may decide such an instance differently).  A condition on the boxes, not a measurement;
  * at least 8 distinct final active sets, so the batch really is a fleet of different solves;
  * over the six configurations, at least one instance with an empty final set and one with more than 16 active components (the
    k x k system beyond the LDS).  Not per configuration: A bounds channel 1 of every instance tightly enough that none stays
    empty (3 .. 49 active), and under the CONVEX slack box a slack component is active on every instance; the empty sets are B's
    "no bound" rows with slack NONE.  Sets beyond 16 occur in A and B in both modes.
"""
import numpy as np
import pytest

import _instance_bounds_cases as IC


@pytest.mark.parametrize("mode", list(IC.MODES))
@pytest.mark.parametrize("name", IC.NAMES)
def test_boxes_in_the_reference(name, mode):
    sols = [IC.reference(name, mode, i) for i in range(IC.B32)]
    iters = [s.iters for s in sols]
    nact = [int(np.count_nonzero(s.active)) for s in sols]
    margins = np.array([s.margin for s in sols])
    print(name, mode, "iters", min(iters), "..", max(iters), "active", min(nact), "..", max(nact), "min margin %.1e" % margins.min(),
          "below 1e-6:", int(np.sum(margins < 1e-6)))
    assert all(s.status == "optimal" for s in sols), [s.status for s in sols]
    assert int(np.sum(margins < 1e-6)) <= 4, np.sort(margins)[:6]
    sets = {(tuple(s.idx[s.active > 0]), tuple(s.idx[s.active < 0])) for s in sols}
    assert len(sets) >= 8, len(sets)


def test_empty_and_large_sets_occur():
    nact = {(name, mode): [int(np.count_nonzero(IC.reference(name, mode, i).active)) for i in range(IC.B32)]
            for name in IC.NAMES for mode in IC.MODES}
    assert min(min(v) for v in nact.values()) == 0, nact
    for mode in IC.MODES:
        assert max(nact[("A", mode)]) > 16 and max(nact[("B", mode)]) > 16, nact
