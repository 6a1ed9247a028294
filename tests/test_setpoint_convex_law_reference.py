"""CPU: the premises the GPU tests of tests/test_gpu_setpoint_convex_law.py rest on, and a numpy model of the algorithm of
DDMPC_OPT_SETPOINT_CONVEX_LAW (`_setpoint_convex_ref.model_step`: the law + S, slack offsets 0, the iteration on M, the output
stage) against the full-space reference.

Premises: every reference solve of `_setpoint_convex_ref.CASES` is optimal, its active count and margin are those recorded
there (both homes of the k x k system hit), so the GPU test's cap on instances left out of the `iters` / signed-set rule (1 in
16) is met by the reference alone; every solve of the schedule loops is optimal.  Bars: TOL_U / TOL_COST of the GPU suites.
"""
import numpy as np
import pytest

import _setpoint_convex_ref as ref

TOL_U, TOL_COST = 1e-8, 1e-9
CELLS = [(box, tec, False) for box, tec in ref.CASES] + [(box, tec, True) for box, tec in ref.DIAG_CASES]
IDS = ["%s-%s%s" % (b, "terminal" if t else "no-terminal", "-diag" if d else "") for b, t, d in CELLS]


def _model_vs_helper(spec, b, sol, bounds, compare_set):
    t = ref.tank()
    u, cost, status, iters, act, rows, kind = ref.model_step(spec, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], t["us"][b],
                                                             t["ys"][b], **bounds)
    assert status == 0
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("model b=%d iters %d/%d err_u %.1e err_cost %.1e" % (b, iters, sol.iters, eu, ec))
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    if compare_set and sol.margin >= 1e-7:
        assert iters == sol.iters and np.array_equal(ref.helper_order(spec, act, rows, kind), sol.active), (b, iters, sol.iters)


@pytest.mark.parametrize("box,tec,diag", CELLS, ids=IDS)
def test_step_premises_and_model(box, tec, diag):
    spec = ref.spec(tec, diag)
    bounds = ref.BOXES[box]
    want = ref.CASES[(box, tec)]
    ks, margins = [], []
    for b in range(ref.B8):
        sol = ref.step_reference(box, tec, diag, b)
        assert sol.status == "optimal", (box, tec, b, sol.status)
        ks.append(int(np.count_nonzero(sol.active)))
        margins.append(float(sol.margin))
        if b in (0, 5):                                         # the model on two instances per cell
            _model_vs_helper(spec, b, sol, bounds, want["rule"])
    print(box, tec, diag, "active", ks, "margins %.1e .. %.1e" % (min(margins), max(margins)),
          "iters", [ref.step_reference(box, tec, diag, b).iters for b in range(ref.B8)])
    if not want["rule"]:
        return
    left_out = sum(mg < 1e-7 for mg in margins)
    assert left_out * 16 <= ref.B8, (left_out, margins)
    if diag:                                                    # (other weights: the counts of the table are the scalar ones)
        assert min(ks) >= 1, ks
        return
    assert want["k"][0] <= min(ks) and max(ks) <= want["k"][1], ks
    assert min(margins) >= want["margin"], margins
    if want["home"] == "lds":
        assert max(ks) <= 16, ks
    if want["home"] == "global":
        assert min(ks) > 16, ks
    if box == "slack-only":
        assert all(ref.step_reference(box, tec, diag, b).iters == 2 for b in range(ref.B8))
        n_in, n_out = ref.n_boxed(spec, bounds)
        assert n_in == 0 and n_out == 0 and ref.step_reference(box, tec, diag, 0).active.size == spec.L * spec.p


@pytest.mark.parametrize("nms", ref.LOOP_NMS)
@pytest.mark.parametrize("box", ref.LOOP_BOXES)
def test_every_solve_of_the_schedule_loop_is_optimal(box, nms):
    case, u_ref, y_ref = ref.loop_case()
    assert u_ref.shape == (ref.LOOP_B, ref.LOOP_STEPS, 2)
    for t_change in ref.LOOP_CHANGES:                           # the setpoints change at two steps, for every instance
        assert np.all(np.any(u_ref[:, t_change] != u_ref[:, t_change - 1], axis=1))
    worst, ks = np.inf, []
    for b in range(ref.LOOP_B):
        sols = ref.loop_reference(box, b, nms)[5]               # (schedule_loop raises on a solve that is not optimal)
        assert len(sols) == -(-ref.LOOP_STEPS // nms) and all(s.status == "optimal" for s in sols)
        worst = min(worst, min(s.margin for s in sols))
        ks.append([int(np.count_nonzero(s.active)) for s in sols])
    print(box, nms, "smallest margin %.1e" % worst, "active counts", ks)
    assert any(k > 0 for row in ks for k in row)                # the loop meets the box
