"""CPU: the premises the GPU tests of tests/test_gpu_setpoint_box_loop.py rest on, so that a failure there can only mean the
kernel (ddmpc_closed_loop_setpoint_box_kernel<SAFE, YB> and, at 268 rows, ddmpc_setpoint_box_step_kernel).

For every case of `_setpoint_box_ref.LOOP_CASES` / `BIG_CASES` and every instance compared with the reference: every reference
solve optimal, every margin at least 1e-7 (nobody is left out), the active counts that keep a case from passing on a simpler
path (output components active, more than 16 components active where both homes of the k x k system are to be met), the gap in
`iters` around the iteration cap, the schedule rows inside the bounds under the terminal constraint except those meant to be
refused.  The stops at the cap are a finding of the numpy model of tests/test_setpoint_box_law_reference.py as well.
"""
import numpy as np
import pytest

import _setpoint_box_ref as ref
import test_setpoint_box_law_reference as model
from test_gpu_setpoint_box_law import _ref_loop

MARGIN = 1e-7
INF = np.inf
NMS = ref.LOOP_NMS


def _loops(name, nms, rows=None, steps=None):
    c = ref.LOOP_CASES[name]
    out = {}
    for b in (c["rows"] if rows is None else rows):
        r = ref.loop_reference(name, b, nms, steps)
        assert all(s.status == "optimal" for s in r[5]), (name, nms, b)
        margin = min(s.margin for s in r[5])
        print("%s nstep %d instance %d: margin %.1e iters %s" % (name, nms, b, margin, [s.iters for s in r[5]]))
        assert margin >= MARGIN, (name, nms, b, margin)
        out[b] = r
    return out


def _counts(name, sols):
    case = ref.loop_case(name)[0]
    return [ref.active_counts(case["spec"], ref.LOOP_CASES[name]["bounds"], s) for s in sols]


def _inside(name, skip=()):
    """Every schedule row of the case inside the bounds of its channel, the instances of `skip` from the switch on apart."""
    _, u_ref, y_ref = ref.loop_case(name)
    bd = ref.LOOP_CASES[name]["bounds"]
    for v, lo, hi in ((u_ref, bd.get("u_min"), bd.get("u_max")), (y_ref, bd.get("y_min"), bd.get("y_max"))):
        if lo is None:
            continue
        ok = np.all((v >= np.asarray(lo, float)) & (v <= np.asarray(hi, float)), axis=2)
        for b in skip:
            assert not np.any(ok[b, ref.T_SWITCH:]) and np.all(ok[b, :ref.T_SWITCH]), (name, b)
            ok[b, ref.T_SWITCH:] = True
        assert np.all(ok), name


@pytest.mark.parametrize("nms", NMS)
def test_output_bounds_only(nms):
    refs = _loops("y-only", nms)
    _inside("y-only")
    ks = [k for _, k in _counts("y-only", refs[3][5])]
    print("instance 3 active outputs", ks)
    n_first = 6 if nms == 1 else 3                      # the solves of the first six / twelve steps
    assert all(k >= 2 for k in ks[:n_first]), ks
    assert all(k >= 1 for _, k in _counts("y-only", refs[0][5])[:2])
    # the upper bounds matter: instance 0 without them
    case, u_ref, y_ref = ref.loop_case("y-only")
    open_top = _ref_loop(case, 0, u_ref[0], y_ref[0], nms, dict(y_min=ref.LOOP_CASES["y-only"]["bounds"]["y_min"], y_max=[INF, INF]))
    d = np.max(np.abs(open_top[1] - refs[0][1]))
    print("instance 0, y_sys against the loop with y_max = +inf: %.2e" % d)
    assert d >= 5e-3


@pytest.mark.parametrize("nms", NMS)
def test_input_and_output_bounds_without_the_terminal_constraint(nms):
    refs = _loops("u-and-y", nms)
    for b in (0, 3):
        ks = _counts("u-and-y", refs[b][5])
        print("instance %d active (inputs, outputs)" % b, ks)
        assert ks[0][0] >= 2 and ks[0][1] >= 1, (b, ks)
    assert _counts("u-and-y", refs[0][5])[0][1] >= 2
    # the output bounds matter to what the loop applies with n_mpc_step = 4 (with 1 the held outputs lie beyond the step in use)
    case, u_ref, y_ref = ref.loop_case("u-and-y")
    bd = ref.LOOP_CASES["u-and-y"]["bounds"]
    no_y = _ref_loop(case, 0, u_ref[0], y_ref[0], nms, dict(u_min=bd["u_min"], u_max=bd["u_max"]))
    d = np.max(np.abs(no_y[1] - refs[0][1]))
    print("instance 0, y_sys against the loop without output bounds: %.2e" % d)
    assert nms == 1 or d >= 6e-2


@pytest.mark.parametrize("nms", NMS)
def test_schedule_leaving_the_box(nms):
    refs = _loops("leaving", nms)
    _, u_ref, _ = ref.loop_case("leaving")
    assert np.all(u_ref[[1, 3], ref.T_SWITCH:, 0] == 2.3) and np.all(u_ref[:, :ref.T_SWITCH] <= 2.0)
    for b in (1, 3):
        ks = [k for k, _ in _counts("leaving", refs[b][5])]
        print("instance %d active inputs" % b, ks)
        assert max(ks) > 16 and min(ks) <= 16, ks        # both homes of the k x k system
        u = refs[b][0]
        assert np.max(u) <= 2.0 and np.min(u) >= 0.0
        assert np.any((u > 0.0) & (u < 2.0)), b         # the inputs are not all at a bound
    t_sw = ref.t_stop(nms) // nms
    ks = [k for k, _ in _counts("leaving", refs[3][5])]
    assert ks[t_sw] > ks[t_sw - 1], ks                  # the switch out of the box shows


@pytest.mark.parametrize("nms", NMS)
def test_refused_setpoint_premises(nms):
    _inside("refused", skip=(1,))
    _inside("tight-terminal")
    t_stop = ref.t_stop(nms)
    assert t_stop == (10 if nms == 1 else 12)
    r = _loops("refused", nms, steps=t_stop)[1]
    assert r[0].shape[0] == t_stop and len(r[5]) == t_stop // nms
    # the truncated loop is the start of the loop on the unchanged schedule
    full = _loops("tight-terminal", nms, rows=(1,))[1]
    assert np.array_equal(full[0][:t_stop], r[0]) and np.array_equal(full[1][:t_stop], r[1])


@pytest.mark.parametrize("nms", NMS)
def test_iteration_cap_premises(nms):
    cap = ref.LOOP_CASES["cap"]["max_iter"]
    _inside("cap")
    t_stop = ref.t_stop(nms)
    refs = _loops("cap", nms, rows=(0, 1, 2, 3))
    k_stop = t_stop // nms
    for b, r in refs.items():
        it = [s.iters for s in r[5]]
        if b != 1:
            assert max(it) <= cap - 1, (b, it)
            continue
        assert max(it[:k_stop]) <= cap - 1 and it[k_stop] >= cap + 1, it
        assert r[5][k_stop].margin >= MARGIN
    _loops("cap", nms, steps=t_stop)
    # the model: status 4 at the stopping solve, 0 at the solve before it (windows of the reference loop cut there)
    case, u_ref, y_ref = ref.loop_case("cap")
    bd = ref.LOOP_CASES["cap"]["bounds"]
    for t, want in ((t_stop, 4), (t_stop - nms, 0)):
        r = ref.loop_reference("cap", 1, nms, t)
        st, it = model.model_step(case["spec"], case["u_d"][1], case["y_d"][1], r[3], r[4], u_ref[1, t], y_ref[1, t], max_iter=cap, **bd)[2:4]
        print("model at step %d: status %d iters %d" % (t, st, it))
        assert st == want and (it == cap if want else it == refs[1][5][t // nms].iters), (t, st, it)


def test_iteration_cap_with_output_bounds_premises():
    name = "u-and-y-cap"
    cap = ref.LOOP_CASES[name]["max_iter"]
    case, u_ref, y_ref = ref.loop_case(name)
    bd = ref.LOOP_CASES[name]["bounds"]
    for nms in NMS:
        refs = _loops(name, nms)
        assert refs[0][5][0].iters >= cap + 2           # instance 0 stops at its first solve
        assert _counts(name, refs[0][5])[0][1] >= 2
    for b in (0, 3):
        first = ref.loop_reference(name, b, 1)[5][0]
        got = {mi: model.model_step(case["spec"], case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], u_ref[b, 0], y_ref[b, 0],
                                    max_iter=mi, **bd)[2:4] for mi in (cap, 100)}
        print("instance %d first solve: reference iters %d, model (status, iters) %s" % (b, first.iters, got))
        assert got[100] == (0, first.iters)
        assert got[cap] == ((4, cap) if first.iters > cap else (0, first.iters))
    assert ref.loop_reference(name, 0, 1)[5][0].iters > cap


@pytest.mark.parametrize("name", list(ref.BIG_CASES))
def test_largest_shape_premises(name):
    tec, bounds, nbox = ref.BIG_CASES[name]
    s = ref.big_spec(tec)
    assert (s.m + s.p) * (s.L + s.n) == 268
    ks = []
    for b in range(ref.BIG_B):
        sol = ref.big_step_reference(name, b)
        assert sol.status == "optimal" and sol.active.size == nbox, (name, b, sol.status, sol.active.size)
        assert sol.margin >= MARGIN, (name, b, sol.margin)
        ks.append(int(np.count_nonzero(sol.active)))
        print("%s b=%d iters %d k %d margin %.1e" % (name, b, sol.iters, ks[-1], sol.margin))
    assert min(ks) > 16, ks
    if "y_min" in bounds:
        assert all(ref.active_counts(s, bounds, ref.big_step_reference(name, b))[1] >= 1 for b in range(ref.BIG_B))
    for b in (0, ref.BIG_B - 1):
        sols = ref.big_loop_reference(name, b)[5]
        assert len(sols) == ref.BIG_STEPS // ref.BIG_NMS and all(x.status == "optimal" for x in sols)
        assert min(x.margin for x in sols) >= MARGIN, (name, b)
        print("%s loop b=%d iters %s k %s" % (name, b, [x.iters for x in sols], [int(np.count_nonzero(x.active)) for x in sols]))
    if name == "u-tight":                               # more than 16 active in every solve of the loop
        assert all(np.count_nonzero(x.active) > 16 for b in (0, ref.BIG_B - 1) for x in ref.big_loop_reference(name, b)[5])


@pytest.mark.parametrize("name,row,safe", ref.LOOP_TWINS, ids=["%s-row%d-%s" % (n, r, "safe" if s else "plain") for n, r, s in ref.LOOP_TWINS])
def test_loop_and_step_twin_premises(name, row, safe):
    case, u_ref, y_ref = ref.loop_case(name)
    c = ref.LOOP_CASES[name]
    its = []
    for b in range(case["B"]):
        sol = ref.solve(case["spec"], case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], u_ref[b, row], y_ref[b, row], **c["bounds"])
        assert sol.status == "optimal" and sol.margin >= MARGIN, (name, b, sol.status, sol.margin)
        its.append(sol.iters)
    print(name, row, "iters", its)
    assert min(its) >= 2
    assert (max(its) > (c["max_iter"] or 100)) == safe  # the safeguard has an instance to finish exactly where it is on
