"""ddmpc_closed_loop_setpoint_box_kernel<SAFE, YB> (csrc/ddmpc_setpoint_box_law.hpp): the fused loop of a bounded handle with a
setpoint schedule under output bounds, the safeguard and stops, and both kernels of DDMPC_OPT_SETPOINT_BOX_LAW at 268 rows.

The loop of test_gpu_setpoint_box_law._tank_loop (four-tank, L = 30, n = 4, N = 400, 136 rows, batch 4, 21 steps, a setpoint
switch at step 10) under the bounds, schedules and caps of `_setpoint_box_ref.LOOP_CASES`; instances against the schedule loop
of the full-space helper for n_mpc_step 1 and 4.  Bars are the project's own, from test_gpu_setpoint_box_law.py: inputs 1e-8,
outputs, final state and output window 1e-9 of max(1, max|y|), law against law 1e-10.  The premises of every case (reference
solves optimal, margins >= 1e-7, the active counts, the gap in `iters` around the caps, where an instance stops) are held on
the CPU by tests/test_setpoint_box_loop_reference.py.

Which instantiation a test launches: <false, true> 1, 2, 7;  <false, false> 3, 4, 5, 7;  <true, false> 5, 7;  <true, true> 6, 7;
section 8 launches <false, false> and <false, true> of the step and of the loop at 268 rows (a block of five waves)."""
import numpy as np
import pytest

import _setpoint_box_ref as ref
import test_gpu_parity as T
import test_gpu_setpoint_box_law as G
from test_gpu_setpoint_box_law import STEP_KERNEL_LOOP, TOL_LAW, _check_loop, _check_step, _engine, _tank_loop

pytestmark = pytest.mark.gpu

INF = np.inf
NMS = ref.LOOP_NMS


class _Loop:
    """The engine of a case of ref.LOOP_CASES and its loop arguments."""

    def __init__(self, name, **kw):
        c = ref.LOOP_CASES[name]
        self.name, self.bounds = name, c["bounds"]
        self.case, self.u_ref, self.y_ref = ref.loop_case(name)
        if c["max_iter"]:
            kw.setdefault("max_iter", c["max_iter"])
        self.eng = T._engine(self.case["spec"], 400, self.case["B"], **kw)
        self.eng.set_setpoint_box_law(True)
        G._bound(self.eng, **self.bounds)
        self.eng.set_data(self.case["u_d"], self.case["y_d"])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()
        return False

    def run(self, nms, u_ref=None, y_ref=None, steps=None):
        case, pl = self.case, self.case["plant"]
        u_ref = self.u_ref if u_ref is None else u_ref
        y_ref = self.y_ref if y_ref is None else y_ref
        out = self.eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"][:, :steps],
                                             u_ref[:, :steps], y_ref[:, :steps], n_mpc_step=nms)
        assert self.eng.closed_loop_kernel_name() == STEP_KERNEL_LOOP
        return out

    def refs(self, nms, rows=None):
        return {b: ref.loop_reference(self.name, b, nms) for b in (ref.LOOP_CASES[self.name]["rows"] if rows is None else rows)}


def _bit_equal(a, b, rows):
    for x, y in zip(a, b):
        assert np.array_equal(x[rows], y[rows], equal_nan=True)


def _check_stopped(tag, out, base, b, t_stop, code, cut):
    """Instance b stopped at step t_stop with status `code`: NaN rows from there on, the rows before and the neighbours bit-equal
    to `base` (the call in which it does not stop), and -- the documented rule: x and the windows as they stood -- its final
    state and windows those of the reference loop run for exactly t_stop steps (`cut`)."""
    u_sys, y_sys, status, x_end, up_end, yp_end = out
    keep = np.arange(status.size) != b
    assert status[b] == code and np.all(status[keep] == 0), (tag, status)
    assert np.all(np.isnan(u_sys[b, t_stop:])) and np.all(np.isnan(y_sys[b, t_stop:])), tag
    assert np.array_equal(u_sys[b, :t_stop], base[0][b, :t_stop]) and np.array_equal(y_sys[b, :t_stop], base[1][b, :t_stop]), tag
    _bit_equal(out, base, keep)
    assert cut[0].shape[0] == t_stop
    head = (u_sys[:, :t_stop], y_sys[:, :t_stop], np.zeros_like(status), x_end, up_end, yp_end)
    _check_loop("%s stopped at %d" % (tag, t_stop), head, {b: cut}, (b,))
    assert not np.array_equal(x_end[b], base[3][b])     # (the state did not move on with the loop)


# ----------------------------------------------------------------------------------- 1. output bounds only, <false, true>
@pytest.mark.parametrize("nms", NMS)
def test_output_bounds_only(gpu, nms):
    with _Loop("y-only") as lp:
        out = lp.run(nms)
        lp.eng.set_output_bounds(lp.bounds["y_min"], [INF, INF])
        open_top = lp.run(nms)
    refs = lp.refs(nms)
    assert np.all(out[2] == 0) and np.all(open_top[2] == 0)
    _check_loop("y-only <false,true> nstep %d" % nms, out, refs, (0, 3))
    ks = [ref.active_counts(lp.case["spec"], lp.bounds, s)[1] for s in refs[3][5]]
    print("instance 3 active outputs", ks)
    assert all(k >= 2 for k in ks[:6 if nms == 1 else 3]), ks      # (not the unbounded law: the solves of the first steps)
    d = np.max(np.abs(out[1] - open_top[1]))
    print("y_sys against the run with y_max = +inf: %.2e" % d)
    assert d > 1e-3                                     # (the reference loops differ by 5e-3 and more: held on the CPU)


# -------------------------------------------------------- 2. input and output bounds, no terminal constraint, <false, true>
@pytest.mark.parametrize("nms", NMS)
def test_input_and_output_bounds_without_the_terminal_constraint(gpu, nms):
    with _Loop("u-and-y") as lp:
        out = lp.run(nms)
        lp.eng.set_output_bounds(None, None)
        open_low = lp.run(nms)
    refs = lp.refs(nms)
    assert np.all(out[2] == 0) and np.all(open_low[2] == 0)
    _check_loop("u-and-y <false,true> nstep %d" % nms, out, refs, (0, 3))
    for b in (0, 3):
        ks = [ref.active_counts(lp.case["spec"], lp.bounds, s) for s in refs[b][5]]
        print("instance %d active (inputs, outputs)" % b, ks)
        assert ks[0][0] >= 2 and ks[0][1] >= 1, ks
    d = np.max(np.abs(out[1] - open_low[1]))
    # with n_mpc_step = 1 the outputs held at a bound lie beyond the one step in use and the first input is at its own bound
    # either way: the reference loops with and without output bounds are equal there, so only n_mpc_step = 4 can tell
    print("y_sys against the run without output bounds: %.2e" % d)
    assert nms == 1 or d > 1e-3                         # (the reference loops differ by 6e-2 and more: held on the CPU)


# ------------------------------------------------ 3. a schedule that leaves the box, no terminal constraint, <false, false>
@pytest.mark.parametrize("nms", NMS)
def test_schedule_leaving_the_box_without_the_terminal_constraint(gpu, nms):
    _, u0, y0 = _tank_loop()
    with _Loop("leaving") as lp:
        out = lp.run(nms)
        base = lp.run(nms, u0, y0)
    assert np.all(lp.u_ref[[1, 3], ref.T_SWITCH:, 0] == 2.3) and np.array_equal(lp.y_ref, y0)
    assert np.all(out[2] == 0) and np.all(base[2] == 0)
    _check_loop("leaving <false,false> nstep %d" % nms, out, lp.refs(nms), (1, 3))
    print("u_sys spans %.3f .. %.3f" % (np.min(out[0]), np.max(out[0])))
    assert np.max(out[0]) <= 2.0 and np.min(out[0]) >= 0.0
    assert np.max(out[0][[1, 3]]) == 2.0                # (held at the bound exactly)
    _bit_equal(out, base, [0, 2])
    assert not np.array_equal(out[0][[1, 3]], base[0][[1, 3]])


# ---------------------------------------------------------------- 4. refused mid-loop: outside the bounds, a NaN setpoint
@pytest.mark.parametrize("nms", NMS)
def test_refused_setpoints_stop_with_the_state_as_it_stood(gpu, nms):
    t_stop = ref.t_stop(nms)
    _, u0, y0 = _tank_loop()
    with _Loop("refused") as lp:
        base = lp.run(nms, u0, y0)
        outside = lp.run(nms)
        u_nan, y_nan = u0.copy(), y0.copy()
        u_nan[1, ref.T_SWITCH:] = np.nan
        y_nan[1, ref.T_SWITCH:, 1] = np.nan
        nan_u = lp.run(nms, u_nan, y0)
        nan_y = lp.run(nms, u0, y_nan)
    assert np.all(base[2] == 0)
    assert np.all(lp.u_ref[1, ref.T_SWITCH:, 0] == 2.3) and np.array_equal(lp.u_ref[[0, 2, 3]], u0[[0, 2, 3]])
    cut = ref.loop_reference("refused", 1, nms, t_stop)
    print("t_stop", t_stop, "statuses", outside[2].tolist(), nan_u[2].tolist(), nan_y[2].tolist())
    _check_stopped("outside the bounds nstep %d" % nms, outside, base, 1, t_stop, 2, cut)
    _check_stopped("NaN input setpoint nstep %d" % nms, nan_u, base, 1, t_stop, 4, cut)
    _check_stopped("NaN output setpoint nstep %d" % nms, nan_y, base, 1, t_stop, 4, cut)


# ------------------------------------------ 5. a stop at the iteration cap mid-loop, <false, false>, then <true, false>
@pytest.mark.parametrize("nms", NMS)
def test_iteration_cap_mid_loop_and_the_safeguard(gpu, nms):
    t_stop = ref.t_stop(nms)
    with _Loop("cap", max_iter=100) as lp:
        base = lp.run(nms)
    with _Loop("cap") as lp:
        off = lp.run(nms)
        lp.eng.set_box_safeguard(True)
        on = lp.run(nms)
    assert np.all(base[2] == 0)
    print("t_stop", t_stop, "statuses: safeguard off", off[2].tolist(), "on", on[2].tolist())
    _check_stopped("cap <false,false> nstep %d" % nms, off, base, 1, t_stop, 4, ref.loop_reference("cap", 1, nms, t_stop))
    assert np.all(on[2] == 0)
    _check_loop("cap <true,false> nstep %d" % nms, on, lp.refs(nms), (1,))
    _bit_equal(on, off, [0, 2, 3])
    _check_loop("cap max_iter 100 nstep %d" % nms, base, lp.refs(nms), (1,))


# ----------------------------------------------------------------------------- 6. safeguard with output bounds, <true, true>
@pytest.mark.parametrize("nms", NMS)
def test_safeguard_with_output_bounds(gpu, nms):
    with _Loop("u-and-y-cap") as lp:
        cap = ref.LOOP_CASES["u-and-y-cap"]["max_iter"]
        off = lp.run(nms)
        lp.eng.set_box_safeguard(True)
        on = lp.run(nms)
    refs = lp.refs(nms)
    print("statuses: safeguard off", off[2].tolist(), "on", on[2].tolist())
    assert np.any(off[2] == 4)
    stopped = [b for b in refs if refs[b][5][0].iters >= cap + 2]
    assert stopped
    for b in stopped:                                   # stopped at the first solve: nothing moved
        assert off[2][b] == 4 and np.all(np.isnan(off[0][b])) and np.all(np.isnan(off[1][b]))
        assert np.array_equal(off[3][b], lp.case["x0"][b]) and np.array_equal(off[4][b], lp.case["up"][b])
        assert np.array_equal(off[5][b], lp.case["yp"][b])
    assert np.all(on[2] == 0)
    _check_loop("u-and-y-cap <true,true> nstep %d" % nms, on, refs, (0, 3))
    never = [b for b in refs if max(s.iters for s in refs[b][5]) <= cap]
    _bit_equal(on, off, never)                          # below the cap the safeguard changes nothing


# ------------------------------------------------------------------------ 7. loop and step agree, all four instantiations
TWINS = ref.LOOP_TWINS


@pytest.mark.parametrize("name,row,safe", TWINS, ids=["%s-row%d-%s" % (n, r, "safe" if s else "plain") for n, r, s in TWINS])
def test_loop_and_step_agree(gpu, name, row, safe):
    nms = 4
    with _Loop(name) as lp:
        case, m = lp.case, lp.case["spec"].m
        lp.eng.set_box_safeguard(safe)
        us, ys = lp.u_ref[:, row], lp.y_ref[:, row]
        u, _, status, iters = (x.copy() for x in lp.eng.step_setpoints(case["up"], case["yp"], us, ys))
        out = lp.run(nms, np.repeat(us[:, None], nms, axis=1), np.repeat(ys[:, None], nms, axis=1), steps=nms)
    yb = "y_min" in lp.bounds
    e = G._rel(out[0].reshape(case["B"], -1), u[:, :nms * m])
    print("%s <%s,%s> loop against step: %.2e  statuses %s / %s  iters %s" % (name, str(safe).lower(), str(yb).lower(), e, out[2].tolist(),
                                                                              status.tolist(), iters.tolist()))
    assert np.array_equal(out[2], status) and np.all(status == 0)
    assert e < TOL_LAW
    assert np.max(iters) >= 2                            # (an iteration took place)
    if safe:
        assert np.max(iters) > ref.LOOP_CASES[name]["max_iter"]    # (and the safeguard finished an instance)


# ------------------------------------------------------------------------------------------- 8. largest shape, step and loop
@pytest.mark.parametrize("name", list(ref.BIG_CASES))
def test_268_rows_step_and_loop(gpu, name):
    tec, bounds, nbox = ref.BIG_CASES[name]
    spec, t, pl = ref.big_spec(tec), ref.big(), ref.big()["plant"]
    Bn, n_steps = ref.BIG_B, ref.BIG_STEPS
    u_ref, y_ref = np.repeat(t["us"][:, None], n_steps, axis=1), np.repeat(t["ys"][:, None], n_steps, axis=1)
    with _engine(spec, bounds, B=Bn) as eng:
        u, cost, status, iters = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
        out = eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], t["x0"], t["up"], t["yp"], t["w"], u_ref, y_ref,
                                        n_mpc_step=ref.BIG_NMS)
        assert eng.closed_loop_kernel_name() == STEP_KERNEL_LOOP
    print("%s: 268 rows, box list %d, statuses: step %s loop %s" % (name, nbox, status.tolist(), out[2].tolist()))
    left_out = 0
    for b in range(Bn):
        left_out += _check_step(name, spec, b, ref.big_step_reference(name, b), u[b], cost[b], status[b], iters[b], refined_ok=True, **bounds)
    assert left_out == 0
    rows = (0, Bn - 1)
    _check_loop("%s 268 rows" % name, out, {b: ref.big_loop_reference(name, b) for b in rows}, rows, refined_ok=True)
