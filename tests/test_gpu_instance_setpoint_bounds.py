"""DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS: per-instance bounds (ddmpc_set_instance_input_bounds / _output_bounds) together with
per-instance, per-step setpoints (DDMPC_OPT_SETPOINT_BOX_LAW / _SETPOINT_CONVEX_LAW) on one handle of at most 271 rows -- the
channel-table (BoxChannels) instantiations of ddmpc_setpoint_box_step_kernel / ddmpc_closed_loop_setpoint_box_kernel
(csrc/ddmpc_setpoint_box_law.hpp), labelled "ddmpc_closed_loop_instance_setpoint_box_kernel" / "..._instance_setpoint_convex_kernel".

Fixtures, boxes and references: tests/_instance_setpoint_cases.py; every instance is compared with the reference of
tests/_setpoint_box_ref.py solved with ITS OWN bounds and setpoint.  Bars are the project's own (tests/test_gpu_setpoint_box_law.py):
inputs 1e-8 and cost 1e-9, relative; loop outputs and states 1e-9 of max(1, max|y|); law against law 1e-10.  `iters` and the
signed active set are compared where the reference's margin is at least 1e-7, and at most 1 in 16 compared instances may be left
out; tests/test_instance_setpoint_bounds_reference.py holds on the CPU that today none is.

The setpoint calls return optimal_u and the cost, and ddmpc_get_solution is refused after them, so "an active component equals its
instance's bound bit for bit" is asserted on the inputs (read off optimal_u); the output components of a box are judged through
`iters`, the inputs and the cost, as in tests/test_gpu_setpoint_box_law.py.

The <SAFE, YB, SLACK> instantiations with the channel table and the tests that launch them (step / loop):
  <0, 0, 0>  step: own reference[A-none, A-none-tec], refusal, safeguard (off)   loop: fused loop[none], refusal, twin, safeguard (off)
  <0, 1, 0>  step: own reference[C-none, C-none-tec], safeguard[C] (off)          loop: uniform rows[c-row0-none]
  <0, 0, 1>  step: own reference[A-convex-tec]                                    loop: uniform rows[u02-convex-tec]
  <0, 1, 1>  step: own reference[C-convex-tec], m != p                            loop: fused loop[convex-tec]
  <1, 0, 0>  step: safeguard[A], uniform rows[u02-none]                           loop: safeguard in the loop, uniform rows[u02-none]
  <1, 1, 0>  step: safeguard[C], uniform rows[c-row0-none]                        loop: uniform rows[c-row0-none]
  <1, 0, 1>  step + loop: uniform rows[u02-convex-tec]
  <1, 1, 1>  step + loop: uniform rows[c-row0-convex-tec]

One departure from the cases as first written down: box A leaves input channel 0 of instance 7 unbounded, so the setpoint
u_s = (2.3, 1.0) lies outside no bound of that instance.  The refusal test therefore bounds channel 0 of instance 7 ([0, 2] on both
channels, channel 0 unbounded at instance 3 only), and also asserts that under A proper instance 7 is NOT refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

import _instance_setpoint_cases as SC
import _setpoint_box_ref as ref
import test_gpu_closed_loop_plants as CP
import test_gpu_parity as T
from test_gpu_setpoint_box_law import _check_loop, _check_step, _input_set, _refused, _rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_U, TOL_COST, TOL_LAW = 1e-8, 1e-9, 1e-10
B8 = SC.B8
LOOP_NAME = {0: "ddmpc_closed_loop_instance_setpoint_box_kernel", 1: "ddmpc_closed_loop_instance_setpoint_convex_kernel"}
SHARED_LOOP_NAME = {0: "ddmpc_closed_loop_setpoint_box_kernel", 1: "ddmpc_closed_loop_setpoint_convex_kernel"}


def _law(eng, mode, on=True):
    (eng.set_setpoint_convex_law if SC.MODES[mode][0] else eng.set_setpoint_box_law)(on)


def _engine(mode, bx, B=B8, order="bounds-first", data=None, **kw):
    """A handle with the option, the rows of `bx` and option 19 / 20 (by the mode), the last two in the given order."""
    t = ref.tank() if data is None else data
    eng = T._engine(SC.spec_of(mode), 400, B, **kw)
    eng.set_instance_setpoint_bounds(True)
    if order == "bounds-first":
        SC.set_box(eng, bx)
        _law(eng, mode)
    else:
        _law(eng, mode)
        SC.set_box(eng, bx)
    eng.set_data(t["u_d"][:B], t["y_d"][:B])
    return eng


def _copy(call):
    return [np.asarray(x).copy() for x in call]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _loop_args(t, w, B=B8):
    pl = orc.FOUR_TANK
    return (pl["A"], pl["B"], pl["C"], pl["D"], t["x_end"][:B], t["up"][:B], t["yp"][:B], w)


def _const(v, n_steps):
    return np.repeat(np.asarray(v, float)[:, None], n_steps, axis=1)


# ---------------------------------------------------------------------------- 1. step against every instance's own reference
@pytest.mark.parametrize("order", ["bounds-first", "option-first"])
@pytest.mark.parametrize("mode", list(SC.MODES))
@pytest.mark.parametrize("name", SC.NAMES)
def test_step_against_every_instances_own_reference(gpu, name, mode, order):
    spec = SC.spec_of(mode)
    t = ref.tank()
    bx = SC.box(name)
    with _engine(mode, bx, order=order) as eng:
        u, cost, status, iters = _copy(eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
    left_out = 0
    for b in range(B8):
        sol = SC.step_reference(name, mode, b)
        # (_check_step: bars; iters; the inputs' signed set read off optimal_u by `==` against instance b's OWN bounds -- an active
        #  free input equals that instance's bound bit for bit, and no input sits at a neighbour's)
        left_out += _check_step("%s %s" % (name, mode), spec, b, sol, u[b], cost[b], status[b], iters[b], **SC.row(bx, b))
    assert left_out * 16 <= B8, left_out
    assert np.all(iters >= 2)
    if name == "A" and mode == "none":
        assert iters.tolist() == SC.A_NONE_ITERS


# ------------------------------------------------------------------------------------------- 2. uniform rows are the shared form
UNIFORM = {"u02": dict(u_min=[0.0, 0.0], u_max=[2.0, 2.0]),
           "c-row0": dict(u_min=[-4.0, -4.0], u_max=[6.0, 6.0], y_min=[-np.inf, 0.3], y_max=[1.1, np.inf])}


@pytest.mark.parametrize("mode", ["none", "convex-tec"])
@pytest.mark.parametrize("box", list(UNIFORM))
def test_uniform_rows_are_bit_equal_to_the_shared_bounds(gpu, box, mode):
    spec = SC.spec_of(mode)
    slack = SC.MODES[mode][0]
    t = ref.tank()
    bd = UNIFORM[box]
    if box == "c-row0":
        ulo, uhi, ylo, yhi = SC.box("C")
        assert np.array_equal(ulo[0], bd["u_min"]) and np.array_equal(yhi[0], bd["y_max"]) and np.array_equal(ylo[0], bd["y_min"])
    n_steps = 8
    w = spec.eps_max * np.random.default_rng(4).uniform(-1.0, 1.0, (B8, n_steps, spec.p))
    u_ref, y_ref = _const(t["us"], n_steps), _const(t["ys"], n_steps)

    def run(per_instance):
        out = {}
        with T._engine(spec, 400, B8) as eng:
            if per_instance:
                eng.set_instance_setpoint_bounds(True)
                eng.set_instance_input_bounds(np.tile(bd["u_min"], (B8, 1)), np.tile(bd["u_max"], (B8, 1)))
                if "y_min" in bd:
                    eng.set_instance_output_bounds(np.tile(bd["y_min"], (B8, 1)), np.tile(bd["y_max"], (B8, 1)))
            else:
                eng.set_input_bounds(bd["u_min"], bd["u_max"])
                if "y_min" in bd:
                    eng.set_output_bounds(bd["y_min"], bd["y_max"])
            _law(eng, mode)
            eng.set_data(t["u_d"], t["y_d"])
            for safe in (False, True):
                eng.set_box_safeguard(safe)
                res = _copy(eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
                for nms in (1, 3):
                    res += _copy(eng.closed_loop_setpoints(*_loop_args(t, w), u_ref, y_ref, n_mpc_step=nms))
                    res.append(eng.closed_loop_kernel_name())
                out[safe] = res
        return out

    shared, inst = run(False), run(True)
    for safe in (False, True):
        print(box, mode, "safeguard", safe, "status", shared[safe][2].tolist(), "iters", shared[safe][3].tolist())
        assert np.any(shared[safe][3] >= 2)                            # the box acts
        for a, b in zip(shared[safe], inst[safe]):
            if isinstance(a, str):
                assert (a, b) == (SHARED_LOOP_NAME[slack], LOOP_NAME[slack])
            else:
                assert _same(a, b)


# ------------------------------------------------------------------------------------------- 3. existing calls are unaffected
@pytest.mark.parametrize("mode", ["none-tec", "convex-tec"])
def test_existing_calls_are_unaffected(gpu, mode):
    spec = SC.spec_of(mode)
    t = ref.tank()
    bx = SC.box("C")
    w = spec.eps_max * np.random.default_rng(2).uniform(-1.0, 1.0, (B8, 9, spec.p))
    got = []
    for option in (False, True):
        with T._engine(spec, 400, B8) as eng:
            if option:
                eng.set_instance_setpoint_bounds(True)
                _law(eng, mode)
            SC.set_box(eng, bx)
            eng.set_data(t["u_d"], t["y_d"])
            res = _copy(eng.solve(t["up"], t["yp"])) + [eng.get_solution("ybar")]
            res += _copy(eng.step(t["up"], t["yp"])) + [eng.get_solution("ubar"), eng.get_solution("sigma")]
            res += _copy(eng.closed_loop(*_loop_args(t, w), n_mpc_step=2)) + [eng.get_solution("ubar"), eng.gain()]
            assert eng.closed_loop_kernel_name() == "ddmpc_closed_loop_instance_box_kernel"
            if option:
                # every row at the handle's own setpoint: the step of ddmpc_step to rounding, same iters and status
                u0, c0, s0, i0 = res[5:9]
                u1, c1, s1, i1 = _copy(eng.step_setpoints(t["up"], t["yp"], np.tile(spec.u_s, (B8, 1)), np.tile(spec.y_s, (B8, 1))))
                ec = np.max(np.abs(c1 - c0) / np.abs(c0))
                print("step_setpoints at the handle's setpoint vs step (%s): u %.2e cost %.2e iters %s" % (mode, _rel(u1, u0), ec, i1.tolist()))
                assert np.array_equal(s0, s1) and np.array_equal(i0, i1) and np.all(s1 <= 1) and np.all(i1 >= 2)
                assert _rel(u1, u0) < TOL_LAW and ec < TOL_LAW
                _refused(lambda: eng.get_solution("ubar"), L.ERR_NOT_READY, "ddmpc_step_setpoints")
                again = _copy(eng.step(t["up"], t["yp"]))                # (the handle's own setpoint was neither read nor changed)
                assert all(_same(a, b) for a, b in zip(again, res[5:9]))
            got.append(res)
    for a, b in zip(*got):
        assert _same(a, b)


# ------------------------------------------------------------------------------------------- 4. the refusal reads the instance's row
def test_the_refusal_reads_the_instances_row(gpu):
    mode = "none-tec"
    spec = SC.spec_of(mode)
    t = ref.tank()
    bx = SC.box("A", ufree=(3,))                                       # instance 7: [0, 2] on both channels; instance 0: [-4, 6]
    assert np.array_equal(bx[0][7], [0.0, 0.0]) and np.array_equal(bx[1][7], [2.0, 2.0]) and np.array_equal(bx[1][0], [6.0, 6.0])
    bad_u = t["us"].copy()
    bad_u[[0, 7]] = SC.BAD_US
    others = np.array([b not in (0, 7) for b in range(B8)])
    n_steps, nms, t_bad = 8, 2, 4
    w = spec.eps_max * np.random.default_rng(6).uniform(-1.0, 1.0, (B8, n_steps, spec.p))
    with _engine(mode, bx) as eng:
        u0, c0, s0, i0 = _copy(eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
        u1, c1, s1, i1 = _copy(eng.step_setpoints(t["up"], t["yp"], bad_u, t["ys"]))
        print("refusal: status", s1.tolist(), "iters", i1.tolist())
        assert np.all(s0 == 0)
        assert s1[7] == 2 and i1[7] == 0 and np.all(np.isnan(u1[7])) and np.isnan(c1[7])
        sol = SC.solve_at(mode, bx, 0, SC.BAD_US, t["ys"][0])           # inside instance 0's wider box: solved
        assert not _check_step("refusal", spec, 0, sol, u1[0], c1[0], s1[0], i1[0], **SC.row(bx, 0))
        for a, b in ((u1, u0), (c1, c0), (s1, s0), (i1, i0)):
            assert np.array_equal(a[others], b[others])
        # a NaN setpoint: solver_error there, the neighbours bit-equal
        for in_u in (True, False):
            nu, ny = t["us"].copy(), t["ys"].copy()
            (nu if in_u else ny)[3, 1] = np.nan
            u2, c2, s2, i2 = _copy(eng.step_setpoints(t["up"], t["yp"], nu, ny))
            k3 = np.arange(B8) != 3
            assert s2[3] == 4 and np.all(s2[k3] == 0)
            for a, b in ((u2, u0), (c2, c0), (i2, i0)):
                assert np.array_equal(a[k3], b[k3])
        # the fused loop: the schedule of instances 0 and 7 goes to the bad setpoint at step 4, instance 3's to NaN
        u_ref, y_ref = _const(t["us"], n_steps), _const(t["ys"], n_steps)
        good = _copy(eng.closed_loop_setpoints(*_loop_args(t, w), u_ref, y_ref, n_mpc_step=nms))
        assert eng.closed_loop_kernel_name() == LOOP_NAME[0] and np.all(good[2] == 0)
        u_bad = u_ref.copy()
        u_bad[[0, 7], t_bad:] = SC.BAD_US
        u_bad[3, t_bad:, 0] = np.nan
        stop = _copy(eng.closed_loop_setpoints(*_loop_args(t, w), u_bad, y_ref, n_mpc_step=nms))
    print("refusal in the loop: status", stop[2].tolist())
    keep = np.array([b not in (0, 3, 7) for b in range(B8)])
    assert stop[2][7] == 2 and stop[2][3] == 4 and stop[2][0] == 0 and np.all(stop[2][keep] == 0)
    for b in (3, 7):
        assert np.all(np.isnan(stop[0][b, t_bad:])) and np.all(np.isnan(stop[1][b, t_bad:]))
        assert np.array_equal(stop[0][b, :t_bad], good[0][b, :t_bad]) and np.array_equal(stop[1][b, :t_bad], good[1][b, :t_bad])
    assert np.all(np.isfinite(stop[0][0])) and not np.array_equal(stop[0][0, t_bad:], good[0][0, t_bad:])
    for a, b in zip(stop, good):
        assert np.array_equal(a[keep], b[keep])
    # box A proper leaves channel 0 of instance 7 unbounded: the same setpoint is inside its row, and it is solved
    bx = SC.box("A")
    with _engine(mode, bx) as eng:
        u3, c3, s3, i3 = _copy(eng.step_setpoints(t["up"], t["yp"], bad_u, t["ys"]))
    sol = SC.solve_at(mode, bx, 7, SC.BAD_US, t["ys"][7])
    assert not _check_step("not refused", spec, 7, sol, u3[7], c3[7], s3[7], i3[7], **SC.row(bx, 7))


# ------------------------------------------------------------------------------------------- 5. fused loop against the schedule reference
@pytest.mark.parametrize("nms", SC.LOOP_NMS)
@pytest.mark.parametrize("mode", list(SC.LOOP_MODES))
def test_fused_loop_against_the_schedule_reference(gpu, mode, nms):
    case, u_ref, y_ref = SC.loop_case(mode)
    pl, Bn = case["plant"], case["B"]
    bx = SC.loop_box(SC.LOOP_MODES[mode])
    args = (pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"])
    with _engine(mode, bx, B=Bn, data=case) as eng:
        out = _copy(eng.closed_loop_setpoints(*args, u_ref, y_ref, n_mpc_step=nms))
        assert eng.closed_loop_kernel_name() == LOOP_NAME[SC.MODES[mode][0]]
    refs = {b: SC.loop_reference(mode, b, nms) for b in range(Bn)}
    _check_loop("%s nstep %d" % (mode, nms), out, refs, range(Bn))
    ulo, uhi = bx[0], bx[1]
    for b in range(Bn):
        assert all(s.margin >= SC.MARGIN for s in refs[b][5]), b
        assert np.all(out[0][b] >= ulo[b]) and np.all(out[0][b] <= uhi[b]), b      # inside ITS box, the bound itself included


def test_loop_and_step_twins_are_bit_equal(gpu):
    """n_steps = n_mpc_step = 4 on a constant schedule: the loop's one solve is the step's, and the four inputs it applies are the
    step's first four, bit for bit (both modes of the loop fixture)."""
    for mode in SC.LOOP_MODES:
        case, u_ref, y_ref = SC.loop_case(mode)
        pl, Bn, m = case["plant"], case["B"], case["spec"].m
        bx = SC.loop_box(SC.LOOP_MODES[mode])
        us, ys = u_ref[:, 0], y_ref[:, 0]
        with _engine(mode, bx, B=Bn, data=case) as eng:
            u, cost, status, iters = _copy(eng.step_setpoints(case["up"], case["yp"], us, ys))
            out = _copy(eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"][:, :4],
                                                  _const(us, 4), _const(ys, 4), n_mpc_step=4))
        print("twin", mode, "status", status.tolist(), "iters", iters.tolist())
        assert np.all(status == 0) and np.all(out[2] == 0) and np.all(iters >= 2)
        assert np.array_equal(out[0].reshape(Bn, -1), u[:, :4 * m])


# ----------------------------------------------------------------------------------------------------------- 6. safeguard
@pytest.mark.parametrize("name", SC.NAMES)
def test_safeguard_finishes_the_instances_at_the_cap(gpu, name):
    mode, cap = "none", 6
    spec = SC.spec_of(mode)
    t = ref.tank()
    bx = SC.box(name)
    res = {}
    with _engine(mode, bx, max_iter=cap) as eng:
        for safe in (False, True):
            eng.set_box_safeguard(safe)
            res[safe] = _copy(eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
    ref_iters = np.array([SC.step_reference(name, mode, b).iters for b in range(B8)])
    print("safeguard %s: reference iters %s  GPU iters off %s on %s  status off %s on %s" %
          (name, ref_iters.tolist(), res[False][3].tolist(), res[True][3].tolist(), res[False][2].tolist(), res[True][2].tolist()))
    over = ref_iters > cap
    assert np.nonzero(over)[0].tolist() == [6, 7]
    u0, c0, s0, i0 = res[False]
    u1, c1, s1, i1 = res[True]
    assert np.all(s0[over] == 4) and np.all(i0[over] == cap) and np.all(s0[~over] == 0)
    assert np.all(s1 == 0) and np.all(i1[over] > cap)
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[~over], b[~over])
    for b in np.nonzero(over)[0]:
        sol = SC.step_reference(name, mode, b)                          # (the optimum is unique: the primal-dual reference, uncapped)
        eu = np.max(np.abs(u1[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(c1[b] - sol.cost) / abs(sol.cost)
        print("safeguard %s b=%d iters %d err_u %.1e err_cost %.1e" % (name, b, i1[b], eu, ec))
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        lo, hi = bx[0][b], bx[1][b]
        mine = _input_set(spec, u1[b], lo, hi)                          # held at ITS bounds exactly
        assert np.array_equal(mine, sol.active[:mine.size]), b


def test_safeguard_in_the_loop(gpu):
    mode, cap, name = "none", 6, "A"
    spec = SC.spec_of(mode)
    t = ref.tank()
    bx = SC.box(name)
    w = spec.eps_max * np.random.default_rng(7).uniform(-1.0, 1.0, (B8, 4, spec.p))
    res = {}
    with _engine(mode, bx, max_iter=cap) as eng:
        for safe in (False, True):
            eng.set_box_safeguard(safe)
            res[safe] = _copy(eng.closed_loop_setpoints(*_loop_args(t, w), _const(t["us"], 4), _const(t["ys"], 4), n_mpc_step=4))
            assert eng.closed_loop_kernel_name() == LOOP_NAME[0]
    print("safeguard in the loop: status off %s on %s" % (res[False][2].tolist(), res[True][2].tolist()))
    over = np.array([SC.step_reference(name, mode, b).iters > cap for b in range(B8)])
    assert np.all(res[False][2][over] == 4) and np.all(res[False][2][~over] == 0) and np.all(np.isnan(res[False][0][over]))
    assert np.all(res[True][2] == 0)
    for a, b in zip(res[False], res[True]):
        assert np.array_equal(a[~over], b[~over])
    for b in np.nonzero(over)[0]:
        sol = SC.step_reference(name, mode, b)
        eu = np.max(np.abs(res[True][0][b].reshape(-1) - sol.optimal_u[:4 * spec.m])) / np.max(np.abs(sol.optimal_u))
        print("safeguard in the loop b=%d err_u %.1e" % (b, eu))
        assert eu < TOL_U, (b, eu)


# ------------------------------------------------------------------------------------------- 7. channel indexing with m != p
def test_channel_indexing_on_a_plant_with_m_ne_p(gpu):
    case, ulo, uhi, ylo, yhi, us, ys = SC.mne()
    spec = case["spec"]
    with CP.engine(case) as eng:
        eng.set_instance_setpoint_bounds(True)
        eng.set_setpoint_convex_law(True)
        eng.set_instance_input_bounds(ulo, uhi)
        eng.set_instance_output_bounds(ylo, yhi)
        eng.set_data(case["u_d"], case["y_d"])
        u, cost, status, iters = _copy(eng.step_setpoints(case["up"], case["yp"], us, ys))
    print("m != p status", status.tolist(), "iters", iters.tolist(), "perturbation", SC.MNE_PERTURBATION)
    nfree = spec.L - spec.n
    for b in range(4):
        sol = SC.mne_reference(b)
        nu_act, ny_act = SC.mne_active(spec, sol)
        assert sol.margin >= 1e-6 and nu_act >= 1 and ny_act >= 1
        assert not _check_step("m != p", spec, b, sol, u[b], cost[b], status[b], iters[b], u_min=ulo[b], u_max=uhi[b], refined_ok=True)
        free_u = u[b].reshape(spec.L, spec.m)[:nfree]
        assert np.sum(free_u[:, 1] == uhi[b, 1]) == nu_act, b            # held at ITS bound exactly


# ----------------------------------------------------------------------------------------------------------- 8. option surface
def test_option_surface(gpu):
    t = ref.tank()
    lib = L.load()
    base = dict(n=4, m=2, p=2, L_=30, N=400, Q=3.0, R=1e-4, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002,
                lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0)
    dense_q = 3.0 * np.eye(60) + 0.1 * (np.eye(60, k=1) + np.eye(60, k=-1))
    lo, hi = np.zeros((2, 2)), np.full((2, 2), 2.0)
    up, yp, us, ys = t["up"][:2], t["yp"][:2], t["us"][:2], t["ys"][:2]
    with BatchedDDMPC(**base) as eng:
        assert lib.ddmpc_set_option(eng._h, L.OPT_INSTANCE_SETPOINT_BOUNDS, 2) == L.ERR_INVALID
        assert lib.ddmpc_set_option(eng._h, L.OPT_INSTANCE_SETPOINT_BOUNDS, -1) == L.ERR_INVALID
    for over, words in ((dict(L_=64), ("271", "272")),                # 4 (64 + 4) = 272 rows
                        (dict(controller_type=L.NOMINAL), ("NOMINAL",)),
                        (dict(Q=dense_q), ("DDMPC_WEIGHT_DENSE",))):
        with BatchedDDMPC(**{**base, **over}) as eng:
            for word in words:
                _refused(lambda: eng.set_instance_setpoint_bounds(True), L.ERR_UNSUPPORTED, word)
            eng.set_instance_setpoint_bounds(False)                   # 0 is accepted there
    for slack, law in ((L.SLACK_NONE, "set_setpoint_box_law"), (L.SLACK_CONVEX, "set_setpoint_convex_law")):
        name = "DDMPC_OPT_SETPOINT_BOX_LAW" if slack == L.SLACK_NONE else "DDMPC_OPT_SETPOINT_CONVEX_LAW"
        with BatchedDDMPC(slack_type=slack, **base) as eng:
            # without the option the two refuse each other as they always did
            eng.set_instance_input_bounds(lo, hi)
            _refused(lambda: getattr(eng, law)(True), L.ERR_UNSUPPORTED, "per-instance")
            # bounds, the option, then 19 / 20
            eng.set_instance_setpoint_bounds(True)
            getattr(eng, law)(True)
            # 1 -> 0 with both present: refused, the message says which to remove first
            _refused(lambda: eng.set_instance_setpoint_bounds(False), L.ERR_UNSUPPORTED, name)
            _refused(lambda: eng.set_instance_setpoint_bounds(False), L.ERR_UNSUPPORTED, "remove")
            eng.set_data(t["u_d"][:2], t["y_d"][:2])
            assert np.all(eng.step_setpoints(up, yp, us, ys)[2] == 0)
            # changing the option forgets nothing ddmpc_prepare kept
            eng.set_instance_setpoint_bounds(True)
            assert eng.setpoint_gain().shape == (2, 4, 136)
            # ... and either of the two may go first
            getattr(eng, law)(False)
            eng.set_instance_setpoint_bounds(False)
            _refused(lambda: getattr(eng, law)(True), L.ERR_UNSUPPORTED, "per-instance")
            eng.set_instance_setpoint_bounds(True)
            getattr(eng, law)(True)
            eng.set_instance_input_bounds(None, None)
            eng.set_instance_setpoint_bounds(False)
            _refused(lambda: eng.set_instance_input_bounds(lo, hi), L.ERR_UNSUPPORTED, name)
            eng.set_instance_setpoint_bounds(True)
            eng.set_instance_output_bounds(np.full((2, 2), 0.3), np.full((2, 2), 1.1))       # the option first, then the bounds
    # every other refusal of the bounds calls stays with the option on
    with BatchedDDMPC(**base) as eng:
        eng.set_instance_setpoint_bounds(True)
        eng.set_refinement("always")
        _refused(lambda: eng.set_instance_input_bounds(lo, hi), L.ERR_UNSUPPORTED, "REFINE_ALWAYS")
    q = np.full(60, 3.0)
    q[2 * 7 + 1] = 0.0                                                # output channel 1, free step 7
    with BatchedDDMPC(**{**base, "Q": q, "R": np.full(60, 1e-4), "slack_type": L.SLACK_CONVEX}) as eng:
        eng.set_instance_setpoint_bounds(True)                        # (a zero Q entry under the slack box: both refuse it, in either order)
        _refused(lambda: eng.set_instance_input_bounds(lo, hi), L.ERR_UNSUPPORTED, "Q entry")
        _refused(lambda: eng.set_setpoint_convex_law(True), L.ERR_UNSUPPORTED, "Q entry 0")
    # with the option 1 and neither 19 nor 20 on, a bounded handle refuses the setpoint calls as it does today
    pl = orc.FOUR_TANK
    with BatchedDDMPC(**base) as eng:
        eng.set_instance_setpoint_bounds(True)
        eng.set_instance_input_bounds(lo, hi)
        eng.set_data(t["u_d"][:2], t["y_d"][:2])
        _refused(lambda: eng.step_setpoints(up, yp, us, ys), L.ERR_UNSUPPORTED, "DDMPC_OPT_SETPOINT_LAW")
        _refused(lambda: eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], np.zeros((2, 4)), up, yp, np.zeros((2, 3, 2)),
                                                   _const(us, 3), _const(ys, 3)), L.ERR_UNSUPPORTED, "DDMPC_OPT_SETPOINT_LAW")
        _refused(lambda: eng.set_setpoint_law(True), L.ERR_UNSUPPORTED, "bounds")       # option 18 keeps refusing bounds


# ----------------------------------------------------------------------------------------------------------- 9. example script
def test_example_script_with_both_spreads(gpu, tmp_path):
    """--bound_spread together with --setpoint_spread turns the option on: instance b tracks its own equilibrium inside
    [0 - S b / 7, 2 + S b / 7]; every instance against the schedule reference with its own row and setpoint."""
    t_sim, Bn, sp_spread, b_spread = 24, 8, 0.05, 0.5
    out = tmp_path / "loop.npz"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "batched_data_driven_mpc_example.py"), "--setpoint_spread",
                          str(sp_spread), "--bound_spread", str(b_spread), "--u_min", "0", "--u_max", "2", "--batch", str(Bn),
                          "--t_sim", str(t_sim), "--seed", "0", "--out", str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert LOOP_NAME[0] in res.stdout
    z = np.load(out)
    spec = orc.spec_from_params()
    us = spec.u_s + sp_spread * np.random.default_rng(0).uniform(-1.0, 1.0, (Bn, spec.m))
    ys = us @ ref.dc_gain(orc.FOUR_TANK).T
    assert np.all(z["status"] == 0) and np.array_equal(z["u_s"], us) and np.array_equal(z["y_s"], ys)
    grow = b_spread * np.arange(Bn) / (Bn - 1)
    for b in range(Bn):
        lo, hi = np.full(2, 0.0 - grow[b]), np.full(2, 2.0 + grow[b])
        inst = orc.generate_instance(b)
        w = inst["plant"].eps_max * inst["rng"].uniform(-1.0, 1.0, (t_sim + 1, spec.p))
        u_r, y_r, _, _, _ = ref.schedule_loop(spec, inst["u_d"], inst["y_d"], inst["plant"], w, np.tile(us[b], (t_sim + 1, 1)),
                                              np.tile(ys[b], (t_sim + 1, 1)), u_min=lo, u_max=hi, n_mpc_step=spec.n)
        eu = np.max(np.abs(z["u_sys"][b] - u_r)) / np.max(np.abs(u_r))
        ey = np.max(np.abs(z["y_sys"][b] - y_r)) / max(1.0, np.max(np.abs(y_r)))
        print("example instance %d: u %.2e  y %.2e  min u %.3f max u %.3f" % (b, eu, ey, z["u_sys"][b].min(), z["u_sys"][b].max()))
        assert eu < TOL_U and ey < 1e-9, (b, eu, ey)
        assert np.min(z["u_sys"][b]) >= lo[0] and np.max(z["u_sys"][b]) <= hi[0]
    # beyond 271 rows the combination raises with a message that names the limit ((2 + 2)(64 + 4) = 272 rows)
    cfg = tmp_path / "long.yaml"
    src = open(os.path.join(ROOT, "examples", "config", "controllers", "data_driven_mpc_example_params.yaml")).read()
    assert "L: 30" in src
    cfg.write_text(src.replace("L: 30", "L: 64"))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "batched_data_driven_mpc_example.py"), "--setpoint_spread",
                          str(sp_spread), "--bound_spread", str(b_spread), "--u_min", "0", "--u_max", "2", "--batch", "2", "--t_sim", "4",
                          "--controller_config_path", str(cfg)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-1000:], res.stderr[-1000:])
    assert res.returncode != 0 and "271" in res.stderr and "272" in res.stderr
