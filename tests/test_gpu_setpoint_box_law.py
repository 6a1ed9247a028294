"""DDMPC_OPT_SETPOINT_BOX_LAW: per-instance, per-step setpoints on handles with input / output bounds (ddmpc_step_setpoints and
ddmpc_closed_loop_setpoints on Route::BoxLaw; kernels in csrc/ddmpc_setpoint_box_law.hpp).

Four-tank, L = 30, n = 4, N = 400 (136 rows: both homes of the k x k system), batch 8.  References: the full-space bounded solve
and the schedule loop of tests/_setpoint_box_ref.py.  Bars are the project's own: inputs 1e-8, cost 1e-9, outputs and states 1e-9
of max(1, max|y|), law against law 1e-10.  `iters` and the signed active set are compared only where the reference's margin is
at least 1e-7, and at most 1 in 16 compared instances may be left out (the rule of test_gpu_input_bounds.py).  The premises
(every reference solve optimal, the margins, the active counts) are held on the CPU by tests/test_setpoint_box_law_reference.py.

The new calls return optimal_u and the cost, and ddmpc_get_solution is not available after them: the signed active set is read
off the inputs (an input held at a bound is that bound exactly); the output components of a box are judged through `iters`,
the inputs and the cost."""
import os
import subprocess
import sys

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

import _box_safeguard_ref as sg
import _setpoint_box_ref as ref
import _setpoint_law_ref as sref
import test_gpu_closed_loop_plants as plants
import test_gpu_parity as T
import test_setpoint_box_law_reference as model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_U, TOL_COST, TOL_Y, TOL_LAW = 1e-8, 1e-9, 1e-9, 1e-10
INF = np.inf
B8 = ref.B8
STEP_KERNEL_LOOP = "ddmpc_closed_loop_setpoint_box_kernel"


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _refused(fn, code, word):
    with pytest.raises(L.DDMPCError) as e:
        fn()
    assert e.value.code == code and word in e.value.message, (e.value.code, e.value.message)


def _bound(eng, u_min=None, u_max=None, y_min=None, y_max=None):
    if u_min is not None:
        eng.set_input_bounds(u_min, u_max)
    if y_min is not None:
        eng.set_output_bounds(y_min, y_max)


def _engine(spec, box, B=B8, option=True, **kw):
    t = ref.tank()
    eng = T._engine(spec, 400, B, **kw)
    if option:
        eng.set_setpoint_box_law(True)
    _bound(eng, **box)
    eng.set_data(t["u_d"][:B], t["y_d"][:B])
    return eng


def _input_set(spec, u, lo, hi):
    """The signed set of the bounded inputs, read off optimal_u [L m], in the order of the helper's box (time, channel)."""
    nfree = spec.L - spec.n if spec.tec else spec.L
    lo, hi = np.broadcast_to(np.asarray(lo, float), (spec.m,)), np.broadcast_to(np.asarray(hi, float), (spec.m,))
    ch = np.nonzero(np.isfinite(lo) | np.isfinite(hi))[0]
    v = u.reshape(spec.L, spec.m)[:nfree][:, ch]
    return ((v == hi[ch]).astype(int) - (v == lo[ch]).astype(int)).reshape(-1)


def _check_step(tag, spec, b, sol, u, cost, status, iters, u_min=None, u_max=None, refined_ok=False, **_):
    """Instance b against its reference: bars; iters and the inputs' signed set under the margin rule -> left out?
    refined_ok: the law of an instance may come from refining solves (DDMPC_REFINE_AUTO), and such an instance reports
    optimal_inaccurate when its final active set is not empty, as on ddmpc_step; it is held to the same bars."""
    assert sol.status == "optimal", (tag, b, sol.status)
    assert status == 0 or (refined_ok and status == 1 and np.count_nonzero(sol.active) > 0), (tag, b, status)
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s b=%d iters %d/%d k %d margin %.1e err_u %.1e err_cost %.1e" %
          (tag, b, iters, sol.iters, np.count_nonzero(sol.active), sol.margin, eu, ec))
    assert eu < TOL_U and ec < TOL_COST, (tag, b, eu, ec)
    if sol.margin < 1e-7:
        return True
    assert iters == sol.iters, (tag, b, iters, sol.iters)
    if u_min is not None:
        mine = _input_set(spec, u, u_min, u_max)
        assert np.array_equal(mine, sol.active[:mine.size]), (tag, b)
        v = u.reshape(spec.L, spec.m)[:spec.L - spec.n if spec.tec else spec.L]
        lo, hi = np.asarray(u_min, float), np.asarray(u_max, float)
        assert np.all(v >= lo - 1e-12 * np.maximum(np.abs(lo), 1.0)) and np.all(v <= hi + 1e-12 * np.maximum(np.abs(hi), 1.0)), (tag, b)
    return False


# ------------------------------------------------------------------------------------------------------ 1. option contract
def test_option_contract(gpu):
    t = ref.tank()
    base = dict(n=4, m=2, p=2, L_=30, N=400, Q=3.0, R=1e-4, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002,
                lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0)
    dense_q = 3.0 * np.eye(60) + 0.1 * (np.eye(60, k=1) + np.eye(60, k=-1))
    refusals = [
        (dict(controller_type=L.NOMINAL), "NOMINAL"),
        (dict(slack_type=L.SLACK_CONVEX), "CONVEX"),
        (dict(Q=dense_q), "DDMPC_WEIGHT_DENSE"),
        (dict(L_=64), "271"),                                         # 4 * (64 + 4) = 272 rows
        (dict(N=6000), "LDS"),                                        # the trajectory is beyond the LDS
        (dict(m=17, p=17, n=8, L_=16, N=600, u_s=np.zeros(17), y_s=np.zeros(17)), "n*(m+p)"),      # n (m + p) = 272
    ]
    for over, word in refusals:
        with BatchedDDMPC(**{**base, **over}) as eng:
            _refused(lambda: eng.set_setpoint_box_law(True), L.ERR_UNSUPPORTED, word)
            eng.set_setpoint_box_law(False)                           # 0 is accepted everywhere
    lib = L.load()
    up, yp, us, ys = t["up"][:2], t["yp"][:2], t["us"][:2], t["ys"][:2]
    for setb in (lambda e: e.set_input_bounds(0.0, 2.0), lambda e: e.set_output_bounds(0.0, 2.0)):
        with BatchedDDMPC(**base) as eng:                             # bounds first, then the option
            setb(eng)
            eng.set_setpoint_box_law(True)
            eng.set_setpoint_law(True)                                # both on: accepted, 19 governs
        with BatchedDDMPC(**base) as eng:                             # the option first, then the bounds
            eng.set_setpoint_box_law(True)
            setb(eng)
        with BatchedDDMPC(**base) as eng:                             # with only 18 on the bounds stay refused
            eng.set_setpoint_law(True)
            _refused(lambda: setb(eng), L.ERR_UNSUPPORTED, "DDMPC_OPT_SETPOINT_LAW")
    with BatchedDDMPC(**base) as eng:
        assert lib.ddmpc_set_option(eng._h, L.OPT_SETPOINT_BOX_LAW, 2) == L.ERR_INVALID
        eng.set_data(t["u_d"][:2], t["y_d"][:2])
        _refused(lambda: eng.step_setpoints(up, yp, us, ys), L.ERR_UNSUPPORTED, "DDMPC_OPT_SETPOINT_LAW")
    pl = orc.FOUR_TANK
    w = np.zeros((2, 3, 2))
    with BatchedDDMPC(**base) as eng:                                 # the three calls with 19 alone, bounded
        eng.set_setpoint_box_law(True)
        eng.set_input_bounds(0.0, 2.0)
        _refused(lambda: eng.step_setpoints(up, yp, us, ys), L.ERR_NOT_READY, "ddmpc_set_data")
        eng.set_data(t["u_d"][:2], t["y_d"][:2])
        _refused(eng.setpoint_gain, L.ERR_NOT_READY, "ddmpc_prepare")
        eng.prepare()
        assert eng.setpoint_gain().shape == (2, 4, 136)
        eng.step(up, yp)
        first = eng.get_solution("ubar")
        _, _, st, _ = eng.step_setpoints(up, yp, us, ys)
        assert np.all(st == 0)
        _refused(lambda: eng.get_solution("ubar"), L.ERR_NOT_READY, "ddmpc_step_setpoints")
        eng.step(up, yp)                                              # readable again after a step
        assert np.array_equal(eng.get_solution("ubar"), first)
        out = eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], np.zeros((2, 4)), up, yp, w,
                                        np.repeat(us[:, None], 3, axis=1), np.repeat(ys[:, None], 3, axis=1))
        assert eng.closed_loop_kernel_name() == STEP_KERNEL_LOOP and np.all(out[2] == 0)
        _refused(lambda: eng.get_solution("sigma"), L.ERR_NOT_READY, "ddmpc_closed_loop_setpoints")
        eng.set_setpoint_box_law(False)                               # changing the value forgets the preparation
        eng.set_setpoint_box_law(True)
        _refused(eng.setpoint_gain, L.ERR_NOT_READY, "ddmpc_prepare")


# ------------------------------------------------------------------------------------------- 2. step against the reference
STEP_CELLS = [(box, tec, False) for box in ref.STEP_BOXES for tec in (True, False)] + [("tight", True, True)]


@pytest.mark.parametrize("box,tec,diag", STEP_CELLS, ids=["%s-%s%s" % (b, "terminal" if t else "no-terminal", "-diag" if d else "")
                                                          for b, t, d in STEP_CELLS])
def test_step_against_the_reference(gpu, box, tec, diag):
    spec = ref.spec(tec, diag)
    t = ref.tank()
    lo, hi, home = ref.STEP_BOXES[box]
    bounds = dict(u_min=lo, u_max=hi)
    with _engine(spec, bounds, diag=diag) as eng:
        u, cost, status, iters = eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"])
    left_out, ks = 0, []
    for b in range(B8):
        sol = ref.step_reference(box, tec, diag, b)
        left_out += _check_step(box, spec, b, sol, u[b], cost[b], status[b], iters[b], **bounds)
        ks.append(int(np.count_nonzero(sol.active)))
    assert left_out * 16 <= B8, left_out
    if home == "lds":                                   # both homes of the k x k system: LDS up to 16, the global slice beyond
        assert 1 <= min(ks) and max(ks) <= 16 and np.all(iters >= 2), ks
    if home == "global":
        assert min(ks) > 16, ks


# ------------------------------------------------------------------------------------------------------ 3. output bounds
@pytest.mark.parametrize("name", list(ref.Y_CASES))
def test_output_bounds(gpu, name):
    tec, bounds = ref.Y_CASES[name]
    spec = ref.spec(tec)
    t = ref.tank()
    with _engine(spec, bounds) as eng:
        u, cost, status, iters = eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"])
    left_out = 0
    for b in range(B8):
        sol = ref.y_reference(name, b)
        assert np.count_nonzero(sol.active) >= 1
        left_out += _check_step(name, spec, b, sol, u[b], cost[b], status[b], iters[b], **bounds)
    assert left_out == 0, left_out                      # (nobody is left out in these cases: held on the CPU)
    assert np.all(iters >= 2)


# ------------------------------------------------------------------------------------------- 4. setpoints outside the box
def test_setpoint_outside_the_box(gpu):
    t = ref.tank()
    us, ys = ref.outside_setpoints(t)
    bounds = dict(u_min=[0.0, 0.0], u_max=[2.0, 2.0])
    bad = sorted(ref.OUTSIDE)
    keep = np.array([b not in ref.OUTSIDE for b in range(B8)])
    # without the terminal constraint such a setpoint is legitimate: the inputs go to the bound
    spec = ref.spec(False)
    with _engine(spec, bounds) as eng:
        u, cost, status, iters = eng.step_setpoints(t["up"], t["yp"], us, ys)
    for b in bad:
        assert not _check_step("outside", spec, b, ref.outside_reference(b), u[b], cost[b], status[b], iters[b], **bounds)
    # with it: infeasible, NaN, iters 0 there; the other five bit-equal to a call without them
    spec = ref.spec(True)
    with _engine(spec, bounds) as eng:
        u0, c0, s0, i0 = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"]))
        u1, c1, s1, i1 = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], us, ys))
        assert np.all(s0 == 0)
        assert np.all(s1[bad] == 2) and np.all(i1[bad] == 0) and np.all(np.isnan(u1[bad])) and np.all(np.isnan(c1[bad]))
        for a, b_ in ((u1, u0), (c1, c0), (s1, s0), (i1, i0)):
            assert np.array_equal(a[keep], b_[keep])
        # a NaN setpoint: solver_error there, the neighbours bit-equal
        for in_u in (True, False):
            nu, ny = t["us"].copy(), t["ys"].copy()
            (nu if in_u else ny)[3, 1] = np.nan
            u2, c2, s2, i2 = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], nu, ny))
            k3 = np.arange(B8) != 3
            assert s2[3] == 4 and np.all(s2[k3] == 0)
            for a, b_ in ((u2, u0), (c2, c0), (i2, i0)):
                assert np.array_equal(a[k3], b_[k3])


# ------------------------------------------------------------------------------------------- 5. identity and independence
@pytest.mark.parametrize("box", ["wide", "tight"])
def test_identity_and_independence(gpu, box):
    spec = ref.spec()
    t = ref.tank()
    lo, hi, _ = ref.STEP_BOXES[box]
    own_u, own_y = np.tile(spec.u_s, (B8, 1)), np.tile(spec.y_s, (B8, 1))
    d = t
    with _engine(spec, dict(u_min=lo, u_max=hi)) as eng:
        u0, c0, s0, i0 = (x.copy() for x in eng.step(t["up"], t["yp"]))
        u1, c1, s1, i1 = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], own_u, own_y))
        assert np.array_equal(s0, s1) and np.all(s1 == 0)
        # iters where the margin allows (the reference at the handle's own setpoints)
        left_out = 0
        for b in range(B8):
            sol = ref.solve(spec, d["u_d"][b], d["y_d"][b], t["up"][b], t["yp"][b], spec.u_s, spec.y_s, u_min=lo, u_max=hi)
            if sol.margin < 1e-7:
                left_out += 1
                continue
            assert i0[b] == i1[b] == sol.iters, (b, i0[b], i1[b], sol.iters)
        assert left_out * 16 <= B8
        ec = np.max(np.abs(c1 - c0) / np.abs(c0))
        print("step_setpoints at the handle's setpoints vs step (%s): u %.2e cost %.2e" % (box, _rel(u1, u0), ec))
        assert _rel(u1, u0) < TOL_LAW and ec < TOL_LAW
        # the setpoints of instances 1 .. 7 change: instance 0 stays bit-equal
        mix_u, mix_y = own_u.copy(), own_y.copy()
        mix_u[1:], mix_y[1:] = t["us"][1:], t["ys"][1:]
        u2, c2, s2, i2 = (x.copy() for x in eng.step_setpoints(t["up"], t["yp"], mix_u, mix_y))
        assert np.array_equal(u2[0], u1[0]) and c2[0] == c1[0] and s2[0] == 0 and i2[0] == i1[0]
        assert not np.array_equal(u2[1:], u1[1:])
        # the handle's own setpoints were neither read nor changed
        u4, c4, _, i4 = eng.step(t["up"], t["yp"])
        assert np.array_equal(u4, u0) and np.array_equal(c4, c0) and np.array_equal(i4, i0)


# ------------------------------------------------------------------------------------- 6. no change for the existing calls
def test_existing_calls_are_bit_equal_with_the_option_on(gpu):
    spec = ref.spec()
    t = ref.tank()
    pl = orc.FOUR_TANK
    w = spec.eps_max * np.random.default_rng(2).uniform(-1.0, 1.0, (B8, 9, spec.p))
    got = []
    for option in (False, True):
        with _engine(spec, dict(u_min=[0.0, 0.0], u_max=[2.0, 2.0]), option=option) as eng:
            cold = [x.copy() for x in eng.solve(t["up"], t["yp"])]
            sol = eng.get_solution("ybar")
            warm = [x.copy() for x in eng.step(t["up"], t["yp"])]
            solw = eng.get_solution("sigma")
            loop = eng.closed_loop(pl["A"], pl["B"], pl["C"], pl["D"], t["x_end"], t["up"], t["yp"], w, n_mpc_step=2)
            assert eng.closed_loop_kernel_name() == "ddmpc_closed_loop_box_kernel"
            got.append(cold + [sol] + warm + [solw] + list(loop) + [eng.get_solution("ubar"), eng.gain()])
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    # without a finite bound the new calls are those of DDMPC_OPT_SETPOINT_LAW, bit-equal
    got = []
    n_steps = w.shape[1]
    u_ref, y_ref = np.repeat(t["us"][:, None], n_steps, axis=1), np.repeat(t["ys"][:, None], n_steps, axis=1)
    for which in (18, 19):
        with T._engine(spec, 400, B8) as eng:
            (eng.set_setpoint_law if which == 18 else eng.set_setpoint_box_law)(True)
            eng.set_data(t["u_d"], t["y_d"])
            step = [x.copy() for x in eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"])]
            loop = eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], t["x_end"], t["up"], t["yp"], w, u_ref, y_ref, n_mpc_step=2)
            assert eng.closed_loop_kernel_name() == "ddmpc_closed_loop_setpoint_kernel"
            got.append(step + list(loop) + [eng.setpoint_gain()])
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert np.all(got[0][2] == 0) and np.all(got[0][3] == 1)


# ----------------------------------------------------------------------------------------------------------- 7. fused loop
_LOOP = {}


def _tank_loop():
    """The construction of test_gpu_setpoint_law.py: B = 4, 21 steps, instance b switches at step 10 between two equilibria."""
    if not _LOOP:
        from direct_data_driven_mpc_amd.harness import generate_batch
        Bn, n_steps = 4, 21
        spec = ref.spec()
        pl = orc.FOUR_TANK
        d = generate_batch(range(Bn), N=400)
        A, Bm, Cm, D = (np.asarray(pl[k], float) for k in ("A", "B", "C", "D"))
        dc = Cm @ np.linalg.inv(np.eye(A.shape[0]) - A) @ Bm + D
        rng = np.random.default_rng(21)
        us12 = spec.u_s + rng.uniform(-0.3, 0.3, (2, Bn, spec.m))
        u_ref = np.where(np.arange(n_steps)[None, :, None] < 10, us12[0][:, None, :], us12[1][:, None, :])
        y_ref = u_ref @ dc.T
        w = spec.eps_max * rng.uniform(-1.0, 1.0, (Bn, n_steps, spec.p))
        up = d["u_d"][:, -spec.n:, :].reshape(Bn, -1).copy()
        yp = d["y_d"][:, -spec.n:, :].reshape(Bn, -1).copy()
        _LOOP.update(case=dict(spec=spec, plant=pl, B=Bn, u_d=d["u_d"], y_d=d["y_d"], x0=d["x_end"].copy(), up=up, yp=yp, w=w),
                     u_ref=u_ref, y_ref=y_ref)
    return _LOOP["case"], _LOOP["u_ref"], _LOOP["y_ref"]


def _ref_loop(case, b, u_ref, y_ref, nms, bounds):
    pl = case["plant"]
    plant = orc.Plant(pl["A"], pl["B"], pl["C"], pl["D"], pl["eps_max"])
    plant.x = case["x0"][b].copy()
    u, y, up, yp, sols = ref.schedule_loop(case["spec"], case["u_d"][b], case["y_d"][b], plant, case["w"][b], u_ref, y_ref,
                                           n_mpc_step=nms, u_past=case["up"][b], y_past=case["yp"][b], **bounds)
    return u, y, plant.x, up, yp, sols


def _check_loop(tag, out, refs, rows, refined_ok=False):
    u_sys, y_sys, status, x_end, up_end, yp_end = out
    assert np.all(status <= (1 if refined_ok else 0)), (tag, status)
    for b in rows:
        u_r, y_r, x_r, up_r, yp_r = refs[b][:5]
        ysc = max(1.0, np.max(np.abs(y_r)))
        usc = np.max(np.abs(u_r))
        eu, ey, ex = np.max(np.abs(u_sys[b] - u_r)) / usc, np.max(np.abs(y_sys[b] - y_r)) / ysc, np.max(np.abs(x_end[b] - x_r)) / ysc
        ew = max(np.max(np.abs(up_end[b] - up_r)) / usc, np.max(np.abs(yp_end[b] - yp_r)) / ysc)
        print("%s instance %d: u %.2e  y %.2e  x_end %.2e  windows %.2e" % (tag, b, eu, ey, ex, ew))
        assert eu < TOL_U and ey < TOL_Y and ex < TOL_Y, (tag, b, eu, ey, ex)
        assert np.max(np.abs(up_end[b] - up_r)) / usc < TOL_U and np.max(np.abs(yp_end[b] - yp_r)) / ysc < TOL_Y, (tag, b, ew)


@pytest.mark.parametrize("nms", [1, 4])
@pytest.mark.parametrize("box", ["tight", "wide"])
def test_fused_loop_with_a_setpoint_switch(gpu, box, nms):
    case, u_ref, y_ref = _tank_loop()
    spec, pl, Bn = case["spec"], case["plant"], case["B"]
    lo, hi, _ = ref.STEP_BOXES[box]
    bounds = dict(u_min=lo, u_max=hi)
    n_steps = u_ref.shape[1]
    args = (pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"])
    with T._engine(spec, 400, Bn) as eng:
        eng.set_setpoint_box_law(True)
        eng.set_input_bounds(lo, hi)
        eng.set_data(case["u_d"], case["y_d"])
        out = eng.closed_loop_setpoints(*args, u_ref, y_ref, n_mpc_step=nms)
        assert eng.closed_loop_kernel_name() == STEP_KERNEL_LOOP
        # a constant schedule at the handle's own setpoints is the fused bounded closed loop
        const = eng.closed_loop_setpoints(*args, np.tile(spec.u_s, (Bn, n_steps, 1)), np.tile(spec.y_s, (Bn, n_steps, 1)), n_mpc_step=nms)
        fused = eng.closed_loop(*args, n_mpc_step=nms)
        assert eng.closed_loop_kernel_name() == "ddmpc_closed_loop_box_kernel"
        # one instance's schedule goes NaN at step 10: the first solve at or after it reads a NaN row (step 10, or 12 with
        # n_mpc_step = 4)
        u_nan = u_ref.copy()
        u_nan[1, 10:] = np.nan
        stop = eng.closed_loop_setpoints(*args, u_nan, y_ref, n_mpc_step=nms)
    rows = (0, Bn - 1)
    refs = {b: _ref_loop(case, b, u_ref[b], y_ref[b], nms, bounds) for b in rows}
    _check_loop("%s nstep %d" % (box, nms), out, refs, rows)
    for b in rows:
        assert all(s.margin >= 1e-7 for s in refs[b][5]), b
    if box == "tight":                                  # the switch shows in the active count of instance 3
        ks = [int(np.count_nonzero(s.active)) for s in refs[Bn - 1][5]]
        t_sw = 10 // nms if nms == 1 else 3             # the first solve that sees the second setpoint
        print("instance 3 active counts", ks)
        assert ks[t_sw] != ks[t_sw - 1], ks
    assert np.array_equal(const[2], fused[2]) and np.all(fused[2] == 0)
    for k, (a, b) in enumerate(zip(const, fused)):
        if k != 2:
            print("constant schedule vs fused bounded closed_loop, output %d: %.2e" % (k, _rel(a, b)))
            assert _rel(a, b) < TOL_LAW, (k, _rel(a, b))
    assert not np.allclose(out[0][:, 12:], const[0][:, 12:])
    # the stopped instance: NaN rows from the first solve on a NaN row on, status 4; the others bit-equal
    t_stop = 10 if nms == 1 else 12
    keep = np.arange(Bn) != 1
    assert stop[2][1] == 4 and np.all(stop[2][keep] == 0)
    assert np.all(np.isnan(stop[0][1, t_stop:])) and np.all(np.isnan(stop[1][1, t_stop:]))
    assert np.array_equal(stop[0][1, :t_stop], out[0][1, :t_stop]) and np.array_equal(stop[1][1, :t_stop], out[1][1, :t_stop])
    for a, b in zip(stop, out):
        assert np.array_equal(a[keep], b[keep])


# ----------------------------------------------------------------------------------------------------------- 8. safeguard
def test_safeguard_finishes_the_cycling_instances(gpu):
    # a box of width 0.2 around u_s = (1, 1), on which the primal-dual rule cycles; per-instance setpoints inside it
    spec = ref.spec()
    t = ref.tank()
    lo, hi = [0.9, 0.9], [1.1, 1.1]
    bounds = dict(u_min=lo, u_max=hi)
    cap = 50
    rng = np.random.default_rng(8)
    us = spec.u_s + rng.uniform(-0.08, 0.08, (B8, spec.m))
    ys = spec.y_s + rng.uniform(-0.05, 0.05, (B8, spec.p))
    res = {}
    for safe in (False, True):
        with _engine(spec, bounds, max_iter=cap) as eng:
            eng.set_box_safeguard(safe)
            res[safe] = [x.copy() for x in eng.step_setpoints(t["up"], t["yp"], us, ys)]
    u0, c0, s0, i0 = res[False]
    u1, c1, s1, i1 = res[True]
    # which instances cycle is the model's finding (the rule of BoxTab::test, from the empty set, cap 50)
    cyc = np.array([model.model_step(spec, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], us[b], ys[b], max_iter=cap, **bounds)[2] == 4
                    for b in range(B8)])
    print("cycling", np.nonzero(cyc)[0].tolist(), "status", s0.tolist(), s1.tolist(), "iters", i0.tolist(), i1.tolist())
    assert np.any(cyc)
    assert np.all(s0[cyc] == 4) and np.all(i0[cyc] == cap) and np.all(s0[~cyc] == 0)
    assert np.all(s1 == 0) and np.all(i1[cyc] > cap) and np.array_equal(i1[~cyc], i0[~cyc])
    assert np.array_equal(u1[~cyc], u0[~cyc]) and np.array_equal(c1[~cyc], c0[~cyc])
    for b in range(B8):
        sps = sref.with_setpoints(spec, us[b], ys[b])
        # the reference: the CPU safeguarded solve where the rule cycles, the primal-dual helper elsewhere
        sol = (sg.solve_safeguarded(sps, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], lo, hi) if cyc[b] else
               ref.solve(spec, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], us[b], ys[b], **bounds))
        eu = np.max(np.abs(u1[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(c1[b] - sol.cost) / abs(sol.cost)
        print("safeguard b=%d cycling %s iters %d err_u %.1e err_cost %.1e" % (b, bool(cyc[b]), i1[b], eu, ec))
        assert sol.status == "optimal" and eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        # the certificate on x completed from the GPU's inputs: the full-space problem with ubar fixed to them
        qp = orc.build_fullspace_qp(sps, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b])
        u_idx = np.arange(qp.sl["ubar"].start + spec.n * spec.m, qp.sl["ubar"].stop)
        E = np.zeros((u_idx.size, qp.P.shape[0]))
        E[np.arange(u_idx.size), u_idx] = 1.0
        x, _ = orc._kkt_solve(qp.P, qp.q, np.vstack([qp.A, E]), np.concatenate([qp.b, u1[b]]))
        x[u_idx] = u1[b]                                # (the GPU's inputs themselves, not the completion's 1e-11 copy of them)
        cert = ref.kkt_certificate(spec, t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], us[b], ys[b], x, **bounds)
        tol = 1e-8 * cert["grad_scale"]
        assert cert["res_stat"] < tol and cert["dual_sign"] < tol, (b, cert)
        assert cert["res_box"] <= 1e-12 * 1.1, (b, cert)


# -------------------------------------------------------------------------------------------------------- 9. second shape
def test_one_bounded_channel_on_a_plant_with_five_channels(gpu):
    # "m>p-ns>n": 60 rows, m = 3, p = 2; channel 0 in [u_s[0] - 0.35, u_s[0] + 0.35], setpoints u_s +- 0.3 (inside: the terminal
    # constraint).  On the CPU: every reference solve optimal, active sets of 0 .. 5, margins >= 1e-3.
    case, nms = plants._table_case("m>p-ns>n")
    s, Bn = case["spec"], case["B"]
    n_steps = case["w"].shape[1]
    rng = np.random.default_rng(5)
    u_ref = np.stack([s.u_s[None] + rng.uniform(-0.3, 0.3, (n_steps, s.m)) for _ in range(Bn)])
    y_ref = np.stack([s.y_s[None] + rng.uniform(-0.3, 0.3, (n_steps, s.p)) for _ in range(Bn)])
    lo, hi = [s.u_s[0] - 0.35, -INF, -INF], [s.u_s[0] + 0.35, INF, INF]
    bounds = dict(u_min=lo, u_max=hi)
    pl = case["plant"]
    with plants.engine(case) as eng:
        eng.set_setpoint_box_law(True)
        eng.set_input_bounds(lo, hi)
        eng.set_data(case["u_d"], case["y_d"])
        u, cost, status, iters = eng.step_setpoints(case["up"], case["yp"], u_ref[:, 0], y_ref[:, 0])
        out = eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], case["x0"], case["up"], case["yp"], case["w"], u_ref,
                                        y_ref, n_mpc_step=nms)
        assert eng.closed_loop_kernel_name() == STEP_KERNEL_LOOP
    active = 0
    for b in range(Bn):
        sol = ref.solve(s, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], u_ref[b, 0], y_ref[b, 0], **bounds)
        assert sol.margin >= 1e-7
        assert not _check_step("m>p-ns>n", s, b, sol, u[b], cost[b], status[b], iters[b], refined_ok=True, **bounds)
        active += int(np.count_nonzero(sol.active))
    assert active >= 1
    refs = [_ref_loop(case, b, u_ref[b], y_ref[b], nms, bounds) for b in range(Bn)]
    assert all(x.margin >= 1e-7 for r in refs for x in r[5])
    print("m>p-ns>n statuses: step", status.tolist(), "loop", out[2].tolist())
    _check_loop("m>p-ns>n", out, refs, range(Bn), refined_ok=True)      # (under the default refinement instance 0's law is refined)


# ----------------------------------------------------------------------------------------------- 10. allocator independence
def test_results_do_not_depend_on_what_the_allocator_hands_back(gpu):
    spec = ref.spec()
    t = ref.tank()
    lib = L.load()
    res = []
    for fill in (0, 255, 63):
        lib.ddmpc_debug_poison_allocations(fill)
        try:
            with _engine(spec, dict(u_min=[0.0, 0.0], u_max=[2.0, 2.0])) as eng:
                eng.prepare()
                res.append([x.copy() for x in eng.step_setpoints(t["up"], t["yp"], t["us"], t["ys"])] + [eng.setpoint_gain()])
        finally:
            lib.ddmpc_debug_poison_allocations(0)
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)
    assert np.all(res[0][2] == 0)


# ------------------------------------------------------------------------------------------------------ 11. example script
def test_example_script_tracks_per_instance_setpoints_inside_the_box(gpu, tmp_path):
    t_sim, Bn, spread = 40, 8, 0.05
    out = tmp_path / "loop.npz"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "batched_data_driven_mpc_example.py"), "--setpoint_spread",
                          str(spread), "--u_min", "0", "--u_max", "2", "--batch", str(Bn), "--t_sim", str(t_sim), "--seed", "0",
                          "--out", str(out)], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert STEP_KERNEL_LOOP in res.stdout
    z = np.load(out)
    spec = orc.spec_from_params()
    pl = orc.FOUR_TANK
    A, Bm, Cm, D = (np.asarray(pl[k], float) for k in ("A", "B", "C", "D"))
    us = spec.u_s + spread * np.random.default_rng(0).uniform(-1.0, 1.0, (Bn, spec.m))
    ys = us @ (Cm @ np.linalg.inv(np.eye(A.shape[0]) - A) @ Bm + D).T
    assert z["u_sys"].shape == (Bn, t_sim + 1, spec.m) and np.all(z["status"] == 0)
    assert np.array_equal(z["u_s"], us) and np.array_equal(z["y_s"], ys)
    assert np.min(z["u_sys"]) >= 0.0 and np.max(z["u_sys"]) <= 2.0
    for b in range(Bn):
        inst = orc.generate_instance(b)
        w = inst["plant"].eps_max * inst["rng"].uniform(-1.0, 1.0, (t_sim + 1, spec.p))
        u_r, y_r, _, _, _ = ref.schedule_loop(spec, inst["u_d"], inst["y_d"], inst["plant"], w, np.tile(us[b], (t_sim + 1, 1)),
                                              np.tile(ys[b], (t_sim + 1, 1)), u_min=[0.0, 0.0], u_max=[2.0, 2.0], n_mpc_step=spec.n)
        eu = np.max(np.abs(z["u_sys"][b] - u_r)) / np.max(np.abs(u_r))
        ey = np.max(np.abs(z["y_sys"][b] - y_r)) / max(1.0, np.max(np.abs(y_r)))
        print("example instance %d: u %.2e  y %.2e" % (b, eu, ey))
        assert eu < TOL_U and ey < TOL_Y, (b, eu, ey)
