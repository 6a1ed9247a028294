"""DDMPC_OPT_LARGE_BOX_LAW: bounds beyond 271 rows, ddmpc_step and the per-step ddmpc_closed_loop serve the instances whose law
of the empty active set violates no component of the box table from that law in one launch (rr3_law_box_step_kernel,
ddmpc_rr3_box_law.hpp, DESIGN 5.5.2 "Law inside the box") and re-solve only the others, by the launches of the option 0
restricted to them (the instance filter of rr3_solve_box_kernel, rr3_solve_box_wide_kernel and rr3_box_safeguard_kernel).

Bars: a law-served instance against the solve on the same handle (or the same step with the option 0) 1e-9 relative -- REL of
tests/test_gpu_large_robust_law.py, the project's bar for law against solve --; a re-solved instance bit-equal to the option 0;
against the full-space helper inputs 1e-8 and cost 1e-9, the bars of tests/test_gpu_large_bounds.py.  The fixture, its window
families and the helper's margins (>= 1e-7 on every instance used, none left out) are pinned on the CPU by
tests/test_large_box_law_reference.py, whose cached helper solutions these tests share."""
import ctypes as C

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _input_bounds_ref as uref
import test_large_box_law_reference as T
from test_gpu_large_bounds import TOL_COST, TOL_U, U_CH0, _bounded_engine, _code
from test_gpu_large_box_safeguard import CASES as SAFE_CASES, MAX_ITER as SAFE_MAX_ITER
from test_gpu_large_robust_law import REL, SOL, _cfg5_robust, _rel, _served, _windows
from test_gpu_round5 import _spec_engine

pytestmark = pytest.mark.gpu

B8, N = T.B8, T.N
CAPS = {"u_wide": None, "y_up": None, "u_cap": 128}        # [0, 2] on the tail has more than 64 components active: capacity 128


def _out(res):
    return tuple(np.array(x, copy=True) for x in res)


def _sols(eng):
    return {w: eng.get_solution(w) for w in SOL}


def _engine(slack, box, law, B=B8, rows=None, cap=None, warm=False, safe=False, refine=None, boxes=None, **kw):
    """A bounded 296-row handle of the fixture with its data and box set, the law option as asked."""
    spec, d, _, _ = T.fixture(slack)
    rows = slice(0, B) if rows is None else rows
    eng = _bounded_engine(spec, N, B, **kw)
    if refine is not None:
        eng.set_refinement(refine)
    if cap is not None:
        eng.set_large_box_capacity(cap)
    if safe:
        eng.set_large_box_safeguard(True)
    if warm:
        eng.set_large_box_warm_start(True)
    if law is not None:
        eng.set_large_box_law(law)
    eng.set_data(d["u_d"][rows], d["y_d"][rows])
    ubox, ybox = boxes if boxes is not None else T.BOXES[box]
    if ubox is not None:
        eng.set_input_bounds(*ubox)
    if ybox is not None:
        eng.set_output_bounds(*ybox)
    return eng


def _mixed(slack):
    """Even instances on the data tail, odd ones near the setpoint."""
    up, yp = (x.copy() for x in T.windows(slack, "setpoint"))
    tu, ty = T.windows(slack, "tail")
    up[::2], yp[::2] = tu[::2], ty[::2]
    return up, yp


def _record(eng, b, cap):
    """[k, state, iterations, k] and the peak k of instance b from the record of the last step (ddmpc_debug_workspace)."""
    rv = (eng.m + eng.p) * (eng.L + eng.n) + 1 & ~1
    nm = 4 + (cap or 64) + rv + 4
    meta = np.full(nm, -1, np.int32)
    L.check(L.load().ddmpc_debug_workspace(eng._h, b, C.c_void_p(), 0, C.c_void_p(meta.ctypes.data), nm, C.c_void_p(), C.c_void_p()))
    return meta[:4].tolist(), meta[4 + (cap or 64):4 + (cap or 64) + rv].copy(), int(meta[nm - 2])


def _close(t, ts, s, ss, rows, tag):
    """Rows of (outputs, solutions) t against s at the law-against-solve bar, every figure printed first."""
    eu = _rel(t[0][rows], s[0][rows])
    ec = float(np.max(np.abs(t[1][rows] - s[1][rows]) / np.abs(s[1][rows])))
    es = {w: _rel(ts[w][rows], ss[w][rows]) for w in SOL}
    print("%s: u %.1e cost %.1e" % (tag, eu, ec), " ".join("%s %.1e" % kv for kv in es.items()))
    assert np.array_equal(t[2][rows], s[2][rows]) and np.array_equal(t[3][rows], s[3][rows]), (tag, t[2], s[2], t[3], s[3])
    assert eu <= REL and ec <= REL, (tag, eu, ec)
    for w in SOL:
        assert es[w] <= REL, (tag, w, es[w])


def _bit_equal(t, ts, s, ss, rows, tag):
    for a, b_ in zip(t, s):
        assert np.array_equal(a[rows], b_[rows], equal_nan=True), tag
    for w in SOL:
        assert np.array_equal(ts[w][rows], ss[w][rows], equal_nan=True), (tag, w)


def _step(eng, up, yp):
    return _out(eng.step(up, yp)), _sols(eng)


def _three_steps(slack, box, cap=None, refine=None):
    """Mixed batch, then every instance at the setpoint, then every instance on the tail, on a handle with the option 0 and on
    one with 1: per step ((outputs, solutions) of 0, (outputs, solutions) of 1)."""
    wins = [_mixed(slack), T.windows(slack, "setpoint"), T.windows(slack, "tail")]
    res = {}
    for law in (False, True):
        with _engine(slack, box, law, cap=cap, refine=refine) as eng:
            eng.prepare()
            res[law] = [_step(eng, up, yp) for up, yp in wins]
    return list(zip(res[False], res[True]))


def _check_three_steps(steps, tag):
    even, odd, every = np.arange(0, B8, 2), np.arange(1, B8, 2), np.arange(B8)
    (s, ss), (t, ts) = steps[0]                                                   # mixed
    print(tag, "mixed: status", t[2], "iters", t[3])
    assert np.all(t[2] == 0) and np.all(t[3][odd] == 1) and np.all(t[3][even] >= 2)
    _close(t, ts, s, ss, odd, tag + " mixed, odd (law)")
    _bit_equal(t, ts, s, ss, even, tag + " mixed, even (re-solved)")
    assert np.all(np.any(t[0][odd] != s[0][odd], axis=1))                         # the law served them, not the re-solve
    (s, ss), (t, ts) = steps[1]                                                   # every instance at the setpoint
    assert np.all(t[2] == 0) and np.all(t[3] == 1)
    _close(t, ts, s, ss, every, tag + " setpoint")
    (s, ss), (t, ts) = steps[2]                                                   # every instance on the tail: nothing of the
    assert np.all(t[3] >= 2)                                                      # earlier steps leaks into the re-solve
    _bit_equal(t, ts, s, ss, every, tag + " tail")


# ------------------------------------------------------------------------------------------------ 1. contract
def test_contract_of_the_option(gpu):
    spec, d, up, yp = T.fixture("convex")
    sup, syp = T.windows("convex", "setpoint")
    nf, r = spec.n * (spec.m + spec.p), (spec.m + spec.p) * spec.Ln
    assert L.OPT_LARGE_BOX_LAW == 17 and r == 296
    with _engine("convex", "u_wide", None) as eng:
        for bad in (2, -1):
            code, msg = _code(lambda v: L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_LARGE_BOX_LAW, v)), bad)
            assert code == L.ERR_INVALID and "DDMPC_OPT_LARGE_BOX_LAW" in msg, (bad, msg)
        eng.set_large_box_law(True)
        code, msg = _code(eng.gain)                                               # no law before ddmpc_prepare
        assert code == L.ERR_NOT_READY
        code, msg = _code(eng.set_large_affine_law, True)                         # the unbounded option stays refused with bounds
        assert code == L.ERR_UNSUPPORTED and "LARGE_AFFINE_LAW" in msg
        eng.prepare()
        g = eng.gain()
        assert g.shape == (B8, nf + 1, r)
        t = _out(eng.step(sup, syp))
        assert np.all(t[2] == 0) and np.all(t[3] == 1)
        al, ub = eng.get_solution("alpha"), eng.get_solution("ubar")
        w = np.concatenate([sup, syp], axis=1)
        lam, rd = spec.lamb_alpha * spec.eps_max, np.diag(spec.R)
        nfree = spec.L - spec.n if spec.tec else spec.L
        for b in range(B8):
            H = orc.hankel_matrix(np.concatenate([d["u_d"][b], d["y_d"][b]], axis=1), spec.Ln)
            beta = g[b, 0] + g[b, 1:].T @ w[b]                                   # row 0 plus the window rows, component order
            assert _rel(H.T @ beta, al[b]) <= REL, b
            bu = beta.reshape(spec.Ln, spec.m + spec.p)[spec.n:spec.n + nfree, :spec.m]
            ubar = np.asarray(spec.u_s, float).reshape(-1)[None, :] - lam * bu / rd[:nfree * spec.m].reshape(nfree, spec.m)
            assert _rel(ubar, ub[b].reshape(spec.Ln, spec.m)[spec.n:spec.n + nfree]) <= REL, b
        eng.set_large_box_law(False)                                              # either value forgets the preparation and the solution
        code, msg = _code(eng.get_solution, "ubar")
        assert code == L.ERR_NOT_READY
        code, msg = _code(eng.gain)
        assert code == L.ERR_UNSUPPORTED
    # accepted without effect: no bounds at 296 rows, and a bounded handle of 136 rows
    res = []
    for call in (False, True):
        with _spec_engine(spec, N, B8) as eng:
            if call:
                eng.set_large_box_law(True)
            eng.set_data(d["u_d"], d["y_d"])
            eng.prepare()
            res.append(_out(eng.step(up, yp)))
            code, msg = _code(eng.gain)
            assert code == L.ERR_UNSUPPORTED
    assert all(np.array_equal(a, b_) for a, b_ in zip(*res))
    spec_s = orc.spec_from_params(slack_var_constraint_type=1)
    assert (spec_s.m + spec_s.p) * spec_s.Ln == 136
    ds = harness.generate_batch(range(4))
    ups = ds["u_d"][:, -spec_s.n:, :].reshape(4, -1).copy(); yps = ds["y_d"][:, -spec_s.n:, :].reshape(4, -1).copy()
    res = []
    for call in (False, True):
        with _spec_engine(spec_s, ds["u_d"].shape[1], 4) as eng:
            if call:
                eng.set_large_box_law(True)
            eng.set_data(ds["u_d"], ds["y_d"])
            eng.set_input_bounds(*T.U_CAP)
            eng.prepare()
            res.append(_out(eng.step(ups, yps)))
    assert all(np.array_equal(a, b_, equal_nan=True) for a, b_ in zip(*res)) and np.any(res[0][3] >= 2)


# ------------------------------------------------------------------------------------------------ 2. inside the box
@pytest.mark.parametrize("slack", T.SLACKS)
@pytest.mark.parametrize("box", list(T.BOXES))
def test_inside_the_box_the_law_serves_the_step(gpu, box, slack):
    spec, d, _, _ = T.fixture(slack)
    up, yp = T.windows(slack, "setpoint")
    cap = CAPS[box]
    with _engine(slack, box, True, cap=cap) as eng:
        eng.prepare()
        s, ss = _out(eng.solve(up, yp)), _sols(eng)
        t, ts = _step(eng, up, yp)
        recs = [_record(eng, b, cap) for b in range(B8)]
    assert np.all(t[2] == 0) and np.all(t[3] == 1)
    _close(t, ts, s, ss, np.arange(B8), "%s %s step against solve" % (box, slack))
    assert _served(s, t) >= 0.9
    for b, (head, act, peak) in enumerate(recs):                                  # what a bounded kernel leaves at the first test
        assert head == [0, 0, 1, 0] and not np.any(act) and peak == 0, (b, head, peak)
    for b in range(B8):
        sol = T.reference(slack, box, "setpoint", b)
        eu = np.max(np.abs(t[0][b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(t[1][b] - sol.cost) / abs(sol.cost)
        print("%s %s b=%d helper iters %d margin %.1e err_u %.1e err_cost %.1e" % (box, slack, b, sol.iters, sol.margin, eu, ec))
        assert sol.status == "optimal" and sol.margin >= 1e-7 and sol.iters == 1
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)


# ------------------------------------------------------------------------------------------------ 3. mixed batch
@pytest.mark.parametrize("slack", T.SLACKS)
@pytest.mark.parametrize("box", list(T.BOXES))
def test_mixed_batch_law_and_filtered_resolve(gpu, box, slack):
    """[-4, 6] and the output box at the default capacity (rr3_solve_box_kernel, both instantiations), [0, 2] at capacity 128 (the
    wide kernel)."""
    _check_three_steps(_three_steps(slack, box, cap=CAPS[box]), "%s %s" % (box, slack))


# ------------------------------------------------------------------------------------------------ 4. refinement
@pytest.mark.parametrize("mode", ["off", "auto", "always"])
def test_refinement_modes(gpu, mode):
    _check_three_steps(_three_steps("convex", "u_wide", refine=mode), "u_wide convex refine=%s" % mode)


# ------------------------------------------------------------------------------------------------ 5. with the warm start
def test_with_the_warm_start(gpu):
    slack, box, cap = "convex", "u_cap", 128
    tail, setp = T.windows(slack, "tail"), T.windows(slack, "setpoint")
    res = {}
    for law in (False, True):
        with _engine(slack, box, law, cap=cap, warm=True) as eng:
            eng.prepare()
            res[law] = [_step(eng, *w) for w in (tail, setp, tail)]
    every = np.arange(B8)
    for i in (0, 2):                                                              # on the tail: the seeded launches, filtered
        (s, ss), (t, ts) = res[False][i], res[True][i]
        print("warm start, step %d: status" % (i + 1), t[2], "iters", t[3])
        assert np.all(t[2] == 0) and np.all(t[3] >= 2)
        _bit_equal(t, ts, s, ss, every, "step %d" % (i + 1))
    (s, ss), (t, ts) = res[False][1], res[True][1]
    assert np.all(s[3] == 1) and np.all(t[3] == 1) and np.all(t[2] == 0)
    _close(t, ts, s, ss, every, "warm start, step 2")
    for law in (False, True):                                                     # the step inside the box left an empty seed:
        _bit_equal(*res[law][2], *res[law][0], every, "step 3 = an unseeded step")  # step 3 is step 1, which had none


# ------------------------------------------------------------------------------------------------ 6. with the safeguard
def test_with_the_safeguard(gpu):
    """The cycling case of tests/test_gpu_large_box_safeguard.py (u in [0.9, 1.1], slack NONE, max_iter 50, capacity 192) on the
    tail: instance 3 reaches the cap and is finished by rr3_box_safeguard_kernel, filtered."""
    c = SAFE_CASES["B"]
    up, yp = T.windows(c["slack"], "tail")
    res = {}
    for law in (False, True):
        with _engine(c["slack"], None, law, cap=192, safe=True, boxes=(c["box"]["u"], c["box"]["y"]), max_iter=SAFE_MAX_ITER) as eng:
            eng.prepare()
            res[law] = _step(eng, up, yp)
    (s, ss), (t, ts) = res[False], res[True]
    print("safeguard: status", t[2], "iters", t[3])
    assert np.all(t[2] == 0) and t[3][3] == SAFE_MAX_ITER + 124
    _bit_equal(t, ts, s, ss, np.arange(B8), "safeguard")


# ------------------------------------------------------------------------------------------------ 7. invalidation
def test_invalidation(gpu):
    slack = "convex"
    spec, d, _, _ = T.fixture(slack)
    d2 = harness.generate_batch(range(100, 100 + B8), N=N)
    up, yp = _mixed(slack)
    every, odd = np.arange(B8), np.arange(1, B8, 2)

    def pair(eng, tag):
        """A step against a solve at the same windows; some instances are served by the law, some re-solved."""
        t, ts = _step(eng, up, yp)
        s, ss = _out(eng.solve(up, yp)), _sols(eng)
        print(tag, "status", t[2], "iters", t[3])
        _close(t, ts, s, ss, every, tag)
        assert np.all(t[3][odd] == 1) and np.any(t[3] >= 2), tag
        assert np.all(np.any(t[0][odd] != s[0][odd], axis=1)), tag              # the law served them: a law formed anew
        return t

    with _engine(slack, "u_wide", True) as eng:
        t0 = pair(eng, "first")
        eng.set_data(d2["u_d"], d2["y_d"])
        t1 = pair(eng, "set_data")
        assert not np.allclose(t1[0], t0[0])
        eng.set_setpoints(np.asarray(spec.u_s) * 1.5, np.asarray(spec.y_s) * 1.5)
        up[1::2] = (up[1::2] - np.tile(spec.u_s, spec.n)) + 1.5 * np.tile(spec.u_s, spec.n)   # the odd windows follow the setpoint
        yp[1::2] = (yp[1::2] - np.tile(spec.y_s, spec.n)) + 1.5 * np.tile(spec.y_s, spec.n)
        t2 = pair(eng, "set_setpoints")
        assert not np.allclose(t2[0], t1[0])
        eng.set_input_bounds(*U_CH0)
        t3 = pair(eng, "set_input_bounds")
        assert not np.allclose(t3[0], t2[0])
        eng.set_refinement("off")
        t4 = pair(eng, "set_refinement")
        assert not np.array_equal(t4[0], t3[0])
        eng.set_large_box_law(False)                                              # the option 0: the step is the solve again, bit for bit
        t, ts = _step(eng, up, yp)
        s, ss = _out(eng.solve(up, yp)), _sols(eng)
        _bit_equal(t, ts, s, ss, every, "option 0")


# ------------------------------------------------------------------------------------------------ 8. per-step closed loop
@pytest.mark.parametrize("n_mpc_step", [1, 2])
def test_per_step_closed_loop_against_the_reference_loop(gpu, n_mpc_step):
    """Inputs in [-4, 6], slack NONE, 20 steps from the data tail, instances 0 and 1, noise seed 5: the first solves are
    re-solves, the later ones are served by the law."""
    slack, Bq, n_steps = "none", 2, 20
    spec, d, up, yp = T.fixture(slack)
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (Bq, n_steps, 2))
    with _engine(slack, "u_wide", True, B=Bq) as eng:
        u_sys, y_sys, st, _, _, _ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up[:Bq], yp[:Bq], w,
                                                    n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        recs = [_record(eng, b, None) for b in range(Bq)]
    assert np.all(st == 0)
    assert np.min(u_sys) >= -4.0 and np.max(u_sys) <= 6.0
    for b, (head, act, peak) in enumerate(recs):                                  # the record of the loop's last solve: the law
        assert head == [0, 0, 1, 0] and not np.any(act) and peak == 0, (b, head, peak)
    for b in range(Bq):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        ur, yr = uref.closed_loop_bounded(spec, d["u_d"][b], d["y_d"][b], plant, w[b], T.U_WIDE[0], T.U_WIDE[1], n_mpc_step=n_mpc_step)
        eu, ey = np.max(np.abs(u_sys[b] - ur)) / np.max(np.abs(ur)), np.max(np.abs(y_sys[b] - yr)) / np.max(np.abs(yr))
        print("loop n_mpc_step=%d b=%d err_u %.1e err_y %.1e" % (n_mpc_step, b, eu, ey))
        assert eu < 1e-8 and ey < 1e-8, (b, eu, ey)


# ------------------------------------------------------------------------------------------------ 9. the cfg-5 size
REL_OFF, REL_OFF_ALPHA = 1e-7, 1e-6                       # law against solve on the unrefined factor at 608 rows: the bars of
                                                          # test_cfg5_size_refinement_off_law_serves (tests/test_gpu_large_robust_law.py)


@pytest.mark.parametrize("refine", ["auto", "off"])
def test_mixed_batch_at_the_cfg5_size(gpu, refine):
    """m = p = 8, n = 8, L = 30: 608 rows, CONVEX, n(m+p) + 1 = 129 right-hand sides of the law (three 64-column blocks), inputs
    in [-10, 10] at capacity 256.  By the numpy restatement (tests/test_large_box_law_reference.law_of) the law's inputs of the
    setpoint windows stay within [-1.49, 1.23] and their slacks within 0.17 of the slack box on all 16 instances; every tail
    window leaves the slack box (by a factor of 4.7 and more).  By the restatement of tests/test_large_bounds_reference.py the
    tail instances 0, 2, 4, 6 and 12 end after 2 - 5 solves (8 - 16 active) and 8, 10, 14 cycle to the max_iter cap (status 4, up
    to 241 active: within the capacity) -- of those the outputs, status and iters are compared, not the workspace nobody wrote.
    AUTO: no law of this size reaches the refinement threshold, every instance is "no law" and re-solved -- the
    assertions of the mixed batch hold with every instance bit-equal to the option 0.  OFF: the law serves the odd instances, at
    the bars of law against solve on the unrefined factor."""
    B = 16
    spec, N5, d, up, yp = _cfg5_robust(B, "convex")
    assert (spec.m + spec.p) * spec.Ln == 608 and spec.n * (spec.m + spec.p) + 1 == 129
    mu, my = (x.copy() for x in _windows(d, up, yp, spec, "setpoint"))
    mu[::2], my[::2] = up[::2], yp[::2]
    even, odd = np.arange(0, B, 2), np.arange(1, B, 2)
    res = {}
    for law in (False, True):
        with _bounded_engine(spec, N5, B) as eng:
            eng.set_refinement(refine)
            eng.set_large_box_capacity(256)
            eng.set_large_box_law(law)
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_input_bounds([-10.0] * spec.m, [10.0] * spec.m)
            eng.prepare()
            res[law] = _step(eng, mu, my)
    (s, ss), (t, ts) = res[False], res[True]
    print("cfg5 refine=%s: status" % refine, t[2], "iters", t[3])
    assert np.all(t[2][odd] == 0) and np.all(t[3][odd] == 1) and np.all(t[3][even] >= 2)
    for a, b_ in zip(t, s):
        assert np.array_equal(a[even], b_[even], equal_nan=True)
    done = even[t[2][even] == 0]
    assert done.size >= 4
    _bit_equal(t, ts, s, ss, done, "cfg5 even (re-solved)")
    served = float(np.mean(np.any(t[0][odd] != s[0][odd], axis=1)))
    if refine == "auto":
        _close(t, ts, s, ss, odd, "cfg5 auto, odd")
        assert served == 0.0                                                      # "no law": the filtered re-solve, bit for bit
    else:
        eu = _rel(t[0][odd], s[0][odd])
        ec = float(np.max(np.abs(t[1][odd] - s[1][odd]) / np.abs(s[1][odd])))
        es = {w: _rel(ts[w][odd], ss[w][odd]) for w in SOL}
        print("cfg5 off, odd (law): served %.2f u %.1e cost %.1e" % (served, eu, ec), " ".join("%s %.1e" % kv for kv in es.items()))
        assert served >= 0.9
        assert np.array_equal(t[2][odd], s[2][odd]) and np.array_equal(t[3][odd], s[3][odd])
        assert eu <= REL_OFF and ec <= REL_OFF
        for w in SOL:
            assert es[w] <= (REL_OFF_ALPHA if w == "alpha" else REL_OFF), (w, es[w])
