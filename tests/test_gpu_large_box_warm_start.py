"""DDMPC_OPT_LARGE_BOX_WARM_START: bounds beyond 271 rows, ddmpc_step and the per-step ddmpc_closed_loop start the primal-dual
iteration from the signed set the last solve ended with (the seeded instantiation of rr3_solve_box_wide_kernel and
rr3_box_keep_seed_kernel, ddmpc_rr3_box_wide.hpp, DESIGN 5.5.2 "Warm start").

Against the seeded reduced-space helper tests/_large_box_warm_ref.py (pinned on the CPU by
tests/test_large_box_warm_reference.py, whose fixture and closed loops these tests share) at the bars of
tests/test_gpu_large_box_capacity.py: inputs 1e-8, cost 1e-9 relative, status identical; solve counts and signed sets are
compared where the helper's margin is >= 1e-7, and at most 2 of 8 instances may be left out of that comparison -- by the
helper none is (the smallest margin of a seeded run is 1.1e-6, case D instance 1), which is asserted.  The windows come from
the helper's closed loop and are fed to ddmpc_step, so the rounding of the GPU never feeds back into them.

Fixture: four-tank, L = 70, N = 700, 296 rows, instances 0 .. 7 from the data tail, max_iter 50, DDMPC_OPT_LARGE_BOUNDS = 1.
"""
import ctypes as C

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _large_box_safeguard_ref as sref
import test_large_box_warm_reference as T
from test_gpu_large_bounds import _bounded_engine, _code, _full_x, _sections, _signed_active

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
LH, N, MAX_ITER = T.LH, T.N, T.MAX_ITER
_EMPTY = {}


def _windows(case, rows, n_win=4, loops=None):
    """The helper-driven windows of the instances `rows`: per window (u_past [len(rows), n m], y_past [len(rows), n p])."""
    loops = loops or {b: T.loop(case, b, n_win) for b in rows}
    assert all(len(loops[b]) == n_win for b in rows)
    return loops, [(np.stack([loops[b][w].window[0] for b in rows]), np.stack([loops[b][w].window[1] for b in rows]))
                   for w in range(n_win)]


def _empty(case, b, sol):
    """The empty start of the helper on the window of `sol`, computed once."""
    key = (case, b, sol.window[0].tobytes(), sol.window[1].tobytes())
    if key not in _EMPTY:
        _EMPTY[key] = T.problem(case, b).solve(*sol.window, None, max_iter=MAX_ITER)
    return _EMPTY[key]


def _engine(case, rows, cap, warm, safe=False, refine=None, max_iter=MAX_ITER):
    """A prepared engine of the instances `rows` of a case."""
    c, d, spec = T.CASES[case], T.data(), T.spec_of(case)
    eng = _bounded_engine(spec, N, len(rows), max_iter=max_iter)
    if refine is not None:
        eng.set_refinement(refine)
    if cap is not None:
        eng.set_large_box_capacity(cap)
    if safe:
        eng.set_large_box_safeguard(True)
    if warm is not None:
        eng.set_large_box_warm_start(warm)
    eng.set_data(d["u_d"][rows], d["y_d"][rows])
    if c["box"]["u"] is not None:
        eng.set_input_bounds(*c["box"]["u"])
    if c["box"]["y"] is not None:
        eng.set_output_bounds(*c["box"]["y"])
    eng.prepare()
    return eng


def _out(res):
    return [x.copy() for x in res]


def _check(case, b, sol, s, x, i, tag, iters=None):
    """Row i of a step against the helper's solution `sol` of instance b, every figure printed first."""
    spec = T.spec_of(case)
    na, nu, ny = _sections(spec, N)
    u, cost, st, it = s[0][i], s[1][i], s[2][i], s[3][i]
    want = sol.iters if iters is None else iters
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s %s b=%d status %d iters %d/%d k %d peak %d margin %.1e err_u %.1e err_cost %.1e" %
          (case, tag, b, st, it, want, np.count_nonzero(sol.active), sol.peak, sol.margin, eu, ec))
    assert sol.status == "optimal" and st == 0, (b, sol.status, st)
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    if sol.margin >= 1e-7:                                                         # (the exclusion rule; true of every instance here)
        assert it == want, (b, it, want)
        assert np.array_equal(_signed_active(x[i], sol), sol.active), b
    hard = (sol.idx >= na) & (sol.idx < na + nu + ny)                              # an active input or output equals its bound bit for bit
    for side, bnd in ((1, sol.hi), (-1, sol.lo)):
        on = hard & (sol.active == side)
        assert np.array_equal(x[i][sol.idx[on]], bnd[on]), (b, side)


def _margins_hold(case, loops):
    """At most 2 of 8 instances may be left out of the count and set comparison: by the helper, none is."""
    mg = {b: min(s.margin for s in sl) for b, sl in loops.items()}
    print("case %s margins of the seeded loops" % case, {b: "%.1e" % v for b, v in mg.items()})
    left_out = [b for b, v in mg.items() if v < 1e-7]
    assert left_out == [], left_out


def _bit_equal(a, b_):
    for p, q in zip(a, b_):
        assert np.array_equal(p, q, equal_nan=True)


def _record_iters(eng, i, cap):
    lib = L.load()
    rv = (eng.m + eng.p) * (eng.L + eng.n) + 1 & ~1
    nm = 4 + cap + rv + 4
    meta = np.zeros(nm, np.int32)
    L.check(lib.ddmpc_debug_workspace(eng._h, i, C.c_void_p(), 0, C.c_void_p(meta.ctypes.data), nm, C.c_void_p(), C.c_void_p()))
    return int(meta[1]), int(meta[2])


# ------------------------------------------------------------------------------------------------ 1. contract
def test_contract_of_the_option(gpu):
    d = T.data()
    spec = T.spec_of("A")
    rows = [0, 1]
    loops, win = _windows("A", rows)
    with _bounded_engine(spec, N, 2) as eng:
        for bad in (-1, 2, 16):
            code, msg = _code(lambda v: L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_LARGE_BOX_WARM_START, v)), bad)
            assert code == L.ERR_INVALID and "DDMPC_OPT_LARGE_BOX_WARM_START" in msg, (bad, msg)
        eng.set_data(d["u_d"][rows], d["y_d"][rows])
        eng.set_input_bounds(*T.CASES["A"]["box"]["u"])
        eng.set_large_box_capacity(128)
        eng.prepare()
        for on in (True, False):
            eng.solve(*win[0])
            eng.get_solution("ubar")
            eng.set_large_box_warm_start(on)
            code, _ = _code(eng.get_solution, "ubar")                              # the call forgets the last solution ...
            assert code == L.ERR_NOT_READY
        eng.set_large_box_warm_start(True)
        t = _out(eng.step(*win[0]))                                                # ... and keeps what prepare kept
        f = _out(eng.solve(*win[0]))
        assert np.all(f[2] == 0)
        _bit_equal(f, t)
    # accepted without effect: 136 rows with bounds, 296 rows without bounds (slack NONE), slack-only CONVEX at 296 rows, NOMINAL
    spec136 = orc.spec_from_params(slack_var_constraint_type=1, L=30)
    nom136 = orc.spec_from_params(controller_type=0, L=30)
    d136 = harness.generate_batch(range(2), N=400)
    w136 = (d136["u_d"][:, -spec136.n:, :].reshape(2, -1).copy(), d136["y_d"][:, -spec136.n:, :].reshape(2, -1).copy())
    assert (spec136.m + spec136.p) * spec136.Ln == 136
    configs = [(spec136, 400, d136, w136, True), (T.spec_of("B"), N, d, win[0], False), (spec, N, d, win[0], False),
               (nom136, 400, d136, w136, False)]
    for sp, nn, dd, w, box in configs:
        res = []
        for on in (None, True):
            with _bounded_engine(sp, nn, 2) as eng:
                if on:
                    eng.set_large_box_warm_start(True)
                eng.set_data(dd["u_d"][:2], dd["y_d"][:2])
                if box:
                    eng.set_input_bounds([-4.0, -4.0], [6.0, 6.0])
                res.append(_out(eng.solve(*w)) + _out(eng.step(*w)) + _out(eng.step(*w)))
        assert np.all(res[0][2] == 0)
        _bit_equal(res[0], res[1])


# ------------------------------------------------------------------------------------------------ 2. the first step after prepare
def test_first_step_after_prepare_has_no_seed(gpu):
    rows = [0, 1, 2, 3]
    loops, win = _windows("A", rows)
    with _engine("A", rows, 128, None) as e0, _engine("A", rows, 128, True) as e1:
        a, b_ = _out(e0.step(*win[0])), _out(e1.step(*win[0]))
        assert np.all(a[2] == 0) and [int(v) for v in a[3]] == [loops[b][0].iters for b in rows]
        _bit_equal(a, b_)                                                          # above capacity 64: bit-equal to the option 0
    # at capacity 64 the option moves the handle to the wide kernel: it agrees with the twin to rounding
    with _engine("A", rows, 64, None) as e0, _engine("A", rows, 64, True) as e1:
        a, xa = _out(e0.step(*win[0])), _full_x(e0)
        b_, xb = _out(e1.step(*win[0])), _full_x(e1)
    fine = [i for i, b in enumerate(rows) if loops[b][0].peak <= 64]
    assert fine == [0, 2] and np.all(a[2][fine] == 0)
    assert np.array_equal(a[2], b_[2]) and np.array_equal(a[3], b_[3])             # (instances 1 and 3 outgrow 64: status 4 in both)
    for q, name in enumerate(("u_opt", "cost")):
        e = np.max(np.abs(a[q][fine] - b_[q][fine])) / np.max(np.abs(a[q][fine]))
        print("capacity 64, the option against the twin kernel: %s rel %.1e" % (name, e))
        assert e <= 1e-12
    for i in fine:
        sol = loops[rows[i]][0]
        assert np.array_equal(_signed_active(xa[i], sol), _signed_active(xb[i], sol))


# ------------------------------------------------------------------------------------------------ 3. seeded sequences
@pytest.mark.parametrize("case,rows,cap", [("A", [0, 1, 2, 3], 128), ("B", [0, 1, 2], 128), ("D", [0, 1], 192)])
def test_seeded_sequences_take_the_helpers_solves(gpu, case, rows, cap):
    """Four windows.  A: 3 - 5 solves where the empty start has 7 - 10; B: 3 - 6 instead of 16 - 27 (instance 1 peaks at exactly
    128 components at window 0); D: 3 - 4 instead of 5 - 7 at 124 - 138 components."""
    loops, win = _windows(case, rows)
    _margins_hold(case, loops)
    assert max(s.peak for sl in loops.values() for s in sl) <= cap
    if case == "B":
        assert loops[1][0].peak == 128
    for b in rows:
        emp = [_empty(case, b, s).iters for s in loops[b]]
        print("case %s b=%d solves per window: empty %s seeded %s" % (case, b, emp, [s.iters for s in loops[b]]))
        assert all(s.seeded and s.iters < e for s, e in zip(loops[b][1:], emp[1:]))
    for refine in ("off", None):
        with _engine(case, rows, cap, True, refine=refine) as eng:
            for w, (up, yp) in enumerate(win):
                s = _out(eng.step(up, yp))
                x = _full_x(eng)
                for i, b in enumerate(rows):
                    _check(case, b, loops[b][w], s, x, i, "window %d refine=%s" % (w, refine))


# ------------------------------------------------------------------------------------------------ 4. the cold contract
def test_solve_keeps_the_cold_contract_and_leaves_a_seed(gpu):
    rows = [0, 1, 2]
    loops, win = _windows("B", rows)
    with _engine("B", rows, 128, None) as e0, _engine("B", rows, 128, True) as e1:
        e1.step(*win[0])                                                           # (a seed is there: ddmpc_solve must not read it)
        for w in (1, 0):
            _bit_equal(_out(e0.solve(*win[w])), _out(e1.solve(*win[w])))
        s = _out(e1.step(*win[1]))                                                 # seeded by the solve at window 0
        x = _full_x(e1)
        for i, b in enumerate(rows):
            _check("B", b, loops[b][1], s, x, i, "step behind ddmpc_solve")


# ------------------------------------------------------------------------------------------------ 5. what drops the seed
def test_seed_is_dropped(gpu):
    rows = [0, 2]
    c, d = T.CASES["A"], T.data()
    loops, win = _windows("A", rows)
    events = {
        "set_data": lambda e: e.set_data(d["u_d"][rows], d["y_d"][rows]),
        "set_setpoints": lambda e: e.set_setpoints(T.spec_of("A").u_s, T.spec_of("A").y_s),
        "set_input_bounds": lambda e: e.set_input_bounds(*c["box"]["u"]),
        "set_output_bounds": lambda e: e.set_output_bounds(None, None),
        "prepare": lambda e: (e.set_refinement("auto"), e.prepare()),              # (the option forgets what prepare kept: a new one)
        "option 12": lambda e: e.set_large_bounds(True),
        "option 13": lambda e: e.set_large_box_capacity(128),
        "option 14": lambda e: e.set_large_box_safeguard(False),
        "option 16": lambda e: e.set_large_box_warm_start(True),
    }
    with _engine("A", rows, 128, None) as e0:
        base = _out(e0.step(*win[1]))
    emp = [_empty("A", b, loops[b][1]).iters for b in rows]
    assert [int(v) for v in base[3]] == emp and np.all(base[2] == 0)
    with _engine("A", rows, 128, True) as eng:
        eng.step(*win[0])
        s = _out(eng.step(*win[1]))
        assert [int(v) for v in s[3]] == [loops[b][1].iters for b in rows] and all(a < e for a, e in zip(s[3], emp))   # seeded
        for name, ev in events.items():
            eng.step(*win[0])
            ev(eng)
            s = _out(eng.step(*win[1]))
            print("after %s: iters %s (empty start %s)" % (name, s[3], emp))
            _bit_equal(base, s)


# ------------------------------------------------------------------------------------------------ 6. status > 1 leaves an empty seed
def test_a_failed_instance_leaves_an_empty_seed(gpu):
    """Case B at capacity 128: instance 3 ends at the cap of 50 (status 4); instance 0 next to it converges.  At the next step
    both get the past window of instance 0's second window: instance 3 starts empty (17 solves), instance 0 seeded (4)."""
    rows = [3, 0]
    d = T.data()
    loops, win0 = _windows("B", [0])
    n = T.spec_of("B").n
    tail3 = (d["u_d"][3][-n:].reshape(-1), d["y_d"][3][-n:].reshape(-1))
    first = (np.stack([tail3[0], loops[0][0].window[0]]), np.stack([tail3[1], loops[0][0].window[1]]))
    w1 = loops[0][1].window
    second = (np.stack([w1[0], w1[0]]), np.stack([w1[1], w1[1]]))
    ref3 = T.problem("B", 3).solve(*w1, None, max_iter=MAX_ITER)
    print("instance 3 at the window of instance 0: %s iters %d peak %d margin %.1e" % (ref3.status, ref3.iters, ref3.peak, ref3.margin))
    assert ref3.status == "optimal" and ref3.margin >= 1e-7 and ref3.peak <= 128
    with _engine("B", rows, 128, None) as e0, _engine("B", rows, 128, True) as eng:
        s = _out(eng.step(*first))
        assert s[2][0] == 4 and s[3][0] == MAX_ITER and s[2][1] == 0
        s = _out(eng.step(*second))
        x = _full_x(eng)
        _check("B", 3, ref3, s, x, 0, "behind status 4")
        _check("B", 0, loops[0][1], s, x, 1, "the neighbour, seeded")
        b0 = _out(e0.step(*second))
        for q in range(4):
            assert np.array_equal(s[q][0], b0[q][0])                               # from the empty set: the bits of the option 0


# ------------------------------------------------------------------------------------------------ 7. the restart at the cap
def test_a_seeded_run_at_the_cap_starts_again(gpu):
    """[-4, 6] CONVEX, max_iter = 3 (tests/test_large_box_warm_reference.py): window 2 takes 3 solves from the empty set, window 3
    seeded with its set would take 4 -- the seeded run ends at the cap, the empty start finishes in 2: optimal, 3 - 1 + 2 = 4."""
    rows = [0, 2]
    loops, win = _windows("W", rows, n_win=5)
    prob = {b: T.problem("W", b) for b in rows}
    want = {b: prob[b].solve(*loops[b][3].window, loops[b][2].set, max_iter=3) for b in rows}
    for b in rows:
        print("b=%d helper: fell back %s iters %d margin %.1e" % (b, want[b].fell_back, want[b].iters, want[b].margin))
        assert want[b].fell_back and want[b].status == "optimal" and want[b].iters == 4 and want[b].margin >= 1e-7
    with _engine("W", rows, 128, True, max_iter=3) as eng, _engine("W", rows, 128, None, max_iter=3) as e0:
        s = _out(eng.step(*win[2]))
        assert np.all(s[2] == 0) and np.all(s[3] == 3)
        s = _out(eng.step(*win[3]))
        x = _full_x(eng)
        for i, b in enumerate(rows):
            _check("W", b, want[b], s, x, i, "restart")
        b0 = _out(e0.step(*win[3]))
        assert np.all(b0[3] == 2)
        for q in range(3):
            assert np.array_equal(s[q], b0[q])                                     # the restarted run is the option 0's: the same bits


# ------------------------------------------------------------------------------------------------ 8. with the safeguard
def test_with_the_safeguard(gpu):
    """Option 14 on, case B, capacity 192, instances 2, 3, 4.  Instance 3 ends at the cap at window 0 and is finished by the primal
    method (50 + 124); the steps at its next three windows start from the safeguard's final set: 3 5 4 solves instead of 19 18
    18.  The neighbours stay at the bars with the seeded counts."""
    rows = [2, 3, 4]
    d, spec = T.data(), T.spec_of("B")
    n = spec.n
    tail3 = (d["u_d"][3][-n:].reshape(-1), d["y_d"][3][-n:].reshape(-1))
    prim = sref.solve_primal(spec, d["u_d"][3], d["y_d"][3], *tail3, T.CASES["B"]["box"])
    assert prim.status == "optimal" and prim.peak <= 192
    loops = {b: (T.loop("B", 3, 4, first=prim) if b == 3 else T.loop("B", b, 4)) for b in rows}
    loops, win = _windows("B", rows, loops=loops)
    print("instance 3: seeded %s empty %s" % ([s.iters for s in loops[3][1:]], [_empty("B", 3, s).iters for s in loops[3][1:]]))
    assert [s.iters for s in loops[3][1:]] == [3, 5, 4]
    _margins_hold("B", loops)
    with _engine("B", rows, 192, True, safe=True) as eng, _engine("B", rows, 192, None, safe=True) as e0:
        s = _out(eng.solve(*win[0]))
        _bit_equal(s, _out(e0.solve(*win[0])))                                     # as today
        x = _full_x(eng)
        _check("B", 3, prim, s, x, 1, "window 0, safeguard", iters=MAX_ITER + prim.iters)
        for w in (1, 2, 3):
            s = _out(eng.step(*win[w]))
            x = _full_x(eng)
            for i, b in enumerate(rows):
                _check("B", b, loops[b][w], s, x, i, "window %d, option 14 on" % w)


# ------------------------------------------------------------------------------------------------ 9. the per-step closed loop
def test_per_step_closed_loop(gpu):
    rows, n_steps = [0, 1, 2], 4
    c, d, spec = T.CASES["A"], T.data(), T.spec_of("A")
    P = orc.FOUR_TANK
    n = spec.n
    up = d["u_d"][rows][:, -n:, :].reshape(len(rows), -1).copy()
    yp = d["y_d"][rows][:, -n:, :].reshape(len(rows), -1).copy()
    w = np.stack([T.noise(b, n_steps) for b in rows])
    out, its = [], []
    for on in (None, True):
        with _engine("A", rows, 128, on) as eng:
            out.append(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][rows], up, yp, w))
            assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
            its.append([_record_iters(eng, i, 128) for i in range(len(rows))])
    assert np.all(out[0][2] == 0) and np.all(out[1][2] == 0)                       # no stopped instance
    for q, name in ((0, "u_sys"), (1, "y_sys")):
        e = np.max(np.abs(out[0][q] - out[1][q])) / np.max(np.abs(out[0][q]))
        print("per-step loop with the option against without: %s rel %.1e" % (name, e))
        assert e <= 1e-9
    print("solves of the last step (status, iterations): without", its[0], "with", its[1])
    for i, b in enumerate(rows):                                                   # the loop's own steps seed each other
        assert its[0][i] == (0, _empty("A", b, T.loop("A", b)[3]).iters) and its[1][i] == (0, T.loop("A", b)[3].iters)


# ------------------------------------------------------------------------------------------------ 10. the controller class
def test_controller_class_passes_the_option_through(gpu):
    from direct_data_driven_mpc.direct_data_driven_mpc_controller import (
        DataDrivenMPCType, DirectDataDrivenMPCController, SlackVarConstraintTypes)
    c, d = T.CASES["A"], T.data()
    cfg = harness.controller_params()
    b = 1
    ctrl = DirectDataDrivenMPCController(
        n=4, m=2, p=2, u_d=d["u_d"][b], y_d=d["y_d"][b], L=LH, Q=cfg["Q"] * np.eye(2 * LH), R=cfg["R"] * np.eye(2 * LH),
        u_s=cfg["u_s"].reshape(-1, 1), y_s=cfg["y_s"].reshape(-1, 1), eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
        lamb_sigma=cfg["lamb_sigma"], c=cfg["c"], slack_var_constraint_type=SlackVarConstraintTypes.CONVEX,
        controller_type=DataDrivenMPCType.ROBUST, n_mpc_step=cfg["n_mpc_step"])
    ctrl.set_input_bounds(*c["box"]["u"])
    ctrl.set_large_box_capacity(128)
    assert ctrl.get_problem_solve_status() == "optimal"
    u0 = ctrl.get_optimal_control_input().copy()
    ctrl.set_large_box_warm_start(True)
    assert ctrl.get_problem_solve_status() == "optimal"
    u1 = ctrl.get_optimal_control_input().copy()
    sol = T.loop("A", b)[0]
    eu = np.max(np.abs(u1 - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    print("controller class err_u %.1e, against the option off %.1e" % (eu, np.max(np.abs(u1 - u0))))
    assert eu < TOL_U
    ctrl._engine.close()
    ctrl._engine = None
    ctrl.update_and_solve_data_driven_mpc()                                        # a new engine handle: the option is set again
    assert ctrl._large_box_warm_start is True
    assert ctrl.get_problem_solve_status() == "optimal" and np.array_equal(ctrl.get_optimal_control_input(), u1)
