"""DDMPC_OPT_LARGE_BOX_SAFEGUARD: bounds beyond 271 rows, an instance whose primal-dual iteration ends at max_iter is solved
again inside the same call by the primal active-set method of DESIGN 5.5 on the reduced system (rr3_box_safeguard_kernel,
ddmpc_rr3_box_safe.hpp).

Against the reduced-space helper tests/_large_box_safeguard_ref.py (pinned on the CPU by
tests/test_large_box_safeguard_reference.py) at the bars of tests/test_gpu_large_box_capacity.py: inputs 1e-8, cost 1e-9
relative, status identical; solve counts and signed sets are compared where the helper's margin is >= 1e-7, and at most 2 of 8
instances may be left out of that comparison -- by the helper none is (the smallest margin is 1.8e-6 on the cases A and B,
2.9e-3 on the box [-4, 6]), which is asserted.  Under DDMPC_REFINE_OFF and under the default where outputs are compared.

Fixture: four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7 at the data tail, DDMPC_OPT_LARGE_BOUNDS = 1.  The primal method
per instance (solves; largest working set; final set):
  u in [-4, 6], NONE / CONVEX   4 - 8;      6 - 10;    6 - 10
  case A  u in [0, 2], CONVEX   68 - 129;   59 - 103;  45 - 71      (19 - 45 releases)
  case B  u in [0.9, 1.1], NONE 124 - 147;  132;       117 - 126    (the set of the first solve has 111 - 124 components; the
                                                                     129th joins at solve 6 - 19, at solve 15 on instance 3)
  case E  instance 1            277;        264;       249          (the 257th component joins at solve 61)
"""
import ctypes as C

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _large_box_ref as lref
import _large_box_safeguard_ref as sref
from test_gpu_large_bounds import _bounded_engine, _code, _full_x, _sections, _signed_active
from test_gpu_round5 import _four_tank_long

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
B8, LH, N, MAX_ITER = 8, 70, 700, 50
CASES = dict(lref.CASES)
CASES["Wn"] = dict(box=dict(u=([-4.0, -4.0], [6.0, 6.0]), y=None), slack="none")
CASES["Wc"] = dict(box=dict(u=([-4.0, -4.0], [6.0, 6.0]), y=None), slack="convex")

_DATA, _REF = {}, {}


def _data(slack):
    if slack not in _DATA:
        _DATA[slack] = _four_tank_long(B8, LH, N, slack)
    return _DATA[slack]


def _ref(case, b, kind="primal"):
    """The primal helper's ("primal") or the primal-dual helper's ("pd", max_iter 50) solution of instance b, computed once."""
    if (case, b, kind) not in _REF:
        c = CASES[case]
        spec, d, up, yp = _data(c["slack"])
        args = (spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], c["box"])
        _REF[(case, b, kind)] = sref.solve_primal(*args) if kind == "primal" else lref.solve_reduced(*args, max_iter=MAX_ITER)
    return _REF[(case, b, kind)]


def _setup(eng, case, rows, cap, safe, refine):
    c = CASES[case]
    spec, d, up, yp = _data(c["slack"])
    if refine is not None:
        eng.set_refinement(refine)
    if cap is not None:
        eng.set_large_box_capacity(cap)
    if safe:
        eng.set_large_box_safeguard(True)
    eng.set_data(d["u_d"][rows], d["y_d"][rows])
    if c["box"]["u"] is not None:
        eng.set_input_bounds(*c["box"]["u"])
    if c["box"]["y"] is not None:
        eng.set_output_bounds(*c["box"]["y"])


def _run(case, cap, safe, max_iter=MAX_ITER, rows=None, refine=None, prepare=False):
    """(solve outputs, [alpha; ubar; ybar; sigma], step outputs on kept factors, peak k per instance) of the instances `rows`."""
    c = CASES[case]
    spec, d, up, yp = _data(c["slack"])
    rows = list(range(B8)) if rows is None else list(rows)
    with _bounded_engine(spec, N, len(rows), max_iter=max_iter) as eng:
        _setup(eng, case, rows, cap, safe, refine)
        s = [x.copy() for x in eng.solve(up[rows], yp[rows])]
        x = _full_x(eng)
        rec = [_record(eng, i, cap) for i in range(len(rows))]
        assert [q[:2] for q in rec] == [(int(s[2][i]), int(s[3][i])) for i in range(len(rows))]   # the record reads the same result
        peak = [q[2] for q in rec]
        t = None
        if prepare:
            eng.prepare()
            t = [x_.copy() for x_ in eng.step(up[rows], yp[rows])]
    return s, x, t, peak


def _record(eng, i, cap):
    """(state, iterations, peak k) of instance i from the record of the last solve (ddmpc_debug_workspace)."""
    lib = L.load()
    rv = (eng.m + eng.p) * (eng.L + eng.n) + 1 & ~1
    nm = 4 + (cap or 64) + rv + 4
    meta = np.zeros(nm, np.int32)
    L.check(lib.ddmpc_debug_workspace(eng._h, i, C.c_void_p(), 0, C.c_void_p(meta.ctypes.data), nm, C.c_void_p(), C.c_void_p()))
    return int(meta[1]), int(meta[2]), int(meta[nm - 2])


def _check(case, b, s, x, i, max_iter, tag):
    """Row i of a solve that went through the safeguard against the primal helper's solution of instance b."""
    c = CASES[case]
    spec, d, _, _ = _data(c["slack"])
    sol = _ref(case, b)
    na, nu, ny = _sections(spec, N)
    u, cost, st, it = s[0][i], s[1][i], s[2][i], s[3][i]
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s %s b=%d status %d iters %d (%d + %d) k %d largest %d margin %.1e err_u %.1e err_cost %.1e" %
          (case, tag, b, st, it, max_iter, sol.iters, np.count_nonzero(sol.active), sol.peak, sol.margin, eu, ec))
    assert sol.status == "optimal" and st == 0, (b, sol.status, st)
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    if sol.margin >= 1e-7:                                                         # (the exclusion rule; true of every instance here)
        assert it == max_iter + sol.iters, (b, it, sol.iters)
        assert np.array_equal(_signed_active(x[i], sol), sol.active), b
    hard = (sol.idx >= na) & (sol.idx < na + nu + ny)                              # an active input or output equals its bound bit for bit
    for side, bnd in ((1, sol.hi), (-1, sol.lo)):
        on = hard & (sol.active == side)
        assert np.array_equal(x[i][sol.idx[on]], bnd[on]), (b, side)
    return sol


def _margins_hold(case, rows):
    """At most 2 of 8 instances may be left out of the count and set comparison: by the helper, none is."""
    left_out = [b for b in rows if _ref(case, b).margin < 1e-7]
    print("case %s margins of the primal method" % case, ["%.1e" % _ref(case, b).margin for b in rows])
    assert left_out == [], left_out


def _bit_equal(a, b_, rows=None):
    for p, q in zip(a, b_):
        p, q = (p, q) if rows is None else (p[rows], q[rows])
        assert np.array_equal(p, q, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 1. contract
def test_contract_of_the_option(gpu):
    lib = L.load()
    spec, d, up, yp = _data("convex")
    box = CASES["Wc"]["box"]["u"]
    with _bounded_engine(spec, N, 2) as eng:
        for bad in (2, -1, 14):
            code, msg = _code(lambda v: L.check(lib.ddmpc_set_option(eng._h, L.OPT_LARGE_BOX_SAFEGUARD, v)), bad)
            assert code == L.ERR_INVALID and "DDMPC_OPT_LARGE_BOX_SAFEGUARD" in msg, (bad, msg)
        eng.set_data(d["u_d"][:2], d["y_d"][:2])
        eng.set_input_bounds(*box)
        for on in (True, False, True):
            eng.solve(up[:2], yp[:2])
            eng.get_solution("ubar")
            eng.set_large_box_safeguard(on)
            code, msg = _code(eng.get_solution, "ubar")                            # the call forgets the last solution
            assert code == L.ERR_NOT_READY
        # a kept prepare stays valid: step after the call equals a fresh solve
        eng.set_large_box_safeguard(False)
        eng.prepare()
        eng.set_large_box_safeguard(True)
        t = [x.copy() for x in eng.step(up[:2], yp[:2])]
        f = [x.copy() for x in eng.solve(up[:2], yp[:2])]
        assert np.all(f[2] == 0)
        _bit_equal(f, t)

    def outputs(spec_, n_cols, dd, a, b_, prep, bounded):
        with _bounded_engine(spec_, n_cols, 2) as eng:
            eng.set_data(dd["u_d"][:2], dd["y_d"][:2])
            if bounded:
                eng.set_input_bounds(*box)
            prep(eng)
            return [x.copy() for x in eng.solve(a[:2], b_[:2])]

    # no effect on a handle of at most 271 rows, nor on an unbounded 296-row CONVEX handle: bit-equal results
    spec136 = orc.spec_from_params(slack_var_constraint_type=1, L=30)
    d136 = harness.generate_batch(range(2), N=400)
    up136 = d136["u_d"][:, -spec136.n:, :].reshape(2, -1).copy()
    yp136 = d136["y_d"][:, -spec136.n:, :].reshape(2, -1).copy()
    assert (spec136.m + spec136.p) * spec136.Ln == 136
    for args in ((spec136, 400, d136, up136, yp136), (spec, N, d, up, yp)):
        bounded = args[0] is spec136
        base = outputs(*args, lambda eng: None, bounded)
        assert np.all(base[2] == 0)
        _bit_equal(base, outputs(*args, lambda eng: eng.set_large_box_safeguard(True), bounded))
    # DDMPC_OPT_BOX_SAFEGUARD (option 11) still has no effect at 296 rows
    base = outputs(spec, N, d, up, yp, lambda eng: None, True)
    assert np.all(base[2] == 0)
    _bit_equal(base, outputs(spec, N, d, up, yp, lambda eng: eng.set_box_safeguard(True), True))
    # with the option the wide kernels serve the handle at capacity 64 too: the instances that converge agree to rounding
    # (DESIGN 5.5.2 measured 4e-15: the wide kernel forms the right-hand side of the k x k system differently), same status and iters
    safe = outputs(spec, N, d, up, yp, lambda eng: eng.set_large_box_safeguard(True), True)
    for q, name in enumerate(("u_opt", "cost")):
        e = np.max(np.abs(safe[q] - base[q])) / np.max(np.abs(base[q]))
        print("capacity 64, option 1 against 0: %s rel %.1e" % (name, e))
        assert e <= 1e-12
    assert np.array_equal(safe[2], base[2]) and np.array_equal(safe[3], base[3])


# ------------------------------------------------------------------------------------------------ 2. case B at capacity 192
def test_case_b_the_cycling_instance_is_solved_at_capacity_192(gpu):
    """u in [0.9, 1.1], slack NONE, max_iter 50: instance 3 cycles to the cap (status 4 without the option) and is optimal after
    124 solves of the primal method with working sets of up to 132 components; the other seven keep their bits."""
    others = [0, 1, 2, 4, 5, 6, 7]
    _margins_hold("B", range(B8))
    sol = _ref("B", 3)
    assert _ref("B", 3, "pd").status == "solver_error" and (sol.iters, sol.peak) == (124, 132)
    for refine in ("off", None):
        s0, _, _, _ = _run("B", 192, False, refine=refine)
        assert s0[2][3] == 4 and s0[3][3] == MAX_ITER and np.all(s0[2][others] == 0)
        s, x, _, peak = _run("B", 192, True, refine=refine)
        print("B status", s[2], "iters", s[3], "peak", peak)
        _check("B", 3, s, x, 3, MAX_ITER, "cap=192 refine=%s" % refine)
        assert s[3][3] == MAX_ITER + 124 and peak[3] == 132
        _bit_equal(s, s0, others)                                                  # below max_iter: bit-equal to the option 0
        s1, x1, _, _ = _run("B", 192, True, rows=[3], refine=refine)
        for a, b_ in zip(s, s1):
            assert np.array_equal(a[[3]], b_)                                      # the same bits alone in a batch
        assert np.array_equal(x[3], x1[0])


# ------------------------------------------------------------------------------------------------ 3. every instance through the safeguard
@pytest.mark.parametrize("case,cap", [("Wn", 64), ("Wc", 64), ("A", 128)])
def test_every_instance_through_the_safeguard(gpu, case, cap):
    """max_iter = 3 sends all eight instances to the primal method (the primal-dual rule needs 4 or more iterations on each).
    [-4, 6] at capacity 64: one block of columns, sets of at most 10.  Case A at capacity 128: two blocks, up to 129 solves with
    up to 45 releases -- every release moves the last column into the slot of the leaving one."""
    _margins_hold(case, range(B8))
    assert all(_ref(case, b, "pd").status == "optimal" and _ref(case, b, "pd").iters > 3 for b in range(B8))
    if case == "A":
        assert max(_ref(case, b).peak for b in range(B8)) > 64 and max(_ref(case, b).releases for b in range(B8)) >= 40
    for refine in ("off", None):
        s, x, t, peak = _run(case, cap, True, max_iter=3, refine=refine, prepare=True)
        _bit_equal(s, t)                                                           # ddmpc_step on kept factors is bit-equal to ddmpc_solve
        s50, x50, _, _ = _run(case, cap, True, refine=refine)                      # the primal-dual rule below its cap of 50
        assert np.all(s50[2] == 0) and np.all(s50[3] < MAX_ITER)
        for b in range(B8):
            sol = _check(case, b, s, x, b, 3, "cap=%d refine=%s" % (cap, refine))
            assert peak[b] >= sol.peak
            pd = _ref(case, b, "pd")
            assert s50[3][b] == pd.iters and np.array_equal(_signed_active(x50[b], pd), _signed_active(x[b], pd))
        eu = max(np.max(np.abs(s[0][b] - s50[0][b])) / np.max(np.abs(s50[0][b])) for b in range(B8))
        ec = max(abs(s[1][b] - s50[1][b]) / abs(s50[1][b]) for b in range(B8))
        print("%s refine=%s: the primal method against the primal-dual rule, inputs %.1e cost %.1e" % (case, refine, eu, ec))
        assert eu < TOL_U and ec < TOL_COST


# ------------------------------------------------------------------------------------------------ 4. the capacity inside the safeguard
@pytest.mark.parametrize("case,cap,b", [("B", 128, 3), ("E", 256, 1)])
def test_working_set_beyond_the_capacity(gpu, case, cap, b):
    """The working set of the primal method outgrows the capacity: status 4, NaN outputs, iters = max_iter + the number of the
    solve that could not be made.  Case B instance 3 at capacity 128: the set of the first solve has 115 components and the 129th
    joins at solve 15, so iters = 65.  Case E instance 1 at capacity 256: 197 at the first solve, the 257th at solve 61, iters = 111.
    (The set of the first solve is what hat(empty) violates -- 115 of 132 here, in the full-space method too -- not all nbox
    components, so the refusal does not come at the first solve, iters = 51.)  The neighbours are bit-equal to the option 0."""
    others = [i for i in range(B8) if i != b]
    sol = _ref(case, b)
    over = sol.first_over(cap)
    assert sol.margin >= 1e-7 and over == {"B": 15, "E": 61}[case] and sol.sizes[0] <= cap
    assert _ref(case, b, "pd").status == "solver_error"
    for refine in ("off", None):
        s0, _, _, _ = _run(case, cap, False, refine=refine)
        s, _, t, _ = _run(case, cap, True, refine=refine, prepare=True)
        _bit_equal(s, t)
        print(case, "status", s[2], "iters", s[3])
        assert s0[2][b] == 4 and s0[3][b] == MAX_ITER
        assert s[2][b] == 4 and s[3][b] == MAX_ITER + over, (s[2][b], s[3][b], over)
        assert np.all(np.isnan(s[0][b])) and np.isnan(s[1][b])
        _bit_equal(s, s0, others)


# ------------------------------------------------------------------------------------------------ 5. step and loop
def test_step_and_per_step_closed_loop_case_b(gpu):
    """Case B, capacity 192, option on: ddmpc_step on kept factors is bit-equal to ddmpc_solve; the record shows a peak of at
    least 132 for instance 3; a 3-step per-step closed loop (instances 3, 0, 5; noise seed 5) has no stopped instance and equals
    a loop driven by the helpers -- the primal-dual helper, and the primal helper where that one ends at the cap -- to 1e-8."""
    c = CASES["B"]
    spec, d, up, yp = _data("none")
    s, _, t, peak = _run("B", 192, True, prepare=True)
    _bit_equal(s, t)
    assert np.all(s[2] == 0) and peak[3] >= 132
    rows, n_steps = [3, 0, 5], 3
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (len(rows), n_steps, 2))
    with _bounded_engine(spec, N, len(rows), max_iter=MAX_ITER) as eng:
        _setup(eng, "B", rows, 192, True, None)
        u_sys, y_sys, st, _, _, _ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][rows], up[rows], yp[rows], w)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
    print("loop status", st)
    assert np.all(st == 0)                                                         # no stopped instance
    m, p = spec.m, spec.p
    for i, b in enumerate(rows):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        upb, ypb = up[b].copy(), yp[b].copy()
        ur, yr = np.zeros((n_steps, m)), np.zeros((n_steps, p))
        for k in range(n_steps):
            sol = lref.solve_reduced(spec, d["u_d"][b], d["y_d"][b], upb, ypb, c["box"], max_iter=MAX_ITER)
            how = "primal-dual, %d" % sol.iters
            if sol.status != "optimal":
                sol = sref.solve_primal(spec, d["u_d"][b], d["y_d"][b], upb, ypb, c["box"])
                how = "primal, %d solves, largest %d" % (sol.iters, sol.peak)
            print("loop b=%d step %d: %s (%s) margin %.1e" % (b, k, sol.status, how, sol.margin))
            assert sol.status == "optimal"
            u = sol.optimal_u[:m]
            y = plant.step(u, w[i][k])
            ur[k], yr[k] = u, y
            upb, ypb = np.concatenate([upb[m:], u]), np.concatenate([ypb[p:], y])
        eu, ey = np.max(np.abs(u_sys[i] - ur)) / np.max(np.abs(ur)), np.max(np.abs(y_sys[i] - yr)) / np.max(np.abs(yr))
        print("loop b=%d err_u %.1e err_y %.1e" % (b, eu, ey))
        assert eu < 1e-8 and ey < 1e-8, (b, eu, ey)


# ------------------------------------------------------------------------------------------------ 6. the controller class
def test_controller_class_passes_the_option_through(gpu):
    from direct_data_driven_mpc.direct_data_driven_mpc_controller import (
        DataDrivenMPCType, DirectDataDrivenMPCController, SlackVarConstraintTypes)
    c = CASES["B"]
    spec, d, up, yp = _data("none")
    cfg = harness.controller_params()
    b = 3
    ctrl = DirectDataDrivenMPCController(
        n=4, m=2, p=2, u_d=d["u_d"][b], y_d=d["y_d"][b], L=LH, Q=cfg["Q"] * np.eye(2 * LH), R=cfg["R"] * np.eye(2 * LH),
        u_s=cfg["u_s"].reshape(-1, 1), y_s=cfg["y_s"].reshape(-1, 1), eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
        lamb_sigma=cfg["lamb_sigma"], c=cfg["c"], slack_var_constraint_type=SlackVarConstraintTypes.NONE,
        controller_type=DataDrivenMPCType.ROBUST, n_mpc_step=cfg["n_mpc_step"])
    assert ctrl.get_problem_solve_status() == "optimal"
    ctrl.set_large_box_capacity(192)
    ctrl.set_input_bounds(*c["box"]["u"])
    assert ctrl.get_problem_solve_status() == "solver_error"                       # the primal-dual rule cycles to its cap
    ctrl.set_large_box_safeguard(True)
    assert ctrl.get_problem_solve_status() == "optimal"
    u1 = ctrl.get_optimal_control_input().copy()
    sol = _ref("B", b)
    eu = np.max(np.abs(u1 - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    print("controller class err_u %.1e" % eu)
    assert eu < TOL_U
    ctrl._engine.close()
    ctrl._engine = None
    ctrl.update_and_solve_data_driven_mpc()                                        # a new engine handle: the option is set again
    assert ctrl.get_problem_solve_status() == "optimal" and np.array_equal(ctrl.get_optimal_control_input(), u1)
