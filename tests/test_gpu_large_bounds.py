"""Input and output bounds for ROBUST controllers of 272 .. 1024 rows (ddmpc_set_input_bounds / ddmpc_set_output_bounds on
Route::RobustPhases; ddmpc_rr3_box.hpp): the table-driven box of the phase kernels -- the factor of the empty
active set kept, every active slack, input or output component a column of the Woodbury update on the trailing block of the
union "boxed last" order, one refinement pass on the final active set.

Against the full-space primal-dual active set of tests/_output_bounds_ref.py / tests/_input_bounds_ref.py at the bars of this
size (tests/test_gpu_large_robust_law.py): inputs 1e-8, cost 1e-9 relative, iteration counts and signed active sets equal
wherever the helper's margin is >= 1e-7 -- which it is on every instance below (checked on the CPU with the helper and with the
numpy restatement of tests/test_large_bounds_reference.py before the cases were written here), so no instance is left out.

Every handle opts in with DDMPC_OPT_LARGE_BOUNDS = 1 (`set_large_bounds`); without it the calls stay refused at this size.

Fixture: four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7 at the data tail, unless stated."""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

import _input_bounds_ref as uref
import _output_bounds_ref as yref
import test_gpu_closed_loop_plants as CP
from test_gpu_round5 import _four_tank_long, _spec_engine

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
INF = np.inf
B8, LH, N = 8, 70, 700
U_WIDE = ([-4.0, -4.0], [6.0, 6.0])                     # case 2
U_CH0 = ([-1.0, -INF], [3.0, INF])                      # case 3: channel 0 only
Y_UP = ([-INF, -INF], [0.66, 0.775])                    # case 4
U_CAP = ([0.0, 0.0], [2.0, 2.0])                        # case 6

_DATA, _REF = {}, {}


def _data(slack):
    if slack not in _DATA:
        _DATA[slack] = _four_tank_long(B8, LH, N, slack)
    return _DATA[slack]


def _opt_in(eng):
    """DDMPC_OPT_LARGE_BOUNDS: without it a handle beyond 271 rows refuses finite bounds, as before the option existed."""
    eng.set_large_bounds(True)
    return eng


def _bounded_engine(spec, N, B, **kw):
    return _opt_in(_spec_engine(spec, N, B, **kw))


def _reference(key, spec, u_d, y_d, up, yp, b, ubox, ybox, max_iter=100):
    """The helper's solution of instance b, computed once per configuration and instance."""
    if (key, b) not in _REF:
        ylo, yhi = ybox if ybox is not None else (-INF, INF)
        kw = dict(u_min=ubox[0], u_max=ubox[1]) if ubox is not None else {}
        _REF[(key, b)] = yref.solve_bounded(spec, u_d[b], y_d[b], up[b], yp[b], ylo, yhi, max_iter=max_iter, **kw)
    return _REF[(key, b)]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _full_x(eng):
    return np.concatenate([eng.get_solution(w) for w in ("alpha", "ubar", "ybar", "sigma")], axis=1)


def _signed_active(x, sol):
    """An active component sits on its bound (inputs and outputs exactly; a terminal slack is reconstructed as (y_s + bound) -
    y_s): within 1e-9 of the size of its box, a hundredth of the smallest distance the margin rule leaves to an inactive one."""
    v = x[sol.idx]
    tol = 1e-9 * np.maximum(np.where(np.isfinite(sol.lo), np.abs(sol.lo), 0.0), np.where(np.isfinite(sol.hi), np.abs(sol.hi), 0.0))
    with np.errstate(invalid="ignore"):
        return (np.abs(v - sol.hi) <= tol).astype(int) - (np.abs(v - sol.lo) <= tol).astype(int)


def _sections(spec, n_cols):
    """Sizes of [alpha; ubar; ybar; sigma]."""
    return n_cols - spec.Ln + 1, spec.Ln * spec.m, spec.Ln * spec.p


def _check_against(sol, b, spec, u_d, y_d, u, cost, it, x, tag):
    """Instance b of a solve against the helper's solution, every figure printed first."""
    na, nu, ny = _sections(spec, u_d.shape[1])
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s b=%d iters %d/%d k %d margin %.1e err_u %.1e err_cost %.1e" %
          (tag, b, it, sol.iters, np.count_nonzero(sol.active), sol.margin, eu, ec))
    assert sol.status == "optimal" and sol.margin >= 1e-7, (b, sol.status, sol.margin)
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    assert it == sol.iters, (b, it, sol.iters)
    assert np.array_equal(_signed_active(x, sol), sol.active), b
    # an active input or output equals its bound bit for bit
    hard = (sol.idx >= na) & (sol.idx < na + nu + ny)
    for side, bnd in ((1, sol.hi), (-1, sol.lo)):
        on = hard & (sol.active == side)
        assert np.array_equal(x[sol.idx[on]], bnd[on]), (b, side)
    # H alpha = [ubar; ybar + sigma]
    H = orc.hankel_matrix(np.concatenate([u_d[b], y_d[b]], axis=1), spec.Ln)
    z = H @ x[:na]
    ub = x[na:na + nu].reshape(spec.Ln, spec.m)
    yb = x[na + nu:na + nu + ny].reshape(spec.Ln, spec.p)
    sg = x[na + nu + ny:].reshape(spec.Ln, spec.p)
    zz = np.concatenate([ub, yb + sg], axis=1).reshape(-1)
    assert np.max(np.abs(z - zz)) <= 1e-8 * np.max(np.abs(zz)), b


def _solve_and_step(make, u_d, y_d, up, yp, ubox, ybox, refine=None):
    """(solve outputs, its [alpha; ubar; ybar; sigma], step outputs on the kept factors) of one bounded handle."""
    with make() as eng:
        if refine is not None:
            eng.set_refinement(refine)
        eng.set_data(u_d, y_d)
        if ubox is not None:
            eng.set_input_bounds(*ubox)
        if ybox is not None:
            eng.set_output_bounds(*ybox)
        s = [x.copy() for x in eng.solve(up, yp)]
        x = _full_x(eng)
        eng.prepare()
        t = [x_.copy() for x_ in eng.step(up, yp)]
    return s, x, t


def _compare(key, spec, make, u_d, y_d, up, yp, ubox, ybox, rows=None):
    """Case 2's assertions: every instance against the helper, step bit-equal to solve, under REFINE_OFF and the default."""
    rows = range(u_d.shape[0]) if rows is None else rows
    refs = {}
    for refine in ("off", None):
        s, x, t = _solve_and_step(make, u_d, y_d, up, yp, ubox, ybox, refine)
        for a, b_ in zip(s, t):
            assert np.array_equal(a, b_)                                   # ddmpc_step on kept factors is bit-equal to ddmpc_solve
        assert np.all(s[2][list(rows)] == 0), s[2]
        for b in rows:
            sol = refs[b] = _reference(key, spec, u_d, y_d, up, yp, b, ubox, ybox)
            _check_against(sol, b, spec, u_d, y_d, s[0][b], s[1][b], s[3][b], x[b], "%s refine=%s" % (key, refine))
    return refs, x


# ------------------------------------------------------------------------------------------------ 1. contract
def _code(fn, *a):
    with pytest.raises(L.DDMPCError) as e:
        fn(*a)
    return e.value.code, e.value.message


SETTERS = (("set_input_bounds", U_CAP, "u"), ("set_output_bounds", ([0.60, 0.72], [0.70, 0.82]), "y"))


def test_refusals(gpu):
    spec, d, up, yp = _data("convex")
    for name, ok, v in SETTERS:
        with _spec_engine(spec, N, 2) as eng:                                     # without the option: refused as it always was
            code, msg = _code(getattr(eng, name), *ok)
            assert code == L.ERR_UNSUPPORTED and "271" in msg and "DDMPC_OPT_LARGE_BOUNDS" in msg
            getattr(eng, name)([-INF, -INF], [INF, INF])
        with _bounded_engine(spec, N, 2) as eng:
            fn = getattr(eng, name)
            for lo, hi, word in (([np.nan, 0.0], [2.0, 2.0], v + "_min"), ([0.0, 0.0], [2.0, np.nan], v + "_max"),
                                 ([0.0, 2.0], [2.0, 2.0], v + "_min"), ([0.0, 3.0], [2.0, 2.0], v + "_min"),
                                 (None, [2.0, 2.0], v + "_min"), ([0.0, 0.0], None, v + "_max"),
                                 ([1.5, 0.0], [3.0, 2.0], v + "_s")):             # terminal constraint, u_s = (1, 1), y_s = (0.65, 0.77)
                code, msg = _code(fn, lo, hi)
                assert code == L.ERR_INVALID and word in msg, (name, lo, hi, msg)
            fn(*ok)
            eng.set_refinement("always")                                          # every refinement mode at this size
            eng.set_refinement("off")
            eng.set_box_safeguard(True)                                           # accepted, no effect beyond 271 rows
            bad = (np.array([2.5, 2.5]), np.array([0.65, 0.77])) if v == "u" else (np.array([1.0, 1.0]), np.array([0.75, 0.77]))
            code, msg = _code(eng.set_setpoints, *bad)
            assert code == L.ERR_INVALID and v + "_s" in msg
            code, msg = _code(eng.solve_from_host, d["u_d"][:2], d["y_d"][:2], up[:2], yp[:2])
            assert code == L.ERR_UNSUPPORTED and "ddmpc_solve_from_host" in msg
            # the reverse order: what would take a bounded handle off the phase kernels is refused
            code, msg = _code(eng.set_large_pipeline, "one_workgroup")
            assert code == L.ERR_UNSUPPORTED and "ONE_WORKGROUP" in msg
            code, msg = _code(eng.set_large_affine_law, True)
            assert code == L.ERR_UNSUPPORTED and "LARGE_AFFINE_LAW" in msg
            code, msg = _code(eng.debug_stamps, True)
            assert code == L.ERR_UNSUPPORTED and "ddmpc_debug_stamps" in msg
            eng.set_large_pipeline("phases")
            eng.set_large_affine_law(False)
            code, msg = _code(eng.set_large_bounds, False)                        # not under a bounded handle
            assert code == L.ERR_UNSUPPORTED and "remove the bounds" in msg
            fn(None, None)
            eng.set_large_bounds(False)
            code, msg = _code(fn, *ok)
            assert code == L.ERR_UNSUPPORTED and "271" in msg
        # a handle currently on the one-workgroup route, or with the affine law
        for prep, word in ((lambda e: e.set_large_pipeline("one_workgroup"), "DDMPC_OPT_LARGE_PIPELINE"),
                           (lambda e: e.debug_stamps(True), "ddmpc_debug_stamps"),
                           (lambda e: e.set_large_affine_law(True), "DDMPC_OPT_LARGE_AFFINE_LAW")):
            with _bounded_engine(spec, N, 2) as eng:
                prep(eng)
                code, msg = _code(getattr(eng, name), *ok)
                assert code == L.ERR_UNSUPPORTED and word in msg, msg
                getattr(eng, name)([-INF, -INF], [INF, INF])                      # all infinite: accepted anywhere
        with _bounded_engine(spec, N, 65536) as eng:
            code, msg = _code(getattr(eng, name), *ok)
            assert code == L.ERR_UNSUPPORTED and "65535" in msg
        with _bounded_engine(orc.spec_from_params(controller_type=0, L=LH), N, 2) as eng:
            code, msg = _code(getattr(eng, name), *ok)
            assert code == L.ERR_UNSUPPORTED and "ROBUST" in msg
        with _bounded_engine(orc.spec_from_params(slack_var_constraint_type=1, L=271), 1400, 2) as eng:   # 1100 rows
            code, msg = _code(getattr(eng, name), *ok)
            assert code == L.ERR_UNSUPPORTED and "1024" in msg
        dspec = orc.spec_from_params(L=LH)
        Rd = dspec.R.copy()
        Rd[0, 1] = Rd[1, 0] = 1e-5
        dspec.R = Rd
        with _bounded_engine(dspec, N, 2) as eng:
            code, msg = _code(getattr(eng, name), *ok)
            assert code == L.ERR_UNSUPPORTED and "DENSE" in msg
    # zero weights: a bounded channel with an R / Q entry of 0 on a free step; under CONVEX with output bounds a Q entry of 0 anywhere
    kw = dict(n=4, m=2, p=2, L_=LH, N=N, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002, lamb_alpha=50.0,
              lamb_sigma=1000.0, c=1.0)
    q = np.full(2 * LH, 3.0)
    q[2 * 7 + 1] = 0.0                                                            # output channel 1, free step 7
    rw = np.full(2 * LH, 1e-4)
    rw[2 * 9 + 0] = 0.0                                                           # input channel 0, free step 9
    with BatchedDDMPC(Q=q, R=1e-4, slack_type=L.SLACK_NONE, **kw) as eng:
        _opt_in(eng)
        code, msg = _code(eng.set_output_bounds, [0.60, 0.72], [0.70, 0.82])
        assert code == L.ERR_UNSUPPORTED and "Q entry" in msg
        eng.set_output_bounds([0.60, -INF], [0.70, INF])                          # the unweighted channel is not bounded: fine
    with BatchedDDMPC(Q=q, R=1e-4, slack_type=L.SLACK_CONVEX, **kw) as eng:
        _opt_in(eng)
        code, msg = _code(eng.set_output_bounds, [0.60, -INF], [0.70, INF])
        assert code == L.ERR_UNSUPPORTED and "Q entry" in msg
    with BatchedDDMPC(Q=3.0 * np.ones(2 * LH), R=rw, slack_type=L.SLACK_NONE, **kw) as eng:
        _opt_in(eng)
        code, msg = _code(eng.set_input_bounds, [0.0, -INF], [2.0, INF])
        assert code == L.ERR_UNSUPPORTED and "R entry" in msg
        eng.set_input_bounds([-INF, 0.0], [INF, 2.0])


def test_infinite_bounds_are_bit_equal_none_restores_and_the_solution_is_forgotten(gpu):
    spec, d, up, yp = _data("convex")

    def run(prep):
        with _bounded_engine(spec, N, B8) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            prep(eng)
            out = [x.copy() for x in eng.solve(up, yp)]
            eng.prepare()
            return out + [x.copy() for x in eng.step(up, yp)]

    def infinite(eng):
        eng.set_input_bounds([-INF, -INF], [INF, INF])
        eng.set_output_bounds([-INF, -INF], [INF, INF])

    def bounded_then_removed(eng):
        eng.set_input_bounds(*U_WIDE)
        eng.set_output_bounds(*Y_UP)
        u, _, st, it = eng.solve(up, yp)
        assert np.all(st == 0) and np.all(it >= 2) and np.max(u) <= 6.0 and np.min(u) >= -4.0
        eng.get_solution("ubar")
        eng.set_output_bounds(None, None)
        code, msg = _code(eng.get_solution, "ubar")                               # the call forgets the last solution
        assert code == L.ERR_NOT_READY
        eng.solve(up, yp)
        eng.set_input_bounds(None, None)
        code, msg = _code(eng.get_solution, "ubar")
        assert code == L.ERR_NOT_READY

    fresh = run(lambda eng: None)
    assert np.all(fresh[2] == 0)
    for prep in (infinite, bounded_then_removed):
        for a, b_ in zip(fresh, run(prep)):
            assert np.array_equal(a, b_)


# ------------------------------------------------------------------------------------------------ 2 - 5. against the helper
@pytest.mark.parametrize("slack", ["none", "convex"])
def test_input_bounds_on_every_channel(gpu, slack):
    """Inputs in [-4, 6]: every free input row is boxed, so n0 = 0 and the "trailing block" is the whole system.  Helper: 4 - 5
    solves, 6 - 10 active, margins >= 1.4e-3."""
    spec, d, up, yp = _data(slack)
    _compare("u-wide-" + slack, spec, lambda: _bounded_engine(spec, N, B8), d["u_d"], d["y_d"], up, yp, U_WIDE, None)


def test_input_bounds_on_one_channel_are_a_true_trailing_block(gpu):
    """Inputs of channel 0 in [-1, 3], slack NONE: 66 boxed rows behind 230 others, n0 = 192 > 0.  Helper: 5 - 6 solves, peak
    6 - 9 active, margins >= 2e-4."""
    spec, d, up, yp = _data("none")
    refs, x = _compare("u-ch0", spec, lambda: _bounded_engine(spec, N, B8), d["u_d"], d["y_d"], up, yp, U_CH0, None)
    na, nu, _ = _sections(spec, N)
    ub = x[:, na:na + nu].reshape(B8, spec.Ln, 2)[:, spec.n:spec.L]                # free steps
    assert np.min(ub[:, :, 0]) == -1.0 or np.max(ub[:, :, 0]) == 3.0


@pytest.mark.parametrize("slack", ["none", "convex"])
def test_output_bounds(gpu, slack):
    """y <= (0.66, 0.775).  Helper: 2 - 4 solves, peak 19 - 34 active, margins >= 3.5e-5.  Under slack NONE the boxed row has
    D0 = 1/q + 1/lamb_sigma and keeps 1/lamb_sigma when its output is held."""
    spec, d, up, yp = _data(slack)
    refs, x = _compare("y-up-" + slack, spec, lambda: _bounded_engine(spec, N, B8), d["u_d"], d["y_d"], up, yp, None, Y_UP)
    na, nu, ny = _sections(spec, N)
    yb = x[:, na + nu:na + nu + ny].reshape(B8, spec.Ln, 2)[:, spec.n:spec.L]
    assert np.all(yb <= np.asarray(Y_UP[1]) * (1 + 1e-12))                         # ybar within the box
    assert np.any(yb == np.asarray(Y_UP[1]))
    if slack == "convex":
        # rows with the slack AND the output active: the helper has none on these eight instances with this box (its slack
        # components stay inside +- c eps_max wherever an output is held), so the kernels' hard-row state is exercised by the
        # numpy statement of tests/test_output_bounds_reference.py and by the 136-row tests only
        both = 0
        for sol in refs.values():
            on = {int(i) for i, a in zip(sol.idx, sol.active) if a}
            both += sum(1 for i in on if na + nu <= i < na + nu + ny and i + ny in on)
        print("rows with both components active in the helper:", both)
        assert both == 0


@pytest.mark.parametrize("slack", ["none", "convex"])
def test_input_and_output_bounds_together(gpu, slack):
    """Inputs in [-4, 6] with y <= (0.66, 0.775).  Helper: 5 - 6 solves, peak 27 - 46 active, margins >= 1.5e-5."""
    spec, d, up, yp = _data(slack)
    _compare("uy-" + slack, spec, lambda: _bounded_engine(spec, N, B8), d["u_d"], d["y_d"], up, yp, U_WIDE, Y_UP)


# ------------------------------------------------------------------------------------------------ 6. the cap of 64 components
def test_more_than_64_active_components_is_a_solver_error_of_that_instance(gpu):
    """Inputs in [0, 2], CONVEX.  On the CPU (numpy restatement of the kernel's iteration) instances 1, 3, 4 peak at 67, 69, 71
    active components and the others at 46 - 58 (8 - 12 solves, margins >= 1.8e-6): the first three report solver_error with NaN
    outputs at the iteration where the set outgrew RR3_KMAX = 64, the others match the helper and do not depend on them."""
    spec, d, up, yp = _data("convex")
    over, fine = [1, 3, 4], [0, 2, 5, 6, 7]
    s, x, t = _solve_and_step(lambda: _bounded_engine(spec, N, B8), d["u_d"], d["y_d"], up, yp, U_CAP, None)
    for a, b_ in zip(s, t):
        assert np.array_equal(a, b_, equal_nan=True)
    print("status", s[2], "iters", s[3])
    assert np.all(s[2][over] == 4) and np.all(s[2][fine] == 0)                     # (status 5 never reaches the caller)
    assert np.all(np.isnan(s[0][over])) and np.all(np.isnan(s[1][over]))
    assert np.all(s[3][over] >= 2) and np.all(s[3][over] < 50)
    for b in fine:
        sol = _reference("u-cap", spec, d["u_d"], d["y_d"], up, yp, b, U_CAP, None)
        _check_against(sol, b, spec, d["u_d"], d["y_d"], s[0][b], s[1][b], s[3][b], x[b], "cap")
    s5, _, _ = _solve_and_step(lambda: _bounded_engine(spec, N, len(fine)), d["u_d"][fine], d["y_d"][fine], up[fine], yp[fine],
                               U_CAP, None)
    for a, b_ in zip(s, s5):
        assert np.array_equal(a[fine], b_)                                         # the same bits without the three neighbours


# ------------------------------------------------------------------------------------------------ 7. m != p
def test_one_bounded_output_on_a_plant_with_m_ne_p(gpu):
    """(2 + 3)(53 + 2) = 275 rows, CONVEX, y_s[0] = 1.173: channel 0 bounded below at 1.123.  Helper: 3 - 4 solves, 2 - 18
    active, margins >= 2.2e-5."""
    case = CP.make_case(2, 3, 1, 2, 53, "convex", feedthrough=False, B=4)
    spec = case["spec"]
    assert (spec.m + spec.p) * spec.Ln == 275
    ybox = ([1.123, -INF, -INF], [INF, INF, INF])
    _compare("m-ne-p", spec, lambda: _opt_in(CP.engine(case)), case["u_d"], case["y_d"], case["up"], case["yp"], None, ybox)


# ------------------------------------------------------------------------------------------------ 8. iteration cap
def test_iteration_cap(gpu):
    spec, d, up, yp = _data("convex")
    out = {}
    for cap in (3, 50):
        with _bounded_engine(spec, N, B8, max_iter=cap) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_output_bounds(*Y_UP)                # 2 - 4 solves: some instances end within a cap of 3, some do not
            out[cap] = [x.copy() for x in eng.solve(up, yp)]
    u3, c3, s3, i3 = out[3]
    u50, c50, s50, i50 = out[50]
    more = i50 > 3
    print("iters", i50, "capped", i3, s3)
    assert np.all(s50 == 0) and np.any(more) and np.any(~more)
    assert np.all(s3[more] == 4) and np.all(i3[more] == 3)
    assert np.all(s3[~more] == 0) and np.array_equal(u3[~more], u50[~more]) and np.array_equal(c3[~more], c50[~more])
    assert np.array_equal(i3[~more], i50[~more])


# ------------------------------------------------------------------------------------------------ 9. per-step closed loop
def test_per_step_closed_loop_against_the_reference_loop(gpu):
    """Inputs in [-1, 3], slack NONE, 4 steps, n_mpc_step = 1, instances 0 and 1, noise seed 5.  On the CPU every solve of both
    loops is optimal (5 - 7 solves, 9 - 22 active) with margins >= 4.3e-5: the first seed tried."""
    spec, d, up, yp = _data("none")
    Bq, n_steps = 2, 4
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (Bq, n_steps, 2))
    box = ([-1.0, -1.0], [3.0, 3.0])
    with _bounded_engine(spec, N, Bq) as eng:
        eng.set_data(d["u_d"][:Bq], d["y_d"][:Bq])
        eng.set_input_bounds(*box)
        u_sys, y_sys, st, _, _, _ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up[:Bq], yp[:Bq], w)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
    assert np.all(st == 0)
    assert np.min(u_sys) >= -1.0 and np.max(u_sys) <= 3.0
    for b in range(Bq):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        ur, yr = uref.closed_loop_bounded(spec, d["u_d"][b], d["y_d"][b], plant, w[b], box[0], box[1])
        eu, ey = np.max(np.abs(u_sys[b] - ur)) / np.max(np.abs(ur)), np.max(np.abs(y_sys[b] - yr)) / np.max(np.abs(yr))
        print("loop b=%d err_u %.1e err_y %.1e" % (b, eu, ey))
        assert eu < 1e-8 and ey < 1e-8, (b, eu, ey)


# ------------------------------------------------------------------------------------------------ 10. the Python layers
def test_controller_class_and_engine_pass_the_bounds_through(gpu):
    from direct_data_driven_mpc.direct_data_driven_mpc_controller import (
        DataDrivenMPCType, DirectDataDrivenMPCController, SlackVarConstraintTypes)
    spec, d, up, yp = _data("convex")
    cfg = harness.controller_params()
    ctrl = DirectDataDrivenMPCController(
        n=4, m=2, p=2, u_d=d["u_d"][0], y_d=d["y_d"][0], L=LH, Q=cfg["Q"] * np.eye(2 * LH), R=cfg["R"] * np.eye(2 * LH),
        u_s=cfg["u_s"].reshape(-1, 1), y_s=cfg["y_s"].reshape(-1, 1), eps_max=cfg["eps_max"], lamb_alpha=cfg["lamb_alpha"],
        lamb_sigma=cfg["lamb_sigma"], c=cfg["c"], slack_var_constraint_type=SlackVarConstraintTypes.CONVEX,
        controller_type=DataDrivenMPCType.ROBUST, n_mpc_step=cfg["n_mpc_step"])
    assert ctrl.get_problem_solve_status() == "optimal"
    u0 = ctrl.get_optimal_control_input().copy()
    assert np.max(u0) > 6.0 or np.min(u0) < -4.0                                   # the unbounded solution leaves the box
    ctrl.set_input_bounds(*U_WIDE)
    ctrl.set_output_bounds(*Y_UP)
    assert ctrl.get_problem_solve_status() == "optimal"
    u1 = ctrl.get_optimal_control_input().copy()
    sol = _reference("uy-convex", spec, d["u_d"], d["y_d"], up, yp, 0, U_WIDE, Y_UP)
    assert _rel(u1, sol.optimal_u) < TOL_U
    ctrl._engine.close()
    ctrl._engine = None
    ctrl.update_and_solve_data_driven_mpc()                                        # a new engine handle: the bounds are set again
    assert ctrl.get_problem_solve_status() == "optimal" and np.array_equal(ctrl.get_optimal_control_input(), u1)
    ctrl.set_output_bounds(None, None)
    ctrl.set_input_bounds(None, None)
    assert np.array_equal(ctrl.get_optimal_control_input(), u0)
