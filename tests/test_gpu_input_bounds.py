"""Input bounds u_min <= u <= u_max for ROBUST controllers up to 271 rows (ddmpc_set_input_bounds): the primal-dual active-set
iteration over the slack box and the bounded input rows on the affine law and M = K0^-1 E_box.  Against the full-space
reference of tests/_input_bounds_ref.py at the standard bars, ddmpc_step against ddmpc_solve on the same handle at 1e-10, the
fused closed loop against the per-step cold path."""

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

import _input_bounds_ref as ref
import test_gpu_closed_loop_plants as CP
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
INF = np.inf
B32, SEED0 = 32, 500
FUSED = "ddmpc_closed_loop_box_kernel"
NA, NU = 400 - 34 + 1, 34 * 2                           # four-tank, L = 30, n = 4, N = 400: alpha; ubar = ybar = sigma entries

# name: (slack CONVEX?, terminal constraint, u_min, u_max, k beyond the LDS home of the k x k system?)
CONFIGS = {
    "convex-tec-wide":      (1, True, [-4.0, -4.0], [6.0, 6.0], False),
    "convex-tec-tight":     (1, True, [0.0, 0.0], [2.0, 2.0], True),
    "convex-tec-one-sided": (1, True, [-INF, 0.5], [3.0, INF], None),
    "none-wide":            (0, False, [-4.0, -4.0], [6.0, 6.0], False),
    "none-tight":           (0, False, [0.0, 0.0], [2.0, 2.0], True),
    "none-one-sided":       (0, False, [-INF, 0.5], [3.0, INF], None),
}

_DATA = {}
_REF = {}


def _data():
    if not _DATA:
        d = generate_batch(range(SEED0, SEED0 + B32), N=400)
        _DATA.update(d=d, up=d["u_d"][:, -4:, :].reshape(B32, -1).copy(), yp=d["y_d"][:, -4:, :].reshape(B32, -1).copy())
    return _DATA["d"], _DATA["up"], _DATA["yp"]


def _spec(name):
    slack, tec = CONFIGS[name][:2]
    return orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)


def _reference(name, b):
    """The helper's solution of instance b at the data tail, computed once per configuration and instance."""
    if (name, b) not in _REF:
        d, up, yp = _data()
        _REF[(name, b)] = ref.solve_bounded(_spec(name), d["u_d"][b], d["y_d"][b], up[b], yp[b], *CONFIGS[name][2:4])
    return _REF[(name, b)]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _full_x(eng):
    """[alpha; ubar; ybar; sigma] of the last solve, the stacking of the full-space QP."""
    return np.concatenate([eng.get_solution(w) for w in ("alpha", "ubar", "ybar", "sigma")], axis=1)


def _signed_active(x, sol):
    """An active component sits on its bound (inputs exactly; a terminal slack is reconstructed as (y_s + bound) - y_s): within
    1e-9 of the size of its box, a hundredth of the smallest distance the margin rule leaves to an inactive one."""
    v = x[sol.idx]
    tol = 1e-9 * np.maximum(np.where(np.isfinite(sol.lo), np.abs(sol.lo), 0.0), np.where(np.isfinite(sol.hi), np.abs(sol.hi), 0.0))
    with np.errstate(invalid="ignore"):
        return (np.abs(v - sol.hi) <= tol).astype(int) - (np.abs(v - sol.lo) <= tol).astype(int)


def _free_inputs(spec, ubar):
    nfree = spec.L - spec.n if spec.tec else spec.L
    return ubar[:, spec.n * spec.m:(spec.n + nfree) * spec.m].reshape(ubar.shape[0], nfree, spec.m)


def _within(u, lo, hi):
    lo, hi = np.asarray(lo), np.asarray(hi)
    return np.all(u >= lo - 1e-12 * np.maximum(np.abs(lo), 1.0)) and np.all(u <= hi + 1e-12 * np.maximum(np.abs(hi), 1.0))


# ------------------------------------------------------------------------------------------------ 1. contract
def _code(fn, *a):
    with pytest.raises(L.DDMPCError) as e:
        fn(*a)
    return e.value.code, e.value.message


def test_refusals(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    with T._engine(spec, 400, 2) as eng:
        for lo, hi, word in (([np.nan, 0.0], [2.0, 2.0], "u_min"), ([0.0, 0.0], [2.0, np.nan], "u_max"),
                             ([0.0, 2.0], [2.0, 2.0], "u_min"), ([0.0, 3.0], [2.0, 2.0], "u_min"),
                             (None, [2.0, 2.0], "u_min"), ([0.0, 0.0], None, "u_max"),
                             ([1.5, 0.0], [3.0, 2.0], "u_s")):                   # terminal constraint, u_s = (1, 1)
            code, msg = _code(eng.set_input_bounds, lo, hi)
            assert code == L.ERR_INVALID and word in msg, (lo, hi, msg)
        eng.set_input_bounds([0.0, 0.0], [2.0, 2.0])
        code, msg = _code(eng.set_refinement, "always")
        assert code == L.ERR_UNSUPPORTED and "REFINE_ALWAYS" in msg
        code, msg = _code(eng.set_setpoints, np.array([2.5, 1.0]), np.array([0.65, 0.77]))
        assert code == L.ERR_INVALID and "u_s" in msg
        code, msg = _code(eng.solve_from_host, d["u_d"][:2], d["y_d"][:2], up[:2], yp[:2])
        assert code == L.ERR_UNSUPPORTED and "ddmpc_solve_from_host" in msg
        eng.set_convex_warm_law(True)                                            # accepted, no effect
        eng.set_convex_update(False)
    with T._engine(spec, 400, 2) as eng:
        eng.set_refinement("always")
        code, msg = _code(eng.set_input_bounds, [0.0, 0.0], [2.0, 2.0])
        assert code == L.ERR_UNSUPPORTED and "REFINE_ALWAYS" in msg
    with T._engine(orc.spec_from_params(controller_type=0), 400, 2) as eng:
        code, msg = _code(eng.set_input_bounds, [0.0, 0.0], [2.0, 2.0])
        assert code == L.ERR_UNSUPPORTED and "ROBUST" in msg
        eng.set_input_bounds([-INF, -INF], [INF, INF])                           # all infinite: accepted anywhere
    with T._engine(orc.spec_from_params(slack_var_constraint_type=1, L=64), 600, 2) as eng:      # (2 + 2)(64 + 4) = 272 rows
        code, msg = _code(eng.set_input_bounds, [0.0, 0.0], [2.0, 2.0])
        assert code == L.ERR_UNSUPPORTED and "271" in msg
    dspec = orc.spec_from_params()
    Rd = dspec.R.copy()
    Rd[0, 1] = Rd[1, 0] = 1e-5
    dspec.R = Rd
    with T._engine(dspec, 400, 2) as eng:
        code, msg = _code(eng.set_input_bounds, [0.0, 0.0], [2.0, 2.0])
        assert code == L.ERR_UNSUPPORTED and "DENSE" in msg
    r = np.full(60, 1e-4)
    r[2 * 7 + 1] = 0.0                                                           # channel 1, free step 7
    kw = dict(n=4, m=2, p=2, L_=30, N=400, Q=3.0, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002, lamb_alpha=50.0,
              lamb_sigma=1000.0, c=1.0)
    with BatchedDDMPC(R=r, **kw) as eng:
        code, msg = _code(eng.set_input_bounds, [0.0, 0.0], [2.0, 2.0])
        assert code == L.ERR_UNSUPPORTED and "R entry" in msg
        eng.set_input_bounds([0.0, -INF], [2.0, INF])                            # the unweighted channel is not bounded: fine


def test_infinite_bounds_are_bit_equal_and_none_restores(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    Bq = 8
    d, up, yp = _data()
    u_d, y_d, up, yp = d["u_d"][:Bq], d["y_d"][:Bq], up[:Bq], yp[:Bq]
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (Bq, 10, 2))

    def run(prep):
        with T._engine(spec, 400, Bq) as eng:
            eng.set_data(u_d, y_d)
            prep(eng)
            out = [x.copy() for x in eng.solve(up, yp)] + [x.copy() for x in eng.step(up, yp)]
            out += [np.asarray(x).copy() for x in eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up, yp, w)]
            return out, eng.closed_loop_kernel_name()

    def bounded_then_removed(eng):
        eng.set_input_bounds([0.0, 0.0], [2.0, 2.0])
        u, _, st, it = eng.step(up, yp)
        assert np.all(it >= 2) and np.max(u.reshape(Bq, 30, 2)[:, :26]) <= 2.0
        eng.set_input_bounds(None, None)

    fresh, k0 = run(lambda eng: None)
    for prep in (lambda eng: eng.set_input_bounds([-INF, -INF], [INF, INF]), bounded_then_removed):
        got, k1 = run(prep)
        assert k1 == k0 != FUSED
        for a, b in zip(fresh, got):
            assert np.array_equal(a, b)


def test_get_solution_not_ready_after_the_call(gpu):
    spec = orc.spec_from_params()
    d, up, yp = _data()
    with T._engine(spec, 400, 2) as eng:
        eng.set_data(d["u_d"][:2], d["y_d"][:2])
        eng.solve(up[:2], yp[:2])
        eng.get_solution("ubar")
        eng.set_input_bounds([0.0, 0.0], [2.0, 2.0])
        code, _ = _code(eng.get_solution, "ubar")
        assert code == L.ERR_NOT_READY
        eng.step(up[:2], yp[:2])
        eng.get_solution("ubar")
        eng.set_input_bounds([-INF, -INF], [INF, INF])
        code, _ = _code(eng.get_solution, "ubar")
        assert code == L.ERR_NOT_READY


# ------------------------------------------------------------------------------------------------ 2 / 3. solve and step against the reference
@pytest.mark.parametrize("name", list(CONFIGS))
def test_solve_and_step_against_the_reference(gpu, name):
    slack, tec, lo, hi, k_global = CONFIGS[name]
    spec = _spec(name)
    d, up, yp = _data()
    rows = list(range(0, B32, 4))
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_input_bounds(lo, hi)
        us, cs, ss, its = (x.copy() for x in eng.step(up, yp))
        xs = _full_x(eng)
        uc, cc, sc, itc = (x.copy() for x in eng.solve(up, yp))
        xc = _full_x(eng)
    # step against solve on all instances
    assert np.array_equal(ss, sc) and np.array_equal(its, itc) and np.all(ss == 0), (ss, sc, its, itc)
    assert _rel(us, uc) < 1e-10 and np.max(np.abs(cs - cc) / np.abs(cc)) < 1e-10
    nb = spec.n * spec.m
    for x, u in ((xs, us), (xc, uc)):
        ubar = x[:, NA:NA + NU]
        assert _rel(ubar[:, nb:], u) < 1e-12
        assert _within(_free_inputs(spec, ubar), lo, hi)
    # against the reference on every fourth instance
    left_out, ks, both = 0, [], 0
    for b in rows:
        sol = _reference(name, b)
        assert sol.status == "optimal"
        eu = np.max(np.abs(us[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(cs[b] - sol.cost) / abs(sol.cost)
        print("%s b=%d iters %d/%d k %d margin %.1e err_u %.1e err_cost %.1e" %
              (name, b, its[b], sol.iters, np.count_nonzero(sol.active), sol.margin, eu, ec))
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        if sol.margin < 1e-7:
            left_out += 1
            continue
        assert its[b] == sol.iters, (b, its[b], sol.iters)
        assert np.array_equal(_signed_active(xs[b], sol), sol.active), b
        assert np.array_equal(_signed_active(xc[b], sol), sol.active), b
        ks.append(int(np.count_nonzero(sol.active)))
        on = sol.idx[sol.active != 0]
        both += bool(np.any(on >= NA + 2 * NU) and np.any(on < NA + NU))        # a slack and an input at their bounds
        # H alpha = [ubar; ybar + sigma]
        H = orc.hankel_matrix(np.concatenate([d["u_d"][b], d["y_d"][b]], axis=1), spec.Ln)
        z = H @ xs[b, :NA]
        ub, yb, sg = (xs[b, NA + i * NU:NA + (i + 1) * NU].reshape(34, 2) for i in range(3))
        zz = np.concatenate([ub, yb + sg], axis=1).reshape(-1)
        assert np.max(np.abs(z - zz)) <= 1e-8 * np.max(np.abs(zz)), b
    assert left_out * 16 <= len(rows), left_out
    assert both >= 1 or not slack, both
    # both homes of the k x k system: LDS up to 16 active components, the instance's global slice beyond
    if k_global is False:
        assert max(ks) <= 16 and min(ks) >= 1 and np.all(its[rows] >= 2), ks
    if k_global is True:
        assert min(ks) > 16, ks


# ------------------------------------------------------------------------------------------------ 4. a second shape
def test_one_bounded_channel_on_a_plant_with_m_ne_p(gpu):
    case = CP.make_case(2, 3, 1, 2, 7, "convex", feedthrough=False, B=8, n_steps=6)          # (2 + 3)(7 + 2) = 45 rows
    spec = case["spec"]
    lo, hi = [spec.u_s[0] - 0.1, -INF], [spec.u_s[0] + 0.1, INF]                             # channel 1 is not in the box list
    with CP.engine(case) as eng:
        eng.set_data(case["u_d"], case["y_d"])
        eng.set_input_bounds(lo, hi)
        us, cs, ss, its = (x.copy() for x in eng.step(case["up"], case["yp"]))
        ubar = eng.get_solution("ubar")
        uc, cc, sc, itc = (x.copy() for x in eng.solve(case["up"], case["yp"]))
    assert np.array_equal(ss, sc) and np.array_equal(its, itc) and np.all(ss == 0)
    assert _rel(us, uc) < 1e-10 and np.max(np.abs(cs - cc) / np.abs(cc)) < 1e-10
    free = _free_inputs(spec, ubar)
    assert _within(free[:, :, 0], lo[0], hi[0]) and np.max(free[:, :, 1]) > 0.9                # channel 1 roams (0.98 .. 2.7 unbounded)
    hit = 0
    for b in range(8):
        sol = ref.solve_bounded(spec, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], lo, hi)
        assert sol.status == "optimal" and sol.margin >= 1e-7
        assert np.max(np.abs(us[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U, b
        assert abs(cs[b] - sol.cost) / abs(sol.cost) < TOL_COST, b
        assert its[b] == sol.iters
        hit += int(np.any(free[b, :, 0] == hi[0]))
    assert hit >= 4


# ------------------------------------------------------------------------------------------------ 5. iteration cap
def test_iteration_cap(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    lo, hi = [0.8, 0.8], [1.2, 1.2]                     # u_s +- 0.2: tight enough to make the rule cycle on some instances
    out = {}
    for cap in (3, 50):
        with T._engine(spec, 400, B32, max_iter=cap) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_input_bounds(lo, hi)
            out[cap] = [x.copy() for x in eng.step(up, yp)] + [x.copy() for x in eng.solve(up, yp)]
    u3, c3, s3, i3, uc3, cc3, sc3, ic3 = out[3]
    u50, c50, s50, i50 = out[50][:4]
    assert np.array_equal(s3, sc3) and np.array_equal(i3, ic3)
    more = (i50 > 3) | (s50 == 4)
    assert np.any(more) and np.all(s3[more] == 4) and np.all(i3[more] == 3)
    assert np.all(s3[~more] == 0) and np.array_equal(u3[~more], u50[~more]) and np.array_equal(c3[~more], c50[~more])
    assert np.array_equal(i3[~more], i50[~more])
    assert _rel(u3[~more], uc3[~more]) < 1e-10 if np.any(~more) else True


# ------------------------------------------------------------------------------------------------ 6. no read of the trajectories after prepare
def test_no_read_of_the_trajectories_after_prepare(gpu):
    torch = pytest.importorskip("torch")
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(3).uniform(-1.0, 1.0, (B32, 12, 2))
    ut = torch.tensor(d["u_d"], device="cuda:0")
    yt = torch.tensor(d["y_d"], device="cuda:0")
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(ut, yt)
        eng.set_input_bounds([-4.0, -4.0], [6.0, 6.0])
        eng.prepare()
        s0 = [x.copy() for x in eng.step(up, yp)]
        cl0 = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w)
        assert eng.closed_loop_kernel_name() == FUSED
        torch.cuda.synchronize()
        ut.fill_(float("nan"))
        yt.fill_(float("nan"))
        torch.cuda.synchronize()
        s1 = [x.copy() for x in eng.step(up, yp)]
        cl1 = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w)
    assert np.all(s0[3] >= 2) and np.all(s0[2] == 0) and np.all(np.isfinite(s1[0]))
    for a, b in zip(s0 + list(cl0), s1 + list(cl1)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 7. closed loop
@pytest.mark.parametrize("n_mpc_step", [1, 2])
def test_fused_closed_loop_against_the_cold_path(gpu, n_mpc_step):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    lo, hi = [-4.0, -4.0], [6.0, 6.0]
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B32, 20, 2))
    out = {}
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_input_bounds(lo, hi)
        eng.set_closed_loop_path("cold")
        out["cold"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        ub_cold = eng.get_solution("ubar")
        eng.set_closed_loop_path("auto")
        out["fused"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == FUSED
        ub = eng.get_solution("ubar")
    for a, b in zip(out["cold"], out["fused"]):
        assert np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))) < 1e-9
    assert np.array_equal(out["cold"][2], out["fused"][2]) and np.all(out["fused"][2] == 0)
    assert _within(out["fused"][0], lo, hi) and _within(out["cold"][0], lo, hi)
    assert np.max(out["fused"][0]) == 6.0                               # the bound is met along the way
    assert np.max(np.abs(ub - ub_cold)) < 1e-9 and _within(_free_inputs(spec, ub), lo, hi)


def test_closed_loop_against_a_loop_driven_by_the_reference(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    Bq, n_steps = 2, 6
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B32, 20, 2))[:Bq, :n_steps]
    with T._engine(spec, 400, Bq) as eng:
        eng.set_data(d["u_d"][:Bq], d["y_d"][:Bq])
        eng.set_input_bounds(0.0, 2.0)
        u_sys, y_sys, st, _, _, _ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up[:Bq], yp[:Bq], w)
        assert eng.closed_loop_kernel_name() == FUSED
    assert np.all(st == 0) and _within(u_sys, 0.0, 2.0)
    for b in range(Bq):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        ur, yr = ref.closed_loop_bounded(spec, d["u_d"][b], d["y_d"][b], plant, w[b], 0.0, 2.0)
        assert np.max(np.abs(u_sys[b] - ur)) / np.max(np.abs(ur)) < TOL_U, b
        assert np.max(np.abs(y_sys[b] - yr)) / np.max(np.abs(yr)) < TOL_U, b


# ------------------------------------------------------------------------------------------------ 8. refinement
def test_laws_from_refining_solves_report_inaccurate_with_an_active_set(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = _data()
    lo, hi = [-4.0, -4.0], [6.0, 6.0]
    rng = np.random.default_rng(7)
    up, yp = up.copy(), yp.copy()
    half = B32 // 2                                     # second half: windows near the setpoint, inside both boxes
    up[half:] = np.tile(spec.u_s, 4)[None] + 0.01 * rng.uniform(-1, 1, up[half:].shape)
    yp[half:] = np.tile(spec.y_s, 4)[None] + 0.002 * rng.uniform(-1, 1, yp[half:].shape)
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_input_bounds(lo, hi)
        L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_REFINE_RES_LOG10, 3000))      # AUTO flags every instance
        us, cs, ss, its = (x.copy() for x in eng.step(up, yp))
        x = _full_x(eng)
        uc, cc, sc, itc = (x_.copy() for x_ in eng.solve(up, yp))
    assert np.array_equal(ss, sc) and np.array_equal(its, itc)
    free = _free_inputs(spec, x[:, NA:NA + NU])
    sg = x[:, NA + 2 * NU + 8:]
    bound = spec.c * spec.eps_max
    nact = np.sum((free == 6.0) | (free == -4.0), axis=(1, 2)) + np.sum(np.abs(np.abs(sg) - bound) <= 1e-9 * bound, axis=1)
    assert np.array_equal(ss, np.where(nact > 0, 1, 0)), (ss, nact)
    assert np.any(ss == 1) and np.any(ss == 0)
    assert np.array_equal(its == 1, nact == 0)
    for b in (0, 4, half, half + 4):
        sol = ref.solve_bounded(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], lo, hi)
        assert sol.status == "optimal" and (np.count_nonzero(sol.active) > 0) == (ss[b] == 1)
        assert np.max(np.abs(us[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U, b
