"""DDMPC_OPT_LARGE_SETPOINTS: per-instance, per-step setpoints beyond 271 rows (Route::RobustPhases) -- ddmpc_step_setpoints and
ddmpc_closed_loop_setpoints on the kept factors (rr3_solve_kernel with the Rr3Setpoint argument, ddmpc_rr3.hpp) and, with
DDMPC_OPT_LARGE_AFFINE_LAW, on the law extended by S (rr3_setpoint_law_step_kernel, ddmpc_rr3_law.hpp); DESIGN.md 9e.

References: the full-space oracle at the instance's setpoints and ref.schedule_loop.  Bars are the project's own: inputs 1e-8,
cost 1e-9, outputs 1e-9 (TOL_U / TOL_COST / TOL_Y); law against the kept-factor step REL = 1e-9, unrefined REL_OFF = 1e-7
(test_gpu_large_robust_law.py).  No instance is left out of a comparison.

Shapes: four-tank L = 64 (272 rows: the first size past the boundary, last 64-block of 16 rows) and L = 70 (296 rows) at
N = 700, slack NONE and CONVEX with c = 0.05 (the box binds); the five-channel 300-row case (m != p: the rho % (m+p) channel
map); the 8 x 8-channel 608-row size at batch 8.  Setpoints u_s +- 0.5, y_s +- 0.2 per instance (rng(11)), +- 0.3 on the
five-channel case.

The 608-row CONVEX case and the stated limit.  With the terminal constraint a setpoint that is no equilibrium of the plant
binds the terminal slacks: at 608 rows the oracle ends with 66 .. 88 slack components at the bound on all eight instances at
u_s +- 0.5, y_s +- 0.2 (57 .. 65 at a tenth of that spread; computed on a CPU from the oracle alone).  More than 64 is the stated
limit of the two calls (solver_error; the fall-back kernel knows the shared setpoints only), so at that case every instance
whose oracle set exceeds 64 must report solver_error and every other one must meet the bars -- the rule of the limit test,
decided per instance from the oracle.  The case "608-eq" adds what that one cannot show: per-instance setpoints that are
equilibria (a_b (u_s, y_s), a_b in [0.5, 1.5]), where the sets stay small and every instance is compared at the bars.
"""
import functools

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _setpoint_law_ref as ref
import test_gpu_closed_loop_plants as plants
from test_gpu_large_robust_law import _cfg5_robust
from test_gpu_round5 import _four_tank_long, _spec_engine

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST, TOL_Y = 1e-8, 1e-9, 1e-9
REL, REL_OFF = 1e-9, 1e-7
KMAX = 64                                   # slack components switched at once that the setpoint calls hold (the stated limit)
SOL = ("alpha", "ubar", "ybar", "sigma")


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _setpoints(spec, B, du=0.5, dy=0.2, seed=11):
    rng = np.random.default_rng(seed)
    return spec.u_s + rng.uniform(-du, du, (B, spec.m)), spec.y_s + rng.uniform(-dy, dy, (B, spec.p))


@functools.lru_cache(maxsize=None)
def _case(rows, slack, c_box=0.05):
    """dict(spec, N, B, u_d, y_d, up, yp, us, ys) of a shape; built once and never written to."""
    if rows in ("272", "296"):
        B, N = 6, 700
        spec, d, up, yp = _four_tank_long(B, 64 if rows == "272" else 70, N, slack, c_box if slack == "convex" else 1.0)
        us, ys = _setpoints(spec, B)
        extra = dict(plant=dict(orc.FOUR_TANK), x0=d["x_end"].copy())
    elif rows == "300":
        g = plants.LARGE
        c = plants.make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], slack, B=4, n_steps=6)
        spec, N, B, d, up, yp = c["spec"], c["N"], 4, c, c["up"], c["yp"]
        us, ys = _setpoints(spec, B, 0.3, 0.3)
        extra = dict(plant=c["plant"], x0=c["x0"])
    else:
        B = 8
        spec, N, d, up, yp = _cfg5_robust(B, slack)
        if rows == "608-eq":
            a = np.random.default_rng(11).uniform(0.5, 1.5, B)
            us, ys = a[:, None] * spec.u_s[None, :], a[:, None] * spec.y_s[None, :]
        else:
            us, ys = _setpoints(spec, B)
        extra = {}
    r = (spec.m + spec.p) * (spec.L + spec.n)
    assert r == int(rows[:3])
    return dict(spec=spec, N=N, B=B, u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, us=us, ys=ys, **extra)


@functools.lru_cache(maxsize=None)
def _oracle(rows, slack, c_box=0.05):
    c = _case(rows, slack, c_box)
    return [orc.solve_fullspace(ref.with_setpoints(c["spec"], c["us"][b], c["ys"][b]), c["u_d"][b], c["y_d"][b], c["up"][b], c["yp"][b])
            for b in range(c["B"])]


def _engine(c, law=False, refine=None, option=True):
    eng = _spec_engine(c["spec"], c["N"], c["B"])
    if refine is not None:
        eng.set_refinement(refine)
    if law:
        eng.set_large_affine_law(True)
    if option:
        eng.set_large_setpoints(True)
    eng.set_data(c["u_d"], c["y_d"])
    return eng


def _copy(t):
    return tuple(x.copy() for x in t)


def _equal(a, b, rows=None):
    sel = slice(None) if rows is None else rows
    return all(np.array_equal(x[sel], y[sel], equal_nan=True) for x, y in zip(a, b))


def _refused(fn, code, word):
    with pytest.raises(L.DDMPCError) as e:
        fn()
    assert e.value.code == code and word in e.value.message, (e.value.code, e.value.message)


def _check_oracle(c, sols, out, tag, crowded=False):
    """Every instance: identical status and iteration count, inputs and cost at the bars.  crowded (the 608-row size alone, see
    the module docstring): where the oracle's final set exceeds the stated limit of 64 switched components, solver_error
    instead; at every other shape the oracle's sets must stay within 64, so that no instance can leave the comparison."""
    u, cost, status, iters = out
    for b, sol in enumerate(sols):
        assert sol.status == "optimal", (tag, b)
        nact = int(np.sum(sol.active != 0)) if sol.active is not None else 0
        assert crowded or nact <= KMAX, (tag, b, nact)
        if nact > KMAX:
            print("%s b=%d oracle set %d > %d: status %d" % (tag, b, nact, KMAX, status[b]))
            assert status[b] == 4, (tag, b, nact)
            continue
        eu, ec = _rel(u[b], sol.optimal_u), abs(cost[b] - sol.cost) / abs(sol.cost)
        print("%s b=%d status %d iters %d (oracle %d, set %d) eu %.2e ec %.2e" % (tag, b, status[b], iters[b], sol.iters, nact, eu, ec))
        assert status[b] == 0 and iters[b] == max(sol.iters, 1), (tag, b)
        assert eu < TOL_U and ec < TOL_COST, (tag, b, eu, ec)


# ------------------------------------------------------------------------------------------------------ 1. option contract
def test_option_contract(gpu):
    from direct_data_driven_mpc_amd.engine import BatchedDDMPC
    base = dict(n=4, m=2, p=2, L_=70, N=700, Q=3.0, R=1e-4, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002,
                lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0)
    dense_q = 3.0 * np.eye(140) + 0.1 * (np.eye(140, k=1) + np.eye(140, k=-1))
    refusals = [
        (dict(controller_type=L.NOMINAL), "NOMINAL"),
        (dict(Q=dense_q), "DDMPC_WEIGHT_DENSE"),
        (dict(L_=30, N=400), "DDMPC_OPT_SETPOINT_LAW"),                # 136 rows: the message points to options 18 - 20
        (dict(L_=63), "DDMPC_OPT_SETPOINT_CONVEX_LAW"),                # 268 rows
        (dict(L_=271, N=1400, batch=1), "1024"),                       # 1100 rows
        (dict(m=17, p=17, n=8, L_=16, N=600, u_s=np.zeros(17), y_s=np.zeros(17)), "n*(m+p)"),      # n (m + p) = 272, 816 rows
    ]
    for slack in (L.SLACK_NONE, L.SLACK_CONVEX):
        for over, word in refusals:
            with BatchedDDMPC(**{**base, "slack_type": slack, **over}) as eng:
                _refused(lambda: eng.set_large_setpoints(True), L.ERR_UNSUPPORTED, word)
                eng.set_large_setpoints(False)                         # 0 is accepted everywhere
    lib = L.load()
    with BatchedDDMPC(**base) as eng:                                  # not on the phase kernels: pipeline, stamps
        eng.set_large_pipeline("one_workgroup")
        _refused(lambda: eng.set_large_setpoints(True), L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_PIPELINE")
        eng.set_large_pipeline("phases")
        eng.debug_stamps(True)
        _refused(lambda: eng.set_large_setpoints(True), L.ERR_UNSUPPORTED, "ddmpc_debug_stamps")
        eng.debug_stamps(False)
        eng.set_large_setpoints(True)
        _refused(lambda: eng.set_large_pipeline("one_workgroup"), L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        _refused(lambda: eng.debug_stamps(True), L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        assert lib.ddmpc_set_option(eng._h, L.OPT_LARGE_SETPOINTS, 2) == L.ERR_INVALID
        assert lib.ddmpc_set_option(eng._h, L.OPT_LARGE_SETPOINTS, -1) == L.ERR_INVALID
    with BatchedDDMPC(**{**base, "batch": 65536}) as eng:              # (no data: nothing of this size is allocated)
        _refused(lambda: eng.set_large_setpoints(True), L.ERR_UNSUPPORTED, "65535")
    for bounds in ("input", "output"):
        setb = (lambda e: e.set_input_bounds(0.0, 2.0)) if bounds == "input" else (lambda e: e.set_output_bounds(0.0, 2.0))
        with BatchedDDMPC(**base) as eng:                              # bounds first, then the option
            eng.set_large_bounds(True)
            setb(eng)
            _refused(lambda: eng.set_large_setpoints(True), L.ERR_UNSUPPORTED, "bounds")
        with BatchedDDMPC(**base) as eng:                              # the option first, then the bounds
            eng.set_large_bounds(True)
            eng.set_large_setpoints(True)
            _refused(lambda: setb(eng), L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
    # options 18 - 20 keep their refusals at this size
    with BatchedDDMPC(**base) as eng:
        _refused(lambda: eng.set_setpoint_law(True), L.ERR_UNSUPPORTED, "271")
        _refused(lambda: eng.set_setpoint_box_law(True), L.ERR_UNSUPPORTED, "271")
    c = _case("296", "none")
    pl = c["plant"]
    w = np.zeros((c["B"], 3, 2))
    sched = (np.repeat(c["us"][:, None], 3, axis=1), np.repeat(c["ys"][:, None], 3, axis=1))
    with _engine(c, option=False) as eng:                              # the three calls with the option off
        loop = lambda: eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], c["x0"], c["up"], c["yp"], w, *sched)
        _refused(lambda: eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]), L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        _refused(loop, L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        _refused(eng.setpoint_gain, L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        _refused(eng.setpoint_gain, L.ERR_UNSUPPORTED, "needs DDMPC_OPT_SETPOINT_LAW = 1")       # (the present words stay)
    with _spec_engine(c["spec"], c["N"], c["B"]) as eng:               # option on, no data yet
        eng.set_large_setpoints(True)
        _refused(lambda: eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]), L.ERR_NOT_READY, "ddmpc_set_data")
    with _engine(c) as eng:
        eng.prepare()
        _refused(eng.setpoint_gain, L.ERR_NOT_READY, "DDMPC_OPT_LARGE_AFFINE_LAW")                # no law: no S
        out = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
        assert np.all(out[2] == 0)
        _refused(lambda: eng.get_solution("alpha"), L.ERR_NOT_READY, "ddmpc_step_setpoints")
        eng.step(c["up"], c["yp"])
        assert eng.get_solution("alpha").shape[0] == c["B"]
        loop = lambda: eng.closed_loop_setpoints(pl["A"], pl["B"], pl["C"], pl["D"], c["x0"], c["up"], c["yp"], w, *sched)
        loop()
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        _refused(lambda: eng.get_solution("alpha"), L.ERR_NOT_READY, "ddmpc_closed_loop_setpoints")
        eng.solve(c["up"], c["yp"])
        assert eng.get_solution("ubar").shape[0] == c["B"]
    with _engine(c, law=True) as eng:                                  # changing the value forgets the preparation
        eng.prepare()
        assert eng.setpoint_gain().shape == (c["B"], 4, 296)
        eng.set_large_setpoints(False)
        eng.set_large_setpoints(True)
        _refused(eng.setpoint_gain, L.ERR_NOT_READY, "DDMPC_OPT_LARGE_AFFINE_LAW")


# ------------------------------------------------------------------------------------- 2. the existing calls stay bit-equal
@pytest.mark.parametrize("law", [False, True], ids=["factors", "law"])
@pytest.mark.parametrize("slack", ["none", "convex"])
def test_existing_calls_bit_equal_with_the_option_on(gpu, slack, law):
    c = _case("296", slack)
    pl = c["plant"]
    w = 0.002 * np.random.default_rng(3).uniform(-1.0, 1.0, (c["B"], 4, 2))
    res = {}
    for on in (False, True):
        with _engine(c, law=law, option=on) as eng:
            eng.prepare()
            out = [_copy(eng.solve(c["up"], c["yp"]))]
            out.append(tuple(eng.get_solution(x) for x in SOL))
            out.append(_copy(eng.step(c["up"], c["yp"])))
            out.append(tuple(eng.get_solution(x) for x in SOL))
            if law:
                out.append((eng.gain(),))
            out.append(_copy(eng.closed_loop(pl["A"], pl["B"], pl["C"], pl["D"], c["x0"], c["up"], c["yp"], w)))
            out.append(tuple(eng.get_solution(x) for x in SOL))
            res[on] = out
    assert len(res[False]) == len(res[True])
    for k, (a, b_) in enumerate(zip(res[False], res[True])):
        assert _equal(a, b_), k
    assert np.all(res[True][0][2] == 0)


# ------------------------------------------------------------------------------------- 3. kept-factor step: derived equalities
@pytest.mark.parametrize("refine", ["off", "auto", "always"])
@pytest.mark.parametrize("slack", ["none", "convex"])
@pytest.mark.parametrize("rows", ["272", "296", "300"])
def test_kept_factor_step_bit_equalities(gpu, rows, slack, refine):
    c = _case(rows, slack)
    spec, B = c["spec"], c["B"]
    with _engine(c, refine=refine) as eng:
        eng.prepare()
        own = _copy(eng.step(c["up"], c["yp"]))
        same = _copy(eng.step_setpoints(c["up"], c["yp"], np.tile(spec.u_s, (B, 1)), np.tile(spec.y_s, (B, 1))))
        assert _equal(own, same)                                       # every instance at the handle's own setpoint: ddmpc_step
        assert np.all(own[2] == 0)
        mixed = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
        assert not np.array_equal(mixed[0], own[0])
        for b in range(B):                                             # the only way to move a shared setpoint, instance by instance
            eng.set_setpoints(c["us"][b], c["ys"][b])
            eng.prepare()
            one = _copy(eng.step(c["up"], c["yp"]))
            assert _equal(one, mixed, rows=slice(b, b + 1)), b
        if slack == "convex":
            print("rows %s refine %s iters %s" % (rows, refine, mixed[3]))


# ------------------------------------------------------------------------------------------------- 4. against the oracle
@pytest.mark.parametrize("slack", ["none", "convex"])
@pytest.mark.parametrize("rows", ["272", "296", "300", "608", "608-eq"])
def test_kept_factor_step_matches_oracle(gpu, rows, slack):
    c = _case(rows, slack)
    with _engine(c) as eng:
        out = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))            # (prepares)
    _check_oracle(c, _oracle(rows, slack), out, "%s/%s" % (rows, slack), crowded=rows == "608")


# ------------------------------------------------------------------------------------------------------- 5. the law with S
def test_setpoint_gain_is_the_law_of_beta_in_component_order(gpu):
    c = _case("296", "none")
    spec, B = c["spec"], c["B"]
    with _engine(c, law=True) as eng:
        eng.prepare()
        g, S = eng.gain(), eng.setpoint_gain()
        assert S.shape == (B, 4, 296)
        w =np.concatenate([c["up"], c["yp"]], axis=1)
        s = np.concatenate([c["us"], c["ys"]], axis=1)
        for b in range(B):
            eng.set_setpoints(c["us"][b], c["ys"][b])
            eng.solve(c["up"], c["yp"])
            al = eng.get_solution("alpha")[b]
            H = orc.hankel_matrix(np.concatenate([c["u_d"][b], c["y_d"][b]], axis=1), spec.L + spec.n)
            beta = g[b, 1:].T @ w[b] + S[b].T @ s[b]
            e = _rel(H.T @ beta, al)
            print("b=%d |H'beta - alpha| / |alpha| = %.2e" % (b, e))
            assert e <= REL, b


def _law_vs_factors(c, refine):
    with _engine(c, refine=refine) as eng:
        kept = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
    with _engine(c, law=True, refine=refine) as eng:
        eng.prepare()
        eng.setpoint_gain()                                            # S is there: the law route is the one that runs
        law = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
    return kept, law


def _check_law_step(c, kept, law, bar, tag):
    """Every instance: bit-equal to the kept-factor setpoint step (re-solved) or within `bar` of it (served).  -> served mask"""
    B = c["B"]
    served = np.zeros(B, dtype=bool)
    assert np.array_equal(kept[2], law[2]) and np.array_equal(kept[3], law[3]), tag
    for b in range(B):
        if _equal(kept, law, rows=slice(b, b + 1)):
            continue
        served[b] = True
        eu, ec = _rel(law[0][b], kept[0][b]), abs(law[1][b] - kept[1][b]) / abs(kept[1][b])
        print("%s b=%d served: eu %.2e ec %.2e" % (tag, b, eu, ec))
        assert law[3][b] == 1 and eu <= bar and ec <= bar, (tag, b, eu, ec)
    print("%s served fraction %.2f" % (tag, served.mean()))
    return served


@pytest.mark.parametrize("refine", ["off", "auto"])
@pytest.mark.parametrize("slack,c_box", [("none", 1.0), ("convex", 0.05), ("convex", 1.0)])     # (c = 1.0: a mostly empty set, the law serves under the box)
def test_law_step_at_296_rows(gpu, slack, c_box, refine):
    c = _case("296", slack, c_box)
    kept, law = _law_vs_factors(c, refine)
    served = _check_law_step(c, kept, law, REL_OFF if refine == "off" else REL, "296/%s-%g/%s" % (slack, c_box, refine))
    inside = kept[3] == 1                                              # (CONVEX: an instance that leaves the box is re-solved, bit-equal)
    assert not np.any(served & ~inside)
    if refine == "off":
        assert np.all(served[inside]), served                         # a sound factor and inside the box: the law serves
        if slack == "none":
            assert np.all(served)
    else:
        _check_oracle(c, _oracle("296", slack, c_box), law, "296/%s-%g/auto/law" % (slack, c_box))


@pytest.mark.parametrize("refine", ["off", "auto"])
def test_law_step_at_608_rows(gpu, refine):
    c = _case("608", "none")
    kept, law = _law_vs_factors(c, refine)
    served = _check_law_step(c, kept, law, REL_OFF if refine == "off" else REL, "608/none/%s" % refine)
    if refine == "off":
        assert np.all(served)


# ------------------------------------------------------------------------------------------------------------ 6. isolation
@pytest.mark.parametrize("law", [False, True], ids=["factors", "law"])
@pytest.mark.parametrize("slack", ["none", "convex"])
def test_nan_setpoint_is_that_instance_alone(gpu, slack, law):
    c = _case("296", slack)
    bad = 2
    rest = np.arange(c["B"]) != bad
    with _engine(c, law=law) as eng:
        good = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
        for k, v in (("u", np.nan), ("y", np.nan), ("y", np.inf)):
            us, ys = c["us"].copy(), c["ys"].copy()
            (us if k == "u" else ys)[bad, 1] = v
            out = _copy(eng.step_setpoints(c["up"], c["yp"], us, ys))
            assert out[2][bad] == 4, (k, v, out[2])
            assert _equal(good, out, rows=rest), (k, v)


# ---------------------------------------------------------------------------------------------------------------- 7. limit
def test_more_than_64_switched_components_is_solver_error(gpu):
    B, N = 6, 700
    spec, d, up, yp = _four_tank_long(B, 70, N, "convex", c_box=0.01)
    sp = [_setpoints(spec, 1, seed=11 + b) for b in range(B)]
    us, ys = np.concatenate([s[0] for s in sp]), np.concatenate([s[1] for s in sp])
    over = []
    for b in range(B):
        sol = orc.solve_fullspace(ref.with_setpoints(spec, us[b], ys[b]), d["u_d"][b], d["y_d"][b], up[b], yp[b])
        over.append(sol.status == "optimal" and int(np.sum(sol.active != 0)) > KMAX)
    assert all(over)                                                   # (tests/test_large_setpoints_reference.py: 77 .. 103)
    with _spec_engine(spec, N, B) as eng:
        eng.set_large_setpoints(True)
        eng.set_data(d["u_d"], d["y_d"])
        out = _copy(eng.step_setpoints(up, yp, us, ys))
        assert np.all(out[2] == 4), out[2]
        own = _copy(eng.step(up, yp))                                  # the same handle's step still goes through the fall-back
        assert np.all(own[2] == 0), own[2]


# ---------------------------------------------------------------------------------------------------------- 8. closed loop
def _schedule(c, n_steps, seed=5):
    """A setpoint per instance and step: the instance's own (u_s +- spread) with a step change half-way."""
    rng = np.random.default_rng(seed)
    spec, B = c["spec"], c["B"]
    us2 = c["us"] + rng.uniform(-0.1, 0.1, c["us"].shape)
    ys2 = c["ys"] + rng.uniform(-0.05, 0.05, c["ys"].shape)
    u_ref = np.empty((B, n_steps, spec.m)); y_ref = np.empty((B, n_steps, spec.p))
    h = n_steps // 2
    u_ref[:, :h], u_ref[:, h:] = c["us"][:, None], us2[:, None]
    y_ref[:, :h], y_ref[:, h:] = c["ys"][:, None], ys2[:, None]
    return u_ref, y_ref


@functools.lru_cache(maxsize=None)
def _loop_reference(rows, slack, nms, n_steps=6):
    c = _case(rows, slack, 1.0)
    pl = c["plant"]
    u_ref, y_ref = _schedule(c, n_steps)
    w = _loop_noise(c, n_steps)
    out = []
    for b in range(c["B"]):
        plant = orc.Plant(pl["A"], pl["B"], pl["C"], pl["D"], pl["eps_max"])
        plant.x = c["x0"][b].copy()
        out.append(ref.schedule_loop(c["spec"], c["u_d"][b], c["y_d"][b], plant, w[b], u_ref[b], y_ref[b], n_mpc_step=nms,
                                     u_past=c["up"][b], y_past=c["yp"][b]))
    return out


def _loop_noise(c, n_steps):
    return 0.002 * np.random.default_rng(3).uniform(-1.0, 1.0, (c["B"], n_steps, c["spec"].p))


@pytest.mark.parametrize("law", [False, True], ids=["factors", "law"])
@pytest.mark.parametrize("nms", [1, 2])
@pytest.mark.parametrize("rows,slack", [("296", "none"), ("300", "convex")])
def test_closed_loop_setpoints(gpu, rows, slack, nms, law):
    n_steps = 6
    c = _case(rows, slack, 1.0)
    spec, B, pl = c["spec"], c["B"], c["plant"]
    u_ref, y_ref = _schedule(c, n_steps)
    w = _loop_noise(c, n_steps)
    args = (pl["A"], pl["B"], pl["C"], pl["D"], c["x0"], c["up"], c["yp"], w)
    with _engine(c, law=law) as eng:
        out = eng.closed_loop_setpoints(*args, u_ref, y_ref, n_mpc_step=nms)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        assert np.all(out[2] == 0)
        for b, (u_o, y_o, up_o, yp_o) in enumerate(_loop_reference(rows, slack, nms)):
            eu = np.max(np.abs(out[0][b] - u_o)) / np.max(np.abs(u_o))
            ey = np.max(np.abs(out[1][b] - y_o)) / max(1.0, np.max(np.abs(y_o)))
            print("%s/%s nms %d law %d b=%d eu %.2e ey %.2e" % (rows, slack, nms, law, b, eu, ey))
            assert eu < TOL_U and ey < TOL_Y, (b, eu, ey)
            assert np.max(np.abs(out[4][b] - up_o)) <= TOL_U * np.max(np.abs(u_o))
            assert np.max(np.abs(out[5][b] - yp_o)) <= TOL_Y * max(1.0, np.max(np.abs(y_o)))
        if not law:
            # a constant schedule at the handle's setpoints: ddmpc_closed_loop on the prepared per-step path, bit for bit
            const = eng.closed_loop_setpoints(*args, np.tile(spec.u_s, (B, n_steps, 1)), np.tile(spec.y_s, (B, n_steps, 1)), n_mpc_step=nms)
            plain = eng.closed_loop(*args, n_mpc_step=nms)
            assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
            assert _equal(const, plain)
        # an instance whose setpoint is not finite at a later solve stops there: NaN rows from that solve on, status 4
        bad, t_bad = 1, 2 * nms
        u_nan = u_ref.copy()
        u_nan[bad, t_bad, 0] = np.nan
        stop = eng.closed_loop_setpoints(*args, u_nan, y_ref, n_mpc_step=nms)
        rest = np.arange(B) != bad
        assert stop[2][bad] == 4 and np.all(stop[2][rest] == 0)
        assert np.array_equal(stop[0][bad, :t_bad], out[0][bad, :t_bad]) and np.array_equal(stop[1][bad, :t_bad], out[1][bad, :t_bad])
        assert np.all(np.isnan(stop[0][bad, t_bad:])) and np.all(np.isnan(stop[1][bad, t_bad:]))
        assert _equal(tuple(x[rest] for x in stop), tuple(x[rest] for x in out))


# --------------------------------------------------------------------------------------------------------- 9. invalidation
def test_invalidation_drops_s_with_the_law(gpu):
    c = _case("296", "none")
    d2 = harness.generate_batch(range(100, 100 + c["B"]), N=c["N"])
    not_ready = lambda eng: _refused(eng.setpoint_gain, L.ERR_NOT_READY, "DDMPC_OPT_LARGE_AFFINE_LAW")
    with _engine(c, law=True) as eng:
        eng.prepare()
        S0 = eng.setpoint_gain()
        eng.set_data(d2["u_d"], d2["y_d"])
        not_ready(eng)
        t1 = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))             # rebuilds
        S1 = eng.setpoint_gain()
        assert not np.allclose(S1, S0) and np.all(t1[2] == 0)
        L.check(L.load().ddmpc_set_option(eng._h, L.OPT_REFINE_MAX, 2))
        not_ready(eng)
        t2 = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
        assert _rel(t2[0], t1[0]) <= REL and eng.setpoint_gain().shape == S0.shape
        eng.set_large_affine_law(False)
        not_ready(eng)
        t3 = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))             # on the kept factors
        not_ready(eng)
        assert _rel(t3[0], t1[0]) <= REL
        eng.set_large_affine_law(True)
        eng.prepare()
        assert eng.setpoint_gain().shape == S0.shape
        eng.set_large_setpoints(False)
        _refused(eng.setpoint_gain, L.ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_SETPOINTS")
        eng.set_large_setpoints(True)
        not_ready(eng)
        t4 = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
        assert np.array_equal(t4[2], t2[2]) and _rel(t4[0], t2[0]) <= REL and eng.setpoint_gain().shape == S0.shape
