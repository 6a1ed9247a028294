"""Warm control steps under the CONVEX slack box without cold re-solves (DDMPC_OPT_CONVEX_WARM_LAW): ddmpc_prepare forms
M = K0^-1 E_box next to the affine law, and ddmpc_step / ddmpc_closed_loop run the whole active-set iteration on the two.
Parity against ddmpc_solve on the same handle (same iterations and status, 1e-10) and against the full-space oracle at the
standard bars."""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9


def _windows(spec, up, yp, family, rng):
    """data tail (most instances leave the box), near the setpoint (mostly inside), random."""
    n = spec.n
    if family == "tail":
        return up, yp
    if family == "setpoint":
        return (np.tile(spec.u_s, n)[None] + 0.01 * rng.uniform(-1, 1, up.shape),
                np.tile(spec.y_s, n)[None] + 0.002 * rng.uniform(-1, 1, yp.shape))
    return rng.uniform(-1.0, 1.0, up.shape), rng.uniform(0.0, 1.0, yp.shape)


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _step_vs_solve(eng, spec, up, yp, tol=1e-10):
    uw, cw, sw, iw = (x.copy() for x in eng.step(up, yp))
    sg = eng.get_solution("sigma")
    uc, cc, sc, ic = (x.copy() for x in eng.solve(up, yp))
    sgc = eng.get_solution("sigma")
    assert np.array_equal(iw, ic) and np.array_equal(sw, sc)
    ok = sw == 0
    assert _rel(uw[ok], uc[ok]) < tol and np.max(np.abs(cw[ok] - cc[ok]) / np.abs(cc[ok])) < tol
    npred = spec.n * spec.p
    bound = spec.c * spec.eps_max
    assert np.max(np.abs(sg[ok] - sgc[ok])) < tol * max(bound, np.max(np.abs(sgc[ok])))
    assert np.max(np.abs(sg[ok][:, npred:])) <= bound * (1 + 1e-12)
    return uw, cw, sw, iw, sg


def _active_count(spec, sg):
    bound = spec.c * spec.eps_max
    return np.sum(np.abs(np.abs(sg[:, spec.n * spec.p:]) - bound) <= 1e-9 * bound, axis=1)


def test_option_contract(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    with T._engine(spec, 400, 2) as eng:
        eng.set_convex_warm_law(True)
        eng.set_convex_warm_law(False)
        with pytest.raises(L.DDMPCError) as e:
            L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_CONVEX_WARM_LAW, 2))
        assert e.value.code == L.ERR_INVALID
    with T._engine(orc.spec_from_params(), 400, 2) as eng:               # slack NONE: accepted, no effect
        u_d, y_d, up, yp = T._instances(2)
        eng.set_data(u_d, y_d)
        u0, c0, _, _ = (x.copy() for x in eng.step(up, yp))
        eng.set_convex_warm_law(True)
        u1, c1, _, _ = eng.step(up, yp)
        assert np.array_equal(u0, u1) and np.array_equal(c0, c1)
    with T._engine(orc.spec_from_params(controller_type=0), 400, 2) as eng:   # NOMINAL: accepted
        eng.set_convex_warm_law(True)
    dspec = orc.spec_from_params(slack_var_constraint_type=1)
    Qd = dspec.Q.copy()
    Qd[0, 1] = Qd[1, 0] = 0.1
    dspec.Q = Qd
    with T._engine(dspec, 400, 2) as eng:
        with pytest.raises(L.DDMPCError) as e:
            eng.set_convex_warm_law(True)
        assert e.value.code == L.ERR_UNSUPPORTED
        eng.set_convex_warm_law(False)
    big = orc.spec_from_params(slack_var_constraint_type=1, L=64)        # (2 + 2)(64 + 4) = 272 rows
    with T._engine(big, 600, 2) as eng:
        with pytest.raises(L.DDMPCError) as e:
            eng.set_convex_warm_law(True)
        assert e.value.code == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("family", ["tail", "setpoint", "random"])
def test_step_parity_three_window_families(gpu, family):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 1024
    u_d, y_d, up, yp = T._instances(B, seed0=500)
    up, yp = _windows(spec, up, yp, family, np.random.default_rng(7))
    with T._engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        eng.set_convex_warm_law(True)
        eng.prepare()
        uw, cw, sw, iw, _ = _step_vs_solve(eng, spec, up, yp)
    T._check(spec, u_d, y_d, up, yp, uw, cw, sw, range(0, B, 16))
    if family == "tail":
        assert np.any(iw == 1) and np.any(iw >= 2)
    if family == "setpoint":
        assert np.any(iw == 1)


def test_no_cold_resolve_after_prepare(gpu):
    # the data are borrowed device tensors: after prepare() their contents are overwritten with NaN behind the handle's back;
    # a step that re-solved anything cold would read them
    torch = pytest.importorskip("torch")
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 64
    u_d, y_d, up, yp = T._instances(B, seed0=900)
    d = generate_batch(range(900, 900 + B))
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(3).uniform(-1.0, 1.0, (B, 41, 2))
    ut = torch.tensor(u_d, device="cuda:0")
    yt = torch.tensor(y_d, device="cuda:0")
    with T._engine(spec, 400, B) as eng:
        eng.set_convex_warm_law(True)
        eng.set_data(ut, yt)
        eng.prepare()
        u0, c0, s0, i0 = (x.copy() for x in eng.step(up, yp))
        cl0 = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w)
        torch.cuda.synchronize()
        ut.fill_(float("nan"))
        yt.fill_(float("nan"))
        torch.cuda.synchronize()
        u1, c1, s1, i1 = (x.copy() for x in eng.step(up, yp))
        cl1 = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w)
    assert np.any(i0 >= 2) and np.all(s0 == 0)
    assert np.all(np.isfinite(u1)) and np.all(np.isfinite(c1))
    assert np.array_equal(u0, u1) and np.array_equal(c0, c1) and np.array_equal(s0, s1) and np.array_equal(i0, i1)
    assert np.all(cl0[2] == 0)
    for a, b in zip(cl0, cl1):
        assert np.array_equal(a, b)
    T._check(spec, u_d, y_d, up, yp, u1, c1, s1, range(0, B, 8))


def test_many_switched_components_and_iteration_cap(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    spec.c = 0.02                                      # a small box: most predicted slacks end at their bound
    B = 256
    u_d, y_d, up, yp = T._instances(B, seed0=40)
    up, yp = _windows(spec, up, yp, "random", np.random.default_rng(11))
    with T._engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        eng.set_convex_warm_law(True)
        uw, cw, sw, iw, sg = _step_vs_solve(eng, spec, up, yp)
    k = _active_count(spec, sg)
    assert np.max(k[sw == 0]) >= 16, np.max(k)
    rows = [b for b in range(0, B, 16) if sw[b] == 0]
    assert len(rows) >= 8
    T._check(spec, u_d, y_d, up, yp, uw, cw, sw, rows)
    with T._engine(spec, 400, B, max_iter=2) as eng:   # the cap: solver_error on exactly the cold solve's instances
        eng.set_data(u_d, y_d)
        eng.set_convex_warm_law(True)
        uw, cw, sw, iw = (x.copy() for x in eng.step(up, yp))
        uc, cc, sc, ic = eng.solve(up, yp)
    assert np.array_equal(sw, sc) and np.array_equal(iw, ic)
    assert np.any(sw == 4) and np.any(sw == 0)
    ok = sw == 0
    assert _rel(uw[ok], uc[ok]) < 1e-10


def test_step_parity_cfg4(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1, L=60)          # (2 + 2)(60 + 4) = 256 rows
    B = 256
    u_d, y_d, up, yp = T._instances(B, N=1000, seed0=300)
    with T._engine(spec, 1000, B) as eng:
        eng.set_data(u_d, y_d)
        eng.set_convex_warm_law(True)
        for family in ("tail", "random"):
            upf, ypf = _windows(spec, up, yp, family, np.random.default_rng(5))
            uw, cw, sw, iw, _ = _step_vs_solve(eng, spec, upf, ypf)
            assert np.any(iw >= 2)
    T._check(spec, u_d, y_d, upf, ypf, uw, cw, sw, range(0, B, 64))


@pytest.mark.parametrize("n_mpc_step", [1, 3])
def test_closed_loop_against_cold_path(gpu, n_mpc_step):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B, n_steps = 64, 61
    d = generate_batch(range(170, 170 + B))
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B, n_steps, 2))
    up = d["u_d"][:, -4:, :].reshape(B, -1); yp = d["y_d"][:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    out = {}
    with T._engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_closed_loop_path("cold")
        out["cold"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        eng.set_convex_warm_law(True)
        eng.set_closed_loop_path("auto")
        out["warm"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        # the last solve's variables are those of the final control step
        sg = eng.get_solution("sigma")
        assert np.max(np.abs(sg[:, 8:])) <= spec.c * spec.eps_max * (1 + 1e-12)
    for a, b in zip(out["cold"], out["warm"]):
        assert np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))) < 1e-9
    assert np.array_equal(out["cold"][2], out["warm"][2]) and np.all(out["warm"][2] == 0)


def test_invalidation_and_refinement(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 64
    u_d, y_d, up, yp = T._instances(B, seed0=60)
    with T._engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        eng.set_convex_warm_law(True)
        _step_vs_solve(eng, spec, up, yp)
        eng.set_setpoints(np.array([0.8, 1.1]), np.array([0.5, 0.9]))
        _step_vs_solve(eng, spec, up, yp)
        u_d2, y_d2, up2, yp2 = T._instances(B, seed0=160)
        eng.set_data(u_d2, y_d2)
        _step_vs_solve(eng, spec, up2, yp2)
        eng.set_refinement("off")
        _step_vs_solve(eng, spec, up2, yp2)
        eng.set_refinement("always")                   # every law refined: the box goes to the filtered cold launch
        _, _, _, iw, _ = _step_vs_solve(eng, spec, up2, yp2)
        assert np.any(iw >= 2)


@pytest.mark.parametrize("refine", ["auto", "always"])
@pytest.mark.parametrize("case", [1, 4, 10])
def test_random_plants_with_refinement(gpu, case, refine):
    # the CONVEX cases of the random-plant sweep (test_gpu_parity.py::test_random_systems_against_oracle, tools/small_fuzz.py):
    # the same plants, data and parameters, ill-conditioned data that AUTO refinement flags
    rng = np.random.default_rng(1000 + case)
    m, p = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3)][case % 6]
    ns = int(rng.integers(2, 5))
    n = ns
    Lh = int(rng.integers(2 * n, 2 * n + 9))
    if (m + p) * (Lh + n) > 200:
        Lh = max(2 * n, 200 // (m + p) - n)
    N = (m + 1) * (Lh + 2 * n) + int(rng.integers(80, 200))
    eps = 0.002
    tec = case % 5 != 4
    if case % 2 == 0:
        Q = 2.0 * np.eye(p * Lh); R = 0.05 * np.eye(m * Lh)
    else:
        Q = np.diag(rng.uniform(1.0, 4.0, p * Lh)); R = np.diag(rng.uniform(0.01, 0.1, m * Lh))
    plant = T._random_plant(rng, ns, m, p, eps)
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=Q, R=R, u_s=rng.uniform(-0.5, 0.5, m), y_s=rng.uniform(-0.5, 0.5, p),
                      robust=True, eps_max=eps, lamb_alpha=20.0, lamb_sigma=500.0, c=1.0, slack="convex", tec=tec)
    B = 3
    d = generate_batch(range(case * 10, case * 10 + B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with T._engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_refinement(refine)
        eng.set_convex_warm_law(True)
        uw, cw, sw, iw = (x.copy() for x in eng.step(up, yp))
        uc, cc, sc, ic = eng.solve(up, yp)
    assert np.array_equal(sw, sc) and np.array_equal(iw, ic)
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(sw[b])] == sol.status == "optimal"
        scale = max(np.max(np.abs(sol.optimal_u)), 1e-3)
        assert np.max(np.abs(uw[b] - sol.optimal_u)) / scale < TOL_U, (case, b)
        assert abs(cw[b] - sol.cost) <= TOL_COST * max(abs(sol.cost), 1e-6), (case, b)
