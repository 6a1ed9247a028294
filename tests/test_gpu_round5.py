"""GPU tests added in round 5: the advisor's untested API sequences of round 4 (plants with more than 16 channels on the
structured Gram, the pipeline switch between ddmpc_prepare and ddmpc_step, ddmpc_solve -> ddmpc_prepare with the affine law ->
ddmpc_get_solution) and this round's kernels (see the section headers)."""
import os
import sys

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOL_U, TOL_COST = 1e-8, 1e-9


def _spec_engine(spec, N, B, **kw):
    return BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                        controller_type=L.ROBUST if spec.robust else L.NOMINAL,
                        slack_type=L.SLACK_CONVEX if spec.slack == "convex" else L.SLACK_NONE, eps_max=spec.eps_max,
                        lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec, **kw)


# ------------------------------------------------------------------ structured Gram, more than 16 channels
@pytest.mark.parametrize("m,p", [(9, 9), (10, 7), (4, 16)])
def test_structured_gram_with_more_than_sixteen_channels(gpu, m, p):
    """hankel_matrix.py:5-53 has no bound on the channel count.  ddmpc_gram_tiles_kernel formed the lag sums of the first 16
    channels only (four row groups of four), so for m + p > 16 the default Gram mode read lag sums nobody had written (LDS, so
    the allocation-poison test could not see it; advisor finding of round 4).  The kernel now passes over the row groups in
    fours.  Both Gram modes against the full-space oracle and against each other, with and without the slack box."""
    rng = np.random.default_rng(900 + 7 * m + p)
    ns = n = 2
    nch = m + p
    Lh = max(2 * n, 250 // nch - n)                      # as many rows as the largest register-resident instance takes
    while nch * (Lh + n) > 268:
        Lh -= 1
    N = (m + 1) * (Lh + 2 * n) + 60
    A = rng.normal(size=(ns, ns)); A *= 0.8 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.002)
    B = 3
    d = harness.generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    for slack in ("none", "convex"):
        spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=rng.uniform(-0.5, 0.5, m),
                          y_s=rng.uniform(-0.5, 0.5, p), robust=True, eps_max=0.002, lamb_alpha=20.0, lamb_sigma=500.0, c=1.0,
                          slack=slack, tec=True)
        res = {}
        for mode in (L.GRAM_DENSE, L.GRAM_STRUCTURED, L.GRAM_AUTO):
            with _spec_engine(spec, N, B, gram_mode=mode) as eng:
                assert "cold" in eng.kernel_name()
                eng.set_refinement("always")
                eng.set_data(d["u_d"], d["y_d"])
                u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
            res[mode] = (u, cost, status, iters)
            for b in range(B):
                sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
                assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
                assert np.max(np.abs(u[b] - sol.optimal_u)) / max(np.max(np.abs(sol.optimal_u)), 1e-3) < 1e-8, (mode, b)
                assert abs(cost[b] - sol.cost) <= 1e-8 * max(abs(sol.cost), 1e-6), (mode, b)
        dn, st = res[L.GRAM_DENSE], res[L.GRAM_STRUCTURED]
        assert np.array_equal(dn[3], st[3])
        assert np.max(np.abs(dn[0] - st[0])) <= 1e-9 * np.max(np.abs(dn[0]))
        assert np.array_equal(res[L.GRAM_AUTO][0], st[0])


def test_explicit_structured_gram_on_a_trajectory_beyond_the_gram_launch_lds(gpu):
    # Five channels x 3700 steps: more than ddmpc_gram_tiles_kernel (and the cold-solve kernel) can stage in LDS.  Until round 4
    # AUTO fell back to the dense product there and an explicit DDMPC_GRAM_STRUCTURED was dropped silently (advisor finding);
    # since round 5 such trajectories take the STREAMING structured Gram (rr2_gram_kernel + rr2_pack_tiles_kernel), so the
    # request is served: STRUCTURED == AUTO bit for bit, and both meet the compiled C restatement.  (Should a shape ever be
    # unservable, ddmpc_create answers DDMPC_ERR_UNSUPPORTED naming DDMPC_GRAM_STRUCTURED -- ddmpc_api.hip.)
    from oracle import oracle_c
    m, p, n, Lh, N, B = 3, 2, 2, 20, 3700, 3
    rng = np.random.default_rng(5)
    A = rng.normal(size=(n, n)); A *= 0.8 / max(abs(np.linalg.eigvals(A)))
    # (noise 0.05: cond(H) is the signal-to-noise ratio of the data, and without the trajectory on chip there is no refining variant --
    #  an ill-conditioned data set of this length is reported "optimal_inaccurate", which is not what this test is about)
    plant = dict(A=A, B=rng.normal(size=(n, m)), C=0.3 * rng.normal(size=(p, n)), D=np.zeros((p, m)), eps_max=0.05)
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=0.1 * np.ones(m), y_s=0.1 * np.ones(p),
                      robust=True, eps_max=0.05, lamb_alpha=2.0, lamb_sigma=500.0, c=1.0, slack="none", tec=True)
    d = harness.generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    res = {}
    for mode in (L.GRAM_AUTO, L.GRAM_STRUCTURED):
        with _spec_engine(spec, N, B, gram_mode=mode) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            res[mode] = tuple(x.copy() for x in eng.solve(up, yp))
    assert all(np.array_equal(a, b_) for a, b_ in zip(res[L.GRAM_AUTO], res[L.GRAM_STRUCTURED]))
    uo, co, so, _ = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=4)
    u, cost, status, _ = res[L.GRAM_AUTO]
    assert np.all(status == 0) and np.all(so == 0)
    assert np.max(np.max(np.abs(u - uo), axis=1) / np.max(np.abs(uo), axis=1)) < TOL_U and np.max(np.abs(cost - co) / np.abs(co)) < TOL_COST


# ------------------------------------------------------------------ pipeline switch between ddmpc_prepare and ddmpc_step
@pytest.mark.parametrize("case", ["nominal_cfg5", "robust_convex_296"])
def test_prepare_under_stamps_then_step_without_them(gpu, case):
    # Controllers beyond 271 rows.  ddmpc_debug_stamps selects the one-workgroup route (the phase kernels carry no stamps), and the
    # two routes keep different things next to the factors (Minv blocks, live masks; ROBUST: other slices altogether): what
    # ddmpc_prepare kept serves only the route it was formed on, and a step on the other route prepares again (advisor findings of
    # rounds 4 and 5 -- for ROBUST the step read the other layout: a GPU memory fault, or wrong results).  The cold solve on the
    # phase route comes first: it sizes every workspace of that route, so a step that mixed the layouts fails an assertion here.
    B = 3
    if case == "nominal_cfg5":
        from test_gpu_round3 import _config5
        spec, plant, N, d, up, yp = _config5(B)
    else:
        N = 700
        spec, d, up, yp = _four_tank_long(B, 70, N, "convex")
    with _spec_engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        ref = tuple(x.copy() for x in eng.solve(up, yp))                 # phase route
        eng.debug_stamps(True)
        ref1 = tuple(x.copy() for x in eng.solve(up, yp))                # one-workgroup route
        eng.prepare()
        eng.debug_stamps(False)
        w = tuple(x.copy() for x in eng.step(up, yp))
        eng.debug_stamps(True)                                           # ... and the other way round
        w2 = tuple(x.copy() for x in eng.step(up, yp))
        eng.debug_stamps(False)
        eng.prepare()
        eng.debug_stamps(True)
        c1 = tuple(x.copy() for x in eng.solve(up, yp))                  # a cold solve on the other route overwrites the workspace ...
        eng.debug_stamps(False)
        w3 = tuple(x.copy() for x in eng.step(up, yp))                   # ... so the step prepares again
    assert np.all(ref[2] == 0) and np.all(ref1[2] == 0)
    assert all(np.array_equal(a, b_) for a, b_ in zip(w, ref))           # same route, same factors: bit-equal
    assert all(np.array_equal(a, b_) for a, b_ in zip(w3, ref))
    assert all(np.array_equal(a, b_) for a, b_ in zip(w2, ref1)) and all(np.array_equal(a, b_) for a, b_ in zip(c1, ref1))
    assert np.max(np.abs(w2[0] - w[0])) <= TOL_U * np.max(np.abs(w[0]))  # the other route: inside the bars
    assert np.max(np.abs(w2[1] - w[1]) / np.abs(w[1])) < TOL_COST


def test_debug_workspace_reads_the_route_of_the_last_solve(gpu):
    # ddmpc_debug_workspace returned the rr3 record whenever one had ever been allocated, also after the pipeline changed (advisor
    # finding of round 5).  It reads what the last solve left on the route that served it: ROBUST at 296 rows on the phase kernels
    # leaves the rr3 record; the one-workgroup kernel leaves nothing this call reads.
    import ctypes as C
    B, N = 2, 700
    spec, d, up, yp = _four_tank_long(B, 70, N, "convex")
    rv = ((spec.m + spec.p) * (spec.L + spec.n) + 1) & ~1
    RR3_KMAX = 64                                                        # ddmpc_rr3.hpp
    lib = L.load()
    na, nm = C.c_int64(-1), C.c_int64(-1)
    with _spec_engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.solve(up, yp)
        L.check(lib.ddmpc_debug_workspace(eng._h, 0, None, 0, None, 0, C.byref(na), C.byref(nm)))
        assert na.value == 0 and nm.value == 4 + RR3_KMAX + rv + 4
        eng.set_large_pipeline("one_workgroup")
        eng.solve(up, yp)
        assert lib.ddmpc_debug_workspace(eng._h, 0, None, 0, None, 0, C.byref(na), C.byref(nm)) == L.ERR_NOT_READY


# ------------------------------------------------------------------ solve -> prepare (affine law) -> get_solution(alpha)
def test_prepare_with_the_affine_law_after_solve_keeps_alpha_readable(gpu):
    # with DDMPC_OPT_LARGE_AFFINE_LAW ddmpc_prepare runs its unit-window solves in the vectors the last solve kept for the
    # on-demand x = L^-T w of ddmpc_get_solution(ALPHA) (advisor finding of round 4: alpha came back from a unit window's w)
    from test_gpu_round3 import _config5
    B = 2
    spec, plant, N, d, up, yp = _config5(B)
    with _spec_engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = (x.copy() for x in eng.solve(up, yp))
        al0 = eng.get_solution("alpha")
    with _spec_engine(spec, N, B) as eng:
        eng.set_large_affine_law(True)
        eng.set_data(d["u_d"], d["y_d"])
        u1, cost1, status1, _ = (x.copy() for x in eng.solve(up, yp))
        eng.prepare()
        al1 = eng.get_solution("alpha")
        ub1 = eng.get_solution("ubar")
    assert np.all(status == 0) and np.array_equal(u, u1)
    assert np.array_equal(al0, al1)
    assert np.array_equal(ub1[:, spec.n * spec.m:], u)
    # alpha reproduces the trajectory: H alpha = [ubar; ybar]
    from direct_data_driven_mpc_amd.utilities.hankel_matrix import hankel_matrix
    Hu = hankel_matrix(d["u_d"][0], spec.L + spec.n)
    assert np.max(np.abs(Hu @ al1[0] - ub1[0])) <= 1e-7 * np.max(np.abs(ub1[0]))


# ------------------------------------------------------------------ slack CONVEX: active-set iterations on the kept factor
def _four_tank(B, N=400, L_=30, **over):
    spec = orc.spec_from_params(slack_var_constraint_type=1, L=L_, **over)
    d = harness.generate_batch(range(B), N=N)
    n = spec.n
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    return spec, d, up, yp


@pytest.mark.parametrize("cfg", ["cfg2", "cfg4"])
def test_convex_rank_update_equals_refactoring(gpu, cfg):
    """controller.py:631-677: the box on sigma[n*p:].  Since round 5 the active-set iterations after the first keep the factor
    of the empty active set (rank-k update, ddmpc_cold2.hpp `rank_update`; DDMPC_OPT_CONVEX_UPDATE).  Against the variant that
    factors the system again in every iteration (rounds 1-4): identical statuses, iteration counts and active sets on every
    instance, solutions and costs 1e-10 apart; against the compiled C restatement (re-factoring, structured Gram): equal
    iteration counts, the standard bars; the bound holds everywhere."""
    from oracle import oracle_c
    B, N, L_ = (1024, 400, 30) if cfg == "cfg2" else (256, 1000, 60)
    spec, d, up, yp = _four_tank(B, N, L_)
    res = {}
    for upd in (True, False):
        with _spec_engine(spec, N, B) as eng:
            eng.set_convex_update(upd)
            eng.set_data(d["u_d"], d["y_d"])
            u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
            sig = eng.get_solution("sigma")
            uh = tuple(x.copy() for x in eng.solve_from_host(d["u_d"], d["y_d"], up, yp))
        res[upd] = (u, cost, status, iters, sig)
        assert np.array_equal(uh[0], u) and np.array_equal(uh[3], iters)       # the chunked host path runs the same kernel
    a, b = res[True], res[False]
    assert np.all(a[2] == 0) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[3].max() >= 2 and np.mean(a[3] >= 2) > 0.5                        # the box does bind on these data
    bound = spec.c * spec.eps_max
    act_a = np.sign(a[4][:, spec.n * spec.p:]) * (np.abs(a[4][:, spec.n * spec.p:]) >= bound * (1 - 1e-12))
    act_b = np.sign(b[4][:, spec.n * spec.p:]) * (np.abs(b[4][:, spec.n * spec.p:]) >= bound * (1 - 1e-12))
    assert np.array_equal(act_a, act_b)
    assert np.max(np.abs(a[4][:, spec.n * spec.p:])) <= bound * (1 + 1e-12)
    assert np.max(np.max(np.abs(a[0] - b[0]), axis=1) / np.max(np.abs(b[0]), axis=1)) < 1e-10
    assert np.max(np.abs(a[1] - b[1]) / np.abs(b[1])) < 1e-10
    uo, co, so, io = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=8)
    assert np.all(so == 0) and np.array_equal(io, a[3])
    assert np.max(np.max(np.abs(a[0] - uo), axis=1) / np.max(np.abs(uo), axis=1)) < TOL_U
    assert np.max(np.abs(a[1] - co) / np.abs(co)) < TOL_COST


@pytest.mark.parametrize("c_box", [0.6, 0.25, 0.05])
def test_convex_rank_update_with_many_active_components(gpu, c_box):
    """A tighter box (`c` below the reference's 1, controller_creation.py:119): more slack components reach their bound --
    up to dozens per instance at c = 0.05 -- so the iterations mix rank-k updates (k <= 4) with the fall-back to a new
    factorisation (k > 4, after which every further iteration factors again).  Every instance against the full-space oracle
    of the reference formulation: status, iteration count, optimal_u, cost; and against the re-factoring variant."""
    B = 24
    spec, d, up, yp = _four_tank(B)
    spec.c = c_box
    res = {}
    for upd in (True, False):
        with _spec_engine(spec, 400, B) as eng:
            eng.set_convex_update(upd)
            eng.set_data(d["u_d"], d["y_d"])
            res[upd] = tuple(x.copy() for x in eng.solve(up, yp))
            sig = eng.get_solution("sigma")
    u, cost, status, iters = res[True]
    assert np.array_equal(status, res[False][2]) and np.array_equal(iters, res[False][3])
    assert np.max(np.abs(u - res[False][0])) <= 1e-9 * np.max(np.abs(u))
    nact = np.sum(np.abs(sig[:, spec.n * spec.p:]) >= spec.c * spec.eps_max * (1 - 1e-12), axis=1)
    if c_box <= 0.05:
        assert nact.max() > 4                                  # the fall-back did run
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
        assert int(iters[b]) == sol.iters, (b, int(iters[b]), sol.iters, int(nact[b]))
        assert np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U
        assert abs(cost[b] - sol.cost) / abs(sol.cost) < TOL_COST


def test_convex_rank_update_in_warm_steps_and_closed_loop(gpu):
    # ddmpc_step with the slack box: the affine law of the empty active set + a filtered cold launch for the instances that
    # leave the box -- that launch is the rank-update kernel now; results equal ddmpc_solve's bit for bit
    B = 64
    spec, d, up, yp = _four_tank(B)
    with _spec_engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        cold = tuple(x.copy() for x in eng.solve(up, yp))
        warm = tuple(x.copy() for x in eng.step(up, yp))
    assert np.array_equal(cold[2], warm[2]) and np.array_equal(cold[3], warm[3])
    flagged = cold[3] >= 2
    assert flagged.any() and (~flagged).any()
    assert np.array_equal(cold[0][flagged], warm[0][flagged]) and np.array_equal(cold[1][flagged], warm[1][flagged])
    assert np.max(np.abs(cold[0] - warm[0])) <= 1e-9 * np.max(np.abs(cold[0]))


# ------------------------------------------------------------------ ROBUST beyond 271 rows on the phase kernels (ddmpc_rr3.hpp)
def _four_tank_long(B, L_, N, slack, c_box=1.0):
    spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=L_)
    spec.c = c_box
    d = harness.generate_batch(range(B), N=N)
    n = spec.n
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    return spec, d, up, yp


@pytest.mark.parametrize("slack", ["none", "convex"])
def test_large_robust_phase_kernels_agree_with_the_one_workgroup_kernel(gpu, slack):
    """controller.py:541-545, 631-677 at 296 rows (four-tank, L = 70: beyond the register-resident kernels).  Round 5 moved the
    ROBUST scheme at these sizes onto the lock-step pipeline (ddmpc_rr3.hpp: factor of the empty active set, slack-box iterations
    as Woodbury updates on the trailing block).  Against the one-workgroup kernel of rounds 1-4 (DDMPC_OPT_LARGE_PIPELINE, which
    re-factors the Schur block of the boxed components per iteration): equal statuses and iteration counts, solutions 1e-9 apart;
    against the full-space oracle at the standard bars; ddmpc_step on the kept factors bit-equal to ddmpc_solve."""
    B, L_, N = 6, 70, 700
    spec, d, up, yp = _four_tank_long(B, L_, N, slack)
    res = {}
    for pipe in ("phases", "one_workgroup"):
        with _spec_engine(spec, N, B) as eng:
            assert eng.kernel_name() == "ddmpc_large_solve_kernel"
            eng.set_large_pipeline(pipe)
            eng.set_data(d["u_d"], d["y_d"])
            res[pipe] = tuple(x.copy() for x in eng.solve(up, yp))
            sg = eng.get_solution("sigma")
            w = tuple(x.copy() for x in eng.step(up, yp))
            assert all(np.array_equal(a, b_) for a, b_ in zip(w, res[pipe]))
            if slack == "convex":
                assert np.max(np.abs(sg[:, spec.n * spec.p:])) <= spec.c * spec.eps_max * (1 + 1e-12)
    a, b_ = res["phases"], res["one_workgroup"]
    assert np.all(a[2] == 0) and np.array_equal(a[2], b_[2]) and np.array_equal(a[3], b_[3])
    assert np.max(np.abs(a[0] - b_[0])) <= 1e-9 * np.max(np.abs(b_[0])) and np.max(np.abs(a[1] - b_[1]) / np.abs(b_[1])) < 1e-9
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert sol.status == "optimal" and int(a[3][b]) == max(sol.iters, 1)
        assert np.max(np.abs(a[0][b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U
        assert abs(a[1][b] - sol.cost) / abs(sol.cost) < TOL_COST


def test_large_robust_phase_kernels_hand_crowded_active_sets_to_the_fall_back(gpu):
    """A box tight enough that more than 64 slack components reach their bound (c = 0.01 at 296 rows): the phase solve keeps at most
    64 columns of W, marks such instances and ddmpc_large_solve_kernel finishes them on a small persistent grid.  Every instance
    against the full-space oracle (status, iteration count, optimal_u, cost), whichever path served it."""
    B, L_, N = 6, 70, 700
    spec, d, up, yp = _four_tank_long(B, L_, N, "convex", c_box=0.01)
    with _spec_engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
        sg = eng.get_solution("sigma")
    nact = np.sum(np.abs(sg[:, spec.n * spec.p:]) >= spec.c * spec.eps_max * (1 - 1e-12), axis=1)
    assert nact.max() > 64, nact                                      # the fall-back did serve at least one instance
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
        assert int(iters[b]) == sol.iters, (b, int(iters[b]), sol.iters, int(nact[b]))
        assert np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U
        assert abs(cost[b] - sol.cost) / abs(sol.cost) < TOL_COST


# ------------------------------------------------------------------ the rank decision of exact-data NOMINAL problems
def test_rank_decision_on_the_plant_whose_noise_pivot_sits_above_the_fixed_tolerance(gpu):
    """hankel_matrix.py:82 decides ranks with a data-scaled tolerance; the phase kernels used a fixed 1e-8 x (largest diagonal)
    pivot rule.  The 9-channel plant of `_exact_plant_case(154, 5, 4, ...)` leaves a rounding residue of 1.4e-8 on ONE dependent
    row of ONE of its first six instances (tools/pivot_gap_study.py: instance 3 accepted 231 pivots where rank H = m (L + n) + n =
    230, the next genuine pivot is 1.1e-5): in round 4 that instance came back "optimal" with a wrong input sequence and the
    test was moved to other seeds.  Round 5: rr2_rank_margin_kernel judges the decision from the pivot candidates afterwards --
    more pivots than rank H can have => a tolerance in the middle of the gap and one more factorisation; a decision without a
    clear margin => "optimal_inaccurate", never a silent "optimal".  Both pipelines against the model-based solution at the
    standard bars, all six instances."""
    from oracle.nominal_exact import solve_nominal_model_based_batch
    from test_gpu_round4 import _exact_plant_case
    m, p, n, Lh, N, B = 5, 4, 5, 40, 1200, 6
    spec, plant, d, up, yp = _exact_plant_case(154, m, p, n, Lh, N, B)
    u_ref, c_ref, feas = solve_nominal_model_based_batch(spec, plant, up, yp)
    assert np.max(feas) < 1e-10
    res = {}
    for mode in ("phases", "one_workgroup"):
        with _spec_engine(spec, N, B) as eng:
            eng.set_large_pipeline(mode)
            eng.set_data(d["u_d"], d["y_d"])
            res[mode] = tuple(x.copy() for x in eng.solve(up, yp))
            if mode == "phases":
                w = tuple(x.copy() for x in eng.step(up, yp))          # the kept factors are the re-factored ones
                assert np.array_equal(w[0], res[mode][0]) and np.array_equal(w[2], res[mode][2])
    for mode, (u, c, st, it) in res.items():
        assert np.all((st == 0) | (st == 1)), (mode, st)               # optimal, or optimal_inaccurate where the margin is thin
        eu = np.max(np.abs(u - u_ref), axis=1) / np.max(np.abs(u_ref), axis=1)
        ec = np.abs(c - c_ref) / np.abs(c_ref)
        assert eu.max() < TOL_U and ec.max() < TOL_COST, (mode, eu, ec)
    print("statuses on the phase kernels:", res["phases"][2], "one workgroup:", res["one_workgroup"][2])


# ------------------------------------------------------------------ trajectories beyond the LDS of the cold-solve kernel
@pytest.mark.parametrize("N,slack", [(6000, "none"), (6000, "convex"), (20000, "none")])
def test_trajectories_beyond_the_lds(gpu, N, slack):
    """hankel_matrix.py:39-51 takes any N >= L; the register-resident kernels stage the whole trajectory in LDS and refused
    N = 6000 at create time until round 4.  Now G = H H' of such data sets comes from the streaming Gram kernel of the phase
    pipeline (trajectory in chunks), is re-laid into the cold kernel's tiles and the kernel runs without a trajectory region.
    Four-tank, L = 30, against the full-space oracle at the standard bars: ddmpc_solve, the chunked ddmpc_solve_from_host,
    ddmpc_prepare / ddmpc_step; refinement ALWAYS (which needs the trajectory on chip) is refused, not ignored."""
    B = 4
    spec = orc.spec_from_params(N=N, slack_var_constraint_type=1 if slack == "convex" else 0)
    d = harness.generate_batch(range(40, 40 + B), N=N)
    n = spec.n
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with _spec_engine(spec, N, B) as eng:
        assert "cold" in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
        al = eng.get_solution("alpha"); ub = eng.get_solution("ubar")
        uh = tuple(x.copy() for x in eng.solve_from_host(d["u_d"], d["y_d"], up, yp))
        eng.set_data(d["u_d"], d["y_d"])
        uw = tuple(x.copy() for x in eng.step(up, yp))
        eng.set_refinement("always")                      # (refused for such handles until the refining variant learnt to
        ur = tuple(x.copy() for x in eng.solve(up, yp))   #  window the trajectory: test_refinement_on_trajectories_beyond_the_lds)
    assert np.array_equal(ur[2], status) and np.array_equal(ur[3], iters) and np.max(np.abs(ur[0] - u)) <= 1e-9 * np.max(np.abs(u))
    assert np.array_equal(uh[0], u) and np.array_equal(uh[2], status)
    assert np.max(np.abs(uw[0] - u)) <= 1e-9 * np.max(np.abs(u)) and np.array_equal(uw[2], status)
    Hu = orc.hankel_matrix(d["u_d"][0], spec.Ln)
    assert np.max(np.abs(Hu @ al[0] - ub[0])) <= 1e-8 * np.max(np.abs(ub[0]))
    # checkers: the compiled C restatement (reduced form, structured Gram) on every instance; the full-space oracle of the
    # reference formulation on one instance at N = 6000 (its dense KKT system has N + 3 (L + n) (m + p) / ... unknowns: ~10 s there,
    # ~200 s at N = 20000, where the numpy reduced form stands in)
    from oracle import oracle_c
    from oracle.reduced_form import solve_reduced
    uo, co, so, io = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=4)
    assert np.all(status == 0) and np.array_equal(so, status) and np.array_equal(io, iters)
    assert np.max(np.max(np.abs(u - uo), axis=1) / np.max(np.abs(uo), axis=1)) < TOL_U
    assert np.max(np.abs(cost - co) / np.abs(co)) < TOL_COST
    if N <= 6000:
        sol = orc.solve_fullspace(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0])
        ref_u, ref_c, ref_it = sol.optimal_u, sol.cost, max(sol.iters, 1)
        assert sol.status == "optimal"
    else:
        red = solve_reduced(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0])
        ref_u, ref_c, ref_it = red["optimal_u"], red["cost"], red["iters"]
    assert int(iters[0]) == ref_it
    assert np.max(np.abs(u[0] - ref_u)) / np.max(np.abs(ref_u)) < TOL_U and abs(cost[0] - ref_c) / abs(ref_c) < TOL_COST


# ------------------------------------------------------------------ phase pipelines: several lags per matrix tile
@pytest.mark.parametrize("m,p", [(1, 1), (1, 2), (2, 3), (3, 3), (3, 4), (4, 4)])
def test_robust_phase_pipeline_gram_with_several_lags_per_tile(gpu, m, p):
    """hankel_matrix.py:5-53 through controller.py:506-538 on the phase kernels (more than 271 rows).  Plants of at most eight
    channels take rr2_gram_packed_kernel -- 16 / (m + p) lags in the rows of one matrix tile, with rows left over when the channel
    count does not divide 16: channel counts two to eight of the ROBUST scheme with the slack box against the full-space oracle."""
    rng = np.random.default_rng(1200 + 10 * m + p)
    n = 2
    nch = m + p
    Lh = 300 // nch                                       # r = nch (Lh + n) > 271 rows
    N = (m + 1) * (Lh + 2 * n) + 90
    A = rng.normal(size=(n, n)); A *= 0.8 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(n, m)), C=rng.normal(size=(p, n)), D=np.zeros((p, m)), eps_max=0.002)
    B = 3
    d = harness.generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=rng.uniform(-0.3, 0.3, m),
                      y_s=rng.uniform(-0.3, 0.3, p), robust=True, eps_max=0.002, lamb_alpha=20.0, lamb_sigma=500.0, c=1.0,
                      slack="convex", tec=True)
    with _spec_engine(spec, N, B) as eng:
        assert nch * (Lh + n) > 271 and "large" in eng.kernel_name()
        eng.set_refinement("always")
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
        assert np.max(np.abs(u[b] - sol.optimal_u)) / max(np.max(np.abs(sol.optimal_u)), 1e-3) < TOL_U, b
        assert abs(cost[b] - sol.cost) <= TOL_COST * max(abs(sol.cost), 1e-6), b


@pytest.mark.parametrize("shape,seed", [((1, 2, 3, 100, 700), 31), ((3, 3, 3, 50, 900), 32), ((3, 4, 4, 40, 900), 33), ((4, 4, 4, 36, 900), 34)],
                         ids=["3ch", "6ch", "7ch", "8ch"])
def test_nominal_phase_pipeline_gram_with_several_lags_per_tile(gpu, shape, seed):
    """The same for the NOMINAL scheme on exact data (rank-revealing factorisation of the packed Gram matrix): the phase kernels
    against the model-based solution of the QP and against the one-workgroup kernels, which form their Gram matrix themselves
    (channel counts 2, 4, 5 and 9: tests/test_gpu_round4.py)."""
    from oracle.nominal_exact import solve_nominal_model_based_batch
    from test_gpu_round4 import _exact_plant_case
    m, p, n, Lh, N = shape
    B = 3
    spec, plant, d, up, yp = _exact_plant_case(seed, m, p, n, Lh, N, B)
    u_ref, c_ref, feas = solve_nominal_model_based_batch(spec, plant, up, yp)
    assert np.max(feas) < 1e-10
    res = {}
    for mode in ("phases", "one_workgroup"):
        with _spec_engine(spec, N, B) as eng:
            assert (m + p) * (Lh + n) > 271 and "nominal_rr" in eng.kernel_name()
            eng.set_large_pipeline(mode)
            eng.set_data(d["u_d"], d["y_d"])
            res[mode] = tuple(x.copy() for x in eng.solve(up, yp))
    u, c, st, it = res["phases"]
    assert np.all(st == 0), st
    eu = np.max(np.max(np.abs(u - u_ref), axis=1) / np.max(np.abs(u_ref), axis=1))
    ec = np.max(np.abs(c - c_ref) / np.abs(c_ref))
    assert eu < TOL_U and ec < TOL_COST, (eu, ec)
    a, bq = res["phases"], res["one_workgroup"]
    assert np.max(np.abs(a[0] - bq[0])) < 1e-7 * np.max(np.abs(bq[0]))


@pytest.mark.parametrize("m,p,N", [(3, 2, 5000), (1, 2, 9000), (4, 4, 3000), (5, 5, 2600)])
def test_trajectories_beyond_the_lds_with_other_channel_counts(gpu, m, p, N):
    """hankel_matrix.py:39-51 takes any N >= L for any channel count.  Plants of 3, 5, 8 and 10 channels with trajectories the cold
    kernel cannot stage: the streaming Gram launch passes the trajectory through its LDS in several chunks, with 5 / 3 / 2 lags per
    matrix tile (one tile row left over at five and three channels) or one (ten channels), and writes the kernel's tiles directly.
    Against the compiled C restatement on every instance and the full-space oracle on one; slack box on."""
    from oracle import oracle_c
    rng = np.random.default_rng(7000 + 10 * m + p)
    n = 3
    nch = m + p
    Lh = 130 // nch - n
    A = rng.normal(size=(n, n)); A *= 0.85 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(n, m)), C=rng.normal(size=(p, n)), D=np.zeros((p, m)), eps_max=0.02)
    B = 4
    d = harness.generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=rng.uniform(-0.3, 0.3, m),
                      y_s=rng.uniform(-0.3, 0.3, p), robust=True, eps_max=0.02, lamb_alpha=20.0, lamb_sigma=500.0, c=0.2,
                      slack="convex", tec=True)
    with _spec_engine(spec, N, B) as eng:
        assert "cold" in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
        with pytest.raises(L.DDMPCError):                 # the staged launch cannot hold this trajectory
            eng.set_gram_launch("staged")
    u_c, c_c, st_c, it_c = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=2)
    # every instance against the compiled restatement -- itself a Gram-route solve without refinement, good to ~1e-9 on these
    # plants, while the GPU refines what its streamed residual check keeps flagged -- and one against the full-space oracle
    assert not np.count_nonzero(st_c) and np.all(status == 0), status
    assert np.array_equal(iters, it_c)
    assert np.max(np.max(np.abs(u - u_c), axis=1) / np.max(np.abs(u_c), axis=1)) < TOL_U
    assert np.max(np.abs(cost - c_c) / np.abs(c_c)) < 1e-8
    sol = orc.solve_fullspace(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0])
    assert np.max(np.abs(u[0] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U
    assert abs(cost[0] - sol.cost) / abs(sol.cost) < TOL_COST and int(iters[0]) == sol.iters


@pytest.mark.parametrize("m,p,N", [(3, 2, 5000), (2, 2, 6000)])
def test_refinement_on_trajectories_beyond_the_lds(gpu, m, p, N):
    """The refining kernel variant on a trajectory the kernel cannot stage: its products with the implicit Hankel matrix pass the
    trajectory through a window of LDS chunk by chunk (ddmpc_cold2.hpp, KParams::stage_xs = 0).  Random plants with the noise level
    of the four-tank example leave the Gram route at ~5e-8 (the compiled restatement is no better): under AUTO the streamed
    residual check keeps those instances flagged and the refining variant brings them inside the bars against the full-space
    oracle; DDMPC_REFINE_ALWAYS, refused for such handles until this round, does the same for every instance; OFF shows what
    the refinement bought.  ddmpc_solve and the chunked ddmpc_solve_from_host."""
    rng = np.random.default_rng(7100 + 10 * m + p)
    n = 3
    nch = m + p
    Lh = 130 // nch - n
    A = rng.normal(size=(n, n)); A *= 0.85 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(n, m)), C=rng.normal(size=(p, n)), D=np.zeros((p, m)), eps_max=0.002)
    B = 300                                               # (ddmpc_solve_from_host splits 256 instances and more into chunks)
    d = harness.generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.05 * np.eye(m * Lh), u_s=rng.uniform(-0.3, 0.3, m),
                      y_s=rng.uniform(-0.3, 0.3, p), robust=True, eps_max=0.002, lamb_alpha=20.0, lamb_sigma=500.0, c=1.0,
                      slack="convex", tec=True)
    sols = [orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b]) for b in range(2)]
    err = {}
    for mode in ("off", "auto", "always"):
        with _spec_engine(spec, N, B) as eng:
            eng.set_refinement(mode)
            eng.set_data(d["u_d"], d["y_d"])
            u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
            sol = [eng.get_solution(w) for w in ("alpha", "ubar")]
            uh, ch, sh, ih = eng.solve_from_host(d["u_d"], d["y_d"], up, yp)
            solh = [eng.get_solution(w) for w in ("alpha", "ubar")]
            eng.set_data(d["u_d"], d["y_d"])
            uw = eng.step(up, yp)                         # (the affine law of ddmpc_prepare is refined the same way)
        assert np.all(status == 0), (mode, np.unique(status))
        if mode != "off":                                 # (the refining pass also refines the beta ddmpc_get_solution reads)
            assert all(np.array_equal(a, b) for a, b in zip(sol, solh)), mode
        if mode != "off":
            assert np.array_equal(uw[2], status) and np.max(np.abs(uw[0] - u)) <= 1e-8 * np.max(np.abs(u)), mode
        assert np.array_equal(uh, u) and np.array_equal(ch, cost) and np.array_equal(sh, status) and np.array_equal(ih, iters), mode
        err[mode] = max(np.max(np.abs(u[b] - s.optimal_u)) / np.max(np.abs(s.optimal_u)) for b, s in enumerate(sols))
        ec = max(abs(cost[b] - s.cost) / abs(s.cost) for b, s in enumerate(sols))
        assert all(int(iters[b]) == s.iters for b, s in enumerate(sols)), mode
        if mode != "off":
            assert err[mode] < TOL_U and ec < TOL_COST, (mode, err[mode], ec)
    assert err["always"] <= err["off"]


# ------------------------------------------------------------------ dense weighting matrices, NOMINAL beyond 271 rows
@pytest.mark.parametrize("shape", [(2, 3, 3, 60, 900), (2, 2, 4, 70, 700), (5, 4, 5, 40, 1200)], ids=["5ch-315rows", "4ch-296rows", "9ch-405rows"])
def test_dense_weighting_matrices_of_nominal_controllers_beyond_the_register_resident_kernels(gpu, shape):
    """controller.py:708-710 takes any PSD Q, R; until the second half of round 5 a NOMINAL controller beyond 271 rows with dense
    matrices was refused.  On the phase kernels the reduced normal matrix is T = C'(W C) (rr2_wc_kernel, rr2_cwc_kernel) and the
    products with W in the solve are launches of their own (rr2_wapply_kernel).  Exact data of seeded plants against the model-based
    solution of the QP (oracle/nominal_exact.py, dense matrices: tests/test_oracle.py), the warm step on the kept factors, the
    diagonal case given as dense matrices against the diagonal path, and the one-workgroup pipeline refusing."""
    from oracle.nominal_exact import solve_nominal_model_based
    from test_gpu_round4 import _exact_plant_case
    m, p, n, Lh, N = shape
    B = 3
    spec, plant, d, up, yp = _exact_plant_case({9: 4, 5: 125, 4: 142}[m + p], m, p, n, Lh, N, B)
    rng = np.random.default_rng(77 + m)

    def spd(k, s):
        X = rng.normal(size=(k, k))
        return s * (np.eye(k) + 0.3 * (X @ X.T) / k)
    Qd, Rd = spd(p * Lh, 3.0), spd(m * Lh, 1e-2)
    spec_d = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=Qd, R=Rd, u_s=spec.u_s, y_s=spec.y_s, robust=False, eps_max=0.0, lamb_alpha=0.0,
                        lamb_sigma=0.0, c=0.0, slack="none", tec=True)
    with _spec_engine(spec_d, N, B) as eng:
        assert (m + p) * (Lh + n) > 271 and "nominal_rr" in eng.kernel_name()
        with pytest.raises(L.DDMPCError, match="phase kernels only"):
            eng.set_large_pipeline("one_workgroup")
        with pytest.raises(L.DDMPCError, match="scalar / diagonal weights"):
            eng.set_large_affine_law(True)
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
        ub = eng.get_solution("ubar")
        eng.set_data(d["u_d"], d["y_d"])
        uw = eng.step(up, yp)
    assert np.all(status == 0), status
    assert np.array_equal(uw[0], u) and np.array_equal(uw[1], cost) and np.array_equal(ub[:, n * m:], u)
    for b in range(B):
        mod = solve_nominal_model_based(spec_d, plant, up[b], yp[b])
        assert mod["feas_residual"] < 1e-10
        assert np.max(np.abs(u[b] - mod["optimal_u"])) / np.max(np.abs(mod["optimal_u"])) < TOL_U, b
        assert abs(cost[b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), b
    # a diagonal weighting handed over as dense matrices: the dense code path against the diagonal one
    qd, rd = rng.uniform(1.0, 4.0, p * Lh), rng.uniform(0.01, 0.1, m * Lh)
    res = {}
    for kind in ("diag", "dense"):
        sp = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=np.diag(qd) + (1e-300 if kind == "dense" else 0.0), R=np.diag(rd), u_s=spec.u_s, y_s=spec.y_s,
                        robust=False, eps_max=0.0, lamb_alpha=0.0, lamb_sigma=0.0, c=0.0, slack="none", tec=True)
        with _spec_engine(sp, N, B) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            res[kind] = tuple(x.copy() for x in eng.solve(up, yp))
    assert np.array_equal(res["diag"][2], res["dense"][2])
    assert np.max(np.abs(res["diag"][0] - res["dense"][0])) <= 1e-9 * np.max(np.abs(res["diag"][0]))
    assert np.max(np.abs(res["diag"][1] - res["dense"][1]) / np.abs(res["diag"][1])) <= 1e-9
    # ... and the diagonal path against the model-based solution of the QP with these weights (two implementations that agree
    # with each other are not yet right)
    sp = orc.QPSpec(**{**spec.__dict__, "Q": np.diag(qd), "R": np.diag(rd)})
    assert np.all(res["diag"][2] == 0), res["diag"][2]
    for b in range(B):
        mod = solve_nominal_model_based(sp, plant, up[b], yp[b])
        assert mod["feas_residual"] < 1e-10
        assert np.max(np.abs(res["diag"][0][b] - mod["optimal_u"])) / np.max(np.abs(mod["optimal_u"])) < TOL_U, b
        assert abs(res["diag"][1][b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), b


# ------------------------------------------------------------------ more than 1024 rows (ROBUST)
@pytest.mark.parametrize("slack", ["none", "convex"])
def test_robust_scheme_beyond_1024_rows(gpu, slack):
    """hankel_matrix.py:47 has no size bound.  ROBUST controllers of 1025 .. 2048 rows -- here the four-tank plant with L = 271,
    1100 rows -- run on the 1024-thread instance of ddmpc_large_solve_kernel (the phase kernels address 16-column chunks with
    64-bit masks: 1024 rows): cold solve, the solve on the kept factors and the variables against the full-space oracle."""
    B = 2
    L_, N = 271, 1400
    spec = orc.spec_from_params(L=L_, N=N, slack_var_constraint_type=1 if slack == "convex" else 0)
    d = harness.generate_batch(range(B), N=N)
    n = spec.n
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with _spec_engine(spec, N, B) as eng:
        assert (spec.m + spec.p) * (L_ + n) == 1100 and "large_solve" in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, iters = (x.copy() for x in eng.solve(up, yp))
        sg = eng.get_solution("sigma")
        eng.set_data(d["u_d"], d["y_d"])
        uw = eng.step(up, yp)
    assert np.all(status == 0) and np.array_equal(uw[0], u) and np.array_equal(uw[2], status)
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert sol.status == "optimal" and (slack == "none" or int(iters[b]) == sol.iters)
        assert np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U, b
        assert abs(cost[b] - sol.cost) <= TOL_COST * abs(sol.cost), b
        assert np.max(np.abs(sg[b] - sol.sigma.ravel())) <= 1e-9 * max(1.0, np.max(np.abs(sol.sigma)))
    # NOMINAL controllers stop at 1524 rows (test_nominal_scheme_beyond_1024_rows), and nothing goes beyond 2048
    with pytest.raises(L.DDMPCError, match="too large"):
        BatchedDDMPC(n=4, m=2, p=2, L_=400, N=2000, Q=3.0, R=1e-4, u_s=spec.u_s, y_s=spec.y_s, batch=1, controller_type=L.NOMINAL)
    with pytest.raises(L.DDMPCError, match="too large"):
        BatchedDDMPC(n=4, m=2, p=2, L_=520, N=2700, Q=3.0, R=1e-4, u_s=spec.u_s, y_s=spec.y_s, batch=1, controller_type=L.ROBUST,
                     eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0)


def test_nominal_scheme_beyond_1024_rows(gpu):
    """NOMINAL controllers of 1025 .. 1524 rows (ten r-vectors of the one-workgroup kernel + its panel scratch in 160 KB of LDS) run on
    the 1024-thread instance of ddmpc_nominal_rr_kernel: a SISO plant with L = 600 (1206 rows, exact data) against the model-based
    solution, the step on the kept factors; more than 1524 rows are refused when the controller is created."""
    from oracle.nominal_exact import solve_nominal_model_based
    from test_gpu_round4 import _exact_plant_case
    m, p, n, Lh, N = 1, 1, 3, 600, 1500
    B = 2
    spec, plant, d, up, yp = _exact_plant_case(11, m, p, n, Lh, N, B)
    with _spec_engine(spec, N, B) as eng:
        assert (m + p) * (Lh + n) == 1206 and "nominal_rr" in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = (x.copy() for x in eng.solve(up, yp))
        eng.set_data(d["u_d"], d["y_d"])
        uw = eng.step(up, yp)
    assert np.all(status == 0), status
    assert np.max(np.abs(uw[0] - u)) <= 1e-9 * np.max(np.abs(u)) and np.array_equal(uw[2], status)
    for b in range(B):
        mod = solve_nominal_model_based(spec, plant, up[b], yp[b])
        assert mod["feas_residual"] < 1e-10
        assert np.max(np.abs(u[b] - mod["optimal_u"])) / np.max(np.abs(mod["optimal_u"])) < TOL_U, b
        assert abs(cost[b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), b
    with pytest.raises(L.DDMPCError, match="too large"):
        BatchedDDMPC(n=3, m=1, p=1, L_=800, N=1900, Q=3.0, R=1e-4, u_s=spec.u_s, y_s=spec.y_s, batch=1, controller_type=L.NOMINAL)
