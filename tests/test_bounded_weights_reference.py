"""The premises of tests/test_gpu_bounded_weights.py, on the references alone (no GPU): bounded ROBUST controllers under weights
that change with the step and with the channel, and with a zero weight next to a box.  Cases: tests/_bounded_weights_cases.py.

1. Every reference instance a GPU case compares is `optimal`, and at most one instance in eight per case has a margin below the
   one (1e-6 up to 271 rows, 1e-7 beyond) under which two correct implementations may count or decide differently -- with the
   three or four rows per case used here: none.  The reduced-space helper that serves the 296-row ramp cases agrees with the
   full-space helper on the first row of each (count, signed set, inputs 1e-9, cost 1e-10).
2. The final active set of the first row of every case holds components with at least three distinct d_s: with fewer, the case
   would test nothing a scalar weight does not.
3. The compositions the GPU cases need: reference counts above the forced max_iter on at least two rows (safeguards), peaks in
   (64, 256] (capacity), a window inside the box and one outside (box law), seeded runs that are kept (warm starts), the bounds of
   the m != p cases cutting an input and an output.
4. Each of the five MUTATIONS of tests/test_gpu_large_weights.py, applied to q and to r separately, moves optimal_u by at least
   1e-5 or the cost by at least 1e-6 relative -- 1000 bars -- on four cases.
5. A mistake in the box table ALONE shows without the refinement pass: one Woodbury update on the final active set (the kept
   factor of the empty set, W = L^-1 E, the k x k system diag(1 / d_s) - W'W) with the d_s column rolled by one over the active
   components, factor and targets as they are, moves the inputs by at least 1000 bars against the same update with the right
   column.  This is what the DDMPC_REFINE_OFF cases rest on: the refinement pass forms its residual with the true D(state) and
   would pull such a solve back.
"""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import ddmpc_oracle as orc

import _bounded_weights_cases as BW
import _box_warm_ref as wref
import _instance_bounds_cases as IC
import _large_box_safeguard_ref as lsref
import _large_box_warm_ref as lwref
import _large_setpoint_bounds_cases as SC
from test_gpu_large_robust_law import _windows
from test_gpu_large_weights import MUTATIONS, ramp, with_weights

INF = np.inf


def _distinct_d_s(spec, N, sol):
    on = sol.idx[sol.active != 0]
    return len(set(BW.d_s_of(spec, N, on).tolist())), int(on.size)


def _premises(tag, fixture, spec, N, sols):
    """Premises 1 and 2 of one case from the references of its rows."""
    below = 0
    for b, sol in sols.items():
        print("%s b=%d %s iters %d k %d margin %.1e" % (tag, b, sol.status, sol.iters, np.count_nonzero(sol.active), sol.margin))
        assert sol.status == "optimal", (tag, b, sol.status)
        below += sol.margin < BW.MARGIN[fixture]
    assert below * 8 <= len(sols), (tag, below)
    nd, k = _distinct_d_s(spec, N, next(iter(sols.values())))
    print("%s first row: %d active components, %d distinct d_s" % (tag, k, nd))
    assert nd >= 3, (tag, nd)


# ------------------------------------------------------------------------------------------------ 1, 2. every case
@pytest.mark.parametrize("name", list(BW.CASES))
def test_references_are_optimal_within_the_margin_cap_and_hold_distinct_d_s(name):
    c, spec, N, d = BW.case_of(name)
    assert (spec.m + spec.p) * spec.Ln == {"small": 136, "small-mp": 45, "large": 296, "large-mp": 300}[c.fixture]
    q, r = np.diag(spec.Q).reshape(spec.L, spec.p), np.diag(spec.R).reshape(spec.L, spec.m)
    if c.profile == "ramp":
        for w in (q, r):                                   # no two steps of a channel, no two channels of a step alike
            assert np.all(np.diff(w, axis=0) > 0) and np.all(np.diff(w, axis=1) > 0)
    else:                                                  # the unweighted channel carries no bound
        zq, zr = np.nonzero(np.any(q == 0.0, axis=0))[0], np.nonzero(np.any(r == 0.0, axis=0))[0]
        assert zq.size + zr.size == 1
        for ch in zq:
            assert c.ybox is None or not (np.isfinite(c.ybox[0][ch]) or np.isfinite(c.ybox[1][ch]))
        for ch in zr:
            assert c.ubox is None or not (np.isfinite(c.ubox[0][ch]) or np.isfinite(c.ubox[1][ch]))
    sols = {b: BW.reference(name, b) for b in c.rows}
    _premises(name, c.fixture, spec, N, sols)
    assert min(s.iters for s in sols.values()) >= 2        # the box acts on every row
    if BW.reduced(name):
        b = c.rows[0]
        red, full = sols[b], BW.reference(name, b, full=True)
        eu = np.max(np.abs(red.optimal_u - full.optimal_u)) / np.max(np.abs(full.optimal_u))
        ec = abs(red.cost - full.cost) / abs(full.cost)
        print("%s b=%d reduced against full space: u %.1e cost %.1e iters %d/%d margin %.1e/%.1e" %
              (name, b, eu, ec, red.iters, full.iters, red.margin, full.margin))
        assert eu < 1e-9 and ec < 1e-10 and red.iters == full.iters
        assert np.array_equal(red.idx, full.idx) and np.array_equal(red.active, full.active)


# ------------------------------------------------------------------------------------------------ 3. compositions
@pytest.mark.parametrize("name,cap", [("s-u02-convex", 9), ("s-uy2-convex", 8), ("l-ucap-convex", 9)])
def test_forced_iteration_caps_cut_at_least_two_rows(name, cap):
    c = BW.CASES[name]
    its = [BW.reference(name, b).iters for b in c.rows]
    print(name, "reference counts", its, "cap", cap)
    assert sum(i > cap for i in its) >= 2 and sum(i <= cap for i in its) >= 1


def test_large_safeguard_rows_have_an_optimal_primal_reference():
    name, cap = "l-ucap-convex", 9
    c, spec, N, d = BW.case_of(name)
    for b in c.rows:
        if BW.reference(name, b).iters <= cap:
            continue
        sol = lsref.solve_primal(spec, d["u_d"][b], d["y_d"][b], d["up"][b], d["yp"][b], dict(u=c.ubox, y=c.ybox))
        print("b=%d primal reference: %s, %d solves, largest set %d, margin %.1e" %
              (b, sol.status, sol.iters, sol.peak, sol.margin))
        assert sol.status == "optimal" and sol.peak <= 128 and sol.margin >= 1e-7


def test_capacity_case_peaks_between_64_and_256():
    """Case D of test_gpu_large_box_capacity.py under the ramp: peaks 128, 136, 130, 135 on rows 0 .. 3 (128 .. 139 over all eight
    seeds; 131 .. 139 with scalar weights), so no search for another box was needed."""
    name = "l-ytight-convex"
    peaks = [BW.reference(name, b).peak for b in BW.CASES[name].rows]
    print("peaks", peaks)
    assert all(64 < k <= 256 for k in peaks)


def test_box_law_windows_inside_and_outside_the_box():
    name = "l-uy-none"
    c, spec, N, d = BW.case_of(name)
    rows = list(c.rows)
    sup, syp = _windows(None, d["up"][rows], d["yp"][rows], spec, "setpoint")
    for i, b in enumerate(rows):
        inside = BW.solve_reduced(spec, d, b, c.ubox, c.ybox, up=sup[i], yp=syp[i])
        print("b=%d setpoint window: iters %d margin %.1e; tail: iters %d" %
              (b, inside.iters, inside.margin, BW.reference(name, b).iters))
        assert inside.status == "optimal" and inside.iters == 1 and inside.margin >= 1e-7
        assert BW.reference(name, b).iters >= 2


def test_warm_start_seeds_are_kept():
    """Up to 271 rows: the second window of the first box, seeded with the first reference's set.  Beyond: the second window of
    the reference's own loop on U_WIDE + Y_UP.  Both seeded runs end optimal without falling back, in fewer solves than from the
    empty set on some row."""
    name = "s-u02-convex"
    c, spec, N, d = BW.case_of(name)
    P = d["plant"]
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (8, 2))
    fewer = 0
    for b in c.rows:
        first = BW.reference(name, b)
        u0 = first.optimal_u[:spec.m]
        y0 = P["C"] @ d["x_end"][b] + P["D"] @ u0 + w[b]
        up2, yp2 = np.concatenate([d["up"][b][spec.m:], u0]), np.concatenate([d["yp"][b][spec.p:], y0])
        sol = wref.solve_seeded(spec, d["u_d"][b], d["y_d"][b], up2, yp2, c.ubox[0], c.ubox[1], seed=first.active)
        cold = wref.solve_seeded(spec, d["u_d"][b], d["y_d"][b], up2, yp2, c.ubox[0], c.ubox[1])
        print("small b=%d seeded %d solves (empty start %d), margin %.1e" % (b, sol.iters, cold.iters, sol.margin))
        assert sol.status == "optimal" and sol.seeded and not sol.fell_back and sol.margin >= 1e-6
        fewer += sol.iters < cold.iters
    assert fewer >= 1
    name = "l-uy-none"
    c, spec, N, d = BW.case_of(name)
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (8, 2, 2))
    fewer = 0
    for b in c.rows:
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        prob = lwref.Reduced(spec, d["u_d"][b], d["y_d"][b], dict(u=c.ubox, y=c.ybox))
        sols = lwref.closed_loop_seeded(spec, d["u_d"][b], d["y_d"][b], plant, w[b], dict(u=c.ubox, y=c.ybox), u_past=d["up"][b],
                                        y_past=d["yp"][b], max_iter=100, problem=prob)[2]
        cold = prob.solve(*sols[1].window, None, max_iter=100)
        print("large b=%d seeded %d solves (empty start %d), margin %.1e" % (b, sols[1].iters, cold.iters, sols[1].margin))
        assert len(sols) == 2 and all(s.status == "optimal" and s.margin >= 1e-7 for s in sols)
        assert sols[1].seeded and not sols[1].fell_back
        fewer += sols[1].iters < cold.iters
    assert fewer >= 1


def test_instance_bounds_rows():
    """Box C of tests/_instance_bounds_cases.py, first 8 rows, slack NONE, ramp: every row with its own bounds."""
    spec, N, d, (ulo, uhi, ylo, yhi) = BW.instance_case()
    dd, _, _ = IC.data()
    assert np.array_equal(dd["u_d"][:8], d["u_d"])         # the fixture's seeds are that module's first eight
    # the rows that differ in kind from the others: 3 and 7 have no bound on input channel 0, 5 none on output channel 1
    assert np.array_equal(np.argwhere(~np.isfinite(uhi)), [[3, 0], [7, 0]]) and np.array_equal(np.argwhere(~np.isfinite(yhi)), [[5, 1]])
    sols = {b: BW.instance_reference(b) for b in range(8)}
    _premises("instance bounds C", "small", spec, N, sols)
    assert min(s.iters for s in sols.values()) >= 2


@pytest.mark.parametrize("b", range(8))
def test_instance_bounds_loop_is_optimal_at_every_solve(b):
    """The 6-step reference loop of every row the GPU test compares: closed_loop_bounded raises unless each solve is optimal."""
    ur, yr, x_end = BW.instance_loop_reference(b)
    _, _, _, (ulo, uhi, ylo, yhi) = BW.instance_case()
    print("b=%d loop inputs in [%.3f, %.3f]" % (b, ur.min(), ur.max()))
    assert ur.shape == (6, 2) and np.all(np.isfinite(ur)) and np.all(np.isfinite(yr)) and np.all(np.isfinite(x_end))
    assert np.all(ur >= ulo[b] - 1e-12) and np.all(ur <= uhi[b] + 1e-12)


def test_setpoint_bounds_case():
    c = dict(SC.case("296/none/uy"))
    c["spec"] = with_weights(c["spec"], *ramp(c["spec"]))
    sols = {b: SC.full_reference(c, b) for b in range(c["B"])}      # every row the GPU test compares
    _premises("setpoint bounds", "large", c["spec"], c["N"], sols)


@pytest.mark.parametrize("name", ["s-mp-convex", "l-mp-convex"])
def test_m_ne_p_bounds_cut_an_input_and_an_output(name):
    c, spec, N, d = BW.case_of(name)
    assert spec.m != spec.p and np.any(d["plant"]["D"] != 0.0)
    na, nu, ny = BW.sections(spec, N)
    n_u = n_y = 0
    for b in c.rows:
        sol = BW.reference(name, b)
        on = sol.idx[sol.active != 0]
        n_u += int(np.sum((on >= na) & (on < na + nu)))
        n_y += int(np.sum((on >= na + nu) & (on < na + nu + ny)))
    print(name, "active inputs", n_u, "active outputs", n_y)
    assert n_u >= 1 and n_y >= 1


# ------------------------------------------------------------------------------------------------ 4. the mutations
@pytest.mark.parametrize("name", ["s-u02-convex", "s-uy-none", "l-ucap-convex", "l-uy-none"])
def test_each_mutation_of_a_weight_table_moves_the_reference_by_1000_bars(name):
    c, spec, N, d = BW.case_of(name)
    b = c.rows[0]
    base = BW.reference(name, b)
    q, r = ramp(BW.fixture(c.fixture, c.slack, c.tec)[0])
    for which in ("q", "r"):
        for mut, fn in MUTATIONS.items():
            qm, rm = (fn(q, spec.n), r) if which == "q" else (q, fn(r, spec.n))
            sol = BW.reference(name, b, spec=with_weights(spec, qm, rm), tag=(which, mut))
            du = np.max(np.abs(sol.optimal_u - base.optimal_u)) / np.max(np.abs(base.optimal_u))
            dc = abs(sol.cost - base.cost) / abs(base.cost)
            print("%s %s, %s: u %.1e cost %.1e" % (name, which, mut, du, dc))
            assert sol.status == "optimal" and (du >= 1e-5 or dc >= 1e-6), (name, which, mut, du, dc)


# ------------------------------------------------------------------------------------------------ 5. the box table alone
def woodbury_inputs(prob, up, yp, act, dd):
    """The inputs of the free steps (u = u_s - lam D0 beta, or the bound where held; step-major) after ONE Woodbury update of the
    kept factor
    of the empty set on the signed set `act` (table order), with `dd` as the d_s column of the k x k system: the statements of
    tests/_large_box_ref.solve_reduced's iteration, the k x k system solved by LU so that a wrong column cannot stop it."""
    t0 = prob._t0(np.asarray(up, float).reshape(-1), np.asarray(yp, float).reshape(-1))
    y = sla.solve_triangular(prob.Lf, t0[prob.perm], lower=True)
    lst = np.nonzero(act)[0]
    E = np.zeros((prob.r - prob.n0, lst.size))
    E[prob.cpos[lst] - prob.n0, np.arange(lst.size)] = 1.0
    W = np.zeros((prob.r, lst.size))
    W[prob.n0:] = sla.solve_triangular(prob.LTT, E, lower=True)
    shift = np.where(act[lst] > 0, prob.hi[lst], prob.lo[lst]) - prob.a[lst]
    WW = W.T @ W
    ev = np.linalg.solve(np.diag(1.0 / dd[lst]) - WW, W.T @ y + WW @ shift) + shift
    beta = sla.solve_triangular(prob.Lf, y + W @ ev, lower=True, trans="T")
    held = {int(prob.cpos[s]): (prob.hi[s] if act[s] > 0 else prob.lo[s]) for s in lst if not prob.cy[s]}
    u = []
    for i in range(prob.r):
        rho = int(prob.perm[i])
        kind, ch, kp = prob.kinds[rho]
        if kind == "ufree":                                # a held input sits on its bound, a free one follows beta
            u.append((rho, held[i] if i in held else prob.u_s[ch] - prob.lam * prob.D0[rho] * beta[i]))
    return np.array([v for _, v in sorted(u)])


@pytest.mark.parametrize("name", ["l-ucap-convex", "l-uy-none", "l-uch0-none"])
def test_a_rolled_d_s_column_alone_moves_the_inputs_by_1000_bars(name):
    c, spec, N, d = BW.case_of(name)
    b = c.rows[0]
    sol = BW.reference(name, b)
    prob = lwref.Reduced(spec, d["u_d"][b], d["y_d"][b], dict(u=c.ubox, y=c.ybox))
    act = prob.table_set(sol)
    lst = np.nonzero(act)[0]
    right = woodbury_inputs(prob, d["up"][b], d["yp"][b], act, prob.dd)
    free = sol.optimal_u[:right.size]                      # (the free steps come first; the terminal ones are fixed to u_s)
    e0 = np.max(np.abs(right - free)) / np.max(np.abs(free))
    rolled = prob.dd.copy()
    rolled[lst] = np.roll(prob.dd[lst], 1)
    assert np.count_nonzero(rolled[lst] != prob.dd[lst]) >= 3
    wrong = woodbury_inputs(prob, d["up"][b], d["yp"][b], act, rolled)
    e1 = np.max(np.abs(wrong - right)) / np.max(np.abs(right))
    print("%s b=%d k %d: the update with the right column is %.1e from the reference, with the rolled one %.1e from the right one" %
          (name, b, lst.size, e0, e1))
    assert e0 < 1e-8                                       # the restated update is the reference's
    assert e1 >= 1e-5, e1
