"""CPU: a numpy model of the algorithm of DDMPC_OPT_SETPOINT_BOX_LAW against the full-space helper, and the premises the GPU
tests of tests/test_gpu_setpoint_box_law.py rest on (every reference solve optimal, the margins that let `iters` and the active
set be compared, both homes of the k x k system hit, the setpoint switch visible in the active count).

The model is what csrc/ddmpc_setpoint_box_law.hpp computes: beta0 = past P + s S with (P, S) of `_setpoint_law_ref.law`;
M = K0^-1 E_box; per-instance offsets a_s = s[channel of s]; the iteration rule of BoxTab::test from the empty set; the output
stage with the instance's setpoint as target.  Bars: TOL_U / TOL_COST of the GPU suites.
"""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc
from oracle import reduced_form as rf

import _setpoint_box_ref as ref
import _setpoint_law_ref as sref

TOL_U, TOL_COST = 1e-8, 1e-9
INF = np.inf


def model_step(spec, u_d, y_d, u_past, y_past, u_s, y_s, u_min=None, u_max=None, y_min=None, y_max=None, max_iter=100):
    """-> (optimal_u, cost, status, iters, signed set by boxed component, rows of the components)."""
    n, m, p, L, Ln = spec.n, spec.m, spec.p, spec.L, spec.Ln
    nch = m + p
    nat = sref.natural_of_internal(spec)
    sp = sref.with_setpoints(spec, u_s, y_s)
    K0, G, lamD = sref.reduced_matrix(spec, u_d, y_d)
    P, S = sref.law(spec, u_d, y_d)
    lam = spec.lamb_alpha * spec.eps_max
    s = np.concatenate([sp.u_s, sp.y_s])
    past = np.concatenate([np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)])
    beta0 = past @ P + s @ S
    lo_ch = np.concatenate([np.broadcast_to(-INF if u_min is None else np.asarray(u_min, float), (m,)),
                            np.broadcast_to(-INF if y_min is None else np.asarray(y_min, float), (p,))])
    hi_ch = np.concatenate([np.broadcast_to(INF if u_max is None else np.asarray(u_max, float), (m,)),
                            np.broadcast_to(INF if y_max is None else np.asarray(y_max, float), (p,))])
    nfree = L - n if spec.tec else L
    qd = np.diag(spec.Q)
    rows, a, c, lo, hi, invd = [], [], [], [], [], []
    for rho in range(Ln * nch):
        k, ch = divmod(rho, nch)
        if not (n <= k < n + nfree) or not (np.isfinite(lo_ch[ch]) or np.isfinite(hi_ch[ch])):
            continue
        # input: hat = u_s - lam D0 beta, d = lam D0;  output: hat = y_s - lam beta / q, d = lam / q
        d = lamD[rho] if ch < m else lam / qd[(k - n) * p + (ch - m)]
        rows.append(rho); a.append(s[ch]); c.append(-d); lo.append(lo_ch[ch]); hi.append(hi_ch[ch]); invd.append(1.0 / d)
    rows = np.asarray(rows, int)
    a, c, lo, hi, invd = (np.asarray(v, float) for v in (a, c, lo, hi, invd))
    E = np.zeros((Ln * nch, rows.size))
    E[rows, np.arange(rows.size)] = 1.0
    M = np.linalg.solve(K0, E)                                 # [r, nbox]

    def test(beta_rows, act):
        hat = a + c * beta_rows
        up, dn = hat > hi, hat < lo
        return np.where(act > 0, up.astype(int), np.where(act < 0, -dn.astype(int), up.astype(int) - dn.astype(int)))

    act = np.zeros(rows.size, dtype=int)
    beta, iters, status = beta0.copy(), 1, 0
    while True:
        new = test(beta[rows], act)
        if np.array_equal(new, act):
            break
        act = new
        if iters >= max_iter:
            status = 4
            break
        iters += 1
        A = np.nonzero(act)[0]
        shift = np.where(act[A] > 0, hi[A], lo[A]) - a[A]
        MAA = M[np.ix_(rows[A], A)]
        ev = shift + np.linalg.solve(np.diag(invd[A]) - MAA, beta0[rows[A]] + MAA @ shift)
        beta = beta0 + M[:, A] @ ev
    # output stage (natural stacking), the instance's setpoint as target
    t = rf.component_tables(sp, u_past, y_past)[1][nat]
    z_int = t - lamD * beta
    bnat = np.empty_like(beta); bnat[nat] = beta
    sigma = np.zeros(Ln * p)
    sigma[n * p:] = -lam * bnat[Ln * m + n * p:] / spec.lamb_sigma
    held = {}
    for j in np.nonzero(act)[0]:
        rho = rows[j]
        bd = hi[j] if act[j] > 0 else lo[j]
        ch = rho % nch
        if ch < m:
            z_int[rho] = bd
        else:                                                 # ybar = bound, w = bound + sigma
            held[nat[rho] - Ln * m] = bd
    z = np.empty_like(z_int); z[nat] = z_int
    ubar, w = z[:Ln * m].copy(), z[Ln * m:].copy()
    for i, bd in held.items():
        w[i] = bd + sigma[i]
    sigma[:n * p] = w[:n * p] - np.asarray(y_past, float).reshape(-1)
    if spec.tec:
        sigma[L * p:] = w[L * p:] - np.tile(sp.y_s, n)
    ybar = w - sigma
    du = ubar[n * m:] - np.tile(sp.u_s, L)
    dy = ybar[n * p:] - np.tile(sp.y_s, L)
    cost = float(du @ (np.diag(spec.R) * du) + dy @ (np.diag(spec.Q) * dy) + lam * beta @ (G @ beta) + spec.lamb_sigma * sigma @ sigma)
    return ubar[n * m:].copy(), cost, status, iters, act, rows


def _model_vs_helper(spec, inst, b, us, ys, **box):
    u_d, y_d, up, yp = inst["u_d"][b], inst["y_d"][b], inst["up"][b], inst["yp"][b]
    sol = ref.solve(spec, u_d, y_d, up, yp, us, ys, **box)
    u, cost, status, iters, act, rows = model_step(spec, u_d, y_d, up, yp, us, ys, **box)
    assert sol.status == "optimal" and status == 0
    # the helper lists the box in the order of x = [alpha; ubar; ybar; sigma]: the inputs, then the outputs, each by time
    k, ch = np.divmod(rows, spec.m + spec.p)
    act = act[np.lexsort((ch, k, ch >= spec.m))]
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    if sol.margin >= 1e-7:
        assert iters == sol.iters and np.array_equal(act, sol.active), (b, iters, sol.iters)
    return sol


@pytest.mark.parametrize("tec", [True, False], ids=["terminal", "no-terminal"])
@pytest.mark.parametrize("box", list(ref.STEP_BOXES))
def test_model_against_the_helper_and_step_premises(box, tec):
    spec = ref.spec(tec)
    inst = ref.tank()
    lo, hi, home = ref.STEP_BOXES[box]
    ks, left_out = [], 0
    for b in range(ref.B8):
        sol = ref.step_reference(box, tec, False, b)
        assert sol.status == "optimal"
        left_out += sol.margin < 1e-7
        ks.append(int(np.count_nonzero(sol.active)))
        if b in (0, 5):                                         # the model on two instances per cell
            _model_vs_helper(spec, inst, b, inst["us"][b], inst["ys"][b], u_min=lo, u_max=hi)
    print(box, tec, "active counts", ks, "left out", left_out)
    assert left_out * 16 <= ref.B8
    if home == "lds":
        assert 1 <= min(ks) and max(ks) <= 16, ks
    if home == "global":
        assert min(ks) > 16, ks


def test_model_with_output_bounds_and_premises():
    inst = ref.tank()
    for name, (tec, box) in ref.Y_CASES.items():
        spec = ref.spec(tec)
        left_out = 0
        for b in range(ref.B8):
            sol = ref.y_reference(name, b)
            assert sol.status == "optimal" and np.count_nonzero(sol.active) >= 1, (name, b)
            left_out += sol.margin < 1e-7
        assert left_out * 16 <= ref.B8, (name, left_out)
        _model_vs_helper(spec, inst, 1, inst["us"][1], inst["ys"][1], **box)


def test_setpoint_outside_the_box_without_the_terminal_constraint():
    spec = ref.spec(False)
    inst = ref.tank()
    us, ys = ref.outside_setpoints(inst)
    at_lo = at_hi = False
    for b in ref.OUTSIDE:
        sol = _model_vs_helper(spec, inst, b, us[b], ys[b], u_min=[0.0, 0.0], u_max=[2.0, 2.0])
        assert sol.margin >= 1e-7
        at_lo |= bool(np.any(sol.active < 0)); at_hi |= bool(np.any(sol.active > 0))
    assert at_lo and at_hi                                      # inputs at both bounds
