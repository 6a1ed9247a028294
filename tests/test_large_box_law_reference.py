"""DDMPC_OPT_LARGE_BOX_LAW (ddmpc_rr3_box_law.hpp, DESIGN 5.5.2 "Law inside the box"), on the CPU: the step rule restated in numpy,
and the premises of tests/test_gpu_large_box_law.py where they can be checked without a GPU.

The rule: beta(w) = g0 + G' w is the law of the EMPTY active set (K0^-1 applied to t0 and to the unit windows, from the reduced
form of oracle/reduced_form.py); a step is served by the law when no component of the box table -- slack sigma_hat = -lam beta /
lamb_sigma, input u_hat = u_s - lam beta / r, output y_hat = y_s - lam beta / q, each strictly outside its lo / hi -- is violated,
which is the first test of the bounded kernels.  Against the full-space helper tests/_output_bounds_ref.solve_bounded:

  * "the law violates nothing"  <=>  the helper stops after one solve (iters == 1);
  * where it violates nothing, optimal_u and the cost from the law equal the helper's to 1e-10 relative;
  * the fixture's table -- margins, solve counts and active components of the two window families under the three boxes.

Fixture (that of tests/test_gpu_large_bounds.py): four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7; "tail" windows are the
last n rows of the data, "setpoint" windows those of tests/test_gpu_large_robust_law.py (seed 0, offsets 1e-3)."""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc
from oracle import reduced_form as rf

import _output_bounds_ref as yref

INF = np.inf
B8, LH, N = 8, 70, 700
U_WIDE = ([-4.0, -4.0], [6.0, 6.0])
Y_UP = ([-INF, -INF], [0.66, 0.775])
U_CAP = ([0.0, 0.0], [2.0, 2.0])
BOXES = {"u_wide": (U_WIDE, None), "y_up": (None, Y_UP), "u_cap": (U_CAP, None)}
# per box: margin of the setpoint windows; solve counts, active components at the optimum and margin of the tail windows
TABLE = {"u_wide": dict(set_margin=0.8, tail_iters=(4, 5), tail_active=(6, 10), tail_margin=1e-3),
         "y_up": dict(set_margin=2e-3, tail_iters=(2, 4), tail_active=(18, 32), tail_margin=4e-5),
         "u_cap": dict(set_margin=0.3, tail_iters=(8, 12), tail_active=(45, 71), tail_margin=2e-6)}
SLACKS = ("none", "convex")
FAMILIES = ("setpoint", "tail")

_DATA, _REF, _LAW = {}, {}, {}


def fixture(slack):
    """(spec, data, tail windows) of the four-tank at 296 rows, batch 8."""
    if slack not in _DATA:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=LH)
        d = harness.generate_batch(range(B8), N=N)
        n = spec.n
        _DATA[slack] = (spec, d, d["u_d"][:, -n:, :].reshape(B8, -1).copy(), d["y_d"][:, -n:, :].reshape(B8, -1).copy())
    return _DATA[slack]


def windows(slack, family):
    """Past windows of a family: the data tail, or small offsets (1e-3, seed 0) from [u_s; y_s]."""
    spec, d, up, yp = fixture(slack)
    if family == "tail":
        return up, yp
    rng = np.random.default_rng(0)
    us = np.tile(np.asarray(spec.u_s, dtype=float), spec.n)
    ys = np.tile(np.asarray(spec.y_s, dtype=float), spec.n)
    return us[None, :] + 1e-3 * rng.standard_normal((B8, us.size)), ys[None, :] + 1e-3 * rng.standard_normal((B8, ys.size))


def reference(slack, box, family, b):
    """The helper's solution of instance b, computed once."""
    key = (slack, box, family, b)
    if key not in _REF:
        spec, d, _, _ = fixture(slack)
        up, yp = windows(slack, family)
        ubox, ybox = BOXES[box]
        ylo, yhi = ybox if ybox is not None else (-INF, INF)
        kw = dict(u_min=ubox[0], u_max=ubox[1]) if ubox is not None else {}
        _REF[key] = yref.solve_bounded(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], ylo, yhi, **kw)
    return _REF[key]


def law_of(spec, u_d, y_d):
    """(law [r][nf + 1], D0): column 0 = K0^-1 t0, column 1 + j = K0^-1 (the target of the unit window e_j), natural stacking."""
    n, m, p = spec.n, spec.m, spec.p
    H = np.vstack([orc.hankel_matrix(u_d, spec.Ln), orc.hankel_matrix(y_d, spec.Ln)])
    lam = spec.lamb_alpha * spec.eps_max
    zu, zy = np.zeros(n * m), np.zeros(n * p)
    D0, t0 = rf.component_tables(spec, zu, zy)
    cols = [t0]
    for j in range(n * (m + p)):
        e = np.zeros(n * (m + p))
        e[j] = 1.0
        cols.append(rf.component_tables(spec, e[:n * m], e[n * m:])[1] - t0)
    K0 = H @ H.T + lam * np.diag(D0)
    Lc = np.linalg.cholesky(K0)
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.stack(cols, axis=1))), D0, H


def law_step(spec, law, D0, H, u_past, y_past, ubox, ybox):
    """The step rule: (served by the law?, optimal_u, cost) -- the outputs are those of the empty active set."""
    n, m, p, Lh, Ln = spec.n, spec.m, spec.p, spec.L, spec.Ln
    lam, ls = spec.lamb_alpha * spec.eps_max, spec.lamb_sigma
    w = np.concatenate([np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)])
    beta = law[:, 0] + law[:, 1:] @ w
    _, t = rf.component_tables(spec, u_past, y_past)
    z = t - lam * D0 * beta
    nfree = Lh - n if spec.tec else Lh
    rd, qd = np.diag(spec.R), np.diag(spec.Q)
    u_s, y_s = np.asarray(spec.u_s, float).reshape(-1), np.asarray(spec.y_s, float).reshape(-1)
    out = False
    if spec.slack == "convex":                                              # every slack of the prediction window
        sh = -lam * beta[Ln * m + n * p:] / ls
        out |= bool(np.any((sh > spec.c * spec.eps_max) | (sh < -spec.c * spec.eps_max)))
    for kp in range(nfree):
        for ch in range(m):
            if ubox is not None:
                hat = u_s[ch] - lam * beta[(n + kp) * m + ch] / rd[kp * m + ch]
                out |= bool(hat > ubox[1][ch] or hat < ubox[0][ch])
        for ch in range(p):
            if ybox is not None:
                hat = y_s[ch] - lam * beta[Ln * m + (n + kp) * p + ch] / qd[kp * p + ch]
                out |= bool(hat > ybox[1][ch] or hat < ybox[0][ch])
    ubar, wv = z[:Ln * m], z[Ln * m:]
    sigma = np.zeros(Ln * p)
    sigma[:n * p] = wv[:n * p] - np.asarray(y_past, float).reshape(-1)
    sigma[n * p:] = -lam * beta[Ln * m + n * p:] / ls
    if spec.tec:
        sigma[Lh * p:] = wv[Lh * p:] - np.tile(y_s, n)
    ybar = wv - sigma
    du, dy = ubar[n * m:] - np.tile(u_s, Lh), ybar[n * p:] - np.tile(y_s, Lh)
    cost = float(du @ (rd * du) + dy @ (qd * dy) + lam * beta @ (H @ (H.T @ beta)) + ls * sigma @ sigma)
    return (not out), ubar[n * m:].copy(), cost


def _sig1(v):
    """A margin at the one significant digit the fixture's table states its figures to (0.77 reads 0.8 there)."""
    return float("%.0e" % v)


def law(slack, b):
    if (slack, b) not in _LAW:
        spec, d, _, _ = fixture(slack)
        _LAW[(slack, b)] = law_of(spec, d["u_d"][b], d["y_d"][b])
    return _LAW[(slack, b)]


@pytest.mark.parametrize("slack", SLACKS)
@pytest.mark.parametrize("box", list(BOXES))
def test_the_law_serves_exactly_the_steps_the_helper_ends_after_one_solve(box, slack):
    spec, d, _, _ = fixture(slack)
    ubox, ybox = BOXES[box]
    row = TABLE[box]
    for family in FAMILIES:
        up, yp = windows(slack, family)
        for b in range(B8):
            sol = reference(slack, box, family, b)
            g, D0, H = law(slack, b)
            inside, u, cost = law_step(spec, g, D0, H, up[b], yp[b], ubox, ybox)
            k = int(np.count_nonzero(sol.active))
            eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
            ec = abs(cost - sol.cost) / abs(sol.cost)
            print("%s %s %s b=%d: %s iters %d k %d margin %.1e inside %d err_u %.1e err_cost %.1e" %
                  (box, slack, family, b, sol.status, sol.iters, k, sol.margin, inside, eu, ec))
            assert sol.status == "optimal" and sol.margin >= 1e-7, (b, sol.status, sol.margin)
            assert inside == (sol.iters == 1), (b, inside, sol.iters)
            if inside:
                assert eu <= 1e-10 and ec <= 1e-10, (b, eu, ec)
            if family == "setpoint":
                assert sol.iters == 1 and _sig1(sol.margin) >= row["set_margin"], (b, sol.iters, sol.margin)
            else:
                assert row["tail_iters"][0] <= sol.iters <= row["tail_iters"][1], (b, sol.iters)
                assert row["tail_active"][0] <= k <= row["tail_active"][1], (b, k)
                assert _sig1(sol.margin) >= row["tail_margin"], (b, sol.margin)
