"""The yardstick of the output-bound tests (tests/_output_bounds_ref.py) against a numpy statement of the reduced table the
kernels iterate on: the output of a free prediction row as a third kind of boxed component next to the slack and the
input, two components on one row under the CONVEX slack box.  On the CPU.

Reduced system (oracle/reduced_form.py, stacking z = [ubar; ybar + sigma]): K0 = G + lam D0, t0 of the empty active set; a
component s on row rho has hat_s = a_s + c_s beta_rho, bounds lo_s / hi_s, and when active changes K by -d_s e_rho e_rho' and t by
(bound - a_s) e_rho:
    slack   a = 0,    c = -lam / lamb_sigma,  lo / hi = -+ c eps_max,  d = lam / lamb_sigma
    input   a = u_s,  c = -lam / r,           lo / hi = u_min / u_max,  d = lam / r
    output  a = y_s,  c = -lam / q,           lo / hi = y_min / y_max,  d = lam / q
"""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc
from oracle import reduced_form as rf

import _output_bounds_ref as yref

INF = np.inf
TWO_SIDED = ([0.60, 0.72], [0.70, 0.82])
COMBINED = dict(y=([0.55, 0.65], [0.72, 0.85]), u=(-4.0, 6.0))
MODES = {"convex-tec": (1, True), "convex": (1, False), "none": (0, False)}

_CACHE = {}


def _instance(seed, n=4):
    if seed not in _CACHE:
        d = orc.generate_instance(seed)
        _CACHE[seed] = (d["u_d"], d["y_d"], d["u_d"][-n:].reshape(-1), d["y_d"][-n:].reshape(-1))
    return _CACHE[seed]


def solve_reduced_table(spec, u_d, y_d, u_past, y_past, y_min, y_max, u_min=None, u_max=None, max_iter=100):
    """The primal-dual active set over the table above, one dense solve of K(A) beta = t(A) per iteration.  Returns the solve
    count, the signed set keyed by the position of the component in x = [alpha; ubar; ybar; sigma], x and the cost."""
    n, m, p, L, Ln = spec.n, spec.m, spec.p, spec.L, spec.Ln
    H = np.vstack([orc.hankel_matrix(u_d, Ln), orc.hankel_matrix(y_d, Ln)])
    G = H @ H.T
    lam, ls = spec.lamb_alpha * spec.eps_max, spec.lamb_sigma
    convex = spec.slack == "convex"
    bound = spec.c * spec.eps_max
    act0 = np.zeros(L * p, dtype=int)
    D0, t0 = rf.component_tables(spec, u_past, y_past, act0)
    rdiag, qdiag = np.diag(spec.R), np.diag(spec.Q)
    u_s, y_s = np.asarray(spec.u_s, float).reshape(-1), np.asarray(spec.y_s, float).reshape(-1)
    nfree = L - n if spec.tec else L
    na, nu, ny = H.shape[1], Ln * m, Ln * p
    y_min, y_max = np.broadcast_to(np.asarray(y_min, float), (p,)), np.broadcast_to(np.asarray(y_max, float), (p,))
    comps = []                                          # (row, a, c, lo, hi, d, position in x, kind)
    if convex:
        for kp in range(L):
            for ch in range(p):
                comps.append((nu + (n + kp) * p + ch, 0.0, -lam / ls, -bound, bound, lam / ls, na + nu + ny + (n + kp) * p + ch, "s"))
    if u_min is not None:
        lo, hi = np.broadcast_to(np.asarray(u_min, float), (m,)), np.broadcast_to(np.asarray(u_max, float), (m,))
        for kp in range(nfree):
            for ch in range(m):
                if np.isfinite(lo[ch]) or np.isfinite(hi[ch]):
                    r_ = rdiag[kp * m + ch]
                    comps.append(((n + kp) * m + ch, u_s[ch], -lam / r_, lo[ch], hi[ch], lam / r_, na + (n + kp) * m + ch, "u"))
    for kp in range(nfree):
        for ch in range(p):
            if np.isfinite(y_min[ch]) or np.isfinite(y_max[ch]):
                q_ = qdiag[kp * p + ch]
                comps.append((nu + (n + kp) * p + ch, y_s[ch], -lam / q_, y_min[ch], y_max[ch], lam / q_, na + nu + (n + kp) * p + ch, "y"))
    rows = np.array([c[0] for c in comps])
    a, c, lo, hi, d = (np.array([cc[i] for cc in comps], float) for i in range(1, 6))
    K0 = G + lam * np.diag(D0)
    act = np.zeros(len(comps), dtype=int)
    beta = np.linalg.solve(K0, t0)
    iters, status = 1, "optimal"
    while True:
        hat = a + c * beta[rows]
        new = np.where(act > 0, (hat > hi).astype(int), np.where(act < 0, -(hat < lo).astype(int), (hat > hi).astype(int) - (hat < lo)))
        if np.array_equal(new, act):
            break
        act = new
        if iters >= max_iter:
            status = "solver_error"
            break
        iters += 1
        K, t = K0.copy(), t0.copy()
        for s in np.nonzero(act)[0]:
            K[rows[s], rows[s]] -= d[s]
            t[rows[s]] += (hi[s] if act[s] > 0 else lo[s]) - a[s]
        beta = np.linalg.solve(K, t)
    # the variables from beta and the final set
    z = G @ beta
    ubar, w = z[:nu].copy(), z[nu:]
    ybar, sigma = np.zeros(ny), np.zeros(ny)
    yp = np.asarray(y_past, float).reshape(-1)
    ybar[:n * p], sigma[:n * p] = yp, w[:n * p] - yp
    state = {(cc[0], cc[7]): (s, act[s]) for s, cc in enumerate(comps)}
    for s, cc in enumerate(comps):
        if cc[7] == "u" and act[s]:
            ubar[cc[0]] = hi[s] if act[s] > 0 else lo[s]
    both = 0
    for kp in range(L):
        for ch in range(p):
            i = (n + kp) * p + ch
            b_ = beta[nu + i]
            if spec.tec and kp >= L - n:
                ybar[i], sigma[i] = y_s[ch], w[i] - y_s[ch]
                continue
            ss, sa = state.get((nu + i, "s"), (None, 0))
            sy, say = state.get((nu + i, "y"), (None, 0))
            sigma[i] = sa * bound if sa else -lam * b_ / ls
            ybar[i] = (hi[sy] if say > 0 else lo[sy]) if say else y_s[ch] - lam * b_ / qdiag[kp * p + ch]
            both += bool(sa and say)
    alpha = H.T @ beta
    du = ubar[n * m:] - np.tile(u_s, L)
    dy = ybar[n * p:] - np.tile(y_s, L)
    cost = float(du @ (rdiag * du) + dy @ (qdiag * dy) + lam * beta @ (G @ beta) + ls * sigma @ sigma)
    signed = {cc[6]: int(act[s]) for s, cc in enumerate(comps)}
    return dict(status=status, iters=iters, signed=signed, x=np.concatenate([alpha, ubar, ybar, sigma]), cost=cost,
                optimal_u=ubar[n * m:].copy(), both=both)


@pytest.mark.parametrize("box", ["two-sided", "combined"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("seed", [500, 501, 502, 503])
def test_reduced_table_is_the_full_space_iteration(seed, mode, box):
    slack, tec = MODES[mode]
    spec = orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)
    u_d, y_d, up, yp = _instance(seed)
    if box == "two-sided":
        kw = dict(y_min=TWO_SIDED[0], y_max=TWO_SIDED[1])
    else:
        kw = dict(y_min=COMBINED["y"][0], y_max=COMBINED["y"][1], u_min=COMBINED["u"][0], u_max=COMBINED["u"][1])
    sol = yref.solve_bounded(spec, u_d, y_d, up, yp, **kw)
    red = solve_reduced_table(spec, u_d, y_d, up, yp, **kw)
    eu = np.max(np.abs(red["optimal_u"] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(red["cost"] - sol.cost) / abs(sol.cost)
    print("%s %s seed %d: %s iters %d/%d k %d both %d margin %.1e err_u %.1e err_cost %.1e" %
          (mode, box, seed, sol.status, red["iters"], sol.iters, np.count_nonzero(sol.active), red["both"], sol.margin, eu, ec))
    assert red["status"] == sol.status == "optimal"
    assert red["iters"] == sol.iters
    assert np.array_equal(np.array([red["signed"][int(i)] for i in sol.idx]), sol.active)
    assert eu < 1e-8 and ec < 1e-9, (eu, ec)
    if box == "two-sided" and slack:
        assert red["both"] >= 1                         # a row with its slack and its output at their bounds
    # the helper's certificate on both solutions
    for x in (sol.x, red["x"]):
        cert = yref.kkt_certificate(spec, u_d, y_d, up, yp, kw["y_min"], kw["y_max"], x, u_min=kw.get("u_min"), u_max=kw.get("u_max"))
        tol = 1e-9 * cert["grad_scale"]
        assert cert["res_eq"] < tol and cert["res_box"] < tol and cert["res_stat"] < tol and cert["dual_sign"] < tol, cert


def test_infinite_output_bounds_are_the_input_bound_helper():
    import _input_bounds_ref as ref
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    u_d, y_d, up, yp = _instance(500)
    a = ref.solve_bounded(spec, u_d, y_d, up, yp, 0.0, 2.0)
    b = yref.solve_bounded(spec, u_d, y_d, up, yp, -INF, INF, u_min=0.0, u_max=2.0)
    assert np.array_equal(a.x, b.x) and a.iters == b.iters and np.array_equal(a.active, b.active) and np.array_equal(a.idx, b.idx)
    assert ref.box_of is yref._INPUT_BOX_OF             # the helper is left as it was
