"""Reference solution of the Data-Driven MPC QP with input bounds u_min <= ubar[k] <= u_max on the free prediction steps.

A helper, not a test.  The full-space problem is `oracle.ddmpc_oracle.build_fullspace_qp` as it is; the box is the union of its
`box_idx` (the slack components of a CONVEX controller) and the entries of ubar[n*m:] on the free prediction steps (all L of
them, or the first L - n with the terminal constraint) of the channels with a finite bound, each with its own lo / hi.  The
iteration is the oracle's primal-dual active set (`solve_fullspace`) over that union: from the empty set, keep a bound while
its multiplier has the right sign, add one when the free value violates it, stop when the set repeats.

`margin` says how far the run was from deciding differently: the smaller of
  * the smallest distance of an inactive boxed value to its nearer finite bound, relative to the size of that component's box
    (the larger of its finite |lo|, |hi|), and
  * min |mu| / max |mu| over the active set,
taken over all iterations.  A run with a tiny margin may legitimately differ in iteration count or active set between two
correct implementations.
"""
from dataclasses import dataclass
from typing import Dict

import numpy as np

from oracle import ddmpc_oracle as orc


@dataclass
class BoundedSolution:
    status: str
    x: np.ndarray
    cost: float
    optimal_u: np.ndarray
    ubar: np.ndarray
    ybar: np.ndarray
    sigma: np.ndarray
    alpha: np.ndarray
    iters: int
    idx: np.ndarray                 # positions in x of the boxed components, ascending
    lo: np.ndarray
    hi: np.ndarray
    active: np.ndarray              # signed active set over idx
    margin: float


def box_of(spec, qp, u_min, u_max):
    """(idx, lo, hi) of the union box; components without a finite bound on either side are left out."""
    n, m, L = spec.n, spec.m, spec.L
    u_min = np.broadcast_to(np.asarray(u_min, float), (m,))
    u_max = np.broadcast_to(np.asarray(u_max, float), (m,))
    idx = [int(i) for i in qp.box_idx]
    lo = [-qp.bound] * len(idx)
    hi = [qp.bound] * len(idx)
    u0 = qp.sl["ubar"].start
    nfree = L - n if spec.tec else L
    for k in range(nfree):
        for ch in range(m):
            if np.isfinite(u_min[ch]) or np.isfinite(u_max[ch]):
                idx.append(u0 + (n + k) * m + ch)
                lo.append(float(u_min[ch]))
                hi.append(float(u_max[ch]))
    order = np.argsort(idx)
    return np.asarray(idx, int)[order], np.asarray(lo, float)[order], np.asarray(hi, float)[order]


def solve_bounded(spec, u_d, y_d, u_past, y_past, u_min, u_max, max_iter: int = 100) -> BoundedSolution:
    qp = orc.build_fullspace_qp(spec, u_d, y_d, u_past, y_past)
    idx, lo, hi = box_of(spec, qp, u_min, u_max)
    nx, nb, ne = qp.P.shape[0], idx.size, qp.A.shape[0]
    scale = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    act = np.zeros(nb, dtype=int)
    status, iters, margin = orc.OPTIMAL, 0, np.inf
    if nb == 0:
        x, _ = orc._kkt_solve(qp.P, qp.q, qp.A, qp.b)
    else:
        x = None
        for iters in range(1, max_iter + 1):
            a = np.nonzero(act)[0]
            Eb = np.zeros((a.size, nx))
            Eb[np.arange(a.size), idx[a]] = 1.0
            val = np.where(act > 0, hi, lo)
            x, nu = orc._kkt_solve(qp.P, qp.q, np.vstack([qp.A, Eb]), np.concatenate([qp.b, val[a]]))
            mu = np.zeros(nb)
            mu[a] = nu[ne:]
            v = x[idx]
            new = np.zeros(nb, dtype=int)
            new[(act == 1) & (mu > 0)] = 1
            new[(act == -1) & (mu < 0)] = -1
            new[(act == 0) & (v > hi)] = 1
            new[(act == 0) & (v < lo)] = -1
            free = act == 0
            if np.any(free):
                d = np.minimum(np.where(np.isfinite(hi), np.abs(v - hi), np.inf), np.where(np.isfinite(lo), np.abs(v - lo), np.inf))
                margin = min(margin, float(np.min(d[free] / scale[free])))
            if a.size:
                margin = min(margin, float(np.min(np.abs(mu[a])) / max(np.max(np.abs(mu[a])), 1e-300)))
            if np.array_equal(new, act):
                break
            act = new
        else:
            status = orc.SOLVER_ERROR
    if not np.all(np.isfinite(x)):
        status = orc.SOLVER_ERROR
    sl = qp.sl
    ubar = x[sl["ubar"]]
    return BoundedSolution(status=status, x=x, cost=float(x @ qp.P @ x + qp.q @ x + qp.const), optimal_u=ubar[spec.n * spec.m:].copy(),
                           ubar=ubar, ybar=x[sl["ybar"]], sigma=x[sl["sigma"]], alpha=x[sl["alpha"]], iters=iters, idx=idx, lo=lo,
                           hi=hi, active=act, margin=float(margin))


def kkt_certificate(spec, u_d, y_d, u_past, y_past, u_min, u_max, x, act_tol: float = 1e-9) -> Dict[str, float]:
    """Solver-independent optimality certificate of `x` for the bounded problem: equality and box residuals, the stationarity
    residual with multipliers fitted by least squares on the constraints active at `x`, the worst wrong-signed bound multiplier."""
    qp = orc.build_fullspace_qp(spec, u_d, y_d, u_past, y_past)
    idx, lo, hi = box_of(spec, qp, u_min, u_max)
    v = x[idx]
    res_eq = float(np.max(np.abs(qp.A @ x - qp.b)))
    res_box = float(np.max(np.maximum(np.maximum(v - hi, lo - v), 0.0))) if idx.size else 0.0
    up = np.nonzero(v >= hi - act_tol)[0]
    dn = np.nonzero(v <= lo + act_tol)[0]
    a = np.concatenate([up, dn])
    Eb = np.zeros((a.size, x.size))
    Eb[np.arange(a.size), idx[a]] = 1.0
    G = np.vstack([qp.A, Eb]).T
    g = -(2.0 * qp.P @ x + qp.q)
    mult = np.linalg.lstsq(G, g, rcond=None)[0]
    res_stat = float(np.max(np.abs(G @ mult - g)))
    mu = mult[qp.A.shape[0]:]
    bad = 0.0
    if up.size:
        bad = max(bad, float(np.max(np.maximum(-mu[:up.size], 0.0))))
    if dn.size:
        bad = max(bad, float(np.max(np.maximum(mu[up.size:], 0.0))))
    return dict(res_eq=res_eq, res_box=res_box, res_stat=res_stat, dual_sign=bad, grad_scale=float(np.max(np.abs(g))))


def closed_loop_bounded(spec, u_d, y_d, plant, w_sys, u_min, u_max, n_mpc_step=1, u_past=None, y_past=None):
    """`oracle.ddmpc_oracle.closed_loop` with the bounded solve."""
    n, m, p = spec.n, spec.m, spec.p
    n_steps = w_sys.shape[0]
    up = (u_d[-n:].reshape(-1) if u_past is None else np.asarray(u_past, float).reshape(-1)).copy()
    yp = (y_d[-n:].reshape(-1) if y_past is None else np.asarray(y_past, float).reshape(-1)).copy()
    u_sys, y_sys = np.zeros((n_steps, m)), np.zeros((n_steps, p))
    for t in range(0, n_steps, n_mpc_step):
        sol = solve_bounded(spec, u_d, y_d, up, yp, u_min, u_max)
        if sol.status != orc.OPTIMAL:
            raise ValueError("MPC problem was not solved optimally.")
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = sol.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w_sys[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys
