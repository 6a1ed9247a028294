"""numpy reference of the setpoint-parametric affine law (DDMPC_OPT_SETPOINT_LAW), shared by the CPU and the GPU tests.

The reduced system K0 beta = t of oracle/reduced_form.py is linear in t, and t is linear in the setpoints: a component that
takes its target from a setpoint (every prediction step) has t_i = s[channel of i], s = [u_s; y_s].  So

    beta = sum_f past[f] P[f, :] + sum_c s[c] S[c, :],     P[f, :] = K0^-1 e_(row of past entry f),   S[c, :] = K0^-1 1_c,

with 1_c the multi-hot vector of the setpoint components of channel c.  Everything here is stated on
`oracle.reduced_form.component_tables`; rows are in the library's internal order rho = k (m + p) + ch (ch < m: ubar, else
ybar + sigma), the order of `BatchedDDMPC.gain()` and `setpoint_gain()`.
"""
import dataclasses

import numpy as np

from oracle import ddmpc_oracle as orc
from oracle import reduced_form as rf


def natural_of_internal(spec):
    """nat[rho] = index in the natural stacking z = [ubar (Ln m); w (Ln p)] of the internal row rho = k (m + p) + ch."""
    m, p, Ln = spec.m, spec.p, spec.Ln
    nat = np.empty(Ln * (m + p), dtype=int)
    for k in range(Ln):
        for ch in range(m + p):
            nat[k * (m + p) + ch] = k * m + ch if ch < m else Ln * m + k * p + (ch - m)
    return nat


def with_setpoints(spec, u_s, y_s):
    return dataclasses.replace(spec, u_s=np.asarray(u_s, float).reshape(-1), y_s=np.asarray(y_s, float).reshape(-1))


def multi_hot(spec):
    """[m + p, r], internal order: row c is the right-hand side t of the reduced system at the zero past window and the unit
    setpoint e_c -- one in every component of channel c that takes its target from a setpoint, zero elsewhere."""
    n, m, p = spec.n, spec.m, spec.p
    nat = natural_of_internal(spec)
    E = np.eye(m + p)
    out = np.stack([rf.component_tables(with_setpoints(spec, E[c, :m], E[c, m:]), np.zeros(n * m), np.zeros(n * p))[1][nat]
                    for c in range(m + p)])
    assert set(np.unique(out)) <= {0.0, 1.0}
    return out


def past_hot(spec):
    """[n (m + p), r], internal order: row f is t at zero setpoints and the unit past window e_f (f over [u_past; y_past])."""
    n, m, p = spec.n, spec.m, spec.p
    nat = natural_of_internal(spec)
    zero = with_setpoints(spec, np.zeros(m), np.zeros(p))
    E = np.eye(n * (m + p))
    return np.stack([rf.component_tables(zero, E[f, :n * m], E[f, n * m:])[1][nat] for f in range(n * (m + p))])


def reduced_matrix(spec, u_d, y_d):
    """(K0, G, lam D), internal order: K0 = G + lam D of the empty active set."""
    n, m, p = spec.n, spec.m, spec.p
    nat = natural_of_internal(spec)
    H = np.vstack([orc.hankel_matrix(u_d, spec.Ln), orc.hankel_matrix(y_d, spec.Ln)])[nat]
    G = H @ H.T
    lam = spec.lamb_alpha * spec.eps_max
    D = rf.component_tables(spec, np.zeros(n * m), np.zeros(n * p))[0][nat]
    return G + lam * np.diag(D), G, lam * D


def law(spec, u_d, y_d):
    """(P [n (m + p), r], S [m + p, r]) by a direct solve with K0 (numpy's LU on the explicit Gram matrix: the unrefined route)."""
    K0, _, _ = reduced_matrix(spec, u_d, y_d)
    return np.linalg.solve(K0, past_hot(spec).T).T, np.linalg.solve(K0, multi_hot(spec).T).T


def law_step(spec, u_d, y_d, P, S, u_past, y_past, u_s, y_s):
    """Evaluate the law at a window and a setpoint -> (optimal_u [L m], cost), the output stage of the reduced form."""
    n, m, p, L, Ln = spec.n, spec.m, spec.p, spec.L, spec.Ln
    nat = natural_of_internal(spec)
    sp = with_setpoints(spec, u_s, y_s)
    past = np.concatenate([np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)])
    beta = past @ P + np.concatenate([sp.u_s, sp.y_s]) @ S
    _, G, lamD = reduced_matrix(spec, u_d, y_d)
    lam = spec.lamb_alpha * spec.eps_max
    t = rf.component_tables(sp, u_past, y_past)[1][nat]
    z = np.empty_like(t)
    z[nat] = t - lamD * beta                                   # natural stacking [ubar; w]
    bnat = np.empty_like(beta)
    bnat[nat] = beta
    ubar, w = z[:Ln * m], z[Ln * m:]
    sigma = np.zeros(Ln * p)
    sigma[:n * p] = w[:n * p] - np.asarray(y_past, float).reshape(-1)
    sigma[n * p:] = -lam * bnat[Ln * m + n * p:] / spec.lamb_sigma
    if spec.tec:
        sigma[L * p:] = w[L * p:] - np.tile(sp.y_s, n)
    ybar = w - sigma
    du = ubar[n * m:] - np.tile(sp.u_s, L)
    dy = ybar[n * p:] - np.tile(sp.y_s, L)
    cost = float(du @ (np.diag(spec.R) * du) + dy @ (np.diag(spec.Q) * dy) + lam * beta @ (G @ beta)
                 + spec.lamb_sigma * sigma @ sigma)
    return ubar[n * m:].copy(), cost


def inputs_from_beta(spec, beta, u_past, y_past, u_s, y_s):
    """optimal_u [L m] of a beta in internal order: z = t - lam D beta on the input rows of the prediction steps."""
    n, m = spec.n, spec.m
    nat = natural_of_internal(spec)
    D, t = rf.component_tables(with_setpoints(spec, u_s, y_s), u_past, y_past)
    z = t[nat] - spec.lamb_alpha * spec.eps_max * D[nat] * beta
    return z.reshape(spec.Ln, m + spec.p)[n:, :m].reshape(-1)


def schedule_loop(spec, u_d, y_d, plant, w_sys, u_ref, y_ref, n_mpc_step=1, u_past=None, y_past=None):
    """orc.closed_loop with a setpoint schedule: the solve made at step t is the full-space QP with the setpoints
    (u_ref[t], y_ref[t]); `plant` (orc.Plant) is stepped in place.  Returns (u_sys, y_sys, u_past_end, y_past_end)."""
    n, m, p = spec.n, spec.m, spec.p
    n_steps = w_sys.shape[0]
    up = (u_d[-n:].reshape(-1) if u_past is None else np.asarray(u_past, float).reshape(-1)).copy()
    yp = (y_d[-n:].reshape(-1) if y_past is None else np.asarray(y_past, float).reshape(-1)).copy()
    u_sys = np.zeros((n_steps, m))
    y_sys = np.zeros((n_steps, p))
    for t in range(0, n_steps, n_mpc_step):
        sol = orc.solve_fullspace(with_setpoints(spec, u_ref[t], y_ref[t]), u_d, y_d, up, yp)
        if sol.status not in (orc.OPTIMAL, orc.OPTIMAL_INACCURATE):
            raise ValueError("MPC problem was not solved optimally.")
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = sol.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w_sys[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys, up, yp
