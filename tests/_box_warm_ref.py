"""Reference of the seeded active-set iteration (DDMPC_OPT_BOX_WARM_START) on the full-space problem of `_input_bounds_ref.py`.

A helper, not a test.  The rule of DESIGN 5.5, with the kernels' count convention (1 = the law, i.e. the solve of the empty
set, + 1 per solve of a non-empty set):

1. the empty set is solved and tested.  No violation: it is optimal, `iters` = 1, the set left is empty;
2. a violation and an empty seed: `_input_bounds_ref.solve_bounded` as it is;
3. a violation and a non-empty seed: the seed is solved for (solve number 2) and the rule of `solve_bounded` -- keep a bound
   while its multiplier has the right sign, add one where the free value violates it, stop when the set repeats -- goes on from
   there, at most `max_iter` solves in all;
4. a seeded run that ends at the cap, or whose KKT system is singular, is given up and `solve_bounded` starts from the empty
   set with a fresh cap; `iters` = every solve made, the law counted once.

`margin` is `solve_bounded`'s, taken over every solve made here, those of a run that was given up included.  The safeguard
(DDMPC_OPT_BOX_SAFEGUARD) is not stated here: behind a seeded run at the cap it starts from the empty set's law, so
`_box_safeguard_ref.py` describes it whatever the seed was.
"""
from dataclasses import dataclass, replace
from typing import List, Optional

import numpy as np

from oracle import ddmpc_oracle as orc

import _input_bounds_ref as ref


@dataclass
class SeededSolution:
    sol: ref.BoundedSolution        # x, cost, optimal_u, active, idx, lo, hi, status; iters and margin as described above
    seeded: bool                    # a non-empty seed was installed
    fell_back: bool                 # ... and given up (cap or singular system): the result is the empty start's

    def __getattr__(self, name):
        if name == "sol":
            raise AttributeError(name)
        return getattr(self.sol, name)


def _step(qp, idx, lo, hi, scale, act):
    """One solve for the signed set `act`: (x, the set the rule asks for next, the margin of this solve)."""
    nx, ne = qp.P.shape[0], qp.A.shape[0]
    a = np.nonzero(act)[0]
    Eb = np.zeros((a.size, nx))
    Eb[np.arange(a.size), idx[a]] = 1.0
    val = np.where(act > 0, hi, lo)
    x, nu = orc._kkt_solve(qp.P, qp.q, np.vstack([qp.A, Eb]), np.concatenate([qp.b, val[a]]))
    mu = np.zeros(idx.size)
    mu[a] = nu[ne:]
    v = x[idx]
    new = np.zeros(idx.size, dtype=int)
    new[(act == 1) & (mu > 0)] = 1
    new[(act == -1) & (mu < 0)] = -1
    new[(act == 0) & (v > hi)] = 1
    new[(act == 0) & (v < lo)] = -1
    margin = np.inf
    free = act == 0
    if np.any(free):
        d = np.minimum(np.where(np.isfinite(hi), np.abs(v - hi), np.inf), np.where(np.isfinite(lo), np.abs(v - lo), np.inf))
        margin = min(margin, float(np.min(d[free] / scale[free])))
    if a.size:
        margin = min(margin, float(np.min(np.abs(mu[a])) / max(np.max(np.abs(mu[a])), 1e-300)))
    return x, new, margin


def _solution(spec, qp, idx, lo, hi, x, act, iters, margin):
    sl = qp.sl
    ubar = x[sl["ubar"]]
    return ref.BoundedSolution(status=orc.OPTIMAL, x=x, cost=float(x @ qp.P @ x + qp.q @ x + qp.const),
                               optimal_u=ubar[spec.n * spec.m:].copy(), ubar=ubar, ybar=x[sl["ybar"]], sigma=x[sl["sigma"]],
                               alpha=x[sl["alpha"]], iters=iters, idx=idx, lo=lo, hi=hi, active=act, margin=float(margin))


def solve_seeded(spec, u_d, y_d, u_past, y_past, u_min, u_max, seed: Optional[np.ndarray] = None,
                 max_iter: int = 100) -> SeededSolution:
    """The bounded solve started from the signed set `seed` (over `box_of`'s components; None or all zero: the empty start)."""
    if seed is None or not np.any(seed):
        return SeededSolution(ref.solve_bounded(spec, u_d, y_d, u_past, y_past, u_min, u_max, max_iter=max_iter), False, False)
    qp = orc.build_fullspace_qp(spec, u_d, y_d, u_past, y_past)
    idx, lo, hi = ref.box_of(spec, qp, u_min, u_max)
    seed = np.asarray(seed, dtype=int)
    if seed.shape != idx.shape:
        raise ValueError("the seed belongs to another box list")
    scale = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    empty = np.zeros(idx.size, dtype=int)
    x, new, margin = _step(qp, idx, lo, hi, scale, empty)              # 1. the law
    if not np.any(new):
        return SeededSolution(_solution(spec, qp, idx, lo, hi, x, empty, 1, margin), False, False)
    act, iters, done = seed.copy(), 1, False                            # 3. the seeded run
    while iters < max_iter:
        iters += 1
        try:
            x, new, mg = _step(qp, idx, lo, hi, scale, act)
        except np.linalg.LinAlgError:
            break
        margin = min(margin, mg)
        if not np.all(np.isfinite(x)):
            break
        if np.array_equal(new, act):
            done = True
            break
        act = new
    if done:
        return SeededSolution(_solution(spec, qp, idx, lo, hi, x, act, iters, margin), True, False)
    cold = ref.solve_bounded(spec, u_d, y_d, u_past, y_past, u_min, u_max, max_iter=max_iter)      # 4. given up
    cold = replace(cold, iters=iters - 1 + cold.iters, margin=min(margin, cold.margin))
    return SeededSolution(cold, True, True)


def closed_loop_seeded(spec, u_d, y_d, plant, w_sys, u_min, u_max, n_mpc_step: int = 1, u_past=None, y_past=None,
                       max_iter: int = 100, carry: bool = True):
    """`_input_bounds_ref.closed_loop_bounded` with the set of every solve carried, as it is, into the next (carry = False: every
    solve from the empty set).  Returns (u_sys, y_sys, the solution of every solve); stops behind a solve that is not optimal."""
    n, m, p = spec.n, spec.m, spec.p
    n_steps = w_sys.shape[0]
    up = (u_d[-n:].reshape(-1) if u_past is None else np.asarray(u_past, float).reshape(-1)).copy()
    yp = (y_d[-n:].reshape(-1) if y_past is None else np.asarray(y_past, float).reshape(-1)).copy()
    u_sys, y_sys = np.full((n_steps, m), np.nan), np.full((n_steps, p), np.nan)
    sols: List[SeededSolution] = []
    seed = None
    for t in range(0, n_steps, n_mpc_step):
        s = solve_seeded(spec, u_d, y_d, up, yp, u_min, u_max, seed if carry else None, max_iter=max_iter)
        s.window = (up.copy(), yp.copy())
        sols.append(s)
        if s.status != orc.OPTIMAL:
            break
        seed = s.active.copy()
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = s.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w_sys[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys, sols
