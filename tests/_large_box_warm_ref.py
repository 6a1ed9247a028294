"""Reference of the seeded reduced-space iteration (DDMPC_OPT_LARGE_BOX_WARM_START, DESIGN 5.5.2 "Warm start").

A helper, not a test.  `Reduced` restates tests/_large_box_ref.py::solve_reduced -- the same statements in the same order, the
part that depends on the data alone (Hankel matrix, the kept factor, the box table) formed once per instance and shared by the
windows of a closed loop -- and starts its iteration from a signed set.  The count convention is the kernels': `iters` counts
the tests, each of which follows a solve, 1 = the empty set's.

1. the empty set is solved and tested.  No violation: optimal, `iters` = 1, the set left is empty;
2. a violation and no seed (None, all zero): the iteration of `solve_reduced`, statement for statement;
3. a violation and a non-empty seed: `act` := the seed instead of what the test asked for, then the unchanged loop -- solve
   (number 2), test, ... with the releasing rule and the `max_iter` cap;
4. a seeded run that meets a singular k x k system, more than `capacity` active components or the cap is given up: the empty
   set and its beta again, a fresh cap.  `iters` = every solve attempted, the empty set's once: a run given up at the cap has
   made max_iter solves, of which the restarted run repeats none but the empty set's (max_iter - 1 + its own count); one given
   up on the k x k system or the capacity at test number q had q + 1 attempted (q + the restarted run's count).
   `safeguard=True` states the exception: the seeded run at the cap is not started again (status "solver_error", `iters` =
   max_iter, `at_cap`), it is what rr3_box_safeguard_kernel then solves from the empty set's solution.

`margin` is `solve_reduced`'s, over every test made, those of a run that was given up included.  `set` is the final signed
set over the box table's components in table order: what the next window is seeded with.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import scipy.linalg as sla

from oracle import ddmpc_oracle as orc

import _large_box_ref as lref
from test_large_bounds_reference import _kinds, box_order

INF = np.inf


@dataclass
class SeededReduced:
    status: str
    iters: int
    cost: float
    optimal_u: np.ndarray
    idx: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    active: np.ndarray              # the final set in the order of x = [alpha; ubar; ybar; sigma] (as ReducedSolution.active)
    margin: float
    set: np.ndarray                 # the final set in table order (all zero unless optimal): the next window's seed
    sizes: List[int] = field(default_factory=list)
    peak: int = 0
    both: int = 0
    signed: dict = field(default_factory=dict)
    seeded: bool = False            # a non-empty seed was installed
    fell_back: bool = False         # ... and given up: the result is the empty start's
    at_cap: bool = False            # the last run ended at its own cap
    window: tuple = ()


class Reduced:
    """The reduced problem of one instance and one box; `solve` per past window."""

    def __init__(self, spec, u_d, y_d, box):
        n, m, p, Ln = spec.n, spec.m, spec.p, spec.Ln
        nch, r = m + p, (m + p) * Ln
        Hu, Hy = orc.hankel_matrix(u_d, Ln), orc.hankel_matrix(y_d, Ln)
        H = np.zeros((r, Hu.shape[1]))
        for k in range(Ln):
            H[k * nch:k * nch + m] = Hu[k * m:(k + 1) * m]
            H[k * nch + m:(k + 1) * nch] = Hy[k * p:(k + 1) * p]
        self.spec, self.box, self.H, self.r = spec, box, H, r
        self.lam, self.ls, self.bound = spec.lamb_alpha * spec.eps_max, spec.lamb_sigma, spec.c * spec.eps_max
        lam, ls, bound = self.lam, self.ls, self.bound
        convex = spec.slack == "convex"
        rd, qd = np.diag(spec.R), np.diag(spec.Q)
        self.u_s, self.y_s = np.asarray(spec.u_s, float).reshape(-1), np.asarray(spec.y_s, float).reshape(-1)
        u_s, y_s = self.u_s, self.y_s
        self.kinds = kinds = _kinds(spec)
        D0, D1, w = np.zeros(r), np.zeros(r), np.zeros(r)
        for rho, (kind, ch, kp) in enumerate(kinds):
            if kind == "ufree":
                w[rho] = rd[kp * m + ch]; D0[rho] = D1[rho] = 1.0 / w[rho]
            elif kind == "wint":
                D0[rho] = D1[rho] = 1.0 / ls
            elif kind == "wterm":
                D0[rho] = 1.0 / ls
            elif kind != "ufix":
                w[rho] = qd[kp * p + ch]; D0[rho] = 1.0 / w[rho] + 1.0 / ls; D1[rho] = 1.0 / w[rho]
        self.D0, self.D1, self.w = D0, D1, w
        self.perm, self.nA, self.cpos, self.cy = perm, nA, cpos, cy = box_order(spec, box)
        self.n0 = n0 = nA & ~63
        self.ulo, self.uhi = (np.broadcast_to(np.asarray(v, float), (m,)) for v in (box["u"] or (-INF, INF)))
        self.ylo, self.yhi = (np.broadcast_to(np.asarray(v, float), (p,)) for v in (box["y"] or (-INF, INF)))
        tab, self.seen = [], {}
        for s, (i, isy) in enumerate(zip(cpos, cy)):
            rho = int(perm[i])
            kind, ch, kp = kinds[rho]
            if isy:
                tab.append((y_s[ch], -lam * D1[rho], self.ylo[ch], self.yhi[ch], lam * D1[rho], "y"))
            elif kind == "ufree":
                tab.append((u_s[ch], -lam * D0[rho], self.ulo[ch], self.uhi[ch], lam * D0[rho], "u"))
            else:
                assert convex and kind in ("wpred", "wterm")
                tab.append((0.0, -lam / ls, -bound, bound, lam * (D0[rho] - D1[rho]), "s"))
            assert self.seen.setdefault((i, tab[-1][5]), s) == s
        self.a, self.c, self.lo, self.hi, self.dd = (np.array([t[q] for t in tab], float) for q in range(5))
        self.nbox = len(tab)
        self.scale = np.maximum(np.where(np.isfinite(self.lo), np.abs(self.lo), 0.0), np.where(np.isfinite(self.hi), np.abs(self.hi), 0.0))
        K0 = (H @ H.T + lam * np.diag(D0))[np.ix_(perm, perm)]
        self.Lf = np.linalg.cholesky(K0)
        self.LTT = self.Lf[n0:, n0:]

    def _t0(self, up, yp):
        spec, n, m, p = self.spec, self.spec.n, self.spec.m, self.spec.p
        t0 = np.zeros(self.r)
        for rho, (kind, ch, kp) in enumerate(self.kinds):
            if kind == "ufix":
                t0[rho] = up[(kp + n) * m + ch] if kp < 0 else self.u_s[ch]
            elif kind == "ufree":
                t0[rho] = self.u_s[ch]
            elif kind == "wint":
                t0[rho] = yp[(kp + n) * p + ch]
            else:
                t0[rho] = self.y_s[ch]
        return t0

    def solve(self, u_past, y_past, seed: Optional[np.ndarray] = None, max_iter: int = 50, safeguard: bool = False,
              capacity: Optional[int] = None) -> SeededReduced:
        a, c, lo, hi, dd, scale, cpos, r, n0 = self.a, self.c, self.lo, self.hi, self.dd, self.scale, self.cpos, self.r, self.n0
        Lf, LTT, perm = self.Lf, self.LTT, self.perm
        up, yp = np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)
        t0 = self._t0(up, yp)
        y = sla.solve_triangular(Lf, t0[perm], lower=True)
        beta0 = sla.solve_triangular(Lf, y, lower=True, trans="T")
        if seed is not None:
            seed = np.asarray(seed, dtype=int)
            if seed.shape != (self.nbox,):
                raise ValueError("the seed belongs to another box table")
            if not np.any(seed):
                seed = None
        beta, act = beta0, np.zeros(self.nbox, dtype=int)
        iters, status, sizes, margin = 0, "optimal", [], np.inf
        run0, phase, at_cap = 0, 0, False                        # phase: 0 no seed yet, 1 the seeded run, 2 started again / no seed
        while True:
            iters += 1
            hat = a + c * beta[cpos]
            new = np.where(act > 0, (hat > hi).astype(int), np.where(act < 0, -(hat < lo).astype(int), (hat > hi).astype(int) - (hat < lo)))
            free = act == 0
            if np.any(free):
                d = np.minimum(np.where(np.isfinite(hi), np.abs(hat - hi), np.inf), np.where(np.isfinite(lo), np.abs(hat - lo), np.inf))
                margin = min(margin, float(np.min(d[free] / scale[free])))
            if np.any(~free):
                mu = np.abs((hat - np.where(act > 0, hi, lo))[~free] / c[~free])
                margin = min(margin, float(np.min(mu) / max(np.max(mu), 1e-300)))
            if np.array_equal(new, act):
                break
            act = new
            if iters - run0 >= max_iter:
                if phase != 1 or safeguard:
                    status, at_cap = "solver_error", True
                    break
                iters -= 1                                        # (the test that found the cap followed a solve already counted)
                act, beta, run0, phase = np.zeros(self.nbox, dtype=int), beta0, iters, 2
                continue
            if phase == 0:
                phase = 2
                if seed is not None:
                    act, phase = seed.copy(), 1
            lst = np.nonzero(act)[0]
            sizes.append(int(lst.size))
            ok = capacity is None or lst.size <= capacity
            if ok:
                E = np.zeros((r - n0, lst.size))
                E[cpos[lst] - n0, np.arange(lst.size)] = 1.0
                W = np.zeros((r, lst.size))
                W[n0:] = sla.solve_triangular(LTT, E, lower=True)
                shift = np.where(act[lst] > 0, hi[lst], lo[lst]) - a[lst]
                WW = W.T @ W
                try:
                    Ls = np.linalg.cholesky(np.diag(1.0 / dd[lst]) - WW)
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                if phase != 1:
                    status = "solver_error"
                    break
                act, beta, run0, phase = np.zeros(self.nbox, dtype=int), beta0, iters, 2
                continue
            hv = W.T @ y + WW @ shift
            ev = sla.cho_solve((Ls, True), hv) + shift
            beta = sla.solve_triangular(Lf, y + W @ ev, lower=True, trans="T")
        seeded = seed is not None and len(sizes) > 0
        fell_back = seeded and run0 > 0
        out = self._outputs(t0, beta, act, status)
        return SeededReduced(status=status, iters=iters, margin=float(margin), sizes=sizes, peak=max(sizes) if sizes else 0,
                             set=act.copy() if status == "optimal" else np.zeros(self.nbox, dtype=int), seeded=seeded,
                             fell_back=fell_back, at_cap=at_cap, window=(up.copy(), yp.copy()), **out)

    def _outputs(self, t0, beta, act, status):
        """The output stage of `solve_reduced`: one more solve of the system of the final set, then z, the cost and the sets."""
        spec, r, perm, kinds, H = self.spec, self.r, self.perm, self.kinds, self.H
        n, m, p, Ln = spec.n, spec.m, spec.p, spec.Ln
        lam, ls, bound, D0, D1, w = self.lam, self.ls, self.bound, self.D0, self.D1, self.w
        u_s, y_s, ulo, uhi, ylo, yhi, seen = self.u_s, self.y_s, self.ulo, self.uhi, self.ylo, self.yhi, self.seen
        sa, say = np.zeros(r, int), np.zeros(r, int)
        for s, (i, isy) in enumerate(zip(self.cpos, self.cy)):
            (say if isy else sa)[i] = act[s]
        if status == "optimal" and np.any(act):
            Dv, tv = np.zeros(r), np.zeros(r)
            for i in range(r):
                rho = int(perm[i])
                kind, ch, kp = kinds[rho]
                Dv[i] = D1[rho] if sa[i] else D0[rho]
                tv[i] = t0[rho] + sa[i] * bound
                if kind == "ufree" and sa[i]:
                    Dv[i], tv[i] = 0.0, (uhi[ch] if sa[i] > 0 else ulo[ch])
                if say[i]:
                    Dv[i], tv[i] = (0.0 if sa[i] else 1.0 / ls), (yhi[ch] if say[i] > 0 else ylo[ch]) + sa[i] * bound
            Hp = H[perm]
            Kf = sla.cho_factor(Hp @ Hp.T + lam * np.diag(Dv), lower=True)
            beta = sla.cho_solve(Kf, tv)
            Hl, bl = Hp.astype(np.longdouble), beta.astype(np.longdouble)
            res = tv.astype(np.longdouble) - (Hl @ (Hl.T @ bl) + lam * Dv.astype(np.longdouble) * bl)
            beta = beta + sla.cho_solve(Kf, res.astype(float))
        nu, ny = Ln * m, Ln * p
        ubar = np.zeros(nu)
        cost, both, signed, bnds = 0.0, 0, {}, {}
        na = H.shape[1]
        for i in range(r):
            rho = int(perm[i])
            kind, ch, kp = kinds[rho]
            k = kp + n
            b_ = beta[i]
            D = D1[rho] if sa[i] else D0[rho]
            t = t0[rho] + sa[i] * bound
            if kind == "ufree" and sa[i]:
                D, t = 0.0, (uhi[ch] if sa[i] > 0 else ulo[ch])
            if say[i]:
                D, t = (0.0 if sa[i] else 1.0 / ls), (yhi[ch] if say[i] > 0 else ylo[ch]) + sa[i] * bound
            z = t - lam * D * b_
            cost += lam * b_ * z
            if kind in ("ufix", "ufree"):
                ubar[k * m + ch] = z
                if kind == "ufree":
                    cost += w[rho] * (z - u_s[ch]) ** 2
                    if (i, "u") in seen:
                        signed[na + k * m + ch] = int(sa[i]); bnds[na + k * m + ch] = (ulo[ch], uhi[ch])
                continue
            j = k * p + ch
            if kind == "wint":
                sg = z - t0[rho]
            elif kind == "wterm":
                sg = z - y_s[ch]
            else:
                sg = sa[i] * bound if sa[i] else -lam * b_ / ls
            yb = (t - sa[i] * bound) if say[i] else z - sg
            cost += ls * sg * sg + (w[rho] * (yb - y_s[ch]) ** 2 if kind == "wpred" else 0.0)
            both += bool(sa[i] and say[i])
            if (i, "s") in seen:
                signed[na + nu + ny + j] = int(sa[i]); bnds[na + nu + ny + j] = (-bound, bound)
            if (i, "y") in seen:
                signed[na + nu + j] = int(say[i]); bnds[na + nu + j] = (ylo[ch], yhi[ch])
        idx = np.array(sorted(signed), int)
        return dict(cost=float(cost), optimal_u=ubar[n * m:].copy(), idx=idx,
                    lo=np.array([bnds[int(i)][0] for i in idx], float), hi=np.array([bnds[int(i)][1] for i in idx], float),
                    active=np.array([signed[int(i)] for i in idx], int), both=both, signed=signed)

    def table_set(self, sol) -> np.ndarray:
        """The signed set of a solution given in x order (ReducedSolution / SafeguardedSolution: idx, active) in table order."""
        spec = self.spec
        n, m, p, Ln = spec.n, spec.m, spec.p, spec.Ln
        na, nu, ny = self.H.shape[1], Ln * m, Ln * p
        by_x = dict(zip((int(i) for i in sol.idx), (int(v) for v in sol.active)))
        out = np.zeros(self.nbox, dtype=int)
        for s, (i, isy) in enumerate(zip(self.cpos, self.cy)):
            kind, ch, kp = self.kinds[int(self.perm[i])]
            k = kp + n
            if isy:
                out[s] = by_x[na + nu + k * p + ch]
            elif kind == "ufree":
                out[s] = by_x[na + k * m + ch]
            else:
                out[s] = by_x[na + nu + ny + k * p + ch]
        return out


def solve_seeded(spec, u_d, y_d, u_past, y_past, box, seed=None, max_iter=50, **kw) -> SeededReduced:
    return Reduced(spec, u_d, y_d, box).solve(u_past, y_past, seed, max_iter=max_iter, **kw)


def closed_loop_seeded(spec, u_d, y_d, plant, w_sys, box, n_mpc_step: int = 1, u_past=None, y_past=None, max_iter: int = 50,
                       carry: bool = True, problem: Optional[Reduced] = None, first: Optional[SeededReduced] = None, **kw):
    """The closed loop of `_box_warm_ref.closed_loop_seeded` on the reduced problem: the set of every solve carried, as it is, into
    the next (carry = False: every solve from the empty set).  `first`: the solution of the first window, where another method
    found it (its `set` is carried).  Returns (u_sys, y_sys, the solution of every solve, each with its `window`); stops behind
    a solve that is not optimal."""
    n, m, p = spec.n, spec.m, spec.p
    prob = problem if problem is not None else Reduced(spec, u_d, y_d, box)
    n_steps = w_sys.shape[0]
    up = (u_d[-n:].reshape(-1) if u_past is None else np.asarray(u_past, float).reshape(-1)).copy()
    yp = (y_d[-n:].reshape(-1) if y_past is None else np.asarray(y_past, float).reshape(-1)).copy()
    u_sys, y_sys = np.full((n_steps, m), np.nan), np.full((n_steps, p), np.nan)
    sols: List[SeededReduced] = []
    seed = None
    for t in range(0, n_steps, n_mpc_step):
        if t == 0 and first is not None:
            s = first
            s.window = (up.copy(), yp.copy())
        else:
            s = prob.solve(up, yp, seed if carry else None, max_iter=max_iter, **kw)
        sols.append(s)
        if s.status != "optimal":
            break
        seed = s.set.copy() if hasattr(s, "set") else prob.table_set(s)
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = s.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w_sys[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys, sols


__all__ = ["Reduced", "SeededReduced", "solve_seeded", "closed_loop_seeded", "lref"]
