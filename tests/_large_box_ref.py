"""Reduced-space reference for bounds beyond 271 rows with many active components (DDMPC_OPT_LARGE_BOX_CAPACITY).

A helper, not a test.  `solve_reduced` is the iteration of tests/test_large_bounds_reference.py::solve_trailing_block -- the kept
factor of the empty active set, every active component a column of W = L^-1 E, the k x k system diag(1 / d_s) - W'W, the table
of DESIGN 5.5 / 5.5.1 -- extended to return what the GPU tests at this size need without the full-space helper (0.2 s per solve
at 296 rows, 20 - 46 solves per instance in the tightest case):

  * `sizes`: the number of active components in every iteration that solved a system (its maximum is `peak`), so a test knows
    the iteration at which an instance outgrows a capacity (`first_over`);
  * `margin`, as defined in tests/_input_bounds_ref.py, in the reduced variables: over all iterations the smaller of the
    smallest distance of an inactive boxed value hat_s = a_s + c_s beta to its nearer finite bound, relative to the size of that
    component's box, and min |mu| / max |mu| over the active set, with mu_s = (hat_s - bound_s) / |c_s| -- the multiplier of the
    held component up to one factor common to all (hat_s is the value the component would take if it alone were released);
  * `idx`, `lo`, `hi`, `active`: the boxed components in the order of x = [alpha; ubar; ybar; sigma] with the signed final set,
    the fields tests/test_gpu_large_bounds.py reads from the full-space helper's solution.

The factor, the per-row table and the Hankel matrix of an instance are formed once and shared by its iterations.

The outputs come from one more solve of the system of the FINAL active set, (G + lam D(state)) beta = t(state), by a Cholesky
factorisation of that matrix itself and one step of iterative refinement with the residual in extended precision -- not from
the Woodbury update of the last iteration, which at 250 active components differs between two numpy statements of the same
iteration by 5e-9 in the inputs (measured against solve_trailing_block), half the bar the GPU tests hold the kernels to.  The
iteration, and so the solve count, the sets and the margin, is untouched by that.
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np
import scipy.linalg as sla

from oracle import ddmpc_oracle as orc

from test_large_bounds_reference import _kinds, box_order

INF = np.inf


@dataclass
class ReducedSolution:
    status: str
    iters: int
    cost: float
    optimal_u: np.ndarray
    idx: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    active: np.ndarray
    margin: float
    sizes: List[int] = field(default_factory=list)
    peak: int = 0
    both: int = 0
    signed: dict = field(default_factory=dict)

    def first_over(self, cap):
        """The value of `iters` at which the active set first has more than cap components, or None."""
        for q, k in enumerate(self.sizes):
            if k > cap:
                return q + 1
        return None


def solve_reduced(spec, u_d, y_d, u_past, y_past, box, max_iter=50):
    n, m, p, Lh, Ln = spec.n, spec.m, spec.p, spec.L, spec.Ln
    nch, r = m + p, (m + p) * Ln
    Hu, Hy = orc.hankel_matrix(u_d, Ln), orc.hankel_matrix(y_d, Ln)
    H = np.zeros((r, Hu.shape[1]))
    for k in range(Ln):
        H[k * nch:k * nch + m] = Hu[k * m:(k + 1) * m]
        H[k * nch + m:(k + 1) * nch] = Hy[k * p:(k + 1) * p]
    lam, ls, bound = spec.lamb_alpha * spec.eps_max, spec.lamb_sigma, spec.c * spec.eps_max
    convex = spec.slack == "convex"
    rd, qd = np.diag(spec.R), np.diag(spec.Q)
    u_s, y_s = np.asarray(spec.u_s, float).reshape(-1), np.asarray(spec.y_s, float).reshape(-1)
    kinds = _kinds(spec)
    up, yp = np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)
    D0, D1, t0, w = np.zeros(r), np.zeros(r), np.zeros(r), np.zeros(r)
    for rho, (kind, ch, kp) in enumerate(kinds):
        if kind == "ufix":
            t0[rho] = up[(kp + n) * m + ch] if kp < 0 else u_s[ch]
        elif kind == "ufree":
            w[rho] = rd[kp * m + ch]; D0[rho] = D1[rho] = 1.0 / w[rho]; t0[rho] = u_s[ch]
        elif kind == "wint":
            D0[rho] = D1[rho] = 1.0 / ls; t0[rho] = yp[(kp + n) * p + ch]
        elif kind == "wterm":
            D0[rho] = 1.0 / ls; t0[rho] = y_s[ch]
        else:
            w[rho] = qd[kp * p + ch]; D0[rho] = 1.0 / w[rho] + 1.0 / ls; D1[rho] = 1.0 / w[rho]; t0[rho] = y_s[ch]
    perm, nA, cpos, cy = box_order(spec, box)
    n0 = nA & ~63
    ulo, uhi = (np.broadcast_to(np.asarray(v, float), (m,)) for v in (box["u"] or (-INF, INF)))
    ylo, yhi = (np.broadcast_to(np.asarray(v, float), (p,)) for v in (box["y"] or (-INF, INF)))
    tab, seen = [], {}
    for s, (i, isy) in enumerate(zip(cpos, cy)):
        rho = int(perm[i])
        kind, ch, kp = kinds[rho]
        if isy:
            tab.append((y_s[ch], -lam * D1[rho], ylo[ch], yhi[ch], lam * D1[rho], "y"))
        elif kind == "ufree":
            tab.append((u_s[ch], -lam * D0[rho], ulo[ch], uhi[ch], lam * D0[rho], "u"))
        else:
            assert convex and kind in ("wpred", "wterm")
            tab.append((0.0, -lam / ls, -bound, bound, lam * (D0[rho] - D1[rho]), "s"))
        assert seen.setdefault((i, tab[-1][5]), s) == s
    a, c, lo, hi, dd = (np.array([t[q] for t in tab], float) for q in range(5))
    scale = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    K0 = (H @ H.T + lam * np.diag(D0))[np.ix_(perm, perm)]
    Lf = np.linalg.cholesky(K0)
    y = sla.solve_triangular(Lf, t0[perm], lower=True)
    beta = sla.solve_triangular(Lf, y, lower=True, trans="T")
    LTT = Lf[n0:, n0:]
    act = np.zeros(len(tab), dtype=int)
    iters, status, sizes, margin = 0, "optimal", [], np.inf
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
        if iters >= max_iter:
            status = "solver_error"
            break
        lst = np.nonzero(act)[0]
        sizes.append(int(lst.size))
        E = np.zeros((r - n0, lst.size))
        E[cpos[lst] - n0, np.arange(lst.size)] = 1.0                     # (the unit vectors vanish above the trailing block)
        W = np.zeros((r, lst.size))
        W[n0:] = sla.solve_triangular(LTT, E, lower=True)
        shift = np.where(act[lst] > 0, hi[lst], lo[lst]) - a[lst]
        WW = W.T @ W
        Ls = np.linalg.cholesky(np.diag(1.0 / dd[lst]) - WW)
        hv = W.T @ y + WW @ shift
        ev = sla.cho_solve((Ls, True), hv) + shift
        beta = sla.solve_triangular(Lf, y + W @ ev, lower=True, trans="T")
    # output stage: D(state), t(state) per row
    sa, say = np.zeros(r, int), np.zeros(r, int)
    for s, (i, isy) in enumerate(zip(cpos, cy)):
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
    return ReducedSolution(status=status, iters=iters, cost=float(cost), optimal_u=ubar[n * m:].copy(), idx=idx,
                           lo=np.array([bnds[int(i)][0] for i in idx], float), hi=np.array([bnds[int(i)][1] for i in idx], float),
                           active=np.array([signed[int(i)] for i in idx], int), margin=float(margin), sizes=sizes,
                           peak=max(sizes) if sizes else 0, both=both, signed=signed)


# ---- the fixture and the cases of the capacity tests: four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7 at the data tail
Y_TIGHT = ([0.645, 0.765], [0.655, 0.775])
CASES = {
    "A": dict(box=dict(u=([0.0, 0.0], [2.0, 2.0]), y=None), slack="convex"),
    "B": dict(box=dict(u=([0.9, 0.9], [1.1, 1.1]), y=None), slack="none"),
    "C": dict(box=dict(u=None, y=Y_TIGHT), slack="none"),
    "D": dict(box=dict(u=None, y=Y_TIGHT), slack="convex"),
    "E": dict(box=dict(u=([0.8, 0.8], [1.2, 1.2]), y=Y_TIGHT), slack="none"),
}
