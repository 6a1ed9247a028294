"""Reduced-space reference of the safeguard beyond 271 rows (DDMPC_OPT_LARGE_BOX_SAFEGUARD): the primal
active-set method of DESIGN 5.5 (tests/_box_safeguard_ref.py states it on the full-space QP) on the reduced system of
tests/_large_box_ref.py.

A helper, not a test.  The kept factor of the empty active set, every boxed component s a column of W = L_TT^-1 E, the system
S = diag(1 / d_s) - W'W of the working set, the table a, c, lo, hi, d, shift of DESIGN 5.5 / 5.5.1.  With hat_s = a_s + c_s beta
at the component's position:

  1. v = clip(hat(empty set), lo, hi); the working set = the components hat violates, each on the side it violates.
  2. Solve for the working set; v+ = hat outside it.  An inactive component with v+ outside its box blocks at
     alpha = (bound - v) / (v+ - v).
  3. If one blocks: v += alpha (v+ - v) with the smallest alpha (lowest component on ties); that component joins at its bound.
  4. Otherwise v = v+; the active component with the largest g_s = act_s (bound_s - hat_s) / |c_s| (lowest component on ties) is
     released if g_s > 0; if none is, the working set is optimal.

The cap is 4 nbox + 16 solves.  `iters` counts the solves of 2, `sizes` the working set of each, `margin` says how far the run was
from deciding differently -- the smallest, over all solves, of
  * blocks or does not block: when none blocks, the distance of every inactive v+ to its nearer finite bound, relative to the
    size of that component's box; when exactly one does, its distance beyond the bound;
  * which one blocks first: (alpha_2 - alpha_1) / alpha_2 of the two smallest step lengths;
  * released or optimal: |g_1| / max |g| of the largest multiplier g_1 (its sign decides), and (g_1 - g_2) / g_1 against the
    second largest when g_1 is released.
A component that is barely outside its box while another blocks earlier, or a small multiplier that is not the largest, changes
no decision and does not enter.
The values hat at the boxed positions need no substitution per solve: beta[pos] = beta0[pos] + (W'W)[:, set] ev, the same
quantity the kernels form as L_TT^-T (y + W ev).  The outputs come from a direct solve of the system of the final set, as in
`_large_box_ref.solve_reduced`.
"""
from dataclasses import dataclass, field
from typing import List

import numpy as np
import scipy.linalg as sla

from oracle import ddmpc_oracle as orc

from test_large_bounds_reference import _kinds, box_order

INF = np.inf


@dataclass
class SafeguardSolution:
    status: str
    iters: int                      # solves of the primal method
    cost: float
    optimal_u: np.ndarray
    idx: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    active: np.ndarray
    margin: float
    sizes: List[int] = field(default_factory=list)
    peak: int = 0
    signed: dict = field(default_factory=dict)
    releases: int = 0

    def first_over(self, cap):
        """The number (from 1) of the first solve whose working set has more than cap components, or None."""
        for q, k in enumerate(self.sizes):
            if k > cap:
                return q + 1
        return None


def solve_primal(spec, u_d, y_d, u_past, y_past, box, cap=None):
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
    nbox = len(tab)
    scale = np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0))
    K0 = (H @ H.T + lam * np.diag(D0))[np.ix_(perm, perm)]
    Lf = np.linalg.cholesky(K0)
    y = sla.solve_triangular(Lf, t0[perm], lower=True)
    beta0 = sla.solve_triangular(Lf, y, lower=True, trans="T")
    E = np.zeros((r - n0, nbox))
    E[cpos - n0, np.arange(nbox)] = 1.0                                     # (the unit vectors vanish above the trailing block)
    Wall = sla.solve_triangular(Lf[n0:, n0:], E, lower=True)
    Gall = Wall.T @ Wall
    hy = Wall.T @ y[n0:]
    hat = a + c * beta0[cpos]
    act = (hat > hi).astype(int) - (hat < lo).astype(int)
    v = np.clip(hat, lo, hi)
    cap = 4 * nbox + 16 if cap is None else cap
    status, iters, sizes, margin, releases = "solver_error", 0, [], np.inf, 0
    while iters < cap:
        iters += 1
        lst = np.nonzero(act)[0]
        sizes.append(int(lst.size))
        free = act == 0
        bnd = np.where(act > 0, hi, lo)
        shift = (bnd - a)[lst]
        G = Gall[np.ix_(lst, lst)]
        try:
            Ls = np.linalg.cholesky(np.diag(1.0 / dd[lst]) - G)
        except np.linalg.LinAlgError:
            break
        ev = sla.cho_solve((Ls, True), hy[lst] + G @ shift) + shift
        hat = a + c * (beta0[cpos] + Gall[:, lst] @ ev)
        upv, dnv = free & (hat > hi), free & (hat < lo)
        d = np.minimum(np.where(np.isfinite(hi), np.abs(hat - hi), np.inf), np.where(np.isfinite(lo), np.abs(hat - lo), np.inf))
        block = np.nonzero(upv | dnv)[0]
        if block.size == 1:
            margin = min(margin, float(d[block[0]] / scale[block[0]]))
        elif block.size == 0 and np.any(free):
            margin = min(margin, float(np.min(d[free] / scale[free])))
        if block.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.fmax((np.where(upv, hi, lo)[block] - v[block]) / (hat[block] - v[block]), 0.0)
            q = int(np.argmin(ratio))                                        # (argmin: the first of equal values)
            if block.size > 1:
                two = np.sort(ratio)[:2]
                margin = min(margin, float((two[1] - two[0]) / max(two[1], 1e-300)))
            s = block[q]
            v[free] += float(ratio[q]) * (hat[free] - v[free])
            act[s] = 1 if upv[s] else -1
            v[s] = hi[s] if upv[s] else lo[s]
            continue
        v[free] = hat[free]
        g = np.where(free, -np.inf, act * (bnd - hat) / np.abs(c))          # > 0: the multiplier has the wrong sign
        s = int(np.argmax(g)) if lst.size else 0
        if lst.size:
            margin = min(margin, float(abs(g[s]) / max(np.max(np.abs(g[lst])), 1e-300)))
        if lst.size == 0 or not g[s] > 0.0:
            status = "optimal"
            break
        if lst.size > 1:
            two = np.sort(g[lst])[-2:]
            margin = min(margin, float((two[1] - two[0]) / two[1]))
        act[s] = 0
        releases += 1
    # output stage: D(state), t(state) per row, one direct solve of the final system with a refinement step
    sa, say = np.zeros(r, int), np.zeros(r, int)
    for s, (i, isy) in enumerate(zip(cpos, cy)):
        (say if isy else sa)[i] = act[s]

    def row(i):
        rho = int(perm[i])
        kind, ch, kp = kinds[rho]
        D, t = (D1[rho] if sa[i] else D0[rho]), t0[rho] + sa[i] * bound
        if kind == "ufree" and sa[i]:
            D, t = 0.0, (uhi[ch] if sa[i] > 0 else ulo[ch])
        if say[i]:
            D, t = (0.0 if sa[i] else 1.0 / ls), (yhi[ch] if say[i] > 0 else ylo[ch]) + sa[i] * bound
        return rho, kind, ch, kp, D, t

    rows = [row(i) for i in range(r)]
    Dv, tv = np.array([q[4] for q in rows]), np.array([q[5] for q in rows])
    beta = beta0
    if status == "optimal" and np.any(act):
        Hp = H[perm]
        Kf = sla.cho_factor(Hp @ Hp.T + lam * np.diag(Dv), lower=True)
        beta = sla.cho_solve(Kf, tv)
        Hl, bl = Hp.astype(np.longdouble), beta.astype(np.longdouble)
        res = tv.astype(np.longdouble) - (Hl @ (Hl.T @ bl) + lam * Dv.astype(np.longdouble) * bl)
        beta = beta + sla.cho_solve(Kf, res.astype(float))
    nu, ny, na = Ln * m, Ln * p, H.shape[1]
    ubar = np.zeros(nu)
    cost, signed, bnds = 0.0, {}, {}
    for i, (rho, kind, ch, kp, D, t) in enumerate(rows):
        k, b_ = kp + n, beta[i]
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
        if (i, "s") in seen:
            signed[na + nu + ny + j] = int(sa[i]); bnds[na + nu + ny + j] = (-bound, bound)
        if (i, "y") in seen:
            signed[na + nu + j] = int(say[i]); bnds[na + nu + j] = (ylo[ch], yhi[ch])
    idx = np.array(sorted(signed), int)
    return SafeguardSolution(status=status, iters=iters, cost=float(cost) if status == "optimal" else float("nan"),
                             optimal_u=ubar[n * m:].copy(), idx=idx, lo=np.array([bnds[int(i)][0] for i in idx], float),
                             hi=np.array([bnds[int(i)][1] for i in idx], float),
                             active=np.array([signed[int(i)] for i in idx], int), margin=float(margin), sizes=sizes,
                             peak=max(sizes) if sizes else 0, signed=signed, releases=releases)
