"""Input and output bounds beyond 271 rows (ddmpc_rr3_box.hpp), on the CPU.

1. The trailing-block formulation the bounded phase kernels run, restated in numpy: the reduced system in the union "boxed last"
   order (the order comes from the library's own host builder), the factor of the EMPTY active set kept, every active component
   a column of W = L^-1 E (two components of one row give two equal columns), the k x k system diag(1 / d_s) - W'W with each
   component's own d_s, the right-hand side with the component's own shift, and the table of DESIGN 5.5 / 5.5.1 -- a K_WPRED row
   under slack NONE has D0 = 1/q + 1/lamb_sigma and keeps 1/lamb_sigma when its output is held.  Against the full-space helper
   (tests/_output_bounds_ref.py) on the boxes 2, 4 and 5 of tests/test_gpu_large_bounds.py, two instances each: equal solve
   counts and signed sets, inputs to 1e-8 and cost to 1e-9 relative.
2. The host builder of the order (ddmpc_debug_large_box_order, no device): a permutation, the boxed class exactly the union of
   slack rows, bounded free input rows and bounded free output rows, nA and the component list right, for the boxes 2, 3, 4.
"""
import ctypes as C

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd import harness
from oracle import ddmpc_oracle as orc

import _output_bounds_ref as yref

INF = np.inf
L_LONG, N_LONG = 70, 700                                # four-tank, (2 + 2)(70 + 4) = 296 rows
BOX2 = dict(u=([-4.0, -4.0], [6.0, 6.0]), y=None)
BOX3 = dict(u=([-1.0, -INF], [3.0, INF]), y=None)
BOX4 = dict(u=None, y=([-INF, -INF], [0.66, 0.775]))
BOX5 = dict(u=BOX2["u"], y=BOX4["y"])

_DATA = {}


def _four_tank(slack):
    if slack not in _DATA:
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, L=L_LONG)
        d = harness.generate_batch(range(2), N=N_LONG)
        n = spec.n
        _DATA[slack] = (spec, d, d["u_d"][:, -n:, :].reshape(2, -1).copy(), d["y_d"][:, -n:, :].reshape(2, -1).copy())
    return _DATA[slack]


def box_order(spec, box):
    """(perm, nA, component positions, output flags) from the library's host builder."""
    lib = L.load()
    m, p, r = spec.m, spec.p, (spec.m + spec.p) * (spec.L + spec.n)
    arr = lambda v, k: None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, float), (k,)))
    ul, uh = (arr(box["u"][0], m), arr(box["u"][1], m)) if box["u"] is not None else (None, None)
    yl, yh = (arr(box["y"][0], p), arr(box["y"][1], p)) if box["y"] is not None else (None, None)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p()
    perm = np.zeros(r, np.int32)
    comp = np.zeros(2 * 2 * r, np.int32)
    n_a, nbox = C.c_int32(), C.c_int32()
    L.check(lib.ddmpc_debug_large_box_order(m, p, spec.n, spec.L, int(spec.tec), int(spec.slack == "convex"), ptr(ul), ptr(uh),
                                            ptr(yl), ptr(yh), ptr(perm), C.addressof(n_a), ptr(comp), 2 * r, C.addressof(nbox)))
    return perm, n_a.value, comp[:nbox.value].copy(), comp[2 * r:2 * r + nbox.value].copy()


def _kinds(spec):
    """Per row rho = k (m + p) + ch of the kernels' order: (kind, channel, prediction step)."""
    n, m, p, Lh = spec.n, spec.m, spec.p, spec.L
    out = []
    for rho in range((m + p) * (Lh + n)):
        k, ch = divmod(rho, m + p)
        kp = k - n
        term = spec.tec and kp >= Lh - n
        if ch < m:
            out.append(("ufix" if kp < 0 or term else "ufree", ch, kp))
        else:
            out.append(("wint" if kp < 0 else "wterm" if term else "wpred", ch - m, kp))
    return out


def solve_trailing_block(spec, u_d, y_d, u_past, y_past, box, max_iter=100):
    """The iteration of rr3_solve_box_kernel in numpy (no refinement pass: double precision on the CPU does not need it)."""
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
    # the table, by component (ascending position, the slack before the output on a shared row)
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
    # the kept factor of the empty active set, permuted
    K0 = (H @ H.T + lam * np.diag(D0))[np.ix_(perm, perm)]
    Lf = np.linalg.cholesky(K0)
    y = np.linalg.solve(Lf, t0[perm])
    beta = np.linalg.solve(Lf.T, y)
    act = np.zeros(len(tab), dtype=int)
    iters, status, peak = 0, "optimal", 0
    while True:
        iters += 1
        hat = a + c * beta[cpos]
        new = np.where(act > 0, (hat > hi).astype(int), np.where(act < 0, -(hat < lo).astype(int), (hat > hi).astype(int) - (hat < lo)))
        if np.array_equal(new, act):
            break
        act = new
        if iters >= max_iter:
            status = "solver_error"
            break
        lst = np.nonzero(act)[0]
        peak = max(peak, lst.size)
        E = np.zeros((r, lst.size))
        E[cpos[lst], np.arange(lst.size)] = 1.0
        assert not np.any(E[:n0])                       # the unit vectors vanish above the trailing block: W = [0; L_TT^-1 E_T]
        W = np.zeros((r, lst.size))
        W[n0:] = np.linalg.solve(Lf[n0:, n0:], E[n0:])
        shift = np.where(act[lst] > 0, hi[lst], lo[lst]) - a[lst]
        Sm = np.diag(1.0 / dd[lst]) - W.T @ W
        Ls = np.linalg.cholesky(Sm)                     # positive definite: K(A) >= G > 0
        hv = W.T @ y + (W.T @ W) @ shift
        ev = np.linalg.solve(Ls.T, np.linalg.solve(Ls, hv)) + shift
        beta = np.linalg.solve(Lf.T, y + W @ ev)
    # output stage: D(state), t(state) per row
    sa, say = np.zeros(r, int), np.zeros(r, int)
    for s, (i, isy) in enumerate(zip(cpos, cy)):
        (say if isy else sa)[i] = act[s]
    nu, ny = Ln * m, Ln * p
    ubar, ybar, sigma = np.zeros(nu), np.zeros(ny), np.zeros(ny)
    cost, both, signed = 0.0, 0, {}
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
                    signed[na + k * m + ch] = int(sa[i])
            continue
        j = k * p + ch
        if kind == "wint":
            sg = z - t0[rho]
        elif kind == "wterm":
            sg = z - y_s[ch]
        else:
            sg = sa[i] * bound if sa[i] else -lam * b_ / ls
        yb = (t - sa[i] * bound) if say[i] else z - sg
        ybar[j], sigma[j] = yb, sg
        cost += ls * sg * sg + (w[rho] * (yb - y_s[ch]) ** 2 if kind == "wpred" else 0.0)
        both += bool(sa[i] and say[i])
        if (i, "s") in seen:
            signed[na + nu + ny + j] = int(sa[i])
        if (i, "y") in seen:
            signed[na + nu + j] = int(say[i])
    return dict(status=status, iters=iters, signed=signed, cost=float(cost), optimal_u=ubar[n * m:].copy(), both=both, peak=peak,
                n0=n0, nA=nA)


CASES = [("box2", BOX2, "convex"), ("box4", BOX4, "none"), ("box4", BOX4, "convex"), ("box5", BOX5, "convex")]


@pytest.mark.parametrize("name,box,slack", CASES, ids=["%s-%s" % (c[0], c[2]) for c in CASES])
def test_trailing_block_formulation_is_the_full_space_iteration(name, box, slack):
    spec, d, up, yp = _four_tank(slack)
    for b in range(2):
        kw = {}
        if box["u"] is not None:
            kw.update(u_min=box["u"][0], u_max=box["u"][1])
        ylo, yhi = box["y"] if box["y"] is not None else (-INF, INF)
        sol = yref.solve_bounded(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], ylo, yhi, **kw)
        red = solve_trailing_block(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], box)
        eu = np.max(np.abs(red["optimal_u"] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(red["cost"] - sol.cost) / abs(sol.cost)
        print("%s %s b=%d: %s iters %d/%d k %d peak %d both %d n0 %d nA %d margin %.1e err_u %.1e err_cost %.1e" %
              (name, slack, b, sol.status, red["iters"], sol.iters, np.count_nonzero(sol.active), red["peak"], red["both"],
               red["n0"], red["nA"], sol.margin, eu, ec))
        assert red["status"] == sol.status == "optimal" and sol.margin >= 1e-7
        assert red["iters"] == sol.iters
        assert np.array_equal(np.array([red["signed"][int(i)] for i in sol.idx]), sol.active)
        assert eu < 1e-8 and ec < 1e-9, (eu, ec)


@pytest.mark.parametrize("box,slack", [(BOX2, "none"), (BOX2, "convex"), (BOX3, "none"), (BOX4, "none"), (BOX4, "convex")],
                         ids=["box2-none", "box2-convex", "box3-none", "box4-none", "box4-convex"])
def test_boxed_last_order_is_the_union(box, slack):
    spec, _, _, _ = _four_tank(slack)
    m, p = spec.m, spec.p
    r = (m + p) * spec.Ln
    perm, nA, cpos, cy = box_order(spec, box)
    assert np.array_equal(np.sort(perm), np.arange(r))                      # a permutation
    kinds = _kinds(spec)
    fin = lambda pair, ch: pair is not None and (np.isfinite(pair[0][ch]) or np.isfinite(pair[1][ch]))
    slack_row = lambda rho: slack == "convex" and kinds[rho][0] in ("wpred", "wterm")
    in_row = lambda rho: kinds[rho][0] == "ufree" and fin(box["u"], kinds[rho][1])
    out_row = lambda rho: kinds[rho][0] == "wpred" and fin(box["y"], kinds[rho][1])
    union = [rho for rho in range(r) if slack_row(rho) or in_row(rho) or out_row(rho)]
    assert nA == r - len(union)
    assert perm[nA:].tolist() == union                                      # exactly the union, time order inside the class
    assert perm[:nA].tolist() == [rho for rho in range(r) if rho not in set(union)]
    want = []                                                               # components: ascending position, slack before output
    for i in range(nA, r):
        rho = int(perm[i])
        want += [(i, 0)] * (int(slack_row(rho)) + int(in_row(rho))) + [(i, 1)] * int(out_row(rho))
    assert list(zip(cpos.tolist(), cy.tolist())) == want
    if box is BOX3:
        assert nA & ~63 > 0                                                 # one bounded input channel: a true trailing block
    no = box_order(spec, dict(u=None, y=None))
    assert no[2].size == 0 and no[1] == (r - sum(slack_row(rho) for rho in range(r)))
