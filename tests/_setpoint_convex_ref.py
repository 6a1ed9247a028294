"""Cases, references and a numpy model for DDMPC_OPT_SETPOINT_CONVEX_LAW: per-instance, per-step setpoints under the CONVEX slack
box, slack-only or next to input / output bounds (the SLACK instantiations of csrc/ddmpc_setpoint_box_law.hpp).

A helper, not a test.  The references are `_setpoint_box_ref.solve` / `_setpoint_box_ref.schedule_loop` with a CONVEX spec: their
union box holds the slack components next to the bounded inputs and outputs, and the slack components alone without bounds.
`BoundedSolution.active` is in the order of x = [alpha; ubar; ybar; sigma]: inputs, outputs, slack.

Data, windows and setpoints are those of `_setpoint_box_ref.tank()` (four-tank, L = 30, n = 4, N = 400: 136 rows, batch 8).
"""
import dataclasses

import numpy as np

from oracle import ddmpc_oracle as orc

import _setpoint_box_ref as bref
import _setpoint_law_ref as sref

INF = np.inf
B8 = bref.B8
tank = bref.tank

# name: the bounds
BOXES = {
    "slack-only": {},
    "wide": dict(u_min=[-4.0, -4.0], u_max=[6.0, 6.0]),
    "tight": dict(u_min=[0.0, 0.0], u_max=[2.0, 2.0]),
    "y": dict(y_min=[0.3, 0.3], y_max=[1.1, 1.1]),
}
# (box, terminal constraint): active counts (lo, hi) of the reference, the smallest margin it keeps, home of the k x k system,
# whether `iters` and the signed set are compared.  (With the terminal constraint instance 0 keeps 1.84e-4 in all three boxes
# that have it in the rule: "2e-4" would be its rounding.  "tight" with the terminal constraint: instance 3 sits at margin 1e-7, so
# the case serves the bars only.)
CASES = {
    ("slack-only", True): dict(k=(1, 4), margin=1.8e-4, home="lds", rule=True),
    ("slack-only", False): dict(k=(1, 4), margin=2e-4, home="lds", rule=True),
    ("wide", True): dict(k=(8, 12), margin=1.8e-4, home="lds", rule=True),
    ("wide", False): dict(k=(8, 12), margin=2e-4, home="lds", rule=True),
    ("tight", False): dict(k=(36, 53), margin=3e-6, home="global", rule=True),
    ("tight", True): dict(k=None, margin=None, home=None, rule=False),
    ("y", True): dict(k=(4, 10), margin=1.8e-4, home="lds", rule=True),
    ("y", False): dict(k=(4, 10), margin=1.8e-4, home="lds", rule=True),
}
# diagonal weights (Q, R of `_setpoint_box_ref.spec(diag=True)`): (box, terminal constraint)
DIAG_CASES = [("slack-only", True), ("wide", False)]

_CACHE = {}


def spec(tec=True, diag=False):
    s = orc.spec_from_params(slack_var_constraint_type=1, tec=tec)
    if diag:
        d = bref.spec(tec, diag=True)
        s = dataclasses.replace(s, Q=d.Q, R=d.R)
    return s


def step_reference(box, tec, diag, b):
    key = ("step", box, tec, diag, b)
    if key not in _CACHE:
        t = tank()
        _CACHE[key] = bref.solve(spec(tec, diag), t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], t["us"][b], t["ys"][b],
                                 **BOXES[box])
    return _CACHE[key]


def n_boxed(spec_, bounds):
    """(inputs, outputs) among the helper's boxed components; the slack components follow them."""
    nfree = spec_.L - spec_.n if spec_.tec else spec_.L

    def count(lo, hi, nchan):
        if lo is None:
            return 0
        lo, hi = np.broadcast_to(np.asarray(lo, float), (nchan,)), np.broadcast_to(np.asarray(hi, float), (nchan,))
        return nfree * int(np.count_nonzero(np.isfinite(lo) | np.isfinite(hi)))
    return count(bounds.get("u_min"), bounds.get("u_max"), spec_.m), count(bounds.get("y_min"), bounds.get("y_max"), spec_.p)


# ------------------------------------------------------------------------------------------------------------------------
# The fused loop: instances 0 .. 3 of tank(), from the end of their data; 20 steps; the setpoint of every instance changes at
# steps 7 and 14 (three equilibria u_s +- 0.3 with y_s through the dc gain, default_rng(31)); noise eps_max U(-1, 1),
# default_rng(32).  With n_mpc_step = 4 the solves at steps 8 and 16 are the first to see a new setpoint.  Held on the CPU:
# every solve of every instance is optimal, slack-only and under u in [-4, 6], n_mpc_step 1 and 4.
LOOP_B, LOOP_STEPS, LOOP_CHANGES, LOOP_NMS = 4, 20, (7, 14), (1, 4)
LOOP_BOXES = ("slack-only", "wide")


def loop_case():
    if "loop" not in _CACHE:
        t, s, pl = tank(), spec(), orc.FOUR_TANK
        dc = bref.dc_gain(pl)
        rng = np.random.default_rng(31)
        us3 = s.u_s + rng.uniform(-0.3, 0.3, (3, LOOP_B, s.m))
        seg = np.searchsorted(np.asarray(LOOP_CHANGES), np.arange(LOOP_STEPS), side="right")
        u_ref = np.stack([us3[seg, b] for b in range(LOOP_B)])                  # [B, steps, m]
        y_ref = u_ref @ dc.T
        w = s.eps_max * np.random.default_rng(32).uniform(-1.0, 1.0, (LOOP_B, LOOP_STEPS, s.p))
        case = dict(spec=s, plant=pl, B=LOOP_B, w=w, x0=t["x_end"][:LOOP_B].copy(),
                    **{k: t[k][:LOOP_B] for k in ("u_d", "y_d", "up", "yp")})
        _CACHE["loop"] = (case, u_ref, y_ref)
    return _CACHE["loop"]


def loop_reference(box, b, nms):
    """(u_sys, y_sys, x_end, u_past_end, y_past_end, sols) of instance b."""
    key = ("loop", box, b, nms)
    if key not in _CACHE:
        case, u_ref, y_ref = loop_case()
        pl = case["plant"]
        plant = orc.Plant(pl["A"], pl["B"], pl["C"], pl["D"], pl["eps_max"])
        plant.x = case["x0"][b].copy()
        u, y, up, yp, sols = bref.schedule_loop(case["spec"], case["u_d"][b], case["y_d"][b], plant, case["w"][b], u_ref[b],
                                                y_ref[b], n_mpc_step=nms, u_past=case["up"][b], y_past=case["yp"][b],
                                                **BOXES[box])
        _CACHE[key] = (u, y, plant.x, up, yp, sols)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------------
def model_step(spec_, u_d, y_d, u_past, y_past, u_s, y_s, u_min=None, u_max=None, y_min=None, y_max=None, max_iter=100):
    """What the step kernel computes, in numpy -> (optimal_u, cost, status, iters, signed set by boxed component, rows of the
    components, kinds of the components: 0 slack, 1 input, 2 output).

    beta0 = past P + s S with (P, S) of `_setpoint_law_ref.law`; the box list in ascending row order, the slack before the
    output on a shared row; offsets a = 0 for a slack component and the instance's setpoint of the channel otherwise;
    M = K0^-1 E by boxed row; the rule of BoxTab::test from the empty set; the output stage with the instance's setpoint as
    target."""
    n, m, p, L, Ln = spec_.n, spec_.m, spec_.p, spec_.L, spec_.Ln
    nch = m + p
    sp = sref.with_setpoints(spec_, u_s, y_s)
    K0, G, _ = sref.reduced_matrix(spec_, u_d, y_d)
    P, S = sref.law(spec_, u_d, y_d)
    lam, ls, bound = spec_.lamb_alpha * spec_.eps_max, spec_.lamb_sigma, spec_.c * spec_.eps_max
    s = np.concatenate([sp.u_s, sp.y_s])
    u_past, y_past = np.asarray(u_past, float).reshape(-1), np.asarray(y_past, float).reshape(-1)
    beta0 = np.concatenate([u_past, y_past]) @ P + s @ S
    lo_ch = np.concatenate([np.broadcast_to(-INF if u_min is None else np.asarray(u_min, float), (m,)),
                            np.broadcast_to(-INF if y_min is None else np.asarray(y_min, float), (p,))])
    hi_ch = np.concatenate([np.broadcast_to(INF if u_max is None else np.asarray(u_max, float), (m,)),
                            np.broadcast_to(INF if y_max is None else np.asarray(y_max, float), (p,))])
    nfree = L - n if spec_.tec else L
    qd, rd = np.diag(spec_.Q), np.diag(spec_.R)
    rows, kind, a, c, lo, hi, d = [], [], [], [], [], [], []

    def add(rho, kd, a_, d_, lo_, hi_):
        rows.append(rho); kind.append(kd); a.append(a_); c.append(-d_); lo.append(lo_); hi.append(hi_); d.append(d_)

    for rho in range(Ln * nch):
        k, ch = divmod(rho, nch)
        if k < n:
            continue
        free, fin = k < n + nfree, np.isfinite(lo_ch[ch]) or np.isfinite(hi_ch[ch])
        if ch < m:
            if free and fin:
                add(rho, 1, s[ch], lam / rd[(k - n) * m + ch], lo_ch[ch], hi_ch[ch])
            continue
        add(rho, 0, 0.0, lam / ls, -bound, bound)                 # sigma = -lam beta / lamb_sigma inside +- c eps_max
        if free and fin:
            add(rho, 2, s[ch], lam / qd[(k - n) * p + (ch - m)], lo_ch[ch], hi_ch[ch])
    rows, kind = np.asarray(rows, int), np.asarray(kind, int)
    a, c, lo, hi, d = (np.asarray(v, float) for v in (a, c, lo, hi, d))
    M = np.linalg.solve(K0, np.eye(Ln * nch))                  # M[:, rho] = K0^-1 e_rho

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
        MAA = M[np.ix_(rows[A], rows[A])]                         # (two components of one row share its column)
        # K(A) = K0 - E_A diag(d_A) E_A',  t(A) = t0 + E_A shift_A:  beta = beta0 + M_A ev
        ev = shift + np.linalg.solve(np.diag(1.0 / d[A]) - MAA, beta0[rows[A]] + MAA @ shift)
        beta = beta0 + M[:, rows[A]] @ ev
    # output stage, the instance's setpoint as target
    state = {(int(rows[j]), int(kind[j])): (int(act[j]), hi[j] if act[j] > 0 else lo[j]) for j in range(rows.size)}
    ubar, ybar, sigma = np.zeros((Ln, m)), np.zeros((Ln, p)), np.zeros((Ln, p))
    for rho in range(Ln * nch):
        k, ch = divmod(rho, nch)
        free = n <= k < n + nfree
        if ch < m:
            if k < n:
                ubar[k, ch] = u_past[k * m + ch]
            elif not free:
                ubar[k, ch] = sp.u_s[ch]
            else:
                sa, bd = state.get((rho, 1), (0, 0.0))
                ubar[k, ch] = bd if sa else sp.u_s[ch] - lam * beta[rho] / rd[(k - n) * m + ch]
            continue
        cy = ch - m
        if k < n:
            ybar[k, cy], sigma[k, cy] = y_past[k * p + cy], -lam * beta[rho] / ls
            continue
        sa, _ = state[(rho, 0)]
        sigma[k, cy] = sa * bound if sa else -lam * beta[rho] / ls
        if not free:
            ybar[k, cy] = sp.y_s[cy]
        else:
            say, bd = state.get((rho, 2), (0, 0.0))
            ybar[k, cy] = bd if say else sp.y_s[cy] - lam * beta[rho] / qd[(k - n) * p + cy]
    du = (ubar[n:] - sp.u_s).reshape(-1)
    dy = (ybar[n:] - sp.y_s).reshape(-1)
    sg = sigma.reshape(-1)
    cost = float(du @ (rd * du) + dy @ (qd * dy) + lam * beta @ (G @ beta) + ls * sg @ sg)
    return ubar[n:].reshape(-1).copy(), cost, status, iters, act, rows, kind


def helper_order(spec_, act, rows, kind):
    """The model's signed set in the order of `BoundedSolution.active`: inputs, outputs, slack, each by (time, channel)."""
    return act[np.lexsort((rows, (kind + 2) % 3))]              # kind 1 (input) -> 0, 2 (output) -> 1, 0 (slack) -> 2
