"""Reference solution of the Data-Driven MPC QP with output bounds y_min <= ybar[k] <= y_max (and, optionally, input bounds) on
the free prediction steps.

A helper, not a test.  It is tests/_input_bounds_ref.py with a larger union box: the entries (n + k) p + ch of ybar on the free
prediction steps k (all L, or the first L - n with the terminal constraint) of the channels with a finite bound join the slack
components and the bounded inputs, each with its own lo / hi.  The iteration, `margin`, the certificate and the loop driver are
that module's own functions, called with its `box_of` replaced for the duration of the call; the bounds travel through its
`u_min` / `u_max` arguments as the pairs (u_min, y_min) / (u_max, y_max).
"""
from contextlib import contextmanager

import numpy as np

import _input_bounds_ref as ref

INF = np.inf


def box_of(spec, qp, lo_pair, hi_pair):
    """(idx, lo, hi) of the union box over [alpha; ubar; ybar; sigma]: slack, bounded inputs, bounded outputs, ascending."""
    (u_min, y_min), (u_max, y_max) = lo_pair, hi_pair
    idx, lo, hi = (list(a) for a in _INPUT_BOX_OF(spec, qp, u_min, u_max))
    n, p, L = spec.n, spec.p, spec.L
    y_min = np.broadcast_to(np.asarray(y_min, float), (p,))
    y_max = np.broadcast_to(np.asarray(y_max, float), (p,))
    y0 = qp.sl["ybar"].start
    nfree = L - n if spec.tec else L
    for k in range(nfree):
        for ch in range(p):
            if np.isfinite(y_min[ch]) or np.isfinite(y_max[ch]):
                idx.append(y0 + (n + k) * p + ch)
                lo.append(float(y_min[ch]))
                hi.append(float(y_max[ch]))
    order = np.argsort(idx)
    return np.asarray(idx, int)[order], np.asarray(lo, float)[order], np.asarray(hi, float)[order]


_INPUT_BOX_OF = ref.box_of


@contextmanager
def _union_box():
    ref.box_of = box_of
    try:
        yield
    finally:
        ref.box_of = _INPUT_BOX_OF


def _pairs(u_min, u_max, y_min, y_max):
    return (-INF if u_min is None else u_min, y_min), (INF if u_max is None else u_max, y_max)


def solve_bounded(spec, u_d, y_d, u_past, y_past, y_min, y_max, u_min=None, u_max=None, max_iter: int = 100):
    """`_input_bounds_ref.solve_bounded` over the union box with the outputs (u_min / u_max None: no input bounds)."""
    lo, hi = _pairs(u_min, u_max, y_min, y_max)
    with _union_box():
        return ref.solve_bounded(spec, u_d, y_d, u_past, y_past, lo, hi, max_iter=max_iter)


def kkt_certificate(spec, u_d, y_d, u_past, y_past, y_min, y_max, x, u_min=None, u_max=None, act_tol: float = 1e-9):
    lo, hi = _pairs(u_min, u_max, y_min, y_max)
    with _union_box():
        return ref.kkt_certificate(spec, u_d, y_d, u_past, y_past, lo, hi, x, act_tol=act_tol)


def closed_loop_bounded(spec, u_d, y_d, plant, w_sys, y_min, y_max, u_min=None, u_max=None, n_mpc_step=1, u_past=None, y_past=None):
    lo, hi = _pairs(u_min, u_max, y_min, y_max)
    with _union_box():
        return ref.closed_loop_bounded(spec, u_d, y_d, plant, w_sys, lo, hi, n_mpc_step=n_mpc_step, u_past=u_past, y_past=y_past)
