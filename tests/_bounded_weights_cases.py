"""Bounded controllers under weights that change with the step and with the channel: the fixtures, weight profiles, boxes and
cases that tests/test_bounded_weights_reference.py (CPU, the premises) and tests/test_gpu_bounded_weights.py (the kernels) share,
and the reference solution of every (case, instance), computed once per process.

A helper, not a test.  Fixtures (the project's own, at the smallest sizes that reach the kernels):
  small     four-tank, L = 30, n = 4, N = 400, 136 rows, seeds 500 .. 507, the data tail as the window
  small-mp  m = 2, p = 3, n = 2, L = 7, 45 rows, D != 0 (test_gpu_closed_loop_plants.make_case), seeds 0 .. 7
  large     four-tank, L = 70, N = 700, 296 rows, seeds 0 .. 7 (DDMPC_OPT_LARGE_BOUNDS = 1)
  large-mp  test_gpu_closed_loop_plants.LARGE: (m, p, n, L) = (2, 3, 2, 58), 300 rows, seeds 0 .. 3
Weight profiles, all on `ramp` of tests/test_gpu_large_weights.py (no two steps of a channel and no two channels of a step share
a value; q0, r0: the scalars the spec came with):
  ramp      the ramp itself
  r-zero    the ramp with r[2::3, 1] = 0: input channel 1 unweighted at every third step
  q-zero    the ramp with q[0::3, 1] = 0: output channel 1 unweighted at every third step
The zero profiles go with boxes that leave the unweighted channel unbounded and with slack NONE (under CONVEX a Q entry of 0 is
refused with output bounds; the r-zero case beyond 271 rows also runs under CONVEX, input bounds only).

Rows.  A case uses the first four instances of its fixture, with two exceptions.  The zero-weight cases use the first three: their
references come from the full-space helper alone (2 .. 6 s per instance at 296 rows), and three is what their margins were
checked on (>= 8.7e-6).  "s-uy2-convex" (u in [-4, 6] with the two-sided output box, CONVEX) uses rows 2 .. 5: on rows 1 and 6 the
reference iteration cycles to its cap, on rows 0 and 7 it ends with margins of 5.3e-7 and 7.7e-7, below the 1e-6 of this size;
rows 2 .. 5 end optimal with margins of 2.4e-6 .. 2.1e-5.  The margins of every row used are asserted, and printed, by
tests/test_bounded_weights_reference.py.

Every component of a box has its own d_s = lam / r (inputs), lam / q (outputs) or lam / lamb_sigma (slacks), lam = lamb_alpha *
eps_max: `d_s_of` names it from the position in x = [alpha; ubar; ybar; sigma], for the premise that an active set holds at
least three distinct values.
"""
import dataclasses

import numpy as np

from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

import _output_bounds_ref as yref
import test_gpu_closed_loop_plants as CP
from test_gpu_large_weights import ramp, with_weights
from test_gpu_round5 import _four_tank_long

INF = np.inf
MARGIN = {"small": 1e-6, "small-mp": 1e-6, "large": 1e-7, "large-mp": 1e-7}

# boxes of the four-tank fixtures
U_02 = ([0.0, 0.0], [2.0, 2.0])                        # = U_CAP of test_gpu_large_bounds.py
U_ONE_SIDED = ([-INF, 0.5], [3.0, INF])
U_WIDE = ([-4.0, -4.0], [6.0, 6.0])
U_CH0 = ([-1.0, -INF], [3.0, INF])
U0_02 = ([0.0, -INF], [2.0, INF])                      # item 7: u_0 in [0, 2]
U0_WIDE = ([-4.0, -INF], [6.0, INF])                   # item 7: u_0 in [-4, 6]
Y_UP = ([-INF, -INF], [0.66, 0.775])
Y0_UP = ([-INF, -INF], [0.66, INF])                    # item 7: y_0 <= 0.66
Y_TWO_SIDED = ([0.60, 0.72], [0.70, 0.82])             # test_gpu_output_bounds.BOXES["two-sided"]
Y_TIGHT = ([0.645, 0.765], [0.655, 0.775])             # case D of test_gpu_large_box_capacity.py
# the m != p plants.  Chosen from the unbounded reference alone: at 45 rows (u_s = (0.33, 0.32), y_s = (1.08, 0.49, 0.14)) input
# channel 1 reaches 0.60 .. 0.91 and output channel 1 falls to -0.04 .. -0.62 on seeds 0 .. 3; at 300 rows (u_s = (0.43, 0.46),
# y_s = (-0.32, 2.53, 4.29)) input channel 1 reaches 0.90 .. 1.28 and output channel 1 falls to -3.3 .. 1.3
MP_U, MP_Y = ([-INF, -INF], [INF, 0.45]), ([-INF, 0.1, -INF], [INF, INF, INF])
LMP_U, LMP_Y = ([-INF, -INF], [INF, 0.8]), ([-INF, 1.0, -INF], [INF, INF, INF])


def r_zero(spec):
    q, r = ramp(spec)
    r[2::3, 1] = 0.0
    return q, r


def q_zero(spec):
    q, r = ramp(spec)
    q[0::3, 1] = 0.0
    return q, r


PROFILES = {"ramp": ramp, "r-zero": r_zero, "q-zero": q_zero}


@dataclasses.dataclass(frozen=True)
class Case:
    fixture: str
    slack: str                      # "none" / "convex"
    tec: bool
    ubox: tuple = None
    ybox: tuple = None
    profile: str = "ramp"
    rows: tuple = (0, 1, 2, 3)      # the instances of the fixture the case uses


CASES = {
    # ---- up to 271 rows (items 1, 2, 3, 4, 7)
    "s-u02-convex":      Case("small", "convex", True, U_02),
    "s-uy-none":         Case("small", "none", False, U_ONE_SIDED, Y_UP),
    "s-uy2-convex":      Case("small", "convex", True, U_WIDE, Y_TWO_SIDED, "ramp", (2, 3, 4, 5)),
    "s-rzero-u0":        Case("small", "none", False, U0_02, None, "r-zero", (0, 1, 2)),
    "s-qzero-y0":        Case("small", "none", False, None, Y0_UP, "q-zero", (0, 1, 2)),
    "s-qzero-y0-u0":     Case("small", "none", False, U0_WIDE, Y0_UP, "q-zero", (0, 1, 2)),
    # ---- beyond 271 rows (items 8 .. 14, 16)
    "l-ucap-convex":     Case("large", "convex", True, U_02),
    "l-uy-none":         Case("large", "none", True, U_WIDE, Y_UP),
    "l-uch0-none":       Case("large", "none", True, U_CH0),
    "l-ytight-convex":   Case("large", "convex", True, None, Y_TIGHT),
    "l-rzero-u0":        Case("large", "none", True, U0_02, None, "r-zero", (0, 1, 2)),
    "l-rzero-u0-convex": Case("large", "convex", True, U0_02, None, "r-zero", (0, 1, 2)),
    "l-qzero-y0":        Case("large", "none", True, None, Y0_UP, "q-zero", (0, 1, 2)),
    "l-qzero-y0-u0":     Case("large", "none", True, U0_WIDE, Y0_UP, "q-zero", (0, 1, 2)),
    # ---- m != p (items 6, 15): one input and one output channel bounded, CONVEX
    "s-mp-convex":       Case("small-mp", "convex", True, MP_U, MP_Y),
    "l-mp-convex":       Case("large-mp", "convex", True, LMP_U, LMP_Y),
}

_FIX, _REF = {}, {}


def fixture(name, slack, tec):
    """(spec with its scalar weights, N, dict of u_d, y_d, up, yp, x_end and the plant matrices) of a fixture, 8 instances."""
    key = (name, slack, tec)
    if key in _FIX:
        return _FIX[key]
    if name == "small":
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0, tec=tec)
        N = 400
        d = generate_batch(range(500, 508), N=N)
        up, yp = d["u_d"][:, -4:, :].reshape(8, -1).copy(), d["y_d"][:, -4:, :].reshape(8, -1).copy()
        out = dict(u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, x_end=d["x_end"], plant=orc.FOUR_TANK)
    elif name == "large":
        assert tec
        spec, d, up, yp = _four_tank_long(8, 70, 700, slack)
        N = 700
        out = dict(u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, x_end=d["x_end"], plant=orc.FOUR_TANK)
    else:
        assert tec
        if name == "small-mp":
            case = CP.make_case(2, 3, 1, 2, 7, slack, feedthrough=True, B=8, n_steps=6)
        else:
            g = CP.LARGE
            case = CP.make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], slack, B=4, n_steps=g["n_steps"], seed0=g["seed0"])
        spec, N = case["spec"], case["N"]
        out = dict(u_d=case["u_d"], y_d=case["y_d"], up=case["up"], yp=case["yp"], x_end=case["x0"], plant=case["plant"],
                   w=case["w"])
    _FIX[key] = (spec, N, out)
    return _FIX[key]


def case_of(name):
    """(Case, weighted spec, N, data) of a case."""
    c = CASES[name]
    spec0, N, d = fixture(c.fixture, c.slack, c.tec)
    return c, with_weights(spec0, *PROFILES[c.profile](spec0)), N, d


def solve_ref(spec, d, b, ubox, ybox, up=None, yp=None, max_iter=100):
    """The full-space helper on instance b of the data `d` (at the window up, yp; default: the fixture's)."""
    ylo, yhi = ybox if ybox is not None else (-INF, INF)
    kw = dict(u_min=ubox[0], u_max=ubox[1]) if ubox is not None else {}
    return yref.solve_bounded(spec, d["u_d"][b], d["y_d"][b], d["up"][b] if up is None else up, d["yp"][b] if yp is None else yp,
                              ylo, yhi, max_iter=max_iter, **kw)


def reduced(name):
    """Whether `reference` of a case is the reduced-space helper."""
    c = CASES[name]
    return c.fixture == "large" and c.profile == "ramp"


def solve_reduced(spec, d, b, ubox, ybox, up=None, yp=None, max_iter=100):
    """The reduced-space helper on instance b of the data `d` (at the window up, yp; default: the fixture's)."""
    import _large_box_ref as lref                          # (needs the built library for the host's "boxed last" order)
    return lref.solve_reduced(spec, d["u_d"][b], d["y_d"][b], d["up"][b] if up is None else up, d["yp"][b] if yp is None else yp,
                              dict(u=ubox, y=ybox), max_iter=max_iter)


def reference(name, b, spec=None, tag=None, full=False):
    """The reference solution of instance b of a case, once per process: the full-space helper (tests/_output_bounds_ref.py), or
    for the 296-row ramp cases the reduced-space helper tests/_large_box_ref.solve_reduced (0.2 s instead of 2 .. 6 s per
    instance, with the set size of every iteration; the premises test holds it against the full-space helper on instance 0 of each
    such case; `full`: the full-space helper all the same).  It cannot state the exact zero weight, whose cases stay on the
    full-space helper.  `spec` / `tag`: the same case under other weights (the mutations of the premises test), cached under its
    tag."""
    key = (name, b, tag, full)
    if key not in _REF:
        c, s, N, d = case_of(name)
        fn = solve_reduced if reduced(name) and not full else solve_ref
        _REF[key] = fn(s if spec is None else spec, d, b, c.ubox, c.ybox)
    return _REF[key]


def loop_ref(spec, d, b, w, ubox, ybox, nms):
    """(u_sys, y_sys, x_end) of tests/_output_bounds_ref.closed_loop_bounded on instance b of the data `d` from the fixture's
    window and end state under the noise w [steps, p]; it raises unless every solve of the loop is optimal."""
    P = d["plant"]
    plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
    plant.x = d["x_end"][b].copy()
    ylo, yhi = ybox if ybox is not None else (-INF, INF)
    kw = dict(u_min=ubox[0], u_max=ubox[1]) if ubox is not None else {}
    ur, yr = yref.closed_loop_bounded(spec, d["u_d"][b], d["y_d"][b], plant, w, ylo, yhi, n_mpc_step=nms, u_past=d["up"][b],
                                      y_past=d["yp"][b], **kw)
    return ur, yr, plant.x.copy()


# ---- item 5: box C of tests/_instance_bounds_cases.py on the first 8 instances (the seeds of the small fixture), slack NONE
def instance_case():
    """(weighted spec, N, data, (u_min, u_max, y_min, y_max) with one row per instance)."""
    import _instance_bounds_cases as IC
    spec0, N, d = fixture("small", "none", False)
    return with_weights(spec0, *ramp(spec0)), N, d, tuple(a[:8] for a in IC.box("C"))


def instance_reference(b):
    """Instance b at the data tail under ITS row of box C, once per process."""
    if ("instance", b) not in _REF:
        spec, N, d, (ulo, uhi, ylo, yhi) = instance_case()
        _REF[("instance", b)] = solve_ref(spec, d, b, (ulo[b], uhi[b]), (ylo[b], yhi[b]))
    return _REF[("instance", b)]


def instance_loop_noise():
    return 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (8, 6, 2))


def instance_loop_reference(b):
    """The 6-step loop (n_mpc_step = 1) of instance b under its row of box C, once per process."""
    if ("instance-loop", b) not in _REF:
        spec, N, d, (ulo, uhi, ylo, yhi) = instance_case()
        _REF[("instance-loop", b)] = loop_ref(spec, d, b, instance_loop_noise()[b], (ulo[b], uhi[b]), (ylo[b], yhi[b]), 1)
    return _REF[("instance-loop", b)]


def sections(spec, n_cols):
    """Sizes of alpha, ubar, ybar (= sigma) in x = [alpha; ubar; ybar; sigma]."""
    return n_cols - spec.Ln + 1, spec.Ln * spec.m, spec.Ln * spec.p


def d_s_of(spec, N, idx):
    """d_s of the boxed components at the positions `idx` of x: lam / r[step, channel] for an input, lam / q[step, channel] for
    an output, lam / lamb_sigma for a slack."""
    na, nu, ny = sections(spec, N)
    lam = spec.lamb_alpha * spec.eps_max
    q, r = np.diag(spec.Q), np.diag(spec.R)
    out = []
    for i in np.asarray(idx, int):
        if i < na + nu:
            k, ch = divmod(i - na, spec.m)
            out.append(lam / r[(k - spec.n) * spec.m + ch])
        elif i < na + nu + ny:
            k, ch = divmod(i - na - nu, spec.p)
            out.append(lam / q[(k - spec.n) * spec.p + ch])
        else:
            out.append(lam / spec.lamb_sigma)
    return np.array(out)
