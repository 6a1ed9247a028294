"""Per-instance bounds together with per-instance setpoints (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS): the fixtures, boxes and
references the CPU and the GPU tests share, each reference computed once per process.

A helper, not a test.  The reference is `_setpoint_box_ref.solve` / `schedule_loop`, run per instance with THAT INSTANCE's own
bounds and setpoints; a +-inf entry of a row leaves the component out of the helper's box (the kernels never activate it).

Step fixture: `_setpoint_box_ref.tank()` -- four-tank, L = 30, n = 4, N = 400 (136 rows), 8 instances, seeds 500 .. 507, data-tail
windows, its per-instance setpoints `us` / `ys`.  With t = b / 7:
  A: u in [-4 + 4 t, 6 - 4 t] on both channels, channel 0 unbounded where b % 4 == 3 (instance 0: [-4, 6]; instance 7: channel 1 in [0, 2]);
  C: A, plus y_min = [-inf, 0.3 + 0.1 t], y_max = [1.1 - 0.1 t, +inf], y_max[0] = +inf at b == 5.
Modes: slack NONE without and with the terminal constraint, the CONVEX slack box with it.

Loop fixture: `_tank_loop()` of tests/test_gpu_setpoint_box_law.py -- 4 instances, 21 steps, a switch at step 10.  With t = b / 3
the bounds are A's formula with channel 0 unbounded at b == 2; `none` (no terminal constraint) runs with the inputs only,
`convex-tec` with C's output bounds added.  NONE with output bounds at n_mpc_step = 1 is no compared case: one reference solve
there has margin 9e-8.

m != p: the plant and the rows of `mne_case()` in tests/test_gpu_instance_bounds.py (m = 2, p = 3, 45 rows, CONVEX with the
terminal constraint), per-instance setpoints = the spec's plus MNE_PERTURBATION * default_rng(MNE_SEED).uniform(-1, 1).
"""
import numpy as np

from oracle import ddmpc_oracle as orc

import _setpoint_box_ref as ref

INF = np.inf
B8 = ref.B8
MODES = {"none": (0, False), "none-tec": (0, True), "convex-tec": (1, True)}
NAMES = ("A", "C")
MARGIN = 1e-7                       # iters and the signed set are compared where the reference keeps at least this
A_NONE_ITERS = [5, 4, 5, 4, 5, 6, 7, 7]     # the reference's solve counts for A under `none`
BAD_US = [2.3, 1.0]                 # outside [0, 2] on channel 0, inside [-4, 6]
LOOP_B, LOOP_NMS = 4, (1, 4)
LOOP_MODES = {"none": "A", "convex-tec": "C"}
# 0.02 with default_rng(0).  Chosen on the CPU reference alone: with seed 23, the first tried, instance 2 has no active input at
# 0.02, 0.01, 0.005, 0.0025 and 0.001 (its one active input is marginal: shrinking moves it the wrong way), so the seed was changed
# instead of the size; with seed 0 every reference solve is optimal in 3 .. 5 solves, keeps margin >= 1.6e-3 and has at least one
# active input and one active output (tests/test_instance_setpoint_bounds_reference.py).
MNE_PERTURBATION, MNE_SEED = 0.02, 0

_CACHE = {}


def spec_of(mode):
    slack, tec = MODES[mode]
    return orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)


def box(name, B=B8, ufree=(3, 7), yfree=(5,)):
    """(u_min, u_max, y_min, y_max), [B, 2] each or None for a kind the box does not bound: t = b / (B - 1); ufree: the instances
    whose input channel 0 has no bound; yfree: the instances whose y_max[0] is +inf."""
    t = np.arange(B) / (B - 1.0)
    ulo = np.repeat((-4.0 + 4.0 * t)[:, None], 2, axis=1)
    uhi = np.repeat((6.0 - 4.0 * t)[:, None], 2, axis=1)
    for b in ufree:
        if b < B:
            ulo[b, 0], uhi[b, 0] = -INF, INF
    if name == "A":
        return ulo, uhi, None, None
    assert name == "C"
    ylo = np.stack([np.full(B, -INF), 0.3 + 0.1 * t], axis=1)
    yhi = np.stack([1.1 - 0.1 * t, np.full(B, INF)], axis=1)
    for b in yfree:
        if b < B:
            yhi[b, 0] = INF
    return ulo, uhi, ylo, yhi


def loop_box(name):
    return box(name, B=LOOP_B, ufree=(2,), yfree=())


def row(bx, b):
    """The keyword bounds of instance b for `_setpoint_box_ref.solve` / `schedule_loop`."""
    ulo, uhi, ylo, yhi = bx
    kw = dict(u_min=ulo[b], u_max=uhi[b])
    if ylo is not None:
        kw.update(y_min=ylo[b], y_max=yhi[b])
    return kw


def set_box(eng, bx):
    ulo, uhi, ylo, yhi = bx
    eng.set_instance_input_bounds(ulo, uhi)
    if ylo is not None:
        eng.set_instance_output_bounds(ylo, yhi)


def solve_at(mode, bx, b, us, ys, max_iter=100):
    t = ref.tank()
    return ref.solve(spec_of(mode), t["u_d"][b], t["y_d"][b], t["up"][b], t["yp"][b], us, ys, max_iter=max_iter, **row(bx, b))


def step_reference(name, mode, b):
    """Instance b of the step fixture at its own setpoint under its own row of box `name`."""
    key = ("step", name, mode, b)
    if key not in _CACHE:
        t = ref.tank()
        _CACHE[key] = solve_at(mode, box(name), b, t["us"][b], t["ys"][b])
    return _CACHE[key]


def loop_case(mode):
    """(case, u_ref, y_ref) of `_tank_loop` with the mode's spec."""
    from test_gpu_setpoint_box_law import _tank_loop
    case, u_ref, y_ref = _tank_loop()
    return dict(case, spec=spec_of(mode)), u_ref, y_ref


def loop_reference(mode, b, nms):
    """(u_sys, y_sys, x_end, u_past_end, y_past_end, sols) of instance b of the loop fixture."""
    key = ("loop", mode, b, nms)
    if key not in _CACHE:
        from test_gpu_setpoint_box_law import _ref_loop
        case, u_ref, y_ref = loop_case(mode)
        _CACHE[key] = _ref_loop(case, b, u_ref[b], y_ref[b], nms, row(loop_box(LOOP_MODES[mode]), b))
    return _CACHE[key]


def mne():
    """(case, u_min, u_max, y_min, y_max, u_s [4, 2], y_s [4, 3]) of the m != p case."""
    if "mne" not in _CACHE:
        from test_gpu_instance_bounds import mne_case
        case, ulo, uhi, ylo, yhi = mne_case()
        s = case["spec"]
        rng = np.random.default_rng(MNE_SEED)
        us = np.asarray(s.u_s, float) + MNE_PERTURBATION * rng.uniform(-1.0, 1.0, (4, s.m))
        ys = np.asarray(s.y_s, float) + MNE_PERTURBATION * rng.uniform(-1.0, 1.0, (4, s.p))
        _CACHE["mne"] = (case, ulo, uhi, ylo, yhi, us, ys)
    return _CACHE["mne"]


def mne_reference(b):
    key = ("mne", b)
    if key not in _CACHE:
        case, ulo, uhi, ylo, yhi, us, ys = mne()
        _CACHE[key] = ref.solve(case["spec"], case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], us[b], ys[b],
                                u_min=ulo[b], u_max=uhi[b], y_min=ylo[b], y_max=yhi[b])
    return _CACHE[key]


def mne_active(s, sol):
    """(active inputs, active outputs) of a BoundedSolution of the m != p case (x = [alpha; ubar; ybar; sigma])."""
    x0 = sol.x.size - 2 * s.Ln * s.p - s.Ln * s.m
    usec = (sol.idx >= x0) & (sol.idx < x0 + s.Ln * s.m)
    ysec = (sol.idx >= x0 + s.Ln * s.m) & (sol.idx < x0 + s.Ln * (s.m + s.p))
    return int(np.sum(usec & (sol.active != 0))), int(np.sum(ysec & (sol.active != 0)))
