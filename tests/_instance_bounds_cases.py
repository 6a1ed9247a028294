"""Per-instance bounds (ddmpc_set_instance_input_bounds / ddmpc_set_instance_output_bounds): the fixture and the three boxes the
CPU and the GPU tests share, and the reference of every instance computed once per process.

A helper, not a test.  Fixture: four-tank, L = 30, n = 4, N = 400, 32 instances (seeds 500 .. 531), past window = data tail.
With t = b / 31:
  A (inputs):  u in [-4 + 4.5 t, 6 - 4.5 t] on both channels, channel 0 unbounded where b % 4 == 3;
  B (outputs): the three boxes of test_gpu_output_bounds.BOXES and "no bound", assigned as (b // 2) % 4;
  C (both):    u in [-4 - t, 6 + t], channel 0 unbounded where b % 4 == 3; y <= [0.66 + 0.03 t, 0.775 + 0.03 t], output channel 1
               unbounded where b % 8 == 5.
The reference of instance b is tests/_output_bounds_ref.solve_bounded with ITS OWN bounds (infinite ones leave the component out
of the helper's box, as the kernels never activate it), so a per-instance reference is a loop over the batch.
"""
import numpy as np

from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

import _output_bounds_ref as yref

INF = np.inf
B32, SEED0 = 32, 500
MODES = {"convex-tec": (1, True), "none": (0, False)}
Y_BOXES = [([0.60, 0.72], [0.70, 0.82]),          # test_gpu_output_bounds.BOXES: two-sided, mild-upper, one-channel
           ([-INF, -INF], [0.66, 0.775]),
           ([-INF, 0.70], [INF, 0.80]),
           ([-INF, -INF], [INF, INF])]            # ... and no bound
NAMES = ("A", "B", "C")

_DATA = {}
_REF = {}


def data():
    if not _DATA:
        d = generate_batch(range(SEED0, SEED0 + B32), N=400)
        _DATA.update(d=d, up=d["u_d"][:, -4:, :].reshape(B32, -1).copy(), yp=d["y_d"][:, -4:, :].reshape(B32, -1).copy())
    return _DATA["d"], _DATA["up"], _DATA["yp"]


def spec_of(mode):
    slack, tec = MODES[mode]
    return orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)


def box(name):
    """(u_min, u_max, y_min, y_max), each [32, 2] or None for a kind the box does not bound."""
    t = np.arange(B32) / (B32 - 1.0)
    b = np.arange(B32)
    if name == "A":
        lo = np.repeat((-4.0 + 4.5 * t)[:, None], 2, axis=1)
        hi = np.repeat((6.0 - 4.5 * t)[:, None], 2, axis=1)
        lo[b % 4 == 3, 0], hi[b % 4 == 3, 0] = -INF, INF
        return lo, hi, None, None
    if name == "B":
        lo = np.array([Y_BOXES[(i // 2) % 4][0] for i in b], dtype=float)
        hi = np.array([Y_BOXES[(i // 2) % 4][1] for i in b], dtype=float)
        return None, None, lo, hi
    if name == "C":
        ulo = np.repeat((-4.0 - t)[:, None], 2, axis=1)
        uhi = np.repeat((6.0 + t)[:, None], 2, axis=1)
        ulo[b % 4 == 3, 0], uhi[b % 4 == 3, 0] = -INF, INF
        ylo = np.full((B32, 2), -INF)
        yhi = np.stack([0.66 + 0.03 * t, 0.775 + 0.03 * t], axis=1)
        yhi[b % 8 == 5, 1] = INF
        return ulo, uhi, ylo, yhi
    raise KeyError(name)


def rows_of(bx, i):
    """Instance i's own (u_min, u_max, y_min, y_max) for the helper: infinite arrays for a kind the box does not bound."""
    ulo, uhi, ylo, yhi = bx
    none_lo, none_hi = np.full(2, -INF), np.full(2, INF)
    return (none_lo if ulo is None else ulo[i], none_hi if uhi is None else uhi[i],
            none_lo if ylo is None else ylo[i], none_hi if yhi is None else yhi[i])


def reference(name, mode, i, max_iter=100):
    """The helper's solution of instance i of box `name` at the data tail, computed once."""
    key = (name, mode, i, max_iter)
    if key not in _REF:
        d, up, yp = data()
        ulo, uhi, ylo, yhi = rows_of(box(name), i)
        _REF[key] = yref.solve_bounded(spec_of(mode), d["u_d"][i], d["y_d"][i], up[i], yp[i], ylo, yhi, u_min=ulo, u_max=uhi,
                                       max_iter=max_iter)
    return _REF[key]


def set_box(eng, bx):
    """The box on an engine through the per-instance calls (a kind the box does not bound is left alone)."""
    ulo, uhi, ylo, yhi = bx
    if ulo is not None:
        eng.set_instance_input_bounds(ulo, uhi)
    if ylo is not None:
        eng.set_instance_output_bounds(ylo, yhi)
