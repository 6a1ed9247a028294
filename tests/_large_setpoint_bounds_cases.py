"""Cases of DDMPC_OPT_LARGE_SETPOINT_BOUNDS (per-instance setpoints on bounded handles beyond 271 rows), shared by
tests/test_large_setpoint_bounds_reference.py (CPU) and tests/test_gpu_large_setpoint_bounds.py.  A helper, not a test.

A case is a shape, a slack kind, one setpoint per instance and a box (the bounds are the handle's: one box for the batch):

  shape "272" / "296": four-tank, L = 64 / 70, N = 700, batch 6 at the data tail; CONVEX with c = 0.05 (the slack box binds)
  shape "300": the five-channel plant of test_gpu_closed_loop_plants.LARGE (m = 2, p = 3), batch 4
  shape "608": the 8 x 8-channel size of test_gpu_large_robust_law._cfg5_robust, batch 4
  setpoints "spread": u_s +- 0.5, y_s +- 0.2 drawn with rng(11) (+- 0.3 on the five-channel plant, a tenth of the four-tank spread
            at 608 rows);  "eq": the equilibria a_b (u_s, y_s), a_b in [0.5, 1.5] drawn with rng(11)

The references are computed once per case and never written to: `full` is tests/_output_bounds_ref.solve_bounded (the full-space
iteration, the reference of the bars), `reduced` is tests/_large_box_ref.solve_reduced (the set size of every iteration), both
on tests/_setpoint_law_ref.with_setpoints(spec, us[b], ys[b]).
"""
import functools

import numpy as np

from oracle import ddmpc_oracle as orc

import _large_box_ref as lref
import _large_box_safeguard_ref as sref
import _output_bounds_ref as yref
import _setpoint_law_ref as ref
import test_gpu_closed_loop_plants as plants
from test_gpu_large_robust_law import _cfg5_robust
from test_gpu_round5 import _four_tank_long

INF = np.inf
C_BOX = 0.05

U_WIDE = ([-4.0, -4.0], [6.0, 6.0])
U_TIGHT = ([0.0, 0.0], [2.0, 2.0])
U_EQ_TIGHT = ([0.0, 0.0], [2.5, 2.5])
Y_SPREAD = ([0.44, 0.56], [0.86, 0.98])
Y_EQ = ([0.2, 0.2], [1.2, 1.3])

# name -> (shape, slack, setpoints, input box, output box, capacity the case needs)
CASES = {
    "296/none/u": ("296", "none", "spread", U_WIDE, None, 64),
    "296/none/y": ("296", "none", "spread", None, Y_SPREAD, 64),
    "296/none/uy": ("296", "none", "spread", U_WIDE, Y_SPREAD, 64),
    "296/none/u-tight": ("296", "none", "spread", U_TIGHT, None, 128),
    "296/convex/u": ("296", "convex", "eq", U_WIDE, None, 64),
    "296/convex/y": ("296", "convex", "eq", None, Y_EQ, 64),
    "296/convex/u-tight": ("296", "convex", "eq", U_EQ_TIGHT, None, 128),
    "272/none/u": ("272", "none", "spread", U_WIDE, None, 64),
    "272/convex/y": ("272", "convex", "eq", None, Y_EQ, 64),
}


def spread(spec, B, du=0.5, dy=0.2, seed=11):
    rng = np.random.default_rng(seed)
    return spec.u_s + rng.uniform(-du, du, (B, spec.m)), spec.y_s + rng.uniform(-dy, dy, (B, spec.p))


def equilibria(spec, B, seed=11):
    a = np.random.default_rng(seed).uniform(0.5, 1.5, B)
    return a[:, None] * np.asarray(spec.u_s, float)[None, :], a[:, None] * np.asarray(spec.y_s, float)[None, :]


@functools.lru_cache(maxsize=None)
def shape(rows, slack):
    """dict(spec, N, B, u_d, y_d, up, yp, plant, x0) of a shape; built once and never written to."""
    if rows in ("272", "296"):
        B, N = 6, 700
        spec, d, up, yp = _four_tank_long(B, 64 if rows == "272" else 70, N, slack, C_BOX if slack == "convex" else 1.0)
        extra = dict(plant=dict(orc.FOUR_TANK), x0=d["x_end"].copy())
    elif rows == "300":
        g = plants.LARGE
        c = plants.make_case(g["m"], g["p"], g["ns"], g["n"], g["Lh"], slack, B=4, n_steps=6)
        spec, N, B, d, up, yp = c["spec"], c["N"], 4, c, c["up"], c["yp"]
        extra = dict(plant=c["plant"], x0=c["x0"])
    else:
        B = 4
        spec, N, d, up, yp = _cfg5_robust(B, slack)
        extra = {}
    assert (spec.m + spec.p) * (spec.L + spec.n) == int(rows)
    return dict(spec=spec, N=N, B=B, u_d=d["u_d"], y_d=d["y_d"], up=up, yp=yp, **extra)


def make(rows, slack, kind, ubox, ybox, cap, us=None, ys=None):
    """A case from its parts (us / ys given: those setpoints instead of the drawn ones)."""
    c = dict(shape(rows, slack))
    if us is None:
        us, ys = (equilibria if kind == "eq" else spread)(c["spec"], c["B"])
    c.update(us=us, ys=ys, ubox=ubox, ybox=ybox, cap=cap)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    return make(*CASES[name])


# The cases on other plants and the safeguard case: boxes around the plant's own setpoint, setpoints drawn with their own spread.
MAX_ITER_SAFE = 50


@functools.lru_cache(maxsize=None)
def case_300():
    """m = 2, p = 3 under CONVEX: u_s +- 0.6 around setpoints u_s +- 0.3, y_s +- 0.3; the wide kernel (the peak is 63 of 64)."""
    sh = shape("300", "convex")
    spec = sh["spec"]
    us, ys = spread(spec, sh["B"], 0.3, 0.3)
    return make("300", "convex", None, (list(spec.u_s - 0.6), list(spec.u_s + 0.6)), None, 128, us, ys)


@functools.lru_cache(maxsize=None)
def case_608():
    """An output box y_s +- 1 at setpoints u_s +- 0.05, y_s +- 0.02: on this plant (R = 1e-4) the reference iteration cycles or
    takes 10 - 30 iterations under every input box tried (u_s +- 0.3 .. 6)."""
    sh = shape("608", "none")
    spec = sh["spec"]
    us, ys = spread(spec, sh["B"], 0.05, 0.02)
    return make("608", "none", None, None, (list(spec.y_s - 1.0), list(spec.y_s + 1.0)), 64, us, ys)


@functools.lru_cache(maxsize=None)
def case_safe():
    """u in [0.9, 1.1] (the cycling family of test_gpu_large_box_safeguard.py), setpoints inside the box: u_s +- 0.05,
    y_s +- 0.01; max_iter = MAX_ITER_SAFE, capacity 192."""
    sh = shape("296", "none")
    us, ys = spread(sh["spec"], sh["B"], 0.05, 0.01)
    return make("296", "none", None, ([0.9, 0.9], [1.1, 1.1]), None, 192, us, ys)


def primal_reference(c, b):
    """tests/_large_box_safeguard_ref.solve_primal (the method of the safeguard) at the instance's setpoint."""
    spec = ref.with_setpoints(c["spec"], c["us"][b], c["ys"][b])
    return sref.solve_primal(spec, c["u_d"][b], c["y_d"][b], c["up"][b], c["yp"][b], box_of(c))


def box_of(c):
    return dict(u=c["ubox"], y=c["ybox"])


def full_reference(c, b, max_iter=100):
    ylo, yhi = c["ybox"] if c["ybox"] is not None else (-INF, INF)
    kw = dict(u_min=c["ubox"][0], u_max=c["ubox"][1]) if c["ubox"] is not None else {}
    spec = ref.with_setpoints(c["spec"], c["us"][b], c["ys"][b])
    return yref.solve_bounded(spec, c["u_d"][b], c["y_d"][b], c["up"][b], c["yp"][b], ylo, yhi, max_iter=max_iter, **kw)


def reduced_reference(c, b, max_iter=50):
    spec = ref.with_setpoints(c["spec"], c["us"][b], c["ys"][b])
    return lref.solve_reduced(spec, c["u_d"][b], c["y_d"][b], c["up"][b], c["yp"][b], box_of(c), max_iter=max_iter)


@functools.lru_cache(maxsize=None)
def full(name):
    c = case(name)
    return [full_reference(c, b) for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reduced(name):
    c = case(name)
    return [reduced_reference(c, b) for b in range(c["B"])]


def schedule_loop_bounded(c, b, w_sys, u_ref, y_ref, n_mpc_step=1):
    """tests/_setpoint_law_ref.schedule_loop under the case's bounds for instance b: the solve made at step t is solve_bounded with
    the setpoints (u_ref[t], y_ref[t]).  Returns (u_sys, y_sys, u_past_end, y_past_end, the smallest margin of its solves)."""
    spec, pl = c["spec"], c["plant"]
    n, m, p = spec.n, spec.m, spec.p
    plant = orc.Plant(pl["A"], pl["B"], pl["C"], pl["D"], pl["eps_max"])
    plant.x = c["x0"][b].copy()
    ylo, yhi = c["ybox"] if c["ybox"] is not None else (-INF, INF)
    kw = dict(u_min=c["ubox"][0], u_max=c["ubox"][1]) if c["ubox"] is not None else {}
    n_steps = w_sys.shape[0]
    up, yp = c["up"][b].copy(), c["yp"][b].copy()
    u_sys, y_sys, margin = np.zeros((n_steps, m)), np.zeros((n_steps, p)), np.inf
    for t in range(0, n_steps, n_mpc_step):
        sol = yref.solve_bounded(ref.with_setpoints(spec, u_ref[t], y_ref[t]), c["u_d"][b], c["y_d"][b], up, yp, ylo, yhi, **kw)
        assert sol.status == "optimal", (b, t, sol.status)
        margin = min(margin, sol.margin)
        for k in range(t, min(t + n_mpc_step, n_steps)):
            u = sol.optimal_u[(k - t) * m:(k - t + 1) * m]
            y = plant.step(u, w_sys[k])
            u_sys[k], y_sys[k] = u, y
            up = np.concatenate([up[m:], u])
            yp = np.concatenate([yp[p:], y])
    return u_sys, y_sys, up, yp, margin
