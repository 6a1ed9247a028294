"""Bounded ROBUST controllers under DDMPC_WEIGHT_DIAG weights that change with the step and with the channel, and with a zero
weight next to a box: every kernel that reads the per-component box table (c_s = -lam / w, d_s = lam / w with the component's
own w = r or q of its prediction step and channel), each against an independent reference.

With scalar weights every input component shares one d_s and every output component another, so a column of the active list
that carries the d_s or the shift of another component, or a table indexed by the wrong step or channel, goes unnoticed: every
bounded test before this file ran Q = 3, R = 1e-4 (the option 19 / 20 step tests excepted).  The profile here is `ramp` of
tests/test_gpu_large_weights.py; tests/test_bounded_weights_reference.py shows on the CPU that the final active set of every
case holds at least three distinct d_s, that each of the five MUTATIONS of the weight tables moves the reference by 1000 bars
and more, and that a Woodbury update with the d_s column rolled by one over the active components does too.

Cases, fixtures and references: tests/_bounded_weights_cases.py.  Bars (the project's): inputs 1e-8 of max|u_ref|, cost 1e-9
relative, on every instance of every case; loops: inputs 1e-8, outputs and end state 1e-9 of max(1, max|y_ref|); ddmpc_step after
ddmpc_prepare bit-equal to ddmpc_solve except under the warm-start options (1e-10 up to 271 rows as in test_gpu_box_warm_start.py,
the seeded reference beyond) and the box law (a law step against the solve 1e-9, test_gpu_large_box_law.py).  Where the
reference margin is >= 1e-6 (up to 271 rows) or 1e-7 (beyond): equal solve count, equal signed active set, every active input or
output on its bound bit for bit, H alpha = [ubar; ybar + sigma] to 1e-8 (`_check_against` of tests/test_gpu_large_bounds.py).  At
most one instance in eight per case may fall below (asserted on the CPU; by the reference none does on the rows used here).
Every figure is printed before it is asserted.

Which kernel reads the table in which test, and how that is asserted (the library names the loop kernel through
ddmpc_closed_loop_kernel_name and, beyond 271 rows, leaves the route record of ddmpc_debug_workspace with the peak set size; a
step kernel up to 271 rows has no name to read, so the instantiation follows from what the handle was given and from iters >= 2,
the box acting):
  test_small_solve_step_and_solution[s-u02-convex]   ddmpc_box_step_kernel<0, 0>, ddmpc_reconstruct_kernel (get_solution)
  test_small_solve_step_and_solution[s-uy-none / s-uy2-convex]   ddmpc_box_step_kernel<0, 1> (output bounds set)
  test_small_safeguard                               ddmpc_box_step_kernel<1, 0> and <1, 1>: iters > max_iter on the capped rows
  test_small_warm_start                              the seeded instantiation: iters of the second step = the seeded reference's
  test_small_fused_loop                              ddmpc_closed_loop_box_kernel (name asserted)
  test_small_instance_bounds                         the channel-table (BoxChannels) instantiations of ddmpc_box_step_kernel and of
                                                     ddmpc_closed_loop_box_kernel (label "ddmpc_closed_loop_instance_box_kernel" asserted)
  test_small_m_ne_p                                  ddmpc_box_step_kernel<0, 1> and ddmpc_closed_loop_box_kernel (name) at 45 rows
  test_small_zero_weight_next_to_a_box               the same kernels with 1e25 on the diagonal of K0 next to the box
  test_large_solve_step_and_solution                 rr3_solve_box_kernel<REFINE_PASS>, both values (route record: phases)
  test_large_capacity                                rr3_solve_box_wide_kernel (record: peak in (64, 256] = the reference's)
  test_large_safeguard                               rr3_box_safeguard_kernel (iters = max_iter + the primal reference's)
  test_large_warm_start                              the seeded wide kernel (iters = the seeded reference's, below the cold count)
  test_large_box_law                                 rr3_law_box_step_kernel (iters 1, differs from the solve in some bit) and the
                                                     filtered bounded solve (bit-equal to the option 0)
  test_large_setpoint_bounds                         the setpoint instantiation of rr3_solve_box_kernel (ddmpc_step_setpoints)
  test_large_per_step_loop                           prepare / step + ddmpc_plant_kernel (name asserted)
  test_large_m_ne_p                                  rr3_solve_box_kernel at 300 rows, five channels
  test_large_zero_weight_next_to_a_box               rr3_solve_box_kernel with D0 = 1e25 on rows next to the boxed block

Measured on an MI355X (worst relative error over every row of a group; for information -- the assertions use the bars above;
u = optimal_u, c = cost).  The file takes 12 s there (36 tests, the references included; the slowest, test_small_safeguard on
the third box, 2.4 s, of which the primal reference takes most).  No test failed on the unmodified library: no bug was found.
  up to 271 rows, three boxes        u 4.2e-11  c 7.1e-12      safeguard (iters = max_iter + the primal reference's solves on all five
                                                               capped rows: 60, 75, 112, 156, 168)  u 4.2e-11  c 3.9e-12
  warm start, second step            u 1.1e-11  c 1.6e-12      (3 .. 4 solves where the empty start takes 9 .. 13; beyond 271 rows 4 .. 5)
  fused loops                        u 6.1e-13  y 3.5e-13  x_end 1.8e-13  (on the first box the applied input sits on a bound at every
                                                               step: the loop agrees with the reference to the bit in u)
  per-instance bounds                u 2.9e-12  c 7.7e-13      loop, all 8 rows: u 3.2e-13  y 6.3e-14  x_end 1.1e-13
  45 rows, m != p (REFINE_OFF)       u 1.2e-10  c 1.0e-10      loop u 1.2e-10  y 1.8e-10
  zero weights, 136 rows             u 6.5e-13  c 6.2e-13
  296 rows, REFINE_OFF / default     u 5.4e-11 / 1.8e-14  c 3.6e-12 / 4.0e-15
  capacity 192 (REFINE_OFF)          u 1.3e-10  c 1.5e-11      peaks 128, 136, 130, 135 in the record and in the reference
  large safeguard                    u 1.4e-14  c 9.6e-16      (9 + 117 and 9 + 95 iters on rows 1 and 3)
  large warm start / box law         u 4.5e-15 / 2.6e-12  c 2.1e-15 / 6.8e-13
  per-step loop, 296 rows            u 0  y 5.6e-17  x_end 2.2e-16  (the applied input sits on a bound at every step)
  300 rows, m != p                   u 6.9e-12  c 1.9e-12
  zero weights, 296 rows             REFINE_OFF u 3.4e-12  c 1.3e-12; default u 7.3e-13  c 1.4e-13
test_large_m_ne_p runs the 300-row plant under the default refinement only: under DDMPC_REFINE_OFF the unrefined factor of that
plant does not reach the bar with or without bounds (DESIGN 5.5.2 has the figures), so an assertion there would measure the
factor, not the box table.

Sensitivity on the real code (two scratch builds of the host tables, not committed; each run once).
  `build_large_box` gives every input component the D0 of the first boxed input: 18 of the 36 tests here fail -- every test
  beyond 271 rows but test_large_capacity, test_large_zero_weight_next_to_a_box[l-qzero-y0-off] and [l-qzero-y0-auto], whose
  boxes hold no input component.  Of the 126 earlier tests of test_gpu_large_bounds, _large_box_capacity, _large_box_safeguard,
  _large_box_warm_start, _large_box_law and _large_setpoint_bounds none notices.
  `build_box_list` does the same: 14 fail -- every test up to 271 rows but test_small_zero_weight_next_to_a_box[s-qzero-y0]
  (outputs only).  Of the 161 earlier tests of test_gpu_input_bounds, _output_bounds, _instance_bounds, _box_safeguard,
  _box_warm_start, _setpoint_box_law, _setpoint_convex_law and _setpoint_box_loop two notice, the option 19 and 20 step tests with
  diagonal weights: test_gpu_setpoint_box_law::test_step_against_the_reference[tight-terminal-diag] and
  test_gpu_setpoint_convex_law::test_step_against_the_reference[wide-no-terminal-diag].
"""
import numpy as np
import pytest

from oracle import ddmpc_oracle as orc

import _bounded_weights_cases as BW
import _box_safeguard_ref as sgref
import _box_warm_ref as wref
import _instance_bounds_cases as IC
import _large_box_safeguard_ref as lsref
import _large_box_warm_ref as lwref
import _large_setpoint_bounds_cases as SC
import _output_bounds_ref as yref
import test_gpu_large_bounds as LB
import test_gpu_large_weights as LW
from test_gpu_large_box_safeguard import _record
from test_gpu_large_robust_law import _windows
from test_gpu_large_setpoint_bounds import _check_instance as _check_setpoint_instance

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST, TOL_Y = 1e-8, 1e-9, 1e-9
INF = np.inf
FUSED, FUSED_INSTANCE, PLANT = "ddmpc_closed_loop_box_kernel", "ddmpc_closed_loop_instance_box_kernel", "ddmpc_plant_kernel"


def _copy(res):
    return [np.asarray(x).copy() for x in res]


def _bit_equal(a, b, tag=""):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), tag


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _handle(spec, N, d, rows, ubox, ybox, large, **opts):
    """A DDMPC_WEIGHT_DIAG handle (asserted by LW._engine) on the instances `rows` with its data and box; `opts`: max_iter and the
    engine's option setters by name (refinement="off", large_box_capacity=128, box_safeguard=True, ...)."""
    kw = {k: opts.pop(k) for k in ("max_iter",) if k in opts}
    eng = LW._engine(spec, N, len(rows), **kw)
    if large:
        eng.set_large_bounds(True)
    for name, v in opts.items():
        getattr(eng, "set_" + name)(v)
    eng.set_data(d["u_d"][rows], d["y_d"][rows])
    if ubox is not None:
        eng.set_input_bounds(*ubox)
    if ybox is not None:
        eng.set_output_bounds(*ybox)
    return eng


def _case_handle(name, rows=None, **opts):
    c, spec, N, d = BW.case_of(name)
    rows = list(c.rows if rows is None else rows)
    return _handle(spec, N, d, rows, c.ubox, c.ybox, c.fixture.startswith("large"), **opts), c, spec, N, d, rows


def _check(sol, b, fixture, spec, d, u, cost, it, x, tag, iters=None):
    """Instance b of the fixture against its reference: the bars always; count, signed set, bounds held bit for bit and the
    Hankel identity (LB._check_against) where the margin allows.  Returns the errors."""
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s b=%d iters %d/%d k %d margin %.1e err_u %.1e err_cost %.1e" %
          (tag, b, it, sol.iters if iters is None else iters, np.count_nonzero(sol.active), sol.margin, eu, ec))
    assert sol.status == "optimal", (tag, b, sol.status)
    assert eu < TOL_U and ec < TOL_COST, (tag, b, eu, ec)
    if sol.margin >= BW.MARGIN[fixture]:
        if iters is not None:
            assert it == iters, (tag, b, it, iters)
            it = sol.iters
        LB._check_against(sol, b, spec, d["u_d"], d["y_d"], u, cost, it, x, tag)
    return eu, ec


def _held_and_hankel(sol, b, spec, d, x, tag):
    """The two assertions of LB._check_against that need no margin, for a reference that has none (the primal method's): every
    active input or output on its bound bit for bit, and H alpha = [ubar; ybar + sigma] to 1e-8."""
    na, nu, ny = BW.sections(spec, d["u_d"].shape[1])
    hard = (sol.idx >= na) & (sol.idx < na + nu + ny)
    for side, bnd in ((1, sol.hi), (-1, sol.lo)):
        on = hard & (sol.active == side)
        assert np.array_equal(x[sol.idx[on]], bnd[on]), (tag, b, side)
    H = orc.hankel_matrix(np.concatenate([d["u_d"][b], d["y_d"][b]], axis=1), spec.Ln)
    ub = x[na:na + nu].reshape(spec.Ln, spec.m)
    yb = x[na + nu:na + nu + ny].reshape(spec.Ln, spec.p)
    sg = x[na + nu + ny:].reshape(spec.Ln, spec.p)
    zz = np.concatenate([ub, yb + sg], axis=1).reshape(-1)
    assert np.max(np.abs(H @ x[:na] - zz)) <= 1e-8 * np.max(np.abs(zz)), (tag, b)


def _solve_prepare_step(eng, up, yp):
    s = _copy(eng.solve(up, yp))
    x = LB._full_x(eng)
    eng.prepare()
    t = _copy(eng.step(up, yp))
    return s, x, t, LB._full_x(eng)


def _solve_step_case(name, **opts):
    """ddmpc_solve, ddmpc_prepare + ddmpc_step (bit-equal) and ddmpc_get_solution of a case, every row against its reference."""
    eng, c, spec, N, d, rows = _case_handle(name, **opts)
    with eng:
        s, x, t, xt = _solve_prepare_step(eng, d["up"][rows], d["yp"][rows])
        route = LW._robust_route(eng) if c.fixture.startswith("large") else None
    tag = "%s %s" % (name, opts)
    _bit_equal(s, t, tag)
    assert np.array_equal(x, xt), tag
    assert np.all(s[2] == 0), (tag, s[2])
    assert route in (None, "phases")
    worst = [0.0, 0.0]
    for i, b in enumerate(rows):
        e = _check(BW.reference(name, b), b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], tag)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print("%s worst: u %.2e cost %.2e" % (tag, worst[0], worst[1]))
    assert np.all(s[3] >= 2), (tag, s[3])                  # the box acts on every row: the table is read
    return s, x


# ================================================================================================= up to 271 rows
@pytest.mark.parametrize("name", ["s-u02-convex", "s-uy-none", "s-uy2-convex"])
def test_small_solve_step_and_solution(gpu, name):
    """Item 1: ddmpc_box_step_kernel<0, YB> and ddmpc_reconstruct_kernel on the three boxes."""
    _solve_step_case(name)


@pytest.mark.parametrize("name,cap", [("s-u02-convex", 9), ("s-uy2-convex", 8)])
def test_small_safeguard(gpu, name, cap):
    """Item 2: DDMPC_OPT_BOX_SAFEGUARD with max_iter below the reference's solve count on at least two rows (the reference counts
    9, 12, 9, 10 on the first box and 7, 9, 9, 13 on the third): those rows end in the primal method, against
    _box_safeguard_ref.solve_safeguarded -- the bars, the signed set, `iters` = max_iter + the reference's solves (what
    include/ddmpc.h states for the option; that reference carries no margin, so the count is asserted on every capped row), active
    bounds bit for bit and the Hankel identity; the others below the cap, against the primal-dual reference."""
    eng, c, spec, N, d, rows = _case_handle(name, max_iter=cap, box_safeguard=True)
    with eng:
        s, x, t, xt = _solve_prepare_step(eng, d["up"][rows], d["yp"][rows])
    _bit_equal(s, t, name)
    assert np.array_equal(x, xt) and np.all(s[2] == 0), (name, s[2])
    capped = 0
    for i, b in enumerate(rows):
        pd = BW.reference(name, b)
        if pd.iters <= cap:
            _check(pd, b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], name + " below the cap")
            continue
        capped += 1
        lo, hi = yref._pairs(c.ubox[0], c.ubox[1], *(c.ybox if c.ybox is not None else (-INF, INF)))
        with yref._union_box():
            sol = sgref.solve_safeguarded(spec, d["u_d"][b], d["y_d"][b], d["up"][b], d["yp"][b], lo, hi)
        eu, ec = _rel(s[0][i], sol.optimal_u), abs(s[1][i] - sol.cost) / abs(sol.cost)
        print("%s b=%d safeguard: iters %d (cap %d, primal reference %d solves, kmax %d) err_u %.1e err_cost %.1e" %
              (name, b, s[3][i], cap, sol.iters, sol.kmax, eu, ec))
        assert sol.status == "optimal" and s[3][i] == cap + sol.iters, (name, b, s[3][i], cap, sol.iters)
        assert eu < TOL_U and ec < TOL_COST, (name, b, eu, ec)
        assert np.array_equal(LB._signed_active(x[i], sol), sol.active), (name, b)
        _held_and_hankel(sol, b, spec, d, x[i], name + " safeguard")
    assert capped >= 2, capped


def test_small_warm_start(gpu):
    """Item 3: DDMPC_OPT_BOX_WARM_START on the first box.  The step at the data tail has no seed (the unseeded reference, count
    and set); the step one plant step later starts from its set: against _box_warm_ref.solve_seeded seeded with the first
    reference's set -- the bars and, where the margin allows, the seeded count, the signed set, active bounds bit for bit and the
    Hankel identity, as for every other solve of this file."""
    name = "s-u02-convex"
    eng, c, spec, N, d, rows = _case_handle(name, box_warm_start=True)
    P = d["plant"]
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (8, 2))
    firsts = [BW.reference(name, b) for b in rows]
    up2, yp2 = [], []
    for i, b in enumerate(rows):                           # the second window from the REFERENCE's first input: no GPU rounding
        u0 = firsts[i].optimal_u[:spec.m]
        y0 = P["C"] @ d["x_end"][b] + P["D"] @ u0 + w[b]
        up2.append(np.concatenate([d["up"][b][spec.m:], u0]))
        yp2.append(np.concatenate([d["yp"][b][spec.p:], y0]))
    up2, yp2 = np.stack(up2), np.stack(yp2)
    with eng:
        eng.prepare()
        s1 = _copy(eng.step(d["up"][rows], d["yp"][rows]))
        x1 = LB._full_x(eng)
        s2 = _copy(eng.step(up2, yp2))
        x2 = LB._full_x(eng)
        cold = _copy(eng.solve(up2, yp2))                  # the cold contract: from the empty set
    assert np.all(s1[2] == 0) and np.all(s2[2] == 0) and np.all(cold[2] == 0)
    fewer = 0
    for i, b in enumerate(rows):
        _check(firsts[i], b, c.fixture, spec, d, s1[0][i], s1[1][i], s1[3][i], x1[i], "warm start, first step")
        sol = wref.solve_seeded(spec, d["u_d"][b], d["y_d"][b], up2[i], yp2[i], c.ubox[0], c.ubox[1], seed=firsts[i].active)
        assert sol.seeded and not sol.fell_back
        eu, ec = _rel(s2[0][i], sol.optimal_u), abs(s2[1][i] - sol.cost) / abs(sol.cost)
        print("warm start, second step b=%d iters %d/%d (cold %d) k %d margin %.1e err_u %.1e err_cost %.1e" %
              (b, s2[3][i], sol.iters, cold[3][i], np.count_nonzero(sol.active), sol.margin, eu, ec))
        _check(sol.sol, b, c.fixture, spec, d, s2[0][i], s2[1][i], s2[3][i], x2[i], "warm start, second step")
        fewer += int(s2[3][i] < cold[3][i])
    assert _rel(s2[0], cold[0]) < 1e-10 and np.max(np.abs(s2[1] - cold[1]) / np.abs(cold[1])) < 1e-10
    assert fewer >= 1                                      # the seed was used: fewer solves than from the empty set


def _loop_refs(spec, d, rows, w, ubox, ybox, nms):
    """(u_sys, y_sys, x_end) of closed_loop_bounded per row (it raises unless every solve is optimal)."""
    return [BW.loop_ref(spec, d, b, w[i], ubox, ybox, nms) for i, b in enumerate(rows)]


def _check_loop(out, refs, tag):
    u_sys, y_sys, st, x_end = out[0], out[1], out[2], out[3]
    assert np.all(np.asarray(st) == 0), (tag, st)
    for i, (ur, yr, xr) in enumerate(refs):
        ysc = max(1.0, np.max(np.abs(yr)))
        eu, ey, ex = _rel(u_sys[i], ur), np.max(np.abs(y_sys[i] - yr)) / ysc, np.max(np.abs(x_end[i] - xr)) / ysc
        print("%s row %d: u %.2e y %.2e x_end %.2e" % (tag, i, eu, ey, ex))
        assert eu < TOL_U and ey < TOL_Y and ex < TOL_Y, (tag, i, eu, ey, ex)


def _run_loop(eng, d, rows, w, nms):
    P = d["plant"]
    return eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][rows], d["up"][rows], d["yp"][rows], w, n_mpc_step=nms)


@pytest.mark.parametrize("nms", [1, 2])
@pytest.mark.parametrize("name", ["s-u02-convex", "s-uy-none"])
def test_small_fused_loop(gpu, name, nms):
    """Item 4: ddmpc_closed_loop_box_kernel, 6 steps, against closed_loop_bounded (every solve of it optimal, or it raises)."""
    eng, c, spec, N, d, rows = _case_handle(name, rows=(0, 1))
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (len(rows), 6, spec.p))
    with eng:
        out = _run_loop(eng, d, rows, w, nms)
        assert eng.closed_loop_kernel_name() == FUSED
    _check_loop(out, _loop_refs(spec, d, rows, w, c.ubox, c.ybox, nms), "%s fused loop nms %d" % (name, nms))


def test_small_instance_bounds(gpu):
    """Item 5: box C of tests/_instance_bounds_cases.py (its first 8 rows: the fixture's seeds) through the per-instance calls,
    slack NONE: solve, prepare + step (bit-equal) and a 6-step fused loop, all eight instances -- rows 3 and 7 without a bound
    on input channel 0 and row 5 without one on output channel 1 among them -- against the reference with their own row, the loop's
    status, inputs, outputs and end state included."""
    spec0, N, d = BW.fixture("small", "none", False)
    spec = LW.with_weights(spec0, *LW.ramp(spec0))
    rows = list(range(8))
    ulo, uhi, ylo, yhi = (a[:8] for a in IC.box("C"))
    w = BW.instance_loop_noise()
    with LW._engine(spec, N, 8) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_instance_input_bounds(ulo, uhi)
        eng.set_instance_output_bounds(ylo, yhi)
        s, x, t, xt = _solve_prepare_step(eng, d["up"], d["yp"])
        out = _run_loop(eng, d, rows, w, 1)
        assert eng.closed_loop_kernel_name() == FUSED_INSTANCE
    _bit_equal(s, t)
    assert np.array_equal(x, xt) and np.all(s[2] == 0)
    left_out = 0
    for b in rows:
        sol = BW.instance_reference(b)
        left_out += sol.margin < BW.MARGIN["small"]
        _check(sol, b, "small", spec, d, s[0][b], s[1][b], s[3][b], x[b], "instance bounds")
    assert left_out <= 1, left_out
    assert np.all(s[3] >= 2)
    _check_loop(out, [BW.instance_loop_reference(b) for b in rows], "instance bounds fused loop")


def test_small_m_ne_p(gpu):
    """Item 6: m = 2, p = 3, D != 0, 45 rows, CONVEX: input channel 1 and output channel 1 bounded; solve, step and a 6-step
    fused loop.  DDMPC_REFINE_OFF, as the fused convex legs of test_gpu_closed_loop_plants.run_loop: under the default AUTO
    ddmpc_prepare takes the law of row 0 of this plant from a refining solve, and such a law reports optimal_inaccurate with an
    active set (test_laws_from_refining_solves_report_inaccurate_with_an_active_set) and sends the loop to the per-step path.
    The bars stay the same."""
    name = "s-mp-convex"
    c, spec, N, d = BW.case_of(name)
    assert spec.m != spec.p and np.any(d["plant"]["D"] != 0.0) and (spec.m + spec.p) * spec.Ln == 45
    _solve_step_case(name, refinement="off")
    rows = [0, 1]
    with _case_handle(name, rows=rows, refinement="off")[0] as eng:
        out = _run_loop(eng, d, rows, d["w"][rows], 1)
        assert eng.closed_loop_kernel_name() == FUSED
    _check_loop(out, _loop_refs(spec, d, rows, d["w"][rows], c.ubox, c.ybox, 1), "small m != p fused loop")


@pytest.mark.parametrize("name", ["s-rzero-u0", "s-qzero-y0", "s-qzero-y0-u0"])
def test_small_zero_weight_next_to_a_box(gpu, name):
    """Item 7: a zero weight on an unbounded channel with finite bounds on another (accepted since the bounds exist, never solved
    before): the 1e25 diagonal entry of the unweighted component sits inside K0 next to the box.  The reference uses the exact 0."""
    c, spec, N, d = BW.case_of(name)
    assert np.count_nonzero(np.diag(spec.Q) == 0.0) + np.count_nonzero(np.diag(spec.R) == 0.0) == 10
    _solve_step_case(name)


# ================================================================================================= beyond 271 rows
@pytest.mark.parametrize("refine", ["off", "auto"])
@pytest.mark.parametrize("name", ["l-ucap-convex", "l-uy-none", "l-uch0-none"])
def test_large_solve_step_and_solution(gpu, name, refine):
    """Item 8: rr3_solve_box_kernel<REFINE_PASS>.  DDMPC_REFINE_OFF matters: the refinement pass forms its residual with the
    true D(state), so it can pull a wrong Woodbury solve back towards the right answer."""
    _solve_step_case(name, refinement=refine)


def test_large_capacity(gpu):
    """Item 9: DDMPC_OPT_LARGE_BOX_CAPACITY = 192 on case D of test_gpu_large_box_capacity.py (the output box under CONVEX) with
    the ramp: the reduced reference peaks at 128, 136, 130 and 135 active components on rows 0 .. 3 (128 .. 139 over all eight
    seeds; 131 .. 139 with scalar weights), so the 64-column kernel cannot serve them.  The record's peak equals the reference's."""
    name = "l-ytight-convex"
    eng, c, spec, N, d, rows = _case_handle(name, large_box_capacity=192, refinement="off")
    with eng:
        s, x, t, xt = _solve_prepare_step(eng, d["up"][rows], d["yp"][rows])
        rec = [_record(eng, i, 192) for i in range(len(rows))]
    _bit_equal(s, t)
    assert np.array_equal(x, xt) and np.all(s[2] == 0), s[2]
    for i, b in enumerate(rows):
        red = BW.reference(name, b)
        print("capacity b=%d peak: record %d reference %d" % (b, rec[i][2], red.peak))
        assert 64 < red.peak <= 256 and rec[i][2] == red.peak
        _check(red, b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], "capacity 192")


def test_large_safeguard(gpu):
    """Item 10: DDMPC_OPT_LARGE_BOX_SAFEGUARD on U_CAP under CONVEX, max_iter = 9 (the primal-dual reference takes 8, 11, 8, 12):
    rows 1 and 3 go through rr3_box_safeguard_kernel, against _large_box_safeguard_ref.solve_primal, iters = max_iter + its
    solves; capacity 128 (the primal method's working sets reach 59 .. 103 with scalar weights)."""
    name, cap = "l-ucap-convex", 9
    eng, c, spec, N, d, rows = _case_handle(name, max_iter=cap, large_box_capacity=128, large_box_safeguard=True)
    with eng:
        s, x, t, xt = _solve_prepare_step(eng, d["up"][rows], d["yp"][rows])
    _bit_equal(s, t)
    assert np.array_equal(x, xt) and np.all(s[2] == 0), s[2]
    capped = 0
    for i, b in enumerate(rows):
        pd = BW.reference(name, b)
        if pd.iters <= cap:
            _check(pd, b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], "safeguard, below the cap")
            continue
        capped += 1
        sol = lsref.solve_primal(spec, d["u_d"][b], d["y_d"][b], d["up"][b], d["yp"][b], dict(u=c.ubox, y=c.ybox))
        print("safeguard b=%d: primal reference %d solves, largest set %d" % (b, sol.iters, sol.peak))
        _check(sol, b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], "safeguard, primal", iters=cap + sol.iters)
    assert capped >= 2, capped


def test_large_warm_start(gpu):
    """Item 11: DDMPC_OPT_LARGE_BOX_WARM_START on U_WIDE + Y_UP, two consecutive windows of the reference's own loop (so no GPU
    rounding enters them): the first step has no seed, the second starts from the first's set -- against
    _large_box_warm_ref (Reduced.solve seeded), counts included."""
    name = "l-uy-none"
    eng, c, spec, N, d, rows = _case_handle(name, large_box_warm_start=True)
    P = d["plant"]
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (8, 2, 2))
    loops = []
    for b in rows:
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        loops.append(lwref.closed_loop_seeded(spec, d["u_d"][b], d["y_d"][b], plant, w[b], dict(u=c.ubox, y=c.ybox),
                                              u_past=d["up"][b], y_past=d["yp"][b], max_iter=100)[2])
    with eng:
        eng.prepare()
        fewer = 0
        for k in range(2):
            up = np.stack([lp[k].window[0] for lp in loops])
            yp = np.stack([lp[k].window[1] for lp in loops])
            s = _copy(eng.step(up, yp))
            x = LB._full_x(eng)
            assert np.all(s[2] == 0), s[2]
            for i, b in enumerate(rows):
                sol = loops[i][k]
                assert sol.seeded == (k == 1) and not sol.fell_back
                _check(sol, b, c.fixture, spec, d, s[0][i], s[1][i], s[3][i], x[i], "large warm start window %d" % k)
            if k == 1:
                cold = _copy(eng.solve(up, yp))
                fewer = int(np.sum(s[3] < cold[3]))
    assert fewer >= 1


def test_large_box_law(gpu):
    """Item 12: DDMPC_OPT_LARGE_BOX_LAW on U_WIDE + Y_UP.  Near the setpoint every row stays inside the box (the reference ends
    after one solve) and the law serves the step: iters 1, within 1e-9 of the solve and different from it in some bit; on the
    data tail the filtered bounded solve serves it, bit-equal to the handle without the option."""
    name = "l-uy-none"
    c, spec, N, d = BW.case_of(name)
    rows = list(c.rows)
    sup, syp = _windows(None, d["up"][rows], d["yp"][rows], spec, "setpoint")
    res = {}
    for law in (False, True):
        with _case_handle(name, large_box_law=law)[0] as eng:
            eng.prepare()
            res[law] = (_copy(eng.step(sup, syp)), _copy(eng.solve(sup, syp)), _copy(eng.step(d["up"][rows], d["yp"][rows])),
                        LB._full_x(eng))
    t, s, tail, xtail = res[True]
    assert np.all(t[2] == 0) and np.all(t[3] == 1), (t[2], t[3])
    _bit_equal(tail, res[False][2])
    assert np.array_equal(xtail, res[False][3])
    assert np.all(np.any(t[0] != s[0], axis=1))            # the law served the step, not the solve
    assert _rel(t[0], s[0]) <= 1e-9 and np.max(np.abs(t[1] - s[1]) / np.abs(s[1])) <= 1e-9
    for i, b in enumerate(rows):
        sol = BW.solve_reduced(spec, d, b, c.ubox, c.ybox, up=sup[i], yp=syp[i])
        eu, ec = _rel(t[0][i], sol.optimal_u), abs(t[1][i] - sol.cost) / abs(sol.cost)
        print("box law b=%d reference iters %d margin %.1e err_u %.1e err_cost %.1e" % (b, sol.iters, sol.margin, eu, ec))
        assert sol.status == "optimal" and sol.iters == 1 and sol.margin >= 1e-7
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        _check(BW.reference(name, b), b, c.fixture, spec, d, tail[0][i], tail[1][i], tail[3][i], xtail[i], "box law, tail")
    assert np.all(tail[3] >= 2)


def test_large_setpoint_bounds(gpu):
    """Item 13: DDMPC_OPT_LARGE_SETPOINT_BOUNDS, ddmpc_step_setpoints with the per-instance setpoints of case "296/none/uy" of
    tests/_large_setpoint_bounds_cases.py, against _setpoint_box_ref.solve (through that module's full_reference)."""
    c = dict(SC.case("296/none/uy"))
    c["spec"] = LW.with_weights(c["spec"], *LW.ramp(c["spec"]))
    with LW._engine(c["spec"], c["N"], c["B"]) as eng:
        eng.set_large_bounds(True)
        eng.set_large_setpoint_bounds(True)
        eng.set_data(c["u_d"], c["y_d"])
        eng.set_input_bounds(*c["ubox"])
        eng.set_output_bounds(*c["ybox"])
        eng.prepare()
        out = _copy(eng.step_setpoints(c["up"], c["yp"], c["us"], c["ys"]))
    for b in range(c["B"]):
        _check_setpoint_instance(c, b, SC.full_reference(c, b), out, "setpoint bounds, ramp")
    assert np.any(out[3] >= 2)


def test_large_per_step_loop(gpu):
    """Item 14: the per-step closed loop (prepare / step + ddmpc_plant_kernel), 4 steps on U_WIDE + Y_UP."""
    eng, c, spec, N, d, rows = _case_handle("l-uy-none", rows=(0, 1))
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (len(rows), 4, 2))
    with eng:
        out = _run_loop(eng, d, rows, w, 1)
        assert eng.closed_loop_kernel_name() == PLANT
        assert LW._robust_route(eng) == "phases"
    _check_loop(out, _loop_refs(spec, d, rows, w, c.ubox, c.ybox, 1), "large per-step loop")


def test_large_m_ne_p(gpu):
    """Item 15: test_gpu_closed_loop_plants.LARGE, (m, p, n, L) = (2, 3, 2, 58), 300 rows, CONVEX: input channel 1 and output
    channel 1 bounded, under the default refinement."""
    c, spec, N, d = BW.case_of("l-mp-convex")
    assert (spec.m + spec.p) * spec.Ln == 300 and spec.m != spec.p
    _solve_step_case("l-mp-convex")


@pytest.mark.parametrize("refine", ["off", "auto"])
@pytest.mark.parametrize("name", ["l-rzero-u0", "l-rzero-u0-convex", "l-qzero-y0", "l-qzero-y0-u0"])
def test_large_zero_weight_next_to_a_box(gpu, name, refine):
    """Item 16: the zero-weight cases at 296 rows; the r-zero case also under CONVEX."""
    _solve_step_case(name, refinement=refine)
