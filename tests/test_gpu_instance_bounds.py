"""Per-instance input and output bounds (ddmpc_set_instance_input_bounds / ddmpc_set_instance_output_bounds) on Route::BoxLaw:
the channel-table (BoxChannels) instantiations of the two box kernels, which stage every instance's own bounds in LDS
(csrc/ddmpc_box_law.hpp).  "ddmpc_closed_loop_instance_box_kernel" below is the label ddmpc_closed_loop_kernel_name gives that path.

The eight instantiations and the tests that reach them (step = ddmpc_box_step_kernel<SAFE, YB, BoxChannels>, loop =
ddmpc_closed_loop_box_kernel<SAFE, YB, BoxChannels>; SAFE: DDMPC_OPT_BOX_SAFEGUARD, YB: output bounds on the handle):
  step <0, 0>  test_solve_and_step_against_every_instances_own_reference[A], test_one_hard_row_leaves_its_neighbours_bit_equal,
               test_uniform_rows_are_bit_equal_to_the_shared_call[u02]
  step <1, 0>  test_one_hard_row_leaves_its_neighbours_bit_equal (the safeguard finishes row 7), test_uniform_rows...[u02]
  step <0, 1>  test_solve_and_step_against_every_instances_own_reference[B, C], test_channel_indexing_on_a_plant_with_m_ne_p,
               test_one_kind_per_instance_and_the_other_shared, test_uniform_rows...[u+y]
  step <1, 1>  test_uniform_rows_are_bit_equal_to_the_shared_call[u+y]
  loop <0, 0>  test_fused_loop_against_the_cold_path_and_the_reference, test_uniform_rows...[u02]
  loop <1, 0>  test_uniform_rows_are_bit_equal_to_the_shared_call[u02]
  loop <0, 1>  test_no_read_of_the_trajectories_after_prepare, test_the_warm_start_option_is_accepted_and_not_honoured,
               test_uniform_rows...[u+y]
  loop <1, 1>  test_uniform_rows_are_bit_equal_to_the_shared_call[u+y]
(test_uniform_rows... runs solve, step and the fused loop with the safeguard off and on, bit for bit against the shared-bounds
instantiations, which tests/test_gpu_box_safeguard.py and tests/test_gpu_output_bounds.py hold against their references.)

Fixture and boxes: tests/_instance_bounds_cases.py (four-tank, L = 30, n = 4, N = 400, 32 instances, seeds 500 .. 531, data-tail
windows; boxes A, B, C; modes `none` and `convex-tec`).  Every instance is compared with the full-space reference of
tests/_output_bounds_ref.py solved with ITS OWN bounds, at the project's bars for bounded solves: err_u < 1e-8, err_cost < 1e-9,
relative.  Instances whose reference run has margin >= 1e-6 are also compared in iteration count, signed active set and "held at
its own bound exactly"; tests/test_instance_bounds_reference.py asserts that at most 4 of 32 per configuration fall below.
The reference counts 0 solves when its box is empty (an instance of B without any bound, slack NONE); the kernels count the law
as the first, so `iters` is compared with max(reference, 1).
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from oracle import ddmpc_oracle as orc

import _box_safeguard_ref as sref
import _input_bounds_ref as uref
import _instance_bounds_cases as IC
import _output_bounds_ref as yref
import test_gpu_closed_loop_plants as CP
import test_gpu_output_bounds as OB
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9
INF = np.inf
B32 = IC.B32
FUSED = "ddmpc_closed_loop_instance_box_kernel"
SHARED_FUSED = "ddmpc_closed_loop_box_kernel"
NA, NU = OB.NA, OB.NU
MARGIN = 1e-6


def _rows(v, B=B32, nc=2):
    """One row for every instance."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=float), (B, nc)))


def _outputs(call):
    return [np.asarray(x).copy() for x in call]


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_against(sol, b, spec, d, u, cost, it, x, tag):
    """Instance b of a solve against its own reference (`_check_against` of the output-bounds test, with the margin class): the
    bars for every instance; iteration count, signed active set, bounds held exactly and H alpha = [ubar; ybar + sigma] where
    margin >= 1e-6.  Every figure is printed first."""
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s b=%d iters %d/%d k %d margin %.1e err_u %.1e err_cost %.1e" %
          (tag, b, it, sol.iters, np.count_nonzero(sol.active), sol.margin, eu, ec))
    assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
    if sol.margin < MARGIN:
        return False
    assert it == max(sol.iters, 1), (b, it, sol.iters)
    assert np.array_equal(OB._signed_active(x, sol), sol.active), b
    # an active input or output equals the bound of ITS instance exactly
    usec = (sol.idx >= NA) & (sol.idx < NA + NU)
    ysec = (sol.idx >= NA + NU) & (sol.idx < NA + 2 * NU)
    for side, bnd in ((1, sol.hi), (-1, sol.lo)):
        on = (usec | ysec) & (sol.active == side)
        assert np.array_equal(x[sol.idx[on]], bnd[on]), (b, side)
    H = orc.hankel_matrix(np.concatenate([d["u_d"][b], d["y_d"][b]], axis=1), spec.Ln)
    z = H @ x[:NA]
    ub, yb, sg = (x[NA + i * NU:NA + (i + 1) * NU].reshape(34, 2) for i in range(3))
    zz = np.concatenate([ub, yb + sg], axis=1).reshape(-1)
    assert np.max(np.abs(z - zz)) <= 1e-8 * np.max(np.abs(zz)), b
    return True


# ------------------------------------------------------------------------------------------------ 1. contract
def test_invalid_arguments_name_instance_and_channel(gpu):
    spec = IC.spec_of("convex-tec")                                 # u_s = (1, 1), y_s = (0.65, 0.77), terminal constraint
    Bq = 8
    with T._engine(spec, 400, Bq) as eng:
        for call, nm in ((eng.set_instance_input_bounds, "u"), (eng.set_instance_output_bounds, "y")):
            ok_lo, ok_hi = (_rows([0.0, 0.0], Bq), _rows([2.0, 2.0], Bq))
            lo = ok_lo.copy(); lo[5, 1] = np.nan
            code, msg = OB._code(call, lo, ok_hi)
            assert code == L.ERR_INVALID and nm + "_min" in msg and "instance 5" in msg and "channel 1" in msg, msg
            hi = ok_hi.copy(); hi[3, 0] = np.nan
            code, msg = OB._code(call, ok_lo, hi)
            assert code == L.ERR_INVALID and nm + "_max" in msg and "instance 3" in msg and "channel 0" in msg, msg
            for v in (2.0, 3.0):                                     # a point, an empty box
                lo = ok_lo.copy(); lo[6, 1] = v
                code, msg = OB._code(call, lo, ok_hi)
                assert code == L.ERR_INVALID and "instance 6" in msg and "channel 1" in msg and ">=" in msg, msg
            code, msg = OB._code(call, None, ok_hi)
            assert code == L.ERR_INVALID and nm + "_min" in msg and "null" in msg, msg
            code, msg = OB._code(call, ok_lo, None)
            assert code == L.ERR_INVALID and nm + "_max" in msg and "null" in msg, msg
            # the terminal constraint fixes the last n steps to the setpoint: outside ONE instance's interval
            lo = ok_lo.copy(); lo[2, 0] = 1.5
            code, msg = OB._code(call, lo, ok_hi)
            assert code == L.ERR_INVALID and nm + "_s" in msg and "instance 2" in msg and "channel 0" in msg, msg
            with pytest.raises(ValueError):
                call(ok_lo[:4], ok_hi[:4])                           # not [batch, channels]
        # ddmpc_set_setpoints checks its argument against every row
        lo, hi = _rows([0.0, 0.0], Bq).copy(), _rows([2.0, 2.0], Bq).copy()
        hi[4, 1] = 1.2
        eng.set_instance_input_bounds(lo, hi)
        eng.set_setpoints(np.array([1.1, 1.1]), np.array([0.65, 0.77]))
        code, msg = OB._code(eng.set_setpoints, np.array([1.1, 1.3]), np.array([0.65, 0.77]))
        assert code == L.ERR_INVALID and "instance 4" in msg and "channel 1" in msg and "u_s" in msg, msg
        ylo, yhi = _rows([0.5, 0.5], Bq).copy(), _rows([0.9, 0.9], Bq).copy()
        ylo[7, 0] = 0.7
        eng.set_setpoints(np.array([1.0, 1.0]), np.array([0.75, 0.77]))
        eng.set_instance_output_bounds(ylo, yhi)
        code, msg = OB._code(eng.set_setpoints, np.array([1.0, 1.0]), np.array([0.65, 0.77]))
        assert code == L.ERR_INVALID and "instance 7" in msg and "channel 0" in msg and "y_s" in msg, msg


def test_refusals_name_the_reason(gpu):
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    d, up, yp = IC.data()
    lo, hi = _rows([0.0, 0.0], 2), _rows([2.0, 2.0], 2)
    ylo, yhi = _rows(OB.BOXES["two-sided"][0], 2), _rows(OB.BOXES["two-sided"][1], 2)
    calls = (("set_instance_input_bounds", lo, hi), ("set_instance_output_bounds", ylo, yhi))
    with T._engine(spec, 400, 2) as eng:
        eng.set_instance_input_bounds(lo, hi)
        code, msg = OB._code(eng.set_refinement, "always")
        assert code == L.ERR_UNSUPPORTED and "REFINE_ALWAYS" in msg
        code, msg = OB._code(eng.solve_from_host, d["u_d"][:2], d["y_d"][:2], up[:2], yp[:2])
        assert code == L.ERR_UNSUPPORTED and "ddmpc_solve_from_host" in msg
        code, msg = OB._code(eng.set_setpoint_convex_law, True)      # option 20 on a handle that carries per-instance bounds
        assert code == L.ERR_UNSUPPORTED and "per-instance" in msg
        eng.set_instance_input_bounds(None, None)
        eng.set_setpoint_convex_law(True)                            # ... and in the reverse order
        for name, a, b in calls:
            code, msg = OB._code(getattr(eng, name), a, b)
            assert code == L.ERR_UNSUPPORTED and "DDMPC_OPT_SETPOINT_CONVEX_LAW" in msg, msg
    with T._engine(orc.spec_from_params(), 400, 2) as eng:           # slack NONE: option 19
        eng.set_instance_output_bounds(ylo, yhi)
        code, msg = OB._code(eng.set_setpoint_box_law, True)
        assert code == L.ERR_UNSUPPORTED and "per-instance" in msg
        eng.set_instance_output_bounds(None, None)
        eng.set_setpoint_box_law(True)
        for name, a, b in calls:
            code, msg = OB._code(getattr(eng, name), a, b)
            assert code == L.ERR_UNSUPPORTED and "DDMPC_OPT_SETPOINT_BOX_LAW" in msg, msg
    with T._engine(spec, 400, 2) as eng:
        eng.set_refinement("always")
        for name, a, b in calls:
            code, msg = OB._code(getattr(eng, name), a, b)
            assert code == L.ERR_UNSUPPORTED and "REFINE_ALWAYS" in msg
    with T._engine(orc.spec_from_params(controller_type=0), 400, 2) as eng:
        for name, a, b in calls:
            code, msg = OB._code(getattr(eng, name), a, b)
            assert code == L.ERR_UNSUPPORTED and "ROBUST" in msg
            getattr(eng, name)(_rows([-INF, -INF], 2), _rows([INF, INF], 2))      # all infinite: a removal, accepted anywhere
    with T._engine(orc.spec_from_params(slack_var_constraint_type=1, L=64), 600, 2) as eng:      # (2 + 2)(64 + 4) = 272 rows
        for large_bounds in (False, True):
            eng.set_large_bounds(large_bounds)
            for name, a, b in calls:
                code, msg = OB._code(getattr(eng, name), a, b)
                assert code == L.ERR_UNSUPPORTED and "271" in msg and "272" in msg, msg
    dspec = orc.spec_from_params()
    Rd = dspec.R.copy()
    Rd[0, 1] = Rd[1, 0] = 1e-5
    dspec.R = Rd
    with T._engine(dspec, 400, 2) as eng:
        for name, a, b in calls:
            code, msg = OB._code(getattr(eng, name), a, b)
            assert code == L.ERR_UNSUPPORTED and "DENSE" in msg
    kw = dict(n=4, m=2, p=2, L_=30, N=400, u_s=[1.0, 1.0], y_s=[0.65, 0.77], batch=2, eps_max=0.002, lamb_alpha=50.0,
              lamb_sigma=1000.0, c=1.0, slack_type=L.SLACK_NONE)
    q = np.full(60, 3.0)
    q[2 * 7 + 1] = 0.0                                               # output channel 1, free step 7
    with BatchedDDMPC(Q=q, R=1e-4, **kw) as eng:
        code, msg = OB._code(eng.set_instance_output_bounds, ylo, yhi)
        assert code == L.ERR_UNSUPPORTED and "Q entry" in msg and "channel 1" in msg
        one = ylo.copy(), yhi.copy()
        one[0][:, 1], one[1][:, 1] = -INF, INF
        eng.set_instance_output_bounds(*one)                         # the unweighted channel is bounded in no instance: fine
        one[1][1, 1] = 0.9                                           # ... in ONE instance: the channel is boxed
        code, msg = OB._code(eng.set_instance_output_bounds, *one)
        assert code == L.ERR_UNSUPPORTED and "Q entry" in msg and "channel 1" in msg
    r = np.full(60, 1e-4)
    r[2 * 3 + 0] = 0.0                                               # input channel 0, free step 3
    with BatchedDDMPC(Q=np.full(60, 3.0), R=r, **kw) as eng:
        code, msg = OB._code(eng.set_instance_input_bounds, lo, hi)
        assert code == L.ERR_UNSUPPORTED and "R entry" in msg and "channel 0" in msg
    # (n (m + p) > 256 cannot be reached here: ddmpc_create asks for L >= 2 n, so such a handle has more than 3 * 256 rows and is
    #  refused for its size, the 272-row case above)
    # a box list beyond the 288 components the kernels hold (the case of the output-bounds test): 180 slack + 180 outputs
    with BatchedDDMPC(n=4, m=1, p=3, L_=60, N=400, Q=3.0, R=1e-4, u_s=[1.0], y_s=[0.5, 0.5, 0.5], batch=2, eps_max=0.002,
                      lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0, slack_type=L.SLACK_CONVEX, use_terminal_constraint=False) as eng:
        ylo3, yhi3 = np.full((2, 3), -INF), np.full((2, 3), INF)
        ylo3[0, 0], yhi3[1, 1], yhi3[0, 2] = 0.0, 1.0, 1.0           # every channel bounded in SOME instance: the union counts
        code, msg = OB._code(eng.set_instance_output_bounds, ylo3, yhi3)
        assert code == L.ERR_UNSUPPORTED and "360" in msg and "288" in msg, msg
        yhi3[1, 1], yhi3[0, 2] = INF, INF
        eng.set_instance_output_bounds(ylo3, yhi3)                   # 180 + 60 components: fine


def test_get_solution_not_ready_after_the_call(gpu):
    spec = orc.spec_from_params()
    d, up, yp = IC.data()
    with T._engine(spec, 400, 2) as eng:
        eng.set_data(d["u_d"][:2], d["y_d"][:2])
        for name, a, b in (("set_instance_input_bounds", [0.0, 0.0], [2.0, 2.0]), ("set_instance_output_bounds",) + OB.BOXES["two-sided"]):
            eng.solve(up[:2], yp[:2])
            eng.get_solution("ybar")
            getattr(eng, name)(_rows(a, 2), _rows(b, 2))
            code, _ = OB._code(eng.get_solution, "ybar")
            assert code == L.ERR_NOT_READY
            eng.step(up[:2], yp[:2])
            eng.get_solution("ybar")
            getattr(eng, name)(None, None)
            code, _ = OB._code(eng.get_solution, "ybar")
            assert code == L.ERR_NOT_READY


def test_infinite_rows_are_bit_equal_none_restores_and_the_last_call_wins(gpu):
    spec = IC.spec_of("convex-tec")
    Bq = 8
    d, up, yp = IC.data()
    u_d, y_d, up, yp = d["u_d"][:Bq], d["y_d"][:Bq], up[:Bq], yp[:Bq]
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(5).uniform(-1.0, 1.0, (Bq, 10, 2))
    ulo, uhi, _, _ = IC.box("A")
    a_rows = (ulo[:Bq], uhi[:Bq])
    none = (_rows([-INF, -INF], Bq), _rows([INF, INF], Bq))

    def run(prep):
        with T._engine(spec, 400, Bq) as eng:
            eng.set_data(u_d, y_d)
            prep(eng)
            out = _outputs(eng.solve(up, yp)) + _outputs(eng.step(up, yp))
            out += _outputs(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up, yp, w))
            return out, eng.closed_loop_kernel_name()

    def infinite(eng):
        eng.set_instance_input_bounds(*none)
        eng.set_instance_output_bounds(*none)

    def bounded_then_removed(eng):
        eng.set_instance_input_bounds(*a_rows)
        _, _, st, it = eng.step(up, yp)
        assert np.all(st == 0) and np.all(it >= 2)
        eng.set_instance_input_bounds(None, None)

    def bounded_then_infinite(eng):
        eng.set_instance_input_bounds(*a_rows)
        eng.set_instance_input_bounds(*none)

    fresh, k0 = run(lambda eng: None)
    for prep in (infinite, bounded_then_removed, bounded_then_infinite):
        got, k1 = run(prep)
        assert k1 == k0 and k1 not in (FUSED, SHARED_FUSED)
        for a, b in zip(fresh, got):
            assert _same(a, b)
    # the last call wins between the shared and the per-instance call of one kind
    shared, ks = run(lambda eng: eng.set_input_bounds([0.0, 0.0], [2.0, 2.0]))
    inst, ki = run(lambda eng: eng.set_instance_input_bounds(*a_rows))
    assert ks == SHARED_FUSED and ki == FUSED and not _same(shared[0], inst[0])
    got, k1 = run(lambda eng: (eng.set_instance_input_bounds(*a_rows), eng.set_input_bounds([0.0, 0.0], [2.0, 2.0])))
    assert k1 == SHARED_FUSED and all(_same(a, b) for a, b in zip(shared, got))
    got, k1 = run(lambda eng: (eng.set_input_bounds([0.0, 0.0], [2.0, 2.0]), eng.set_instance_input_bounds(*a_rows)))
    assert k1 == FUSED and all(_same(a, b) for a, b in zip(inst, got))


def test_one_kind_per_instance_and_the_other_shared(gpu):
    """Inputs per instance (the rows of box C) with shared outputs (`mild-upper`), then, on the same handle, shared inputs
    ([-4, 6]) with outputs per instance (the rows of box B): each instance at the bars against the reference with its pair."""
    spec = IC.spec_of("none")
    Bq = 8
    d, up, yp = IC.data()
    culo, cuhi, _, _ = IC.box("C")
    _, _, bylo, byhi = IC.box("B")
    ylo, yhi = OB.BOXES["mild-upper"]
    with T._engine(spec, 400, Bq) as eng:
        eng.set_data(d["u_d"][:Bq], d["y_d"][:Bq])
        eng.set_instance_input_bounds(culo[:Bq], cuhi[:Bq])
        eng.set_output_bounds(ylo, yhi)
        first = _outputs(eng.step(up[:Bq], yp[:Bq]))
        eng.set_input_bounds(*OB.U_BOX)
        eng.set_instance_output_bounds(bylo[:Bq], byhi[:Bq])
        second = _outputs(eng.step(up[:Bq], yp[:Bq]))
    for tag, (u, c, st, it), pair in (("u per instance", first, lambda b: (ylo, yhi, culo[b], cuhi[b])),
                                      ("y per instance", second, lambda b: (bylo[b], byhi[b]) + OB.U_BOX)):
        assert np.all(st == 0), st
        for b in range(Bq):
            y0, y1, u0, u1 = pair(b)
            sol = yref.solve_bounded(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], y0, y1, u_min=u0, u_max=u1)
            eu = np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
            ec = abs(c[b] - sol.cost) / abs(sol.cost)
            print(tag, b, sol.status, "iters %d/%d margin %.1e err_u %.1e err_cost %.1e" % (it[b], sol.iters, sol.margin, eu, ec))
            assert sol.status == "optimal" and eu < TOL_U and ec < TOL_COST, (tag, b, eu, ec)


# ------------------------------------------------------------------------------------------------ 2. uniform rows are the shared call
@pytest.mark.parametrize("mode", list(IC.MODES))
@pytest.mark.parametrize("box", ["u02", "u+y"])
def test_uniform_rows_are_bit_equal_to_the_shared_call(gpu, box, mode):
    spec = IC.spec_of(mode)
    Bq, n_steps = 8, 12
    d, up, yp = IC.data()
    u_d, y_d, up, yp = d["u_d"][:Bq], d["y_d"][:Bq], up[:Bq], yp[:Bq]
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(11).uniform(-1.0, 1.0, (Bq, n_steps, 2))
    ub = ([0.0, 0.0], [2.0, 2.0]) if box == "u02" else OB.U_BOX
    yb = None if box == "u02" else OB.Y_BOX

    def run(per_instance):
        out = {}
        with T._engine(spec, 400, Bq) as eng:
            eng.set_data(u_d, y_d)
            if per_instance:
                eng.set_instance_input_bounds(_rows(ub[0], Bq), _rows(ub[1], Bq))
                if yb:
                    eng.set_instance_output_bounds(_rows(yb[0], Bq), _rows(yb[1], Bq))
            else:
                eng.set_input_bounds(*ub)
                if yb:
                    eng.set_output_bounds(*yb)
            for safe in (False, True):
                eng.set_box_safeguard(safe)
                res = _outputs(eng.solve(up, yp)) + [OB._full_x(eng)] + _outputs(eng.step(up, yp)) + [OB._full_x(eng)]
                for nms in (1, 3):
                    res += _outputs(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up, yp, w, n_mpc_step=nms))
                    res.append(eng.closed_loop_kernel_name())
                out[safe] = res
        return out

    shared, inst = run(False), run(True)
    for safe in (False, True):
        st, it = shared[safe][2], shared[safe][3]
        print(box, mode, "safeguard", safe, "status", st.tolist(), "iters", it.tolist())
        assert np.any(it >= 2)                                        # the box acts
        for a, b in zip(shared[safe], inst[safe]):
            if isinstance(a, str):
                assert (a, b) == (SHARED_FUSED, FUSED)
            else:
                assert _same(a, b)


# ------------------------------------------------------------------------------------------------ 3. against the reference
@pytest.mark.parametrize("mode", list(IC.MODES))
@pytest.mark.parametrize("name", IC.NAMES)
def test_solve_and_step_against_every_instances_own_reference(gpu, name, mode):
    spec = IC.spec_of(mode)
    d, up, yp = IC.data()
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        IC.set_box(eng, IC.box(name))
        uc, cc, sc, itc = _outputs(eng.solve(up, yp))
        xc = OB._full_x(eng)
        eng.prepare()
        us, cs, ss, its = _outputs(eng.step(up, yp))
        xs = OB._full_x(eng)
    for a, b in ((uc, us), (cc, cs), (sc, ss), (itc, its), (xc, xs)):     # ddmpc_solve and ddmpc_prepare + ddmpc_step
        assert np.array_equal(a, b)
    assert np.all(sc == 0), sc
    full = 0
    for b in range(B32):
        sol = IC.reference(name, mode, b)
        assert sol.status == "optimal"
        full += _check_against(sol, b, spec, d, uc[b], cc[b], itc[b], xc[b], "%s %s" % (name, mode))
    print(name, mode, "instances compared in iters and active set:", full)
    assert full >= B32 - 4


# ------------------------------------------------------------------------------------------------ 4. neighbours
def test_one_hard_row_leaves_its_neighbours_bit_equal(gpu):
    """Row 7 of box A becomes [0.9, 1.1] on both channels.  On that instance the primal-dual rule needs 19 solves (slack NONE; it
    does not cycle there), so under a cap of max_iter = 12 -- the other 31 rows of A end in 3 .. 11 -- it is the one instance at
    the cap: solver_error without the safeguard, solved by it with DDMPC_OPT_BOX_SAFEGUARD = 1."""
    mode, cap = "none", 12
    spec = IC.spec_of(mode)
    d, up, yp = IC.data()
    ulo, uhi, _, _ = IC.box("A")
    hlo, hhi = ulo.copy(), uhi.copy()
    hlo[7], hhi[7] = 0.9, 1.1
    pdas = uref.solve_bounded(spec, d["u_d"][7], d["y_d"][7], up[7], yp[7], hlo[7], hhi[7], max_iter=cap)
    assert pdas.status == "solver_error" and pdas.iters == cap
    out = {}
    for key, lo, hi in (("A", ulo, uhi), ("hard", hlo, hhi)):
        with T._engine(spec, 400, B32, max_iter=cap) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_instance_input_bounds(lo, hi)
            for safe in (False, True):
                eng.set_box_safeguard(safe)
                out[key, safe] = _outputs(eng.step(up, yp)) + [OB._full_x(eng)]
    others = np.arange(B32) != 7
    for safe in (False, True):
        a, h = out["A", safe], out["hard", safe]
        assert np.all(a[2] == 0) and np.all(a[3] < cap), (a[2], a[3])
        for x, y in zip(a, h):
            assert np.array_equal(x[others], y[others])
    u0, c0, s0, i0, _ = out["hard", False]
    u1, c1, s1, i1, x1 = out["hard", True]
    print("instance 7: status %d iters %d without the safeguard, status %d iters %d with it" % (s0[7], i0[7], s1[7], i1[7]))
    assert s0[7] == 4 and i0[7] == cap
    sol = sref.solve_safeguarded(spec, d["u_d"][7], d["y_d"][7], up[7], yp[7], hlo[7], hhi[7])
    eu = np.max(np.abs(u1[7] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(c1[7] - sol.cost) / abs(sol.cost)
    print("safeguard reference: %s, %d solves; err_u %.1e err_cost %.1e" % (sol.status, sol.iters, eu, ec))
    assert sol.status == "optimal" and s1[7] == 0 and i1[7] > cap
    assert eu < TOL_U and ec < TOL_COST, (eu, ec)
    assert OB._within(x1[7, NA + 8:NA + NU].reshape(-1, 2), hlo[7], hhi[7])


# ------------------------------------------------------------------------------------------------ 5. channel indexing on m != p
MNE_U_MAX1 = [0.5, 0.7, 0.55, 0.6]          # input channel 1 of instance b; input channel 0 unbounded
MNE_Y_MIN1 = [0.05, -0.4, 0.1, -0.3]        # output channel 1 of instance b; output channels 0 and 2 unbounded


def mne_case():
    """m = 2, p = 3, n = 2, L = 7 with D != 0 ((2 + 3)(7 + 2) = 45 rows, CONVEX with the terminal constraint), batch 4.  The
    channel table holds [u0 u1 y0 y1 y2] twice: input channel 1 is entry 1, output channel 1 is entry 3 -- a table read with the
    outputs first, or indexed by the channel within its kind, takes another instance's or another channel's bound.  Chosen with
    the reference on the CPU: the unbounded solutions reach 0.64 .. 0.97 on input channel 1 and -0.06 .. -0.65 on output channel 1,
    so every bound below cuts; all four end `optimal` in 3 .. 5 solves with margins >= 2e-4 and at least one active input and one
    active output each."""
    case = CP.make_case(2, 3, 1, 2, 7, "convex", feedthrough=True, B=4, n_steps=6)
    ulo, uhi = np.full((4, 2), -INF), np.full((4, 2), INF)
    ylo, yhi = np.full((4, 3), -INF), np.full((4, 3), INF)
    uhi[:, 1] = MNE_U_MAX1
    ylo[:, 1] = MNE_Y_MIN1
    return case, ulo, uhi, ylo, yhi


def test_channel_indexing_on_a_plant_with_m_ne_p(gpu):
    case, ulo, uhi, ylo, yhi = mne_case()
    spec = case["spec"]
    assert np.any(case["plant"]["D"] != 0.0)
    with CP.engine(case) as eng:
        eng.set_data(case["u_d"], case["y_d"])
        eng.set_instance_input_bounds(ulo, uhi)
        eng.set_instance_output_bounds(ylo, yhi)
        us, cs, ss, its = _outputs(eng.step(case["up"], case["yp"]))
        ubar, ybar = eng.get_solution("ubar"), eng.get_solution("ybar")
        uc, cc, sc, itc = _outputs(eng.solve(case["up"], case["yp"]))
    for a, b in ((us, uc), (cs, cc), (ss, sc), (its, itc)):
        assert np.array_equal(a, b)
    assert np.all(ss == 0)
    free_y = OB._free_outputs(spec, ybar)
    nfree = spec.L - spec.n
    free_u = ubar[:, spec.n * spec.m:(spec.n + nfree) * spec.m].reshape(4, nfree, spec.m)
    for b in range(4):
        sol = yref.solve_bounded(spec, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], ylo[b], yhi[b], u_min=ulo[b],
                                 u_max=uhi[b])
        x0 = sol.x.size - 2 * spec.Ln * spec.p - spec.Ln * spec.m                    # [alpha; ubar; ybar; sigma]
        usec = (sol.idx >= x0) & (sol.idx < x0 + spec.Ln * spec.m)
        ysec = (sol.idx >= x0 + spec.Ln * spec.m) & (sol.idx < x0 + spec.Ln * (spec.m + spec.p))
        nu_act, ny_act = int(np.sum(usec & (sol.active != 0))), int(np.sum(ysec & (sol.active != 0)))
        eu = np.max(np.abs(us[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(cs[b] - sol.cost) / abs(sol.cost)
        print("m != p b=%d %s iters %d/%d margin %.1e active inputs %d outputs %d err_u %.1e err_cost %.1e" %
              (b, sol.status, its[b], sol.iters, sol.margin, nu_act, ny_act, eu, ec))
        assert sol.status == "optimal" and sol.margin >= MARGIN and nu_act >= 1 and ny_act >= 1
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        assert its[b] == sol.iters
        assert np.sum(free_u[b, :, 1] == uhi[b, 1]) == nu_act, b                       # held at ITS bound exactly
        assert np.sum(free_y[b, :, 1] == ylo[b, 1]) == ny_act, b


# ------------------------------------------------------------------------------------------------ 6. fused loop
LOOP_ROWS = [0, 9, 18, 27]


def _loop_case():
    d, up, yp = IC.data()
    ulo, uhi, _, _ = IC.box("A")
    r = LOOP_ROWS
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B32, 20, 2))[r, :10]
    return d["u_d"][r], d["y_d"][r], d["x_end"][r], up[r], yp[r], ulo[r], uhi[r], w


@pytest.mark.parametrize("mode,n_mpc_step", [("none", 1), ("none", 3), ("convex-tec", 3)])
def test_fused_loop_against_the_cold_path_and_the_reference(gpu, mode, n_mpc_step):
    """Instances 0, 9, 18, 27 of box A (27: channel 0 unbounded), 10 steps.  On the CPU the reference's loop driver is optimal at
    every solve of all four for n_mpc_step 1 and 3 in both modes."""
    spec = IC.spec_of(mode)
    u_d, y_d, x0, up, yp, ulo, uhi, w = _loop_case()
    P = orc.FOUR_TANK
    out = {}
    with T._engine(spec, 400, 4) as eng:
        eng.set_data(u_d, y_d)
        eng.set_instance_input_bounds(ulo, uhi)
        args = (P["A"], P["B"], P["C"], P["D"], x0, up, yp, w)
        eng.set_closed_loop_path("cold")
        out["cold"] = eng.closed_loop(*args, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        ub_cold = eng.get_solution("ubar")
        eng.set_closed_loop_path("auto")
        out["fused"] = eng.closed_loop(*args, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == FUSED
        ub = eng.get_solution("ubar")
        its = eng.step(up, yp)[3].copy()
    assert np.array_equal(out["cold"][2], out["fused"][2]) and np.all(out["fused"][2] == 0)
    for a, b in zip(out["cold"][:2], out["fused"][:2]):
        assert OB._rel(np.asarray(a), np.asarray(b)) < TOL_U
    assert OB._rel(ub, ub_cold) < TOL_U
    assert np.all(its >= 2)                                                            # the box acts at the first solve of the loop
    u_sys, y_sys = out["fused"][0], out["fused"][1]
    for i, b in enumerate(LOOP_ROWS):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = x0[i].copy()
        ur, yr = uref.closed_loop_bounded(spec, u_d[i], y_d[i], plant, w[i], ulo[i], uhi[i], n_mpc_step=n_mpc_step)
        eu, ey = np.max(np.abs(u_sys[i] - ur)) / np.max(np.abs(ur)), np.max(np.abs(y_sys[i] - yr)) / np.max(np.abs(yr))
        print("loop %s n_mpc_step %d b=%d err_u %.1e err_y %.1e" % (mode, n_mpc_step, b, eu, ey))
        assert eu < TOL_U and ey < TOL_U, (b, eu, ey)
        lo, hi = ulo[i], uhi[i]
        assert OB._within(u_sys[i], lo, hi)


def test_no_read_of_the_trajectories_after_prepare(gpu):
    torch = pytest.importorskip("torch")
    spec = IC.spec_of("convex-tec")
    d, up, yp = IC.data()
    ulo, uhi, ylo, yhi = IC.box("C")
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(3).uniform(-1.0, 1.0, (B32, 12, 2))
    ut = torch.tensor(d["u_d"], device="cuda:0")
    yt = torch.tensor(d["y_d"], device="cuda:0")
    with T._engine(spec, 400, B32) as eng:
        eng.set_data(ut, yt)
        eng.set_instance_input_bounds(ulo, uhi)
        eng.set_instance_output_bounds(ylo, yhi)
        eng.prepare()
        s0 = _outputs(eng.step(up, yp))
        cl0 = _outputs(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w))
        assert eng.closed_loop_kernel_name() == FUSED
        torch.cuda.synchronize()
        ut.fill_(float("nan"))
        yt.fill_(float("nan"))
        torch.cuda.synchronize()
        s1 = _outputs(eng.step(up, yp))
        cl1 = _outputs(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w))
    assert np.all(s0[3] >= 2) and np.all(s0[2] == 0) and np.all(np.isfinite(s1[0]))
    for a, b in zip(s0 + cl0, s1 + cl1):
        assert _same(a, b)


# ------------------------------------------------------------------------------------------------ 7. the warm-start option
def test_the_warm_start_option_is_accepted_and_not_honoured(gpu):
    spec = IC.spec_of("convex-tec")
    Bq = 8
    d, up, yp = IC.data()
    ulo, uhi, ylo, yhi = IC.box("C")
    P = orc.FOUR_TANK
    w = 0.002 * np.random.default_rng(13).uniform(-1.0, 1.0, (Bq, 9, 2))
    out = {}
    for warm in (False, True):
        with T._engine(spec, 400, Bq) as eng:
            eng.set_data(d["u_d"][:Bq], d["y_d"][:Bq])
            eng.set_instance_input_bounds(ulo[:Bq], uhi[:Bq])
            eng.set_instance_output_bounds(ylo[:Bq], yhi[:Bq])
            eng.set_box_warm_start(warm)
            res = _outputs(eng.solve(up[:Bq], yp[:Bq]))
            for _ in range(2):                                                        # (the second would start from the first's set)
                res += _outputs(eng.step(up[:Bq], yp[:Bq])) + [OB._full_x(eng)]
            for _ in range(2):
                res += _outputs(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:Bq], up[:Bq], yp[:Bq], w, n_mpc_step=3))
                assert eng.closed_loop_kernel_name() == FUSED
            res += _outputs(eng.step(up[:Bq], yp[:Bq]))
            out[warm] = res
    assert np.all(out[False][3] >= 2)
    for a, b in zip(out[False], out[True]):
        assert _same(a, b)
