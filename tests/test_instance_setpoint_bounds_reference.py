"""CPU premises of tests/test_gpu_instance_setpoint_bounds.py (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS): the fixtures of
tests/_instance_setpoint_cases.py solved by the reference alone, and the Python surface of the option.

Held here: every reference solve is optimal; no step solve keeps less than the 1e-7 margin under which `iters` and the signed set
would be left out (the smallest is 2.8e-7, C under `convex-tec`, instance 1); the solve counts of A under `none` are
5, 4, 5, 4, 5, 6, 7, 7; the active counts span 4 .. 51 (both homes of the k x k system); every solve of the compared loop cases
keeps at least 1e-7 (measured here: 6.7e-5 under `none`, 4.4e-7 under `convex-tec`); the m != p case at the recorded perturbation."""
import numpy as np

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC

import _instance_setpoint_cases as SC
import _setpoint_box_ref as ref

B8 = SC.B8


def test_python_surface_of_the_option():
    assert L.OPT_INSTANCE_SETPOINT_BOUNDS == 23
    assert callable(BatchedDDMPC.set_instance_setpoint_bounds)


def test_boxes_and_setpoints():
    t = ref.tank()
    ulo, uhi, ylo, yhi = SC.box("C")
    assert np.array_equal(SC.box("A")[0], ulo) and np.array_equal(SC.box("A")[1], uhi)
    assert np.array_equal(ulo[0], [-4.0, -4.0]) and np.array_equal(uhi[0], [6.0, 6.0])
    assert np.array_equal(ulo[7], [-np.inf, 0.0]) and np.array_equal(uhi[7], [np.inf, 2.0])
    assert np.all(np.isinf(ulo[[3, 7], 0])) and np.all(np.isfinite(ulo[[0, 1, 2, 4, 5, 6], 0]))
    assert np.isinf(yhi[5, 0]) and np.all(np.isfinite(np.delete(yhi[:, 0], 5))) and np.all(np.isinf(ylo[:, 0]))
    # the terminal constraint: every instance's setpoint, and the handle's own, inside every row they meet
    s = SC.spec_of("none-tec")
    assert np.all(t["us"] >= ulo) and np.all(t["us"] <= uhi) and np.all(t["ys"] >= ylo) and np.all(t["ys"] <= yhi)
    assert np.all(s.u_s >= ulo) and np.all(s.u_s <= uhi) and np.all(s.y_s >= ylo) and np.all(s.y_s <= yhi)
    lulo, luhi, lylo, lyhi = SC.loop_box("C")
    _, u_ref, y_ref = SC.loop_case("convex-tec")
    assert np.all(np.isinf(lulo[2, 0])) and np.all(np.isfinite(np.delete(lulo[:, 0], 2)))
    assert np.all(u_ref >= lulo[:, None]) and np.all(u_ref <= luhi[:, None])
    assert np.all(y_ref >= lylo[:, None]) and np.all(y_ref <= lyhi[:, None])


def test_step_references():
    ks, margins = [], []
    for name in SC.NAMES:
        for mode in SC.MODES:
            sols = [SC.step_reference(name, mode, b) for b in range(B8)]
            assert all(s.status == "optimal" for s in sols), (name, mode)
            print(name, mode, "iters", [s.iters for s in sols], "k", [int(np.count_nonzero(s.active)) for s in sols],
                  "margins", ["%.1e" % s.margin for s in sols])
            ks += [int(np.count_nonzero(s.active)) for s in sols]
            margins += [s.margin for s in sols]
    assert min(margins) >= SC.MARGIN and 2.5e-7 < min(margins) < 3.1e-7, min(margins)     # nothing is left out today
    assert [SC.step_reference("A", "none", b).iters for b in range(B8)] == SC.A_NONE_ITERS
    assert (min(ks), max(ks)) == (4, 51) and any(k <= 16 for k in ks) and any(k > 16 for k in ks)
    # the safeguard cases (max_iter = 6): the instances whose count exceeds the cap are 6 and 7 under A and under C
    for name in SC.NAMES:
        assert [b for b in range(B8) if SC.step_reference(name, "none", b).iters > 6] == [6, 7]


def test_refusal_references():
    """Instance 0 ([-4, 6]) solves at the setpoint that instance 7's [0, 2] refuses; instance 7 of A proper (channel 0 unbounded)
    solves at it too."""
    t = ref.tank()
    for bx, b in ((SC.box("A", ufree=(3,)), 0), (SC.box("A"), 7)):
        sol = SC.solve_at("none-tec", bx, b, SC.BAD_US, t["ys"][b])
        print("refusal reference b=%d %s iters %d margin %.1e" % (b, sol.status, sol.iters, sol.margin))
        assert sol.status == "optimal" and sol.margin >= SC.MARGIN


def test_loop_references():
    for mode in SC.LOOP_MODES:
        low = []
        for nms in SC.LOOP_NMS:
            for b in range(SC.LOOP_B):
                sols = SC.loop_reference(mode, b, nms)[5]           # (schedule_loop raises on a solve that is not optimal)
                low.append(min(s.margin for s in sols))
        print(mode, "smallest loop margin %.1e" % min(low))
        assert min(low) >= SC.MARGIN


def test_m_ne_p_references():
    case, ulo, uhi, ylo, yhi, us, ys = SC.mne()
    s = case["spec"]
    assert s.m == 2 and s.p == 3 and s.tec
    assert np.all(us >= ulo) and np.all(us <= uhi) and np.all(ys >= ylo) and np.all(ys <= yhi)
    for b in range(4):
        sol = SC.mne_reference(b)
        nu_act, ny_act = SC.mne_active(s, sol)
        print("m != p b=%d %s iters %d margin %.1e active inputs %d outputs %d" % (b, sol.status, sol.iters, sol.margin, nu_act, ny_act))
        assert sol.status == "optimal" and sol.margin >= 1e-6 and nu_act >= 1 and ny_act >= 1
