"""Safeguarded active set for input bounds (DDMPC_OPT_BOX_SAFEGUARD): an instance of a bounded handle whose primal-dual
iteration ends at the max_iter cap is finished by a primal active-set method on the same law, M and box table.  Four-tank,
L = 30, N = 400 (136 rows), batch 32, seeds 500 .. 531 at the data tail: with the box [0.8, 1.2] the primal-dual rule cycles on
instances 4, 20, 24 and 28.  Against the CPU reference of tests/_box_safeguard_ref.py at the standard bars (1e-8 inputs, 1e-9
cost), between two GPU paths at 1e-10.

Tolerances of the KKT certificate of the GPU's solution (test 2), relative to the certificate's own gradient scale: the solution
is held to 1e-8 relative (the bar above) and the certificate's stationarity and multiplier residuals are linear in its error, so
they are held to the same 1e-8; the equality residual is that of the reconstruction H alpha = [ubar; ybar + sigma], which
test_gpu_input_bounds.py holds to 1e-8 of the trajectory; an input at a bound is the bound exactly and a free one is inside the
box up to one rounding of the output stage (1e-12, as `_within` there)."""

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from oracle import ddmpc_oracle as orc

import _box_safeguard_ref as sg
import _input_bounds_ref as ref
import test_gpu_closed_loop_plants as CP
import test_gpu_input_bounds as IB
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST, TOL_GPU = 1e-8, 1e-9, 1e-10
INF = np.inf
B32 = sg.NB
CAP = 50
NBOX = 2 * 26 + 2 * 30                                  # CONVEX + terminal constraint, both channels: 52 inputs, 60 slacks
WIDE = ([-4.0, -4.0], [6.0, 6.0])
FUSED = "ddmpc_closed_loop_box_kernel"
_RUN = {}


def _spec(slack=1, tec=True):
    return orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)


def _run(slack, tec, lo, hi, cap, safe, calls=("step",)):
    """(u, cost, status, iters, x) per call of one engine on the 32 instances, computed once per argument set."""
    key = (slack, tec, tuple(lo), tuple(hi), cap, safe, calls)
    if key not in _RUN:
        d, up, yp = sg.data()
        out = {}
        with T._engine(_spec(slack, tec), 400, B32, max_iter=cap) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_input_bounds(lo, hi)
            if safe is not None:
                eng.set_box_safeguard(safe)
            for c in calls:
                res = [x.copy() for x in (eng.step(up, yp) if c == "step" else eng.solve(up, yp))]
                out[c] = res + [IB._full_x(eng)]
        _RUN[key] = out
    return _RUN[key]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _relc(a, b):
    return np.max(np.abs(a - b) / np.abs(b))


def _against_reference(tag, b, sol, u, cost, x, spec, lo, hi):
    """Instance b of a GPU result against a converged CPU safeguarded solution: bars, signed active set, box."""
    eu = np.max(np.abs(u - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
    ec = abs(cost - sol.cost) / abs(sol.cost)
    print("%s b=%d ref solves %d kmax %d k %d err_u %.1e err_cost %.1e" %
          (tag, b, sol.iters, sol.kmax, np.count_nonzero(sol.active), eu, ec))
    assert sol.status == "optimal"
    assert eu < TOL_U and ec < TOL_COST, (tag, b, eu, ec)
    assert np.array_equal(IB._signed_active(x, sol), sol.active), (tag, b)
    na = x.size - spec.Ln * (spec.m + 2 * spec.p)       # x = [alpha; ubar; ybar; sigma]
    assert IB._within(IB._free_inputs(spec, x[None, na:na + spec.Ln * spec.m]), lo, hi), (tag, b)


# ------------------------------------------------------------------------------------------------ 1. contract
def test_contract_option_values_default_and_bit_equality_below_the_cap(gpu):
    with T._engine(_spec(), 400, 2) as eng:
        for bad in (2, -1):
            with pytest.raises(L.DDMPCError) as e:
                L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_BOX_SAFEGUARD, bad))
            assert e.value.code == L.ERR_INVALID and "DDMPC_OPT_BOX_SAFEGUARD" in e.value.message
        eng.set_box_safeguard(True)                      # accepted without bounds: no effect
        eng.set_box_safeguard(False)
    with T._engine(orc.spec_from_params(controller_type=0), 400, 2) as eng:
        eng.set_box_safeguard(True)                      # ... and on any handle
    never = _run(1, True, *sg.TIGHT, CAP, None)["step"]
    off = _run(1, True, *sg.TIGHT, CAP, False)["step"]
    on = _run(1, True, *sg.TIGHT, CAP, True)["step"]
    for a, b in zip(never, off):
        assert np.array_equal(a, b, equal_nan=True)
    u0, c0, s0, i0 = off[:4]
    cyc = np.zeros(B32, bool)
    cyc[list(sg.CYCLING)] = True
    print("option 0: status", s0.tolist(), "iters", i0.tolist())
    assert np.all(s0[cyc] == 4) and np.all(i0[cyc] == CAP)
    assert np.all(s0[~cyc] == 0) and np.all(i0[~cyc] <= CAP)
    u1, c1, s1, i1 = on[:4]
    assert np.array_equal(u1[~cyc], u0[~cyc]) and np.array_equal(c1[~cyc], c0[~cyc])
    assert np.array_equal(s1[~cyc], s0[~cyc]) and np.array_equal(i1[~cyc], i0[~cyc])
    assert np.all(s1[cyc] == 0) and np.all(i1[cyc] > CAP)


# ------------------------------------------------------------------------------------------------ 2. the cycling instances
def test_cycling_instances_against_the_reference(gpu):
    spec = _spec()
    out = _run(1, True, *sg.TIGHT, CAP, True, ("step", "solve"))
    d, up, yp = sg.data()
    for call in ("step", "solve"):
        u, cost, st, it, x = out[call]
        for b in sg.CYCLING:
            sol = sg.cached("safe", 1, True, b, *sg.TIGHT)
            print("%s b=%d status %d iters %d" % (call, b, st[b], it[b]))
            assert st[b] == 0 and CAP < it[b] <= CAP + 4 * NBOX + 16, (call, b, st[b], it[b])
            assert sol.idx.size == NBOX
            _against_reference(call, b, sol, u[b], cost[b], x[b], spec, *sg.TIGHT)
            cert = ref.kkt_certificate(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b], *sg.TIGHT, x[b])
            print("   certificate", {k: "%.1e" % v for k, v in cert.items()})
            tol = 1e-8 * cert["grad_scale"]
            assert cert["res_stat"] < tol and cert["dual_sign"] < tol, (call, b, cert)
            assert cert["res_eq"] < 1e-8 * np.max(np.abs(x[b])) and cert["res_box"] <= 1e-12 * 1.2, (call, b, cert)
    us, cs, ss, its = out["step"][:4]
    uc, cc, sc, itc = out["solve"][:4]
    assert np.array_equal(ss, sc) and np.array_equal(its, itc)
    assert _rel(us, uc) < TOL_GPU and _relc(cs, cc) < TOL_GPU


# ------------------------------------------------------------------------------------------------ 3. cross-check on all instances
@pytest.mark.parametrize("slack,tec", [(1, True), (0, False)])
def test_every_instance_through_the_safeguard_matches_the_primal_dual_result(gpu, slack, tec):
    u0, c0, s0, i0 = _run(slack, tec, *sg.TIGHT, CAP, False)["step"][:4]
    u1, c1, s1, i1 = _run(slack, tec, *sg.TIGHT, 3, True)["step"][:4]
    nbox = NBOX if slack else 2 * 30
    print("cap 50, option 0: status", s0.tolist(), "iters", i0.tolist())
    print("cap 3, option 1: status", s1.tolist(), "iters", i1.tolist())
    assert np.all(s1 == 0) and np.all(i1 > 3) and np.all(i1 <= 3 + 4 * nbox + 16)
    conv = s0 == 0
    if slack:
        assert np.array_equal(np.nonzero(~conv)[0], sg.CYCLING)
    assert np.count_nonzero(conv) >= B32 // 2
    eu, ec = _rel(u1[conv], u0[conv]), _relc(c1[conv], c0[conv])
    print("err_u %.1e err_cost %.1e" % (eu, ec))
    assert eu < TOL_GPU and ec < TOL_GPU


# ------------------------------------------------------------------------------------------------ 4. both homes of the k x k system
@pytest.mark.parametrize("name,lo,hi", [("lds", *WIDE), ("scratch", *sg.TIGHT)])
def test_both_homes_of_the_working_set_system(gpu, name, lo, hi):
    spec = _spec()
    u, cost, st, it, x = _run(1, True, lo, hi, 1, True)["step"]
    assert np.all(st == 0) and np.all(it >= 1)
    kmax = []
    for b in sg.CYCLING:
        sol = sg.cached("safe", 1, True, b, lo, hi)
        assert it[b] > 1
        _against_reference(name, b, sol, u[b], cost[b], x[b], spec, lo, hi)
        kmax.append(sol.kmax)
    assert (1 <= min(kmax) and max(kmax) <= 16) if name == "lds" else min(kmax) > 16, kmax


# ------------------------------------------------------------------------------------------------ 5. one-sided bounds, another plant
def test_one_sided_and_infinite_bounds(gpu):
    spec = _spec()
    lo, hi = [-INF, 0.5], [3.0, INF]
    u, cost, st, it, x = _run(1, True, lo, hi, 1, True)["step"]
    u0, c0, s0, i0 = _run(1, True, lo, hi, CAP, False)["step"][:4]
    assert np.all(st == 0) and np.all(s0 == 0)
    assert _rel(u, u0) < TOL_GPU and _relc(cost, c0) < TOL_GPU
    for b in (0, 16):
        _against_reference("one-sided", b, sg.cached("safe", 1, True, b, lo, hi), u[b], cost[b], x[b], spec, lo, hi)


def test_one_bounded_channel_on_a_plant_with_m_ne_p(gpu):
    case = CP.make_case(2, 3, 1, 2, 7, "convex", feedthrough=False, B=8, n_steps=6)          # (2 + 3)(7 + 2) = 45 rows
    spec = case["spec"]
    lo, hi = [spec.u_s[0] - 0.1, -INF], [spec.u_s[0] + 0.1, INF]                             # channel 1 is not in the box list
    res = {}
    for cap, safe in ((CAP, False), (1, True)):
        with CP.engine(case, max_iter=cap) as eng:
            eng.set_data(case["u_d"], case["y_d"])
            eng.set_input_bounds(lo, hi)
            eng.set_box_safeguard(safe)
            res[safe] = [x.copy() for x in eng.step(case["up"], case["yp"])] + [IB._full_x(eng)]
    u0, c0, s0, i0 = res[False][:4]
    u1, c1, s1, i1, x1 = res[True]
    assert np.all(s0 == 0) and np.all(s1 == 0) and np.all(i1 > 1)
    assert _rel(u1, u0) < TOL_GPU and _relc(c1, c0) < TOL_GPU
    for b in range(8):
        sol = sg.solve_safeguarded(spec, case["u_d"][b], case["y_d"][b], case["up"][b], case["yp"][b], lo, hi)
        _against_reference("m!=p", b, sol, u1[b], c1[b], x1[b], spec, lo, hi)


# ------------------------------------------------------------------------------------------------ 6. fused closed loop
N_LOOP = 12


def _loop_noise():
    return 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B32, N_LOOP, 2))


@pytest.mark.parametrize("n_mpc_step", [1, 2])
def test_fused_closed_loop_against_the_cold_path(gpu, n_mpc_step):
    d, up, yp = sg.data()
    P = orc.FOUR_TANK
    w = _loop_noise()
    out = {}
    with T._engine(_spec(), 400, B32, max_iter=3) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_input_bounds(*WIDE)
        out["off"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == FUSED
        eng.set_box_safeguard(True)
        eng.set_closed_loop_path("cold")
        out["cold"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == "ddmpc_plant_kernel"
        eng.set_closed_loop_path("auto")
        out["fused"] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
        assert eng.closed_loop_kernel_name() == FUSED              # the kernel name is unchanged
    print("option 0 status", out["off"][2].tolist())
    assert np.any(out["off"][2] == 4)                              # without the safeguard the cap of 3 stops instances
    assert np.all(out["fused"][2] == 0) and np.all(out["cold"][2] == 0)          # no instance stops
    for a, b in zip(out["cold"], out["fused"]):
        a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
        assert np.all(np.isfinite(b))
        assert np.max(np.abs(a - b)) <= TOL_GPU * max(np.max(np.abs(a)), 1.0)
    assert IB._within(out["fused"][0], *WIDE)
    _RUN[("loop", n_mpc_step)] = out["fused"]


@pytest.mark.parametrize("n_mpc_step", [1, 2])
def test_fused_closed_loop_against_a_loop_driven_by_the_reference(gpu, n_mpc_step):
    d, up, yp = sg.data()
    P = orc.FOUR_TANK
    w = _loop_noise()
    if ("loop", n_mpc_step) not in _RUN:
        with T._engine(_spec(), 400, B32, max_iter=3) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_input_bounds(*WIDE)
            eng.set_box_safeguard(True)
            _RUN[("loop", n_mpc_step)] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
            assert eng.closed_loop_kernel_name() == FUSED
    u_sys, y_sys, st = _RUN[("loop", n_mpc_step)][:3]
    for b in (0, 4):
        plant = orc.Plant(P["A"], P["B"], P["C"], P["D"], P["eps_max"])
        plant.x = d["x_end"][b].copy()
        ur, yr = sg.closed_loop_safeguarded(_spec(), d["u_d"][b], d["y_d"][b], plant, w[b], *WIDE, n_mpc_step=n_mpc_step)
        eu, ey = np.max(np.abs(u_sys[b] - ur)) / np.max(np.abs(ur)), np.max(np.abs(y_sys[b] - yr)) / np.max(np.abs(yr))
        print("n_mpc_step %d b=%d err_u %.1e err_y %.1e" % (n_mpc_step, b, eu, ey))
        assert st[b] == 0 and eu < TOL_U and ey < TOL_U, (b, eu, ey)


# ------------------------------------------------------------------------------------------------ 7. refinement
def test_laws_from_refining_solves_report_inaccurate_after_the_safeguard(gpu):
    spec = _spec()
    d, up, yp = sg.data()
    lo, hi = WIDE
    rng = np.random.default_rng(7)
    up, yp = up.copy(), yp.copy()
    half = B32 // 2                                     # second half: windows near the setpoint, inside both boxes
    up[half:] = np.tile(spec.u_s, 4)[None] + 0.01 * rng.uniform(-1, 1, up[half:].shape)
    yp[half:] = np.tile(spec.y_s, 4)[None] + 0.002 * rng.uniform(-1, 1, yp[half:].shape)
    with T._engine(spec, 400, B32, max_iter=1) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        eng.set_input_bounds(lo, hi)
        eng.set_box_safeguard(True)
        L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_REFINE_RES_LOG10, 3000))      # AUTO flags every instance
        us, cs, ss, its = (x.copy() for x in eng.step(up, yp))
        x = IB._full_x(eng)
        uc, cc, sc, itc = (x_.copy() for x_ in eng.solve(up, yp))
    assert np.array_equal(ss, sc) and np.array_equal(its, itc)
    free = IB._free_inputs(spec, x[:, IB.NA:IB.NA + IB.NU])
    sgm = x[:, IB.NA + 2 * IB.NU + 8:]
    bound = spec.c * spec.eps_max
    nact = np.sum((free == 6.0) | (free == -4.0), axis=(1, 2)) + np.sum(np.abs(np.abs(sgm) - bound) <= 1e-9 * bound, axis=1)
    print("status", ss.tolist(), "iters", its.tolist(), "active", nact.tolist())
    assert np.array_equal(ss, np.where(nact > 0, 1, 0)), (ss, nact)
    assert np.any(ss == 1) and np.any(ss == 0)
    assert np.array_equal(its == 1, nact == 0) and np.all(its[nact > 0] > 1)            # (> max_iter: the safeguard ran)
    for b in (0, 4):
        sol = sg.cached("safe", 1, True, b, lo, hi)
        assert np.count_nonzero(sol.active) > 0 and ss[b] == 1
        assert np.max(np.abs(us[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)) < TOL_U, b


# ------------------------------------------------------------------------------------------------ 8. a kept preparation survives
def test_kept_preparation_survives_toggling_the_option(gpu):
    torch = pytest.importorskip("torch")
    d, up, yp = sg.data()
    ut = torch.tensor(d["u_d"], device="cuda:0")
    yt = torch.tensor(d["y_d"], device="cuda:0")
    with T._engine(_spec(), 400, B32, max_iter=3) as eng:
        eng.set_data(ut, yt)
        eng.set_input_bounds(*sg.TIGHT)
        eng.prepare()
        s0 = [x.copy() for x in eng.step(up, yp)]
        torch.cuda.synchronize()
        ut.fill_(float("nan"))                          # a preparation formed again from here on would be NaN
        yt.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.set_box_safeguard(True)
        s1 = [x.copy() for x in eng.step(up, yp)]
        eng.set_box_safeguard(False)
        s2 = [x.copy() for x in eng.step(up, yp)]
    assert np.all(s0[2] == 4) and np.all(s0[3] == 3)    # (every instance needs more than 3 solves on this box)
    assert np.all(s1[2] == 0) and np.all(np.isfinite(s1[0])) and np.all(s1[3] > 3)
    other = _run(1, True, *sg.TIGHT, 3, True)["step"]
    assert np.array_equal(s1[0], other[0]) and np.array_equal(s1[1], other[1])
    for a, b in zip(s0, s2):
        assert np.array_equal(a, b, equal_nan=True)
