"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle
on identical inputs.  Tolerances (fp64): relative error of
optimal_u <= 1e-8 (w.r.t. max|u|), relative error of the cost <= 1e-9, identical
status; Hankel gather bit-exact."""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC, hankel_matrix_batched
from direct_data_driven_mpc_amd.harness import controller_params, generate_batch
from oracle import ddmpc_oracle as orc

pytestmark = pytest.mark.gpu

TOL_U, TOL_COST = 1e-8, 1e-9


def _engine(spec, N, B, **kw):
    Q = np.diag(spec.Q) if kw.pop("diag", False) else spec.Q
    R = np.diag(spec.R) if Q.ndim == 1 else spec.R
    return BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=Q, R=R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                        controller_type=L.ROBUST if spec.robust else L.NOMINAL,
                        slack_type=L.SLACK_CONVEX if spec.slack == "convex" else L.SLACK_NONE,
                        eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c,
                        use_terminal_constraint=spec.tec, **kw)


def _instances(B, N=400, seed0=0):
    d = generate_batch(range(seed0, seed0 + B), N=N)
    n = 4
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy()
    yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    return d["u_d"], d["y_d"], up, yp


def _check(spec, u_d, y_d, up, yp, u, cost, status, rows):
    for b in rows:
        sol = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
        eu = np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
        ec = abs(cost[b] - sol.cost) / max(abs(sol.cost), 1e-300)
        assert eu < TOL_U, (b, eu)
        assert ec < TOL_COST, (b, ec)


# ---------------------------------------------------------------------------- a1
def test_hankel_bit_exact(gpu, golden):
    assert np.array_equal(hankel_matrix_batched(golden["kat_X"][None], 2)[0], golden["kat_H"])
    X = np.stack([golden[f"s{s}_u_d"] for s in range(5)])
    H = hankel_matrix_batched(X, 34)
    assert np.array_equal(H[0], golden["s0_Hu"])
    for s in range(5):
        assert np.array_equal(H[s], orc.hankel_matrix(X[s], 34))
    # ragged/edge shapes: single column (N == L), single channel, L == 1
    for (N, nch, Lh) in ((7, 3, 7), (9, 1, 4), (5, 2, 1)):
        Xr = np.random.default_rng(3).normal(size=(2, N, nch))
        Hr = hankel_matrix_batched(Xr, Lh)
        for b in range(2):
            assert np.array_equal(Hr[b], orc.hankel_matrix(Xr[b], Lh))
    with pytest.raises(ValueError, match="N must be greater than or equal to L"):
        hankel_matrix_batched(np.zeros((1, 3, 2)), 4)


def test_hankel_module_functions(gpu, golden):
    from direct_data_driven_mpc.utilities.hankel_matrix import evaluate_persistent_excitation, hankel_matrix
    assert np.array_equal(hankel_matrix(golden["kat_X"], 2), golden["kat_H"])
    rank, ok = evaluate_persistent_excitation(golden["s0_u_d"], 38)
    assert (rank, ok) == (76, True)
    rank, ok = evaluate_persistent_excitation(np.ones((400, 2)), 38)
    assert (rank, bool(ok)) == (int(golden["const_pe_rank"][0]), False)


# ------------------------------------------------------------------ cold solves
@pytest.mark.parametrize("kw", [dict(), dict(slack_var_constraint_type=1), dict(tec=False),
                                dict(tec=False, slack_var_constraint_type=1)],
                         ids=["robust-none-tec", "robust-convex-tec", "robust-none-ucon", "robust-convex-ucon"])
def test_cold_solve_matches_oracle(gpu, kw):
    spec = orc.spec_from_params(**kw)
    B = 24
    u_d, y_d, up, yp = _instances(B)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        assert np.all(status == 0)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        if spec.slack == "convex":
            sol = orc.solve_fullspace(spec, u_d[0], y_d[0], up[0], yp[0])
            assert int(iters[0]) == sol.iters >= 2          # the box binds at the first step (SURVEY hard parts)
            sig = eng.get_solution("sigma")
            assert np.max(np.abs(sig[:, 8:])) <= spec.c * spec.eps_max * (1 + 1e-12)
        else:
            assert np.all(iters == 1)


def test_golden_fixture_solutions(gpu, golden):
    for tag, kw in (("none", {}), ("convex", dict(slack_var_constraint_type=1)), ("ucon", dict(tec=False))):
        spec = orc.spec_from_params(**kw)
        u_d = np.stack([golden[f"s{s}_u_d"] for s in range(5)])
        y_d = np.stack([golden[f"s{s}_y_d"] for s in range(5)])
        up = u_d[:, -4:, :].reshape(5, -1).copy(); yp = y_d[:, -4:, :].reshape(5, -1).copy()
        with _engine(spec, 400, 5) as eng:
            eng.set_data(u_d, y_d)
            u, cost, status, _ = eng.solve(up, yp)
        for s in range(5):
            ref = golden[f"s{s}_{tag}_u"]
            assert np.max(np.abs(u[s] - ref)) / np.max(np.abs(ref)) < TOL_U
            assert abs(cost[s] - golden[f"s{s}_{tag}_cost"][0]) / golden[f"s{s}_{tag}_cost"][0] < TOL_COST
    # survey known answer + third-party solver (scipy trust-constr), looser by that solver's own accuracy
    assert np.allclose(u[0][:2], golden["s0_ucon_u"][:2])
    spec = orc.spec_from_params()
    with _engine(spec, 400, 1) as eng:
        eng.set_data(golden["s0_u_d"][None], golden["s0_y_d"][None])
        u, cost, _, _ = eng.solve(golden["s0_u_d"][-4:].reshape(1, -1), golden["s0_y_d"][-4:].reshape(1, -1))
    assert np.allclose(u[0, :2], [21.22188171, 20.30350327], atol=5e-9) and abs(cost[0] - 4.543214030) < 5e-10
    assert np.max(np.abs(u[0] - golden["scipy_s0_none_u"])) / np.max(np.abs(u[0])) < 1e-7


def test_nominal_known_answer(gpu):
    # BASELINE configs[0]: nominal + noisy (full-row-rank) Hankel => optimal_u == tile(u_s, L), cost == 0
    spec = orc.spec_from_params(controller_type=0)
    B = 6
    u_d, y_d, up, yp = _instances(B)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.solve(up, yp)
        ub = eng.get_solution("ubar"); yb = eng.get_solution("ybar")
    assert np.all(status == 0)
    assert np.max(np.abs(u - np.tile(spec.u_s, spec.L))) < 1e-12
    assert np.max(np.abs(cost)) < 1e-12
    assert np.max(np.abs(ub[:, :8] - up)) < 1e-12 and np.max(np.abs(yb[:, :8] - yp)) < 1e-12
    for b in range(B):   # oracle's min-norm solve is the less accurate side here
        sol = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        assert np.max(np.abs(u[b] - sol.optimal_u)) < 1e-7


def test_diagonal_weights_and_setpoint_change(gpu):
    spec = orc.spec_from_params()
    rng = np.random.default_rng(5)
    spec.Q = np.diag(rng.uniform(1.0, 5.0, spec.p * spec.L))
    spec.R = np.diag(rng.uniform(5e-5, 5e-4, spec.m * spec.L))
    B = 6
    u_d, y_d, up, yp = _instances(B, seed0=100)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        spec.u_s = np.array([0.8, 1.1]); spec.y_s = np.array([0.5, 0.9])
        eng.set_setpoints(spec.u_s, spec.y_s)                      # controller.py:945-982
        u, cost, status, _ = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))


@pytest.mark.parametrize("Lh,N,slack", [(10, 120, 0), (10, 120, 1), (16, 200, 0), (22, 300, 1), (8, 60, 0)])
def test_other_sizes(gpu, Lh, N, slack):
    # exercises the 5-, 7- and 9-tile-row kernel instances and ragged last k-steps
    spec = orc.spec_from_params(L=Lh, N=N, slack_var_constraint_type=slack)
    B = 5
    u_d, y_d, up, yp = _instances(B, N=N, seed0=40)
    with _engine(spec, N, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.solve(up, yp)
    _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))


def test_siso_system_with_padded_rows(gpu):
    # m = p = 1, n = 2, L = 5: r = 14 is not a multiple of 4 -> dummy identity rows, smallest kernels
    A = np.array([[0.9, 0.2], [0.0, 0.7]]); Bm = np.array([[0.0], [1.0]]); C = np.array([[1.0, 0.0]]); D = np.zeros((1, 1))
    plant = dict(A=A, B=Bm, C=C, D=D, eps_max=0.001)
    for Lh, n in ((5, 2), (9, 2), (4, 2)):
        spec = orc.QPSpec(n=n, m=1, p=1, L=Lh, Q=2.0 * np.eye(Lh), R=0.01 * np.eye(Lh), u_s=np.array([0.3]),
                          y_s=np.array([1.0]), robust=True, eps_max=0.001, lamb_alpha=100.0, lamb_sigma=500.0, c=1.0,
                          slack="convex", tec=True)
        B, N = 4, 80
        d = generate_batch(range(B), N=N, plant=plant)
        up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
        with _engine(spec, N, B) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            u, cost, status, _ = eng.solve(up, yp)
        _check(spec, d["u_d"], d["y_d"], up, yp, u, cost, status, range(B))


def test_variables_and_kkt_certificate(gpu):
    # alpha/ubar/ybar/sigma read back from the GPU must themselves satisfy the KKT
    # conditions of the reference's full-space QP (solver-independent check)
    for kw in (dict(), dict(slack_var_constraint_type=1)):
        spec = orc.spec_from_params(**kw)
        B = 3
        u_d, y_d, up, yp = _instances(B, seed0=7)
        with _engine(spec, 400, B) as eng:
            eng.set_data(u_d, y_d)
            eng.solve(up, yp)
            al, ub, yb, sg = (eng.get_solution(k) for k in ("alpha", "ubar", "ybar", "sigma"))
        for b in range(B):
            x = np.concatenate([al[b], ub[b], yb[b], sg[b]])
            cert = orc.kkt_certificate(spec, u_d[b], y_d[b], up[b], yp[b], x, act_tol=1e-12)
            assert cert["res_eq"] < 1e-9 and cert["res_box"] < 1e-15, cert
            assert cert["res_stat"] < 1e-8 * max(1.0, cert["grad_scale"]) and cert["dual_sign"] < 1e-9, cert
            sol = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
            assert np.max(np.abs(al[b] - sol.alpha)) < 1e-9 and np.max(np.abs(sg[b] - sol.sigma)) < 1e-10


def test_bad_instance_gets_status_not_exception(gpu):
    # a constant (non-exciting) trajectory makes G singular: that instance must come back with an error
    # status while its batch neighbours are solved normally
    spec = orc.spec_from_params(controller_type=0)
    B = 4
    u_d, y_d, up, yp = _instances(B)
    u_d = u_d.copy(); y_d = y_d.copy()
    u_d[2] = 1.0; y_d[2] = 0.5
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.solve(up, yp)
    # (the rank-revealing rescue kernel takes the singular instance: a constant trajectory cannot reach the
    #  setpoint, so the QP is infeasible -- the status CVXPY would report)
    assert L.STATUS_STRINGS[int(status[2])] == "infeasible"
    assert [int(s) for s in status[[0, 1, 3]]] == [0, 0, 0]
    assert np.max(np.abs(u[[0, 1, 3]] - 1.0)) < 1e-12


# ----------------------------------------------- full-size, size-independent properties
def test_full_batch_properties(gpu):
    """BASELINE configs[1] size (B = 4096): all optimal; batch-composition independence
    (bit-exact); device-pointer path == host-pointer path (bit-exact); affine dependence
    of optimal_u on the past window for slack NONE."""
    torch = pytest.importorskip("torch")
    spec = orc.spec_from_params()
    B = 4096
    u_d, y_d, up, yp = _instances(B)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        assert np.all(status == 0) and np.all(iters == 1) and np.all(np.isfinite(u)) and np.all(cost > 0)
        _check(spec, u_d, y_d, up, yp, u, cost, status, [0, 1, 2047, 4095])
        # affine in (u_past, y_past)
        rng = np.random.default_rng(0)
        up2 = up + 0.1 * rng.normal(size=up.shape); yp2 = yp + 0.01 * rng.normal(size=yp.shape)
        u2, _, _, _ = eng.solve(up2, yp2)
        um, _, _, _ = eng.solve(0.5 * (up + up2), 0.5 * (yp + yp2))
        assert np.max(np.abs(um - 0.5 * (u + u2))) / np.max(np.abs(u)) < 1e-9
        # device-resident buffers (torch) give the same bits as the host path
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        eng.set_data(t(u_d), t(y_d))
        ud_, cd_, sd_, _ = eng.solve(t(up), t(yp))
        torch.cuda.synchronize()
        assert np.array_equal(ud_.cpu().numpy(), u) and np.array_equal(cd_.cpu().numpy(), cost)
    sub = slice(1000, 1016)
    with _engine(spec, 400, 16) as eng:
        eng.set_data(u_d[sub], y_d[sub])
        us, cs, _, _ = eng.solve(up[sub], yp[sub])
    assert np.array_equal(us, u[sub]) and np.array_equal(cs, cost[sub])


# -------------------------------------------------------- the class mirror (batch = 1)
def _controller(kind="robust", slack="none", seed=0, **over):
    from direct_data_driven_mpc.direct_data_driven_mpc_controller import (
        DataDrivenMPCType, DirectDataDrivenMPCController, SlackVarConstraintTypes)
    cfg = controller_params()
    inst = orc.generate_instance(seed)
    kw = dict(n=cfg["n"], m=cfg["m"], p=cfg["p"], u_d=inst["u_d"], y_d=inst["y_d"], L=cfg["L"],
              Q=cfg["Q"] * np.eye(cfg["p"] * cfg["L"]), R=cfg["R"] * np.eye(cfg["m"] * cfg["L"]),
              u_s=cfg["u_s"].reshape(-1, 1), y_s=cfg["y_s"].reshape(-1, 1), eps_max=cfg["eps_max"],
              lamb_alpha=cfg["lamb_alpha"], lamb_sigma=cfg["lamb_sigma"], c=cfg["c"],
              slack_var_constraint_type={"none": SlackVarConstraintTypes.NONE, "convex": SlackVarConstraintTypes.CONVEX,
                                         "non_convex": SlackVarConstraintTypes.NON_CONVEX}[slack],
              controller_type=DataDrivenMPCType.ROBUST if kind == "robust" else DataDrivenMPCType.NOMINAL,
              n_mpc_step=cfg["n_mpc_step"])
    kw.update(over)
    return DirectDataDrivenMPCController(**kw), inst


def test_controller_class_construct_and_errors(gpu):
    ctrl, inst = _controller()
    assert ctrl.get_problem_solve_status() == "optimal"
    assert ctrl.optimal_u.shape == (60,)
    assert np.allclose(ctrl.get_optimal_control_input_at_step(0), [21.22188171, 20.30350327], atol=5e-9)
    assert abs(ctrl.get_optimal_cost_value() - 4.543214030) < 5e-10
    assert ctrl.HLn_ud.shape == (68, 367) and np.array_equal(ctrl.HLn_yd, orc.hankel_matrix(inst["y_d"], 34))
    assert ctrl.alpha.value.shape == (367, 1) and ctrl.sigma.value.shape == (68, 1)
    assert np.allclose(ctrl.ubar.value[8:, 0], ctrl.optimal_u)
    with pytest.raises(ValueError, match=r"out of range. It should be within \[0, 29\]"):
        ctrl.get_optimal_control_input_at_step(30)
    with pytest.raises(ValueError, match="Incorrect dimensions"):
        ctrl.store_input_output_measurement(np.zeros(2), np.zeros((2, 1)))
    with pytest.raises(ValueError, match="u_past must be shaped"):
        ctrl.set_past_input_output_data(np.zeros((7, 1)), np.zeros((8, 1)))
    with pytest.raises(ValueError, match="u_s must have shape"):
        ctrl.set_input_output_setpoints(np.zeros(2), np.zeros((2, 1)))
    with pytest.raises(NotImplementedError, match="Non-Convex slack variable"):
        _controller(slack="non_convex")
    with pytest.raises(ValueError, match="not persistently exciting"):
        _controller(u_d=np.ones((400, 2)))
    with pytest.raises(ValueError, match="two times the estimated"):
        _controller(L=6, Q=3 * np.eye(12), R=1e-4 * np.eye(12))
    with pytest.raises(ValueError, match="Output weighting square matrix Q"):
        _controller(Q=np.eye(10))
    nom, _ = _controller(kind="nominal")
    assert np.allclose(nom.optimal_u, 1.0, atol=1e-12) and abs(nom.get_optimal_cost_value()) < 1e-12


@pytest.mark.parametrize("slack,n_mpc_step", [("none", 4), ("convex", 1)])
def test_controller_closed_loop_matches_oracle(gpu, slack, n_mpc_step):
    # the loop of utilities/controller/controller_operation.py:259-305 driven through the class
    # mirror on the GPU vs the same loop on the CPU oracle, identical noise
    ctrl, inst = _controller(slack=slack, n_mpc_step=n_mpc_step)
    plant_gpu = orc.Plant(**orc.FOUR_TANK); plant_gpu.x = inst["plant"].x.copy()
    n_steps = 24
    w = plant_gpu.eps_max * inst["rng"].uniform(-1.0, 1.0, (n_steps, 2))
    u_sys = np.zeros((n_steps, 2)); y_sys = np.zeros((n_steps, 2))
    for t in range(0, n_steps, ctrl.n_mpc_step):
        ctrl.update_and_solve_data_driven_mpc()
        for k in range(t, min(t + ctrl.n_mpc_step, n_steps)):
            u_sys[k] = ctrl.get_optimal_control_input_at_step(n_step=k - t)
            y_sys[k] = plant_gpu.step(u_sys[k], w[k])
            ctrl.store_input_output_measurement(u_sys[k].reshape(-1, 1), y_sys[k].reshape(-1, 1))
    spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == "convex" else 0)
    u_ref, y_ref = orc.closed_loop(spec, inst["u_d"], inst["y_d"], inst["plant"], w, n_mpc_step=n_mpc_step)
    assert np.max(np.abs(u_sys - u_ref)) / np.max(np.abs(u_ref)) < 1e-8
    assert np.max(np.abs(y_sys - y_ref)) < 1e-9


# ------------------------------------------------------------ Gram variants, diagnostics
def test_dense_and_structured_gram_agree(gpu):
    # gram_mode DENSE = plain H H' by MFMA (what the reference's Hankel product amounts to);
    # STRUCTURED = Hankel sliding-window recurrence.  Both must match the oracle.
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 12
    u_d, y_d, up, yp = _instances(B, seed0=300)
    res = {}
    for mode in (L.GRAM_DENSE, L.GRAM_STRUCTURED, L.GRAM_AUTO):
        with _engine(spec, 400, B, gram_mode=mode) as eng:
            eng.set_data(u_d, y_d)
            u, cost, status, iters = eng.solve(up, yp)
            f, b = eng.cost_model()
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        res[mode] = (u, cost, iters, f)
    assert np.max(np.abs(res[L.GRAM_DENSE][0] - res[L.GRAM_STRUCTURED][0])) / np.max(np.abs(res[L.GRAM_DENSE][0])) < 1e-10
    assert np.array_equal(res[L.GRAM_AUTO][0], res[L.GRAM_STRUCTURED][0])       # AUTO == STRUCTURED for m+p == 4
    assert np.array_equal(res[L.GRAM_DENSE][2], res[L.GRAM_STRUCTURED][2])
    assert res[L.GRAM_DENSE][3] > 5 * res[L.GRAM_STRUCTURED][3]                 # dense Gram is charged r^2 c flops


def test_repeatable_and_stamps_do_not_perturb(gpu):
    spec = orc.spec_from_params()
    B = 64
    u_d, y_d, up, yp = _instances(B, seed0=900)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u1, c1, _, _ = eng.solve(up, yp)
        u2, c2, _, _ = eng.solve(up, yp)
        assert np.array_equal(u1, u2) and np.array_equal(c1, c2)                 # bit-reproducible
        eng.debug_stamps(True)
        u3, c3, _, _ = eng.solve(up, yp)
        st = eng.debug_stamps(False, fetch=True).astype(np.int64)
        assert np.array_equal(u1, u3) and np.array_equal(c1, c3)
        assert np.all(st[:, 14] > st[:, 0]) and np.all(np.diff(st[:, 0:7], axis=1) > 0)


# -------------------------------------------------------------- other BASELINE configs
@pytest.mark.parametrize("slack", [0, 1])
def test_long_horizon_config4(gpu, slack):
    # BASELINE configs[3]: L=60, N=1000 robust scheme (r = 256 -> the <17,8> kernel instance)
    spec = orc.spec_from_params(L=60, N=1000, slack_var_constraint_type=slack)
    B = 4
    u_d, y_d, up, yp = _instances(B, N=1000, seed0=11)
    with _engine(spec, 1000, B) as eng:
        assert "17,8" in eng.kernel_name()
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        al = eng.get_solution("alpha")
    _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
    assert al.shape == (B, 937)


@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_robust_scheme_beyond_the_register_resident_kernels(gpu, slack):
    # (m+p)(L+n) = 296 rows > 271: ddmpc_large_solve_kernel (matrices in a global workspace), same outputs,
    # status, iteration count and reconstructed variables as the register-resident kernels
    spec = orc.spec_from_params(L=70, N=1200, slack_var_constraint_type=slack)
    B = 3
    u_d, y_d, up, yp = _instances(B, N=1200, seed0=21)
    with _engine(spec, 1200, B) as eng:
        assert "large_solve" in eng.kernel_name()
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        u2, cost2, status2, _ = eng.step(up, yp)                    # no affine law at this size: a step is a solve
        al = eng.get_solution("alpha"); sg = eng.get_solution("sigma"); yb = eng.get_solution("ybar")
        u3, cost3, status3, _ = eng.solve_from_host(u_d, y_d, up, yp)    # plain upload + solve at this size
    _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
    assert np.array_equal(u, u2) and np.array_equal(cost, cost2) and np.array_equal(status, status2)
    assert np.array_equal(u, u3) and np.array_equal(cost, cost3) and np.array_equal(status, status3)
    for b in range(B):
        ref = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        if slack == 1:
            assert int(iters[b]) == ref.iters
        assert np.max(np.abs(sg[b] - ref.sigma.ravel())) <= 1e-9 * max(1.0, np.max(np.abs(ref.sigma)))
        assert np.max(np.abs(yb[b] - ref.ybar.ravel())) <= 1e-9
        assert np.max(np.abs(al[b] - ref.alpha.ravel())) <= 1e-8 * max(1e-3, np.max(np.abs(ref.alpha)))
    if slack == 0:      # beyond what the global-workspace kernels hold (ROBUST: 2048 rows since round 5, tests/test_gpu_round5.py::
        with pytest.raises(L.DDMPCError, match="too large"):      # test_robust_scheme_beyond_1024_rows): reported when the controller is created
            _engine(orc.spec_from_params(L=520, N=2700), 2700, 1)


@pytest.mark.parametrize("pipeline", ["phases", "one_workgroup"])
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_dense_weighting_matrices_beyond_the_register_resident_kernels(gpu, slack, pipeline):
    # dense SPD Q, R (controller.py:121-124,708-710) at 296 rows: lam * W^-1 is added to the whole Gram matrix (rr3_shift_kernel of
    # the phase pipeline since round 5, ddmpc_large_solve_kernel on the one-workgroup pipeline), the slack box still only switches
    # diagonal entries -- the Woodbury updates of the phase pipeline are unchanged --, z = t - lam W^-1 beta is a product with the
    # matrix shared by the batch; outputs and variables against the full-space oracle
    spec = orc.spec_from_params(L=70, N=1200, slack_var_constraint_type=slack)
    rng = np.random.default_rng(12)
    spec.Q = _spd(rng, spec.p * spec.L, 3.0, 3)
    spec.R = _spd(rng, spec.m * spec.L, 1e-4, 2)
    B = 2
    u_d, y_d, up, yp = _instances(B, N=1200, seed0=31)
    with _engine(spec, 1200, B) as eng:
        assert "large_solve" in eng.kernel_name()
        eng.set_large_pipeline(pipeline)
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        sg = eng.get_solution("sigma"); yb = eng.get_solution("ybar"); ub = eng.get_solution("ubar")
        eng.set_data(u_d, y_d)
        uw = eng.step(up, yp)                             # (the solve on the kept factors)
    assert np.array_equal(uw[0], u) and np.array_equal(uw[2], status)
    _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
    for b in range(B):
        ref = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
        if slack == 1:
            assert int(iters[b]) == ref.iters
        assert np.max(np.abs(sg[b] - ref.sigma.ravel())) <= 1e-9 * max(1.0, np.max(np.abs(ref.sigma)))
        assert np.max(np.abs(yb[b] - ref.ybar.ravel())) <= 1e-8
        assert np.max(np.abs(ub[b] - ref.ubar.ravel())) <= 1e-8 * np.max(np.abs(ref.ubar))


def test_convex_active_set_converges_on_full_batch(gpu):
    # slack CONVEX on 4096 seeds: every instance must reach a stable active set ("optimal"),
    # a sample is compared with the full-space oracle, and the bound must hold everywhere
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 4096
    u_d, y_d, up, yp = _instances(B)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        sig = eng.get_solution("sigma")
    assert np.all(status == 0) and iters.min() >= 1 and iters.max() <= 10
    assert np.max(np.abs(sig[:, 8:])) <= spec.c * spec.eps_max * (1 + 1e-12)
    worst = np.argsort(-iters)[:3].tolist()
    _check(spec, u_d, y_d, up, yp, u, cost, status, [0, 1777, 4095] + worst)
    for b in worst:
        assert int(iters[b]) == orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b]).iters


# ------------------------------------------------------ batched closed loop on the device
@pytest.mark.parametrize("kw,n_mpc_step", [(dict(), 4), (dict(slack_var_constraint_type=1), 1), (dict(tec=False), 1)],
                         ids=["tec-nstep4", "tec-convex-1step", "ucon-1step"])
def test_device_closed_loop_matches_oracle(gpu, kw, n_mpc_step):
    # the loop of utilities/controller/controller_operation.py:259-305 for a batch of
    # instances, entirely on the device, vs the same loop on the CPU oracle with identical noise.
    spec = orc.spec_from_params(**kw)
    B, n_steps = 3, 14
    insts = [orc.generate_instance(s) for s in range(B)]
    u_d = np.stack([i["u_d"] for i in insts]); y_d = np.stack([i["y_d"] for i in insts])
    x0 = np.stack([i["plant"].x for i in insts])
    w = np.stack([i["plant"].eps_max * i["rng"].uniform(-1.0, 1.0, (n_steps, 2)) for i in insts])
    up = u_d[:, -4:, :].reshape(B, -1); yp = y_d[:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u_sys, y_sys, status, x_end, up_end, yp_end = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, up, yp, w,
                                                                      n_mpc_step=n_mpc_step)
    assert np.all(status == 0)
    for b in range(B):
        u_ref, y_ref = orc.closed_loop(spec, u_d[b], y_d[b], insts[b]["plant"], w[b], n_mpc_step=n_mpc_step)
        assert np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8
        assert np.max(np.abs(y_sys[b] - y_ref)) < 1e-9
        assert np.max(np.abs(x_end[b] - insts[b]["plant"].x)) < 1e-9           # oracle plant was advanced in place
        assert np.allclose(up_end[b], u_sys[b, -4:].reshape(-1)) and np.allclose(yp_end[b], y_sys[b, -4:].reshape(-1))


def test_device_closed_loop_beyond_the_register_resident_kernels(gpu):
    # the same loop at L = 70 (296 rows): every step is a full solve on ddmpc_large_solve_kernel (slack box on)
    spec = orc.spec_from_params(L=70, N=1200, slack_var_constraint_type=1)
    B, n_steps = 2, 6
    insts = [orc.generate_instance(s, N=1200) for s in range(B)]
    u_d = np.stack([i["u_d"] for i in insts]); y_d = np.stack([i["y_d"] for i in insts])
    x0 = np.stack([i["plant"].x for i in insts])
    w = np.stack([i["plant"].eps_max * i["rng"].uniform(-1.0, 1.0, (n_steps, 2)) for i in insts])
    up = u_d[:, -4:, :].reshape(B, -1); yp = y_d[:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    with _engine(spec, 1200, B) as eng:
        assert "large_solve" in eng.kernel_name()
        eng.set_data(u_d, y_d)
        u_sys, y_sys, status, x_end, _, _ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, up, yp, w, n_mpc_step=2)
    assert np.all(status == 0)
    for b in range(B):
        u_ref, y_ref = orc.closed_loop(spec, u_d[b], y_d[b], insts[b]["plant"], w[b], n_mpc_step=2)
        assert np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8
        assert np.max(np.abs(y_sys[b] - y_ref)) < 1e-9


def test_paper_reproduction_known_answers(gpu):
    # Behavioural known answers of the reference's reproduction script (seed 4, y_0 = [0.4, 0.4],
    # t_sim = 600; examples/robust_data_driven_mpc_reproduction.py:126-295, README figure): TEC and
    # TEC n-step converge to y_s, UCON diverges past |u| = 15 around k = 384.
    inst = orc.generate_instance(4)
    plant, rng = inst["plant"], inst["rng"]
    u_d, y_d = inst["u_d"], inst["y_d"]
    n, n_steps = 4, 600
    y0 = np.array([0.4, 0.4])
    u_eq = plant.equilibrium_input_from_output(y0)
    x_eq = plant.initial_state_from_trajectory(np.tile(u_eq, n), np.tile(y0, n))     # paper_reproduction.py:80-116
    plant.x = x_eq
    U_n = np.tile(np.array([1.0, 1.0]), (n, 1))                                       # controller_operation.py:190-197
    W_n = plant.eps_max * rng.uniform(-1.0, 1.0, (n, 2))
    Y_n = plant.simulate(U_n, W_n)
    x_start = plant.x.copy()
    P = orc.FOUR_TANK
    out = {}
    for tag, kw, step in (("tec", {}, 1), ("tec_n", {}, 4), ("ucon", dict(tec=False), 1)):
        spec = orc.spec_from_params(**kw)
        w = plant.eps_max * rng.uniform(-1.0, 1.0, (n_steps - n, 2))                  # drawn per controller, in order
        with _engine(spec, 400, 1) as eng:
            eng.set_data(u_d[None], y_d[None])
            u_sys, y_sys, status, *_ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x_start[None], U_n.reshape(1, -1),
                                                       Y_n.reshape(1, -1), w[None], n_mpc_step=step)
        assert status[0] == 0
        out[tag] = (u_sys[0], y_sys[0])
    assert np.allclose(out["tec"][0][0], [8.6604991, 8.53323249], atol=2e-7)
    assert np.allclose(out["tec_n"][0][0], [8.6604991, 8.53323249], atol=2e-7)
    assert np.allclose(out["ucon"][0][0], [7.89630434, 9.2946719], atol=2e-7)
    assert np.all(np.abs(out["tec"][1][-1] - [0.65, 0.77]) < 0.02) and np.all(np.abs(out["tec_n"][1][-1] - [0.65, 0.77]) < 0.02)
    big = np.nonzero(np.max(np.abs(out["ucon"][0]), axis=1) > 15.0)[0]
    assert big.size > 0 and abs(int(big[0]) + n - 384) <= 2          # k counted from the start of the n warm-up steps


def test_device_closed_loop_full_batch_converges(gpu):
    # 512 instances x 201 steps (n-step scheme, 51 solves each) entirely on the device: every
    # instance must settle near the setpoint (y -> (0.65, 0.77), u -> (1, 1))
    spec = orc.spec_from_params()
    B, n_steps = 512, 201
    d = generate_batch(range(B))
    rng = np.random.default_rng(123)
    w = 0.002 * rng.uniform(-1.0, 1.0, (B, n_steps, 2))
    up = d["u_d"][:, -4:, :].reshape(B, -1); yp = d["y_d"][:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u_sys, y_sys, status, *_ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=4)
    assert np.all(status == 0) and np.all(np.isfinite(u_sys))
    assert np.max(np.abs(y_sys[:, -1] - spec.y_s)) < 0.05 and np.max(np.abs(u_sys[:, -1] - spec.u_s)) < 0.5


def test_batched_persistent_excitation_guard(gpu, golden):
    spec = orc.spec_from_params()
    B = 6
    u_d, y_d, up, yp = _instances(B)
    u_bad = u_d.copy(); u_bad[3] = 1.0                       # constant input: not persistently exciting
    with _engine(spec, 400, B) as eng:
        ranks = eng.persistent_excitation_ranks(u_bad)
    assert ranks.tolist() == [76, 76, 76, int(golden["const_pe_rank"][0]), 76, 76]


# --------------------------------------------------- warm path: ddmpc_prepare / ddmpc_step
@pytest.mark.parametrize("kw,N", [(dict(), 400), (dict(tec=False), 400), (dict(controller_type=0), 400),
                                  (dict(L=10, N=120), 120), (dict(L=60, N=1000), 1000)],
                         ids=["robust-none-tec", "robust-none-ucon", "nominal", "small", "config4"])
def test_warm_step_matches_oracle(gpu, kw, N):
    # SURVEY 8(d) "warm" step: per step only u_past / y_past change (controller.py:404-407,577-581), so
    # the engine evaluates the affine law prepared once per data set.  Same tolerances as a cold solve.
    spec = orc.spec_from_params(**kw)
    B = 6
    u_d, y_d, up, yp = _instances(B, N=N, seed0=60)
    rng = np.random.default_rng(17)
    with _engine(spec, N, B) as eng:
        eng.set_data(u_d, y_d)
        eng.prepare()
        for trial in range(3):
            if trial:
                up = rng.uniform(-1.0, 1.0, up.shape); yp = rng.uniform(0.0, 1.0, yp.shape)
            u, cost, status, iters = eng.step(up, yp)
            assert np.all(iters == 1)
            if spec.robust:
                _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
            else:                      # nominal with full-row-rank H: u = u_s, cost = 0 (analytic known answer)
                assert np.all(status == 0) and np.max(np.abs(u - np.tile(spec.u_s, spec.L))) < 1e-9
                assert np.max(np.abs(cost)) < 1e-12
            uc, cc, sc, _ = eng.solve(up, yp)
            assert np.max(np.abs(u - uc)) / np.max(np.abs(uc)) < 1e-10 and np.array_equal(status, sc)
        if spec.robust:
            u, cost, status, _ = eng.step(up, yp)          # variables read back after a WARM step
            al, sg, ub, yb = (eng.get_solution(k) for k in ("alpha", "sigma", "ubar", "ybar"))
            sol = orc.solve_fullspace(spec, u_d[1], y_d[1], up[1], yp[1])
            assert np.max(np.abs(al[1] - sol.alpha)) < 1e-9 and np.max(np.abs(sg[1] - sol.sigma)) < 1e-10
            assert np.max(np.abs(ub[1] - sol.ubar.ravel())) / np.max(np.abs(sol.ubar)) < 1e-8
            assert np.max(np.abs(yb[1] - sol.ybar.ravel())) < 1e-8


def test_warm_step_affine_law_full_batch(gpu):
    # size-independent property at the full BASELINE batch: the warm step is affine in the past window,
    # and the exported gain reproduces it.  4096 instances.
    spec = orc.spec_from_params()
    B = 4096
    u_d, y_d, up, yp = _instances(B)
    rng = np.random.default_rng(3)
    p1 = np.concatenate([up, yp], axis=1); p2 = rng.uniform(-1.0, 1.0, p1.shape)
    a = 0.3
    pm = a * p1 + (1 - a) * p2
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        r1 = eng.step(p1[:, :8].copy(), p1[:, 8:].copy()); r1 = [x.copy() for x in r1]
        r2 = eng.step(p2[:, :8].copy(), p2[:, 8:].copy()); r2 = [x.copy() for x in r2]
        rm = eng.step(pm[:, :8].copy(), pm[:, 8:].copy())
        uc, cc, sc, _ = eng.solve(up, yp)
        gain = eng.gain()
    assert np.all(rm[2] == 0) and np.all(sc == 0)
    scale = np.max(np.abs(r1[0])) + np.max(np.abs(r2[0]))
    assert np.max(np.abs(rm[0] - (a * r1[0] + (1 - a) * r2[0]))) / scale < 1e-10
    assert np.max(np.abs(r1[0] - uc)) / np.max(np.abs(uc)) < 1e-10            # warm == cold on all 4096
    assert np.max(np.abs(r1[1] - cc) / cc) < 1e-9
    # gain: beta = g0 + G' p; optimal_u rows are z = u_s - lam/r * beta on the free input components
    assert gain.shape == (B, 17, 136)
    beta = gain[:, 0, :] + np.einsum("bfr,bf->br", gain[:, 1:, :], p1)
    lam = spec.lamb_alpha * spec.eps_max
    rows = np.array([(4 + k) * 4 + ch for k in range(spec.L - 4) for ch in range(2)])     # free ubar components
    z = np.tile(spec.u_s, spec.L - 4)[None] - lam / spec.R[0, 0] * beta[:, rows]
    assert np.max(np.abs(z - r1[0][:, : 2 * (spec.L - 4)])) / np.max(np.abs(z)) < 1e-10


def test_warm_step_with_slack_box(gpu):
    # slack CONVEX: the affine law is the first active-set iterate; instances it keeps inside the box are
    # final (iters 1), the rest are re-solved cold inside the same ddmpc_step call -> same results as ddmpc_solve
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 64
    u_d, y_d, up, yp = _instances(B, seed0=5)
    rng = np.random.default_rng(2)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        eng.prepare()
        seen = set()
        for trial in range(3):
            if trial == 1:      # windows near the setpoint: the box is mostly inactive
                up = np.tile(spec.u_s, 4)[None] + 0.01 * rng.uniform(-1, 1, up.shape)
                yp = np.tile(spec.y_s, 4)[None] + 0.002 * rng.uniform(-1, 1, yp.shape)
            if trial == 2:
                up = rng.uniform(-1.0, 1.0, up.shape); yp = rng.uniform(0.0, 1.0, yp.shape)
            uw, cw, sw, iw = (x.copy() for x in eng.step(up, yp))
            sg = eng.get_solution("sigma")
            uc, cc, sc, ic = eng.solve(up, yp)
            assert np.array_equal(iw, ic) and np.array_equal(sw, sc)
            assert np.max(np.abs(uw - uc)) / np.max(np.abs(uc)) < 1e-10 and np.max(np.abs(cw - cc) / np.abs(cc)) < 1e-10
            assert np.max(np.abs(sg[:, 8:])) <= spec.c * spec.eps_max * (1 + 1e-12)
            _check(spec, u_d, y_d, up, yp, uw, cw, sw, range(0, B, 7))
            seen |= set(int(i) for i in iw)
        assert 1 in seen and max(seen) >= 2                     # both the warm-only and the re-solved branch ran
        g = eng.gain()                                          # the law of the empty active set
        assert g.shape == (B, 17, 136)
        eng.set_closed_loop_path("warm")


def test_warm_path_invalidation_and_bad_instance(gpu):
    # new setpoints / new data invalidate the prepared law; a singular instance keeps its error status
    spec = orc.spec_from_params()
    B = 4
    u_d, y_d, up, yp = _instances(B, seed0=21)
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.step(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        spec.u_s = np.array([0.8, 1.1]); spec.y_s = np.array([0.5, 0.9])
        eng.set_setpoints(spec.u_s, spec.y_s)
        u, cost, status, _ = eng.step(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        u_d2, y_d2, up2, yp2 = _instances(B, seed0=33)
        eng.set_data(u_d2, y_d2)
        u, cost, status, _ = eng.step(up2, yp2)
        _check(spec, u_d2, y_d2, up2, yp2, u, cost, status, range(B))
    specn = orc.spec_from_params(controller_type=0)
    u_d = u_d.copy(); y_d = y_d.copy(); u_d[2] = 1.0; y_d[2] = 0.5       # constant data: singular Gram
    with _engine(specn, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, _ = eng.step(up, yp)
    assert L.STATUS_STRINGS[int(status[2])] == "infeasible" and [int(s) for s in status[[0, 1, 3]]] == [0, 0, 0]


@pytest.mark.parametrize("kw,n_mpc_step", [(dict(), 1), (dict(), 4), (dict(tec=False), 1), (dict(controller_type=0), 2),
                                           (dict(slack_var_constraint_type=1), 1), (dict(slack_var_constraint_type=1), 3)],
                         ids=["tec-1step", "tec-nstep4", "ucon-1step", "nominal-2step", "convex-1step", "convex-3step"])
def test_closed_loop_warm_and_cold_paths_agree(gpu, kw, n_mpc_step):
    # the fused one-workgroup-per-instance loop (affine law) vs one cold solve per control step
    spec = orc.spec_from_params(**kw)
    B, n_steps = 16, 61
    d = generate_batch(range(70, 70 + B))
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B, n_steps, 2))
    up = d["u_d"][:, -4:, :].reshape(B, -1); yp = d["y_d"][:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    out = {}
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        for path in ("cold", "warm", "auto"):
            eng.set_closed_loop_path(path)
            out[path] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
    for a, b in zip(out["cold"], out["warm"]):
        assert np.max(np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float))) < 1e-9
    for a, b in zip(out["warm"], out["auto"]):
        assert np.array_equal(a, b)                            # AUTO picks the warm path here
    assert np.all(out["warm"][2] == 0)
    # what ddmpc_get_solution reads after the fused loop is the loop's own, whatever a ddmpc_step before it left
    convex = kw.get("slack_var_constraint_type") == 1
    sol = []
    for step_first in (False, True):
        with _engine(spec, 400, B) as eng:
            if convex:
                eng.set_convex_warm_law(True)                  # (the fused loop under the slack box)
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_closed_loop_path("warm")
            if step_first:
                eng.step(up, yp)
            eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step)
            sol.append([eng.get_solution(k) for k in ("alpha", "ubar", "ybar")])
    assert all(np.array_equal(a, b) for a, b in zip(*sol))


# ----------------------------------------------------- device persistent-excitation guard
def test_device_pe_guard_certifies_and_defers(gpu, golden):
    # SURVEY 8(f)-4.  Random four-tank input data is certified on the device (rank 76 for seeds 0-4 in
    # the reference); degenerate data is never certified and gets the reference's exact SVD verdict.
    spec = orc.spec_from_params()
    B = 64
    u_d, y_d, up, yp = _instances(B)
    order, full = spec.L + 2 * spec.n, spec.m * (spec.L + 2 * spec.n)
    ratio = np.empty((B,))
    lib = L.load()
    import ctypes as C
    L.check(lib.ddmpc_pe_guard(C.c_void_p(u_d.ctypes.data), B, 400, 2, order, C.c_void_p(ratio.ctypes.data), L.MEM_HOST, 0))
    # the bound really is a lower bound of sigma_min/sigma_max, and not uselessly loose (factor <= r)
    for b in range(8):
        s = np.linalg.svd(orc.hankel_matrix(u_d[b], order), compute_uv=False)
        assert ratio[b] <= s[-1] / s[0] * (1 + 1e-9) and ratio[b] >= s[-1] / s[0] / full
    assert np.all(ratio > 1e-4)
    u_bad = u_d.copy()
    u_bad[3] = 1.0                                                      # constant: rank m
    t = np.arange(400)
    u_bad[5] = np.stack([np.sin(0.3 * t), np.cos(0.3 * t)], axis=1)     # one sinusoid per channel: rank 4
    u_bad[7] = u_d[7] * 1e-9 + 1.0                                      # nearly constant but still exciting
    with _engine(spec, 400, B) as eng:
        ok, rank = eng.persistent_excitation_guard(u_bad)
        ranks_svd = eng.persistent_excitation_ranks(u_bad[:10])
    assert rank[:10].tolist() == ranks_svd.tolist()                    # identical to the all-SVD path
    assert int(rank[3]) == int(golden["const_pe_rank"][0]) and not ok[3] and not ok[5] and rank[5] < full
    good = np.ones(B, dtype=bool); good[[3, 5]] = False
    assert np.all(ok[good]) and np.all(rank[good] == full)
    # the size of BASELINE configs[4] (m = 8, order L + 2n = 46: 368 rows): the packed matrix no longer fits LDS
    # and goes to a global workspace; same guarantee (lower bound, not uselessly loose)
    big = np.random.default_rng(8).uniform(-1.0, 1.0, (3, 2000, 8))
    rb = np.empty((3,))
    L.check(lib.ddmpc_pe_guard(C.c_void_p(big.ctypes.data), 3, 2000, 8, 46, C.c_void_p(rb.ctypes.data), L.MEM_HOST, 0))
    for b in range(3):
        s = np.linalg.svd(orc.hankel_matrix(big[b], 46), compute_uv=False)
        assert rb[b] <= s[-1] / s[0] * (1 + 1e-9) and rb[b] >= s[-1] / s[0] / 368 and rb[b] > 1e-4


def test_device_pe_guard_full_batch(gpu):
    B = 4096
    u_d, y_d, up, yp = _instances(B)
    spec = orc.spec_from_params()
    with _engine(spec, 400, B) as eng:
        ok, rank = eng.persistent_excitation_guard(u_d)
    assert np.all(ok) and np.all(rank == 76)


# ------------------------------------------------------------- example flow
def test_batched_example_script(gpu, tmp_path):
    # the reference example's flow (YAML configs -> data -> controller -> closed loop) for a batch, with
    # the reference's per-step line format for instance 0 (controller_operation.py:327-329)
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "loop.npz"
    res = subprocess.run([sys.executable, os.path.join(root, "examples", "batched_data_driven_mpc_example.py"),
                          "--batch", "8", "--t_sim", "40", "--seed", "0", "--verbose", "2", "--out", str(out)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("    Time step:")]
    # one line per solve (n_mpc_step = n = 4: t = 0, 4, ..., 40), as controller_operation.py:310-329 prints them
    assert len(lines) == 11 and "MPC cost value:" in lines[0] and "u_1e =" in lines[0] and "y_2e =" in lines[0]
    z = np.load(out)
    assert z["u_sys"].shape == (8, 41, 2) and np.all(z["status"] == 0)
    # instance 0 is the reference example with --seed 0: same closed loop as the oracle (n-step scheme, n = 4)
    inst = orc.generate_instance(0)
    w = inst["plant"].eps_max * inst["rng"].uniform(-1.0, 1.0, (41, 2))
    u_ref, y_ref = orc.closed_loop(orc.spec_from_params(), inst["u_d"], inst["y_d"], inst["plant"], w, n_mpc_step=4)
    assert np.max(np.abs(z["u_sys"][0] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8
    assert np.max(np.abs(z["y_sys"][0] - y_ref)) < 1e-9
    res = subprocess.run([sys.executable, os.path.join(root, "examples", "batched_data_driven_mpc_example.py"),
                          "--batch", "2", "--slack_var_const_type", "NonConvex"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "not currently implemented" in res.stderr


# -------------------------------------------------- dense weighting matrices (a12)
def _spd(rng, size, scale, blocks):
    # block-banded SPD matrix: couples neighbouring prediction steps and channels
    A = rng.normal(size=(size, size)) * 0.2
    W = A @ A.T / size + np.eye(size)
    band = np.abs(np.subtract.outer(np.arange(size), np.arange(size))) <= blocks
    return scale * (W * band + np.diag(np.abs(W * ~band).sum(axis=1)))        # diagonally dominant -> SPD


@pytest.mark.parametrize("kw", [dict(), dict(tec=False), dict(L=10, N=120)], ids=["tec", "ucon", "small"])
def test_dense_weighting_matrices(gpu, kw):
    # the class accepts any Q (pL x pL), R (mL x mL) (controller.py:121-124,327-343,708-710); the loader
    # only builds q*I, r*I.  Dense SPD weights: cold solve, warm step, variables, closed loop vs the oracle.
    spec = orc.spec_from_params(**kw)
    rng = np.random.default_rng(11)
    spec.Q = _spd(rng, spec.p * spec.L, 3.0, 3)
    spec.R = _spd(rng, spec.m * spec.L, 1e-4, 2)
    N = kw.get("N", 400)
    B = 5
    u_d, y_d, up, yp = _instances(B, N=N, seed0=90)
    with _engine(spec, N, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        al, sg, ub, yb = (eng.get_solution(k) for k in ("alpha", "sigma", "ubar", "ybar"))
        sol = orc.solve_fullspace(spec, u_d[2], y_d[2], up[2], yp[2])
        assert np.max(np.abs(al[2] - sol.alpha)) < 1e-9 and np.max(np.abs(sg[2] - sol.sigma)) < 1e-10
        assert np.max(np.abs(ub[2] - sol.ubar.ravel())) / np.max(np.abs(sol.ubar)) < 1e-8
        assert np.max(np.abs(yb[2] - sol.ybar.ravel())) < 1e-8
        up2 = rng.uniform(-1.0, 1.0, up.shape); yp2 = rng.uniform(0.0, 1.0, yp.shape)
        uw, cw, sw, _ = eng.step(up2, yp2)                         # warm step with dense weights
        _check(spec, u_d, y_d, up2, yp2, uw, cw, sw, range(B))
    if not kw:
        insts = [orc.generate_instance(s) for s in range(2)]
        ud = np.stack([i["u_d"] for i in insts]); yd = np.stack([i["y_d"] for i in insts])
        x0 = np.stack([i["plant"].x for i in insts]); n_steps = 10
        w = np.stack([i["plant"].eps_max * i["rng"].uniform(-1.0, 1.0, (n_steps, 2)) for i in insts])
        P = orc.FOUR_TANK
        with _engine(spec, 400, 2) as eng:
            eng.set_data(ud, yd)
            u_sys, y_sys, st, *_ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, ud[:, -4:].reshape(2, -1),
                                                   yd[:, -4:].reshape(2, -1), w, n_mpc_step=2)
        for b in range(2):
            u_ref, y_ref = orc.closed_loop(spec, ud[b], yd[b], insts[b]["plant"], w[b], n_mpc_step=2)
            assert np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8 and np.max(np.abs(y_sys[b] - y_ref)) < 1e-9


def test_dense_weights_rejections(gpu):
    spec = orc.spec_from_params()
    Q = spec.Q.copy(); Q[0, 1] = 0.5                                 # not symmetric
    spec.Q = Q
    with pytest.raises(L.DDMPCError, match="symmetric"):
        _engine(spec, 400, 1)
    spec = orc.spec_from_params()
    Q = spec.Q.copy(); Q[0, 1] = Q[1, 0] = 10.0                      # symmetric but indefinite
    spec.Q = Q
    with pytest.raises(L.DDMPCError, match="positive definite"):
        _engine(spec, 400, 1)
    spec = orc.spec_from_params()
    spec.R = spec.R.copy(); spec.R[3, 3] = -1e-4                     # diagonal, not PSD
    with pytest.raises(L.DDMPCError, match="semi-definite"):
        _engine(spec, 400, 1)


@pytest.mark.parametrize("kw", [dict(), dict(tec=False), dict(L=10, N=120)], ids=["tec", "ucon", "small"])
def test_dense_weighting_matrices_with_the_slack_box(gpu, kw):
    # Dense SPD Q / R together with the CONVEX slack box -- the constructor's DEFAULT slack type (controller.py:111-112)
    # with the weights of controller.py:708-710.  A sigma at its bound only switches the diagonal 1/lamb_sigma term of
    # W^-1 = Q_ff^-1 + P_I / lamb_sigma, so the dense part is shared by every active set.  Cold solve, variables, warm
    # step (affine iterate + cold re-solve of flagged instances) and a short closed loop against the full-space oracle.
    spec = orc.spec_from_params(slack_var_constraint_type=1, **kw)
    rng = np.random.default_rng(12)
    spec.Q = _spd(rng, spec.p * spec.L, 3.0, 3)
    spec.R = _spd(rng, spec.m * spec.L, 1e-4, 2)
    N = kw.get("N", 400)
    B = 6
    u_d, y_d, up, yp = _instances(B, N=N, seed0=40)
    with _engine(spec, N, B) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        sols = [orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b]) for b in range(B)]
        assert [int(i) for i in iters] == [s_.iters for s_ in sols] and max(s_.iters for s_ in sols) >= 2   # the box binds
        sg, yb, al = eng.get_solution("sigma"), eng.get_solution("ybar"), eng.get_solution("alpha")
        for b in range(B):
            assert np.max(np.abs(sg[b] - sols[b].sigma)) < 1e-10 and np.max(np.abs(yb[b] - sols[b].ybar.ravel())) < 1e-8
            assert np.max(np.abs(al[b] - sols[b].alpha)) < 1e-9
        assert np.max(np.abs(sg[:, spec.n * spec.p:])) <= spec.c * spec.eps_max * (1 + 1e-12)
        uw, cw, sw, iw = eng.step(up, yp)
        _check(spec, u_d, y_d, up, yp, uw, cw, sw, range(B))
        assert np.array_equal(iw, iters)
    if not kw:
        insts = [orc.generate_instance(s_) for s_ in range(2)]
        ud = np.stack([i["u_d"] for i in insts]); yd = np.stack([i["y_d"] for i in insts])
        x0 = np.stack([i["plant"].x for i in insts]); n_steps = 8
        w = np.stack([i["plant"].eps_max * i["rng"].uniform(-1.0, 1.0, (n_steps, 2)) for i in insts])
        P = orc.FOUR_TANK
        with _engine(spec, 400, 2) as eng:
            eng.set_data(ud, yd)
            u_sys, y_sys, st, *_ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, ud[:, -4:].reshape(2, -1),
                                                   yd[:, -4:].reshape(2, -1), w, n_mpc_step=1)
        for b in range(2):
            u_ref, y_ref = orc.closed_loop(spec, ud[b], yd[b], insts[b]["plant"], w[b], n_mpc_step=1)
            assert np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8 and np.max(np.abs(y_sys[b] - y_ref)) < 1e-9


@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_positive_semidefinite_diagonal_weights(gpu, slack):
    # Q, R only positive SEMI-definite (controller.py:708-710 takes any PSD matrix): the second output is not weighted
    # at all, every third input step neither.  Unweighted components are free: multiplier zero, z = (G beta).
    spec = orc.spec_from_params(slack_var_constraint_type=slack)
    q = np.diag(spec.Q).copy(); r_ = np.diag(spec.R).copy()
    q[1::2] = 0.0
    r_[::3] = 0.0
    spec.Q, spec.R = np.diag(q), np.diag(r_)
    B = 6
    u_d, y_d, up, yp = _instances(B, seed0=60)
    with _engine(spec, 400, B, diag=True) as eng:
        eng.set_data(u_d, y_d)
        u, cost, status, iters = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
        uw, cw, sw, _ = eng.step(up, yp)
        _check(spec, u_d, y_d, up, yp, uw, cw, sw, range(B))
        sol = orc.solve_fullspace(spec, u_d[0], y_d[0], up[0], yp[0])
        yb = eng.get_solution("ybar")
        assert np.max(np.abs(yb[0] - sol.ybar.ravel())) < 1e-8


def test_long_data_trajectory(gpu):
    # N = 2000 (the data length of BASELINE configs[4]) with the four-tank horizon: c = 1967 Hankel columns,
    # 86 KB of LDS per workgroup (one workgroup per CU), ragged last k-steps of the lag-block loop
    for N, slack in ((2000, 0), (1501, 1)):
        spec = orc.spec_from_params(N=N, slack_var_constraint_type=slack)
        B = 3
        u_d, y_d, up, yp = _instances(B, N=N, seed0=77)
        with _engine(spec, N, B) as eng:
            eng.set_data(u_d, y_d)
            u, cost, status, _ = eng.solve(up, yp)
            _check(spec, u_d, y_d, up, yp, u, cost, status, range(B))
            if slack == 0:
                uw, cw, sw, _ = eng.step(up, yp)
                _check(spec, u_d, y_d, up, yp, uw, cw, sw, range(B))
    # (a trajectory that cannot be staged in LDS was refused at create time until round 4; since round 5 it is solved through a
    #  streaming Gram launch: tests/test_gpu_round5.py::test_trajectories_beyond_the_lds)


# ------------------------------------------------------------- randomized systems
def _random_plant(rng, ns, m, p, eps):
    A = rng.normal(size=(ns, ns))
    A *= 0.85 / max(abs(np.linalg.eigvals(A)))                      # stable, spectral radius 0.85
    return dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=eps)


@pytest.mark.parametrize("refine", ["auto", "always"])
@pytest.mark.parametrize("case", range(12))
def test_random_systems_against_oracle(gpu, case, refine):
    # seeded sweep over plant sizes (m + p != 4 takes the dense-MFMA Gram), horizons that land on every kernel
    # instance, both schemes, all slack / terminal-constraint modes and scalar / diagonal / dense weights
    rng = np.random.default_rng(1000 + case)
    m, p = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 3)][case % 6]
    ns = int(rng.integers(2, 5))
    n = ns
    robust = case % 4 != 3
    Lh = int(rng.integers(2 * n, 2 * n + 9))
    if (m + p) * (Lh + n) > 200:
        Lh = max(2 * n, 200 // (m + p) - n)
    # comfortably above N_min of controller.py:275: with barely enough columns H is nearly rank-deficient
    # (cond(H) ~ 5e5 was seen) and the Gram formulation, which squares it, drops to ~3e-9 in the cost
    N = (m + 1) * (Lh + 2 * n) + int(rng.integers(80, 200))
    eps = 0.002
    slack = "convex" if (robust and case % 3 == 1) else "none"
    tec = case % 5 != 4
    wkind = case % 3 if slack == "none" else case % 2                # dense weights only without the box
    if wkind == 0:
        Q = 2.0 * np.eye(p * Lh); R = 0.05 * np.eye(m * Lh)
    elif wkind == 1:
        Q = np.diag(rng.uniform(1.0, 4.0, p * Lh)); R = np.diag(rng.uniform(0.01, 0.1, m * Lh))
    else:
        Q = _spd(rng, p * Lh, 2.0, 2); R = _spd(rng, m * Lh, 0.05, 2)
    plant = _random_plant(rng, ns, m, p, eps)
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=Q, R=R, u_s=rng.uniform(-0.5, 0.5, m), y_s=rng.uniform(-0.5, 0.5, p),
                      robust=robust, eps_max=eps, lamb_alpha=20.0, lamb_sigma=500.0, c=1.0, slack=slack, tec=tec)
    B = 3
    d = generate_batch(range(case * 10, case * 10 + B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with _engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        # Random plants have output gains of order 1-10 against a noise level of 0.002, so the y rows of H are nearly
        # dependent on its u rows: cond(H) reaches 1e5-5e6 (four-tank data: ~1.3e3) and the Gram route, which squares
        # it, is good to 1e-9..1e-7 only.  With iterative refinement (residual through two exact products with the
        # implicit Hankel matrix) the kernels meet the standard bars -- in the shipped default (AUTO: every solve is checked
        # with that residual and only the instances above the threshold are refined) as well as with refinement ALWAYS.
        eng.set_refinement(refine)
        u, cost, status, iters = eng.solve(up, yp)
        uw, cw, sw, iw = eng.step(up, yp)
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(status[b])] == sol.status == "optimal"
        scale = max(np.max(np.abs(sol.optimal_u)), 1e-3)
        if robust:
            assert np.max(np.abs(u[b] - sol.optimal_u)) / scale < TOL_U, (case, b)
            assert abs(cost[b] - sol.cost) <= TOL_COST * max(abs(sol.cost), 1e-6), (case, b)
        else:
            # nominal scheme on noisy (full-row-rank) data: every trajectory is reachable, so the optimum is the setpoint
            # itself -- u = tile(u_s), cost 0 -- which the kernel returns exactly.  The full-space oracle solves a singular
            # KKT system by truncated least squares and is the LESS accurate side here (up to 2e-7 on these plants):
            us_t = np.tile(spec.u_s, Lh)
            assert np.max(np.abs(u[b] - us_t)) <= 1e-12 * scale and abs(cost[b]) <= 1e-12, (case, b)
            # (3.3e-6 on case 279 of the extended sweep, tools/small_fuzz.py, cond(H) = 3e6)
            assert np.max(np.abs(sol.optimal_u - us_t)) / scale < 1e-5 and abs(sol.cost) < 1e-8, (case, b)
        if spec.slack == "convex" and int(iters[b]) != sol.iters:
            # The primal-dual active-set path is a sequence of sign tests on intermediate iterates; where one of them sits at the
            # bound to rounding, the full-space and the reduced formulation -- both restatements of the same algorithm -- take
            # paths of different length to the same solution (cases 172, 298, 370 of the extended sweep: 3 against 4 iterations on
            # one instance each; every kernel variant agrees with the reduced form there).  Either oracle's count is accepted.
            from oracle.reduced_form import solve_reduced
            assert int(iters[b]) == solve_reduced(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])["iters"], (case, b, int(iters[b]), sol.iters)
    # the affine law of the warm step is formed from refining solves too (ddmpc_prepare; AUTO: for the instances its
    # factor-export launch flags): the warm step meets the cold solve at the same bar
    assert np.max(np.abs(uw - u)) <= TOL_U * max(np.max(np.abs(u)), 1e-3) and np.array_equal(sw, status) and np.array_equal(iw, iters)


def test_noise_free_data(gpu):
    # Exact LTI data: H has rank m(L+n) + n_sys = 72 of 136, the Gram matrix is singular.
    # Robust scheme: G + lam*D stays positive definite (D > 0 on every y component, the hard u rows are
    # independent for persistently exciting inputs) -> same parity as with noisy data.
    # Nominal scheme: the fast path breaks down and the rank-revealing rescue kernel takes over; with the example's
    # rounded setpoint it must report "infeasible" (see test_nominal_scheme_on_exact_data_rank_revealing), never a
    # silently wrong "optimal".
    from direct_data_driven_mpc_amd.harness import FOUR_TANK
    plant = dict(FOUR_TANK); plant["eps_max"] = 0.0
    B = 6
    d = generate_batch(range(B), N=400, plant=plant)
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    for kw in (dict(), dict(slack_var_constraint_type=1)):
        spec = orc.spec_from_params(**kw)
        with _engine(spec, 400, B) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            u, cost, status, _ = eng.solve(up, yp)
            uw, cw, sw, _ = eng.step(up, yp)
        _check(spec, d["u_d"], d["y_d"], up, yp, u, cost, status, range(B))
        assert np.max(np.abs(uw - u)) / np.max(np.abs(u)) < 1e-9
    spec = orc.spec_from_params(controller_type=0)
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = eng.solve(up, yp)
        uw, cw, sw, _ = eng.step(up, yp)
    # (rounded setpoint: the terminal equality is infeasible for exact data, which the rescue kernel detects)
    assert all(L.STATUS_STRINGS[int(s)] == "infeasible" for s in status) and np.array_equal(sw, status)


def test_closed_loop_graph_replay_matches_direct_launches(gpu):
    # the per-step paths (slack box: warm + filtered cold + plant; forced cold: cold + plant) are recorded into a
    # HIP graph and replayed; results must be identical to launching the same kernels one by one.  The last case is a
    # trajectory beyond the LDS (slack box, AUTO refinement, as in test_trajectories_beyond_the_lds): the streamed residual
    # check of its filtered cold launches needs its buffers and the Hankel kernel's LDS limit before the capture starts
    B, n_steps = 32, 45
    w = 0.002 * np.random.default_rng(4).uniform(-1.0, 1.0, (B, n_steps, 2))
    P = orc.FOUR_TANK
    for kw, path, N in ((dict(slack_var_constraint_type=1), "auto", 400), (dict(), "cold", 400),
                        (dict(slack_var_constraint_type=1), "auto", 6000)):
        d = generate_batch(range(200, 200 + B), N=N)
        up = d["u_d"][:, -4:, :].reshape(B, -1); yp = d["y_d"][:, -4:, :].reshape(B, -1)
        spec = orc.spec_from_params(**kw)
        out = {}
        with _engine(spec, N, B) as eng:
            eng.set_data(d["u_d"], d["y_d"])
            eng.set_closed_loop_path(path)
            for graph in (True, False):
                eng.set_closed_loop_graph(graph)
                out[graph] = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=2)
        for a, b in zip(out[True], out[False]):
            assert np.array_equal(a, b)
        assert np.all(out[True][2] == 0)


def test_api_misuse_is_reported_not_crashing(gpu):
    # error behaviour of the C ABI: every misuse returns a code and a message, nothing is launched
    import ctypes as C
    spec = orc.spec_from_params()
    B = 2
    u_d, y_d, up, yp = _instances(B)
    lib = L.load()
    with _engine(spec, 400, B) as eng:
        h = eng._h
        vp = lambda a: C.c_void_p(a.ctypes.data)
        u = np.empty((B, 60)); cost = np.empty(B); st = np.empty(B, np.int32)
        assert lib.ddmpc_solve(h, vp(up), vp(yp), vp(u), vp(cost), vp(st), C.c_void_p(), L.MEM_HOST) == L.ERR_NOT_READY
        assert "ddmpc_set_data" in L.last_error()
        assert lib.ddmpc_step(h, vp(up), vp(yp), vp(u), vp(cost), vp(st), C.c_void_p(), L.MEM_HOST) == L.ERR_NOT_READY
        assert lib.ddmpc_prepare(h) == L.ERR_NOT_READY
        eng.set_data(u_d, y_d)
        out = np.empty((B, 367))
        assert lib.ddmpc_get_solution(h, L.SOL_ALPHA, vp(out), L.MEM_HOST) == L.ERR_NOT_READY
        g = np.empty((B, 17, 136))
        assert lib.ddmpc_get_gain(h, vp(g), L.MEM_HOST) == L.ERR_NOT_READY
        assert lib.ddmpc_solve(h, C.c_void_p(), vp(yp), vp(u), vp(cost), vp(st), C.c_void_p(), L.MEM_HOST) == L.ERR_INVALID
        assert lib.ddmpc_solve(h, vp(up), vp(yp), vp(u), vp(cost), vp(st), C.c_void_p(), 7) == L.ERR_INVALID
        assert lib.ddmpc_set_option(h, 99, 0) == L.ERR_INVALID
        assert lib.ddmpc_set_option(h, L.OPT_CLOSED_LOOP_PATH, 5) == L.ERR_INVALID
        assert lib.ddmpc_get_solution(h, 9, vp(out), L.MEM_HOST) in (L.ERR_INVALID, L.ERR_NOT_READY)
        P = orc.FOUR_TANK
        with pytest.raises(L.DDMPCError, match="n_mpc_step"):
            eng.closed_loop(P["A"], P["B"], P["C"], P["D"], np.zeros((B, 4)), up, yp, np.zeros((B, 5, 2)), n_mpc_step=31)
        with pytest.raises(ValueError):
            eng.closed_loop(P["A"][:3, :3], P["B"], P["C"], P["D"], np.zeros((B, 4)), up, yp, np.zeros((B, 5, 2)))
        # the handle is still usable after all of that
        u2, c2, s2, _ = eng.solve(up, yp)
        _check(spec, u_d, y_d, up, yp, u2, c2, s2, range(B))
    assert lib.ddmpc_solve(None, vp(up), vp(yp), vp(u), vp(cost), vp(st), C.c_void_p(), L.MEM_HOST) == L.ERR_INVALID
    assert lib.ddmpc_destroy(None) == L.OK


@pytest.mark.parametrize("kw,B,n_steps,n_mpc_step", [(dict(), 4, 201, 1), (dict(slack_var_constraint_type=1), 2, 101, 2)],
                         ids=["fused-warm-201", "slack-box-101"])
def test_long_closed_loop_matches_oracle(gpu, kw, B, n_steps, n_mpc_step):
    # long horizons: errors would accumulate through the plant if a step were off; the device loop must stay on
    # the oracle's trajectory from the transient into the steady state
    spec = orc.spec_from_params(**kw)
    insts = [orc.generate_instance(s) for s in range(20, 20 + B)]
    u_d = np.stack([i["u_d"] for i in insts]); y_d = np.stack([i["y_d"] for i in insts])
    x0 = np.stack([i["plant"].x for i in insts])
    w = np.stack([i["plant"].eps_max * i["rng"].uniform(-1.0, 1.0, (n_steps, 2)) for i in insts])
    up = u_d[:, -4:, :].reshape(B, -1); yp = y_d[:, -4:, :].reshape(B, -1)
    P = orc.FOUR_TANK
    with _engine(spec, 400, B) as eng:
        eng.set_data(u_d, y_d)
        u_sys, y_sys, status, *_ = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x0, up, yp, w, n_mpc_step=n_mpc_step)
    assert np.all(status == 0)
    for b in range(B):
        u_ref, y_ref = orc.closed_loop(spec, u_d[b], y_d[b], insts[b]["plant"], w[b], n_mpc_step=n_mpc_step)
        assert np.max(np.abs(u_sys[b] - u_ref)) / np.max(np.abs(u_ref)) < 1e-8
        assert np.max(np.abs(y_sys[b] - y_ref)) < 1e-9
        assert np.all(np.abs(y_sys[b, -1] - spec.y_s) < 0.05)      # near the setpoint (the 1-step scheme wanders with the noise)


def test_pipelined_host_solve(gpu):
    # ddmpc_solve_from_host = set_data + solve with the uploads overlapped with the solves (8 chunks at this size)
    spec = orc.spec_from_params(slack_var_constraint_type=1)
    B = 2500                                               # not a multiple of the chunk count
    u_d, y_d, up, yp = _instances(B)
    with _engine(spec, 400, B) as eng:
        u1, c1, s1, i1 = eng.solve_from_host(u_d, y_d, up, yp)
        uw, cw, sw, iw = eng.step(up, yp)                  # the handle now owns the uploaded data
        sg = eng.get_solution("sigma")
        eng.set_data(u_d, y_d)
        u2, c2, s2, i2 = eng.solve(up, yp)
    assert np.array_equal(u1, u2) and np.array_equal(c1, c2) and np.array_equal(s1, s2) and np.array_equal(i1, i2)
    assert np.max(np.abs(uw - u1)) / np.max(np.abs(u1)) < 1e-10 and np.array_equal(iw, i1)
    assert np.max(np.abs(sg[:, 8:])) <= spec.c * spec.eps_max * (1 + 1e-12)
    _check(spec, u_d, y_d, up, yp, u1, c1, s1, range(0, B, 311))


def test_batched_reproduction_script(gpu, tmp_path):
    # the reproduction flow as a script: seed 4 must print the reference figure's known answers
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "repro.npz"
    res = subprocess.run([sys.executable, os.path.join(root, "examples", "batched_robust_reproduction.py"),
                          "--batch", "3", "--seed", "4", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(out)
    assert np.allclose(z["TEC_1-step_u"][0, 0], [8.6604991, 8.53323249], atol=2e-7)
    assert np.allclose(z["TEC_n-step_u"][0, 0], [8.6604991, 8.53323249], atol=2e-7)
    assert np.allclose(z["UCON_1-step_u"][0, 0], [7.89630434, 9.2946719], atol=2e-7)
    assert "instance 0 at step 384" in res.stdout
    assert np.all(z["TEC_1-step_status"] == 0) and z["TEC_1-step_u"].shape == (3, 597, 2)


def test_device_memory_variants_of_every_entry_point(gpu):
    # every entry point that takes a `mem` flag, called with DEVICE pointers (torch tensors), must agree with its
    # HOST-pointer form
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    spec = orc.spec_from_params()
    B, n_steps = 6, 9
    d = generate_batch(range(B))
    u_d, y_d = d["u_d"], d["y_d"]
    up = u_d[:, -4:, :].reshape(B, -1).copy(); yp = y_d[:, -4:, :].reshape(B, -1).copy()
    w = 0.002 * np.random.default_rng(0).uniform(-1, 1, (B, n_steps, 2))
    P = orc.FOUR_TANK
    lib = L.load()
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    with _engine(spec, 400, B) as eng:
        h = eng._h
        # host references
        eng.set_data(u_d, y_d)
        u_h, c_h, s_h, i_h = (x.copy() for x in eng.step(up, yp))
        al_h = eng.get_solution("alpha"); g_h = eng.gain()
        loop_h = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=2)
        # device forms
        tud, tyd, tup, typ = t(u_d), t(y_d), t(up), t(yp)
        eng.set_data(tud, tyd)
        u_t, c_t, s_t, i_t = eng.step(tup, typ)
        torch.cuda.synchronize()
        assert np.array_equal(u_t.cpu().numpy(), u_h) and np.array_equal(c_t.cpu().numpy(), c_h) and np.array_equal(s_t.cpu().numpy(), s_h)
        al_t = torch.empty((B, 367), dtype=torch.float64, device=dev)
        L.check(lib.ddmpc_get_solution(h, L.SOL_ALPHA, ptr(al_t), L.MEM_DEVICE)); L.check(lib.ddmpc_synchronize(h))
        assert np.array_equal(al_t.cpu().numpy(), al_h)
        g_t = torch.empty((B, 17, 136), dtype=torch.float64, device=dev)
        L.check(lib.ddmpc_get_gain(h, ptr(g_t), L.MEM_DEVICE))
        assert np.array_equal(g_t.cpu().numpy(), g_h)
        x_t, upl, ypl, w_t = t(d["x_end"]), t(up), t(yp), t(w)
        us_t = torch.empty((B, n_steps, 2), dtype=torch.float64, device=dev); ys_t = torch.empty_like(us_t)
        st_t = torch.empty((B,), dtype=torch.int32, device=dev)
        A, Bm, Cm, D = (np.ascontiguousarray(P[k], dtype=np.float64) for k in ("A", "B", "C", "D"))
        pl = L.Plant(4, A.ctypes.data_as(L.c_double_p), Bm.ctypes.data_as(L.c_double_p), Cm.ctypes.data_as(L.c_double_p),
                     D.ctypes.data_as(L.c_double_p))
        L.check(lib.ddmpc_closed_loop(h, C.byref(pl), n_steps, 2, ptr(x_t), ptr(upl), ptr(ypl), ptr(w_t), ptr(us_t), ptr(ys_t),
                                      ptr(st_t), L.MEM_DEVICE))
        L.check(lib.ddmpc_synchronize(h)); torch.cuda.synchronize()
        for a, b in zip(loop_h, (us_t, ys_t, st_t, x_t, upl, ypl)):
            assert np.array_equal(np.asarray(a), b.cpu().numpy())
    # stand-alone entry points
    H_t = torch.empty((B, 34 * 2, 400 - 34 + 1), dtype=torch.float64, device=dev)
    L.check(lib.ddmpc_hankel(ptr(tud), B, 400, 2, 34, ptr(H_t), L.MEM_DEVICE, 0)); torch.cuda.synchronize()
    assert np.array_equal(H_t.cpu().numpy()[0], orc.hankel_matrix(u_d[0], 34))
    r_t = torch.empty((B,), dtype=torch.float64, device=dev); r_h = np.empty((B,))
    L.check(lib.ddmpc_pe_guard(ptr(tud), B, 400, 2, 38, ptr(r_t), L.MEM_DEVICE, 0)); torch.cuda.synchronize()
    L.check(lib.ddmpc_pe_guard(C.c_void_p(u_d.ctypes.data), B, 400, 2, 38, C.c_void_p(r_h.ctypes.data), L.MEM_HOST, 0))
    assert np.array_equal(r_t.cpu().numpy(), r_h)


def test_nominal_scheme_on_exact_data_rank_revealing(gpu):
    # Exact LTI data: rank H = 72 of 136.  With a setpoint that is a true equilibrium the nominal QP is feasible
    # and the rank-revealing rescue kernel must reproduce the SVD-based CPU solve (oracle/nominal_exact.py, an
    # orthogonal-factorisation route that shares nothing with the Gram/Cholesky kernels); with the example's
    # rounded setpoint the terminal equality cannot be met by any exact trajectory -> "infeasible".
    from direct_data_driven_mpc_amd.harness import FOUR_TANK
    from oracle.nominal_exact import solve_nominal_exact
    plant = dict(FOUR_TANK); plant["eps_max"] = 0.0
    B = 5
    d = generate_batch(range(B), N=400, plant=plant)
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    A, Bm, Cm, D = (FOUR_TANK[k] for k in "ABCD")
    spec = orc.spec_from_params(controller_type=0)
    spec.y_s = (Cm @ np.linalg.inv(np.eye(4) - A) @ Bm + D) @ spec.u_s          # the model's equilibrium output for u_s
    rng = np.random.default_rng(3)
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        for trial in range(2):
            if trial:       # another valid past window of the same plant: 4 steps further along a fresh trajectory
                d2 = generate_batch(range(50, 50 + B), N=400, plant=plant)
                up = d2["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d2["y_d"][:, -4:, :].reshape(B, -1).copy()
            u, cost, status, iters = eng.solve(up, yp)
            uw, cw, sw, _ = eng.step(up, yp)
            for b in range(B):
                ref = solve_nominal_exact(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
                assert ref["status"] == "optimal" and L.STATUS_STRINGS[int(status[b])] == "optimal", (trial, b, ref["residual"])
                assert np.max(np.abs(u[b] - ref["optimal_u"])) / np.max(np.abs(ref["optimal_u"])) < 1e-8, (trial, b)
                assert abs(cost[b] - ref["cost"]) <= 1e-8 * max(abs(ref["cost"]), 1e-6)
            assert np.array_equal(uw, u) and np.array_equal(sw, status)
    spec = orc.spec_from_params(controller_type=0)                               # y_s = (0.65, 0.77): not an equilibrium
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = eng.solve(up, yp)
    assert all(L.STATUS_STRINGS[int(s)] == "infeasible" for s in status)
    assert solve_nominal_exact(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0])["status"] == "infeasible"


def test_nominal_closed_loop_on_exact_data(gpu):
    # the nominal scheme driving a noise-free plant from exact data (the basic scheme of the paper): every
    # solve goes through the rescue kernel; the loop must settle at the equilibrium setpoint
    from direct_data_driven_mpc_amd.harness import FOUR_TANK
    plant = dict(FOUR_TANK); plant["eps_max"] = 0.0
    B, n_steps = 4, 120
    d = generate_batch(range(B), N=400, plant=plant)
    A, Bm, Cm, D = (FOUR_TANK[k] for k in "ABCD")
    spec = orc.spec_from_params(controller_type=0)
    spec.y_s = (Cm @ np.linalg.inv(np.eye(4) - A) @ Bm + D) @ spec.u_s
    up = d["u_d"][:, -4:, :].reshape(B, -1); yp = d["y_d"][:, -4:, :].reshape(B, -1)
    with _engine(spec, 400, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u_sys, y_sys, status, *_ = eng.closed_loop(A, Bm, Cm, D, d["x_end"], up, yp, np.zeros((B, n_steps, 2)), n_mpc_step=1)
    assert np.all(status == 0)
    assert np.max(np.abs(y_sys[:, -1, :] - spec.y_s)) < 1e-3 and np.max(np.abs(u_sys[:, -1, :] - spec.u_s)) < 1e-2


def test_nominal_rank_revealing_with_global_workspace(gpu):
    # L = 60 (r = 256): the packed matrices of the rescue kernel no longer fit LDS and live in a global workspace
    from direct_data_driven_mpc_amd.harness import FOUR_TANK
    from oracle.nominal_exact import solve_nominal_exact
    plant = dict(FOUR_TANK); plant["eps_max"] = 0.0
    B, N = 3, 1000
    d = generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    A, Bm, Cm, D = (FOUR_TANK[k] for k in "ABCD")
    spec = orc.spec_from_params(controller_type=0, L=60, N=N)
    spec.y_s = (Cm @ np.linalg.inv(np.eye(4) - A) @ Bm + D) @ spec.u_s
    with _engine(spec, N, B) as eng:
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = eng.solve(up, yp)
    from oracle.nominal_exact import solve_nominal_model_based
    for b in range(B):
        ref = solve_nominal_exact(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        mod = solve_nominal_model_based(spec, plant, up[b], yp[b])       # the well-conditioned yardstick (see the cfg-5 test)
        assert ref["status"] == "optimal" and int(status[b]) == 0
        sc = np.max(np.abs(mod["optimal_u"]))
        assert np.max(np.abs(u[b] - mod["optimal_u"])) / sc < TOL_U, b
        assert abs(cost[b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), b
        if np.max(np.abs(ref["optimal_u"] - mod["optimal_u"])) / sc < 3e-9:
            assert np.max(np.abs(u[b] - ref["optimal_u"])) / sc < TOL_U, b


def test_config5_size_nominal_runs_on_the_rank_revealing_kernel(gpu):
    # BASELINE configs[4]: nominal scheme, m = p = 8, n = 8, L = 30, N = 2000, noise-free data of a random stable
    # plant (SURVEY section 8 proposal): r = 608 rows, rank 312.  No register-resident kernel holds that; the
    # rank-revealing kernel runs it with its matrices in a global workspace, Gram route + adaptive refinement passes with
    # exact Hankel products.  Checked on 32 instances of the configuration against
    #   (i) a MODEL-BASED solve of the same QP (trajectory space from (A, B, C), no Hankel / Gram matrix: well conditioned)
    #       at the standard bar 1e-8 / 1e-9, and
    #  (ii) the SVD-based data-driven CPU solve (oracle/nominal_exact.py), which at this size is itself only ~1e-8 accurate
    #       (exact data rounded to fp64, cond(H) ~ 1e6): wherever the two CPU solves agree to 3e-9 the GPU must meet the
    #       standard bar against the SVD route too; where they do not, the test shows that the SVD route is the one that is off.
    from oracle.nominal_exact import solve_nominal_exact, solve_nominal_model_based
    rng = np.random.default_rng(0)
    ns = n = 8; m = p = 8; Lh = 30; N = 2000
    A = rng.normal(size=(ns, ns)); A *= 0.9 / max(abs(np.linalg.eigvals(A)))
    plant = dict(A=A, B=rng.normal(size=(ns, m)), C=rng.normal(size=(p, ns)), D=np.zeros((p, m)), eps_max=0.0)
    u_s = 0.1 * np.ones(m)
    y_s = (plant["C"] @ np.linalg.inv(np.eye(ns) - A) @ plant["B"]) @ u_s
    spec = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=3.0 * np.eye(p * Lh), R=1e-4 * np.eye(m * Lh), u_s=u_s, y_s=y_s, robust=False,
                      eps_max=0.0, lamb_alpha=0.0, lamb_sigma=0.0, c=0.0, slack="none", tec=True)
    B = 32
    d = generate_batch(range(B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with _engine(spec, N, B) as eng:
        assert eng.kernel_name() == "ddmpc_nominal_rr_kernel"
        ok, rank = eng.persistent_excitation_guard(d["u_d"])
        assert np.all(ok) and np.all(rank == m * (Lh + 2 * n))
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, status, _ = eng.solve(up, yp)
        ub = eng.get_solution("ubar")
        with pytest.raises(L.DDMPCError):
            eng.gain()
    assert np.all(status == 0) and np.array_equal(ub[:, n * m:], u)
    n_svd_off = 0
    for b in range(B):
        mod = solve_nominal_model_based(spec, plant, up[b], yp[b])
        sc = np.max(np.abs(mod["optimal_u"]))
        assert mod["feas_residual"] < 1e-10
        assert np.max(np.abs(u[b] - mod["optimal_u"])) / sc < TOL_U, b
        assert abs(cost[b] - mod["cost"]) <= TOL_COST * abs(mod["cost"]), b
        if b < 8:                                       # the SVD route takes ~2 s per instance
            ref = solve_nominal_exact(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
            assert ref["status"] == "optimal" and ref["rank"] == m * (Lh + n) + ns
            svd_vs_model = np.max(np.abs(ref["optimal_u"] - mod["optimal_u"])) / sc
            gpu_vs_svd = np.max(np.abs(u[b] - ref["optimal_u"])) / sc
            if svd_vs_model < 3e-9:
                assert gpu_vs_svd < TOL_U, b
            else:
                n_svd_off += 1
                assert np.max(np.abs(u[b] - mod["optimal_u"])) / sc < svd_vs_model, b      # the GPU is the closer of the two
            assert abs(cost[b] - ref["cost"]) <= TOL_COST * abs(ref["cost"])
    # the robust scheme at this size runs on ddmpc_large_solve_kernel (noisy data of the same plant)
    specr = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=3.0 * np.eye(p * Lh), R=1e-4 * np.eye(m * Lh), u_s=u_s, y_s=y_s, robust=True,
                       eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0, slack="convex", tec=True)
    dn = generate_batch(range(B), N=N, plant=dict(plant, eps_max=0.002))
    upn = dn["u_d"][:, -n:, :].reshape(B, -1).copy(); ypn = dn["y_d"][:, -n:, :].reshape(B, -1).copy()
    with _engine(specr, N, B) as eng:
        assert eng.kernel_name() == "ddmpc_large_solve_kernel"
        eng.set_data(dn["u_d"], dn["y_d"])
        ur, costr, statusr, itr = eng.solve(upn, ypn)
    # cond(G + lam*D) is ~8e11 at this size (G grows with N and r, lam*D does not) and the Gram route alone is good to
    # ~1e-7 there; the kernel's refinement step (residual through two exact Hankel products) restores the 1e-8 / 1e-9 bar
    _check(specr, dn["u_d"], dn["y_d"], upn, ypn, ur, costr, statusr, range(B))
    for b in range(B):
        assert int(itr[b]) == orc.solve_fullspace(specr, dn["u_d"][b], dn["y_d"][b], upn[b], ypn[b]).iters
    # dense weighting matrices of a NOMINAL controller at this size: refused until round 5, now on the phase kernels
    # (tests/test_gpu_round5.py::test_dense_weighting_matrices_of_nominal_controllers_beyond_the_register_resident_kernels); here the
    # configs[4] plant itself with Q = 3 I + 0.01 (all ones) against the model-based solution
    Qd = 3.0 * np.eye(p * Lh) + 0.01
    specd = orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=Qd, R=1e-4 * np.eye(m * Lh), u_s=u_s, y_s=y_s, robust=False, eps_max=0.0, lamb_alpha=0.0,
                       lamb_sigma=0.0, c=0.0, slack="none", tec=True)
    with BatchedDDMPC(n=n, m=m, p=p, L_=Lh, N=N, Q=Qd, R=1e-4 * np.eye(m * Lh), u_s=u_s, y_s=y_s, batch=4, controller_type=L.NOMINAL) as eng:
        eng.set_data(d["u_d"][:4], d["y_d"][:4])
        ud_, cd_, sd_, _ = eng.solve(up[:4], yp[:4])
    assert np.all(sd_ == 0)
    for b in range(2):
        modd = solve_nominal_model_based(specd, plant, up[b], yp[b])
        assert np.max(np.abs(ud_[b] - modd["optimal_u"])) / np.max(np.abs(modd["optimal_u"])) < TOL_U
        assert abs(cd_[b] - modd["cost"]) <= TOL_COST * abs(modd["cost"])
    # a shape whose trajectory chunks would not fit the kernels' LDS scratch (hundreds of channels, three time steps) is
    # refused when the controller is created, not discovered on the device
    with pytest.raises(L.DDMPCError, match="not supported by the global-workspace kernels"):
        BatchedDDMPC(n=1, m=170, p=170, L_=2, N=4000, Q=1.0, R=1.0, u_s=np.zeros(170), y_s=np.zeros(170), batch=1,
                     controller_type=L.ROBUST, eps_max=0.002, lamb_alpha=50.0, lamb_sigma=1000.0, c=1.0)


def test_plain_c_caller_of_the_abi(gpu, tmp_path):
    # the boundary used from C, not Python: tests/c/capi_caller.c is compiled with gcc against include/ddmpc.h and
    # linked to libddmpc.so; its results must equal the Python layer's bit for bit (same library, same inputs)
    import os, shutil, struct, subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "direct_data_driven_mpc_amd")
    exe = str(tmp_path / "capi_caller")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "capi_caller.c"), "-o", exe, "-L", libdir, "-lddmpc",
                    "-Wl,-rpath," + libdir], check=True)
    for slack in (L.SLACK_NONE, L.SLACK_CONVEX):
        spec = orc.spec_from_params(slack_var_constraint_type=1 if slack == L.SLACK_CONVEX else 0)
        B = 5
        u_d, y_d, up, yp = _instances(B, seed0=40)
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("7i", B, 400, 2, 2, 4, 30, slack))
            for a in (u_d, y_d, up, yp):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        res = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        raw = open(fout, "rb").read()
        nu, ns = B * 60, B * 34 * 2
        d = np.frombuffer(raw[: 8 * (2 * nu + 2 * B + ns)], dtype=np.float64)
        i = np.frombuffer(raw[8 * (2 * nu + 2 * B + ns):], dtype=np.int32)
        u_c, cost_c, u_s, cost_s, sig_c = d[:nu].reshape(B, 60), d[nu:nu + B], d[nu + B:2 * nu + B].reshape(B, 60), \
            d[2 * nu + B:2 * nu + 2 * B], d[2 * nu + 2 * B:].reshape(B, 68)
        with _engine(spec, 400, B) as eng:
            eng.set_data(u_d, y_d)
            u, cost, status, iters = eng.solve(up, yp)
            sig = eng.get_solution("sigma")
            us, cs, _, _ = eng.step(up, yp)
        assert np.array_equal(u_c, u) and np.array_equal(cost_c, cost) and np.array_equal(sig_c, sig)
        assert np.array_equal(u_s, us) and np.array_equal(cost_s, cs)
        assert np.array_equal(i[:B], status) and np.array_equal(i[B:], iters) and np.all(status == 0)
        _check(spec, u_d, y_d, up, yp, u_c, cost_c, i[:B], range(B))


def test_two_handles_from_two_threads(gpu):
    # handles are independent (own stream, own buffers; the error string is thread-local): two host threads driving
    # two controller batches at once must get what they get one after the other
    import threading
    spec = orc.spec_from_params()
    B = 64
    sets = [_instances(B, seed0=s) for s in (100, 300)]
    serial = []
    for u_d, y_d, up, yp in sets:
        with _engine(spec, 400, B) as eng:
            eng.set_data(u_d, y_d)
            serial.append([x.copy() for x in eng.solve(up, yp)])
    out = [None, None]

    def work(k):
        u_d, y_d, up, yp = sets[k]
        with _engine(spec, 400, B) as eng:
            eng.set_data(u_d, y_d)
            for _ in range(20):
                r = eng.solve(up, yp)
            s = eng.step(up, yp)
            out[k] = ([x.copy() for x in r], [x.copy() for x in s])

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        cold, warm = out[k]
        assert all(np.array_equal(a, b) for a, b in zip(cold, serial[k]))
        assert np.max(np.abs(warm[0] - serial[k][0])) <= 1e-10 * np.max(np.abs(serial[k][0])) and np.all(warm[2] == 0)
