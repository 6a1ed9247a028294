"""The fix-up of the cold-solve kernel (ddmpc_cold2.hpp: `fix_tile`) and its output stage at the shapes where their lane tests
differ: a padding row (-1 on the diagonal) inside a diagonal tile that also holds real rows, with the right-hand side column
opening a tile of its own (15 and 63 rows, rE = 16 and 64), three channels either way round (the Gram matrix then comes
ready-made: the `gpre` mode), one and four waves, and the benchmark's own tile row 8 (136 rows).  Every shape runs with slack
NONE and slack CONVEX -- whose second active-set pass reads the rewritten dvec / tvec again -- each with the default
refinement mode and with every instance re-solved by the refining variant; one shape runs with dense weighting matrices
(the `dense_w` branch of both).  Reference: the compiled CPU restatement (`oracle_c.solve_batch`) at the tolerances of
tests/test_gpu_panel_substeps.py; dense weights: the full-space oracle, the checker and tolerances of
tests/test_gpu_large_weights.py."""
import functools

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc
from oracle import oracle_c

TOL_U, TOL_COST = 1e-8, 1e-9

_A = np.array([[0.9, 0.2], [0.0, 0.7]])
P12 = dict(A=_A, B=np.array([[0.0], [1.0]]), C=np.array([[1.0, 0.0], [0.3, 1.0]]), D=np.zeros((2, 1)), eps_max=0.001)   # m = 1, p = 2
P21 = dict(A=_A, B=np.array([[0.0, 0.5], [1.0, 0.2]]), C=np.array([[1.0, 0.4]]), D=np.zeros((1, 2)), eps_max=0.001)     # m = 2, p = 1

# name -> (plant, n, L, N, batch, rows r = (m + p)(L + n), kernel instance)
SHAPES = {
    "r15-m1p2": (P12, 1, 4, 60, 12, 15, "2,1"),        # rE = 16: one padding row in tile 0, the rhs column alone in tile 1
    "r15-m2p1": (P21, 1, 4, 60, 12, 15, "2,1"),        # the same with the channels the other way round
    "r63-m1p2": (P12, 2, 19, 120, 12, 63, "5,4"),      # rE = 64: the same at four waves with helpers
    "r136": (None, 4, 30, 400, 8, 136, "9,4"),         # the benchmark's shape: tile row 8 holds 8 real rows, the rhs column, padding
}


def _spec(name, slack):
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    if plant is None:
        return orc.spec_from_params(L=Lh, N=N, n=n, slack_var_constraint_type=slack)
    m, p = plant["B"].shape[1], plant["C"].shape[0]
    u_s = np.full(m, 0.3)
    y_s = (plant["C"] @ np.linalg.solve(np.eye(2) - plant["A"], plant["B"]) + plant["D"]) @ u_s      # the equilibrium output
    return orc.QPSpec(n=n, m=m, p=p, L=Lh, Q=2.0 * np.eye(p * Lh), R=0.01 * np.eye(m * Lh), u_s=u_s, y_s=y_s,
                      robust=True, eps_max=0.001, lamb_alpha=100.0, lamb_sigma=500.0, c=1.0,
                      slack="convex" if slack else "none", tec=True)


@functools.lru_cache(maxsize=None)
def reference(name, slack):
    """Inputs of one shape and the C restatement's answer (computed once per shape and slack type, never modified)."""
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    spec = _spec(name, slack)
    assert (spec.m + spec.p) * (spec.L + spec.n) == r
    d = generate_batch(range(200, 200 + B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    ref = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=2)
    for a in (d["u_d"], d["y_d"], up, yp) + tuple(ref):
        a.setflags(write=False)
    return spec, d["u_d"], d["y_d"], up, yp, ref


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_c_restatement_solves_every_case(name, slack):
    # (CPU) the reference reports every instance of every case optimal and finite; under the box some instance takes a second
    # active-set iteration, so the pass that reads the rewritten dvec / tvec runs
    u_ref, c_ref, st_ref, it_ref = reference(name, slack)[5]
    assert not np.count_nonzero(st_ref)
    assert np.all(np.isfinite(u_ref)) and np.all(np.isfinite(c_ref))
    if slack:
        assert np.max(it_ref) > 1, it_ref


def test_full_space_oracle_agrees_with_the_c_restatement():
    # (CPU) the reference of the new plants against the full-space oracle, on a sample
    for name in ("r15-m1p2", "r15-m2p1"):
        spec, u_d, y_d, up, yp, (u_ref, c_ref, st_ref, it_ref) = reference(name, 1)
        for b in (0, 7):
            sol = orc.solve_fullspace(spec, u_d[b], y_d[b], up[b], yp[b])
            assert sol.status == "optimal" and sol.iters == it_ref[b]
            assert np.max(np.abs(sol.optimal_u - u_ref[b])) / np.max(np.abs(u_ref[b])) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("refine", ["auto", "always"])
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_fixup_and_outputs_match_c_restatement(gpu, name, slack, refine):
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    spec, u_d, y_d, up, yp, (u_ref, c_ref, st_ref, it_ref) = reference(name, slack)
    assert not np.count_nonzero(st_ref)
    with BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                      controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if slack else L.SLACK_NONE, eps_max=spec.eps_max,
                      lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec) as eng:
        assert inst in eng.kernel_name()
        eng.set_refinement(refine)
        eng.set_data(u_d, y_d)
        u, cost, st, it = eng.solve(up, yp)
    eu = np.max(np.max(np.abs(u - u_ref), axis=1) / np.max(np.abs(u_ref), axis=1))
    ec = np.max(np.abs(cost - c_ref) / np.abs(c_ref))
    print("%s slack=%d refine=%s: err u %.3e cost %.3e iters %s" % (name, slack, refine, eu, ec, sorted(set(it.tolist()))))
    assert np.array_equal(st, st_ref)
    assert eu < TOL_U and ec < TOL_COST, (eu, ec)
    if slack:
        assert np.array_equal(it, it_ref)
    else:
        assert np.all(it == 1)


def _spd(rng, size, scale, blocks):
    # block-banded, diagonally dominant (hence SPD) matrix: couples neighbouring prediction steps and channels
    A = rng.normal(size=(size, size)) * 0.2
    W = A @ A.T / size + np.eye(size)
    band = np.abs(np.subtract.outer(np.arange(size), np.arange(size))) <= blocks
    return scale * (W * band + np.diag(np.abs(W * ~band).sum(axis=1)))


@pytest.mark.gpu
def test_fixup_and_outputs_with_dense_weights(gpu):
    # dense SPD Q, R at 40 rows (three tile columns, two waves, the last tile half padded): lam W^-1 goes into every tile
    # behind the fix-up, and the output stage forms z from a row of it
    n, Lh, N, B = 2, 8, 90, 4
    spec = orc.spec_from_params(L=Lh, N=N, n=n)
    rng = np.random.default_rng(11)
    spec.Q = _spd(rng, spec.p * Lh, 3.0, 3)
    spec.R = _spd(rng, spec.m * Lh, 1e-4, 2)
    d = generate_batch(range(200, 200 + B), N=N)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with BatchedDDMPC(n=n, m=spec.m, p=spec.p, L_=Lh, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                      controller_type=L.ROBUST, slack_type=L.SLACK_NONE, eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha,
                      lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec) as eng:
        assert eng.weight_kind == L.WEIGHT_DENSE and "3,2" in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, st, it = eng.solve(up, yp)
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(st[b])] == sol.status == "optimal"
        eu = float(np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)))
        ec = abs(cost[b] - sol.cost) / abs(sol.cost)
        print("dense instance %d: u %.2e cost %.2e" % (b, eu, ec))
        assert eu < TOL_U and ec <= TOL_COST, (b, eu, ec)
