"""The walks down the tile diagonals of the structured Gram in the cold-solve kernel (ddmpc_cold2.hpp, step (3) of the
structured branch), unrolled with the operands of the next step in flight, at the smallest shapes that reach every multi-wave
kernel instance and every way the last tile row can look: a half-padded last tile, the right-hand side column opening a tile of
its own (the last diagonal tile then holds no real row), a wholly padded tile row, eight waves, and two channels (SISO plants:
two MFMA pairs per walk step).  Every shape runs with slack NONE and slack CONVEX, each with the default refinement mode and
with every instance re-solved by the refining variant; one shape per instance also with the rank-k update of the slack box off
(the second active-set pass then forms, walks and factors again); the benchmark's shape also through prepare() + step() (the
factor export) and with the diagnostic stamps on (helper waves 1..3 then store their arrival at the barrier behind the
fix-up).  Reference: the compiled CPU restatement (`oracle_c.solve_batch`) at the tolerances of tests/test_gpu_cold_fixup.py;
dense weights: the full-space oracle, as there."""
import functools

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc
from oracle import oracle_c

TOL_U, TOL_COST = 1e-8, 1e-9

P11 = dict(A=np.array([[0.9, 0.2], [0.0, 0.7]]), B=np.array([[0.0], [1.0]]), C=np.array([[1.0, 0.4]]), D=np.zeros((1, 1)),
           eps_max=0.001)                                                                                     # m = p = 1

# name -> (plant, n, L, N, batch, rows r = (m + p)(L + n), kernel instance)
SHAPES = {
    "r40": (None, 2, 8, 90, 8, 40, "3,2"),             # one helper owns every off-diagonal tile; half-padded last tile
    "r64": (None, 4, 12, 160, 8, 64, "5,4"),           # the rhs column opens a tile of its own: the last diagonal tile holds no real row
    "r72": (None, 4, 14, 160, 8, 72, "5,4"),           # half-padded last tile
    "r96": (None, 4, 20, 240, 8, 96, "7,4"),           # rhs-only last tile at another split of the diagonals over the helpers
    "r128": (None, 4, 28, 400, 8, 128, "9,4"),         # the same at the headline instance
    "r136": (None, 4, 30, 400, 8, 136, "9,4"),         # the benchmark's shape
    "r256": (None, 4, 60, 600, 4, 256, "17,8"),        # eight waves, seven helpers, walks of up to 16 steps
    "siso-r64": (P11, 2, 30, 200, 8, 64, "5,4"),       # two channels: two MFMA pairs per walk step
    "siso-r80": (P11, 2, 38, 240, 8, 80, "7,4"),       # two channels on an instance with a wholly padded tile row
}
ONE_PER_INSTANCE = ["r40", "r72", "r96", "r136", "r256"]


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
    d = generate_batch(range(300, 300 + B), N=N, plant=plant)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    ref = oracle_c.solve_batch(spec, N, d["u_d"], d["y_d"], up, yp, threads=2)
    for a in (d["u_d"], d["y_d"], up, yp) + tuple(ref):
        a.setflags(write=False)
    return spec, d["u_d"], d["y_d"], up, yp, ref


def _engine(name, slack):
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    spec = reference(name, slack)[0]
    eng = BatchedDDMPC(n=spec.n, m=spec.m, p=spec.p, L_=spec.L, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                       controller_type=L.ROBUST, slack_type=L.SLACK_CONVEX if slack else L.SLACK_NONE, eps_max=spec.eps_max,
                       lamb_alpha=spec.lamb_alpha, lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec)
    assert inst in eng.kernel_name(), eng.kernel_name()
    return eng


def _check(tag, name, slack, out):
    u, cost, st, it = out
    u_ref, c_ref, st_ref, it_ref = reference(name, slack)[5]
    eu = np.max(np.max(np.abs(u - u_ref), axis=1) / np.max(np.abs(u_ref), axis=1))
    ec = np.max(np.abs(cost - c_ref) / np.abs(c_ref))
    print("%s %s slack=%d: err u %.3e cost %.3e iters %s" % (tag, name, slack, eu, ec, sorted(set(it.tolist()))))
    assert np.array_equal(st, st_ref)
    assert eu < TOL_U and ec < TOL_COST, (eu, ec)
    if slack:
        assert np.array_equal(it, it_ref)
    else:
        assert np.all(it == 1)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_c_restatement_solves_every_case(name, slack):
    # (CPU) the reference reports every instance of every case optimal and finite; under the box some instance takes a second
    # active-set iteration
    u_ref, c_ref, st_ref, it_ref = reference(name, slack)[5]
    assert not np.count_nonzero(st_ref)
    assert np.all(np.isfinite(u_ref)) and np.all(np.isfinite(c_ref))
    if slack:
        assert np.max(it_ref) > 1, it_ref


@pytest.mark.gpu
@pytest.mark.parametrize("refine", ["auto", "always"])
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_walks_match_c_restatement(gpu, name, slack, refine):
    spec, u_d, y_d, up, yp, ref = reference(name, slack)
    with _engine(name, slack) as eng:
        eng.set_refinement(refine)
        eng.set_data(u_d, y_d)
        _check("refine=" + refine, name, slack, eng.solve(up, yp))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ONE_PER_INSTANCE)
def test_second_pass_forms_and_walks_again(gpu, name):
    # slack CONVEX with the rank-k update off: every active-set iteration forms the system, walks and factors again
    spec, u_d, y_d, up, yp, ref = reference(name, 1)
    with _engine(name, 1) as eng:
        eng.set_convex_update(False)
        eng.set_data(u_d, y_d)
        _check("refactor", name, 1, eng.solve(up, yp))


@pytest.mark.gpu
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_prepare_then_step_matches(gpu, slack):
    # the factor export of ddmpc_prepare next to the walks, at the benchmark's shape
    spec, u_d, y_d, up, yp, ref = reference("r136", slack)
    with _engine("r136", slack) as eng:
        eng.set_data(u_d, y_d)
        cold = tuple(np.array(a) for a in eng.solve(up, yp))
        eng.prepare()
        warm = eng.step(up, yp)
        _check("cold", "r136", slack, cold)
        _check("step", "r136", slack, warm)
        assert np.max(np.abs(warm[0] - cold[0])) / np.max(np.abs(cold[0])) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
def test_stamps_do_not_change_results(gpu, slack):
    spec, u_d, y_d, up, yp, ref = reference("r136", slack)
    with _engine("r136", slack) as eng:
        eng.set_data(u_d, y_d)
        plain = tuple(np.array(a) for a in eng.solve(up, yp))
        eng.debug_stamps(True)
        stamped = tuple(np.array(a) for a in eng.solve(up, yp))
        st = eng.debug_stamps(False, fetch=True).astype(np.int64)
    for a, b in zip(plain, stamped):
        assert np.array_equal(a, b)
    _check("stamps", "r136", slack, stamped)
    # helper waves 1..3 left the low half of their clock in the upper halves of slots 7..9: later than the panel wave's stamp 2,
    # by less than the whole solve
    t2 = st[:, 2] & 0xffffffff
    for w in (1, 2, 3):
        d = ((st[:, 6 + w] >> 32) - t2) & 0xffffffff
        assert np.all(d > 0) and np.all(d < st[:, 14] - st[:, 0]), (w, d)


def _spd(rng, size, scale, blocks):
    # block-banded, diagonally dominant (hence SPD) matrix: couples neighbouring prediction steps and channels
    A = rng.normal(size=(size, size)) * 0.2
    W = A @ A.T / size + np.eye(size)
    band = np.abs(np.subtract.outer(np.arange(size), np.arange(size))) <= blocks
    return scale * (W * band + np.diag(np.abs(W * ~band).sum(axis=1)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r40", "r64"])
def test_walks_with_dense_weights(gpu, name):
    # dense SPD Q, R on a multi-wave instance: lam W^-1 goes into every tile behind the walks
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    B = 4
    spec = orc.spec_from_params(L=Lh, N=N, n=n)
    rng = np.random.default_rng(11)
    spec.Q = _spd(rng, spec.p * Lh, 3.0, 3)
    spec.R = _spd(rng, spec.m * Lh, 1e-4, 2)
    d = generate_batch(range(300, 300 + B), N=N)
    up = d["u_d"][:, -n:, :].reshape(B, -1).copy(); yp = d["y_d"][:, -n:, :].reshape(B, -1).copy()
    with BatchedDDMPC(n=n, m=spec.m, p=spec.p, L_=Lh, N=N, Q=spec.Q, R=spec.R, u_s=spec.u_s, y_s=spec.y_s, batch=B,
                      controller_type=L.ROBUST, slack_type=L.SLACK_NONE, eps_max=spec.eps_max, lamb_alpha=spec.lamb_alpha,
                      lamb_sigma=spec.lamb_sigma, c=spec.c, use_terminal_constraint=spec.tec) as eng:
        assert eng.weight_kind == L.WEIGHT_DENSE and inst in eng.kernel_name()
        eng.set_data(d["u_d"], d["y_d"])
        u, cost, st, it = eng.solve(up, yp)
    for b in range(B):
        sol = orc.solve_fullspace(spec, d["u_d"][b], d["y_d"][b], up[b], yp[b])
        assert L.STATUS_STRINGS[int(st[b])] == sol.status == "optimal"
        eu = float(np.max(np.abs(u[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u)))
        ec = abs(cost[b] - sol.cost) / abs(sol.cost)
        print("dense %s instance %d: u %.2e cost %.2e" % (name, b, eu, ec))
        assert eu < TOL_U and ec <= TOL_COST, (b, eu, ec)
