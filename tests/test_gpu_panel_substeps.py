"""The panel wave's in-tile factorisation (ddmpc_cold2.hpp: `substep`, `factor_begin`, `factor_end`) at the shapes where it
can go wrong: the last diagonal tile half padded, not padded at all (the right-hand side column then opens a tile of its
own), and nearly all padding (one real pivot group); the full-size `<9,4>` instance; a two-channel plant.  Every shape runs
with slack NONE and slack CONVEX (whose later active-set iterations go through the kept-factor update route), each with
the default refinement mode and with every instance re-solved by the refining variant -- the three kernel variants share
the sub-step.  Reference: the compiled CPU restatement (`oracle_c.solve_batch`), tolerances of tests/test_gpu_parity.py."""
import functools

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.engine import BatchedDDMPC
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc
from oracle import oracle_c

TOL_U, TOL_COST = 1e-8, 1e-9

# m = p = 1, order 2 (the plant of tests/test_gpu_parity.py::test_siso_system_with_padded_rows)
SISO = dict(A=np.array([[0.9, 0.2], [0.0, 0.7]]), B=np.array([[0.0], [1.0]]), C=np.array([[1.0, 0.0]]), D=np.zeros((1, 1)),
            eps_max=0.001)

# name -> (plant, n, L, N, batch, rows r = (m + p)(L + n), kernel instance)
SHAPES = {
    # (the small four-tank shapes estimate the order as n = 2: the controller asks for L >= 2 n)
    "r24-half-padded": (None, 2, 4, 60, 12, 24, "2,1"),       # r = 8 (mod 16): two pivot groups in the last tile
    "r40-half-padded": (None, 2, 8, 90, 12, 40, "3,2"),
    "r32-no-padding": (None, 2, 6, 80, 12, 32, "3,2"),        # r = 0 (mod 16): the rhs column is alone in the last tile
    "r36-one-group": (None, 2, 7, 90, 12, 36, "3,2"),         # r = 4 (mod 16): one real pivot group, three skipped
    "r136-full-size": (None, 4, 30, 400, 8, 136, "9,4"),
    "r24-two-channels": (SISO, 2, 10, 80, 12, 24, "2,1"),     # m + p = 2: the interleaved Gram, r = 8 (mod 16)
}


def _spec(name, slack):
    plant, n, Lh, N, B, r, inst = SHAPES[name]
    if plant is None:
        return orc.spec_from_params(L=Lh, N=N, n=n, slack_var_constraint_type=slack)
    return orc.QPSpec(n=n, m=1, p=1, L=Lh, Q=2.0 * np.eye(Lh), R=0.01 * np.eye(Lh), u_s=np.array([0.3]), y_s=np.array([1.0]),
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
    # (CPU) the reference itself reports every instance of every chosen case optimal
    ref = reference(name, slack)[5]
    assert not np.count_nonzero(ref[2])
    assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("refine", ["auto", "always"])
@pytest.mark.parametrize("slack", [0, 1], ids=["none", "convex"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_panel_substeps_match_c_restatement(gpu, name, slack, refine):
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
