"""Which kernel steps the plant in ddmpc_closed_loop, row by row of the decision the host takes (LoopPath, ddmpc_api.hip).

One handle per row on the four-tank parameters (N = 400, B = 4, 9 plant steps, a solve every 2).  Every row asserts the
kernel ddmpc_closed_loop_kernel_name reports, the statuses, and that the outputs equal the same handle's "cold"-path
outputs within the 1e-9 of test_closed_loop_warm_and_cold_paths_agree.  The fused rows run a second time on the same handle
without new data: the kept law is reused, so the kernel is the same and the outputs are bit-equal.

The table is a record of what the loop does today, not a specification: it was written against the code before the
decision moved into one function, and passed there unchanged.
"""
import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from direct_data_driven_mpc_amd.harness import generate_batch
from oracle import ddmpc_oracle as orc

import test_gpu_parity as T

pytestmark = pytest.mark.gpu

B, N, N_STEPS, N_MPC_STEP = 4, 400, 9, 2
TOL = 1e-9
PLANT = "ddmpc_plant_kernel"
FUSED_AFFINE = "ddmpc_closed_loop_warm_kernel"
FUSED_CONVEX = "ddmpc_closed_loop_convex_warm_kernel"
FUSED_BOX = "ddmpc_closed_loop_box_kernel"
CONVEX = dict(slack_var_constraint_type=1)
NOMINAL = dict(controller_type=0)


def _bounds(eng):
    eng.set_input_bounds([-4.0, -4.0], [6.0, 6.0])


def _cwl_off(eng):
    eng.set_convex_warm_law(True)
    eng.set_refinement("off")


def _cwl_always(eng):                       # every law refined: cwl_nref = B
    eng.set_convex_warm_law(True)
    eng.set_refinement("always")


# id: (spec keywords, options set before the data, singular instance or None, path, kernel)
ROWS = {
    "robust-cold": (dict(), None, None, "cold", PLANT),
    "robust-warm": (dict(), None, None, "warm", FUSED_AFFINE),
    "robust-auto": (dict(), None, None, "auto", FUSED_AFFINE),
    "convex-auto-filtered": (CONVEX, None, None, "auto", PLANT),
    "convex-law-warm": (CONVEX, _cwl_off, None, "warm", FUSED_CONVEX),
    "convex-law-refined-warm": (CONVEX, _cwl_always, None, "warm", PLANT),
    "nominal-warm": (NOMINAL, None, None, "warm", FUSED_AFFINE),
    "nominal-singular-warm": (NOMINAL, None, 2, "warm", PLANT),
    "bounds-auto": (dict(), _bounds, None, "auto", FUSED_BOX),
    "bounds-cold": (dict(), _bounds, None, "cold", PLANT),
}
FUSED_ROWS = [k for k, v in ROWS.items() if v[4] != PLANT]


@pytest.fixture(scope="module")
def inputs():
    d = generate_batch(range(70, 70 + B), N=N)
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B, N_STEPS, 2))
    up = d["u_d"][:, -4:, :].reshape(B, -1).copy()
    yp = d["y_d"][:, -4:, :].reshape(B, -1).copy()
    return d, up, yp, w


def _loop(eng, d, up, yp, w, path):
    P = orc.FOUR_TANK
    eng.set_closed_loop_path(path)
    out = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=N_MPC_STEP)
    return [np.asarray(a).copy() for a in out], eng.closed_loop_kernel_name()


@pytest.mark.parametrize("row,second", [(r, False) for r in ROWS] + [(r, True) for r in FUSED_ROWS],
                         ids=list(ROWS) + [r + "-second-call" for r in FUSED_ROWS])
def test_loop_path(gpu, inputs, row, second):
    kw, options, singular, path, kernel = ROWS[row]
    d, up, yp, w = inputs
    u_d, y_d = d["u_d"], d["y_d"]
    if singular is not None:                # constant data: singular Gram (test_warm_path_invalidation_and_bad_instance)
        u_d = u_d.copy(); y_d = y_d.copy(); u_d[singular] = 1.0; y_d[singular] = 0.5
    with T._engine(orc.spec_from_params(**kw), N, B) as eng:
        if options:
            options(eng)
        eng.set_data(u_d, y_d)
        out, name = _loop(eng, d, up, yp, w, path)
        assert name == kernel, (row, name)
        if second:
            again, name = _loop(eng, d, up, yp, w, path)
            assert name == kernel, (row, name)
            for a, b in zip(out, again):
                assert np.array_equal(a, b), row
            return
        cold, name = _loop(eng, d, up, yp, w, "cold")
        assert name == PLANT, (row, name)
    status = [L.STATUS_STRINGS[int(s)] for s in out[2]]
    want = ["infeasible" if b == singular else "optimal" for b in range(B)]
    print("%s: statuses %s" % (row, status))
    assert status == want, (row, status)
    for a, b, what in zip(out, cold, ("u_sys", "y_sys", "status", "x_end", "u_past", "y_past")):
        a, b = a.astype(float), b.astype(float)
        nan = np.isnan(a)                   # (the loop writes no u_sys / y_sys for an instance without a solution)
        assert np.array_equal(nan, np.isnan(b)) and not np.any(nan[[i for i in range(B) if i != singular]]), (row, what)
        err = np.max(np.abs(a - b)[~nan])
        print("%s: %s vs cold %.2e" % (row, what, err))
        assert err < TOL, (row, what, err)
