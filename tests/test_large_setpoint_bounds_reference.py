"""CPU premises of DDMPC_OPT_LARGE_SETPOINT_BOUNDS (tests/test_gpu_large_setpoint_bounds.py), from the reference
helpers alone.

1. The reduced system of the empty active set does not depend on the setpoint: K0 = G + lam D0 of
   tests/_setpoint_law_ref.reduced_matrix is bit-equal between two setpoints, and so is the "boxed last" order with the
   components of the box table (the bounds are absolute), and with both W = L_TT^-1 E of any set of components, formed here
   from the factor of each K0 and compared bit for bit.  What depends on the setpoint is the target t and, per boxed input /
   output component, the offset a_s and the shifts bound - a_s.
2. The reduced iteration with per-instance a_s and shifts -- tests/_large_box_ref.solve_reduced on
   with_setpoints(spec, us[b], ys[b]) -- reproduces the full-space solve_bounded at the bars: same status, same iteration count,
   same signed set, inputs 1e-8, cost 1e-9 (measured <= 3.4e-12 / 3.3e-13 on the thinnest case).
3. What the GPU file relies on, for every case it compares: every instance optimal with margin >= 1e-7 (the thinnest is
   2.3e-7, "296/none/uy" instance 0), the set of every iteration within the capacity the case runs at (final and peak), and in
   the capacity case exactly the instances 1, 3 and 4 beyond 64 (at iterations 2, 4 and 2).  The margin of the reduced
   iteration is the full-space helper's on every instance computed with both (item 2), so item 3 takes it from the reduced one.
   The same for the cases on the other plants (300 rows: peak 63 of the 128 it runs at; 608 rows: peak 10 of 64) and for the
   safeguard case: instance 4, and only it, ends at the cap of 50 iterations in the primal-dual iteration, the primal method
   ends optimal on it after 128 solves with at most 132 of 192 components and margin 6.1e-5.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import _large_setpoint_bounds_cases as C
import _setpoint_law_ref as ref
from test_large_bounds_reference import box_order

TOL_U, TOL_COST, MARGIN = 1e-8, 1e-9, 1e-7


def test_factor_and_table_do_not_depend_on_the_setpoint():
    for slack in ("none", "convex"):
        c = C.case("296/%s/u" % slack)
        spec = c["spec"]
        moved = ref.with_setpoints(spec, c["us"][1], c["ys"][1])
        for x, y in zip(ref.reduced_matrix(spec, c["u_d"][0], c["y_d"][0]), ref.reduced_matrix(moved, c["u_d"][0], c["y_d"][0])):
            assert np.array_equal(x, y)
        box = dict(u=C.U_WIDE, y=C.Y_EQ)
        for x, y in zip(box_order(spec, box), box_order(moved, box)):
            assert np.array_equal(x, y)
        # W = L_TT^-1 E_T of every fourth boxed component, on the trailing block of the "boxed last" order
        perm, nA, cpos, _ = box_order(spec, box)
        n0, cols = nA & ~63, np.unique(cpos)[::4]
        Ws = []
        for sp in (spec, moved):
            K0 = ref.reduced_matrix(sp, c["u_d"][0], c["y_d"][0])[0]
            Lf = np.linalg.cholesky(K0[np.ix_(perm, perm)])                 # (reduced_matrix: component order)
            E = np.zeros((len(perm) - n0, len(cols)))
            E[cols - n0, np.arange(len(cols))] = 1.0
            Ws.append(sla.solve_triangular(Lf[n0:, n0:], E, lower=True))
        assert np.array_equal(Ws[0], Ws[1]) and np.all(np.isfinite(Ws[0]))


@pytest.mark.parametrize("name", ["296/none/uy", "296/convex/y", "272/none/u"])
def test_reduced_iteration_with_per_instance_offsets_is_the_full_space_one(name):
    c = C.case(name)
    for b, (fu, rd) in enumerate(zip(C.full(name), C.reduced(name))):
        eu = np.max(np.abs(rd.optimal_u - fu.optimal_u)) / np.max(np.abs(fu.optimal_u))
        ec = abs(rd.cost - fu.cost) / abs(fu.cost)
        print("%s b=%d iters %d/%d set %d margin %.1e/%.1e eu %.1e ec %.1e" %
              (name, b, rd.iters, fu.iters, np.count_nonzero(fu.active), rd.margin, fu.margin, eu, ec))
        assert fu.status == rd.status == "optimal" and fu.iters == rd.iters, (b, fu.status, rd.status, fu.iters, rd.iters)
        assert np.array_equal(fu.idx, rd.idx) and np.array_equal(fu.active, rd.active), b
        assert eu < TOL_U and ec < TOL_COST, (b, eu, ec)
        assert fu.margin >= MARGIN and abs(rd.margin - fu.margin) <= 1e-3 * fu.margin, (b, rd.margin, fu.margin)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_conditions_of_the_gpu_cases(name):
    c = C.case(name)
    over = []
    for b, rd in enumerate(C.reduced(name)):
        print("%s b=%d iters %d peak %d final %d margin %.1e over 64 at %s" %
              (name, b, rd.iters, rd.peak, np.count_nonzero(rd.active), rd.margin, rd.first_over(64)))
        assert rd.status == "optimal" and rd.margin >= MARGIN, (b, rd.status, rd.margin)
        assert rd.peak <= c["cap"], (b, rd.peak)
        over.append(rd.first_over(64))
    if name == "296/none/u-tight":
        assert over == [None, 2, None, 4, 2, None], over
    if c["cap"] == 64:
        assert over == [None] * c["B"], over


@pytest.mark.parametrize("which", ["300", "608"])
def test_conditions_of_the_other_plants(which):
    c = C.case_300() if which == "300" else C.case_608()
    for b in range(c["B"]):
        rd = C.reduced_reference(c, b)
        print("%s b=%d iters %d peak %d final %d margin %.1e" % (which, b, rd.iters, rd.peak, np.count_nonzero(rd.active), rd.margin))
        assert rd.status == "optimal" and rd.margin >= MARGIN, (b, rd.status, rd.margin)
        assert rd.peak <= c["cap"], (b, rd.peak)


def test_conditions_of_the_safeguard_case():
    c = C.case_safe()
    pd = [C.reduced_reference(c, b, max_iter=C.MAX_ITER_SAFE) for b in range(c["B"])]
    assert [s.status == "optimal" for s in pd] == [True, True, True, True, False, True], [s.status for s in pd]
    assert pd[4].iters == C.MAX_ITER_SAFE
    for b, s in enumerate(pd):                                         # (the neighbours are compared bit for bit, and must solve)
        assert s.peak <= c["cap"] and (b == 4 or s.margin >= MARGIN), (b, s.peak, s.margin)
    pr = C.primal_reference(c, 4)
    print("safeguard b=4: primal %s after %d solves, peak %d, margin %.1e" % (pr.status, pr.iters, pr.peak, pr.margin))
    assert pr.status == "optimal" and pr.margin >= MARGIN and pr.peak <= c["cap"], (pr.status, pr.margin, pr.peak)
