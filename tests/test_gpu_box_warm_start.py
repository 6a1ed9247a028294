"""DDMPC_OPT_BOX_WARM_START: bounded ROBUST controllers up to 271 rows start the active-set iteration of ddmpc_step and of the
fused closed loop from the signed set the last solve of the handle ended with (box_iterate_seeded, ddmpc_box_law.hpp, DESIGN
5.5).  Four-tank, L = 30, n = 4, N = 400, seeds 500 ..., at the bars of tests/test_gpu_input_bounds.py: inputs 1e-8 relative
and cost 1e-9 against the full-space helper (tests/_box_warm_ref.py, pinned on the CPU by tests/test_box_warm_reference.py),
ddmpc_step against ddmpc_solve 1e-10, the loop with the option against the loop without it 1e-9."""
import contextlib
import types

import numpy as np
import pytest

from direct_data_driven_mpc_amd import _lib as L
from oracle import ddmpc_oracle as orc

import _input_bounds_ref as ref
import test_box_warm_reference as WR
import test_gpu_input_bounds as IB
import test_gpu_large_weights as LW
import test_gpu_parity as T

pytestmark = pytest.mark.gpu

INF = np.inf
TIGHT, WIDE, NARROW = (0.0, 2.0), (-4.0, 6.0), (0.8, 1.2)
FUSED = IB.FUSED
P = orc.FOUR_TANK

_BOX = {}


def _spec(slack=1, tec=True):
    return orc.spec_from_params(slack_var_constraint_type=slack, tec=tec)


@contextlib.contextmanager
def _bounded(spec, B, box, warm, safeguard=False, ybox=None, prepare=True, first=0, **kw):
    """A handle on instances first .. first + B - 1 of the module's data with the box set and the option as asked."""
    d, _, _ = IB._data()
    with T._engine(spec, 400, B, **kw) as eng:
        eng.set_data(d["u_d"][first:first + B], d["y_d"][first:first + B])
        eng.set_input_bounds(*box)
        if ybox is not None:
            eng.set_output_bounds(*ybox)
        if safeguard:
            eng.set_box_safeguard(True)
        if warm:
            eng.set_box_warm_start(True)
        if prepare:
            eng.prepare()
        yield eng


def _windows(B, first=0):
    _, up, yp = IB._data()
    return up[first:first + B], yp[first:first + B]


def _copy(out):
    return [np.asarray(x).copy() for x in out]


def _bit_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def _box_list(spec, box):
    """idx / lo / hi of the boxed components in the full-space stacking (they do not depend on the data)."""
    key = (spec.slack, spec.tec, box)
    if key not in _BOX:
        d, up, yp = IB._data()
        qp = orc.build_fullspace_qp(spec, d["u_d"][0], d["y_d"][0], up[0], yp[0])
        idx, lo, hi = ref.box_of(spec, qp, *box)
        _BOX[key] = types.SimpleNamespace(idx=idx, lo=lo, hi=hi)
    return _BOX[key]


def _plant_step(x, u, w):
    """One step of every instance's four-tank plant: y = C x + D u + w with the state before the update."""
    y = x @ P["C"].T + u @ P["D"].T + w
    return x @ P["A"].T + u @ P["B"].T, y


def _shift(up, yp, u, y):
    return np.concatenate([up[:, u.shape[1]:], u], axis=1), np.concatenate([yp[:, y.shape[1]:], y], axis=1)


# ------------------------------------------------------------------------------------------------ 1. contract
def test_contract(gpu):
    with _bounded(_spec(), 2, TIGHT, False, prepare=False) as eng:
        for bad in (2, -1):
            with pytest.raises(L.DDMPCError) as e:
                L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_BOX_WARM_START, bad))
            assert e.value.code == L.ERR_INVALID and "DDMPC_OPT_BOX_WARM_START" in e.value.message
        eng.set_box_warm_start(True)
        eng.set_box_warm_start(False)
    # accepted and without effect: no finite bound (slack-only CONVEX on the cwl_* kernels, slack NONE), NOMINAL, 608 rows
    d, up, yp = IB._data()
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (4, 6, 2))
    s608, N608, u608, y608, up608, yp608 = LW.robust_case("608", "none", 2)
    cases = [(_spec(1, True), 400, d["u_d"][:4], d["y_d"][:4], up[:4], yp[:4], True),
             (_spec(0, False), 400, d["u_d"][:4], d["y_d"][:4], up[:4], yp[:4], False),
             (orc.spec_from_params(controller_type=0), 400, d["u_d"][:4], d["y_d"][:4], up[:4], yp[:4], False),
             (s608, N608, u608, y608, up608, yp608, False)]

    def outputs(case, warm):
        spec, N, u_d, y_d, upc, ypc, cwl = case
        with T._engine(spec, N, u_d.shape[0]) as eng:
            eng.set_data(u_d, y_d)
            if cwl:
                eng.set_convex_warm_law(True)
            if warm:
                eng.set_box_warm_start(True)
            out = _copy(eng.solve(upc, ypc)) + _copy(eng.step(upc, ypc)) + _copy(eng.step(upc, ypc))
            if N == 400:
                out += _copy(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"][:4], upc, ypc, w))
                assert eng.closed_loop_kernel_name() != FUSED
        return out

    for case in cases:
        _bit_equal(outputs(case, False), outputs(case, True))


# ------------------------------------------------------------------------------------------------ 2. the first solve has no seed
@pytest.mark.parametrize("slack,tec,box,ybox", [(1, True, TIGHT, None), (1, True, WIDE, None), (0, False, TIGHT, None),
                                                (0, False, WIDE, None), (1, True, WIDE, ([0.60, 0.72], [0.70, 0.82]))])
def test_first_step_after_prepare_is_bit_equal(gpu, slack, tec, box, ybox):
    B = 16
    up, yp = _windows(B)
    out = {}
    for warm in (False, True):
        with _bounded(_spec(slack, tec), B, box, warm, ybox=ybox) as eng:
            out[warm] = _copy(eng.step(up, yp))
    print("iters", out[True][3], "status", out[True][2])
    assert np.any(out[False][3] >= 2)
    _bit_equal(out[False], out[True])


# ------------------------------------------------------------------------------------------------ 3. the same window twice
@pytest.mark.parametrize("box", [TIGHT, WIDE])
def test_step_behind_a_solve_at_the_same_window_takes_one_solve(gpu, box):
    B = 32
    spec = _spec()
    up, yp = _windows(B)
    bl = _box_list(spec, box)
    with _bounded(spec, B, box, True) as eng:
        uc, cc, sc, itc = _copy(eng.solve(up, yp))
        xc = IB._full_x(eng)
        us, cs, ss, its = _copy(eng.step(up, yp))
        xs = IB._full_x(eng)
        again = _copy(eng.solve(up, yp))
    with _bounded(spec, B, box, False) as eng:
        cold0 = _copy(eng.solve(up, yp))
    print("solve iters", itc, "step iters", its)
    assert np.all(sc == 0) and np.all(ss == 0)
    assert np.array_equal(its, np.where(itc >= 2, 2, 1)) and np.any(itc > 2), (itc, its)
    assert IB._rel(us, uc) < 1e-10 and np.max(np.abs(cs - cc) / np.abs(cc)) < 1e-10
    for b in range(B):
        assert np.array_equal(IB._signed_active(xs[b], bl), IB._signed_active(xc[b], bl)), b
    assert np.any(IB._signed_active(xc[0], bl) != 0)
    _bit_equal([uc, cc, sc, itc], again)                # the cold contract: from the empty set whatever the seed
    _bit_equal([uc, cc, sc, itc], cold0)


# ------------------------------------------------------------------------------------------------ 4. consecutive windows
def test_consecutive_windows_against_the_seeded_reference(gpu):
    B, n_steps, checked = 8, WR.N_STEPS, (0, 1, 2, 3)
    spec = _spec()
    d, _, _ = IB._data()
    bl = _box_list(spec, TIGHT)
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (10, 2))[:n_steps]        # the noise of WR._loop, for every instance
    iters = {}
    left_out = 0
    with _bounded(spec, B, TIGHT, True) as e1, _bounded(spec, B, TIGHT, False) as e0:
        state = {}
        for warm, eng in ((True, e1), (False, e0)):
            up, yp = (a.copy() for a in _windows(B))
            state[warm] = [d["x_end"][:B].copy(), up, yp]
        for t in range(n_steps):
            got = {}
            for warm, eng in ((True, e1), (False, e0)):
                x, up, yp = state[warm]
                u, c, s, it = _copy(eng.step(up, yp))
                got[warm] = (u, c, s, it)
                if warm:
                    xs = IB._full_x(eng)
                assert np.all(s == 0), (warm, t, s)
                x, y = _plant_step(x, u[:, :2], w[t][None])
                state[warm] = [x, *_shift(up, yp, u[:, :2], y)]
                iters.setdefault(warm, []).append(it)
            u1, c1, _, it1 = got[True]
            u0, c0, _, it0 = got[False]
            assert IB._rel(u1, u0) < 1e-9 and np.max(np.abs(c1 - c0) / np.abs(c0)) < 1e-9, t
            for b in checked:
                sol = WR._loop(IB.SEED0 + b, True)[1][2][t]
                eu = np.max(np.abs(u1[b] - sol.optimal_u)) / np.max(np.abs(sol.optimal_u))
                ec = abs(c1[b] - sol.cost) / abs(sol.cost)
                print("t=%d b=%d iters %d/%d (empty start %d) k %d margin %.1e err_u %.1e err_cost %.1e" %
                      (t, b, it1[b], sol.iters, it0[b], np.count_nonzero(sol.active), sol.margin, eu, ec))
                assert sol.status == "optimal" and eu < IB.TOL_U and ec < IB.TOL_COST, (t, b, eu, ec)
                if sol.margin < 1e-6:
                    left_out += 1
                    continue
                assert it1[b] == sol.iters, (t, b, it1[b], sol.iters)
                assert np.array_equal(IB._signed_active(xs[b], bl), sol.active), (t, b)
    assert left_out * 4 <= n_steps * len(checked), left_out
    assert np.array_equal(iters[True][0], iters[False][0])                              # no seed at the first step
    for t in range(1, n_steps):
        assert np.sum(iters[True][t]) < np.sum(iters[False][t]), (t, iters[True][t], iters[False][t])


# ------------------------------------------------------------------------------------------------ 5. the fused loop
@pytest.mark.parametrize("n_mpc_step", [1, 2])
@pytest.mark.parametrize("box,safeguard", [(TIGHT, False), (NARROW, True)])
def test_fused_loop_against_the_loop_without_the_option(gpu, box, safeguard, n_mpc_step):
    B = 32
    spec = _spec()
    d, _, _ = IB._data()
    up, yp = _windows(B)
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (B, 20, 2))
    out = {}
    with _bounded(spec, B, box, False, safeguard=safeguard) as eng:
        for key, warm in (("empty", False), ("warm", True), ("warm again", None)):
            if warm is not None:
                eng.set_box_warm_start(warm)
            out[key] = _copy(eng.closed_loop(P["A"], P["B"], P["C"], P["D"], d["x_end"], up, yp, w, n_mpc_step=n_mpc_step))
            assert eng.closed_loop_kernel_name() == FUSED
            out[key].append(eng.get_solution("ubar"))
    base = out["empty"]
    assert np.all(base[2] == 0)
    for key in ("warm", "warm again"):                   # ("again": its first solve starts from the set the loop before it left)
        got = out[key]
        assert np.all(got[2] == 0), (key, got[2])
        for a, b in zip(base, got):
            assert np.max(np.abs(a.astype(float) - b.astype(float))) < 1e-9, key
        assert IB._within(got[0], box[0], box[1])
        assert IB._within(IB._free_inputs(spec, got[6]), box[0], box[1])
    assert np.max(base[0]) == box[1]                     # the bound is met along the way


# ------------------------------------------------------------------------------------------------ 6. what drops the seed
def _other_data(eng):
    d, _, _ = IB._data()
    eng.set_data(d["u_d"][8:16], d["y_d"][8:16])


def _new_prepare(eng):
    L.check(eng._lib.ddmpc_set_option(eng._h, L.OPT_REFINE_RES_LOG10, 107))            # (the default) forgets what ddmpc_prepare kept
    eng.prepare()


@pytest.mark.parametrize("event", ["set_setpoints", "set_input_bounds", "nbox", "set_data", "prepare", "toggle"])
def test_seed_lifetime(gpu, event):
    B = 8
    spec = _spec()
    up, yp = _windows(B)
    first_box = ([0.0, -INF], [2.0, INF]) if event == "nbox" else TIGHT
    events = {"set_setpoints": lambda eng: eng.set_setpoints(spec.u_s, spec.y_s),
              "set_input_bounds": lambda eng: eng.set_input_bounds([0.1, 0.0], [2.0, 1.9]),
              "nbox": lambda eng: eng.set_input_bounds(*TIGHT),                          # one channel bounded -> both
              "set_data": _other_data,
              "prepare": _new_prepare,
              "toggle": lambda eng: None}
    out = {}
    for warm in (False, True):
        with _bounded(spec, B, first_box, warm) as eng:
            first = _copy(eng.step(up, yp))
            seeded = _copy(eng.step(up, yp))
            if event == "toggle":
                if warm:
                    eng.set_box_warm_start(True)                                        # setting it, to either value, drops the seed
            else:
                events[event](eng)
            out[warm] = (first, seeded, _copy(eng.step(*(_windows(B, 8) if event == "set_data" else (up, yp)))))
    print(event, "iters", out[True][0][3], out[True][1][3], out[True][2][3])
    _bit_equal(out[False][0], out[True][0])
    assert np.all(out[True][1][3][out[True][0][3] >= 2] == 2)                            # (the seed was there)
    assert np.any(out[True][0][3] > 2) and np.all(out[True][2][2] == 0)
    _bit_equal(out[False][2], out[True][2])


# ------------------------------------------------------------------------------------------------ 7. fall-back
def test_fall_back_at_the_cap(gpu):
    """Cap 3 on [0, 2].  Instances 0 .. 7 start at the data tail (9 and more solves from the empty set), 8 .. 15 thirteen
    closed-loop steps later, where the loop needs 3, 2, 1, 1 solves (seed 508 on the CPU; the others within a step of that).  All
    handles see the windows of a loop driven by a handle with cap 50 and without the option."""
    B, n_steps, cap, ahead = 16, 4, 3, 13
    spec = _spec()
    d, _, _ = IB._data()
    up, yp = (a.copy() for a in _windows(B))
    x = d["x_end"][:B].copy()
    w = 0.002 * np.random.default_rng(9).uniform(-1.0, 1.0, (ahead + n_steps, B, 2))
    with _bounded(spec, B, TIGHT, False) as eng:
        _, _, st, xa, upa, ypa = eng.closed_loop(P["A"], P["B"], P["C"], P["D"], x, up, yp, w[:ahead].transpose(1, 0, 2))
        assert np.all(st == 0)
    x[8:], up[8:], yp[8:] = xa[8:], upa[8:], ypa[8:]
    w = w[ahead:]
    within = 0
    with _bounded(spec, B, TIGHT, False) as e50, _bounded(spec, B, TIGHT, False, max_iter=cap) as e0, \
            _bounded(spec, B, TIGHT, True, max_iter=cap) as e1, _bounded(spec, B, TIGHT, True, safeguard=True, max_iter=cap) as es:
        prev = None
        for t in range(n_steps):
            u50, c50, s50, i50 = _copy(e50.step(up, yp))
            u0, c0, s0, i0 = _copy(e0.step(up, yp))
            u1, c1, s1, i1 = _copy(e1.step(up, yp))
            u_s, c_s, s_s, i_s = _copy(es.step(up, yp))
            print("t=%d cap 50 %s | cap 3: option 0 %s %s | option 1 %s %s | safeguard %s %s" % (t, i50, s0, i0, s1, i1, s_s, i_s))
            assert np.all(s50 == 0)
            ok0 = s0 == 0
            assert np.array_equal(ok0, i50 <= cap) and np.all(s0[~ok0] == 4)
            # never a worse status than without the option; an instance the seed solves beyond that is a gain
            assert np.all(s1[ok0] == 0) and np.all((s1 == 0) | (s1 == 4))
            good = s1 == 0
            if np.any(good):
                assert IB._rel(u1[good], u50[good]) < 1e-10 and np.max(np.abs(c1[good] - c50[good]) / np.abs(c50[good])) < 1e-10
            within += int(np.count_nonzero(ok0 & (i0 >= 2)))
            # a neighbour with an empty seed -- no step before, a failed one, or one without a violation -- is bit-equal
            empty = np.ones(B, bool) if prev is None else (prev[0] > 1) | (prev[1] == 1)
            for a, b in ((u0, u1), (c0, c1), (s0, s1), (i0, i1)):
                assert np.array_equal(a[empty], b[empty], equal_nan=True), t
            prev = (s1, i1)
            # with the safeguard every instance is solved, to the result of cap 50
            assert np.all(s_s == 0)
            assert IB._rel(u_s, u50) < 1e-9 and np.max(np.abs(c_s - c50) / np.abs(c50)) < 1e-9
            if t == 0:
                assert np.all(i_s[i50 > cap] > cap) and np.array_equal(i_s[i50 <= cap], i50[i50 <= cap])
            x, y = _plant_step(x, u50[:, :2], w[t])
            up, yp = _shift(up, yp, u50[:, :2], y)
    assert within >= 4, within


# ------------------------------------------------------------------------------------------------ 8. an invalid seed is never read
def test_first_step_does_not_depend_on_what_the_allocator_hands_back(gpu):
    B = 8
    up, yp = _windows(B)
    lib = L.load()
    out = []
    try:
        for fill in (0, 255, 63):
            lib.ddmpc_debug_poison_allocations(fill)
            with _bounded(_spec(), B, TIGHT, True) as eng:
                out.append(_copy(eng.step(up, yp)))
    finally:
        lib.ddmpc_debug_poison_allocations(0)
    assert np.any(out[0][3] > 2) and np.all(out[0][2] == 0)
    _bit_equal(out[0], out[1])
    _bit_equal(out[0], out[2])
