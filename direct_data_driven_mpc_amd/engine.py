"""Batched Data-Driven MPC QP engine: Python host side over the C ABI.

`BatchedDDMPC` owns one `ddmpc_handle` = one batch of independent controller
instances that share the controller parameters and differ in their data
trajectories (u_d, y_d) and past windows.  This is the data-parallel axis the
reference does not have (one `DirectDataDrivenMPCController` = one instance,
direct_data_driven_mpc_controller.py:22).

Buffers may be numpy arrays (host; the library stages them, calls are
synchronous) or torch CUDA tensors (device resident; calls are asynchronous on
the current torch stream).  torch is plumbing only and is imported lazily.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib as L


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _weights(W, size: int, name: str) -> Tuple[int, np.ndarray]:
    """Accept scalar / 1-D diagonal / 2-D matrix; return (kind, values).  A 2-D matrix that is diagonal is
    passed as its diagonal, anything else as the dense matrix (symmetry and definiteness are checked by
    `ddmpc_create`)."""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 0:
        return L.WEIGHT_SCALAR, W.reshape(1).copy()
    if W.ndim == 1:
        if W.shape[0] != size:
            raise ValueError("%s diagonal must have %d entries" % (name, size))
        d = W
    elif W.ndim == 2:
        if W.shape != (size, size):
            raise ValueError("%s must be %dx%d" % (name, size, size))
        d = np.diag(W)
        if np.any(W != np.diag(d)):
            return L.WEIGHT_DENSE, np.ascontiguousarray(W, dtype=np.float64)
    else:
        raise ValueError("%s has too many dimensions" % name)
    if np.all(d == d[0]):
        return L.WEIGHT_SCALAR, np.array([d[0]], dtype=np.float64)
    return L.WEIGHT_DIAG, np.ascontiguousarray(d, dtype=np.float64)


def _expand_weight(kind: int, v: np.ndarray, size: int, target: int) -> np.ndarray:
    """Bring a weight to the representation `target` (both weights travel in the same kind)."""
    if kind == target:
        return v
    d = np.full(size, v[0]) if kind == L.WEIGHT_SCALAR else v
    return d if target == L.WEIGHT_DIAG else np.ascontiguousarray(np.diag(d))


class BatchedDDMPC:
    def __init__(self, n: int, m: int, p: int, L_: int, N: int, Q, R, u_s, y_s, batch: int,
                 controller_type: int = L.ROBUST, slack_type: int = L.SLACK_NONE,
                 eps_max: Optional[float] = None, lamb_alpha: Optional[float] = None,
                 lamb_sigma: Optional[float] = None, c: Optional[float] = None,
                 use_terminal_constraint: bool = True, device: int = 0, max_iter: int = 0,
                 gram_mode: int = L.GRAM_AUTO):
        self._lib = L.load()
        self.n, self.m, self.p, self.L, self.N, self.batch = int(n), int(m), int(p), int(L_), int(N), int(batch)
        self.device = int(device)
        self.controller_type, self.slack_type = int(controller_type), int(slack_type)
        wk_q, q = _weights(Q, self.p * self.L, "Q")
        wk_r, r = _weights(R, self.m * self.L, "R")
        if wk_q != wk_r:      # mixed: bring both to the richer representation
            target = max(wk_q, wk_r)
            q = _expand_weight(wk_q, q, self.p * self.L, target)
            r = _expand_weight(wk_r, r, self.m * self.L, target)
            wk_q = wk_r = target
        self._q, self._r = q, r
        self.weight_kind = int(wk_q)                     # DDMPC_WEIGHT_* handed to ddmpc_create
        self._us = np.ascontiguousarray(np.asarray(u_s, dtype=np.float64).reshape(-1))
        self._ys = np.ascontiguousarray(np.asarray(y_s, dtype=np.float64).reshape(-1))
        if self._us.size != self.m or self._ys.size != self.p:
            raise ValueError("u_s / y_s must have m / p entries")
        prm = L.Params()
        prm.struct_size = C.sizeof(L.Params)
        prm.m, prm.p, prm.n, prm.L, prm.N = self.m, self.p, self.n, self.L, self.N
        prm.controller_type, prm.slack_type = self.controller_type, self.slack_type
        prm.use_terminal_constraint = 1 if use_terminal_constraint else 0
        prm.weight_kind = wk_q
        prm.Q = self._q.ctypes.data_as(L.c_double_p)
        prm.R = self._r.ctypes.data_as(L.c_double_p)
        prm.eps_max = float(eps_max) if eps_max is not None else 0.0
        prm.lamb_alpha = float(lamb_alpha) if lamb_alpha is not None else 0.0
        prm.lamb_sigma = float(lamb_sigma) if lamb_sigma is not None else 0.0
        prm.c = float(c) if c is not None else 0.0
        prm.u_s = self._us.ctypes.data_as(L.c_double_p)
        prm.y_s = self._ys.ctypes.data_as(L.c_double_p)
        prm.max_iter = int(max_iter)
        prm.gram_mode = int(gram_mode)
        self._h = C.c_void_p()
        L.check(self._lib.ddmpc_create(C.byref(prm), self.batch, self.device, C.byref(self._h)))
        self._keep = {}

    # ---- lifetime ------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ddmpc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- helpers -----------------------------------------------------------
    def _ptr(self, x, shape, name, dtype=np.float64, writable=False):
        """Return (pointer, mem, keepalive) for a numpy array or a torch CUDA tensor."""
        if _is_torch(x):
            import torch
            want = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
            if not x.is_cuda or x.dtype != want or not x.is_contiguous():
                raise ValueError("%s must be a contiguous CUDA tensor of dtype %s" % (name, want))
            if tuple(x.shape) != tuple(shape):
                raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(x.shape)))
            return C.c_void_p(x.data_ptr()), L.MEM_DEVICE, x
        a = np.asarray(x)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(a.shape)))
        if writable:
            if a.dtype != dtype or not a.flags.c_contiguous or not a.flags.writeable:
                raise ValueError("%s must be a writable C-contiguous %s array" % (name, np.dtype(dtype)))
        else:
            a = np.ascontiguousarray(a, dtype=dtype)
        return C.c_void_p(a.ctypes.data), L.MEM_HOST, a

    def _use_torch_stream(self):
        import torch
        self._lib.ddmpc_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    # ---- API ---------------------------------------------------------------
    def set_data(self, u_d, y_d) -> None:
        """u_d [batch,N,m], y_d [batch,N,p] (controller.py:177-179)."""
        pu, mu, ku = self._ptr(u_d, (self.batch, self.N, self.m), "u_d")
        py, my, ky = self._ptr(y_d, (self.batch, self.N, self.p), "y_d")
        if mu != my:
            raise ValueError("u_d and y_d must live in the same memory space")
        if mu == L.MEM_DEVICE:
            self._use_torch_stream()
        L.check(self._lib.ddmpc_set_data(self._h, pu, py, mu))
        self._keep["data"] = (ku, ky)

    def solve(self, u_past, y_past, u_opt=None, cost=None, status=None, iters=None, warm: bool = False):
        """One QP solve per instance.  Returns (u_opt, cost, status, iters).

        warm=False: cold solve (Hankel -> Gram -> KKT -> Cholesky -> solve), `ddmpc_solve`.
        warm=True : `ddmpc_step`, the affine law prepared once per data set; with slack CONVEX the instances
                    whose affine iterate leaves the slack box are re-solved cold inside the same call."""
        return self._solve(u_past, y_past, u_opt, cost, status, iters, warm, None)

    def _solve(self, u_past, y_past, u_opt, cost, status, iters, warm, setpoints):
        """`solve` / `step` (setpoints None) and `step_setpoints` (setpoints = (u_s [batch,m], y_s [batch,p]))."""
        B = self.batch
        dev = _is_torch(u_past)
        if u_opt is None:
            if dev:
                import torch
                kw = dict(device=u_past.device)
                u_opt = torch.empty((B, self.L * self.m), dtype=torch.float64, **kw)
                cost = torch.empty((B,), dtype=torch.float64, **kw)
                status = torch.empty((B,), dtype=torch.int32, **kw)
                iters = torch.empty((B,), dtype=torch.int32, **kw)
            else:
                u_opt = np.empty((B, self.L * self.m))
                cost = np.empty((B,))
                status = np.empty((B,), dtype=np.int32)
                iters = np.empty((B,), dtype=np.int32)
        p1, m1, k1 = self._ptr(u_past, (B, self.n * self.m), "u_past")
        p2, m2, k2 = self._ptr(y_past, (B, self.n * self.p), "y_past")
        p3, m3, k3 = self._ptr(u_opt, (B, self.L * self.m), "u_opt", writable=True)
        p4, m4, k4 = self._ptr(cost, (B,), "cost", writable=True)
        p5, m5, k5 = self._ptr(status, (B,), "status", dtype=np.int32, writable=True)
        if iters is not None:
            p6, m6, k6 = self._ptr(iters, (B,), "iters", dtype=np.int32, writable=True)
        else:
            p6, m6, k6 = C.c_void_p(), m1, None
        mems = {m1, m2, m3, m4, m5, m6}
        if setpoints is not None:
            p7, m7, k7 = self._ptr(setpoints[0], (B, self.m), "u_s")
            p8, m8, k8 = self._ptr(setpoints[1], (B, self.p), "y_s")
            mems |= {m7, m8}
        if len(mems) != 1:
            raise ValueError("all solve buffers must live in the same memory space")
        if m1 == L.MEM_DEVICE:
            self._use_torch_stream()
        if setpoints is not None:
            L.check(self._lib.ddmpc_step_setpoints(self._h, p1, p2, p7, p8, p3, p4, p5, p6, m1))
            self._keep["solve"] = (k1, k2, k3, k4, k5, k6, k7, k8)
            return u_opt, cost, status, iters
        fn = self._lib.ddmpc_step if warm else self._lib.ddmpc_solve
        L.check(fn(self._h, p1, p2, p3, p4, p5, p6, m1))
        self._keep["solve"] = (k1, k2, k3, k4, k5, k6)
        return u_opt, cost, status, iters

    def solve_from_host(self, u_d, y_d, u_past, y_past):
        """`set_data` + `solve` for host arrays in one pipelined call (uploads overlapped with the solves)."""
        B = self.batch
        arrs = []
        for a, shape, name in ((u_d, (B, self.N, self.m), "u_d"), (y_d, (B, self.N, self.p), "y_d"),
                               (u_past, (B, self.n * self.m), "u_past"), (y_past, (B, self.n * self.p), "y_past")):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != shape:
                raise ValueError("%s must have shape %s" % (name, (shape,)))
            arrs.append(a)
        u_opt = np.empty((B, self.L * self.m)); cost = np.empty((B,))
        status = np.empty((B,), dtype=np.int32); iters = np.empty((B,), dtype=np.int32)
        vp = lambda x: C.c_void_p(x.ctypes.data)
        L.check(self._lib.ddmpc_solve_from_host(self._h, *(vp(a) for a in arrs), vp(u_opt), vp(cost), vp(status), vp(iters)))
        self._keep["data"] = (None, None)
        return u_opt, cost, status, iters

    def prepare(self) -> None:
        """Factor once per data set and form the affine law used by `step`."""
        if "data" in self._keep and self._keep["data"][0] is not None and _is_torch(self._keep["data"][0]):
            self._use_torch_stream()
        L.check(self._lib.ddmpc_prepare(self._h))

    def step(self, u_past, y_past, u_opt=None, cost=None, status=None, iters=None):
        """Warm control step (`ddmpc_step`): same outputs as `solve`."""
        return self.solve(u_past, y_past, u_opt, cost, status, iters, warm=True)

    def gain(self) -> np.ndarray:
        """The prepared affine law: [batch, n*(m+p)+1, r] with beta = gain[:,0] + gain[:,1:]^T [u_past; y_past] (component
        order; a large NOMINAL handle's law gives z = [ubar; ybar] instead of beta)."""
        nf = self.n * (self.m + self.p)
        out = np.empty((self.batch, nf + 1, (self.m + self.p) * (self.L + self.n)))
        L.check(self._lib.ddmpc_get_gain(self._h, C.c_void_p(out.ctypes.data), L.MEM_HOST))
        return out

    def set_closed_loop_graph(self, on: bool) -> None:
        """Record the per-step launches of `closed_loop` into one HIP graph and replay it (default off)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_CLOSED_LOOP_GRAPH, 1 if on else 0))

    def set_closed_loop_path(self, path: str) -> None:
        """'auto' | 'cold' | 'warm' (DDMPC_OPT_CLOSED_LOOP_PATH)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_CLOSED_LOOP_PATH, {"auto": 0, "cold": 1, "warm": 2}[path]))

    def set_refinement(self, mode: str = "auto", max_passes: Optional[int] = None, res_log10: Optional[float] = None) -> None:
        """Iterative refinement of the cold solve with exact Hankel products (DDMPC_OPT_REFINE): 'off' | 'auto' |
        'always'; `res_log10`: auto mode re-solves an instance with refinement when the relative exact-Hankel residual of
        its plain solve exceeds 10^res_log10 (resolution 0.1; default -10.7)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_REFINE, {"off": L.REFINE_OFF, "auto": L.REFINE_AUTO, "always": L.REFINE_ALWAYS}[mode]))
        if max_passes is not None:
            L.check(self._lib.ddmpc_set_option(self._h, L.OPT_REFINE_MAX, int(max_passes)))
        if res_log10 is not None:
            L.check(self._lib.ddmpc_set_option(self._h, L.OPT_REFINE_RES_LOG10, int(round(-10 * res_log10))))

    def set_large_pipeline(self, mode: str) -> None:
        """NOMINAL controllers beyond the register-resident kernels: 'phases' (default: one kernel per phase over the whole
        batch) | 'one_workgroup' (DDMPC_OPT_LARGE_PIPELINE)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_PIPELINE,
                                           {"one_workgroup": L.PIPELINE_ONE_WORKGROUP, "phases": L.PIPELINE_PHASES}[mode]))

    def set_convex_update(self, on: bool) -> None:
        """Slack CONVEX on the register-resident kernels: True (default) = active-set iterations after the first keep the first
        factor (rank-k update), False = every iteration factors the system again (DDMPC_OPT_CONVEX_UPDATE)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_CONVEX_UPDATE, 1 if on else 0))

    def set_convex_warm_law(self, on: bool) -> None:
        """Slack CONVEX: True = `prepare` also forms M = K0^-1 E_box and `step` / `closed_loop` run the active-set iterations
        on the law and M, without cold re-solves (DDMPC_OPT_CONVEX_WARM_LAW; costs nbox * r doubles per instance), False
        (default) = instances whose law leaves the box are re-solved cold.  No effect without the slack box."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_CONVEX_WARM_LAW, 1 if on else 0))

    def set_gram_launch(self, kind: str) -> None:
        """Structured Gram of plants with other than two or four channels on the register-resident kernels: "matrix_pipe"
        (default: streaming launch, lag sums and window walk by MFMA) or "staged" (round 4's launch with the whole trajectory
        in LDS) -- DDMPC_OPT_GRAM_LAUNCH."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_GRAM_LAUNCH, {"matrix_pipe": 0, "staged": 1}[kind]))

    def set_large_affine_law(self, on: bool) -> None:
        """Controllers beyond the register-resident kernels: `prepare` also forms an affine law of the past window and `step`
        evaluates it (DDMPC_OPT_LARGE_AFFINE_LAW; default off: `step` repeats the solve on the kept factors).  NOMINAL: the law
        of z.  ROBUST (phase kernels, up to 1024 rows): the law of beta of the empty active set, in the layout of a small ROBUST
        handle's `gain()`; under the slack box the instances that leave it are re-solved on the kept factors in the same step.
        Dense weights, more than 1024 rows or n(m+p) > 256 raise ERR_UNSUPPORTED."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_AFFINE_LAW, 1 if on else 0))

    def set_setpoint_law(self, on: bool) -> None:
        """ROBUST controllers up to 271 rows, slack NONE, scalar / diagonal weights, no bounds: True = `prepare` also forms
        S = K0^-1 [1_c], (m+p) r doubles per instance, which makes the setpoint an argument of the step: `step_setpoints`,
        `closed_loop_setpoints`, `setpoint_gain` (DDMPC_OPT_SETPOINT_LAW).  `solve`, `step`, `closed_loop`, `gain` and
        `get_solution` stay bit-equal to False (default).  Changing the value forgets what `prepare` kept.  Raises
        ERR_UNSUPPORTED on NOMINAL controllers, the CONVEX slack box, dense weights, more than 271 rows, a trajectory beyond
        the LDS, n(m+p) > 256 and a handle with bounds."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_SETPOINT_LAW, 1 if on else 0))

    def set_setpoint_box_law(self, on: bool) -> None:
        """`set_setpoint_law` for handles that carry input / output bounds (DDMPC_OPT_SETPOINT_BOX_LAW): True = `prepare` forms
        S next to the law and M, finite bounds are accepted before or after it, and `step_setpoints` / `closed_loop_setpoints` on
        a bounded handle run the active-set iteration of `step` with the instance's own setpoint in the law, the offsets of the
        boxed components and the output stage (one launch each; `set_box_safeguard` applies).  Without finite bounds the calls
        are those of `set_setpoint_law(True)`, bit-equal.  Per instance: a non-finite setpoint is solver_error; with the
        terminal constraint a setpoint outside the bounds of its channel is infeasible (NaN outputs, iters 0).  `solve`,
        `step`, `closed_loop`, `gain` and `get_solution` stay bit-equal to False (default).  Changing the value forgets what
        `prepare` kept.  Raises ERR_UNSUPPORTED on NOMINAL controllers, the CONVEX slack box, dense weights, more than 271 rows,
        a trajectory beyond the LDS and n(m+p) > 256.  The bounds are the handle's (not per instance), the iteration of the
        new calls starts from the empty set (`set_box_warm_start` is not honoured), and `get_solution` is not available after
        them."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_SETPOINT_BOX_LAW, 1 if on else 0))

    def set_setpoint_convex_law(self, on: bool) -> None:
        """`set_setpoint_law` / `set_setpoint_box_law` for ROBUST controllers with the CONVEX slack box, slack-only or with
        input / output bounds set before or after it (DDMPC_OPT_SETPOINT_CONVEX_LAW): True = `prepare` forms S next to the law
        and, on a slack-only handle, the slack box list and M whether or not `set_convex_warm_law` is on (L p r doubles per
        instance: 65 KB at L = 30, m = p = 2).  `step_setpoints` / `closed_loop_setpoints` then run the active-set iteration
        of `step` with the instance's own setpoint in the law, the offsets of the input / output components (a slack
        component keeps offset 0) and the output stage; `set_box_safeguard` applies on bounded handles.  Per instance: a
        non-finite setpoint is solver_error; with the terminal constraint a setpoint outside the bounds of its channel is
        infeasible (NaN outputs, iters 0).  `solve`, `step`, `closed_loop`, `gain` and `get_solution` stay bit-equal to False
        (default).  Changing the value forgets what `prepare` kept.  Raises ERR_UNSUPPORTED on NOMINAL controllers, slack
        NONE (use `set_setpoint_law` / `set_setpoint_box_law`), dense weights, more than 271 rows, a trajectory beyond the
        LDS, n(m+p) > 256 and a zero Q entry on a boxed output.  The iteration starts from the empty set, and `get_solution`
        is not available after the calls."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_SETPOINT_CONVEX_LAW, 1 if on else 0))

    def set_large_setpoints(self, on: bool) -> None:
        """ROBUST controllers on the phase kernels (272 .. 1024 rows), slack NONE or the CONVEX slack box, scalar / diagonal
        weights, no bounds: True = `step_setpoints` and `closed_loop_setpoints` are open (DDMPC_OPT_LARGE_SETPOINTS).  The
        factor `prepare` keeps does not depend on the setpoint, so the step on the kept factor takes the instance's own
        setpoint: same launches, statuses and `iters` as `step`, active-set iteration under the slack box included.
        With `set_large_affine_law(True)` as well `prepare` forms S = K0^-1 [1_c] next to the law ((m+p) r doubles per
        instance, built and refined apart from it), the step is one launch on the law and S plus the kept-factor solve for
        the instances without a law, without a setpoint law or outside the slack box, and `setpoint_gain` returns S.
        `solve`, `step`, `closed_loop`, `gain` and `get_solution` stay bit-equal to False (default).  Changing the value
        forgets what `prepare` kept.  Raises ERR_UNSUPPORTED on NOMINAL controllers, dense weights, up to 271 rows (use
        `set_setpoint_law` / `set_setpoint_box_law` / `set_setpoint_convex_law`), more than 1024 rows, the one-workgroup
        pipeline, debug stamps, batch > 65535, n(m+p) > 256 and a handle with bounds (bounds, the one-workgroup pipeline and
        stamps are refused afterwards, too).  Under the slack box an instance with more than 64 slack components switched at
        once, or with a failed pivot in the small system of the switched components, is solver_error in the two calls (`step` hands it to a fall-back kernel that knows the shared setpoints only);
        `get_solution` is not available after them."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_SETPOINTS, 1 if on else 0))

    def set_large_setpoint_bounds(self, on: bool) -> None:
        """ROBUST controllers on the phase kernels (272 .. 1024 rows) with input and / or output bounds
        (`set_large_bounds(True)` admits them; either order), slack NONE or the CONVEX slack box, scalar / diagonal weights:
        True = `step_setpoints` and `closed_loop_setpoints` are open (DDMPC_OPT_LARGE_SETPOINT_BOUNDS).  Neither the kept
        factor nor the bounds depend on the setpoint, so the bounded solve of `step` takes the instance's own setpoint as
        target, as the offset of every boxed input / output component and in the output stage; at the handle's own setpoints
        it is bit-equal to `step`.  The capacity and the safeguard apply as to `step`; the warm start and the box law are
        not honoured (empty set, whole batch on the kept factor, the seed is dropped).  Per instance: a non-finite setpoint
        is solver_error, a setpoint outside its channel's bounds under the terminal constraint is infeasible (NaN outputs,
        iters 0), an instance beyond the capacity or with a failed pivot is solver_error.  Without finite bounds the calls
        run what `set_large_setpoints` runs on the kept factors.  `setpoint_gain` raises ERR_UNSUPPORTED (no S at this size
        on a bounded handle); `get_solution` is not available after the calls.  `solve`, `step`, `closed_loop`, `gain` and
        `get_solution` stay bit-equal to False (default); changing the value forgets nothing `prepare` kept.  Raises
        ERR_UNSUPPORTED on NOMINAL controllers, dense weights, up to 271 rows (use `set_setpoint_box_law` /
        `set_setpoint_convex_law`), more than 1024 rows, the one-workgroup pipeline, debug stamps, batch > 65535 and
        n(m+p) > 256.  `set_large_setpoints(True)` keeps refusing bounds."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_SETPOINT_BOUNDS, 1 if on else 0))

    def set_instance_setpoint_bounds(self, on: bool) -> None:
        """Per-instance bounds (`set_instance_input_bounds` / `set_instance_output_bounds`) together with per-instance, per-step
        setpoints (`set_setpoint_box_law` / `set_setpoint_convex_law`) on one handle of at most 271 rows
        (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS): True = the two are accepted on the same handle, in either order, and
        `step_setpoints` / `closed_loop_setpoints` run the iteration of `step` with the instance's own setpoint AND its own
        bounds ('ddmpc_closed_loop_instance_setpoint_box_kernel', under the CONVEX slack box
        'ddmpc_closed_loop_instance_setpoint_convex_kernel').  Per instance: with the terminal constraint a setpoint outside
        that instance's own bounds is infeasible (NaN outputs, iters 0), also when a neighbour's wider box holds it; an active
        input or output equals its instance's bound exactly.  Rows that are all equal give results bit-equal to the shared
        bounds.  `set_box_safeguard` applies; `set_box_warm_start` is not honoured.  `solve`, `step`, `closed_loop`, `gain`,
        `setpoint_gain` and `get_solution` are those of the handle with False (default), with which the two features refuse
        each other as before; changing the value forgets nothing `prepare` kept.  With the terminal constraint the handle's
        own setpoint must still lie inside every instance's row.  Raises ERR_UNSUPPORTED on more than 271 rows (bounds stay
        shared there), NOMINAL controllers and dense weights, and for False while the handle carries per-instance bounds and
        one of the two setpoint options together (remove one first)."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_INSTANCE_SETPOINT_BOUNDS, 1 if on else 0))

    def step_setpoints(self, u_past, y_past, u_s, y_s, u_opt=None, cost=None, status=None, iters=None):
        """Warm control step with one setpoint per instance (`ddmpc_step_setpoints`): u_s [batch,m], y_s [batch,p], in the
        memory space of the windows; same outputs and array / tensor handling as `solve`.  The handle's own setpoints are not
        read; `get_solution` is not available after it (until the next `solve` / `step`).  Needs `set_setpoint_law(True)`,
        `set_setpoint_convex_law(True)` (CONVEX slack box), or
        `set_setpoint_box_law(True)`, which a handle with input / output bounds requires: there the step iterates on the box
        as `step` does (`iters` counts its solves; infeasible with NaN outputs for a setpoint outside the bounds under the
        terminal constraint).  Beyond 271 rows: `set_large_setpoints(True)` -- the step of `step` on the kept factor with the
        instance's setpoint, or with `set_large_affine_law(True)` one launch on the law and S plus the kept-factor solve for
        the instances it leaves; on a handle with bounds there, `set_large_setpoint_bounds(True)` -- the bounded solve of
        `step` with the instance's setpoint."""
        return self._solve(u_past, y_past, u_opt, cost, status, iters, True, (u_s, y_s))

    def setpoint_gain(self) -> np.ndarray:
        """S of the prepared law: [batch, m+p, r], beta = gain[:,1:]^T [u_past; y_past] + S^T [u_s; y_s] (component order).
        Beyond 271 rows (`set_large_setpoints(True)`) S exists only next to the law of `set_large_affine_law(True)`:
        ERR_NOT_READY otherwise."""
        out = np.empty((self.batch, self.m + self.p, (self.m + self.p) * (self.L + self.n)))
        L.check(self._lib.ddmpc_get_setpoint_gain(self._h, C.c_void_p(out.ctypes.data), L.MEM_HOST))
        return out

    def closed_loop_setpoints(self, A, B, Cm, D, x0, u_past, y_past, w, u_ref, y_ref, n_mpc_step: int = 1):
        """`closed_loop` with a setpoint schedule per instance (`ddmpc_closed_loop_setpoints`, one fused launch): u_ref
        [batch,n_steps,m], y_ref [batch,n_steps,p]; the solve made at step t tracks row t.  Needs `set_setpoint_law(True)`,
        `set_setpoint_convex_law(True)` (CONVEX slack box: 'ddmpc_closed_loop_setpoint_convex_kernel'), or
        `set_setpoint_box_law(True)`, which a handle with input / output bounds requires ('ddmpc_closed_loop_setpoint_box_kernel':
        an instance stops at a solve that is not optimal and at a refused setpoint).  Beyond 271 rows
        (`set_large_setpoints(True)`) the loop runs per step ('ddmpc_plant_kernel'), the solve at step t reading row t of the
        schedules in place; n_mpc_step * m has no limit there.  The same holds on a bounded handle beyond 271 rows with
        `set_large_setpoint_bounds(True)`."""
        return self.closed_loop(A, B, Cm, D, x0, u_past, y_past, w, n_mpc_step, _ref=(u_ref, y_ref))

    def closed_loop(self, A, B, Cm, D, x0, u_past, y_past, w, n_mpc_step: int = 1, _ref=None):
        """Batched closed loop on the device (controller_operation.py:259-305 for every instance).

        A,B,Cm,D: plant matrices; x0 [batch,ns]; u_past [batch,n*m], y_past [batch,n*p];
        w [batch,n_steps,p] measurement noise.  Returns (u_sys, y_sys, status, x_end, u_past_end, y_past_end)
        as host arrays (inputs are not modified)."""
        A = np.ascontiguousarray(A, dtype=np.float64); Bm = np.ascontiguousarray(B, dtype=np.float64)
        Cm = np.ascontiguousarray(Cm, dtype=np.float64); D = np.ascontiguousarray(D, dtype=np.float64)
        ns = A.shape[0]
        if A.shape != (ns, ns) or Bm.shape != (ns, self.m) or Cm.shape != (self.p, ns) or D.shape != (self.p, self.m):
            raise ValueError("plant matrices have inconsistent shapes")
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim != 3 or w.shape[0] != self.batch or w.shape[2] != self.p:
            raise ValueError("w must have shape [batch, n_steps, p]")
        n_steps = w.shape[1]
        x = np.array(x0, dtype=np.float64, order="C").reshape(self.batch, ns).copy()
        up = np.array(u_past, dtype=np.float64, order="C").reshape(self.batch, self.n * self.m).copy()
        yp = np.array(y_past, dtype=np.float64, order="C").reshape(self.batch, self.n * self.p).copy()
        u_sys = np.empty((self.batch, n_steps, self.m)); y_sys = np.empty((self.batch, n_steps, self.p))
        status = np.empty((self.batch,), dtype=np.int32)
        pl = L.Plant(ns, A.ctypes.data_as(L.c_double_p), Bm.ctypes.data_as(L.c_double_p),
                     Cm.ctypes.data_as(L.c_double_p), D.ctypes.data_as(L.c_double_p))
        vp = lambda a: C.c_void_p(a.ctypes.data)
        if _ref is not None:
            ur = np.ascontiguousarray(_ref[0], dtype=np.float64); yr = np.ascontiguousarray(_ref[1], dtype=np.float64)
            if ur.shape != (self.batch, n_steps, self.m) or yr.shape != (self.batch, n_steps, self.p):
                raise ValueError("u_ref / y_ref must have shape [batch, n_steps, m] / [batch, n_steps, p]")
            L.check(self._lib.ddmpc_closed_loop_setpoints(self._h, C.byref(pl), n_steps, int(n_mpc_step), vp(x), vp(up), vp(yp),
                                                          vp(w), vp(ur), vp(yr), vp(u_sys), vp(y_sys), vp(status), L.MEM_HOST))
            return u_sys, y_sys, status, x, up, yp
        L.check(self._lib.ddmpc_closed_loop(self._h, C.byref(pl), n_steps, int(n_mpc_step), vp(x), vp(up), vp(yp), vp(w),
                                            vp(u_sys), vp(y_sys), vp(status), L.MEM_HOST))
        return u_sys, y_sys, status, x, up, yp

    def persistent_excitation_ranks(self, u_d) -> np.ndarray:
        """Rank of the order-(L+2n) Hankel matrix of every instance's input data, the reference's
        construction-time guard (controller.py:275-296, hankel_matrix.py:55-87): Hankel gather on the
        GPU, ranks by batched SVD on the host with numpy's default tolerance (exactly the reference's
        test).  An instance is persistently exciting iff its rank equals m*(L+2n)."""
        H = hankel_matrix_batched(np.asarray(u_d, dtype=np.float64), self.L + 2 * self.n, device=self.device)
        return np.linalg.matrix_rank(H)

    PE_CERTIFY_RATIO = 1e-5

    def persistent_excitation_guard(self, u_d):
        """Batched construction-time guard (controller.py:275-296): returns (ok [batch] bool, rank [batch] int).

        Device: `ddmpc_pe_guard` gives a rigorous lower bound of sigma_min/sigma_max of every instance's
        order-(L+2n) input Hankel matrix; a bound above PE_CERTIFY_RATIO (1e-5, nine orders above the SVD
        tolerance max(M,N)*eps and three above the Gram's rounding floor) certifies rank m*(L+2n).
        Host: only the instances left undecided get the reference's exact SVD test (numpy default tolerance)."""
        u_d = np.ascontiguousarray(np.asarray(u_d, dtype=np.float64))
        B, N, m = u_d.shape
        order = self.L + 2 * self.n
        full = m * order
        ratio = np.empty((B,))
        L.check(self._lib.ddmpc_pe_guard(C.c_void_p(u_d.ctypes.data), B, N, m, order, C.c_void_p(ratio.ctypes.data),
                                         L.MEM_HOST, self.device))
        rank = np.full((B,), full, dtype=np.int64)
        undecided = np.nonzero(~(ratio > self.PE_CERTIFY_RATIO))[0]
        if undecided.size:
            H = hankel_matrix_batched(u_d[undecided], order, device=self.device)
            rank[undecided] = np.linalg.matrix_rank(H)
        return rank == full, rank

    def set_setpoints(self, u_s, y_s) -> None:
        us = np.ascontiguousarray(np.asarray(u_s, dtype=np.float64).reshape(-1))
        ys = np.ascontiguousarray(np.asarray(y_s, dtype=np.float64).reshape(-1))
        if us.size != self.m or ys.size != self.p:
            raise ValueError("u_s / y_s must have m / p entries")
        L.check(self._lib.ddmpc_set_setpoints(self._h, C.c_void_p(us.ctypes.data), C.c_void_p(ys.ctypes.data)))
        self._us, self._ys = us, ys

    def set_input_bounds(self, u_min, u_max) -> None:
        """Box on the predicted inputs of the free prediction steps, u_min[ch] <= ubar[k][ch] <= u_max[ch]
        (`ddmpc_set_input_bounds`): arrays of m entries (a scalar is broadcast), -inf / +inf = no bound on that side; both
        None removes the bounds.  ROBUST controllers up to 1024 rows with scalar / diagonal weights; takes effect at the next
        solve and drops what `prepare` kept and the last solution.  Beyond 271 rows: after `set_large_bounds(True)` only (phase
        kernels), and at most the capacity, 64 by default (`set_large_box_capacity`), of boxed components
        -- slack, input, output -- may be active at once: an instance beyond that reports solver_error with NaN outputs."""
        lo = None if u_min is None else np.ascontiguousarray(np.broadcast_to(np.asarray(u_min, dtype=np.float64), (self.m,)))
        hi = None if u_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(u_max, dtype=np.float64), (self.m,)))
        L.check(self._lib.ddmpc_set_input_bounds(self._h, C.c_void_p(lo.ctypes.data) if lo is not None else C.c_void_p(),
                                                 C.c_void_p(hi.ctypes.data) if hi is not None else C.c_void_p()))

    def set_output_bounds(self, y_min, y_max) -> None:
        """Box on the predicted outputs of the free prediction steps, y_min[ch] <= ybar[k][ch] <= y_max[ch]
        (`ddmpc_set_output_bounds`): arrays of p entries (a scalar is broadcast), -inf / +inf = no bound on that side; both
        None removes the bounds.  Same controllers and effects as `set_input_bounds`, and independent of it: either call keeps
        the other's bounds.  The bound is on ybar, not on ybar + sigma; under the CONVEX slack box an infeasible box ends in
        solver_error (there is no infeasibility detection)."""
        lo = None if y_min is None else np.ascontiguousarray(np.broadcast_to(np.asarray(y_min, dtype=np.float64), (self.p,)))
        hi = None if y_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(y_max, dtype=np.float64), (self.p,)))
        L.check(self._lib.ddmpc_set_output_bounds(self._h, C.c_void_p(lo.ctypes.data) if lo is not None else C.c_void_p(),
                                                  C.c_void_p(hi.ctypes.data) if hi is not None else C.c_void_p()))

    def _instance_rows(self, lo, hi, nc: int, what: str):
        """[batch, nc] float64 rows of a per-instance bounds call; None stays None (both: a removal, one: the library refuses it)."""
        rows = []
        for a in (lo, hi):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.shape != (self.batch, nc):
                    raise ValueError("%s: arrays of shape [batch, %d] = (%d, %d) expected, got %s" % (what, nc, self.batch, nc, a.shape))
                a = np.ascontiguousarray(a)
            rows.append(a)
        return rows[0], rows[1]

    def set_instance_input_bounds(self, u_min, u_max) -> None:
        """Input bounds per instance, u_min[b][ch] <= ubar[k][ch] <= u_max[b][ch] (`ddmpc_set_instance_input_bounds`): arrays of
        shape [batch, m], -inf / +inf = no bound on that side for that instance; `None, None` removes the input bounds.  Replaces,
        and is replaced by, `set_input_bounds`; independent of the output bounds.  ROBUST controllers up to 271 rows with scalar /
        diagonal weights; takes effect at the next solve and drops what `prepare` kept and the last solution.  The warm start of
        `set_box_warm_start` is not honoured on such a handle."""
        lo, hi = self._instance_rows(u_min, u_max, self.m, "set_instance_input_bounds")
        L.check(self._lib.ddmpc_set_instance_input_bounds(self._h, C.c_void_p(lo.ctypes.data) if lo is not None else C.c_void_p(),
                                                          C.c_void_p(hi.ctypes.data) if hi is not None else C.c_void_p()))

    def set_instance_output_bounds(self, y_min, y_max) -> None:
        """Output bounds per instance, y_min[b][ch] <= ybar[k][ch] <= y_max[b][ch] (`ddmpc_set_instance_output_bounds`): arrays of
        shape [batch, p]; `None, None` removes the output bounds.  Replaces, and is replaced by, `set_output_bounds`; otherwise as
        `set_instance_input_bounds`."""
        lo, hi = self._instance_rows(y_min, y_max, self.p, "set_instance_output_bounds")
        L.check(self._lib.ddmpc_set_instance_output_bounds(self._h, C.c_void_p(lo.ctypes.data) if lo is not None else C.c_void_p(),
                                                           C.c_void_p(hi.ctypes.data) if hi is not None else C.c_void_p()))

    def set_large_bounds(self, on: bool) -> None:
        """ROBUST controllers beyond 271 rows: True = `set_input_bounds` / `set_output_bounds` are accepted on a handle of
        272 .. 1024 rows (phase kernels; at most the capacity, 64 by default, of boxed components active at once, an instance beyond that reports
        solver_error with NaN outputs), False (default) = both refuse finite bounds at that size (DDMPC_OPT_LARGE_BOUNDS).
        No effect up to 271 rows."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_BOUNDS, 1 if on else 0))

    def set_large_box_capacity(self, k: int) -> None:
        """Bounded handles beyond 271 rows: how many boxed components -- slack, input, output -- may be active at once in an
        iteration (DDMPC_OPT_LARGE_BOX_CAPACITY): 64 (default), 128, 192 or 256; any other value raises.  Costs ldw x k doubles of
        W per instance (ldw: the rows of the trailing block, rounded up to 64) and up to ten 32 KB tiles.  A kept `prepare` stays
        valid; the last solution is forgotten until the next solve.  No effect up to 271 rows or without finite bounds."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_BOX_CAPACITY, int(k)))

    def set_large_box_safeguard(self, on: bool) -> None:
        """Bounded handles beyond 271 rows: True = an instance whose active-set iteration reaches `max_iter` without a stable set is
        solved again inside the same solve / step by the primal active-set method (DDMPC_OPT_LARGE_BOX_SAFEGUARD; `iters` =
        max_iter + its solves; its working sets must fit the capacity, `set_large_box_capacity`), False (default) = solver_error at
        the cap.  With True the wide kernels serve the handle at every capacity.  A kept `prepare` stays valid; the last solution is
        forgotten until the next solve.  No effect up to 271 rows or without finite bounds."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_BOX_SAFEGUARD, 1 if on else 0))

    def set_box_safeguard(self, on: bool) -> None:
        """Input / output bounds: True = an instance whose active-set iteration reaches `max_iter` without a stable set is finished by a
        primal active-set method instead of reporting solver_error (DDMPC_OPT_BOX_SAFEGUARD; `iters` = max_iter + its solves),
        False (default) = solver_error at the cap.  Instances below the cap are unchanged; no effect without finite bounds;
        a kept `prepare` stays valid."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_BOX_SAFEGUARD, 1 if on else 0))

    def set_box_warm_start(self, on: bool) -> None:
        """Input / output bounds up to 271 rows: True = `step` (`solve(..., warm=True)`) and the fused `closed_loop` start the
        active-set iteration from the signed set the last solve of the handle ended with instead of the empty set
        (DDMPC_OPT_BOX_WARM_START); a seeded run that fails starts again from the empty set, so the status is never worse.
        Results agree with False to rounding, `iters` is what the seeded run took.  The first solve after `prepare` and every
        cold `solve` start from the empty set and are bit-equal to False.  Setting it (either value) drops the seed, as do
        `set_data`, `set_setpoints`, `set_input_bounds`, `set_output_bounds` and a new `prepare`.  False (default) = every solve
        from the empty set.  A kept `prepare` stays valid; no effect beyond 271 rows, without finite bounds or on a slack-only
        CONVEX handle."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_BOX_WARM_START, 1 if on else 0))

    def set_large_box_warm_start(self, on: bool) -> None:
        """Bounded handles beyond 271 rows: True = `step` (`solve(..., warm=True)`) and the per-step `closed_loop` start the
        active-set iteration from the signed set the last solve of the handle ended with instead of the empty set
        (DDMPC_OPT_LARGE_BOX_WARM_START); a seeded run that fails starts again from the empty set, so the status is never worse.
        Results agree with False to rounding, `iters` is every solve attempted.  The first step after `prepare` and every cold
        `solve` start from the empty set.  Setting it (either value) drops the seed, as do `set_data`, `set_setpoints`,
        `set_input_bounds`, `set_output_bounds`, a new `prepare`, `set_large_bounds`, `set_large_box_capacity` and
        `set_large_box_safeguard`.  With True the wide kernels serve the handle at every capacity.  A kept `prepare` stays valid;
        the last solution is forgotten until the next solve.  No effect up to 271 rows, without finite bounds or on a slack-only
        CONVEX handle."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_BOX_WARM_START, 1 if on else 0))

    def set_large_box_law(self, on: bool) -> None:
        """Bounded handles beyond 271 rows: True = `prepare` also forms the affine law of the empty active set on the kept factor
        ((n(m+p) + 1) r doubles per instance) and `step` (`solve(..., warm=True)`) and the per-step `closed_loop` serve every
        instance whose law violates no component of the box from it in one launch (`iters` = 1; agrees with the solve to
        rounding); every other instance of the batch is solved in the same call by the launches of False restricted to it and is
        bit-equal to False (DDMPC_OPT_LARGE_BOX_LAW).  `gain()` returns the law after `prepare`.  Cold `solve`s never use the law.
        Setting it (either value) forgets what `prepare` kept, the last solution and the seed of `set_large_box_warm_start`.
        Raises beyond 271 rows when n(m+p) > 256.  False (default) = every step is the whole solve.  No effect up to 271 rows,
        without finite bounds or on a slack-only CONVEX handle."""
        L.check(self._lib.ddmpc_set_option(self._h, L.OPT_LARGE_BOX_LAW, 1 if on else 0))

    def get_solution(self, what: str) -> np.ndarray:
        """`.value` of alpha / ubar / ybar / sigma after the last solve (host array)."""
        sel = {"alpha": L.SOL_ALPHA, "ubar": L.SOL_UBAR, "ybar": L.SOL_YBAR, "sigma": L.SOL_SIGMA}[what]
        Ln = self.L + self.n
        per = {"alpha": self.N - Ln + 1, "ubar": Ln * self.m, "ybar": Ln * self.p, "sigma": Ln * self.p}[what]
        out = np.empty((self.batch, per))
        L.check(self._lib.ddmpc_get_solution(self._h, sel, C.c_void_p(out.ctypes.data), L.MEM_HOST))
        return out

    def synchronize(self) -> None:
        L.check(self._lib.ddmpc_synchronize(self._h))

    def cost_model(self) -> Tuple[float, float]:
        f, b = C.c_double(), C.c_double()
        L.check(self._lib.ddmpc_cost_model(self._h, C.byref(f), C.byref(b)))
        return f.value, b.value

    def debug_stamps(self, enable: bool = True, fetch: bool = False):
        """Diagnostics: enable in-kernel phase stamps / fetch those of the last solve ([batch,16] uint64)."""
        out = np.zeros((self.batch, 16), dtype=np.uint64) if fetch else None
        L.check(self._lib.ddmpc_debug_stamps(self._h, 1 if enable else 0,
                                             C.c_void_p(out.ctypes.data) if fetch else C.c_void_p()))
        return out

    def kernel_name(self) -> str:
        return self._lib.ddmpc_kernel_name(self._h).decode()

    def closed_loop_kernel_name(self) -> str:
        """The kernel that stepped the plant in the last `closed_loop`: one of the fused loops, or 'ddmpc_plant_kernel'
        when the loop ran per step; 'ddmpc_closed_loop_setpoint_kernel' after `closed_loop_setpoints`
        ('ddmpc_closed_loop_setpoint_box_kernel' on a handle with bounds, 'ddmpc_closed_loop_setpoint_convex_kernel' under
        `set_setpoint_convex_law`)."""
        return self._lib.ddmpc_closed_loop_kernel_name(self._h).decode()


def hankel_matrix_batched(X: np.ndarray, L_: int, device: int = 0) -> np.ndarray:
    """Batched hankel_matrix on the GPU: X [B,N,nch] -> [B, L*nch, N-L+1]."""
    lib = L.load()
    X = np.ascontiguousarray(X, dtype=np.float64)
    B, N, nch = X.shape
    if N < L_:
        raise ValueError("N must be greater than or equal to L.")
    H = np.empty((B, L_ * nch, N - L_ + 1))
    L.check(lib.ddmpc_hankel(C.c_void_p(X.ctypes.data), B, N, nch, L_, C.c_void_p(H.ctypes.data), L.MEM_HOST, device))
    return H
