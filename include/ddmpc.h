/*
 * ddmpc.h -- C ABI of the MI355X-native batched Data-Driven MPC QP engine.
 *
 * This is the drop-in boundary for the per-timestep QP path of
 * pavelacamposp/direct_data_driven_mpc.  The reference has no FFI of its own
 * (it is pure Python on CVXPY); each entry point below names the reference
 * interface it replaces (file:line relative to the reference repository root).
 * A Python `ctypes` shim (direct_data_driven_mpc_amd/_lib.py) binds exactly
 * these symbols and re-creates the `DirectDataDrivenMPCController` class
 * surface on top of them; INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every function returns 0 (DDMPC_OK) or a negative DDMPC_ERR_* code and
 *     never throws; `ddmpc_last_error()` returns a thread-local message;
 *   - plain pointers and sizes only; all arrays are C-order fp64 unless noted;
 *   - `mem` says where the caller's buffers live: DDMPC_MEM_HOST (the library
 *     stages them through its own device buffers and the call is synchronous)
 *     or DDMPC_MEM_DEVICE (HIP device pointers, the call is asynchronous on
 *     the handle's stream);
 *   - one handle = one batch of `batch` independent controller instances that
 *     share the controller parameters and differ in their data trajectories
 *     and past windows.  A bad instance never fails a call: it gets a
 *     per-instance status code.
 *   - there is NO CPU fallback: without a HIP device every call fails with
 *     DDMPC_ERR_NO_DEVICE.
 */
#ifndef DDMPC_H
#define DDMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDMPC_ABI_VERSION 2

/* return codes */
#define DDMPC_OK                 0
#define DDMPC_ERR_INVALID       -1  /* bad argument (message says which)            */
#define DDMPC_ERR_UNSUPPORTED   -2  /* valid request the HIP path does not cover     */
#define DDMPC_ERR_NO_DEVICE     -3  /* no usable HIP device                          */
#define DDMPC_ERR_HIP           -4  /* a HIP runtime call failed                     */
#define DDMPC_ERR_NOT_READY     -5  /* e.g. solve before set_data                    */

/* DataDrivenMPCType, direct_data_driven_mpc_controller.py:11-14 */
#define DDMPC_NOMINAL 0
#define DDMPC_ROBUST  1
/* SlackVarConstraintTypes, direct_data_driven_mpc_controller.py:16-20 */
#define DDMPC_SLACK_NON_CONVEX 0    /* rejected, controller.py:664-670 */
#define DDMPC_SLACK_CONVEX     1
#define DDMPC_SLACK_NONE       2

/* per-instance solve status; maps 1:1 onto the CVXPY strings the reference
 * tests for in get_optimal_control_input (controller.py:804-808) */
#define DDMPC_STATUS_OPTIMAL            0   /* "optimal"            */
#define DDMPC_STATUS_OPTIMAL_INACCURATE 1   /* "optimal_inaccurate" */
#define DDMPC_STATUS_INFEASIBLE         2   /* "infeasible"         */
#define DDMPC_STATUS_UNBOUNDED          3   /* "unbounded"          */
#define DDMPC_STATUS_SOLVER_ERROR       4   /* "solver_error"       */

#define DDMPC_WEIGHT_SCALAR 0       /* Q = q*I, R = r*I (what the reference loader builds,
                                       utilities/controller/controller_creation.py:125-127) */
#define DDMPC_WEIGHT_DIAG   1       /* Q = diag(q[0..p*L)), R = diag(r[0..m*L)); entries >= 0 (a zero weight leaves the
                                       component free) */
#define DDMPC_WEIGHT_DENSE  2       /* Q [p*L, p*L], R [m*L, m*L] row-major, symmetric; on the free prediction steps positive
                                       definite once all-zero rows / columns (components without a weight, as zeros on the
                                       diagonal of a DIAG matrix) are set aside (controller.py:121-124,708-710); every slack
                                       mode.  A null space that is not spanned by coordinate axes: DDMPC_ERR_UNSUPPORTED */

#define DDMPC_MEM_HOST   0
#define DDMPC_MEM_DEVICE 1

#define DDMPC_GRAM_AUTO       0     /* = STRUCTURED                                      */
#define DDMPC_GRAM_DENSE      1     /* H H' by fp64 MFMA over the implicit Hankel operand */
#define DDMPC_GRAM_STRUCTURED 2     /* Hankel sliding-window recurrence (hankel_matrix.py:5-53 is generic in the channel count
                                       and so is this: inside the cold-solve kernel for m + p == 2 or 4, by a launch ahead of
                                       it for any other count)                              */

/* ddmpc_get_solution selectors: the `.value` of the reference's cp.Variables
 * (controller.py:434-445) */
#define DDMPC_SOL_ALPHA 0           /* [batch, N-L-n+1]   */
#define DDMPC_SOL_UBAR  1           /* [batch, (L+n)*m]   */
#define DDMPC_SOL_YBAR  2           /* [batch, (L+n)*p]   */
#define DDMPC_SOL_SIGMA 3           /* [batch, (L+n)*p], robust only */

/* ddmpc_set_option */
#define DDMPC_OPT_CLOSED_LOOP_PATH 1
#define DDMPC_PATH_AUTO 0           /* warm: fused loop without inequality; per-step warm + cold re-solves with the slack box */
#define DDMPC_PATH_COLD 1           /* a full cold solve per control step                         */
#define DDMPC_PATH_WARM 2
#define DDMPC_OPT_CLOSED_LOOP_GRAPH 2 /* 1: record the per-step launches of ddmpc_closed_loop into a HIP graph and replay it
                                         (default 0: measured slower than plain asynchronous launches) */

#define DDMPC_OPT_REFINE 3            /* iterative refinement of the cold solve with exact Hankel products (residual
                                         t - (H(H'beta) + lam D beta) from the trajectory, correction through the factor at hand):
                                         0 off, 1 auto (default: every solve is checked with that residual, relative to |t|,
                                         and only the instances above the threshold are solved again with refinement),
                                         2 always.  Passes repeat until the correction is at rounding level or stops shrinking.
                                         ddmpc_prepare forms the affine law of ddmpc_step from refining solves as well
                                         (n(m+p)+1 launches, once per data set): with 2 for every instance, with 1 for the
                                         instances it flags; changing the mode invalidates the law. */
#define DDMPC_REFINE_OFF 0
#define DDMPC_REFINE_AUTO 1
#define DDMPC_REFINE_ALWAYS 2
#define DDMPC_OPT_REFINE_MAX 4        /* cap on refinement passes per factorisation (default 3) */
#define DDMPC_OPT_REFINE_RES_LOG10 5  /* auto mode: refine when |t - (H(H'beta) + lam D beta)|_inf / |t|_inf exceeds
                                         10^(-value/10), value in tenths of a decade below 1 (default DDMPC_REFINE_RES_DEFAULT;
                                         3000 refines everything, 0 only what comes out non-finite) */
#define DDMPC_OPT_LARGE_PIPELINE 6     /* NOMINAL controllers beyond the register-resident kernels ((m+p)(L+n) > 271): how the
                                         data-dependent half of a solve (Gram, rank-revealing Cholesky, C'WC and its factor;
                                         controller.py:506-538) is executed -- results agree to rounding */
#define DDMPC_PIPELINE_ONE_WORKGROUP 0 /* one workgroup per instance runs every phase (ddmpc_nominal_rr_kernel<1>) */
#define DDMPC_PIPELINE_PHASES 1        /* default: one kernel per phase over the whole batch in lock step, several workgroups
                                         per instance, Cholesky by 64-column panels (ddmpc_rr2.hpp) */
#define DDMPC_OPT_LARGE_AFFINE_LAW 7   /* NOMINAL controllers beyond the register-resident kernels, phase-kernel pipeline: 1 = ddmpc_prepare also
                                         forms the affine control law z(past) (solves at the zero window and the n(m+p) unit windows,
                                         once per data set) and ddmpc_step evaluates it in one HBM-bound launch; ddmpc_get_gain then
                                         returns it as [batch][n(m+p)+1][(m+p)(L+n)], z = [ubar; ybar] per component = gain[0] +
                                         gain[1:]' [u_past; y_past].  0 (default): ddmpc_step repeats the solve on the kept factors,
                                         bit-equal to ddmpc_solve (controller.py:389-407).  Scalar / diagonal weights, at most 1024
                                         rows (DDMPC_ERR_UNSUPPORTED otherwise).
                                         ROBUST controllers beyond the register-resident kernels (phase kernels, 272 .. 1024 rows): 1 =
                                         ddmpc_prepare also forms the law of beta of the EMPTY active set on the kept factor K0,
                                         beta(w) = g0 + G'w, w = [u_past; y_past] (the solution of K0 beta = t(w)), refined
                                         with exact Hankel products under DDMPC_OPT_REFINE (off: plain substitution; auto: the instances
                                         whose law residual exceeds the threshold; always: every instance; an instance still above the
                                         threshold after DDMPC_OPT_REFINE_MAX passes has no law and its steps take the re-solve below).
                                         ddmpc_get_gain returns it as [batch][n(m+p)+1][(m+p)(L+n)], beta per component (rho = k(m+p)+ch)
                                         = gain[0] + gain[1:]' [u_past; y_past]: the layout and meaning of a ROBUST gain below 272 rows
                                         (the NOMINAL law above is z, not beta).  ddmpc_step evaluates the law in one HBM-bound launch and
                                         writes outputs, beta / active-set workspace and the rr3 record (ddmpc_get_solution,
                                         ddmpc_debug_workspace); with the CONVEX slack box an instance whose boxed slacks all stay within
                                         c eps_max is optimal as it is (iters 1), the others are re-solved in the same call on the kept
                                         factors, like ddmpc_solve (same iterations, statuses, solutions to rounding).  Scalar / diagonal
                                         weights, at most 1024 rows, n(m+p) <= 256 (DDMPC_ERR_UNSUPPORTED otherwise); no effect with
                                         DDMPC_PIPELINE_ONE_WORKGROUP (ddmpc_get_gain: DDMPC_ERR_NOT_READY) */
#define DDMPC_OPT_CONVEX_UPDATE 8      /* ROBUST controllers with the CONVEX slack box on the register-resident kernels
                                         (controller.py:631-677): 1 (default) = active-set iterations after the first keep the factor
                                         of the empty active set and treat the <= 4 switched slack components as a diagonal modification
                                         of rank k (Woodbury: one block forward substitution on the matrix pipe, a k x k system, one
                                         back substitution); more components, or anything unusual, falls back to 0 = the whole system is
                                         formed and factored again in every iteration (rounds 1-4).  Same active sets, iteration
                                         counts and -- to rounding -- solutions */
#define DDMPC_OPT_GRAM_LAUNCH 9        /* register-resident kernels, structured Gram of plants with other than two or four channels
                                         (hankel_matrix.py:5-53): which launch ahead of the solve forms the Gram tiles.  0 = the
                                         streaming matrix-pipe kernel (trajectory in chunks, several lags per tile for at most eight
                                         channels; the default from six channels on, and what trajectories beyond the LDS take), 1 = the
                                         launch of round 4 that stages the whole trajectory and walks on the vector units (the default
                                         up to five channels).  Same tiles to rounding; DDMPC_ERR_UNSUPPORTED when the requested launch
                                         cannot hold the shape */
#define DDMPC_OPT_CONVEX_WARM_LAW 10     /* ROBUST controllers with the CONVEX slack box on the register-resident kernels: 1 = ddmpc_prepare
                                         also forms M = K0^-1 E_box per instance (K0 the system of the empty active set, E_box the unit
                                         vectors of the p*L boxed slack components; [batch][p*L][(m+p)(L+n)] doubles, 65 KB per instance
                                         at L = 30, m = p = 2, plus p*L(p*L+1)/2 doubles of k x k scratch when p*L > 16), and ddmpc_step /
                                         ddmpc_closed_loop (paths AUTO and WARM) run the whole primal-dual active-set iteration on the law
                                         and M: no cold re-solve, no read of the trajectories.  Same active sets, iteration counts, status
                                         and -- to rounding -- solutions as ddmpc_solve.  Instances whose law ddmpc_prepare formed from
                                         refining solves (DDMPC_REFINE_ALWAYS: all; AUTO: those it flags) keep today's route: ddmpc_step
                                         re-solves those whose law leaves the box with the filtered cold launch, and ddmpc_closed_loop
                                         takes the per-step path when there is any.  0 (default) = the filtered cold re-solve.  Setting
                                         it invalidates the prepared law.  DDMPC_ERR_UNSUPPORTED with dense weights, beyond 271 rows and
                                         for a boxed output component without weight (Q entry 0); no effect without the slack box */
#define DDMPC_OPT_BOX_SAFEGUARD 11      /* (no effect beyond 271 rows) handles with input bounds (ddmpc_set_input_bounds): 1 = an instance whose primal-dual active-set
                                         iteration reaches max_iter without a stable set is not reported DDMPC_STATUS_SOLVER_ERROR but
                                         solved again, in the same launch, by a primal active-set method on the same law, M and box
                                         table (one component enters or leaves the working set per solve, the cost falls with every
                                         move: it ends at the optimum of the strictly convex QP).  It starts from the
                                         empty set, so the result does not depend on max_iter; `iters` reports max_iter plus its solves
                                         (at most 4 nbox + 16, status 4 there or on a non-positive pivot).  Instances that converge
                                         below the cap are bit-equal to 0 in inputs, cost, status and iters.  Honoured by ddmpc_solve,
                                         ddmpc_step and ddmpc_closed_loop (both paths; in the fused loop such an instance carries on).
                                         0 (default) = status 4 at the cap.  Values other than 0 / 1: DDMPC_ERR_INVALID.  Accepted on
                                         any handle, no effect without finite bounds; keeps what ddmpc_prepare kept.  A CONVEX handle
                                         without bounds keeps the slack-only kernels and is not covered: one finite bound puts it on
                                         this route */
#define DDMPC_OPT_LARGE_BOUNDS 12       /* ROBUST controllers beyond 271 rows: 1 = ddmpc_set_input_bounds / ddmpc_set_output_bounds are accepted
                                         on a handle of 272 .. 1024 rows that the phase kernels serve ("Bounds beyond 271 rows" at
                                         ddmpc_set_input_bounds: at most the capacity, 64 by default, of components active at once;
                                         DDMPC_OPT_LARGE_BOX_CAPACITY).  0 (default) = both calls
                                         refuse finite bounds beyond 271 rows with DDMPC_ERR_UNSUPPORTED, as they did before the
                                         option existed; the message names the option.  Opt-in because the limits of that route
                                         (the capacity, no safeguard) are not those of the register-resident one.  Accepted
                                         on any handle, no effect up to 271 rows; 0 on a bounded handle beyond 271 rows is
                                         DDMPC_ERR_UNSUPPORTED (remove the bounds first).  Values other than 0 / 1: DDMPC_ERR_INVALID */
#define DDMPC_OPT_LARGE_BOX_CAPACITY 13 /* bounded handles beyond 271 rows (DDMPC_OPT_LARGE_BOUNDS): the number of components (slack + input +
                                         output) that may be active at once in an iteration = the columns of W kept per instance:
                                         64 (default), 128, 192 or 256; any other value is DDMPC_ERR_INVALID.  64 launches
                                         rr3_solve_box_kernel as before the option existed; above 64 rr3_solve_box_wide_kernel
                                         (the same factor, update, iteration rule and refinement pass; the k x k system as 64 x 64
                                         tiles with a blocked Cholesky) serves ddmpc_solve, ddmpc_step, the per-step
                                         ddmpc_closed_loop and ddmpc_get_solution.  Memory per instance: W, ldw x capacity doubles
                                         (ldw = the rows of the trailing block rounded up to 64: 1.3 MB at 608 rows with every input
                                         channel bounded and capacity 256, 0.67 GB at 512 instances), and up to 10 tiles of 32 KB; an
                                         allocation failure is DDMPC_ERR_HIP at the next solve.  Accepted on any handle; no effect up
                                         to 271 rows or without finite bounds.  Keeps what ddmpc_prepare kept (the factors do not
                                         depend on it) and forgets the last solution: ddmpc_get_solution is DDMPC_ERR_NOT_READY
                                         until the next solve, as after ddmpc_set_input_bounds */
#define DDMPC_OPT_LARGE_BOX_SAFEGUARD 14 /* bounded handles beyond 271 rows (DDMPC_OPT_LARGE_BOUNDS): 1 = an instance whose primal-dual
                                         iteration reaches max_iter without a stable set is solved again inside the same ddmpc_solve /
                                         ddmpc_step call by the primal active-set method of DDMPC_OPT_BOX_SAFEGUARD, stated on the
                                         reduced system of this route (rr3_box_safeguard_kernel): from the empty
                                         set's solution, so the result does not depend on max_iter; one component joins or leaves
                                         the working set per solve; `iters` = max_iter + its solves.  An instance that failed on a
                                         pivot or outgrew the capacity is not solved again.  Status 4 with NaN in u_opt / cost and
                                         `iters` = max_iter + the number (from 1) of the solve that could not be made: more than
                                         4 nbox + 16 solves, a non-positive pivot of the k x k system, a working set larger than
                                         DDMPC_OPT_LARGE_BOX_CAPACITY (the set of the first solve holds every component the empty
                                         set's solution violates).  With 1 the wide kernels serve the handle at every capacity: above
                                         64 an instance that converges below max_iter is bit-equal to 0 in inputs, cost, status and
                                         iters; at capacity 64 it agrees to rounding only (4e-15 measured: the wide kernel forms the
                                         right-hand side of the k x k system differently).  Memory per instance on top of the
                                         capacity's: a second set of tiles, nbox + 16 ldw doubles.  0 (default) = status 4 at the cap.
                                         Values other than 0 / 1: DDMPC_ERR_INVALID.  Accepted on any handle; no effect up to 271
                                         rows, without finite bounds or off the phase kernels; keeps what ddmpc_prepare kept and
                                         forgets the last solution.  A slack-only CONVEX handle is not covered */
#define DDMPC_OPT_BOX_WARM_START 15     /* bounded handles up to 271 rows (ddmpc_set_input_bounds / ddmpc_set_output_bounds): 1 = ddmpc_step and
                                         the fused ddmpc_closed_loop start the primal-dual active-set iteration from the signed set
                                         the last solve of the handle ended with (ddmpc_step, ddmpc_solve or ddmpc_closed_loop; in the
                                         fused loop the set also passes from one solve of the loop to the next), not from the empty
                                         set.  The law is still tested under the empty set first: no violation is `iters` = 1 and an
                                         empty seed.  With a violation and a non-empty seed the seed is solved for (solve number 2)
                                         and the usual test / solve loop goes on under the max_iter cap.  A seeded run that meets a
                                         non-positive pivot, or ends at the cap, starts again from the empty set with a fresh cap --
                                         the status is never worse than with 0 -- except that at the cap with
                                         DDMPC_OPT_BOX_SAFEGUARD = 1 it goes straight to the safeguard; `iters` counts every solve
                                         made, the law once.  The optimum does not depend on the seed: results agree with 0 to
                                         rounding, `iters` differs.  The first solve after ddmpc_prepare has no seed and is bit-equal
                                         to 0; so are ddmpc_solve and DDMPC_PATH_COLD (always from the empty set; they leave a
                                         seed for a following ddmpc_step).  The seed is dropped by everything that makes
                                         ddmpc_get_solution report DDMPC_ERR_NOT_READY on this route (ddmpc_set_data,
                                         ddmpc_set_setpoints, ddmpc_set_input_bounds, ddmpc_set_output_bounds, a new ddmpc_prepare) and
                                         by setting this option to either value; an instance whose solve ended with status > 1
                                         leaves an empty seed.  One byte per boxed component and instance.  0 (default) = every solve
                                         from the empty set, the kernels as they were.  Values other than 0 / 1: DDMPC_ERR_INVALID.
                                         Accepted on any handle; keeps what ddmpc_prepare kept and the last solution.  No effect
                                         beyond 271 rows, without finite bounds, and on a slack-only CONVEX handle (it keeps the
                                         slack-only kernels, as for DDMPC_OPT_BOX_SAFEGUARD) */
#define DDMPC_OPT_LARGE_BOX_WARM_START 16 /* bounded handles beyond 271 rows (DDMPC_OPT_LARGE_BOUNDS): 1 = ddmpc_step and the per-step
                                         ddmpc_closed_loop (DDMPC_PATH_AUTO / _WARM) start the primal-dual iteration from the signed
                                         set the last solve of the handle ended with (ddmpc_step, ddmpc_solve or a step of the loop),
                                         not from the empty set: the rule of DDMPC_OPT_BOX_WARM_START on the reduced system of this
                                         route.  The empty set is still solved and tested first: no violation is
                                         `iters` = 1 and an empty seed.  With a violation and a non-empty seed the seed is solved for
                                         (solve number 2) and the usual test / solve loop goes on under the max_iter cap.  A seeded
                                         run that meets a non-positive pivot, more active components than the capacity, or the cap
                                         starts again from the empty set with a fresh cap -- the status is never worse than with 0 --
                                         except that at the cap with DDMPC_OPT_LARGE_BOX_SAFEGUARD = 1 it goes straight to the
                                         safeguard (`iters` = max_iter + its solves, bit-equal to 0); `iters` counts every solve
                                         attempted, the empty set's once.  The optimum does not depend on the seed: results agree
                                         with 0 to rounding, `iters` differs.  The first step after ddmpc_prepare has no seed;
                                         ddmpc_solve and DDMPC_PATH_COLD always start from the empty set and leave a seed for a
                                         following ddmpc_step.  Without a seed a call is bit-equal to 0 above capacity 64; with 1
                                         the wide kernels serve the handle at every capacity, so at capacity 64 it agrees with 0
                                         to rounding only (as DDMPC_OPT_LARGE_BOX_SAFEGUARD).  The seed is dropped by ddmpc_set_data,
                                         ddmpc_set_setpoints, ddmpc_set_input_bounds, ddmpc_set_output_bounds, a new ddmpc_prepare
                                         (the factors are new) and by setting DDMPC_OPT_LARGE_BOUNDS, _LARGE_BOX_CAPACITY,
                                         _LARGE_BOX_SAFEGUARD or this option to any value; an instance whose call ended with
                                         status > 1 leaves an empty seed, one finished by the safeguard the safeguard's final set.
                                         A stale seed may cost solves and never changes a result.  One byte per row and instance.
                                         0 (default) = every solve from the empty set, the kernels as they were.  Values other than
                                         0 / 1: DDMPC_ERR_INVALID.  Accepted on any handle; keeps what ddmpc_prepare kept and forgets
                                         the last solution (the record layout may change), as DDMPC_OPT_LARGE_BOX_CAPACITY.  No
                                         effect up to 271 rows (DDMPC_OPT_BOX_WARM_START is the option of that size and has no
                                         effect here), without finite bounds, off the phase kernels, and on a slack-only CONVEX
                                         handle (it keeps rr3_solve_kernel) */
#define DDMPC_OPT_LARGE_BOX_LAW 17       /* bounded handles beyond 271 rows (DDMPC_OPT_LARGE_BOUNDS): 1 = ddmpc_prepare also forms the
                                         affine law of the EMPTY active set on the kept factor (beta = g0 + G' w; the kernels,
                                         refinement under DDMPC_OPT_REFINE and "no law" marking after DDMPC_OPT_REFINE_MAX passes of
                                         DDMPC_OPT_LARGE_AFFINE_LAW; (n(m+p) + 1) r doubles per instance, an allocation failure is
                                         DDMPC_ERR_HIP), and ddmpc_step and the per-step ddmpc_closed_loop (DDMPC_PATH_AUTO / _WARM)
                                         run one launch on that law first.  An instance that has a law and whose beta violates no
                                         component of the box table -- hat = a + c beta strictly above hi or strictly below lo; slack,
                                         input and output components alike, the first test of the bounded kernels -- is served by
                                         that launch: status 0, `iters` = 1, u_opt, cost, the empty active set in the workspace
                                         (ddmpc_get_solution and ddmpc_debug_workspace read it like any other step) and, under
                                         DDMPC_OPT_LARGE_BOX_WARM_START, an empty seed.  Such a result agrees with the option 0 to
                                         rounding (1e-9 relative: the law is not the solve).  Every other instance (a violation, or
                                         no law) is solved in the same call by exactly the launches of the option 0 restricted to
                                         it -- at the handle's capacity, seeded, with the safeguard and the refinement launch as set
                                         -- and is bit-equal to the option 0 in u_opt, cost, status, iters, the solution and the
                                         seed it leaves.  ddmpc_solve and DDMPC_PATH_COLD keep the cold contract and never use the
                                         law.  ddmpc_get_gain returns the law on such a handle (the layout of a ROBUST gain: beta of
                                         the empty active set in component order; DDMPC_ERR_NOT_READY before ddmpc_prepare).
                                         0 (default) = every step is the whole solve, the kernels as they were.  Values other than
                                         0 / 1: DDMPC_ERR_INVALID; 1 beyond 271 rows with n(m+p) > 256: DDMPC_ERR_UNSUPPORTED.
                                         Setting it, to either value, forgets what ddmpc_prepare kept (the law is part of it), the
                                         last solution and the seed; with 1, DDMPC_OPT_REFINE_MAX forgets the preparation too.
                                         Accepted on any other handle; no effect up to 271 rows (such a handle is always on the
                                         law), without finite bounds, off the phase kernels, and on a slack-only CONVEX handle (it
                                         keeps rr3_solve_kernel: DDMPC_OPT_LARGE_AFFINE_LAW is its option, and stays refused with
                                         bounds) */
#define DDMPC_OPT_SETPOINT_LAW 18        /* ROBUST controllers on the register-resident kernels, slack NONE, scalar / diagonal weights:
                                         1 = ddmpc_prepare also forms S = K0^-1 [1_0 .. 1_{m+p-1}], the response of beta to the
                                         setpoint of every channel ((m+p) r doubles per instance: 4.4 KB at L = 30, n = 4, m = p = 2,
                                         18 MB at 4096 instances; an allocation failure is DDMPC_ERR_HIP), which makes the setpoint an
                                         argument of the step like the past window: ddmpc_step_setpoints, ddmpc_closed_loop_setpoints
                                         and ddmpc_get_setpoint_gain (see there).  The columns of S are refined exactly as the columns
                                         of the law are (DDMPC_OPT_REFINE).  With 1, ddmpc_solve, ddmpc_step, ddmpc_closed_loop,
                                         ddmpc_get_gain and ddmpc_get_solution launch what they launch with 0 and return bit-equal
                                         results.  0 (default): nothing is formed, the three calls are DDMPC_ERR_UNSUPPORTED.  Values
                                         other than 0 / 1: DDMPC_ERR_INVALID.  Changing the value forgets what ddmpc_prepare kept.
                                         Setting 1 is DDMPC_ERR_UNSUPPORTED, with a message that names the reason, on NOMINAL
                                         controllers, with the CONVEX slack box, with DDMPC_WEIGHT_DENSE, beyond 271 rows, on a
                                         trajectory beyond the LDS, with n(m+p) > 256 and on a handle with input or output bounds;
                                         in the reverse order ddmpc_set_input_bounds / ddmpc_set_output_bounds refuse finite bounds
                                         on a handle with the option on (unless DDMPC_OPT_SETPOINT_BOX_LAW = 1, below).  CONVEX
                                         handles: DDMPC_OPT_SETPOINT_CONVEX_LAW */
#define DDMPC_OPT_SETPOINT_BOX_LAW 19    /* DDMPC_OPT_SETPOINT_LAW for handles that carry input / output bounds (up to 271 rows): 1 =
                                         ddmpc_prepare forms S next to the law and M = K0^-1 E_box (S comes from the empty set's
                                         system and knows no bounds; its columns are refined under DDMPC_REFINE_AUTO as those of the
                                         law are), and ddmpc_step_setpoints / ddmpc_closed_loop_setpoints / ddmpc_get_setpoint_gain
                                         are open.  M does not depend on the setpoint; per instance the setpoint enters the law, the
                                         offsets a_s of the boxed components and the target of the output stage.  Without a finite
                                         bound the calls launch exactly what they launch under DDMPC_OPT_SETPOINT_LAW, bit-equal;
                                         with finite bounds ddmpc_step_setpoints is one launch of "ddmpc_setpoint_box_step_kernel"
                                         (law, violation test, the primal-dual iteration of ddmpc_step on M with the same rule,
                                         max_iter cap and statuses, DDMPC_OPT_BOX_SAFEGUARD honoured, output stage) and
                                         ddmpc_closed_loop_setpoints one fused launch of "ddmpc_closed_loop_setpoint_box_kernel"
                                         (n_mpc_step * m > 256: DDMPC_ERR_UNSUPPORTED).  `iters` counts as in ddmpc_step.  Per
                                         instance: a non-finite setpoint is DDMPC_STATUS_SOLVER_ERROR; with the terminal constraint a
                                         setpoint outside [u_min, u_max] / [y_min, y_max] of its channel is DDMPC_STATUS_INFEASIBLE
                                         with u_opt and cost NaN and iters 0 (in the loop the instance stops there); neighbours are
                                         untouched.  Without the terminal constraint a setpoint outside the box is legitimate.
                                         Finite bounds are accepted on a handle with the option on, and the option on a bounded
                                         handle; with DDMPC_OPT_SETPOINT_LAW = 1 as well this option governs, and with only that
                                         one on the bounds stay refused.  ddmpc_solve, ddmpc_step, ddmpc_closed_loop, ddmpc_get_gain
                                         and ddmpc_get_solution launch what they launch with 0 and return bit-equal results.
                                         0 (default).  Values other than 0 / 1: DDMPC_ERR_INVALID.  Changing the value forgets what
                                         ddmpc_prepare kept.  Setting 1 is DDMPC_ERR_UNSUPPORTED, with a message that names the
                                         reason, on NOMINAL controllers, with the CONVEX slack box, with DDMPC_WEIGHT_DENSE, beyond
                                         271 rows (the phase kernels have no M), on a trajectory beyond the LDS and with
                                         n(m+p) > 256.  CONVEX handles, slack-only or with bounds: DDMPC_OPT_SETPOINT_CONVEX_LAW,
                                         below.  LIMITS: the bounds are the handle's, not per instance; the iteration of the new calls always starts
                                         from the empty set (DDMPC_OPT_BOX_WARM_START is not honoured, and the calls drop the seed);
                                         ddmpc_get_solution after them is DDMPC_ERR_NOT_READY; DDMPC_REFINE_ALWAYS stays refused on
                                         bounded handles */
#define DDMPC_OPT_SETPOINT_CONVEX_LAW 20 /* DDMPC_OPT_SETPOINT_LAW / _SETPOINT_BOX_LAW for ROBUST controllers with the CONVEX slack box
                                         (scalar / diagonal weights, up to 271 rows), slack-only or with input and / or output
                                         bounds; the option and the bounds are accepted in either order.  1 = ddmpc_prepare forms S
                                         next to the law (from the empty set's system, which knows neither the slack box nor the
                                         bounds; refined as the law's columns are) and ddmpc_step_setpoints /
                                         ddmpc_closed_loop_setpoints / ddmpc_get_setpoint_gain are open.  On a slack-only handle
                                         ddmpc_prepare also forms the box list of the slack components, its table and
                                         M = K0^-1 E_box, whether or not DDMPC_OPT_CONVEX_WARM_LAW is on: L p r doubles per instance
                                         (65 KB at L = 30, n = 4, m = p = 2: 0.27 GB at 4096 instances; an allocation failure is
                                         DDMPC_ERR_HIP); a bounded handle has them already.  ddmpc_step_setpoints is one launch of
                                         ddmpc_setpoint_box_step_kernel, ddmpc_closed_loop_setpoints one fused launch of
                                         ddmpc_closed_loop_setpoint_box_kernel, each in its slack-box instantiation (the loop is
                                         labelled "ddmpc_closed_loop_setpoint_convex_kernel"; n_mpc_step * m > 256: DDMPC_ERR_UNSUPPORTED):
                                         the primal-dual iteration of ddmpc_step on the law, S and M -- same rule, max_iter cap,
                                         statuses and count of `iters`; DDMPC_OPT_BOX_SAFEGUARD is honoured on bounded handles.  Per
                                         instance the setpoint enters the law, the offsets of the input and output components (a
                                         slack component keeps a = 0, c = -lam / lamb_sigma, lo / hi = -+ c eps_max) and the target of
                                         the output stage.  The iteration always starts from the empty set (no active-set warm
                                         start; the calls drop the seed).  An instance whose law came from refining solves
                                         (DDMPC_REFINE_AUTO) reports DDMPC_STATUS_OPTIMAL_INACCURATE when its final set is not
                                         empty: no cold re-solve is possible, the cold kernels read the shared setpoint table.  A
                                         non-finite setpoint is DDMPC_STATUS_SOLVER_ERROR for that instance; with the terminal
                                         constraint a setpoint outside [u_min, u_max] / [y_min, y_max] of its channel is
                                         DDMPC_STATUS_INFEASIBLE with u_opt and cost NaN and iters 0 (in the loop the instance stops
                                         there); neighbours are untouched.  ddmpc_get_solution after the calls is
                                         DDMPC_ERR_NOT_READY.  ddmpc_solve, ddmpc_step, ddmpc_closed_loop, ddmpc_get_gain and
                                         ddmpc_get_solution launch what they launch with 0 and return bit-equal results, with
                                         DDMPC_OPT_CONVEX_WARM_LAW on and off, with and without bounds.  0 (default; accepted on
                                         every handle).  Values other than 0 / 1: DDMPC_ERR_INVALID.  Changing the value forgets what
                                         ddmpc_prepare kept.  Setting 1 is DDMPC_ERR_UNSUPPORTED, with a message that names the
                                         reason, on NOMINAL controllers, with slack NONE (options 18 / 19 serve it: the three are
                                         never on together), with DDMPC_WEIGHT_DENSE, beyond 271 rows, on a trajectory beyond the
                                         LDS, with n(m+p) > 256 and where a boxed output component has a Q entry of 0 (the rule of
                                         DDMPC_OPT_CONVEX_WARM_LAW).  LIMITS: the bounds are the handle's, not per instance;
                                         DDMPC_REFINE_ALWAYS stays refused on bounded handles */
#define DDMPC_OPT_LARGE_SETPOINTS 21     /* Per-instance, per-step setpoints beyond 271 rows: 1 = ddmpc_step_setpoints,
                                         ddmpc_closed_loop_setpoints and ddmpc_get_setpoint_gain are open on a ROBUST handle on the
                                         phase kernels (272 .. 1024 rows, scalar / diagonal weights, slack NONE or the CONVEX slack
                                         box, no input / output bounds).  The factor K0 = L L' that ddmpc_prepare keeps does not depend
                                         on the setpoint, so ddmpc_step_setpoints is the step of ddmpc_step on the kept factor with the
                                         instance's own setpoint as the target of its setpoint rows and of the output stage: the same
                                         launches, and under the slack box the same active-set iteration, max_iter cap, statuses and
                                         `iters`.  With DDMPC_OPT_LARGE_AFFINE_LAW = 1 as well, ddmpc_prepare forms
                                         S = K0^-1 [1_c] next to the law ((m+p) r more doubles per instance; built and refined apart
                                         from the law, with the law's threshold and refine_max; an instance whose S misses the
                                         threshold has "no setpoint law", which ddmpc_step does not look at), and the step is one
                                         launch of "rr3_setpoint_law_step_kernel" -- beta = sum_f w_f gain[1+f] + sum_c s_c S[c] --
                                         followed in the same call by the solve on the kept factor for the instances without a law,
                                         without a setpoint law or outside the slack box.  ddmpc_closed_loop_setpoints runs the
                                         per-step path ("ddmpc_plant_kernel"; no limit on n_mpc_step * m).  Per instance a non-finite
                                         setpoint is DDMPC_STATUS_SOLVER_ERROR; neighbours are untouched.  ddmpc_get_solution after
                                         the two calls is DDMPC_ERR_NOT_READY.  ddmpc_solve, ddmpc_step, ddmpc_closed_loop,
                                         ddmpc_get_gain and ddmpc_get_solution launch what they launch with 0 and return bit-equal
                                         results.  0 (default; accepted on every handle).  Values other than 0 / 1:
                                         DDMPC_ERR_INVALID.  Changing the value forgets what ddmpc_prepare kept.  Setting 1 is
                                         DDMPC_ERR_UNSUPPORTED, with a message that names the reason, on NOMINAL controllers, with
                                         DDMPC_WEIGHT_DENSE, up to 271 rows (options 18 - 20 serve those), beyond 1024 rows, on a
                                         handle that is not on the phase kernels (DDMPC_PIPELINE_ONE_WORKGROUP, ddmpc_debug_stamps,
                                         batch > 65535), with n(m+p) > 256 and on a handle with input or output bounds; in the
                                         reverse order the bounds calls, DDMPC_PIPELINE_ONE_WORKGROUP and ddmpc_debug_stamps are
                                         refused on a handle with the option on.  LIMIT (CONVEX): an instance with more than 64 slack
                                         components switched at once, or whose 64 x 64-at-most Woodbury system of the switched
                                         components has a failed pivot, is DDMPC_STATUS_SOLVER_ERROR in the two calls (ddmpc_step hands
                                         such an instance to a fall-back kernel, which knows the handle's shared setpoints only and
                                         is not launched here); with the terminal constraint a setpoint that is no equilibrium of the
                                         plant binds the terminal slacks, n p of them.  Options 18 - 20 keep their refusals beyond
                                         271 rows */
#define DDMPC_OPT_LARGE_SETPOINT_BOUNDS 22 /* Per-instance, per-step setpoints on handles with input / output bounds beyond 271
                                         rows: 1 = ddmpc_step_setpoints and ddmpc_closed_loop_setpoints are open on a ROBUST handle
                                         on the phase kernels (272 .. 1024 rows, scalar / diagonal weights, slack NONE or the CONVEX
                                         slack box) that may carry input bounds, output bounds or both (DDMPC_OPT_LARGE_BOUNDS = 1
                                         admits them, as ever; the option and the bounds are accepted in either order).  The kept
                                         factor and the bounds do not depend on the setpoint: the calls run the bounded solve of
                                         ddmpc_step on the kept factor over the whole batch with the instance's own setpoint as the
                                         target of its setpoint rows, as the offset a_s of every boxed input / output component (the
                                         shifts are bound - a_s, formed on the device) and in the output stage -- the setpoint
                                         instantiations of "rr3_solve_box_kernel" / "rr3_solve_box_wide_kernel" /
                                         "rr3_box_safeguard_kernel".  With every instance given the handle's own setpoints the result
                                         is bit-equal to ddmpc_step on a handle without warm start or box law.  On a handle without
                                         finite bounds the calls run what DDMPC_OPT_LARGE_SETPOINTS runs on the kept factors (no law,
                                         no S).  DDMPC_OPT_LARGE_BOX_CAPACITY and DDMPC_OPT_LARGE_BOX_SAFEGUARD apply as to
                                         ddmpc_step; DDMPC_OPT_LARGE_BOX_WARM_START and DDMPC_OPT_LARGE_BOX_LAW may be on but are not
                                         honoured: the calls start from the empty set, read and keep no seed, and drop the seed with
                                         the record of the last solve.  Per instance (neighbours untouched): a non-finite setpoint is
                                         DDMPC_STATUS_SOLVER_ERROR with NaN outputs; with the terminal constraint a setpoint outside
                                         the bounds of its channel is DDMPC_STATUS_INFEASIBLE with NaN outputs and iters 0; an instance
                                         beyond the capacity or with a failed pivot is DDMPC_STATUS_SOLVER_ERROR with NaN outputs, as
                                         ddmpc_step reports it.  ddmpc_closed_loop_setpoints runs the per-step path
                                         ("ddmpc_plant_kernel").  ddmpc_get_solution after the two calls is DDMPC_ERR_NOT_READY;
                                         ddmpc_get_setpoint_gain is DDMPC_ERR_UNSUPPORTED (no S at this size on a bounded handle)
                                         unless DDMPC_OPT_LARGE_SETPOINTS provides it.  ddmpc_solve, ddmpc_step, ddmpc_closed_loop,
                                         ddmpc_get_gain and ddmpc_get_solution launch what they launch with 0 and return bit-equal
                                         results.  0 (default; accepted on every handle).  Values other than 0 / 1:
                                         DDMPC_ERR_INVALID.  Changing the value forgets nothing ddmpc_prepare kept.  Setting 1 is
                                         DDMPC_ERR_UNSUPPORTED, with a message that names the reason, on NOMINAL controllers, with
                                         DDMPC_WEIGHT_DENSE, up to 271 rows (options 19 / 20 serve those), beyond 1024 rows, on a
                                         handle that is not on the phase kernels (DDMPC_PIPELINE_ONE_WORKGROUP, ddmpc_debug_stamps,
                                         batch > 65535) and with n(m+p) > 256; DDMPC_PIPELINE_ONE_WORKGROUP and ddmpc_debug_stamps are
                                         refused on a handle with the option on.  DDMPC_OPT_LARGE_SETPOINTS keeps every refusal it
                                         has, bounds included, whether or not this option is on.  Not covered: NOMINAL controllers,
                                         dense weights, more than 1024 rows, per-instance bounds, a setpoint form of the large box
                                         law, the active-set warm start for these calls, a fused loop kernel */
#define DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS 23 /* Per-instance bounds (ddmpc_set_instance_input_bounds / _output_bounds) together with
                                         per-instance, per-step setpoints (DDMPC_OPT_SETPOINT_BOX_LAW / _SETPOINT_CONVEX_LAW) on one
                                         handle of at most 271 rows: a fleet whose plants differ in equilibrium AND in actuator range
                                         or safety limits.  1 = the per-instance bounds calls are accepted on a handle with option 19
                                         or 20 on, and options 19 / 20 on a handle that carries per-instance bounds (either order);
                                         every other refusal of those four calls stays.  ddmpc_step_setpoints and
                                         ddmpc_closed_loop_setpoints then launch the channel-table (BoxChannels) instantiations of
                                         ddmpc_setpoint_box_step_kernel / ddmpc_closed_loop_setpoint_box_kernel (the loop is labelled
                                         "ddmpc_closed_loop_instance_setpoint_box_kernel", under the CONVEX slack box
                                         "ddmpc_closed_loop_instance_setpoint_convex_kernel"), which stage the instance's bounds in LDS
                                         once per launch -- the bounds do not move with the schedule -- next to its offsets: the
                                         violation test, the shifts, the safeguard's ratios and "held at its bound exactly" use the
                                         instance's own bound, and with the terminal constraint a setpoint outside THAT INSTANCE's
                                         bounds is DDMPC_STATUS_INFEASIBLE (NaN outputs, iters 0, in the loop the instance stops
                                         there; neighbours untouched, also one whose wider box holds the same setpoint).  The law,
                                         S, the box list and M do not depend on the option: changing it forgets nothing
                                         ddmpc_prepare kept.  Rows that are all equal give results bit-equal to the shared bounds
                                         under option 19 / 20.  DDMPC_OPT_BOX_SAFEGUARD applies; DDMPC_OPT_BOX_WARM_START stays
                                         accepted and not honoured.  ddmpc_solve, ddmpc_step, ddmpc_closed_loop, ddmpc_get_solution,
                                         ddmpc_get_gain and ddmpc_get_setpoint_gain do what they do with 0 (the BoxChannels box
                                         kernels with the handle's shared setpoint); ddmpc_get_solution after a setpoint call stays
                                         DDMPC_ERR_NOT_READY.  0 (default): every call, error text and launched kernel is what it
                                         was before the option existed -- the two features refuse each other.  Values other than
                                         0 / 1: DDMPC_ERR_INVALID.  Setting 1 is DDMPC_ERR_UNSUPPORTED, with a message that names the
                                         reason, beyond 271 rows (bounds stay shared there), on NOMINAL controllers and with
                                         DDMPC_WEIGHT_DENSE; setting 0 is DDMPC_ERR_UNSUPPORTED while the handle carries
                                         per-instance bounds and option 19 or 20 together (remove one of the two first).  Not
                                         covered: with the terminal constraint the handle's own shared setpoint must still lie inside
                                         EVERY instance's row (ddmpc_solve / ddmpc_step use it; the bounds calls and
                                         ddmpc_set_setpoints check it), also when only the setpoint calls are used; more than 271
                                         rows; bounds per prediction step; the active-set warm start on the setpoint calls;
                                         ddmpc_get_solution after them */
#define DDMPC_REFINE_RES_DEFAULT 107  /* 2e-11: benchmark data stays below ~2e-12, the parity bars are missed from ~1.3e-10 on */

typedef struct ddmpc_handle ddmpc_handle;

/* Controller parameters = the constructor arguments of
 * DirectDataDrivenMPCController.__init__ (controller.py:95-116) minus the
 * per-instance data.  All pointers are HOST pointers, copied at create. */
typedef struct ddmpc_params {
  int32_t struct_size;              /* sizeof(ddmpc_params), ABI guard              */
  int32_t m, p, n, L, N;            /* inputs, outputs, est. order, horizon, data length */
  int32_t controller_type;          /* DDMPC_NOMINAL | DDMPC_ROBUST                  */
  int32_t slack_type;               /* DDMPC_SLACK_*                                 */
  int32_t use_terminal_constraint;  /* controller.py:229,489-492                     */
  int32_t weight_kind;              /* DDMPC_WEIGHT_*                                */
  const double* Q;                  /* 1 value (scalar), p*L values (diag) or (p*L)^2 (dense) */
  const double* R;                  /* 1 value (scalar), m*L values (diag) or (m*L)^2 (dense) */
  double eps_max, lamb_alpha, lamb_sigma, c;   /* robust parameters, controller.py:197-205 */
  const double* u_s;                /* [m]                                           */
  const double* y_s;                /* [p]                                           */
  int32_t max_iter;                 /* active-set iteration cap for slack CONVEX (0 -> 50) */
  int32_t gram_mode;                /* DDMPC_GRAM_*                                  */
} ddmpc_params;

int ddmpc_version(void);
const char* ddmpc_last_error(void);

/* Number of visible HIP devices (0 if none); never fails. */
int ddmpc_device_count(void);

/* Problem sizes: (m+p)(L+n) <= 271 rows run on the register-resident cold-solve kernels (all schemes, all weight
 * kinds).  Beyond that, controllers run on single-workgroup kernels that keep their
 * matrices in a global workspace (a Gram-route solve plus refinement with exact Hankel products; throughput: see
 * profiles/README.md): ROBUST ones on ddmpc_large_solve_kernel (same outputs, status, iterations, ddmpc_get_solution),
 * NOMINAL ones on the rank-revealing route -- phase kernels over the whole batch by default, the one-workgroup kernels on
 * request (DDMPC_OPT_LARGE_PIPELINE) -- with ddmpc_get_solution: ubar / ybar from its z, alpha = H'x from the vector it
 * exports.  By default no affine law is formed at that size (ddmpc_get_gain is DDMPC_ERR_UNSUPPORTED unless the
 * controller asked for it with DDMPC_OPT_LARGE_AFFINE_LAW: NOMINAL z(past), ROBUST beta(past) up to 1024 rows); the warm path there is
 * factor reuse -- ddmpc_prepare forms what depends on the data and the weights alone (NOMINAL: Gram, its rank-revealing
 * factor, the reduced normal matrix and its factor; ROBUST: Gram + lam D, the factor of the columns outside the slack
 * box, the Schur complement of the boxed block), ddmpc_step and the per-step closed loop solve on what it kept, with
 * results bit-equal to ddmpc_solve's.  Both schemes run on phase kernels over the whole batch by default up to 1024 rows
 * (round 5: also ROBUST controllers, and dense weighting matrices of either scheme; NOMINAL + dense: phase kernels only);
 * ROBUST controllers of 1025 .. 2048 rows and NOMINAL ones of 1025 .. 1524 (diagonal weights) run on 1024-thread instances of
 * the one-workgroup kernels.  Anything larger is DDMPC_ERR_UNSUPPORTED (reported by ddmpc_create).
 *
 * Replaces DirectDataDrivenMPCController.__init__ parameter validation
 * (controller.py:165-168,211-222,298-343,664-670) for a batch of instances on
 * HIP device `device`.  Does not solve. */
int ddmpc_create(const ddmpc_params* params, int64_t batch, int device, ddmpc_handle** out);
int ddmpc_destroy(ddmpc_handle* h);

/* Use an existing hipStream_t (passed as void*) instead of the handle's own. */
int ddmpc_set_stream(ddmpc_handle* h, void* hip_stream);
int ddmpc_synchronize(ddmpc_handle* h);

/* Per-instance data trajectories u_d [batch,N,m], y_d [batch,N,p]
 * (controller.py:177-179).  HOST: copied.  DEVICE: borrowed -- the buffers must stay valid for as long as the handle
 * uses them.  Their CONTENTS may be rewritten in place between calls: ddmpc_solve / ddmpc_closed_loop with the cold
 * path read the trajectories anew in every call and keep nothing derived from them.  What IS derived from the data and
 * kept is the affine law of the warm path (ddmpc_prepare, ddmpc_step, ddmpc_get_gain, the warm closed loop): after
 * rewriting borrowed data call ddmpc_set_data again (it only re-registers the pointers and drops the law). */
int ddmpc_set_data(ddmpc_handle* h, const double* u_d, const double* y_d, int mem);

/* One control step for every instance = update_and_solve_data_driven_mpc +
 * get_optimal_control_input (+ get_optimal_cost_value / get_problem_solve_status),
 * controller.py:389-407,739-808.  "Cold" solve: implicit Hankel -> Gram ->
 * reduced KKT -> Cholesky -> solve (-> active-set iterations for slack CONVEX).
 *   u_past [batch, n*m], y_past [batch, n*p]   (controller.py:184-185,577-581)
 *   u_opt  [batch, L*m]  = ubar[n*m:]          (controller.py:799-805)
 *   cost   [batch]       = problem.value       (controller.py:778)
 *   status [batch] int32 DDMPC_STATUS_*        (controller.py:755)
 *   iters  [batch] int32 factorisations used (may be NULL)
 * NOMINAL controllers: an instance whose Gram matrix is singular (noise-free data) is re-solved in the same
 * call by a rank-revealing kernel; it comes back "optimal", or "infeasible" when the hard constraints cannot be
 * met by any trajectory in the range of the Hankel matrix. */
int ddmpc_solve(ddmpc_handle* h, const double* u_past, const double* y_past,
                double* u_opt, double* cost, int32_t* status, int32_t* iters, int mem);

/* ddmpc_set_data + ddmpc_solve for HOST buffers in one call, pipelined: the batch is cut into chunks of
 * instances, chunk k+1 is uploaded on a copy stream while chunk k is solved on the compute stream.  Same
 * outputs as ddmpc_solve; afterwards the handle holds the uploaded data (ddmpc_step / ddmpc_get_solution
 * work as after ddmpc_set_data + ddmpc_solve).  All pointers are host pointers. */
int ddmpc_solve_from_host(ddmpc_handle* h, const double* u_d, const double* y_d,
                          const double* u_past, const double* y_past,
                          double* u_opt, double* cost, int32_t* status, int32_t* iters);

/* Warm path = what the reference's per-step entry point could reuse but does not:
 * update_and_solve_data_driven_mpc (controller.py:389-407) rebuilds and re-solves the whole QP
 * although only u_past / y_past changed (:404-407, :577-581); the Hankel matrices, weights and
 * therefore the KKT matrix are step-invariant (:376-377).  For a nominal controller and for a
 * robust one with slack NONE the QP has no inequality, so the solution is an affine function of
 * [u_past; y_past].
 *
 * ddmpc_prepare: one cold factorisation per instance with the Cholesky factor exported, then
 *   nf = n*(m+p) triangular solves per instance give the affine law
 *   beta = gain[:,0] + gain[:,1:] [u_past; y_past].  Invalidated by ddmpc_set_data /
 *   ddmpc_set_setpoints.  With slack CONVEX the law is that of the EMPTY active set (no sigma at its
 *   bound), i.e. the first primal-dual active-set iterate.
 * ddmpc_step: same contract and outputs as ddmpc_solve; uses the affine law (preparing on first
 *   use).  With slack CONVEX an instance whose affine iterate keeps every boxed sigma inside
 *   |sigma| <= c*eps_max is optimal as it is (iters = 1); by default the others are re-solved by the cold
 *   kernel in the same call (full active-set iteration, iters >= 2), so the results equal ddmpc_solve's.
 *   With DDMPC_OPT_CONVEX_WARM_LAW = 1 the active-set iteration runs on the law and M = K0^-1 E_box
 *   instead (rank-k changes of the empty set's system, no cold re-solve; see that option).
 *   The status of a warm step is the status of the factorisation it rests on (solver_error at the
 *   active-set iteration cap, as for ddmpc_solve).
 * ddmpc_get_gain: out [batch, nf+1, r] doubles, r = (m+p)(L+n) components in the internal
 *   time-major order rho = k*(m+p) + ch (ch < m: ubar, else ybar+sigma).
 * Beyond 271 rows: see the note on problem sizes at ddmpc_create (the data-dependent factors are kept; a law only with
 *   DDMPC_OPT_LARGE_AFFINE_LAW: NOMINAL z, ROBUST beta of the empty active set in the layout above, up to 1024 rows). */
int ddmpc_prepare(ddmpc_handle* h);
int ddmpc_step(ddmpc_handle* h, const double* u_past, const double* y_past,
               double* u_opt, double* cost, int32_t* status, int32_t* iters, int mem);
int ddmpc_get_gain(ddmpc_handle* h, double* out, int mem);

/* Engine options (DDMPC_OPT_*). */
int ddmpc_set_option(ddmpc_handle* h, int option, int value);

/* set_input_output_setpoints (controller.py:945-982); takes effect at the next solve. */
int ddmpc_set_setpoints(ddmpc_handle* h, const double* u_s, const double* y_s);

/* Box on the predicted inputs: u_min[ch] <= ubar[k][ch] <= u_max[ch] on every FREE prediction step (the rows that
 * carry R; with the terminal constraint the last n steps stay fixed to u_s) -- the constraint u_k in U of the robust scheme.
 * u_min, u_max: HOST, [m]; -INFINITY / +INFINITY = no bound on that side; both NULL removes the bounds.  Shared by the batch,
 * like every controller parameter.  Takes effect at the next solve; forgets what ddmpc_prepare kept and the last solution,
 * as ddmpc_set_setpoints does (ddmpc_get_solution: DDMPC_ERR_NOT_READY).  Bounds that are all infinite are accepted and leave
 * every result bit-equal to a handle that never had the call.
 *   DDMPC_ERR_INVALID: NaN in either array; u_min[ch] >= u_max[ch]; only one pointer NULL; with the terminal constraint, u_s
 *     outside [u_min, u_max] (the QP is infeasible by construction; ddmpc_set_setpoints checks the same on a bounded handle).
 *   DDMPC_ERR_UNSUPPORTED: NOMINAL controllers; DDMPC_WEIGHT_DENSE; a bounded channel with an R entry of 0 on
 *     a free prediction step; with the CONVEX slack box a Q entry of 0 on one.  Up to 271 rows also: DDMPC_REFINE_ALWAYS (refused
 *     by ddmpc_set_option too once bounds are set); n(m+p) > 256, the one shape for which ddmpc_prepare forms no law at that
 *     size (trajectories beyond the LDS are served: their law comes from the streamed Gram).  Beyond 271 rows: see "Bounds
 *     beyond 271 rows" below.  ddmpc_solve_from_host on a bounded handle is DDMPC_ERR_UNSUPPORTED at every size.
 * How a bounded handle is served.  A bound that is active makes its input row hard, a diagonal rank-k change of the system of
 * the empty active set, exactly what the slack box does.  Every call runs the primal-dual active-set iteration
 * over the whole box list -- the slack components (CONVEX) and the free input rows of the bounded channels, from the empty set; an
 * inactive component goes to the bound it violates, an active one is released when its multiplier changes sign (never moved to
 * the other bound in one step, the rule of the full-space formulation) -- on the affine law and M = K0^-1 E_box that ddmpc_prepare forms
 * (DDMPC_OPT_CONVEX_WARM_LAW and DDMPC_OPT_CONVEX_UPDATE are accepted and have no effect: the handle is always on the law).
 * Same solve count, max_iter cap and status 4 (solver_error) at the cap or on a non-positive pivot as under the slack box; a box
 * tight enough to make the rule cycle (width 0.2 around u_s at the data tail) ends there unless DDMPC_OPT_BOX_SAFEGUARD = 1, which
 * finishes such an instance by a primal active-set method.  In the solution an active input equals its bound exactly.
 * DDMPC_OPT_BOX_WARM_START = 1 starts the iteration of ddmpc_step and of the fused loop from the last solve's set instead.
 *   ddmpc_prepare: law + M, nbox r doubles per instance with nbox = [p L or p (L - n) when CONVEX] + [free steps x bounded
 *     channels] -- 122 KB at L = 30, n = 4, m = p = 2, CONVEX, both channels bounded: 0.5 GB at 4096 instances -- plus
 *     nbox (nbox + 1) / 2 doubles of k x k scratch when nbox > 16.  An allocation failure is DDMPC_ERR_HIP.
 *   ddmpc_step / ddmpc_closed_loop (paths AUTO, WARM: one fused launch, "ddmpc_closed_loop_box_kernel"): no read of the
 *     trajectories.  Instances whose law ddmpc_prepare took from refining solves (DDMPC_REFINE_AUTO, flagged) iterate on that law
 *     and the unrefined M like the others and report DDMPC_STATUS_OPTIMAL_INACCURATE when their final active set is not empty.
 *   ddmpc_solve / DDMPC_PATH_COLD: the cold contract -- the trajectories are read anew, into a preparation of the call's own
 *     (a second set of the buffers above) that is dropped afterwards; a kept ddmpc_prepare stays valid.
 *     DDMPC_OPT_CLOSED_LOOP_GRAPH is ignored.
 * Bounds beyond 271 rows ((m+p)(L+n) = 272 .. 1024; both calls, same arguments and meaning), with DDMPC_OPT_LARGE_BOUNDS = 1;
 * without the option finite bounds are DDMPC_ERR_UNSUPPORTED at this size.  There is no affine law and no M
 * at this size: the phase kernels (DDMPC_PIPELINE_PHASES) keep the factor of the EMPTY active set and treat every active
 * component -- slack, input or output -- as one column of a Woodbury update on the trailing block of the factor, the bounded rows
 * joining the slack rows in the "boxed last" order; one exact-Hankel refinement pass on the system of the final active set
 * follows unless DDMPC_REFINE_OFF (all three refinement modes are accepted: the kept factor plus that pass is the normal solve
 * here).  Same iteration rule, max_iter cap and status 4 at the cap; an active input or output equals its bound exactly.
 * Served by ddmpc_solve, ddmpc_prepare (the factors only) + ddmpc_step (bit-equal to ddmpc_solve), the per-step
 * ddmpc_closed_loop ("ddmpc_plant_kernel": there is no fused loop at this size) and ddmpc_get_solution.
 *   LIMIT: at most the capacity, 64 by default (DDMPC_OPT_LARGE_BOX_CAPACITY: 128, 192 or 256), of components (slack + input +
 *     output) may be active at once in any iteration; W takes ldw x capacity doubles per instance (see the option).  No fall-back
 *     kernel knows the bounds: an instance that exceeds the capacity, or whose k x k pivot is not positive, reports DDMPC_STATUS_SOLVER_ERROR with `iters`
 *     the iteration at which it happened and NaN in u_opt / cost; the other instances of the batch are not affected.
 *   DDMPC_ERR_UNSUPPORTED, each with a message that names the reason: DDMPC_OPT_LARGE_BOUNDS = 0; more than 1024 rows; a handle that is not on the phase
 *     kernels (DDMPC_OPT_LARGE_PIPELINE = DDMPC_PIPELINE_ONE_WORKGROUP, ddmpc_debug_stamps enabled, batch > 65535);
 *     DDMPC_OPT_LARGE_AFFINE_LAW = 1.  In the reverse order the same three are refused on a bounded handle:
 *     ddmpc_set_option(DDMPC_OPT_LARGE_PIPELINE, DDMPC_PIPELINE_ONE_WORKGROUP), ddmpc_set_option(DDMPC_OPT_LARGE_AFFINE_LAW, 1)
 *     and ddmpc_debug_stamps(enable).  NOMINAL, DDMPC_WEIGHT_DENSE and zero weights as above.
 *   DDMPC_OPT_BOX_SAFEGUARD is accepted and has no effect beyond 271 rows; the safeguard of this size is an option of its own,
 *     DDMPC_OPT_LARGE_BOX_SAFEGUARD = 1: an instance at the max_iter cap is solved again by the primal active-set method
 *     (`iters` = max_iter + its solves, working sets up to the capacity; see the option).  The box list has no length limit there.
 *   DDMPC_OPT_BOX_WARM_START is accepted and has no effect beyond 271 rows; the warm start of this size is an option of its own,
 *     DDMPC_OPT_LARGE_BOX_WARM_START = 1: ddmpc_step and the per-step ddmpc_closed_loop start the iteration from the signed set
 *     the last solve ended with; a seeded run that fails starts again from the empty set, ddmpc_solve keeps the cold contract
 *     and leaves a seed (see the option for what drops the seed and how `iters` counts).
 *   DDMPC_OPT_LARGE_BOX_LAW = 1 gives this size a law after all, for the steps that stay inside the box: ddmpc_prepare forms the
 *     law of the empty active set next to the factors ((n(m+p) + 1) r doubles per instance: 40 KB at the four-tank L = 70,
 *     627 KB at 608 rows with n(m+p) = 128), a step whose beta violates no component of the box table is served by one launch
 *     on it (`iters` = 1, agreeing with the solve to rounding), and every other instance of the batch is solved in the same call
 *     by the launches above restricted to it, bit-equal to the option 0.  ddmpc_solve keeps the cold contract. */
int ddmpc_set_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max);

/* Box on the predicted outputs: y_min[ch] <= ybar[k][ch] <= y_max[ch] on every FREE prediction step (the rows that carry Q;
 * all L of them, or the first L - n with the terminal constraint, whose last n steps stay fixed to y_s).  The bound is on
 * ybar, not on ybar + sigma: with DDMPC_SLACK_NONE sigma stays free and the problem is always feasible; with the CONVEX slack
 * box it can be infeasible.  There is NO infeasibility detection: such an instance ends in DDMPC_STATUS_SOLVER_ERROR at the
 * max_iter cap or on a non-positive pivot, as a box that makes the iteration cycle does.
 * y_min, y_max: HOST, [p]; -INFINITY / +INFINITY = no bound on that side; both NULL removes the bounds.  Shared by the batch.
 * Takes effect at the next solve; forgets what ddmpc_prepare kept and the last solution, exactly like ddmpc_set_input_bounds.
 * Bounds that are all infinite leave every result bit-equal to a handle that never had the call.  Independent of the input
 * bounds: a handle may have either or both, and either call keeps the other's bounds.
 *   DDMPC_ERR_INVALID: NaN in either array; y_min[ch] >= y_max[ch]; only one pointer NULL; with the terminal constraint, y_s
 *     outside [y_min, y_max] (ddmpc_set_setpoints checks the same on a bounded handle).
 *   DDMPC_ERR_UNSUPPORTED: NOMINAL controllers; DDMPC_WEIGHT_DENSE; a bounded channel with a Q entry of 0 on
 *     a free prediction step; with the CONVEX slack box a Q entry of 0 on any.  Up to 271 rows also: DDMPC_REFINE_ALWAYS (refused
 *     by ddmpc_set_option too once bounds are set); n(m+p) > 256; a box list of more than 288 components (slack + bounded
 *     inputs + bounded outputs; the count is named, also by ddmpc_prepare when input bounds set later make the list too long).
 *     Beyond 271 rows: "Bounds beyond 271 rows" at ddmpc_set_input_bounds -- 272 .. 1024 rows on the phase kernels, at most the
 *     capacity, 64 by default, of components active at once (DDMPC_OPT_LARGE_BOX_CAPACITY; W: ldw x capacity doubles per instance).  ddmpc_solve_from_host on such a handle is DDMPC_ERR_UNSUPPORTED.
 * How it is served: as an input-bounded handle (above), by ddmpc_solve, ddmpc_step, ddmpc_closed_loop (fused and per step),
 * ddmpc_get_solution and DDMPC_OPT_BOX_SAFEGUARD.  The output is a third kind of boxed component: hat = y_s - lam beta / q,
 * d = lam / q.  A predicted output row carries ybar and sigma, so a CONVEX handle has two components on such a row and both
 * may be active at once (the row is then hard); M keeps one column per boxed ROW (112 columns for 164 components at L = 30,
 * n = 4, m = p = 2, CONVEX with the terminal constraint, every channel bounded).  In the solution an active output equals its
 * bound exactly and sigma = (ybar + sigma) - bound, or +- c eps_max with both active. */
int ddmpc_set_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max);

/* Input bounds per instance: u_min[b][ch] <= ubar[k][ch] <= u_max[b][ch] on every FREE prediction step of instance b -- the
 * meaning of ddmpc_set_input_bounds with one row per instance, for a batch that is a fleet of controllers with different
 * actuator ranges.  u_min, u_max: HOST, [batch][m]; -INFINITY / +INFINITY = instance b has no bound on that side of that
 * channel; both NULL removes the input bounds.  The call replaces, and is replaced by, ddmpc_set_input_bounds: the last call
 * of either wins.  Independent of the output bounds: one kind may be shared while the other is per instance.  Like the shared
 * call it synchronises, forgets what ddmpc_prepare kept and the last solution (ddmpc_get_solution: DDMPC_ERR_NOT_READY) and
 * takes effect at the next solve.
 * The box list, and with it the columns of M, stays shared by the batch: a channel is boxed when ANY instance has a finite
 * bound on it.  An instance whose own bound on a listed channel is infinite never activates those components.  When no
 * instance has a finite bound the call is a removal: every result is bit-equal to a handle that never had it.  Rows that are
 * all equal give results bit-equal to ddmpc_set_input_bounds with that row.
 *   DDMPC_ERR_INVALID, with a message that names instance and channel: NaN in either array; u_min[b][ch] >= u_max[b][ch];
 *     with the terminal constraint, the handle's u_s outside the interval of any instance (ddmpc_set_setpoints checks its
 *     argument against every row on such a handle).  Only one pointer NULL.
 *   DDMPC_ERR_UNSUPPORTED, with a message that names the reason: everything ddmpc_set_input_bounds refuses up to 271 rows
 *     (NOMINAL, DDMPC_WEIGHT_DENSE, a zero weight on a boxed channel, DDMPC_REFINE_ALWAYS, n(m+p) > 256; a box list of more
 *     than 288 components is named by ddmpc_set_instance_output_bounds or ddmpc_prepare; ddmpc_solve_from_host); more than 271
 *     rows, also with DDMPC_OPT_LARGE_BOUNDS = 1 (the phase kernels read the shared bounds); a handle with
 *     DDMPC_OPT_SETPOINT_BOX_LAW or DDMPC_OPT_SETPOINT_CONVEX_LAW on -- in the reverse order ddmpc_set_option refuses those two
 *     on a handle that carries per-instance bounds of either kind -- unless DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1, which admits
 *     both orders (the setpoint calls then run the channel-bounds instantiations of the setpoint-box kernels: see the option).
 * How it is served: Route::BoxLaw as under shared bounds, by the channel-bounds instantiations of its two kernels, which stage
 * the instance's bounds in LDS (ddmpc_box_law.hpp; the fused loop is labelled "ddmpc_closed_loop_instance_box_kernel": the
 * name is the label of the path, the kernel is that instantiation of ddmpc_closed_loop_box_kernel) -- ddmpc_solve with the cold contract
 * and a preparation of the call's own, ddmpc_prepare + ddmpc_step (bit-equal to ddmpc_solve), ddmpc_closed_loop fused and per
 * step, ddmpc_get_solution (an active input equals ITS INSTANCE's bound exactly).  Statuses, `iters`, the max_iter cap and
 * optimal_inaccurate on refined laws are those of the shared-bounds kernels; DDMPC_OPT_BOX_SAFEGUARD applies.
 * DDMPC_OPT_BOX_WARM_START is accepted and not honoured: every solve starts from the empty set and no seed is kept.  A handle
 * without per-instance bounds launches exactly the kernels it launched before these calls existed.
 * Not covered: more than 271 rows; per-instance setpoints on the same handle without DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1
 * (options 19, 20) and beyond 271 rows (option 22); with that option and the terminal constraint, a shared setpoint of the handle
 * outside any instance's row (it stays DDMPC_ERR_INVALID: ddmpc_solve / ddmpc_step use it); the active-set warm start;
 * keeping ddmpc_prepare's law and M across a call that changes bound values only; bounds per prediction step; NOMINAL
 * controllers and dense weights. */
int ddmpc_set_instance_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max);

/* Output bounds per instance: y_min[b][ch] <= ybar[k][ch] <= y_max[b][ch] on every FREE prediction step of instance b -- the
 * meaning of ddmpc_set_output_bounds (a bound on ybar, not on ybar + sigma; no infeasibility detection under the CONVEX slack
 * box) with one row per instance.  y_min, y_max: HOST, [batch][p]; -INFINITY / +INFINITY = no bound on that side for that
 * instance; both NULL removes the output bounds.  Replaces, and is replaced by, ddmpc_set_output_bounds; independent of the
 * input bounds of either form.  Everything else -- side effects, the shared box list (a channel is boxed when any instance has
 * a finite bound on it; no finite bound in the batch is a removal), DDMPC_ERR_INVALID with instance and channel (here y_s
 * against every row under the terminal constraint), DDMPC_ERR_UNSUPPORTED (what ddmpc_set_output_bounds refuses up to 271 rows,
 * the box list over 288 components included; more than 271 rows; options 19 / 20 without DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1),
 * how it is served, the options and what is
 * not covered -- as ddmpc_set_instance_input_bounds.  In the solution an active output equals its instance's bound exactly. */
int ddmpc_set_instance_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max);

/* Values of the optimisation variables of the last ddmpc_solve, ddmpc_solve_from_host, ddmpc_step or ddmpc_closed_loop
 * (controller.py:434-445 `.value`); `out` sized as listed at DDMPC_SOL_*.  DDMPC_ERR_NOT_READY before any of them and after
 * ddmpc_set_data, ddmpc_set_setpoints or a ddmpc_prepare on the register-resident kernels ((m+p)(L+n) <= 271); a
 * ddmpc_prepare beyond 271 rows keeps the solution readable.  Instances of a NOMINAL controller that
 * were solved by the rank-revealing rescue kernel (exact, rank-deficient data) report ubar / ybar from that kernel's
 * own solution and NaN for alpha (any alpha with H alpha = [ubar; ybar] is optimal there; none is formed). */
int ddmpc_get_solution(ddmpc_handle* h, int what, double* out, int mem);

/* hankel_matrix(X, L) for a batch (direct_data_driven_mpc/utilities/hankel_matrix.py:5-53):
 * X [batch,N,nch] -> H [batch, L*nch, N-L+1].  Stand-alone (no handle). */
int ddmpc_hankel(const double* X, int64_t batch, int32_t N, int32_t nch, int32_t L,
                 double* H, int mem, int device);

/* Batched persistent-excitation guard = the construction-time check of the reference
 * (controller.py:275-296 -> evaluate_persistent_excitation, hankel_matrix.py:55-87: rank of the
 * order-`order` Hankel matrix of u_d equals m*order, by SVD).  u_d [batch,N,m]; for every instance
 * ratio_lb[b] receives a rigorous lower bound of sigma_min/sigma_max of that Hankel matrix, from a
 * Cholesky factorisation of its Gram matrix (0 when the factorisation breaks down).  A bound well
 * above the SVD tolerance max(M,N)*eps certifies full rank on the device; the caller runs the exact
 * SVD test only on the instances it leaves undecided (see BatchedDDMPC.persistent_excitation_guard).
 * Stand-alone (no handle).  The packed Gram matrix lives in LDS when it fits (m*order <= ~190 rows), else in
 * a temporary global workspace. */
int ddmpc_pe_guard(const double* u_d, int64_t batch, int32_t N, int32_t m, int32_t order,
                   double* ratio_lb, int mem, int device);

/* LTI plant x+ = A x + B u, y = C x + D u + w (utilities/model_simulation.py:70-98); row-major HOST pointers. */
typedef struct ddmpc_plant {
  int32_t ns;                       /* state dimension                              */
  const double* A;                  /* [ns,ns]                                      */
  const double* B;                  /* [ns,m]                                       */
  const double* C;                  /* [p,ns]                                       */
  const double* D;                  /* [p,m]                                        */
} ddmpc_plant;

/* Batched closed loop, entirely on the device: the driver loop of
 * utilities/controller/controller_operation.py:259-305 (Algorithm 1, and the n-step
 * Algorithm 2 when n_mpc_step > 1) for every instance of the batch:
 *   for t = 0, n_mpc_step, 2 n_mpc_step, ... < n_steps:
 *     QP solve with the current past windows                   (controller.py:389-407)
 *       -- by the affine law of ddmpc_prepare when there is no inequality (the whole loop of an
 *          instance then runs inside one workgroup), else a cold solve per step; see
 *          DDMPC_OPT_CLOSED_LOOP_PATH
 *     for k = t .. min(t + n_mpc_step, n_steps) - 1:
 *       u[k] = optimal_u[(k-t) m : (k-t+1) m]                  (controller.py:839)
 *       y[k] = C x + D u[k] + w[k];  x <- A x + B u[k]         (model_simulation.py:93-98)
 *       FIFO push of (u[k], y[k]) into the past windows         (controller.py:893-895)
 * x [batch,ns], u_past [batch,n*m], y_past [batch,n*p] are updated in place;
 * w [batch,n_steps,p] is the measurement noise; u_sys [batch,n_steps,m], y_sys [batch,n_steps,p]
 * receive the closed-loop trajectories; status [batch] the worst solve status seen (an instance whose
 * solve is not optimal stops evolving -- the reference raises at that point, controller.py:808 --
 * and the rest of its trajectory is NaN).  All buffers follow `mem`.
 * A stopped instance: the rows of u_sys / y_sys from the first step of the failed solve on are NaN, the rows before
 * it are those of a loop that did not stop, and x, u_past, y_past come back as they stood when that solve was
 * made (the state after, and the window of, the last step applied; the caller's own values when the first solve
 * fails).  The other instances of the batch are not affected.
 * Bounds the call enforces: 1 <= plant->ns <= 16 and 1 <= n_mpc_step <= L (DDMPC_ERR_INVALID otherwise); m and p
 * are bounded by the controller only.  The fused one-workgroup loops also need n (m + p) <= 256 and
 * n_mpc_step * m <= 256: beyond either the call runs the per-step path whatever DDMPC_OPT_CLOSED_LOOP_PATH says.
 * ddmpc_get_solution after the call reads the loop's last solve, at the past window that solve saw (the reference's
 * `.value`s after its loop): the last n rows of [u_past on entry; u_sys[0 .. t)] and of [y_past on entry; y_sys[0 .. t)],
 * t = n_mpc_step * ((n_steps - 1) / n_mpc_step) being the step of that solve. */
int ddmpc_closed_loop(ddmpc_handle* h, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step,
                      double* x, double* u_past, double* y_past, const double* w,
                      double* u_sys, double* y_sys, int32_t* status, int mem);

/* Per-instance, per-step setpoints (DDMPC_OPT_SETPOINT_LAW = 1, or DDMPC_OPT_SETPOINT_BOX_LAW = 1 -- see there for what the
 * calls do on a handle with input / output bounds --, or DDMPC_OPT_SETPOINT_CONVEX_LAW = 1 -- see there for what they do under
 * the CONVEX slack box --, or beyond 271 rows DDMPC_OPT_LARGE_SETPOINTS = 1 -- see there and the last paragraph below;
 * DDMPC_ERR_UNSUPPORTED on all three calls without any of them).  The
 * reduced system K0 beta = t is linear in t and t is linear in the setpoints, so with m + p more columns the law of
 * ddmpc_prepare takes the setpoint as an argument:
 *     beta_b = sum_f past_b[f] gain[b][1+f][:] + sum_c s_b[c] S[b][c][:],      s_b = [u_s_b ; y_s_b],
 *     S[b][c][:] = K0_b^-1 1_c,  1_c[rho] = 1 iff rho mod (m+p) = c and row rho takes its target from a setpoint (every
 *     prediction step, free or terminal; rho the internal time-major order of ddmpc_get_gain).
 * With the terminal constraint a setpoint should be an equilibrium of the instance's plant, as for ddmpc_set_setpoints.
 * ddmpc_step_setpoints: ddmpc_step with u_s [batch, m] and y_s [batch, p] (they follow `mem`, like the windows).  Prepares
 *   on first use, then one launch ("ddmpc_setpoint_step_kernel").  status = the status of the factorisation, iters = 1; a
 *   non-finite setpoint gives that instance DDMPC_STATUS_SOLVER_ERROR and leaves its neighbours as they are.  The handle's own
 *   setpoints are neither read nor changed.  DDMPC_ERR_NOT_READY before ddmpc_set_data.
 * ddmpc_closed_loop_setpoints: ddmpc_closed_loop with a schedule u_ref [batch, n_steps, m], y_ref [batch, n_steps, p]: the
 *   solve made at step t uses row t, rows between solves are not read.  Everything else as for ddmpc_closed_loop (arguments,
 *   stopped instances, 1 <= ns <= 16, 1 <= n_mpc_step <= L); an instance also stops, with DDMPC_STATUS_SOLVER_ERROR, at a solve
 *   whose setpoint is not finite.  Always one fused launch ("ddmpc_closed_loop_setpoint_kernel", reported by
 *   ddmpc_closed_loop_kernel_name): there is no per-step path, n_mpc_step * m > 256 is DDMPC_ERR_UNSUPPORTED, and
 *   DDMPC_OPT_CLOSED_LOOP_PATH and DDMPC_OPT_CLOSED_LOOP_GRAPH are ignored.
 * ddmpc_get_setpoint_gain: out [batch, m+p, r] doubles = S.  DDMPC_ERR_NOT_READY before a ddmpc_prepare with the option on.
 * ddmpc_get_solution after either of the first two calls is DDMPC_ERR_NOT_READY (the reconstruction reads the shared
 *   setpoint table); a later ddmpc_solve or ddmpc_step makes the solution readable again.
 * LIMITS: ROBUST controllers only; slack NONE and no input / output bounds (with bounds: DDMPC_OPT_SETPOINT_BOX_LAW; with
 *   the CONVEX slack box, bounded or not: DDMPC_OPT_SETPOINT_CONVEX_LAW); scalar / diagonal weights;
 *   at most 271 rows and a trajectory that fits the LDS; n(m+p) <= 256.  The cold kernels know the handle's shared setpoints
 *   only (ddmpc_solve).  Under DDMPC_REFINE_AUTO the instances whose law and S are refined are chosen from solves at the
 *   handle's own setpoints, not at the ones passed later.
 * Beyond 271 rows (DDMPC_OPT_LARGE_SETPOINTS = 1; ROBUST on the phase kernels, 272 .. 1024 rows, slack NONE or CONVEX, scalar /
 *   diagonal weights, no bounds, n(m+p) <= 256): ddmpc_step_setpoints is the step on the kept factor with the instance's
 *   setpoint (statuses and iters of ddmpc_step), or with DDMPC_OPT_LARGE_AFFINE_LAW = 1 one launch of
 *   "rr3_setpoint_law_step_kernel" and the solve on the kept factor for the instances it leaves.  ddmpc_closed_loop_setpoints
 *   runs per step ("ddmpc_plant_kernel"), reads row t of the schedules in place and has no limit on n_mpc_step * m.
 *   ddmpc_get_setpoint_gain returns S when the law was built with it, else DDMPC_ERR_NOT_READY (without
 *   DDMPC_OPT_LARGE_AFFINE_LAW no S is formed).  LIMITS: under the CONVEX slack box an instance with more than 64 slack components
 *   switched at once, or with a failed pivot in the small system of the switched components, is DDMPC_STATUS_SOLVER_ERROR (the
 *   two cases ddmpc_step hands to its fall-back kernel); bounded handles, the fall-back kernel, NOMINAL controllers, dense weights and
 *   more than 1024 rows are not served. */
int ddmpc_step_setpoints(ddmpc_handle* h, const double* u_past, const double* y_past, const double* u_s, const double* y_s,
                         double* u_opt, double* cost, int32_t* status, int32_t* iters, int mem);
int ddmpc_closed_loop_setpoints(ddmpc_handle* h, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step,
                                double* x, double* u_past, double* y_past, const double* w,
                                const double* u_ref, const double* y_ref,
                                double* u_sys, double* y_sys, int32_t* status, int mem);
int ddmpc_get_setpoint_gain(ddmpc_handle* h, double* out, int mem);

/* Kernel facts for benchmarking: algorithmic flops and bytes of one cold solve
 * with this handle's configuration (see DESIGN.md "Roofline accounting"). */
int ddmpc_cost_model(ddmpc_handle* h, double* flops_per_solve, double* bytes_per_solve);

/* Name of the dominant kernel as it appears in rocprofv3 traces. */
const char* ddmpc_kernel_name(ddmpc_handle* h);

/* Name of the kernel that stepped the plant in the last ddmpc_closed_loop: "ddmpc_closed_loop_warm_kernel" or
 * "ddmpc_closed_loop_convex_warm_kernel" / "ddmpc_closed_loop_box_kernel" (input bounds) when the whole loop ran fused in one launch, "ddmpc_plant_kernel" when it ran
 * per step (DDMPC_PATH_COLD, shapes beyond the fused loops' bounds, NOMINAL instances without a law, laws taken from
 * refining solves under DDMPC_OPT_CONVEX_WARM_LAW, handles beyond 271 rows -- ddmpc_closed_loop_setpoints included there); "ddmpc_closed_loop_setpoint_kernel" /
 * "ddmpc_closed_loop_setpoint_box_kernel" / "ddmpc_closed_loop_setpoint_convex_kernel" after ddmpc_closed_loop_setpoints; "" before the first loop.
 * The names are labels of the path taken: "ddmpc_closed_loop_instance_box_kernel" (per-instance bounds) is the channel-bounds
 * instantiation of ddmpc_closed_loop_box_kernel, "ddmpc_closed_loop_setpoint_convex_kernel" the slack-box instantiation of
 * ddmpc_closed_loop_setpoint_box_kernel, "ddmpc_closed_loop_instance_setpoint_box_kernel" /
 * "ddmpc_closed_loop_instance_setpoint_convex_kernel" (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1 on a handle with per-instance bounds)
 * the channel-bounds instantiations of the same kernel.  Read-only. */
const char* ddmpc_closed_loop_kernel_name(ddmpc_handle* h);

/* Diagnostics only: in-kernel phase stamps (shader-clock ticks) of the next solves.
 * `enable` != 0 turns stamping on (zeroing the buffer); `out` (host, [batch,16] uint64,
 * may be NULL) receives the stamps of the last solve: [0] kernel entry, [1..6] phase
 * ends (staging + tables, lag blocks, base tiles + diagonal walks, Cholesky, [5] = [4], back substitution);
 * [7..11] Cholesky sub-phase sums of wave 0 ([10], [11]: lower 32 bits; their upper halves hold wave 0's ticks in
 * the fix-up of its tiles and at the barrier behind it, plain variant), [14] exit,
 * [15]/[13] the 100 MHz real-time counter at entry/exit.  Off by default; a stamping
 * run must not be used for timing claims. */
int ddmpc_debug_stamps(ddmpc_handle* h, int enable, uint64_t* out);

/* Diagnostics only (problems beyond the register-resident kernels): copies instance `b`'s slice of the global workspace
 * (packed factor of the Gram matrix, then the packed factor of the reduced normal matrix; rows on 128-byte boundaries)
 * and its pivot record [skip (rv) | skipT (rv) | nlive | nRl] to host memory, at most `ws_count` doubles / `meta_count`
 * ints; either output may be NULL.  *ws_avail / *meta_avail (may be NULL) receive the sizes of the slices.
 * Round 5: ws_count < 0 (NOMINAL, phase kernels): the pivot candidates of G's factorisation in the order they were decided on
 * (16 ceil(r / 16) doubles: the pivot where a column was accepted, the residue where it was skipped; tools/pivot_gap_study.py).
 * ROBUST controllers beyond 271 rows on the phase kernels: meta_out receives the per-instance record of the last solve
 * [k, state, iterations, k, switched positions (64), active set (r rounded up to 2), start tick, ticks (100 MHz), peak k of a
 * bounded handle, -] and
 * *ws_avail = 0 (tools/rr3_schedule.py).  What is read is what the last solve left, on the implementation that served it:
 * DDMPC_ERR_NOT_READY when that was none of the above (no solve yet, the register-resident kernels, the one-workgroup ROBUST
 * kernel). */
int ddmpc_debug_workspace(ddmpc_handle* h, int64_t b, double* ws_out, int64_t ws_count, int32_t* meta_out, int64_t meta_count,
                          int64_t* ws_avail, int64_t* meta_avail);

/* Diagnostics only, process-wide: from now on every device buffer the library allocates is pre-filled with `byte` (0: off, the
 * default; 255 gives NaN bit patterns, 63 small finite doubles).  A result that changes with the fill has read memory no kernel
 * wrote -- fresh device memory is zero on this stack, which hides such reads in a standalone run.  Returns the previous setting.
 * (tests/test_gpu_round4.py) */
int ddmpc_debug_poison_allocations(int byte);

/* Diagnostics only, host arithmetic, no device and no handle: the component order of a ROBUST controller beyond 271 rows on
 * the phase kernels, "boxed LAST" -- the boxed class is the union of the slack rows (convex != 0: every predicted output row),
 * the free input rows of the channels with a finite input bound and the free output rows of the channels with a finite output
 * bound; time order inside both classes.  u_min / u_max [m], y_min / y_max [p], both of a kind NULL = no bounds of that kind.
 * perm_out [(m+p)(L+n)]: position -> row; *n_a: the first boxed position; *nbox: components of the box table (0 without bounds);
 * comp_out [2 comp_count]: position of component s, then whether it is an output component (ascending by position, the slack
 * before the output on a shared row), at most comp_count of them.  Any output may be NULL.  (tests/test_large_bounds_reference.py) */
int ddmpc_debug_large_box_order(int32_t m, int32_t p, int32_t n, int32_t L, int32_t use_terminal_constraint, int32_t convex,
                                const double* u_min, const double* u_max, const double* y_min, const double* y_max,
                                int32_t* perm_out, int32_t* n_a, int32_t* comp_out, int64_t comp_count, int32_t* nbox);

#ifdef __cplusplus
}
#endif
#endif /* DDMPC_H */
