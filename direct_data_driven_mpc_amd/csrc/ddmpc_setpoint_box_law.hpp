// ddmpc_setpoint_box_law.hpp -- DDMPC_OPT_SETPOINT_BOX_LAW: per-instance, per-step setpoints on a handle with input / output
// bounds (Route::BoxLaw: ROBUST, slack NONE, scalar / diagonal weights, at most 271 rows).  The two halves it joins:
// ddmpc_box_law.hpp (the primal-dual iteration on the law and M = K0^-1 E_box) and ddmpc_setpoint_law.hpp (S = K0^-1 [1_c]).
//
// M does not depend on the setpoint.  The setpoint s_b = [u_s_b ; y_s_b] of an instance enters its bounded solve in three places:
//   * the law of the empty set, beta0 = sum_f past[f] gain[1 + f] + sum_c s_b[c] S[c]           (setpoint_law_row);
//   * the offset of every boxed component: hat_s = a_s + c_s beta_rho with a_s = s_b[rho_s mod (m+p)] -- without the CONVEX
//     slack box every component is a free input or a free output --, so shift_s = bound - a_s is per instance too.  The
//     kernels keep as[s] in LDS, filled once per solve, and point their copy of the table's `a` at it: box_iterate,
//     box_solve_set and box_safeguard reach the offsets through BoxTab::a only and are used as they stand;
//   * the target tb of the output stage (the overloads of box_component / box_component_y below).
// The handle's own [a] column (d_box_bd, the shared setpoint) is not read here.
//
// Per instance the step refuses (neighbours untouched): a non-finite setpoint -> status 4, nothing iterated; with the terminal
// constraint a setpoint outside the bounds of its channel -> DDMPC_STATUS_INFEASIBLE, u_opt and cost NaN, iters 0 (the last n
// inputs / outputs are fixed to it: the per-instance form of the DDMPC_ERR_INVALID of ddmpc_set_input_bounds / _set_setpoints).
// The iteration always starts from the empty set (no DDMPC_OPT_BOX_WARM_START), and beta / the active set are not written
// (ddmpc_get_solution reconstructs with the shared table and is refused after these kernels).
//
// DDMPC_OPT_SETPOINT_CONVEX_LAW (the SLACK instantiations of the two kernels): the same on a ROBUST handle with the CONVEX slack
// box, slack-only or next to input / output bounds.  The one thing the slack box changes: the box list holds components of two kinds,
//   * input / output components, whose offset is the instance's setpoint of their channel, a_s = s_b[rho_s mod (m+p)];
//   * slack components, sigma_s = c beta_rho with c = -lam / lamb_sigma inside +- c_param eps_max: their offset is 0 whatever the
//     setpoint (setpoint_convex_offset).  On a K_WPRED / K_WTERM row the slack component is T.of[rho]; the output component of
//     the same row, if the channel is bounded, is T.ofy[rho].
// A slack-only handle runs the same table-driven kernels (the instantiations without YB) on a box list of slack components alone
// -- ddmpc_prepare forms that list, its [a | c | lo | hi | 1/d] table and M for it whether or not DDMPC_OPT_CONVEX_WARM_LAW is on
// --, not setpoint twins of ddmpc_warm_convex_step_kernel: box_iterate with such a table IS cwl_iterate (same rule, same count of
// solves), and one pair of kernels serves every CONVEX handle.  The channel bounds `chb` are +-infinity there, so the only
// per-instance refusal left is the non-finite setpoint.  The output stage needs nothing more: the box_component /
// box_component_y overloads below carry the K_WPRED / K_WTERM branches with the slack flag and the K_WINT rows.
//
// DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS (the BoxChannels instantiations of the two kernels, on a handle that carries per-instance bounds):
// next to the offsets as[] the kernels keep blo[s] / bhi[s], the instance's own bounds by boxed component, in LDS -- filled by
// instance_box_fill from the instance's row of the channel table (ddmpc_box_law.hpp), once per launch (the loop kernel: once per
// instance, the bounds do not move with the schedule) -- and point the table's lo / hi at them.  The fill reads the shared lo / hi
// for the slack components of a CONVEX handle, so it runs before the pointers are swapped, and a barrier stands between it and the
// first BoxTab::test.  The per-instance refusal reads the instance's own row instead of the shared `chb`.  Nothing else differs.
// Included by the API translation unit only; nothing here is launched by a handle with both options 0.
#pragma once
#include "ddmpc_box_law.hpp"
#include "ddmpc_setpoint_law.hpp"

namespace ddmpc {

// box_component with the target of the setpoint rows passed in (`tb`: the instance's setpoint of the row's channel) instead of
// read from the shared table row tabd[2]; otherwise its text.
__device__ __forceinline__ double box_component(const KParams& P, int RPs, const BoxTab& T, int rho, int j, double beta, int sa,
                                                const double* pv, double tb, double* z_out) {
  const int kind = P.tabi[0 * RPs + rho];
  const int pidx = P.tabi[1 * RPs + rho];
  const double D = sa ? P.tabd[1 * RPs + rho] : P.tabd[0 * RPs + rho];
  const double wq = P.tabd[3 * RPs + rho];
  const double tp = (pidx >= 0) ? pv[pidx] : tb;
  double z = tp + sa * P.bound - P.lam * D * beta;
  if (kind == K_UFREE && sa != 0) z = T.bound(j, sa);
  double contrib = P.lam * beta * z;
  if (kind == K_UFREE || kind == K_YFREE) { const double dlt = z - tb; contrib += wq * dlt * dlt; }
  else if (kind == K_WINT) { const double sg = z - tp; contrib += P.lamb_sigma * sg * sg; }
  else if (kind == K_WTERM) { const double sg = z - tb; contrib += P.lamb_sigma * sg * sg; }
  else if (kind == K_WPRED) {
    const double sg = (sa != 0) ? sa * P.bound : -P.lam * beta / P.lamb_sigma;
    const double dlt = z - sg - tb;
    contrib += wq * dlt * dlt + P.lamb_sigma * sg * sg;
  }
  *z_out = z;
  return contrib;
}

// ... and box_component_y (a K_WPRED row whose output component jy is held at its bound).
__device__ __forceinline__ double box_component_y(const KParams& P, int RPs, const BoxTab& T, int rho, int jy, double beta, int sa,
                                                  int say, double tb, double* z_out) {
  const double wq = P.tabd[3 * RPs + rho];
  const double yb = T.bound(jy, say);
  const double sg = (sa != 0) ? sa * P.bound : -P.lam * beta / P.lamb_sigma;
  const double z = yb + sg;
  const double dlt = yb - tb;
  *z_out = z;
  return P.lam * beta * z + wq * dlt * dlt + P.lamb_sigma * sg * sg;
}

// The status of a setpoint the step refuses, or 0 (sv [nch] in LDS, settled by a barrier; the same value in every thread).
// chb = [lo (nch) | hi (nch)] per channel, inputs first, +-infinity where a channel has no bound; tec: the terminal constraint.
__device__ __forceinline__ int setpoint_box_refusal(int nch, int tec, const double* sv, const double* __restrict__ chb) {
  int bad = 0, out = 0;
  for (int c = 0; c < nch; ++c) {
    const double v = sv[c];
    bad |= !(fabs(v) < 1e300);
    out |= (v < chb[c]) || (v > chb[nch + c]);
  }
  return bad ? 4 : ((tec && out) ? 2 : 0);
}

// The offset a_j of boxed component j of a CONVEX handle at the setpoint [us (m) ; ys (p)] of the instance: 0 for a slack component.
__device__ __forceinline__ double setpoint_convex_offset(const KParams& P, int RPs, const BoxTab& T, int j, const double* us,
                                                         const double* ys) {
  const int rho = T.rho[j];
  const int kind = P.tabi[0 * RPs + rho];
  if ((kind == K_WPRED || kind == K_WTERM) && T.of[rho] == j) return 0.0;
  const int c = rho % P.nch;
  return (c < P.m) ? us[c] : ys[c - P.m];
}

// One control step of a bounded handle with a setpoint per instance: grid = batch, block = r (YB: max(r, nbox)) rounded up to 64,
// the geometry of ddmpc_box_step_kernel.  Four stages: the law with S against the instance's setpoint; the violation test with
// the instance's offsets; the iteration of ddmpc_box_step_kernel on M (same rule, same max_iter cap, status 4 at the cap or on a
// non-positive pivot; SAFE: box_safeguard behind the cap; `refined` instances report optimal_inaccurate with a non-empty final
// set); the output stage with the instance's setpoint as target.  iters as ddmpc_box_step_kernel counts them.
// u_s [batch][m], y_s [batch][p]; everything else as in ddmpc_box_step_kernel, whose `bd` serves [c | lo | hi | 1/d] here.
// Fixed-size arrays: pv, sv [WARM_MAX_NF] (nf <= WARM_MAX_NF, m + p <= nf), bsh, as [WARM_MAX_R] (r <= 271, nbox <= WARM_MAX_R:
// checked by ddmpc_prepare).
// SLACK (DDMPC_OPT_SETPOINT_CONVEX_LAW): the offsets of a CONVEX handle's box list (setpoint_convex_offset); nothing else differs.
// SAFE is then launched on bounded handles only.
// Extra = BoxChannels (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1 on a handle with per-instance bounds, "INST"): the same stages, statuses
// and iters with the instance's own bounds -- blo, bhi [WARM_MAX_R] in LDS behind the table's lo / hi, as in ddmpc_box_step_kernel --
// and the refusal against the instance's own row of the channel table (`chb` is not read).  The host launches the empty pack
// otherwise: that instantiation is the kernel as it was.
template <bool SAFE, bool YB, bool SLACK = false, class... Extra>
__global__ void ddmpc_setpoint_box_step_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                               const double* __restrict__ sgain, const int* __restrict__ prep_status,
                                               const double* __restrict__ u_past, const double* __restrict__ y_past,
                                               const double* __restrict__ u_s, const double* __restrict__ y_s,
                                               double* __restrict__ u_opt, double* __restrict__ cost, int* __restrict__ status,
                                               int* __restrict__ iters, int nbox, const int* __restrict__ tab,
                                               const double* __restrict__ bd, const double* __restrict__ Mcol, double* __restrict__ sg,
                                               const int* __restrict__ refined, const double* __restrict__ chb, int tec,
                                               Extra... extra) {
  constexpr bool INST = (std::is_same_v<Extra, BoxChannels> || ...);
  [[maybe_unused]] const BoxChannels chan = box_channels_of(extra...);
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double sv[WARM_MAX_NF];
  __shared__ double red[32];
  __shared__ double bsh[WARM_MAX_R];
  __shared__ double as[WARM_MAX_R];                   // the offsets a_s of this instance, by boxed component
  __shared__ CwlLds s;
  const int r = P.r, nch = P.nch;
  BoxTabT<YB> T = box_table<YB>(nbox, tab, bd, r);
  T.a = as;
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nrhs = nf + 1;
  const int nyp = nf - P.npu;
  const long long uo_stride = (long long)(P.Ln - P.npu / P.m) * P.m;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  for (int c = tid; c < nch; c += blockDim.x)
    sv[c] = (c < P.m) ? u_s[b * P.m + c] : y_s[b * P.p + (c - P.m)];
  for (int j = tid; j < nbox; j += blockDim.x) {
    if constexpr (SLACK) {
      as[j] = setpoint_convex_offset(P, RPs, T, j, u_s + b * P.m, y_s + b * P.p);
    } else {
      const int c = T.rho[j] % nch;
      as[j] = (c < P.m) ? u_s[b * P.m + c] : y_s[b * P.p + (c - P.m)];
    }
  }
  if constexpr (INST) {                               // (the fill reads the shared lo / hi of slack components: before the swap)
    __shared__ double blo[WARM_MAX_R];                // the bounds of this instance, by boxed component
    __shared__ double bhi[WARM_MAX_R];
    instance_box_fill<YB>(P, T, chan.chb + b * (long long)(2 * nch), blo, bhi);
    T.lo = blo;
    T.hi = bhi;
    chb = chan.chb + b * (long long)(2 * nch);        // the refusal reads the instance's own row
  }
  __syncthreads();
  const int refuse = setpoint_box_refusal(nch, tec, sv, chb);
  if (refuse == 2) {                                  // (uniform: the whole workgroup leaves)
    const double nanv = __longlong_as_double(0x7ff8000000000000LL);
    for (int rho = tid; rho < r; rho += blockDim.x) {
      const int oidx = P.tabi[2 * RPs + rho];
      if (oidx >= 0) u_opt[b * uo_stride + oidx] = nanv;
    }
    if (tid == 0) { cost[b] = nanv; status[b] = 2; if (iters) iters[b] = 0; }
    return;
  }
  const double* g = gain + b * (long long)nrhs * r;
  const double* sgb = sgain + b * (long long)nch * r;
  int viol = 0;
  for (int rho = tid; rho < r; rho += blockDim.x) {
    const double beta = setpoint_law_row(g, sgb, r, rho, nf, nch, pv, sv);
    bsh[rho] = beta;
    const int j = T.of[rho];
    if (j >= 0 && T.test(j, beta, 0) != 0) viol = 1;
    if constexpr (YB) {
      const int jy = T.ofy[rho];
      if (jy >= 0 && T.test(jy, beta, 0) != 0) viol = 1;
    }
  }
  viol = __syncthreads_or(viol);
  int st = prep_status[b], it = 1;
  int ncol = nbox;
  if constexpr (YB) ncol = T.ncol;
  const double* Mb = Mcol + b * (long long)ncol * r;
  const bool iterate = viol && st <= 1 && refuse == 0;   // (a failed factorisation, a non-finite setpoint: nothing to iterate on)
  if (iterate) {
    double* Sg = sg + b * (long long)(nbox * (nbox + 1) / 2);
    int dst = box_iterate<YB>(P, T, Mb, Sg, bsh, s, &it);
    if constexpr (SAFE) {
      __shared__ BoxSafeLds q;
      if (dst == 4 && !s.fail) {                      // at the cap (not a pivot)
        int more;
        dst = box_safeguard<YB>(P, T, Mb, Sg, bsh, s, q, &more);
        it += more;
      }
    }
    if (dst) st = dst;
    else if (st == 0 && refined != nullptr && refined[b] != 0 && s.kfin > 0) st = 1;
  }
  double part = 0.0;
  bool finite = true;
  for (int rho = tid; rho < r; rho += blockDim.x) {
    double beta = bsh[rho], z;
    const double tb = sv[rho % nch];
    if (!iterate) {
      part += warm_component(P, RPs, rho, beta, pv, tb, &z);
    } else {
      const int j = T.of[rho];
      const int sa = (j >= 0) ? s.act[j] : 0;
      beta = box_beta<YB>(s, T, Mb, r, beta, rho);
      int say = 0, jy = -1;
      if constexpr (YB) {
        jy = T.ofy[rho];
        say = (jy >= 0) ? s.act[jy] : 0;
      }
      if (say != 0) part += box_component_y(P, RPs, T, rho, jy, beta, sa, say, tb, &z);
      else part += box_component(P, RPs, T, rho, j, beta, sa, pv, tb, &z);
    }
    finite = finite && (fabs(beta) < 1e300);
    const int oidx = P.tabi[2 * RPs + rho];
    if (oidx >= 0) u_opt[b * uo_stride + oidx] = z;
  }
  part = wave_sum(part);
  const unsigned long long okmask = __ballot(finite);
  if ((tid & 63) == 0) { red[tid >> 6] = part; red[16 + (tid >> 6)] = (okmask == ~0ull) ? 0.0 : 1.0; }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, bad = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { tot += red[w]; bad += red[16 + w]; }
    if (refuse != 0 || bad != 0.0 || !(fabs(tot) < 1e300)) st = 4;
    cost[b] = tot;
    status[b] = st;
    if (iters) iters[b] = it;
  }
}

// Whole closed loop of one instance of a bounded handle in one workgroup with a setpoint schedule: ddmpc_closed_loop_box_kernel
// with row t0 of the schedule per solve (u_ref [batch][n_steps][m], y_ref [batch][n_steps][p]; rows between solves are not read).
// Per solve: the setpoint and the offsets as[], the law with S on the boxed rows and the n_mpc_step * m input rows in use, the
// iteration, the M_A ev correction of those rows, then the plant / FIFO steps.  An instance stops (NaN rows from that solve on, x
// and the windows as they stood) at a solve that is not optimal / optimal_inaccurate, as in ddmpc_closed_loop_box_kernel, and at a
// refused setpoint: status 4 for a non-finite one, as in ddmpc_closed_loop_setpoint_kernel, DDMPC_STATUS_INFEASIBLE for one
// outside its channel's bounds under the terminal constraint.  A stopped instance makes no further solves.  SAFE, YB: as in
// ddmpc_setpoint_box_step_kernel; an instance the safeguard finishes carries on.  Nothing is kept for ddmpc_get_solution.
// Fixed-size arrays as in ddmpc_closed_loop_box_kernel plus sv [WARM_MAX_NF] and as [WARM_MAX_R]; ddmpc_closed_loop_setpoints
// checks n_mpc_step * m <= WARM_MAX_NF and ns <= 16.  SLACK: as in ddmpc_setpoint_box_step_kernel.
// Extra = BoxChannels: as in ddmpc_setpoint_box_step_kernel; blo / bhi are filled once, before the first solve (the bounds do not
// move with the schedule).
template <bool SAFE, bool YB, bool SLACK = false, class... Extra>
__global__ void ddmpc_closed_loop_setpoint_box_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                                      const double* __restrict__ sgain, const int* __restrict__ prep_status, int ns,
                                                      const double* __restrict__ pl, int n_steps, int n_mpc_step,
                                                      double* __restrict__ x, double* __restrict__ u_past,
                                                      double* __restrict__ y_past, const double* __restrict__ w,
                                                      const double* __restrict__ u_ref, const double* __restrict__ y_ref,
                                                      double* __restrict__ u_sys, double* __restrict__ y_sys,
                                                      int* __restrict__ status_out, int nbox, const int* __restrict__ tab,
                                                      const double* __restrict__ bd, const double* __restrict__ Mcol,
                                                      double* __restrict__ sg, const int* __restrict__ refined,
                                                      const double* __restrict__ chb, int tec, Extra... extra) {
  constexpr bool INST = (std::is_same_v<Extra, BoxChannels> || ...);
  [[maybe_unused]] const BoxChannels chan = box_channels_of(extra...);
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double sv[WARM_MAX_NF];
  __shared__ double uo[WARM_MAX_NF];      // the first n_mpc_step*m entries of optimal_u
  __shared__ double xs[16], xn[16];       // (ns <= 16 is checked by ddmpc_closed_loop_setpoints)
  __shared__ double bsh[WARM_MAX_R];
  __shared__ double as[WARM_MAX_R];       // the offsets a_s of the solve in progress, by boxed component
  __shared__ CwlLds s;
  const int r = P.r;
  BoxTabT<YB> T = box_table<YB>(nbox, tab, bd, r);
  T.a = as;
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nrhs = nf + 1, m = P.m, p = P.p, nch = P.nch;
  const int n = P.npu / m, nyp = nf - P.npu;
  const double* A = pl;
  const double* Bm = A + ns * ns;
  const double* C = Bm + ns * m;
  const double* Dm = C + p * ns;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  if (tid < ns) xs[tid] = x[b * ns + tid];
  if constexpr (INST) {                               // (visible behind the barrier that opens the first solve)
    __shared__ double blo[WARM_MAX_R];                // the bounds of this instance, by boxed component
    __shared__ double bhi[WARM_MAX_R];
    instance_box_fill<YB>(P, T, chan.chb + b * (long long)(2 * nch), blo, bhi);
    T.lo = blo;
    T.hi = bhi;
    chb = chan.chb + b * (long long)(2 * nch);        // the refusal reads the instance's own row
  }
  const int st0 = prep_status[b];
  const bool refd = refined != nullptr && refined[b] != 0;
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);
  const double* g = gain + b * (long long)nrhs * r;
  const double* sgb = sgain + b * (long long)nch * r;
  int ncol = nbox;
  if constexpr (YB) ncol = T.ncol;
  const double* Mb = Mcol + b * (long long)ncol * r;
  double* Sg = sg + b * (long long)(nbox * (nbox + 1) / 2);
  const int nuse = n_mpc_step * m;
  double* up = pv;
  double* yp = pv + P.npu;
  int stc = 0;                                        // worst status so far (uniform over the workgroup)
  for (int t0 = 0; t0 < n_steps; t0 += n_mpc_step) {
    // sv / as were last read in the output stage of the previous solve, ahead of the barrier (__syncthreads_or) that closes it:
    // they are free here, while thread 0 may still be in the plant steps of that solve (which read uo, pv and xs only)
    const double* ur = u_ref + (b * n_steps + t0) * m;
    const double* yr = y_ref + (b * n_steps + t0) * p;
    if (stc <= 1) {
      for (int c = tid; c < nch; c += blockDim.x) sv[c] = (c < m) ? ur[c] : yr[c - m];
      for (int j = tid; j < nbox; j += blockDim.x) {
        if constexpr (SLACK) {
          as[j] = setpoint_convex_offset(P, RPs, T, j, ur, yr);
        } else {
          const int c = T.rho[j] % nch;
          as[j] = (c < m) ? ur[c] : yr[c - m];
        }
      }
    }
    __syncthreads();                                  // the setpoint, the offsets and the window of the last plant steps visible; bsh, uo free
    if (stc <= 1) {                                   // (uniform; a stopped instance makes no further solves)
      int st = st0, it = 1;
      const int refuse = setpoint_box_refusal(nch, tec, sv, chb);
      if (refuse != 0) {
        st = refuse;
      } else {
        int viol = 0;
        for (int rho = tid; rho < r; rho += blockDim.x) {
          const int oidx = P.tabi[2 * RPs + rho];
          const int j = T.of[rho];
          int jy = -1;
          if constexpr (YB) jy = T.ofy[rho];
          if ((oidx >= 0 && oidx < nuse) || j >= 0 || jy >= 0) {
            const double beta = setpoint_law_row(g, sgb, r, rho, nf, nch, pv, sv);
            bsh[rho] = beta;
            if (j >= 0 && T.test(j, beta, 0) != 0) viol = 1;
            if (jy >= 0 && T.test(jy, beta, 0) != 0) viol = 1;
          }
        }
        viol = __syncthreads_or(viol);
        const bool iterate = viol && st <= 1;
        if (iterate) {
          int dst = box_iterate<YB>(P, T, Mb, Sg, bsh, s, &it);
          if constexpr (SAFE) {
            __shared__ BoxSafeLds q;
            if (dst == 4 && !s.fail) {
              int more;
              dst = box_safeguard<YB>(P, T, Mb, Sg, bsh, s, q, &more);
              it += more;
            }
          }
          if (dst) st = dst;
          else if (st == 0 && refd && s.kfin > 0) st = 1;
        }
        int nonfin = 0;
        for (int rho = tid; rho < r; rho += blockDim.x) {
          const int oidx = P.tabi[2 * RPs + rho];
          const int j = T.of[rho];
          int jy = -1;
          if constexpr (YB) jy = T.ofy[rho];
          const bool use = oidx >= 0 && oidx < nuse;
          if (use || j >= 0 || jy >= 0) {
            const int sa = (iterate && j >= 0) ? s.act[j] : 0;
            const double beta = iterate ? box_beta<YB>(s, T, Mb, r, bsh[rho], rho) : bsh[rho];
            nonfin |= !(fabs(beta) < 1e300);
            if (use) {                                // (an input row: no output component)
              double z;
              (void)box_component(P, RPs, T, rho, j, beta, sa, pv, sv[rho % nch], &z);
              uo[oidx] = z;
            }
          }
        }
        if (__syncthreads_or(nonfin)) st = 4;
      }
      stc = (st > stc) ? st : stc;
    }
    if (tid == 0) {
      const int nsub = (t0 + n_mpc_step <= n_steps) ? n_mpc_step : n_steps - t0;
      for (int j = 0; j < nsub; ++j) {
        const int k = t0 + j;
        double* us = u_sys + (b * n_steps + k) * m;
        double* ys = y_sys + (b * n_steps + k) * p;
        if (stc > 1) {
          for (int i = 0; i < m; ++i) us[i] = nanv;
          for (int i = 0; i < p; ++i) ys[i] = nanv;
          continue;
        }
        const double* uk = uo + j * m;
        const double* wk = w + (b * n_steps + k) * p;
        for (int i = 0; i < p; ++i) {              // y = C x + D u + w with the state BEFORE the update
          double sum = wk[i];
          for (int q = 0; q < ns; ++q) sum += C[i * ns + q] * xs[q];
          for (int q = 0; q < m; ++q) sum += Dm[i * m + q] * uk[q];
          ys[i] = sum;
        }
        for (int i = 0; i < ns; ++i) {
          double sum = 0.0;
          for (int q = 0; q < ns; ++q) sum += A[i * ns + q] * xs[q];
          for (int q = 0; q < m; ++q) sum += Bm[i * m + q] * uk[q];
          xn[i] = sum;
        }
        for (int i = 0; i < ns; ++i) xs[i] = xn[i];
        for (int i = 0; i < m; ++i) us[i] = uk[i];
        for (int i = 0; i < (n - 1) * m; ++i) up[i] = up[i + m];       // FIFO shift
        for (int i = 0; i < m; ++i) up[(n - 1) * m + i] = uk[i];
        for (int i = 0; i < (n - 1) * p; ++i) yp[i] = yp[i + p];
        for (int i = 0; i < p; ++i) yp[(n - 1) * p + i] = ys[i];
      }
    }
  }
  __syncthreads();
  for (int f = tid; f < nf; f += blockDim.x) {
    if (f < P.npu) u_past[b * P.npu + f] = pv[f]; else y_past[b * nyp + (f - P.npu)] = pv[f];
  }
  if (tid < ns) x[b * ns + tid] = xs[tid];
  if (tid == 0) status_out[b] = stc;
}

}  // namespace ddmpc
