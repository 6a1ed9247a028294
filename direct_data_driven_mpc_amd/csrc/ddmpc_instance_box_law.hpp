// ddmpc_instance_box_law.hpp -- per-instance input / output bounds (ddmpc_set_instance_input_bounds,
// ddmpc_set_instance_output_bounds) on Route::BoxLaw: ROBUST, slack NONE or the CONVEX slack box, scalar / diagonal weights, at
// most 271 rows.  Twins of ddmpc_box_step_kernel and ddmpc_closed_loop_box_kernel (ddmpc_box_law.hpp) whose bounds come from a
// per-instance channel table instead of the shared [lo | hi] columns of `bd`.
//
// M = K0^-1 E_box, the law and the box list depend on WHICH rows are boxed, not on the bound values: the list is the union over
// the batch (a channel is listed when any instance has a finite bound on it) and stays shared.  The bound values enter the solve
// through BoxTab::lo / BoxTab::hi only -- the violation test, the shifts, the safeguard's ratios and the output stage's "held at
// its bound exactly".  The kernels keep blo[s] / bhi[s] in LDS by boxed component, filled once per launch (the loop kernel: once
// per instance, not per solve), and point their copy of the table at them: box_iterate, box_solve_set, box_safeguard, box_beta,
// box_component and box_component_y are used as they stand.  An instance whose own bound on a listed component is infinite never
// activates it (hat > +inf and hat < -inf are false), so its shift is never formed.
//     chb [batch][lo (nch) | hi (nch)], inputs first, -+infinity where the instance has no bound on the channel;
//     a slack component (CONVEX) keeps -+ c eps_max from the shared `bd`; an input or output component takes its channel's entry.
// The iteration always starts from the empty set (no DDMPC_OPT_BOX_WARM_START instantiations).  beta and the signed active set
// are written as by the shared-bounds kernels: ddmpc_get_solution reconstructs with the same channel table.
// Included by the API translation unit only; nothing here is launched by a handle without per-instance bounds.
#pragma once
#include "ddmpc_box_law.hpp"

namespace ddmpc {

// blo / bhi of one instance by the whole workgroup (no barrier after it).  T still points at the shared `bd` here.  Component j
// on row rho: an input row (rho mod nch < m) carries an input component; on an output row the output component is the one
// T.ofy names (YB), any other is the slack of a CONVEX handle.
template <bool YB>
__device__ __forceinline__ void instance_box_fill(const KParams& P, const BoxTabT<YB>& T, const double* __restrict__ cb,
                                                  double* blo, double* bhi) {
  const int nch = P.nch;
  for (int j = threadIdx.x; j < T.nbox; j += blockDim.x) {
    const int rho = T.rho[j], ch = rho % nch;
    bool chan = ch < P.m;
    if constexpr (YB) chan = chan || T.ofy[rho] == j;
    blo[j] = chan ? cb[ch] : T.lo[j];
    bhi[j] = chan ? cb[nch + ch] : T.hi[j];
  }
}

// One control step of a handle with per-instance bounds: ddmpc_box_step_kernel<SAFE, YB> (same grid, block, arguments, stages,
// statuses and iters) with the channel table `chb` behind `refined`.  Fixed-size arrays: those of ddmpc_box_step_kernel plus
// blo, bhi [WARM_MAX_R] (nbox <= WARM_MAX_R is checked by ddmpc_prepare).
template <bool SAFE, bool YB>
__global__ void ddmpc_instance_box_step_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                               const int* __restrict__ prep_status, const double* __restrict__ u_past,
                                               const double* __restrict__ y_past, double* __restrict__ u_opt,
                                               double* __restrict__ cost, int* __restrict__ status, int* __restrict__ iters,
                                               double* __restrict__ beta_ws, signed char* __restrict__ act_ws, int nbox,
                                               const int* __restrict__ tab, const double* __restrict__ bd,
                                               const double* __restrict__ Mcol, double* __restrict__ sg,
                                               const int* __restrict__ refined, const double* __restrict__ chb) {
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double red[32];
  __shared__ double bsh[WARM_MAX_R];
  __shared__ double blo[WARM_MAX_R];                  // the bounds of this instance, by boxed component
  __shared__ double bhi[WARM_MAX_R];
  __shared__ CwlLds s;
  const int r = P.r;
  BoxTabT<YB> T = box_table<YB>(nbox, tab, bd, r);
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nrhs = nf + 1;
  const int nyp = nf - P.npu;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  instance_box_fill<YB>(P, T, chb + b * (long long)(2 * P.nch), blo, bhi);
  T.lo = blo;
  T.hi = bhi;
  __syncthreads();
  const double* g = gain + b * (long long)nrhs * r;
  int viol = 0;
  for (int rho = tid; rho < r; rho += blockDim.x) {
    // all loads of a chunk of 8 columns are issued before they are consumed (HBM-bound: keep bytes in flight)
    double beta = g[rho];
    const double* gc = g + r + rho;
    int f = 0;
    for (; f + 8 <= nf; f += 8) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = gc[(long long)(f + q) * r];
#pragma unroll
      for (int q = 0; q < 8; ++q) beta += pv[f + q] * v[q];
    }
    for (; f < nf; ++f) beta += pv[f] * gc[(long long)f * r];
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
  const bool iterate = viol && st <= 1;               // (a failed factorisation: nothing to iterate on)
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
    int sa = 0;
    if (!iterate) {
      part += warm_component(P, RPs, rho, beta, pv, bsh, &z);
    } else {
      const int j = T.of[rho];
      sa = (j >= 0) ? s.act[j] : 0;
      beta = box_beta<YB>(s, T, Mb, r, beta, rho);
      int say = 0, jy = -1;
      if constexpr (YB) {
        jy = T.ofy[rho];
        say = (jy >= 0) ? s.act[jy] : 0;
      }
      if (say != 0) part += box_component_y(P, RPs, T, rho, jy, beta, sa, say, &z);
      else part += box_component(P, RPs, T, rho, j, beta, sa, pv, &z);
      sa += 4 * say;
    }
    finite = finite && (fabs(beta) < 1e300);
    const int oidx = P.tabi[2 * RPs + rho];
    if (oidx >= 0) u_opt[b * (long long)((P.Ln - P.npu / P.m) * P.m) + oidx] = z;
    beta_ws[b * (long long)P.rE + rho] = beta;
    act_ws[b * (long long)P.rE + rho] = (signed char)sa;
  }
  part = wave_sum(part);
  const unsigned long long okmask = __ballot(finite);
  if ((tid & 63) == 0) { red[tid >> 6] = part; red[16 + (tid >> 6)] = (okmask == ~0ull) ? 0.0 : 1.0; }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, bad = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { tot += red[w]; bad += red[16 + w]; }
    if (bad != 0.0 || !(fabs(tot) < 1e300)) st = 4;
    cost[b] = tot;
    status[b] = st;
    if (iters) iters[b] = it;
  }
}

// Whole closed loop of one instance of a handle with per-instance bounds in one workgroup: ddmpc_closed_loop_box_kernel<SAFE, YB>
// (same arguments, stages and stops) with the channel table `chb` behind `refined`; blo / bhi are filled once, before the first solve.
// Fixed-size arrays: those of ddmpc_closed_loop_box_kernel plus blo, bhi [WARM_MAX_R].
template <bool SAFE, bool YB>
__global__ void ddmpc_closed_loop_instance_box_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                                      const int* __restrict__ prep_status, int ns, const double* __restrict__ pl,
                                                      int n_steps, int n_mpc_step, double* __restrict__ x,
                                                      double* __restrict__ u_past, double* __restrict__ y_past,
                                                      const double* __restrict__ w, double* __restrict__ u_sys,
                                                      double* __restrict__ y_sys, int* __restrict__ status_out,
                                                      double* __restrict__ beta_ws, signed char* __restrict__ act_ws, int nbox,
                                                      const int* __restrict__ tab, const double* __restrict__ bd,
                                                      const double* __restrict__ Mcol, double* __restrict__ sg,
                                                      const int* __restrict__ refined, const double* __restrict__ chb,
                                                      double* __restrict__ lw_up, double* __restrict__ lw_yp) {
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double uo[WARM_MAX_NF];      // the first n_mpc_step*m entries of optimal_u
  __shared__ double xs[16], xn[16];       // (ns <= 16 is checked by ddmpc_closed_loop)
  __shared__ double bsh[WARM_MAX_R];
  __shared__ double blo[WARM_MAX_R];      // the bounds of this instance, by boxed component
  __shared__ double bhi[WARM_MAX_R];
  __shared__ CwlLds s;
  const int r = P.r;
  BoxTabT<YB> T = box_table<YB>(nbox, tab, bd, r);
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nrhs = nf + 1, m = P.m, p = P.p;
  const int n = P.npu / m, nyp = nf - P.npu;
  const double* A = pl;
  const double* Bm = A + ns * ns;
  const double* C = Bm + ns * m;
  const double* Dm = C + p * ns;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  if (tid < ns) xs[tid] = x[b * ns + tid];
  instance_box_fill<YB>(P, T, chb + b * (long long)(2 * P.nch), blo, bhi);   // (visible behind the barrier that opens the first solve)
  T.lo = blo;
  T.hi = bhi;
  const int st0 = prep_status[b];
  const bool refd = refined != nullptr && refined[b] != 0;
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);
  const double* g = gain + b * (long long)nrhs * r;
  int ncol = nbox;
  if constexpr (YB) ncol = T.ncol;
  const double* Mb = Mcol + b * (long long)ncol * r;
  double* Sg = sg + b * (long long)(nbox * (nbox + 1) / 2);
  const int nuse = n_mpc_step * m;
  double* up = pv;
  double* yp = pv + P.npu;
  int stc = 0;                                        // worst status so far (ddmpc_plant_kernel's st_acc)
  for (int t0 = 0; t0 < n_steps; t0 += n_mpc_step) {
    __syncthreads();
    const bool last = (t0 + n_mpc_step >= n_steps);
    if (last)                                         // the window of the last solve, for ddmpc_get_solution
      for (int f = tid; f < nf; f += blockDim.x) {
        if (f < P.npu) lw_up[b * P.npu + f] = pv[f]; else lw_yp[b * nyp + (f - P.npu)] = pv[f];
      }
    int viol = 0;
    for (int rho = tid; rho < r; rho += blockDim.x) {
      const int oidx = P.tabi[2 * RPs + rho];
      const int j = T.of[rho];
      int jy = -1;
      if constexpr (YB) jy = T.ofy[rho];
      if ((oidx >= 0 && oidx < nuse) || j >= 0 || jy >= 0 || last) {
        double beta = g[rho];
        for (int f = 0; f < nf; ++f) beta += pv[f] * g[(long long)(1 + f) * r + rho];
        bsh[rho] = beta;
        if (j >= 0 && T.test(j, beta, 0) != 0) viol = 1;
        if (jy >= 0 && T.test(jy, beta, 0) != 0) viol = 1;
      }
    }
    viol = __syncthreads_or(viol);
    int st = st0, it = 1;
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
      if (use || j >= 0 || jy >= 0 || last) {
        int sa = (iterate && j >= 0) ? s.act[j] : 0;
        const double beta = iterate ? box_beta<YB>(s, T, Mb, r, bsh[rho], rho) : bsh[rho];
        nonfin |= !(fabs(beta) < 1e300);
        if (use) {                                    // (an input row: no output component)
          double z;
          (void)box_component(P, RPs, T, rho, j, beta, sa, pv, &z);
          uo[oidx] = z;
        }
        if (iterate && jy >= 0) sa += 4 * s.act[jy];
        if (last && beta_ws) { beta_ws[b * (long long)P.rE + rho] = beta; act_ws[b * (long long)P.rE + rho] = (signed char)sa; }
      }
    }
    if (__syncthreads_or(nonfin)) st = 4;
    stc = (st > stc) ? st : stc;
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
