// ddmpc_setpoint_law.hpp -- DDMPC_OPT_SETPOINT_LAW: the setpoint as an argument of the warm step (ROBUST controllers on the
// register-resident kernels, slack NONE, scalar / diagonal weights; Route::Cold).
//
// The reduced system K0 beta = t is linear in t, and t is linear in the setpoints: a row rho < r that takes its target from a
// setpoint (tabi[1][rho] < 0: every prediction step, free or terminal) has t[rho] = s[rho mod (m+p)], s = [u_s; y_s].  So with
//     S[b][c][:] = K0_b^-1 1_c,      1_c[rho] = 1 iff rho < r, rho mod (m+p) = c and tabi[1][rho] < 0,        c < m + p,
// the law of ddmpc_prepare extends to
//     beta_b = sum_f past_b[f] gain[b][1 + f][:] + sum_c s_b[c] S[b][c][:]
// (column 0 of the gain is sum_c s[c] S[c] at the handle's own setpoints and is not read here), and a batch may track one
// setpoint per instance and per step without a new ddmpc_prepare.  m + p more columns of r doubles per instance.
//
// Kernels: ddmpc_setpoint_gain_kernel<NT> (S by substitutions through the exported factor, the scheme of ddmpc_gain_kernel with
// the multi-hot right-hand side 1_c), ddmpc_setpoint_tables_kernel / ddmpc_setpoint_gain_column_kernel (S from refining cold
// solves at the zero past window and the unit setpoint e_c: their beta IS S[c], there is no offset to subtract),
// ddmpc_setpoint_step_kernel (one step: the law above and the output stage with the instance's setpoint as target) and
// ddmpc_closed_loop_setpoint_kernel (the whole loop of an instance in one workgroup, a setpoint per solve).
// Included by the API translation unit only.  ddmpc_gain_kernel, ddmpc_warm_step_kernel and ddmpc_closed_loop_warm_kernel are not
// touched: a handle that never sets the option launches what it always launched.
#pragma once
#include "ddmpc_aux_kernels.hpp"

namespace ddmpc {

// S of every instance by substitutions through the exported factor: grid = batch, block = 256 = 16 groups of 16 lanes, one group
// per right-hand side 1_c (idle groups ride along with a zero right-hand side), the factor streamed through LDS one tile row at a
// time exactly as in ddmpc_gain_kernel (see there for the scheme; the only difference is the right-hand side, which has a one in
// every setpoint row of its channel instead of in one row).  sgain [batch][nch][r].  LDS: 2 x NT x 256 + 2 x 16 doubles.
template <int NT>
__global__ __launch_bounds__(256) void ddmpc_setpoint_gain_kernel(KParams P, int RPs, const double* __restrict__ lfac,
                                                                  const double* __restrict__ lfacT,
                                                                  double* __restrict__ sgain) {
  extern __shared__ __attribute__((aligned(16))) double gsm[];      // 2 x NT x 256 (tile rows) + 2 x 16 (reciprocal pivots)
  auto Lbuf = [&](int buf) __attribute__((always_inline)) -> double* { return gsm + buf * (NT * 256); };
  auto rinv = [&](int buf) __attribute__((always_inline)) -> double* { return gsm + 2 * NT * 256 + buf * 16; };
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, grp = lane >> 4, kk = lane & 15, wave = tid >> 6;
  const int r = P.r, nch = P.nch;
  const double* __restrict__ Lb = lfac + b * (long long)(NT * (NT + 1) / 2 * 256);
  const double* __restrict__ Tb = lfacT + b * (long long)(NT * (NT + 1) / 2 * 256);
  auto tile = [](int I, int J) { return (I * (I + 1) / 2 + J) << 8; };
  const int ntr = (r + 15) >> 4;                      // tile rows that hold real rows
  double stage[NT];
  auto fetch_fwd = [&](int I) __attribute__((always_inline)) {
    static_for<NT>([&](auto J) __attribute__((always_inline)) { if (J <= I) stage[J] = Lb[tile(I, J) + tid]; });
  };
  auto fetch_bwd = [&](int Ji) __attribute__((always_inline)) {
    static_for<NT>([&](auto I2) __attribute__((always_inline)) { if (I2 >= Ji && I2 < ntr) stage[I2] = Tb[tile(I2, Ji) + tid]; });
  };
  auto commit = [&](int buf, int lo, int hi) __attribute__((always_inline)) {      // slots lo..hi of `stage` -> LDS
    static_for<NT>([&](auto J) __attribute__((always_inline)) { if (J >= lo && J <= hi) Lbuf(buf)[J * 256 + tid] = stage[J]; });
  };
  for (int c0 = 0; c0 < nch; c0 += 16) {
    const int c = c0 + wave * 4 + grp;                 // this group's channel (c >= nch: zero right-hand side, nothing stored)
    double y[NT];
    static_for<NT>([&](auto J) __attribute__((always_inline)) { y[J] = 0.0; });
    // ---- forward substitution L y = 1_c ----------------------------------------------------
    __syncthreads();                                   // buffers free (previous pass done)
    fetch_fwd(0);
    commit(0, 0, 0);
    for (int I = 0; I < ntr; ++I) {
      const int buf = I & 1;
      __syncthreads();                                 // tile row I visible; the other buffer is free
      if (I + 1 < ntr) fetch_fwd(I + 1);               // in flight while this tile row is processed
      if (wave == 0 && lane < 16) rinv(buf)[lane] = 1.0 / Lbuf(buf)[I * 256 + lane * 17];
      __syncthreads();
      const double* Lr = Lbuf(buf) + kk;
      const int nrow = (r - 16 * I) < 16 ? (r - 16 * I) : 16;
      for (int ii = 0; ii < nrow; ++ii) {
        double s = 0.0;
        static_for<NT>([&](auto J) __attribute__((always_inline)) {
          if (J < I) s += Lr[J * 256 + ii * 16] * y[J];
          if (J == I) s += (kk < ii) ? Lr[J * 256 + ii * 16] * y[J] : 0.0;
        });
        s = row16_sum(s);
        const int i = 16 * I + ii;                     // (i < r <= RPs: inside the table)
        const double e = (c < nch && i % nch == c && P.tabi[1 * RPs + i] < 0) ? 1.0 : 0.0;
        const double yi = (e - s) * rinv(buf)[ii];
        static_for<NT>([&](auto J) __attribute__((always_inline)) { if (J == I && kk == ii) y[J] = yi; });
      }
      if (I + 1 < ntr) commit(buf ^ 1, 0, I + 1);
    }
    // ---- back substitution L' x = y ----------------------------------------------------------
    __syncthreads();
    fetch_bwd(ntr - 1);
    commit(0, ntr - 1, ntr - 1);
    for (int Ji = ntr - 1; Ji >= 0; --Ji) {
      const int buf = (ntr - 1 - Ji) & 1;
      __syncthreads();
      if (Ji > 0) fetch_bwd(Ji - 1);
      if (wave == 0 && lane < 16) rinv(buf)[lane] = 1.0 / Lbuf(buf)[Ji * 256 + lane * 17];
      __syncthreads();
      const double* Tr = Lbuf(buf) + kk;
      const int nrow = (r - 16 * Ji) < 16 ? (r - 16 * Ji) : 16;
      for (int ii = nrow - 1; ii >= 0; --ii) {
        const int i = 16 * Ji + ii;
        double s = 0.0;
        static_for<NT>([&](auto I2) __attribute__((always_inline)) {
          if (I2 >= Ji && I2 < ntr) {
            const int k = 16 * I2 + kk;
            if (k > i && k < r) s += Tr[I2 * 256 + ii * 16] * y[I2];
            if (k == i) s -= y[I2];                    // the owner lane folds y_i into the sum: no broadcast needed
          }
        });
        s = row16_sum(s);
        const double xi = -s * rinv(buf)[ii];
        static_for<NT>([&](auto J) __attribute__((always_inline)) { if (J == Ji && kk == ii) y[J] = xi; });
      }
      if (Ji > 0) commit(buf ^ 1, Ji - 1, ntr - 1);
    }
    if (c < nch) {
      double* g = sgain + (b * nch + c) * (long long)r;
      static_for<NT>([&](auto J) __attribute__((always_inline)) { if (16 * J + kk < r) g[16 * J + kk] = y[J]; });
    }
  }
}

// Refined S: scratch copies of the parameter tables (4 rows of RPs doubles, the layout of upload_params), one per channel c,
// whose row 2 (the setpoint targets) is the unit setpoint e_c.  A refining cold solve at the zero past window with copy c has
// the right-hand side 1_c.  The handle's own tables are only read.  tabs [nch][4][RPs].
__global__ void ddmpc_setpoint_tables_kernel(int RPs, int nch, const double* __restrict__ tabd, double* __restrict__ tabs) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nch * 4 * RPs) return;
  const int c = idx / (4 * RPs), e = idx - c * (4 * RPs), row = e / RPs, rho = e - row * RPs;
  tabs[idx] = (row == 2) ? ((rho % nch == c) ? 1.0 : 0.0) : tabd[e];
}
// ... and the beta of that solve written as S[c] (AUTO: for the instances the factor-export launch flagged only).
__global__ void ddmpc_setpoint_gain_column_kernel(long long batch, int r, int rE, int nch, int c, const double* __restrict__ beta,
                                                  double* __restrict__ sgain, const int* __restrict__ flags, int epoch) {
  const long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (idx >= batch * r) return;
  const long long b = idx / r;
  if (flags != nullptr && flags[b] != epoch) return;
  const int rho = (int)(idx - b * r);
  sgain[(b * nch + c) * (long long)r + rho] = beta[b * rE + rho];
}

// The output stage of warm_component with the target of the setpoint rows passed in (`tb`: the instance's own setpoint of the
// row's channel) instead of read from the shared table row tabd[2].  Scalar / diagonal weights only: the option refuses dense
// weighting matrices.
__device__ __forceinline__ double warm_component(const KParams& P, int RPs, int rho, double beta, const double* pv, double tb,
                                                 double* z_out) {
  const int kind = P.tabi[0 * RPs + rho];
  const int pidx = P.tabi[1 * RPs + rho];
  const double D = P.tabd[0 * RPs + rho];
  const double wq = P.tabd[3 * RPs + rho];
  const double t = (pidx >= 0) ? pv[pidx] : tb;
  const double z = t - P.lam * D * beta;
  double contrib = P.lam * beta * z;
  if (kind == K_UFREE || kind == K_YFREE) { const double dlt = z - tb; contrib += wq * dlt * dlt; }
  else if (kind == K_WINT) { const double sg = z - t; contrib += P.lamb_sigma * sg * sg; }
  else if (kind == K_WTERM) { const double sg = z - tb; contrib += P.lamb_sigma * sg * sg; }
  else if (kind == K_WPRED) {
    const double sg = -P.lam * beta / P.lamb_sigma;
    const double dlt = z - sg - tb;
    contrib += wq * dlt * dlt + P.lamb_sigma * sg * sg;
  }
  *z_out = z;
  return contrib;
}

// beta[rho] of the law above: nf columns of the gain (from column 1 on) against the window, nch columns of S against the
// setpoint.  pv [nf], sv [nch] in LDS; g = the instance's gain, sg = the instance's S.  All loads of a chunk of 8 columns are
// issued before they are consumed, as in ddmpc_warm_step_kernel (HBM-bound: keep bytes in flight).
__device__ __forceinline__ double setpoint_law_row(const double* __restrict__ g, const double* __restrict__ sg, int r, int rho,
                                                   int nf, int nch, const double* pv, const double* sv) {
  double beta = 0.0;
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
  const double* sc = sg + rho;
  for (int c = 0; c < nch; ++c) beta += sv[c] * sc[(long long)c * r];
  return beta;
}

// One warm step with a setpoint per instance: grid = batch, block = r rounded up to 64.  u_s [batch][m], y_s [batch][p].
// Outputs as ddmpc_warm_step_kernel: status = the status of the factorisation, 4 (solver_error) when anything is not finite
// -- a NaN or infinite setpoint reaches every row of beta through S --, iters = 1.  The beta / active-set workspace is not
// written (ddmpc_get_solution reconstructs with the shared table and is refused after this step).
// Fixed-size arrays: pv [WARM_MAX_NF] (nf = n (m + p) <= WARM_MAX_NF, checked when the option is set), sv [WARM_MAX_NF]
// (m + p <= nf), bsh [WARM_MAX_R] (r <= 271).
__global__ void ddmpc_setpoint_step_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                           const double* __restrict__ sgain, const int* __restrict__ prep_status,
                                           const double* __restrict__ u_past, const double* __restrict__ y_past,
                                           const double* __restrict__ u_s, const double* __restrict__ y_s,
                                           double* __restrict__ u_opt, double* __restrict__ cost, int* __restrict__ status,
                                           int* __restrict__ iters) {
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double sv[WARM_MAX_NF];
  __shared__ double red[32];
  __shared__ double bsh[WARM_MAX_R];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, r = P.r, nrhs = nf + 1, nch = P.nch;
  const int nyp = nf - P.npu;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  for (int c = tid; c < nch; c += blockDim.x)
    sv[c] = (c < P.m) ? u_s[b * P.m + c] : y_s[b * P.p + (c - P.m)];
  __syncthreads();
  const double* g = gain + b * (long long)nrhs * r;
  const double* sg = sgain + b * (long long)nch * r;
  for (int rho = tid; rho < r; rho += blockDim.x) bsh[rho] = setpoint_law_row(g, sg, r, rho, nf, nch, pv, sv);
  __syncthreads();
  double part = 0.0;
  bool finite = true;
  for (int rho = tid; rho < r; rho += blockDim.x) {
    const double beta = bsh[rho];
    double z;
    part += warm_component(P, RPs, rho, beta, pv, sv[rho % nch], &z);
    finite = finite && (fabs(beta) < 1e300);
    const int oidx = P.tabi[2 * RPs + rho];
    if (oidx >= 0) u_opt[b * (long long)((P.Ln - P.npu / P.m) * P.m) + oidx] = z;
  }
  part = wave_sum(part);
  const unsigned long long okmask = __ballot(finite);
  if ((tid & 63) == 0) { red[tid >> 6] = part; red[16 + (tid >> 6)] = (okmask == ~0ull) ? 0.0 : 1.0; }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, bad = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { tot += red[w]; bad += red[16 + w]; }
    int st = prep_status[b];
    if (bad != 0.0 || !(fabs(tot) < 1e300)) st = 4;
    cost[b] = tot;
    status[b] = st;
    if (iters) iters[b] = 1;
  }
}

// Whole closed loop of one instance in one workgroup with a setpoint schedule: ddmpc_closed_loop_warm_kernel with the law above.
// u_ref [batch][n_steps][m], y_ref [batch][n_steps][p]: the solve made at step t0 uses row t0; rows between solves are not read.
// An instance stops (status 4, NaN rows from that solve on, x and the windows as they stood) when the inputs a solve hands to
// the plant are not finite -- a non-finite setpoint --, as it does when its factorisation failed.
// Fixed-size arrays as in ddmpc_closed_loop_warm_kernel (pv, uo [WARM_MAX_NF], xs [16], bsh [WARM_MAX_R]) plus sv [WARM_MAX_NF];
// ddmpc_closed_loop_setpoints checks n_mpc_step * m <= WARM_MAX_NF and ns <= 16, the option n (m + p) <= WARM_MAX_NF and r <= 271.
__global__ void ddmpc_closed_loop_setpoint_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                                  const double* __restrict__ sgain, const int* __restrict__ prep_status, int ns,
                                                  const double* __restrict__ pl, int n_steps, int n_mpc_step,
                                                  double* __restrict__ x, double* __restrict__ u_past,
                                                  double* __restrict__ y_past, const double* __restrict__ w,
                                                  const double* __restrict__ u_ref, const double* __restrict__ y_ref,
                                                  double* __restrict__ u_sys, double* __restrict__ y_sys,
                                                  int* __restrict__ status_out) {
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double sv[WARM_MAX_NF];
  __shared__ double uo[WARM_MAX_NF];      // the first n_mpc_step*m entries of optimal_u
  __shared__ double xs[16];
  __shared__ double bsh[WARM_MAX_R];
  __shared__ int st_sh;
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, r = P.r, nrhs = nf + 1, m = P.m, p = P.p, nch = P.nch;
  const int n = P.npu / m, nyp = nf - P.npu;
  const double* A = pl;
  const double* Bm = A + ns * ns;
  const double* C = Bm + ns * m;
  const double* Dm = C + p * ns;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  if (tid < ns) xs[tid] = x[b * ns + tid];
  if (tid == 0) st_sh = prep_status[b];
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);
  const double* g = gain + b * (long long)nrhs * r;
  const double* sg = sgain + b * (long long)nch * r;
  const int nuse = n_mpc_step * m;
  double* up = pv;
  double* yp = pv + P.npu;
  for (int t0 = 0; t0 < n_steps; t0 += n_mpc_step) {
    for (int c = tid; c < nch; c += blockDim.x)     // (sv was last read before the barrier ahead of the plant steps)
      sv[c] = (c < m) ? u_ref[(b * n_steps + t0) * m + c] : y_ref[(b * n_steps + t0) * p + (c - m)];
    __syncthreads();                                  // the setpoint and the window of the last plant steps visible; bsh, uo free
    for (int rho = tid; rho < r; rho += blockDim.x) {
      const int oidx = P.tabi[2 * RPs + rho];
      if (oidx >= 0 && oidx < nuse) bsh[rho] = setpoint_law_row(g, sg, r, rho, nf, nch, pv, sv);
    }
    __syncthreads();
    for (int rho = tid; rho < r; rho += blockDim.x) {
      const int oidx = P.tabi[2 * RPs + rho];
      if (oidx >= 0 && oidx < nuse) {
        double z;
        (void)warm_component(P, RPs, rho, bsh[rho], pv, sv[rho % nch], &z);
        uo[oidx] = z;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int nsub = (t0 + n_mpc_step <= n_steps) ? n_mpc_step : n_steps - t0;
      int st = st_sh;
      if (st <= 1)
        for (int i = 0; i < nsub * m; ++i)
          if (!(fabs(uo[i]) < 1e300)) st = 4;
      st_sh = st;
      for (int j = 0; j < nsub; ++j) {
        const int k = t0 + j;
        double* us = u_sys + (b * n_steps + k) * m;
        double* ys = y_sys + (b * n_steps + k) * p;
        if (st > 1) {
          for (int i = 0; i < m; ++i) us[i] = nanv;
          for (int i = 0; i < p; ++i) ys[i] = nanv;
          continue;
        }
        const double* uk = uo + j * m;
        const double* wk = w + (b * n_steps + k) * p;
        double xn[16];                             // (ns <= 16: checked by ddmpc_closed_loop_setpoints)
        for (int i = 0; i < p; ++i) {              // y = C x + D u + w with the state BEFORE the update
          double s = wk[i];
          for (int q = 0; q < ns; ++q) s += C[i * ns + q] * xs[q];
          for (int q = 0; q < m; ++q) s += Dm[i * m + q] * uk[q];
          ys[i] = s;
        }
        for (int i = 0; i < ns; ++i) {
          double s = 0.0;
          for (int q = 0; q < ns; ++q) s += A[i * ns + q] * xs[q];
          for (int q = 0; q < m; ++q) s += Bm[i * m + q] * uk[q];
          xn[i] = s;
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
  if (tid == 0) status_out[b] = st_sh;
}

}  // namespace ddmpc
