// ddmpc_rr3_box_law.hpp -- DDMPC_OPT_LARGE_BOX_LAW: control steps of a bounded ROBUST handle on the phase kernels (272 .. 1024 rows)
// served from the affine law of the empty active set while they stay inside the box ("Law inside the box").
//
// The law beta(w) = g0 + G' w is the solution of K0 beta = t(w) on the kept factor of the EMPTY active set: no bound enters it, so
// ddmpc_prepare forms it with the kernels of ddmpc_rr3_law.hpp as they are (the "boxed last" order comes with the descriptor).  The
// first iterate of the bounded kernels (ddmpc_rr3_box.hpp) is a test of that same beta against the component table; a step whose
// beta passes it ends there with the empty set.  rr3_law_box_step_kernel evaluates the law, runs that test and
//   no component outside its box   writes what rr3_solve_box_kernel writes for an instance that stops at the first test
//   a violation, or no law         flags the instance: the bounded solve launches that follow serve the flagged instances only
// A twin of rr3_law_step_kernel and not a parameter of it, for the reason given in ddmpc_rr3_box.hpp: the handles without bounds
// keep their kernel as it is.
#pragma once
#include "ddmpc_rr3_box.hpp"
#include "ddmpc_rr3_law.hpp"

namespace ddmpc {

// One control step on the law under the component table.  grid = batch, RR2_TS threads.  need[b] = si[2 b] = 1 (si: the layout the
// Hankel kernels skip by): instance b is left to the filtered re-solve, and nothing else of it is written.  cap: the columns of W
// of the bounded kernel that serves the handle (the layout of the per-instance record).
__global__ __launch_bounds__(RR2_TS) void rr3_law_box_step_kernel(Rr3 S, KParams P, int RPs, int nf, const double* __restrict__ law,
                                                                  const int* __restrict__ nolaw, const double* __restrict__ u_past,
                                                                  const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                                  double* __restrict__ cost, int* __restrict__ status,
                                                                  int* __restrict__ iters, double* __restrict__ beta_ws,
                                                                  signed char* __restrict__ act_ws, int* __restrict__ need,
                                                                  int* __restrict__ si, Rr3Box X, int cap) {
  __shared__ __attribute__((aligned(16))) double part[RR3_LAW_NG * 1024];
  __shared__ double wv[WARM_MAX_NF + 1];
  __shared__ double tv[1024], bv[1024];
  __shared__ int act[1024];
  __shared__ double red[16];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = nthr >> 6;
  if (nolaw[b] != 0) {                                                      // (workgroup-uniform)
    if (tid == 0) { need[b] = 1; si[2 * b] = 1; }
    return;
  }
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();
  const int r = S.r, nrhs = nf + 1, n = P.npu / P.m;
  const int* perm = S.perm;
  const double* up = u_past + b * (long long)P.npu;
  const double* yp = y_past + b * (long long)(n * P.p);
  for (int j = tid; j < nrhs; j += nthr) wv[j] = (j == 0) ? 1.0 : ((j - 1 < P.npu) ? up[j - 1] : yp[j - 1 - P.npu]);
  __syncthreads();
  // beta = g0 + G' w: tasks (64 components, group of law rows), eight loads in flight per lane
  const double* gl = law + b * nrhs * (long long)r;
  const int nc = (r + 63) >> 6, per = (nrhs + RR3_LAW_NG - 1) / RR3_LAW_NG;
  for (int task = wave; task < nc * RR3_LAW_NG; task += nwave) {
    const int c = task / RR3_LAW_NG, g = task - c * RR3_LAW_NG;
    const int rho = 64 * c + lane, rc = rho < r ? rho : r - 1;
    const int j0 = g * per, j1 = (j0 + per < nrhs) ? j0 + per : nrhs;
    double s0 = 0.0, s1 = 0.0;
    int j = j0;
    for (; j + 8 <= j1; j += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = gl[(long long)(j + e) * r + rc];
#pragma unroll
      for (int e = 0; e < 8; e += 2) { s0 = fma(v[e], wv[j + e], s0); s1 = fma(v[e + 1], wv[j + e + 1], s1); }
    }
    for (; j < j1; ++j) s0 = fma(gl[(long long)j * r + rc], wv[j], s0);
    part[g * 1024 + rho] = s0 + s1;
  }
  __syncthreads();
  for (int i = tid; i < r; i += nthr) {
    const int rho = perm[i];
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < RR3_LAW_NG; ++g) s += part[g * 1024 + rho];
    const int pidx = P.tabi[1 * RPs + rho];
    bv[i] = s;
    tv[i] = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : P.tabd[2 * RPs + rho];
    act[i] = 0;
  }
  __syncthreads();
  // the first test of rr3_solve_box_kernel: every boxed component (slack, input, output) of the empty set against its lo / hi
  int out = 0;
  for (int s = tid; s < X.nbox; s += nthr) {
    const double hat = fma(X.bd[(size_t)R3B_C * X.nbox + s], bv[X.ip[s]], X.bd[(size_t)R3B_A * X.nbox + s]);
    out |= (hat > X.bd[(size_t)R3B_HI * X.nbox + s] || hat < X.bd[(size_t)R3B_LO * X.nbox + s]) ? 1 : 0;
  }
  if (__syncthreads_or(out)) {
    if (tid == 0) { need[b] = 1; si[2 * b] = 1; }
    return;
  }
  int* kq = S.kq + b * S.kstride;
  for (int i = tid; i < r; i += nthr) kq[4 + cap + i] = 0;
  if (tid == 0) {
    need[b] = 0; si[2 * b] = 0;
    kq[0] = 0; kq[1] = 0; kq[2] = 1; kq[3] = 0;
    const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
    kq[4 + cap + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + cap + S.rv + 1] = (int)(t_end - t_begin);
    kq[4 + cap + S.rv + 2] = 0;                                             // the most components active in any iteration
  }
  rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, 0, 1, red, u_opt, cost, status, iters, beta_ws, act_ws);
}

}  // namespace ddmpc
