// ddmpc_rr3_law.hpp -- DDMPC_OPT_LARGE_AFFINE_LAW for ROBUST controllers on the phase kernels (Route::RobustPhases, 272 .. 1024 rows).
//
// With the data and the weights fixed, beta of the empty active set is affine in the past window w = [u_past; y_past]
// (controller.py:577-581):  K0 beta = t(w) = t0 + E w,  so  beta(w) = g0 + G' w  with
//     g0 = K0^-1 t0,   column j of G' = K0^-1 e_pos(j)      (e_pos(j): the position of the component that takes w_j)
// ddmpc_prepare forms it on the factor K0 = L L' that rr3 keeps (packed, "boxed last" order, Minv of every 64 x 64 diagonal block):
//
//   rr3_law_fwd_kernel    Y = L^-1 RHS for 64 right-hand sides per workgroup, grid (column blocks, instances): the rr3_w_forward
//                         scheme (accumulator tiles P = RHS_b - L(b, <b) Y(<b) on the matrix pipe, then Minv_b P through LDS);
//                         the factor is streamed once per column block.  RHS: the n(m+p) unit vectors and t0, or (refinement) a
//                         residual from rr3_law_resid_kernel.
//   rr3_law_bwd_kernel    X = L^-T Y for the same 64 columns, block rows from the last: P = Y_b - L(>b, b)' X(>b) (contraction over
//                         the rows below the block, four per MFMA), X_b = Minv_b' P; X scattered to component order through perm
//                         into the law [batch][n(m+p)+1][r] (or added to it: refinement).
//   rr3_law_resid_kernel  residual E - (H (H' X) + lam D0 X) per column from the exact Hankel products of the phase pipeline (run on
//                         the law columns as a virtual batch); flags the instances above the refinement threshold.
//   rr3_law_step_kernel   per control step: beta = g0 + G' w (the law streamed once), z, optimal_u, cost, status, the beta / active-set
//                         workspace and the rr3 record -- or, under the slack box, a flag when a boxed slack leaves the box (those
//                         instances are re-solved by rr3_solve_kernel on the kept factor, restricted to them).
//   rr3_setpoint_law_step_kernel   DDMPC_OPT_LARGE_SETPOINTS: its twin with a setpoint per instance -- the law's rows 1 .. nf and the
//                         m + p rows of S = K0^-1 [1_c], which the three build kernels form as a second kind of right-hand side.
#pragma once
#include "ddmpc_rr3.hpp"

namespace ddmpc {

// Value of right-hand side c (0: t0, 1 .. nf: the unit window e_{c-1}) at component rho: column c of the law is row c of
// ddmpc_get_gain's [nf+1][r] block.
// The right-hand sides of the three build kernels come in two kinds.  RR3_RHS_LAW: the nf + 1 columns above, into the law.
// RR3_RHS_SETPOINT (DDMPC_OPT_LARGE_SETPOINTS): the m + p multi-hot columns 1_c of ddmpc_setpoint_law.hpp -- one
// where rho mod (m+p) = c and the component takes its target from a setpoint --, `nf` then counts these columns, into S
// [batch][m+p][r].  The kernels' `law` argument is the destination of the kind.
enum : int { RR3_RHS_LAW = 0, RR3_RHS_SETPOINT = 1 };
__device__ __forceinline__ int rr3_law_nrhs(int nf, int kind) { return kind == RR3_RHS_SETPOINT ? nf : nf + 1; }
__device__ __forceinline__ double rr3_law_e(const KParams& P, int RPs, int rho, int c, int kind = RR3_RHS_LAW) {
  const int pidx = P.tabi[1 * RPs + rho];
  if (kind == RR3_RHS_SETPOINT) return (pidx < 0 && rho % P.nch == c) ? 1.0 : 0.0;
  if (c == 0) return (pidx < 0) ? P.tabd[2 * RPs + rho] : 0.0;
  return (pidx == c - 1) ? 1.0 : 0.0;
}

// grid = (ceil((nf+1)/64), instances of the chunk), RR2_TS threads.  Y: chunk-local [instance][column block][VL][64], row-major.
// FROM_BUF: the right-hand sides are rhs [chunk instance][nf+1][r] (component order), else the unit windows and t0.
// only: instances that take part (nullptr: all); nolaw: set to 1 for an instance whose factor has a failed pivot.
template <bool FROM_BUF>
__global__ __launch_bounds__(RR2_TS) void rr3_law_fwd_kernel(Rr3 S, KParams P, int RPs, long long b0, int nf, const double* __restrict__ rhs,
                                                             const int* __restrict__ only, double* __restrict__ Y, int* __restrict__ nolaw,
                                                             int kind) {
  __shared__ __attribute__((aligned(16))) double Pb[64 * 65];
  const int cb = blockIdx.x, ncb = gridDim.x;
  const long long bl = blockIdx.y, b = b0 + bl;
  if (only != nullptr && only[b] == 0) return;                              // (workgroup-uniform)
  const int r = S.r, nrhs = rr3_law_nrhs(nf, kind), VL = (r + 63) & ~63;
  const int* perm = S.perm;
  const double* Lm = S.ws + b * S.stride;
  const double* m64 = S.m64 + b * S.m64_stride;
  const unsigned long long live = S.dd[4 * b + 2];
  double* Yb = Y + (bl * ncb + cb) * (long long)VL * 64;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = wave & 3, ch = wave >> 2;
  const int nb = (r + 63) >> 6;
  if (!FROM_BUF && cb == 0) {
    int bad = 0;
    for (int i = tid; i < r; i += blockDim.x) bad |= S.skip[b * S.s_stride + i] ? 1 : 0;
    if (__syncthreads_or(bad) && tid == 0) nolaw[b] = 1;
  }
  int ccol[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { const int c = 64 * cb + 16 * (ch + 2 * t) + l15; ccol[t] = (c < nrhs) ? c : -1; }
  for (int bk = 0; bk < nb; ++bk) {
    const int i0 = 64 * bk;
    const int irow = i0 + 16 * rt + l15;                                     // A operand: this lane's row of the factor
    const double* Li = Lm + pk_row((size_t)(irow < r ? irow : r - 1)) + 4 * l4;
    const double az = (irow < r) ? 1.0 : 0.0;
    d4 acc[2];
    acc[0] = d4{0.0, 0.0, 0.0, 0.0}; acc[1] = d4{0.0, 0.0, 0.0, 0.0};
    unsigned long long lv = live & ((1ull << (4 * bk)) - 1ull);
    while (lv != 0ull) {
      const int jc = __builtin_ctzll(lv);
      lv &= lv - 1ull;
      const d4 la = *reinterpret_cast<const d4*>(Li + 16 * jc);
      const double* yr = Yb + (size_t)(16 * jc + 4 * l4) * 64 + l15;        // rows 16 jc + 4 l4 + e of Y
      double yv[2][4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[t][e] = yr[(size_t)e * 64 + 16 * (ch + 2 * t)];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t] = rr2_mfma(la[e] * az, yv[t][e], acc[t]);
    }
    // P = RHS - acc into LDS: register q of lane (l4, l15) = entry [16 rt + l4 + 4 q][16 ct + l15]
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rloc = 16 * rt + l4 + 4 * q, i = i0 + rloc;
        double e = 0.0;
        if (i < r && ccol[t] >= 0) {
          const int rho = perm[i];
          e = FROM_BUF ? rhs[(bl * nrhs + ccol[t]) * (long long)r + rho] : rr3_law_e(P, RPs, rho, ccol[t], kind);
        }
        Pb[rloc * 65 + 16 * (ch + 2 * t) + l15] = e - acc[t][q];
      }
    }
    __syncthreads();
    // Y_b = Minv_b P: tile (rt, ct) = sum_{u <= rt} Minv(rt, u) P(u, ct)
    const double* Mb = m64 + (size_t)bk * 4096 + (size_t)(16 * rt + l15) * 64 + 4 * l4;
    d4 x[2];
    x[0] = d4{0.0, 0.0, 0.0, 0.0}; x[1] = d4{0.0, 0.0, 0.0, 0.0};
    for (int u = 0; u <= rt; ++u) {
      const d4 mv = *reinterpret_cast<const d4*>(Mb + 16 * u);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[t] = rr2_mfma(mv[e], Pb[(16 * u + 4 * l4 + e) * 65 + 16 * (ch + 2 * t) + l15], x[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 16 * rt + l4 + 4 * q;
        Yb[(size_t)i * 64 + 16 * (ch + 2 * t) + l15] = (i < r) ? x[t][q] : 0.0;
      }
    __syncthreads();                                                         // the rows of Y of this block are visible (workgroup scope)
  }
}

// X = L^-T Y in place, then law[b][c][perm[i]] = X[i][c] (ADD: +=).  Same grid and Y as rr3_law_fwd_kernel.  nolaw: set to 1 for
// an instance whose law has a non-finite entry.
template <bool ADD>
__global__ __launch_bounds__(RR2_TS) void rr3_law_bwd_kernel(Rr3 S, long long b0, int nf, const int* __restrict__ only, double* __restrict__ Y,
                                                             double* __restrict__ law, int* __restrict__ nolaw, int kind) {
  __shared__ __attribute__((aligned(16))) double Pb[64 * 65];
  const int cb = blockIdx.x, ncb = gridDim.x;
  const long long bl = blockIdx.y, b = b0 + bl;
  if (only != nullptr && only[b] == 0) return;                              // (workgroup-uniform)
  const int r = S.r, nrhs = rr3_law_nrhs(nf, kind), VL = (r + 63) & ~63;
  const int* perm = S.perm;
  const double* Lm = S.ws + b * S.stride;
  const double* m64 = S.m64 + b * S.m64_stride;
  const unsigned long long live = S.dd[4 * b + 2];
  double* Yb = Y + (bl * ncb + cb) * (long long)VL * 64;
  double* lb = law + b * nrhs * (long long)r;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = wave & 3, ch = wave >> 2;
  const int nb = (r + 63) >> 6;
  int bad = 0;
  for (int bk = nb - 1; bk >= 0; --bk) {
    const int k0 = 64 * bk;
    // acc = L(>b, b)' X(>b): A(m, k) = L(i_k, k0 + 16 rt + m), B(k, n) = X(i_k, 16 ct + n), four rows i_k per MFMA
    d4 acc[2];
    acc[0] = d4{0.0, 0.0, 0.0, 0.0}; acc[1] = d4{0.0, 0.0, 0.0, 0.0};
    const int col = k0 + 16 * rt + l15;
    constexpr int NU = 4;
    for (int ib = k0 + 64; ib < r; ib += 4 * NU) {
      double a[NU], xv[NU][2];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int i = ib + 4 * u + l4;
        const bool ok = i < r && ((live >> (i >> 4)) & 1ull) != 0ull;
        const int ic = i < r ? i : r - 1;
        a[u] = Lm[pk_row((size_t)ic) + col];
        a[u] = ok ? a[u] : 0.0;
#pragma unroll
        for (int t = 0; t < 2; ++t) xv[u][t] = Yb[(size_t)ic * 64 + 16 * (ch + 2 * t) + l15];
      }
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t] = rr2_mfma(a[u], xv[u][t], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rloc = 16 * rt + l4 + 4 * q, i = k0 + rloc, cc = 16 * (ch + 2 * t) + l15;
        Pb[rloc * 65 + cc] = ((i < r) ? Yb[(size_t)i * 64 + cc] : 0.0) - acc[t][q];
      }
    __syncthreads();
    // X_b = Minv_b' P: tile (rt, ct) = sum_{u >= rt} Minv(u, rt)' P(u, ct); A(m, k) = Minv(16 u + k, 16 rt + m)
    const double* Mb = m64 + (size_t)bk * 4096 + 16 * rt + l15;
    d4 x[2];
    x[0] = d4{0.0, 0.0, 0.0, 0.0}; x[1] = d4{0.0, 0.0, 0.0, 0.0};
    for (int u = rt; u < 4; ++u) {
      double mv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kr = 16 * u + 4 * l4 + e;
        mv[e] = (k0 + kr < r) ? Mb[(size_t)kr * 64] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) x[t] = rr2_mfma(mv[e], Pb[(16 * u + 4 * l4 + e) * 65 + 16 * (ch + 2 * t) + l15], x[t]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = k0 + 16 * rt + l4 + 4 * q, cc = 16 * (ch + 2 * t) + l15, c = 64 * cb + cc;
        const double v = (i < r) ? x[t][q] : 0.0;
        Yb[(size_t)i * 64 + cc] = v;
        if (i < r && c < nrhs) {
          double* dst = lb + (long long)c * r + perm[i];
          const double nv = ADD ? *dst + v : v;
          *dst = nv;
          bad |= (fabs(nv) < 1e300) ? 0 : 1;
        }
      }
    __syncthreads();
  }
  if (__syncthreads_or(bad) && tid == 0) nolaw[b] = 1;
}

// Residual of law column c of chunk instance bl: R = E_c - (H (H' X) + lam D0 X), ZP: Hankel partial sums of the virtual instance
// bl (nf+1) + c.  flag[b] = 1 when |R|_inf / max(|E_c|_inf, |H (H' X)|_inf, |lam D0 X|_inf) exceeds the refinement threshold, or
// always (force); nolaw (final check): the same flag.  Deliberately NOT a normwise backward error (relative to |G| |X|): a unit
// column's X is large in the null space of H' (G is rank deficient on LTI data), and a window's beta combines such columns with
// cancellation, so column errors that are small relative to |X| are not small relative to beta(w).  Judged relative to |G| |X|,
// 608-row laws passed and served steps 4e-6 .. 1e-5 away from the refined cold solve; judged this way they are marked "no law"
// and their steps take the re-solve.
// grid = (nf+1, instances of the chunk), 256 threads.
__global__ __launch_bounds__(256) void rr3_law_resid_kernel(KParams P, int RPs, long long b0, int nf, const double* __restrict__ law,
                                                            const double* __restrict__ ZP, int VL, double* __restrict__ R,
                                                            int* __restrict__ flag, int force, int* __restrict__ nolaw, int kind) {
  __shared__ double red[8];
  const int c = blockIdx.x, nrhs = rr3_law_nrhs(nf, kind), r = P.r, tid = threadIdx.x;
  const long long bl = blockIdx.y, b = b0 + bl;
  const double* xc = law + (b * nrhs + c) * (long long)r;
  const double* zp = ZP + (bl * nrhs + c) * (long long)RR2_NG * VL;
  double* Rc = R + (bl * nrhs + c) * (long long)r;
  double rmx = 0.0, emx = 0.0;
  for (int rho = tid; rho < r; rho += blockDim.x) {
    const double e = rr3_law_e(P, RPs, rho, c, kind);
    double hz = 0.0;
#pragma unroll
    for (int g = 0; g < RR2_NG; ++g) hz += zp[g * (long long)VL + rho];
    const double dx = P.lam * P.tabd[0 * RPs + rho] * xc[rho];
    const double rv = e - hz - dx;
    Rc[rho] = rv;
    rmx = fmax(rmx, (rv == rv) ? fabs(rv) : 1e300);
    emx = fmax(emx, fmax(fabs(e), fmax(fabs(hz), fabs(dx))));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { rmx = fmax(rmx, __shfl_xor(rmx, off, 64)); emx = fmax(emx, __shfl_xor(emx, off, 64)); }
  if ((tid & 63) == 0) { red[tid >> 6] = rmx; red[4 + (tid >> 6)] = emx; }
  __syncthreads();
  if (tid == 0) {
    double r_ = 0.0, e_ = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { r_ = fmax(r_, red[w]); e_ = fmax(e_, red[4 + w]); }
    if (force || !(r_ / fmax(e_, 1e-300) <= P.refine_res)) {
      flag[b] = 1;
      if (nolaw != nullptr) nolaw[b] = 1;
    }
  }
}

// One control step on the law.  grid = batch, RR2_TS threads.  need[b] = si[2 b] = 1 (si: the layout the Hankel kernels skip by):
// instance b is left to the filtered re-solve (no law, or a
// boxed slack outside the box); else everything rr3_solve_kernel writes for an instance that stops after the first iterate.
constexpr int RR3_LAW_NG = 4;                 // groups of law rows summed apart (then added in LDS)
__global__ __launch_bounds__(RR2_TS) void rr3_law_step_kernel(Rr3 S, KParams P, int RPs, int nf, const double* __restrict__ law,
                                                              const int* __restrict__ nolaw, const double* __restrict__ u_past,
                                                              const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                              double* __restrict__ cost, int* __restrict__ status, int* __restrict__ iters,
                                                              double* __restrict__ beta_ws, signed char* __restrict__ act_ws,
                                                              int* __restrict__ need, int* __restrict__ si) {
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
  int out = 0;
  if (P.convex)                                                            // slack box (controller.py:659): the first iterate's switch test
    for (int i = S.nA + tid; i < r; i += nthr) {
      const double sh = P.sig_scale * bv[i];
      out |= (sh > P.bound || sh < -P.bound) ? 1 : 0;
    }
  if (__syncthreads_or(out)) {
    if (tid == 0) { need[b] = 1; si[2 * b] = 1; }
    return;
  }
  int* kq = S.kq + b * S.kstride;
  for (int i = tid; i < r; i += nthr) kq[4 + RR3_KMAX + i] = 0;
  if (tid == 0) {
    need[b] = 0; si[2 * b] = 0;
    kq[0] = 0; kq[1] = 0; kq[2] = 1; kq[3] = 0;
    const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
    kq[4 + RR3_KMAX + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + RR3_KMAX + S.rv + 1] = (int)(t_end - t_begin);
  }
  rr3_outputs(P, RPs, S, b, perm, tv, bv, act, 0, 1, red, u_opt, cost, status, iters, beta_ws, act_ws, part, part + 1024);
}

// DDMPC_OPT_LARGE_SETPOINTS: the twin of rr3_law_step_kernel with a setpoint per instance.
//     beta = sum_f w_f law[1 + f] + sum_c s_c S[c]        (column 0 of the law, the offset at the shared setpoints, is not read)
// The same streaming scheme over nf + (m+p) rows: the rows of S follow those of the law in the four groups.  tv and tb of the
// output stage come from the window or the instance's setpoint (sp).  An instance with no law, with no setpoint law (nosp) or
// outside the box is left to the filtered solve on the kept factor with the same setpoints.  A non-finite setpoint reaches
// every row of beta through S: status 4 from the output stage (or from the solve, should the switch test flag it).
__global__ __launch_bounds__(RR2_TS) void rr3_setpoint_law_step_kernel(Rr3 S, KParams P, int RPs, int nf, const double* __restrict__ law,
                                                                       const int* __restrict__ nolaw, const double* __restrict__ u_past,
                                                                       const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                                       double* __restrict__ cost, int* __restrict__ status,
                                                                       int* __restrict__ iters, double* __restrict__ beta_ws,
                                                                       signed char* __restrict__ act_ws, int* __restrict__ need,
                                                                       int* __restrict__ si, const double* __restrict__ sgain,
                                                                       const int* __restrict__ nosp, Rr3Setpoint sp) {
  __shared__ __attribute__((aligned(16))) double part[RR3_LAW_NG * 1024];
  __shared__ double wv[2 * WARM_MAX_NF];                                    // the window (nf), then the setpoint (m + p <= nf)
  __shared__ double tv[1024], bv[1024];
  __shared__ int act[1024];
  __shared__ double red[16];
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = nthr >> 6;
  if (nolaw[b] != 0 || nosp[b] != 0) {                                      // (workgroup-uniform)
    if (tid == 0) { need[b] = 1; si[2 * b] = 1; }
    return;
  }
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();
  const int r = S.r, nch = P.nch, nrows = nf + nch, n = P.npu / P.m;
  const int* perm = S.perm;
  const double* up = u_past + b * (long long)P.npu;
  const double* yp = y_past + b * (long long)(n * P.p);
  for (int j = tid; j < nrows; j += nthr)
    wv[j] = (j < P.npu) ? up[j] : (j < nf) ? yp[j - P.npu]
            : (j - nf < P.m) ? sp.us[b * sp.su + (j - nf)] : sp.ys[b * sp.sy + (j - nf - P.m)];
  __syncthreads();
  // row j of the stream: law row 1 + j (j < nf), else row j - nf of S
  const double* gl = law + (b * (nf + 1) + 1) * (long long)r;
  const double* sg = sgain + b * nch * (long long)r;
  const int nc = (r + 63) >> 6, per = (nrows + RR3_LAW_NG - 1) / RR3_LAW_NG;
  for (int task = wave; task < nc * RR3_LAW_NG; task += nwave) {
    const int c = task / RR3_LAW_NG, g = task - c * RR3_LAW_NG;
    const int rho = 64 * c + lane, rc = rho < r ? rho : r - 1;
    const int j0 = g * per, j1 = (j0 + per < nrows) ? j0 + per : nrows;
    double s0 = 0.0, s1 = 0.0;
    int j = j0;
    for (; j + 8 <= j1; j += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (j + e < nf) ? gl[(long long)(j + e) * r + rc] : sg[(long long)(j + e - nf) * r + rc];
#pragma unroll
      for (int e = 0; e < 8; e += 2) { s0 = fma(v[e], wv[j + e], s0); s1 = fma(v[e + 1], wv[j + e + 1], s1); }
    }
    for (; j < j1; ++j) s0 = fma((j < nf) ? gl[(long long)j * r + rc] : sg[(long long)(j - nf) * r + rc], wv[j], s0);
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
    tv[i] = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : rr3_setpoint(P, RPs, rho, b, sp);
    act[i] = 0;
  }
  __syncthreads();
  int out = 0;
  if (P.convex)                                                            // slack box: the first iterate's switch test, on beta
    for (int i = S.nA + tid; i < r; i += nthr) {
      const double sh = P.sig_scale * bv[i];
      out |= (sh > P.bound || sh < -P.bound) ? 1 : 0;
    }
  if (__syncthreads_or(out)) {
    if (tid == 0) { need[b] = 1; si[2 * b] = 1; }
    return;
  }
  int* kq = S.kq + b * S.kstride;
  for (int i = tid; i < r; i += nthr) kq[4 + RR3_KMAX + i] = 0;
  if (tid == 0) {
    need[b] = 0; si[2 * b] = 0;
    kq[0] = 0; kq[1] = 0; kq[2] = 1; kq[3] = 0;
    const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
    kq[4 + RR3_KMAX + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + RR3_KMAX + S.rv + 1] = (int)(t_end - t_begin);
  }
  rr3_outputs(P, RPs, S, b, perm, tv, bv, act, 0, 1, red, u_opt, cost, status, iters, beta_ws, act_ws, part, part + 1024, sp);
}

}  // namespace ddmpc
