// ddmpc_rr3_box.hpp -- input and output bounds for ROBUST controllers beyond the register-resident kernels (272 .. 1024 rows) on
// the phase kernels: rr3_solve_box_kernel, a twin of rr3_solve_kernel (ddmpc_rr3.hpp) whose box is table-driven.
// A twin and not a template parameter of that kernel: with the two in one body the compiler allocated the scalar registers of the
// unbounded instantiation differently (compared in its assembly), and the handles without bounds must keep their kernel as it is.
// Everything else -- the factor of the empty active set, rr3_w_forward, rr3_w_gram, the k x k Cholesky, the substitutions, Rr3Lds --
// is shared.
#pragma once
#include <type_traits>
#include "ddmpc_rr3.hpp"

namespace ddmpc {


// The table of boxed components, shared by the batch (global memory: it stays in L2) and sized by nbox: ascending by POSITION
// in the "boxed last" order, the slack before the output on a shared row.  Component s sits at position ip[s] and is an output
// component when ip[nbox + s] != 0; hat_s = a_s + c_s beta[ip[s]] is tested against lo_s / hi_s by the rule of BoxTab::test
// (ddmpc_box_law.hpp); active, it changes the diagonal by d_s and the target by shlo_s / shhi_s:
//   slack   a = 0,   c = -lam / lamb_sigma, lo / hi = -+ c eps_max,   d = lam (D0 - D1)
//   input   a = u_s, c = -lam / r,          lo / hi = u_min / u_max,  d = lam / r
//   output  a = y_s, c = -lam / q,          lo / hi = y_min / y_max,  d = lam / q
// Behind the seven columns: [u_min (m) | u_max (m) | y_min (p) | y_max (p)] for the output stage (+-infinity where there is none).
struct Rr3Box {
  int nbox;
  const int* ip;                                      // [position (nbox) | output component? (nbox) | setpoint channel, -1 for a slack (nbox) | terminal constraint? (1)]
  const double* bd;                                   // [a | c | lo | hi | 1/d | shlo | shhi] (nbox each), then the bounds per channel
};
enum : int { R3B_A = 0, R3B_C, R3B_LO, R3B_HI, R3B_INVD, R3B_SHLO, R3B_SHHI, R3B_NV };
// DDMPC_OPT_LARGE_BOX_LAW: the instance filter of the bounded kernels (rr3_solve_box_kernel, rr3_solve_box_wide_kernel,
// rr3_box_safeguard_kernel), a trailing argument of their filtered instantiations: a workgroup whose instance has only[b] == 0
// leaves at once (the step on the law served it, ddmpc_rr3_box_law.hpp).  Without the argument a kernel is what it was.
struct Rr3Only {
  const int* only;
};
// A trailing argument pack of those kernels: does it hold a T, and that T.
template <class T, class... A>
inline constexpr bool rr3_has_arg = (std::is_same_v<T, A> || ...);
template <class T, class A0, class... A>
__device__ __forceinline__ T rr3_get_arg(A0 a0, A... a) {
  if constexpr (std::is_same_v<T, A0>) return a0;
  else return rr3_get_arg<T>(a...);
}
// DDMPC_OPT_LARGE_SETPOINT_BOUNDS: a setpoint per instance on a bounded handle -- one trailing Rr3Setpoint
// (ddmpc_rr3.hpp) of the bounded kernels, alone in the pack.  The factor, W, the k x k system and the bounds do not depend on the
// setpoint; it enters through the four helpers below, which without the argument read the shared tables as the kernels always did:
//   rr3_target     the target of a component that takes it from a setpoint (tabi[1][rho] < 0), and tb of the output stage
//   rr3_box_a      the offset a_s of a boxed component: the instance's setpoint of its channel (ip[2 nbox + s]), 0 for a slack
//   rr3_box_shift  bound - a_s, the one subtraction the host makes for the table's columns (build_large_box): with the handle's
//                  own setpoints every value is the table's, bit for bit
// The third block of ip and the flag behind it are read by the instantiations with the argument only.
template <class... A>
__device__ __forceinline__ double rr3_target(const KParams& P, int RPs, int rho, long long b, const A&... a) {
  if constexpr (rr3_has_arg<Rr3Setpoint, A...>) return rr3_setpoint(P, RPs, rho, b, rr3_get_arg<Rr3Setpoint>(a...));
  else return rr3_setpoint(P, RPs, rho, b);
}
template <class... A>
__device__ __forceinline__ double rr3_box_a(const KParams& P, const Rr3Box& X, int s, long long b, const A&... a) {
  if constexpr (rr3_has_arg<Rr3Setpoint, A...>) {
    const int c = X.ip[2 * X.nbox + s];
    if (c < 0) return 0.0;
    const Rr3Setpoint sp = rr3_get_arg<Rr3Setpoint>(a...);
    return (c < P.m) ? sp.us[b * sp.su + c] : sp.ys[b * sp.sy + (c - P.m)];
  } else {
    return X.bd[(size_t)R3B_A * X.nbox + s];
  }
}
template <class... A>
__device__ __forceinline__ double rr3_box_shift(const KParams& P, const Rr3Box& X, int s, bool up, long long b, const A&... a) {
  if constexpr (rr3_has_arg<Rr3Setpoint, A...>) return X.bd[(size_t)(up ? R3B_HI : R3B_LO) * X.nbox + s] - rr3_box_a(P, X, s, b, a...);
  else return X.bd[(size_t)(up ? R3B_SHHI : R3B_SHLO) * X.nbox + s];
}
// The status of a setpoint the solve launch refuses, or 0 (the same value in every thread: the rule of setpoint_box_refusal,
// ddmpc_setpoint_box_law.hpp): 4 for a non-finite one; DDMPC_STATUS_INFEASIBLE for one outside the bounds of its channel when the
// terminal constraint fixes the last n steps to it.
__device__ __forceinline__ int rr3_setpoint_refusal(const KParams& P, const Rr3Box& X, long long b, const Rr3Setpoint& sp) {
  const double* bnd = X.bd + (size_t)R3B_NV * X.nbox;                       // [u_min | u_max | y_min | y_max]
  int bad = 0, out = 0;
  for (int c = 0; c < P.nch; ++c) {
    const bool u = c < P.m;
    const double v = u ? sp.us[b * sp.su + c] : sp.ys[b * sp.sy + (c - P.m)];
    const double lo = u ? bnd[c] : bnd[2 * P.m + (c - P.m)], hi = u ? bnd[P.m + c] : bnd[2 * P.m + P.p + (c - P.m)];
    bad |= !(fabs(v) < 1e300);
    out |= (v < lo) || (v > hi);
  }
  return bad ? 4 : ((X.ip[3 * X.nbox] != 0 && out) ? 2 : 0);
}
// What the bounded kernels keep in LDS behind Rr3Lds::total (doubles): the table indices of the active components (RR3_KMAX
// ints) and their shifts (RR3_KMAX doubles).  Nothing else is indexed by component in LDS.
constexpr int RR3_BOX_LDS = RR3_KMAX / 2 + RR3_KMAX;
// The active set of a row is kept as sa + 4 say (sa: its slack or input component, say: its output component), the encoding of
// the register-resident route (ddmpc_box_law.hpp); the kept record and ddmpc_reconstruct_kernel read the same code.
__device__ __forceinline__ int rr3_sa(int code) { return ((code + 5) & 3) - 1; }
__device__ __forceinline__ int rr3_say(int code) { return ((code + 5) >> 2) - 1; }

// D(state) and t(state) of a row (the four-state table of DESIGN.md 5.5.1): an active input makes its row hard at the bound, an
// active output leaves 1 / lamb_sigma (or nothing, with the slack held too) and moves the target to its bound.
__device__ __forceinline__ void rr3_box_row(const KParams& P, int RPs, const Rr3Box& X, int rho, int code, double t0, double* D, double* t) {
  const int sa = rr3_sa(code), say = rr3_say(code), ch = rho % P.nch;
  const double* bnd = X.bd + (size_t)R3B_NV * X.nbox;
  *D = sa ? P.tabd[1 * RPs + rho] : P.tabd[0 * RPs + rho];
  *t = t0 + sa * P.bound;
  if (sa != 0 && P.tabi[0 * RPs + rho] == K_UFREE) { *D = 0.0; *t = bnd[(sa > 0 ? P.m : 0) + ch]; }
  if (say != 0) { *D = sa ? 0.0 : 1.0 / P.lamb_sigma; *t = bnd[2 * P.m + (say > 0 ? P.p : 0) + ch - P.m] + sa * P.bound; }
}

// Output stage, the twin of rr3_outputs for scalar / diagonal weights: z = t(state) - lam D(state) beta per row, so an active
// input is its bound exactly and an active output gives ybar = bound, sigma = z - bound (= -lam beta / lamb_sigma, or
// +- c eps_max with the slack held too); the cost terms are r (u - u_s)^2 and q (ybar - y_s)^2 + lamb_sigma sigma^2 in every
// state.  An instance that failed (st != 0) reports NaN inputs and cost: no fall-back kernel knows the bounds.
// A...: the trailing pack of the calling kernel (with an Rr3Setpoint: tb is the instance's, and a refused setpoint outside its
// bounds -- st 2 -- reports 0 iterations).
template <class... A>
__device__ __forceinline__ void rr3_box_outputs(const KParams& P, int RPs, const Rr3Box& X, long long b, const int* perm, const double* tv,
                                                const double* bv, const int* act, int st, int iter, double* red, double* __restrict__ u_opt,
                                                double* __restrict__ cost, int* __restrict__ status, int* __restrict__ iters,
                                                double* __restrict__ beta_ws, signed char* __restrict__ act_ws, const A&... a) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // (opaque per call, see rr3_trsv_fwd)
  const int nthr = blockDim.x, r = P.r;
  const int n = P.npu / P.m;
  const double nanv = __longlong_as_double(0x7ff8000000000000LL);
  double part = 0.0, bad = 0.0;
  double* uo = u_opt + b * (long long)((P.Ln - n) * P.m);
  for (int i = tid; i < r; i += nthr) {
    const int rho = perm[i];
    const int oidx = P.tabi[2 * RPs + rho];
    if (st != 0) { if (oidx >= 0) uo[oidx] = nanv; continue; }              // (st: uniform)
    const int code = act[i], s_act = rr3_sa(code), y_act = rr3_say(code);
    const double bb = bv[i];
    double D, t;
    rr3_box_row(P, RPs, X, rho, code, tv[i], &D, &t);
    const double z = t - P.lam * D * bb;
    const double wq = P.tabd[3 * RPs + rho];
    const double tb = rr3_target(P, RPs, rho, b, a...);
    const int kind = P.tabi[0 * RPs + rho];
    if (!(fabs(bb) < 1e300)) bad = 1.0;
    double contrib = P.lam * bb * z;
    if (kind == K_UFREE || kind == K_YFREE) { const double dlt = z - tb; contrib += wq * dlt * dlt; }
    else if (kind == K_WINT) { const double sg = z - tv[i]; contrib += P.lamb_sigma * sg * sg; }
    else if (kind == K_WTERM) { const double sg = z - tb; contrib += P.lamb_sigma * sg * sg; }
    else if (kind == K_WPRED) {
      const double sg = (s_act != 0) ? s_act * P.bound : -P.lam * bb / P.lamb_sigma;
      const double dlt = (y_act != 0) ? t - s_act * P.bound - tb : z - sg - tb;       // (an active output: ybar = its bound exactly)
      contrib += wq * dlt * dlt + P.lamb_sigma * sg * sg;
    }
    part += contrib;
    if (oidx >= 0) uo[oidx] = z;                      // ubar[n*m:], controller.py:799-805
    if (beta_ws) beta_ws[b * (long long)P.rE + rho] = bb;
    if (act_ws) act_ws[b * (long long)P.rE + rho] = (signed char)code;
  }
  const double tot = block_sum(part, red);
  const double nbad = block_sum(bad, red);
  if (tid == 0) {
    if (st == 0 && (nbad != 0.0 || !(fabs(tot) < 1e300))) st = 4;
    cost[b] = (st == 0) ? tot : nanv;
    status[b] = st;
    if (iters) iters[b] = iter > 0 ? iter : 1;
    if constexpr (rr3_has_arg<Rr3Setpoint, A...>) { if (iters && st == 2) iters[b] = 0; }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The solve on the kept factor with the table-driven box (the twin of rr3_solve_kernel; same launch geometry, LDS of
// Rr3Lds::total + RR3_BOX_LDS doubles).  The iteration is the rule of DESIGN.md 5.5: from the empty set every boxed component
// is looked at in every iteration; act holds sa + 4 say per row; list[] the positions, lcomp[] / lsh[] the table indices and
// shifts of the active components, ascending (two components of one row give two equal columns of W); the k x k system is
// diag(1 / d_s) - W'W with each component's own d_s, its right-hand side takes the component's own shift.  More than RR3_KMAX
// active components in an iteration, or a non-positive pivot of the k x k system: status 4 at that iteration.
// Only...: empty (the kernel as it is launched without a filter), one Rr3Only, or one Rr3Setpoint (both launches; the solve
// launch refuses a setpoint by rr3_setpoint_refusal before anything is iterated, and its record keeps the others off the instance).
// ---------------------------------------------------------------------------------------------------------------
template <bool REFINE_PASS, class... Only>
__global__ __launch_bounds__(RR2_TS, 4) void rr3_solve_box_kernel(Rr3 S, KParams P, int RPs, const double* __restrict__ u_past,
                                                               const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                               double* __restrict__ cost, int* __restrict__ status, int* __restrict__ iters,
                                                               double* __restrict__ beta_ws, signed char* __restrict__ act_ws, int defer_outputs,
                                                               Rr3Box X, Only... only) {
  static_assert(sizeof...(Only) == 0 || (sizeof...(Only) == 1 && (rr3_has_arg<Rr3Only, Only...> || rr3_has_arg<Rr3Setpoint, Only...>)),
                "one filter or one setpoint at most");
  extern __shared__ __attribute__((aligned(16))) double r3_lds[];
  const long long b = blockIdx.x;
  if constexpr (rr3_has_arg<Rr3Only, Only...>) {
    if (rr3_get_arg<Rr3Only>(only...).only[b] == 0) return;                 // (workgroup-uniform)
  }
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int r = S.r, nA = S.nA, n0 = S.n0, m = P.m, p = P.p;
  const int n = P.npu / m;
  const Rr3Lds LD = Rr3Lds::make(r);
  double* tv = r3_lds + LD.tv; double* yv = r3_lds + LD.yv; double* y2 = r3_lds + LD.y2; double* bv = r3_lds + LD.bv;
  int* act = reinterpret_cast<int*>(r3_lds + LD.act);
  double* big = r3_lds + LD.big;                             // tile exchange of rr3_w_forward | k x k system | reduction buffer of the backward substitution
  double* red = big; double* Sm = big;
  double* tmp = r3_lds + LD.tmp; double* hpart = tmp + 64;
  double* hv = r3_lds + LD.hv; double* ev = hv + RR3_KMAX;
  int* list = reinterpret_cast<int*>(r3_lds + LD.list);
  int* flagw = list + RR3_KMAX;                              // [0] changed  [1] k  [2] small-system failure  [3] the largest k so far
  int* lcomp = reinterpret_cast<int*>(r3_lds + LD.total);    // table index of the active component in column j ...
  double* lsh = r3_lds + LD.total + RR3_KMAX / 2;            // ... and its shift of t
  constexpr int LDS_ = RR3_KMAX + 1;
  const int* perm = S.perm;
  const double* G = S.ws + b * S.stride;
  const double* m64 = S.m64 + b * S.m64_stride;
  const unsigned long long live = S.dd[4 * b + 2];
  const int nb = (r + 63) >> 6, b0 = n0 >> 6, nT = r - n0;
  double* Vb = S.V + b * S.vstride;                          // [R3_X | R3_BETA | R3_T0]
  double* Wg = S.Wg + b * S.wstride;                         // W, row-major [row - n0][RR3_KMAX]
  double* Lg = Wg + (size_t)S.ldw * RR3_KMAX;                // factor of the k x k system of the final active set
  int* kq = S.kq + b * S.kstride;
  const double* up = u_past + b * (long long)P.npu;
  const double* yp = y_past + b * (long long)(n * p);
  int st = 0, iter = 0, k = 0;
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();   // diagnostics (kq[.. + rv ..]): when this workgroup ran
  // h = W'v on the trailing block (v: LDS, absolute rows), into hv[0 .. k): column x by thread x of each of the 8 row parts
  auto w_times = [&](const double* v) {
    const int x = tid & 63, part = tid >> 6;
    const int per = (nT + 7) >> 3;
    double h = 0.0;
    if (x < k) {
      const int i1 = (part + 1) * per < nT ? (part + 1) * per : nT;
      for (int i = part * per; i < i1; ++i) h = fma(Wg[(size_t)i * RR3_KMAX + x], v[n0 + i], h);
    }
    hpart[part * 64 + x] = h;
    __syncthreads();
    if (tid < k) {
      double t = 0.0;
#pragma unroll
      for (int g = 0; g < 8; ++g) t += hpart[g * 64 + tid];
      hv[tid] = t;
    }
    __syncthreads();
  };
  // v_T += W e on the trailing block (one thread per row; the row of W is contiguous)
  auto w_apply = [&](const double* src, double* dst, const double* e) {
    for (int i = n0 + tid; i < r; i += nthr) {
      double v = src[i];
      const double* wr = Wg + (size_t)(i - n0) * RR3_KMAX;
      for (int x = 0; x < k; ++x) v = fma(wr[x], e[x], v);
      dst[i] = v;
    }
    __syncthreads();
  };

  if constexpr (!REFINE_PASS) {
    double nbad = 0.0;
    for (int i = tid; i < LD.VL; i += nthr) {
      double t = 0.0;
      if (i < r) {
        const int rho = perm[i];
        const int pidx = P.tabi[1 * RPs + rho];
        t = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : rr3_target(P, RPs, rho, b, only...);
        nbad += S.skip[b * S.s_stride + i] ? 1.0 : 0.0;
      }
      tv[i] = t; act[i] = 0; y2[i] = 0.0; bv[i] = 0.0;
    }
    if (tid == 0) flagw[3] = 0;
    if (block_sum(nbad, tmp) != 0.0) st = 4;                 // (uniform) a pivot of K0 failed: not positive definite numerically
    if constexpr (rr3_has_arg<Rr3Setpoint, Only...>) {       // (uniform) a refused setpoint: nothing is iterated
      const int refuse = rr3_setpoint_refusal(P, X, b, rr3_get_arg<Rr3Setpoint>(only...));
      if (refuse != 0) st = refuse;
    }
    __syncthreads();
    if (st == 0) {
      rr3_trsv_fwd<1>(G, m64, r, live, 0, [&](int, int i) { return tv[i]; }, [&](int) { return yv; }, tmp);
      if (X.nbox == 0 || nA >= r) {
        rr3_trsv_bwd(G, m64, r, live, nb, 0, yv, bv, red, tmp);
        iter = 1;
      } else {
        for (int i = tid; i < LD.VL; i += nthr) y2[i] = yv[i];
        __syncthreads();
        rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);         // beta on the trailing block: the empty active set
        for (;;) {
          ++iter;
          if (tid == 0) flagw[0] = 0;
          __syncthreads();
          int ot = threadIdx.x;
          asm volatile("" : "+v"(ot));     // (opaque per iteration: the table addresses are formed here, not kept alive across the kernel)
          // every boxed component against its own lo / hi: an inactive one goes to the bound it violates, an active one is
          // released when its multiplier changes sign, never moved to the other bound in one step.  Two components of one row
          // share act[i]: each adds its own change to the code (the bits of the other one do not enter its decoding).
          for (int s = ot; s < X.nbox; s += nthr) {
            const int i = X.ip[s], isy = X.ip[X.nbox + s];
            const int code = __hip_atomic_load(&act[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int cur = isy ? rr3_say(code) : rr3_sa(code);
            const double hat = fma(X.bd[(size_t)R3B_C * X.nbox + s], bv[i], rr3_box_a(P, X, s, b, only...));
            const int upv = hat > X.bd[(size_t)R3B_HI * X.nbox + s], dnv = hat < X.bd[(size_t)R3B_LO * X.nbox + s];
            const int ns = cur > 0 ? upv : (cur < 0 ? -dnv : upv - dnv);
            if (ns != cur) { atomicAdd(&act[i], (ns - cur) * (isy ? 4 : 1)); flagw[0] = 1; }
          }
          __syncthreads();
          if (flagw[0] == 0) break;
          if (iter >= P.max_iter) { st = 4; break; }
          // the active components, ascending (deterministic column order)
          if (ot < 64) {
            int base = 0;
            for (int s0 = 0; s0 < X.nbox; s0 += 64) {
              const int s = s0 + (ot & 63);
              int a = 0, i = 0;
              if (s < X.nbox) { i = X.ip[s]; a = X.ip[X.nbox + s] ? rr3_say(act[i]) : rr3_sa(act[i]); }
              const unsigned long long mk = __ballot(a != 0);
              const int slot = base + __popcll(mk & ((1ull << (ot & 63)) - 1ull));
              if (a != 0 && slot < RR3_KMAX) {
                list[slot] = i; lcomp[slot] = s;
                lsh[slot] = rr3_box_shift(P, X, s, a > 0, b, only...);
              }
              base += __popcll(mk);
            }
            if ((ot & 63) == 0) { flagw[1] = base; if (base > flagw[3]) flagw[3] = base; }
          }
          __syncthreads();
          k = flagw[1];
          if (k > RR3_KMAX) { st = 4; k = 0; break; }                     // more columns than W holds
          rr3_w_forward(G, m64, r, live, b0, n0, list, k, Wg, big);       // W = L_TT^-1 E_T
          rr3_w_gram(Wg, nT, k, Sm);                                      // Sm = -W'W (big: the tile exchange is done with)
          w_times(yv);                                                    // hv = W'y
          if (tid < k) {                                                  // (d_s > 0 for every component of the table: the host refuses the others)
            double h = hv[tid];
            for (int yy = 0; yy < k; ++yy) {                              // + (W'W) shift
              const double g = -(yy <= tid ? Sm[tid * LDS_ + yy] : Sm[yy * LDS_ + tid]);
              h = fma(g, lsh[yy], h);
            }
            hv[tid] = h;
          }
          __syncthreads();
          if (tid < k) Sm[tid * LDS_ + tid] += X.bd[(size_t)R3B_INVD * X.nbox + lcomp[tid]];   // the component's own 1 / d_s
          __syncthreads();
          rr3_small_cholesky(Sm, k, flagw + 2);
          __syncthreads();
          if (flagw[2] != 0) { st = 4; k = 0; break; }
          rr3_small_solve(Sm, k, hv, ev);
          if (defer_outputs) {                                            // (the reduction buffer of the backward substitution takes Sm's place)
            int oe = threadIdx.x;
            asm volatile("" : "+v"(oe));
            for (int e = oe; e < k * LDS_; e += nthr) Lg[e] = Sm[e];
          }
          __syncthreads();
          if (tid < k) ev[tid] += lsh[tid];                               // y' = y + W (shift + cv) on the trailing block
          __syncthreads();
          w_apply(yv, y2, ev);
          rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);
        }
        if (st == 0) rr3_trsv_bwd(G, m64, r, live, b0, 0, y2, bv, red, tmp);   // the rows in front of the trailing block
      }
    }
    if (defer_outputs && st == 0) {
      // what the refinement launch needs: beta (both orders), t0, the active set (codes), the switched positions (W and the
      // k x k factor are in global memory already)
      double* vx = Vb + (size_t)R3_X * S.VL;
      double* vbeta = Vb + (size_t)R3_BETA * S.VL;
      double* vt0 = Vb + (size_t)R3_T0 * S.VL;
      for (int i = tid; i < r; i += nthr) { vx[perm[i]] = bv[i]; vbeta[i] = bv[i]; vt0[i] = tv[i]; kq[4 + RR3_KMAX + i] = act[i]; }
      if (tid < k) kq[4 + tid] = list[tid];
    }
    if (tid == 0) {
      kq[0] = (st == 0) ? k : 0; kq[1] = st; kq[2] = iter; kq[3] = k;
      const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
      kq[4 + RR3_KMAX + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + RR3_KMAX + S.rv + 1] = (int)(t_end - t_begin);   // (100 MHz ticks)
      kq[4 + RR3_KMAX + S.rv + 2] = flagw[3];                             // the most components active in any iteration
    }
    if (!defer_outputs || st != 0) {
      __syncthreads();
      rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, st, iter, tmp, u_opt, cost, status, iters, beta_ws, act_ws, only...);
    }
  } else {
    // ---- one pass of iterative refinement on the system of the final active set, then the outputs.
    //      rho = t(act) - (H (H' beta) + lam D(act) beta), exact Hankel products (rr2_hankel_mfma_kernel left the partial sums in ZP);
    //      delta = L^-T ( y_rho + W Sm^-1 W' y_rho );  beta += delta
    k = kq[0]; st = kq[1]; iter = kq[2];
    if (st != 0) return;                                                  // (uniform) the solve launch wrote the outputs itself
    const double* vbeta = Vb + (size_t)R3_BETA * S.VL;
    const double* vt0 = Vb + (size_t)R3_T0 * S.VL;
    const double* zp = S.ZP + b * RR2_NG * (long long)S.VL;
    for (int i = tid; i < LD.VL; i += nthr) {
      double bb = 0.0, t0 = 0.0, rho_v = 0.0;
      int a = 0;
      if (i < r) {
        const int rho = perm[i];
        bb = vbeta[i]; t0 = vt0[i]; a = kq[4 + RR3_KMAX + i];
        double hz = 0.0;
#pragma unroll
        for (int g = 0; g < RR2_NG; ++g) hz += zp[g * (long long)S.VL + rho];
        double D, t;
        rr3_box_row(P, RPs, X, rho, a, t0, &D, &t);
        rho_v = t - hz - P.lam * D * bb;
      }
      tv[i] = t0; bv[i] = bb; act[i] = a; y2[i] = rho_v;
    }
    __syncthreads();
    rr3_trsv_fwd<1>(G, m64, r, live, 0, [&](int, int i) { return y2[i]; }, [&](int) { return yv; }, tmp);     // y_rho
    if (k > 0) {
      for (int e = tid; e < k * LDS_; e += nthr) Sm[e] = Lg[e];
      w_times(yv);
      rr3_small_solve(Sm, k, hv, ev);
      __syncthreads();
      w_apply(yv, yv, ev);
    }
    rr3_trsv_bwd(G, m64, r, live, nb, 0, yv, y2, red, tmp);                                                   // delta
    for (int i = tid; i < r; i += nthr) bv[i] += y2[i];
    __syncthreads();
    rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, 0, iter, tmp, u_opt, cost, status, iters, beta_ws, act_ws, only...);
  }
}

}  // namespace ddmpc
