// ddmpc_rr3_box_safe.hpp -- DDMPC_OPT_LARGE_BOX_SAFEGUARD: the primal active-set method of DESIGN.md 5.5 (steps 1 - 4) for the
// bounded phase kernels (272 .. 1024 rows).  rr3_box_safeguard_kernel runs between the solve launch and the
// refinement launch of rr3_solve_box_wide_kernel (ddmpc_rr3_box_wide.hpp) and shares its launch geometry, its LDS carve-up, its
// workspace and its building blocks.  A workgroup whose record does not say "the iteration ended at max_iter" leaves at once;
// the others solve their instance again from the empty set's solution:
//   1  v = clip(hat(empty), lo, hi); the working set = the components hat violates, each on the side it violates
//   2  solve for the working set (the Woodbury update of the wide kernel); an inactive component whose hat leaves its box
//      blocks at alpha = (bound - v) / (hat - v)
//   3  one blocks: v += alpha (hat - v) with the smallest alpha (lowest component on ties), that component joins at its bound
//   4  none blocks: v = hat; the active component with the largest g = act (bound - hat) / |c| (lowest component on ties) is
//      released if g > 0, otherwise the working set is optimal
// A solve changes the working set by ONE component and the columns of W = L_TT^-1 E are independent, so W is kept: the set of
// step 1 goes through rr3w_w_forward 64 columns per pass, a joining component is one column substitution on L_TT (into a
// 16-column strip, then copied behind the last column) plus one row of the Gram tiles, a leaving one is overwritten by the last
// column.  Behind the wide kernel's W and tiles of S an instance keeps
//   Gg   the tiles of -W'W UNFACTORED (the layout of S); every solve copies them to S, adds 1 / d_s and runs the blocked Cholesky
//   v    nbox doubles (rounded up to 16)
//   Wn   the strip of the entering column, [ldw][16]
// The column order of W is the order of arrival -- a fixed function of the instance: every sum and both selections have a fixed
// order.  A finished instance leaves what a converged instance of the wide kernel leaves (record with state 0, positions, codes,
// R3_X / R3_BETA / R3_T0, W, the tile factor of S), so the refinement launch finishes it unchanged; iters = max_iter + solves.
// Status 4 (NaN outputs) at more than 4 nbox + 16 solves, a non-positive pivot of S, or a working set beyond the capacity:
// iters = max_iter + the number of the solve that could not be made.
#pragma once
#include "ddmpc_rr3_box_wide.hpp"

namespace ddmpc {

// doubles per instance behind the wide kernel's workspace (W and the tiles of S)
__host__ __device__ constexpr long long rr3s_extra(int cap, int nbox, int ldw) {
  return rr3w_tiles(cap) * 4096 + ((nbox + 15) & ~15) + 16ll * ldw;
}

// Only...: empty (the kernel as it is launched without a filter), one Rr3Only (DDMPC_OPT_LARGE_BOX_LAW), or one Rr3Setpoint
// (DDMPC_OPT_LARGE_SETPOINT_BOUNDS: the staging, the offsets and the shifts of the instance's setpoint, as in the solve launch).
template <class... Only>
__global__ __launch_bounds__(RR2_TS, 4) void rr3_box_safeguard_kernel(Rr3 S, KParams P, int RPs, const double* __restrict__ u_past,
                                                                   const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                                   double* __restrict__ cost, int* __restrict__ status,
                                                                   int* __restrict__ iters, double* __restrict__ beta_ws,
                                                                   signed char* __restrict__ act_ws, int defer_outputs, Rr3Box X, int cap,
                                                                   Only... only) {
  static_assert(sizeof...(Only) == 0 || (sizeof...(Only) == 1 && (rr3_has_arg<Rr3Only, Only...> || rr3_has_arg<Rr3Setpoint, Only...>)),
                "one filter or one setpoint at most");
  extern __shared__ __attribute__((aligned(16))) double r3_lds[];
  const long long b = blockIdx.x;
  if constexpr (rr3_has_arg<Rr3Only, Only...>) {
    if (rr3_get_arg<Rr3Only>(only...).only[b] == 0) return;                 // (workgroup-uniform)
  }
  int* kq = S.kq + b * S.kstride;
  // (uniform) only an instance whose iteration reached max_iter without a stable set: a capacity or pivot failure ends below
  // max_iter (the cap test precedes the list build in the bounded kernels), a failed pivot of K0 has 0 iterations
  if (__builtin_amdgcn_readfirstlane(kq[1]) != 4 || __builtin_amdgcn_readfirstlane(kq[2]) < P.max_iter) return;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int r = S.r, n0 = S.n0, m = P.m, p = P.p;
  const int n = P.npu / m;
  const int nbox = X.nbox;
  const Rr3Lds LD = Rr3Lds::make(r);
  double* tv = r3_lds + LD.tv; double* yv = r3_lds + LD.yv; double* y2 = r3_lds + LD.y2; double* bv = r3_lds + LD.bv;
  int* act = reinterpret_cast<int*>(r3_lds + LD.act);
  double* big = r3_lds + LD.big;                             // tile exchange of rr3w_w_forward | a diagonal tile of S | reduction buffer | the entering column
  double* red = big; double* Sm = big; double* colv = big;
  double* tmp = r3_lds + LD.tmp; double* hpart = tmp + 64;
  int* isel = reinterpret_cast<int*>(hpart);                 // selection scratch (hpart is free between the products with W)
  int* flagw = reinterpret_cast<int*>(r3_lds + LD.list);     // [1] k of step 1  [2] small-system failure  [4] the slot of the leaving column
  double* hv = r3_lds + LD.total; double* ev = hv + cap;
  double* lsh = ev + cap;
  int* list = reinterpret_cast<int*>(lsh + cap);
  int* lcomp = list + cap;
  const int* perm = S.perm;
  const double* G = S.ws + b * S.stride;
  const double* m64 = S.m64 + b * S.m64_stride;
  const unsigned long long live = S.dd[4 * b + 2];
  const int nb = (r + 63) >> 6, b0 = n0 >> 6, nT = r - n0;
  double* Vb = S.V + b * S.vstride;
  double* Wg = S.Wg + b * S.wstride;                         // W, row-major [row - n0][cap]
  double* Sg = Wg + (size_t)S.ldw * cap;                     // the tiles of S, factored in place
  double* Gg = Sg + rr3w_tiles(cap) * 4096;                  // the tiles of -W'W, kept unfactored
  double* vg = Gg + rr3w_tiles(cap) * 4096;                  // v
  double* Wn = vg + ((nbox + 15) & ~15);                     // the entering column
  const double* up = u_past + b * (long long)P.npu;
  const double* yp = y_past + b * (long long)(n * p);
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  constexpr int NONE = 0x7fffffff;
  int st = 0, k = 0, nsolve = 0, peak = 0;
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();
  // h = W'v on the trailing block (v: LDS, absolute rows), into hv[0 .. k)  (as in rr3_solve_box_wide_kernel)
  auto w_times = [&](const double* v) {
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));     // (opaque per call: nothing derived from it stays alive across the kernel's phases)
    const int xl = ot & 63, part = ot >> 6;
    const int per = (nT + 7) >> 3;
    const int i1 = (part + 1) * per < nT ? (part + 1) * per : nT;
    for (int cb = 0; 64 * cb < k; ++cb) {
      const int x = 64 * cb + xl;
      double h = 0.0;
      if (x < k)
        for (int i = part * per; i < i1; ++i) h = fma(Wg[(size_t)i * cap + x], v[n0 + i], h);
      hpart[part * 64 + xl] = h;
      __syncthreads();
      if (ot < 64 && x < k) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += hpart[g * 64 + ot];
        hv[x] = t;
      }
      __syncthreads();
    }
  };
  auto w_apply = [&](const double* src, double* dst, const double* e) {
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));
    for (int i = n0 + ot; i < r; i += nthr) {
      double v = src[i];
      const double* wr = Wg + (size_t)(i - n0) * cap;
      for (int x = 0; x < k; ++x) v = fma(wr[x], e[x], v);
      dst[i] = v;
    }
    __syncthreads();
  };
  auto stage_tile = [&](int J) {
    const double* T = rr3w_tile(Sg, J, J);
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));
    for (int e = ot; e < 4096; e += nthr) Sm[(e >> 6) * 65 + (e & 63)] = T[e];
  };
  auto s_solve = [&]() {
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));
    const int x = ot & 63, part = ot >> 6;
    const int nblk = (k + 63) >> 6;
    for (int J = 0; J < nblk; ++J) {
      const int kb = (k - 64 * J < 64) ? k - 64 * J : 64;
      stage_tile(J);
      double h = 0.0;
      for (int K = 0; K < J; ++K) {
        const double* T = rr3w_tile(Sg, J, K) + (size_t)x * 64 + 8 * part;
        const d4 a0 = *reinterpret_cast<const d4*>(T), a1 = *reinterpret_cast<const d4*>(T + 4);
        const double* w = hv + 64 * K + 8 * part;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h = fma(a0[e], w[e], h); h = fma(a1[e], w[4 + e], h); }
      }
      hpart[part * 64 + x] = h;
      __syncthreads();
      if (ot < 64) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += hpart[g * 64 + ot];
        h = (ot < kb) ? hv[64 * J + ot] - t : 0.0;
        h = rr3w_tile_fwd(Sm, kb, ot, h);
        if (ot < kb) hv[64 * J + ot] = h;
      }
      __syncthreads();
    }
    for (int J = nblk - 1; J >= 0; --J) {
      const int kb = (k - 64 * J < 64) ? k - 64 * J : 64;
      stage_tile(J);
      double h = 0.0;
      for (int I = J + 1; I < nblk; ++I) {
        const int kbI = (k - 64 * I < 64) ? k - 64 * I : 64;
        const double* T = rr3w_tile(Sg, I, J) + x;
        for (int rr = 8 * part; rr < 8 * part + 8; ++rr)
          if (rr < kbI) h = fma(T[(size_t)rr * 64], ev[64 * I + rr], h);
      }
      hpart[part * 64 + x] = h;
      __syncthreads();
      if (ot < 64) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += hpart[g * 64 + ot];
        h = (ot < kb) ? hv[64 * J + ot] - t : 0.0;
        h = rr3w_tile_bwd(Sm, kb, ot, h);
        if (ot < kb) ev[64 * J + ot] = h;
      }
      __syncthreads();
    }
  };
  // the smallest key over the workgroup, the lowest index among equal keys; every thread gets both (fixed order: the lanes of a
  // wave by butterfly, the waves ascending)
  auto arg_min = [&](double key, int idx, double* kout) -> int {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ok = __shfl_xor(key, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ok < key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { tmp[threadIdx.x >> 6] = key; isel[threadIdx.x >> 6] = idx; }
    __syncthreads();
    double bk = tmp[0];
    int bi = isel[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
      const double ok = tmp[w];
      const int oi = isel[w];
      if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
    }
    *kout = bk;
    return bi;
  };

  // ---- the empty set's solution on the trailing block (as the solve launch formed it)
  for (int i = tid; i < LD.VL; i += nthr) {
    double t = 0.0;
    if (i < r) {
      const int rho = perm[i];
      const int pidx = P.tabi[1 * RPs + rho];
      // TWO COPIES OF ONE STATEMENT, to be edited together: they differ in the last operand only.  The instantiations without a
      // setpoint keep the statement they had (through rr3_target their staging loop was compiled into other code, compared in
      // the assembly); the solve kernels stage the same t through rr3_target alone.
      if constexpr (rr3_has_arg<Rr3Setpoint, Only...>) t = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : rr3_target(P, RPs, rho, b, only...);
      else t = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : P.tabd[2 * RPs + rho];
    }
    tv[i] = t; act[i] = 0; y2[i] = 0.0; bv[i] = 0.0;
  }
  __syncthreads();
  rr3_trsv_fwd<1>(G, m64, r, live, 0, [&](int, int i) { return tv[i]; }, [&](int) { return yv; }, tmp);
  for (int i = tid; i < LD.VL; i += nthr) y2[i] = yv[i];
  __syncthreads();
  rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);
  // ---- step 1
  {
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));
    for (int s = ot; s < nbox; s += nthr) {
      const int i = X.ip[s], isy = X.ip[nbox + s];
      const double hat = fma(X.bd[(size_t)R3B_C * nbox + s], bv[i], rr3_box_a(P, X, s, b, only...));
      const double lo = X.bd[(size_t)R3B_LO * nbox + s], hi = X.bd[(size_t)R3B_HI * nbox + s];
      const int side = (hat > hi) - (hat < lo);
      vg[s] = side > 0 ? hi : (side < 0 ? lo : hat);
      if (side != 0) atomicAdd(&act[i], side * (isy ? 4 : 1));
    }
    __syncthreads();
    if (ot < 64) {                                           // the violated components, ascending
      int base = 0;
      for (int s0 = 0; s0 < nbox; s0 += 64) {
        const int s = s0 + (ot & 63);
        int a = 0, i = 0;
        if (s < nbox) { i = X.ip[s]; a = X.ip[nbox + s] ? rr3_say(act[i]) : rr3_sa(act[i]); }
        const unsigned long long mk = __ballot(a != 0);
        const int slot = base + __popcll(mk & ((1ull << (ot & 63)) - 1ull));
        if (a != 0 && slot < cap) {
          list[slot] = i; lcomp[slot] = s;
          lsh[slot] = rr3_box_shift(P, X, s, a > 0, b, only...);
        }
        base += __popcll(mk);
      }
      if ((ot & 63) == 0) flagw[1] = base;
    }
    __syncthreads();
    k = __builtin_amdgcn_readfirstlane(flagw[1]);
    if (k <= cap) {
      for (int cb = 0; 64 * cb < k; ++cb)
        rr3w_w_forward(G, m64, r, live, b0, n0, list + 64 * cb, (k - 64 * cb < 64) ? k - 64 * cb : 64, Wg + 64 * cb, cap, big);
      rr3w_gram(Wg, cap, nT, k, Gg);
      __syncthreads();
    }
  }
  // ---- steps 2 - 4
  const int lim = 4 * nbox + 16;
  for (;;) {
    ++nsolve;
    if (k > cap || nsolve > lim) { st = 4; break; }           // more columns than W holds | the method's own cap
    if (k > peak) peak = k;
    const int nblk = (k + 63) >> 6;
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));     // (opaque per solve: the table addresses are formed here)
    {                                                         // S = -W'W (the first nblk (nblk + 1) / 2 tiles are those of the blocks in use)
      const d4* src = reinterpret_cast<const d4*>(Gg);
      d4* dst = reinterpret_cast<d4*>(Sg);
      const int ne = nblk * (nblk + 1) / 2 * 1024;
      for (int e = ot; e < ne; e += nthr) dst[e] = src[e];
    }
    __syncthreads();
    w_apply(yv, y2, lsh);                                     // y + W shift
    w_times(y2);                                              // hv = W'(y + W shift)
    if (ot < k) rr3w_tile(Sg, ot >> 6, ot >> 6)[(ot & 63) * 65] += X.bd[(size_t)R3B_INVD * nbox + lcomp[ot]];
    __syncthreads();
    int bad = 0;
    for (int J = 0; J < nblk && !bad; ++J) {                  // blocked Cholesky of S, in place (as in rr3_solve_box_wide_kernel)
      const int kb = (k - 64 * J < 64) ? k - 64 * J : 64;
      if (J > 0) { rr3w_chol_update(Sg, J, nblk); __syncthreads(); }
      stage_tile(J);
      __syncthreads();
      rr3_small_cholesky(Sm, kb, flagw + 2);
      __syncthreads();
      if (flagw[2] != 0) { bad = 1; break; }
      double* TJ = rr3w_tile(Sg, J, J);
      int oj = threadIdx.x;
      asm volatile("" : "+v"(oj));
      for (int e = oj; e < 4096; e += nthr)
        if ((e >> 6) < kb && (e & 63) <= (e >> 6)) TJ[e] = Sm[(e >> 6) * 65 + (e & 63)];
      if (oj < k - 64 * (J + 1)) rr3w_chol_rows(rr3w_tile(Sg, J + 1 + (oj >> 6), J) + (size_t)(oj & 63) * 64, Sm);
      __syncthreads();
    }
    if (bad) { st = 4; break; }
    s_solve();
    if (ot < k) ev[ot] += lsh[ot];
    __syncthreads();
    w_apply(yv, y2, ev);
    rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);  // beta(W) on the trailing block
    // step 2: the first inactive component to leave its box on the way from v to hat
    double key = inf;
    int ks = NONE;
    for (int s = ot; s < nbox; s += nthr) {
      const int i = X.ip[s], isy = X.ip[nbox + s];
      const int cur = isy ? rr3_say(act[i]) : rr3_sa(act[i]);
      if (cur != 0) continue;
      const double hat = fma(X.bd[(size_t)R3B_C * nbox + s], bv[i], rr3_box_a(P, X, s, b, only...));
      const double lo = X.bd[(size_t)R3B_LO * nbox + s], hi = X.bd[(size_t)R3B_HI * nbox + s];
      if (hat > hi || hat < lo) {
        const double v = vg[s];
        const double al = fmax(((hat > hi ? hi : lo) - v) / (hat - v), 0.0);
        if (al < key) { key = al; ks = s; }
      }
    }
    double alpha;
    const int sb = arg_min(key, ks, &alpha);
    if (sb != NONE) {
      // step 3: move to the blocking point; component sb joins at its bound, as column k of W
      const int ib = X.ip[sb], yb = X.ip[nbox + sb];
      const double hb = fma(X.bd[(size_t)R3B_C * nbox + sb], bv[ib], rr3_box_a(P, X, sb, b, only...));
      const int sd = hb > X.bd[(size_t)R3B_HI * nbox + sb] ? 1 : -1;
      if (k >= cap) { k = cap + 1; continue; }                // (uniform) the next solve cannot be made
      for (int s = ot; s < nbox; s += nthr) {
        const int i = X.ip[s], isy = X.ip[nbox + s];
        const int cur = isy ? rr3_say(act[i]) : rr3_sa(act[i]);
        if (cur != 0) continue;
        const double hat = fma(X.bd[(size_t)R3B_C * nbox + s], bv[i], rr3_box_a(P, X, s, b, only...));
        const double v = vg[s];
        vg[s] = (s == sb) ? X.bd[(size_t)(sd > 0 ? R3B_HI : R3B_LO) * nbox + s] : v + alpha * (hat - v);
      }
      __syncthreads();
      if (ot == 0) {
        act[ib] += sd * (yb ? 4 : 1);
        list[k] = ib; lcomp[k] = sb;
        lsh[k] = rr3_box_shift(P, X, sb, sd > 0, b, only...);
      }
      __syncthreads();
      rr3w_w_forward(G, m64, r, live, b0, n0, list + k, 1, Wn, 16, big);    // one column substitution on L_TT
      for (int i = ot; i < S.ldw; i += nthr) {
        const double w = Wn[(size_t)i * 16];
        Wg[(size_t)i * cap + k] = w;
        colv[n0 + i] = w;
      }
      __syncthreads();
      ++k;
      w_times(colv);                                          // its row of the Gram tiles: -W'w
      if (ot < k) rr3w_tile(Gg, (k - 1) >> 6, ot >> 6)[((k - 1) & 63) * 64 + (ot & 63)] = -hv[ot];
      __syncthreads();
      continue;
    }
    // step 4: v = hat; the multipliers of the working set
    for (int s = ot; s < nbox; s += nthr) {
      const int i = X.ip[s], isy = X.ip[nbox + s];
      const int cur = isy ? rr3_say(act[i]) : rr3_sa(act[i]);
      if (cur == 0) vg[s] = fma(X.bd[(size_t)R3B_C * nbox + s], bv[i], rr3_box_a(P, X, s, b, only...));
    }
    key = inf; ks = NONE;
    if (ot < k) {
      const int s = lcomp[ot], i = list[ot];
      const int cur = X.ip[nbox + s] ? rr3_say(act[i]) : rr3_sa(act[i]);
      const double c = X.bd[(size_t)R3B_C * nbox + s];
      const double hat = fma(c, bv[i], rr3_box_a(P, X, s, b, only...));
      const double bd = X.bd[(size_t)(cur > 0 ? R3B_HI : R3B_LO) * nbox + s];
      key = -((double)cur * (bd - hat) / fabs(c));
      ks = s;
    }
    double gneg;
    const int sr = arg_min(key, ks, &gneg);
    if (sr == NONE || !(gneg < 0.0)) break;                   // every multiplier has the right sign: optimal
    // release component sr: the last column takes its slot in W, in the Gram tiles and in the lists
    if (ot < k && lcomp[ot] == sr) flagw[4] = ot;
    __syncthreads();
    const int j = __builtin_amdgcn_readfirstlane(flagw[4]), last = k - 1;
    if (ot == 0) {
      const int i = list[j], isy = X.ip[nbox + sr];
      const int cur = isy ? rr3_say(act[i]) : rr3_sa(act[i]);
      act[i] -= cur * (isy ? 4 : 1);
    }
    if (j != last) {
      for (int i = ot; i < S.ldw; i += nthr) Wg[(size_t)i * cap + j] = Wg[(size_t)i * cap + last];
      if (ot <= last) hv[ot] = rr3w_tile(Gg, last >> 6, ot >> 6)[(last & 63) * 64 + (ot & 63)];   // row `last` of the Gram tiles
      __syncthreads();
      if (ot < last) {
        const double gv = (ot == j) ? hv[last] : hv[ot];
        if (ot <= j) rr3w_tile(Gg, j >> 6, ot >> 6)[(j & 63) * 64 + (ot & 63)] = gv;
        else rr3w_tile(Gg, ot >> 6, j >> 6)[(ot & 63) * 64 + (j & 63)] = gv;
      }
      if (ot == 0) { list[j] = list[last]; lcomp[j] = lcomp[last]; lsh[j] = lsh[last]; }
    }
    k = last;
    __syncthreads();
  }
  const int iter = P.max_iter + nsolve;
  if (st == 0) rr3_trsv_bwd(G, m64, r, live, b0, 0, y2, bv, red, tmp);   // the rows in front of the trailing block
  if (st != 0) k = 0;
  if (defer_outputs && st == 0) {
    double* vx = Vb + (size_t)R3_X * S.VL;
    double* vbeta = Vb + (size_t)R3_BETA * S.VL;
    double* vt0 = Vb + (size_t)R3_T0 * S.VL;
    for (int i = tid; i < r; i += nthr) { vx[perm[i]] = bv[i]; vbeta[i] = bv[i]; vt0[i] = tv[i]; kq[4 + cap + i] = act[i]; }
    if (tid < k) kq[4 + tid] = list[tid];
  }
  if (tid == 0) {
    kq[0] = k; kq[1] = st; kq[2] = iter; kq[3] = k;
    const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
    kq[4 + cap + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + cap + S.rv + 1] = (int)(t_end - t_begin);   // this kernel's own ticks (100 MHz)
    if (peak > kq[4 + cap + S.rv + 2]) kq[4 + cap + S.rv + 2] = peak;    // the larger of both phases
  }
  if (!defer_outputs || st != 0) {
    __syncthreads();
    rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, st, iter, tmp, u_opt, cost, status, iters, beta_ws, act_ws, only...);
  }
}

}  // namespace ddmpc
