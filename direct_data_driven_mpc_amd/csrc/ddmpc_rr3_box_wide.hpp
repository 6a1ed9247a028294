// ddmpc_rr3_box_wide.hpp -- DDMPC_OPT_LARGE_BOX_CAPACITY above 64: the bounded phase kernel with up to 256 active components at
// once.  rr3_solve_box_wide_kernel is a twin of rr3_solve_box_kernel (ddmpc_rr3_box.hpp): the same kept factor
// of the empty active set, the same Woodbury update on the trailing block, the same iteration rule and the same refinement
// pass.  A twin and not a parameter of that kernel, for the reason given there: handles at the default capacity keep their
// kernel as it is.  What differs is written for any number nblk = ceil(k / 64) of 64-column blocks; the capacity `cap` (a
// multiple of 64, a kernel argument) is the only size:
//   W        row-major [row - n0][cap]; one pass of the rr3_w_forward scheme per 64-column block
//   S        = diag(1 / d_s) - W'W as 64 x 64 tiles of the lower block triangle, tile (I, J) at Sg + (I (I + 1) / 2 + J) 4096,
//            row-major, in global memory per instance (L2) behind W; factored in place by a blocked Cholesky whose diagonal
//            tiles go through LDS (rr3_small_cholesky: reciprocal pivots on the diagonal), and kept for the refinement launch
//   LDS      Rr3Lds::total + 4 cap doubles: hv, ev, lsh (cap doubles each), list, lcomp (cap ints each)
//   record   kq = [k, state, iterations, k, switched positions (cap), active set (rv), start tick, ticks, peak k]
// Every sum has a fixed order (tiles and 16 x 16 sub-tiles are dealt to the waves by index, each finished by one wave), so the
// result of an instance does not depend on timing or on its batch neighbours.
#pragma once
#include "ddmpc_rr3_box.hpp"

namespace ddmpc {

__host__ __device__ constexpr int rr3w_lds_extra(int cap) { return 4 * cap; }                           // doubles behind Rr3Lds::total
__host__ __device__ constexpr long long rr3w_tiles(int cap) { return (long long)(cap / 64) * (cap / 64 + 1) / 2; }
__device__ __forceinline__ double* rr3w_tile(double* Sg, int I, int J) { return Sg + (size_t)(I * (I + 1) / 2 + J) * 4096; }

// rr3_w_forward for one 64-column block of W with row stride ldc: Wc points at the block's first column, list at the positions
// of its kb <= 64 columns.  The scheme, the operand layout and the order of the sums are those of rr3_w_forward.
__device__ __forceinline__ void rr3w_w_forward(const double* __restrict__ Lm, const double* __restrict__ m64, int n, unsigned long long live,
                                               int b_lo, int n0, const int* list, int kb, double* Wc, int ldc, double* Pb) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // (opaque per call, see rr3_trsv_fwd)
  const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = wave & 3, ch = wave >> 2;
  const int nb = (n + 63) >> 6;
  const int nct = (kb + 15) >> 4;
  const unsigned long long front = (b_lo > 0) ? ((1ull << (4 * b_lo)) - 1ull) : 0ull;
  int lcol[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) { const int col = 16 * (ch + 2 * t) + l15; lcol[t] = (col < kb) ? list[col] : -1; }
  for (int b = b_lo; b < nb; ++b) {
    const int i0 = 64 * b;
    const int irow = i0 + 16 * rt + l15;
    const double* Li = Lm + pk_row((size_t)(irow < n ? irow : n - 1)) + 4 * l4;
    const double az = (irow < n) ? 1.0 : 0.0;
    d4 acc[2];
    acc[0] = d4{0.0, 0.0, 0.0, 0.0}; acc[1] = d4{0.0, 0.0, 0.0, 0.0};
    unsigned long long lv = live & ((1ull << (4 * b)) - 1ull) & ~front;
    while (lv != 0ull) {
      const int jc = __builtin_ctzll(lv);
      lv &= lv - 1ull;
      const d4 la = *reinterpret_cast<const d4*>(Li + 16 * jc);
      const double* wr = Wc + (size_t)(16 * jc - n0 + 4 * l4) * ldc + l15;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (ch + 2 * t < nct) {                                              // (wave-uniform)
          double wv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[e] = wr[(size_t)e * ldc + 16 * (ch + 2 * t)];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = rr2_mfma(la[e] * az, wv[e], acc[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (ch + 2 * t < nct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rloc = 16 * rt + l4 + 4 * q;
          Pb[rloc * 65 + 16 * (ch + 2 * t) + l15] = ((lcol[t] == i0 + rloc) ? 1.0 : 0.0) - acc[t][q];
        }
      }
    }
    __syncthreads();
    const double* Mb = m64 + (size_t)b * 4096 + (size_t)(16 * rt + l15) * 64 + 4 * l4;
    d4 x[2];
    x[0] = d4{0.0, 0.0, 0.0, 0.0}; x[1] = d4{0.0, 0.0, 0.0, 0.0};
    for (int u = 0; u <= rt; ++u) {
      const d4 mv = *reinterpret_cast<const d4*>(Mb + 16 * u);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (ch + 2 * t < nct) {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[t] = rr2_mfma(mv[e], Pb[(16 * u + 4 * l4 + e) * 65 + 16 * (ch + 2 * t) + l15], x[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (ch + 2 * t < nct) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 16 * rt + l4 + 4 * q;
          Wc[(size_t)(i - n0) * ldc + 16 * (ch + 2 * t) + l15] = (i < n) ? x[t][q] : 0.0;
        }
      }
    }
    __syncthreads();                                                         // the rows of W of this block are visible (workgroup scope)
  }
}

// The tiles of -W'W (rr3_w_gram for two column blocks): tile (I, J), J <= I, entry [x][y] = -sum_i W[i][64 I + x] W[i][64 J + y]
// for 64 I + x < k (on the diagonal tile y <= x).  The 16 x 16 sub-tiles of all tiles are dealt to the eight waves.
__device__ __forceinline__ void rr3w_gram(const double* Wg, int ldc, int nrows, int k, double* Sg) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // (opaque per call, see rr3_trsv_fwd)
  const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = (int)(blockDim.x >> 6);
  const int nblk = (k + 63) >> 6;
  int idx = 0;
  for (int I = 0; I < nblk; ++I) {
    const int kbI = (k - 64 * I < 64) ? k - 64 * I : 64, ncI = (kbI + 15) >> 4;
    for (int J = 0; J <= I; ++J) {
      double* T = rr3w_tile(Sg, I, J);
      for (int a = 0; a < ncI; ++a)
        for (int c = 0; c < (J == I ? a + 1 : 4); ++c, ++idx) {
          if (idx % nwave != wave) continue;                                 // (wave-uniform)
          d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = d4{0.0, 0.0, 0.0, 0.0};
          const double* pa = Wg + (size_t)l4 * ldc + 64 * I + 16 * a + l15;
          const double* pc = Wg + (size_t)l4 * ldc + 64 * J + 16 * c + l15;
          int i = 0;
          for (; i + 8 <= nrows; i += 8) {
            acc0 = rr2_mfma(pa[(size_t)i * ldc], pc[(size_t)i * ldc], acc0);
            acc1 = rr2_mfma(pa[(size_t)(i + 4) * ldc], pc[(size_t)(i + 4) * ldc], acc1);
          }
          for (; i < nrows; i += 4) {
            const bool ok = i + l4 < nrows;
            const double va = ok ? pa[(size_t)i * ldc] : 0.0, vc = ok ? pc[(size_t)i * ldc] : 0.0;
            acc0 = rr2_mfma(va, vc, acc0);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int x = 16 * a + l4 + 4 * q, y = 16 * c + l15;
            if (x < kbI && (J < I || y <= x)) T[x * 64 + y] = -(acc0[q] + acc1[q]);
          }
        }
    }
  }
}

// Block column J of the blocked Cholesky, first half: tile (I, J) -= sum_{K < J} L(I, K) L(J, K)' for I = J .. nblk - 1, on the
// matrix pipe (K ascending, 16 columns of the tiles per four steps).  A lane reads 32 bytes of a row of each tile: the four
// entries feed the four contraction steps, the same permutation on both operands.  Rows of a last, partly filled block row
// that hold no component only ever reach entries nobody reads (a product entry depends on one row of each operand).
__device__ __forceinline__ void rr3w_chol_update(double* Sg, int J, int nblk) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));     // (opaque per call, see rr3_trsv_fwd)
  const int lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = (int)(blockDim.x >> 6);
  int idx = 0;
  for (int I = J; I < nblk; ++I)
    for (int a = 0; a < 4; ++a)
      for (int c = 0; c < (I == J ? a + 1 : 4); ++c, ++idx) {
        if (idx % nwave != wave) continue;                                   // (wave-uniform)
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        for (int K = 0; K < J; ++K) {
          const double* A = rr3w_tile(Sg, I, K) + (size_t)(16 * a + l15) * 64 + 4 * l4;
          const double* B = rr3w_tile(Sg, J, K) + (size_t)(16 * c + l15) * 64 + 4 * l4;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const d4 la = *reinterpret_cast<const d4*>(A + 16 * cc), lb = *reinterpret_cast<const d4*>(B + 16 * cc);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = rr2_mfma(la[e], lb[e], acc);
          }
        }
        double* T = rr3w_tile(Sg, I, J);
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(16 * a + l4 + 4 * q) * 64 + 16 * c + l15] -= acc[q];
      }
}

// Second half: the rows of the tiles below the diagonal tile against L_JJ' (X L_JJ' = T: a forward substitution per row, one
// thread per row, in place; L_JJ in LDS with its reciprocal pivots, row stride 65, every read a broadcast).  Block J is full
// (64 columns) whenever a tile lies below it.  Eight columns at a time in registers.
__device__ __forceinline__ void rr3w_chol_rows(double* row, const double* Sm) {
  constexpr int CH = 8;                                                      // (registers: two workgroups per CU)
  for (int cj = 0; cj < 64 / CH; ++cj) {
    double t[CH];
#pragma unroll
    for (int v = 0; v < CH / 4; ++v) {
      const d4 ld = *reinterpret_cast<const d4*>(row + CH * cj + 4 * v);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[4 * v + e] = ld[e];
    }
    for (int cq = 0; cq < cj; ++cq) {
      double xq[CH];
#pragma unroll
      for (int v = 0; v < CH / 4; ++v) {
        const d4 ld = *reinterpret_cast<const d4*>(row + CH * cq + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) xq[4 * v + e] = ld[e];
      }
      const double* Lq = Sm + (CH * cj) * 65 + CH * cq;
#pragma unroll
      for (int jj = 0; jj < CH; ++jj) {
#pragma unroll
        for (int qq = 0; qq < CH; ++qq) t[jj] = fma(-xq[qq], Lq[jj * 65 + qq], t[jj]);
      }
    }
    const double* Lj = Sm + (CH * cj) * 65 + CH * cj;
#pragma unroll
    for (int jj = 0; jj < CH; ++jj) {
#pragma unroll
      for (int qq = 0; qq < jj; ++qq) t[jj] = fma(-t[qq], Lj[jj * 65 + qq], t[jj]);
      t[jj] *= Lj[jj * 65 + jj];
    }
#pragma unroll
    for (int v = 0; v < CH / 4; ++v) *reinterpret_cast<d4*>(row + CH * cj + 4 * v) = d4{t[4 * v], t[4 * v + 1], t[4 * v + 2], t[4 * v + 3]};
  }
}

// The two halves of rr3_small_solve on one diagonal tile (wave 0, lane = row, kb rows; Sm: row stride 65, reciprocal pivots):
// L w = h, and L' e = w.  h is this lane's entry, the result is returned in its place.
__device__ __forceinline__ double rr3w_tile_fwd(const double* Sm, int kb, int x, double h) {
  const double il = (x < kb) ? Sm[x * 65 + x] : 0.0;
  for (int i = 0; i < kb; ++i) {
    const double e = __shfl(h * il, i, 64);
    if (x == i) h = e;
    else if (x > i && x < kb) h = fma(-Sm[x * 65 + i], e, h);
  }
  return h;
}
__device__ __forceinline__ double rr3w_tile_bwd(const double* Sm, int kb, int x, double h) {
  const double il = (x < kb) ? Sm[x * 65 + x] : 0.0;
  for (int i = kb - 1; i >= 0; --i) {
    const double e = __shfl(h * il, i, 64);
    if (x == i) h = e;
    else if (x < i) h = fma(-Sm[i * 65 + x], e, h);
  }
  return h;
}

// DDMPC_OPT_LARGE_BOX_WARM_START: the signed set the handle's last solve ended with, sa + 4 say per row in COMPONENT order
// ([batch][rE] bytes, the layout of the act_ws workspace; written by rr3_box_keep_seed_kernel behind the last launch of a solve),
// and whether rr3_box_safeguard_kernel follows the launch (a seeded run at the cap is then left to it).
struct Rr3Seed {
  const signed char* set;
  int safeguard;
};

// ---------------------------------------------------------------------------------------------------------------
// The solve on the kept factor with the table-driven box and up to `cap` active components (the twin of rr3_solve_box_kernel;
// same launch geometry, LDS of Rr3Lds::total + rr3w_lds_extra(cap) doubles).  More than cap active components in an iteration,
// or a non-positive pivot in any diagonal tile of S: status 4 at that iteration.
// Seed...: empty (the kernel as it is launched without a seed) or one Rr3Seed ("Warm start"): when the empty
// set's solution violates a bound and the seed holds an active component, the iteration goes on from the seed instead of from
// what the test asked for.  A seeded run that ends at the cap, beyond the capacity or on a non-positive pivot starts again from
// the empty set (act = 0, y' = y, beta of the trailing block by one backward substitution) with a fresh cap; run0 is the count
// before the run in progress, so iter - run0 is that run's own count and iter every solve attempted, the empty set's once.
// The record of a failed instance holds the count of its LAST run (kq[2] >= max_iter: that run ended at its own cap, what
// rr3_box_safeguard_kernel asks), that of a finished one the whole count.
// Behind the seed, or alone: one Rr3Only (DDMPC_OPT_LARGE_BOX_LAW, the instance filter; both launches).
// Or, alone in the pack: one Rr3Setpoint (DDMPC_OPT_LARGE_SETPOINT_BOUNDS, both launches; as in rr3_solve_box_kernel).
// ---------------------------------------------------------------------------------------------------------------
template <bool REFINE_PASS, class... Seed>
__global__ __launch_bounds__(RR2_TS, 4) void rr3_solve_box_wide_kernel(Rr3 S, KParams P, int RPs, const double* __restrict__ u_past,
                                                                    const double* __restrict__ y_past, double* __restrict__ u_opt,
                                                                    double* __restrict__ cost, int* __restrict__ status,
                                                                    int* __restrict__ iters, double* __restrict__ beta_ws,
                                                                    signed char* __restrict__ act_ws, int defer_outputs, Rr3Box X, int cap,
                                                                    Seed... seed) {
  constexpr bool SEEDED = rr3_has_arg<Rr3Seed, Seed...>, ONLY = rr3_has_arg<Rr3Only, Seed...>, SETPOINTS = rr3_has_arg<Rr3Setpoint, Seed...>;
  static_assert(sizeof...(Seed) == (SEEDED ? 1 : 0) + (ONLY ? 1 : 0) + (SETPOINTS ? 1 : 0) && !(REFINE_PASS && SEEDED) &&
                    !(SETPOINTS && (SEEDED || ONLY)),
                "one seed (for the solve launch only) and one filter at most, or one setpoint alone");
  extern __shared__ __attribute__((aligned(16))) double r3_lds[];
  const long long b = blockIdx.x;
  if constexpr (ONLY) {
    if (rr3_get_arg<Rr3Only>(seed...).only[b] == 0) return;                 // (workgroup-uniform)
  }
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int r = S.r, nA = S.nA, n0 = S.n0, m = P.m, p = P.p;
  const int n = P.npu / m;
  const Rr3Lds LD = Rr3Lds::make(r);
  double* tv = r3_lds + LD.tv; double* yv = r3_lds + LD.yv; double* y2 = r3_lds + LD.y2; double* bv = r3_lds + LD.bv;
  int* act = reinterpret_cast<int*>(r3_lds + LD.act);
  double* big = r3_lds + LD.big;                             // tile exchange of rr3w_w_forward | a diagonal tile of S | reduction buffer of the backward substitution
  double* red = big; double* Sm = big;
  double* tmp = r3_lds + LD.tmp; double* hpart = tmp + 64;
  int* flagw = reinterpret_cast<int*>(r3_lds + LD.list);     // [0] changed  [1] k  [2] small-system failure  [3] the largest k so far
  double* hv = r3_lds + LD.total; double* ev = hv + cap;     // right-hand side / solution of the k x k system
  double* lsh = ev + cap;                                    // the shift of t of the active component in column j ...
  int* list = reinterpret_cast<int*>(lsh + cap);             // ... its position ...
  int* lcomp = list + cap;                                   // ... and its table index
  const int* perm = S.perm;
  const double* G = S.ws + b * S.stride;
  const double* m64 = S.m64 + b * S.m64_stride;
  const unsigned long long live = S.dd[4 * b + 2];
  const int nb = (r + 63) >> 6, b0 = n0 >> 6, nT = r - n0;
  double* Vb = S.V + b * S.vstride;                          // [R3_X | R3_BETA | R3_T0]
  double* Wg = S.Wg + b * S.wstride;                         // W, row-major [row - n0][cap]
  double* Sg = Wg + (size_t)S.ldw * cap;                     // the tiles of S, factored in place
  int* kq = S.kq + b * S.kstride;
  const double* up = u_past + b * (long long)P.npu;
  const double* yp = y_past + b * (long long)(n * p);
  int st = 0, iter = 0, k = 0;
  [[maybe_unused]] int run0 = 0, phase = 0;                  // (seeded) the count before the run in progress; 0 no seed yet, 1 the seeded run, 2 started again
  const long long t_begin = (long long)__builtin_amdgcn_s_memrealtime();   // diagnostics (kq[.. + rv ..]): when this workgroup ran
  // h = W'v on the trailing block (v: LDS, absolute rows), into hv[0 .. k): a column per thread of each of the 8 row parts
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
  // v_T += W e on the trailing block (one thread per row; the row of W is contiguous)
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
  auto stage_tile = [&](int J) {                             // diagonal tile J of S into Sm (row stride 65)
    const double* T = rr3w_tile(Sg, J, J);
    int ot = threadIdx.x;
    asm volatile("" : "+v"(ot));
    for (int e = ot; e < 4096; e += nthr) Sm[(e >> 6) * 65 + (e & 63)] = T[e];
  };
  // ev = S^-1 hv on the tile factor: forward and backward over the blocks (hv is used up).  Off-diagonal tiles: plain
  // products, the contraction index split over the 8 row parts and summed in a fixed order.
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

  if constexpr (!REFINE_PASS) {
    double nbad = 0.0;
    for (int i = tid; i < LD.VL; i += nthr) {
      double t = 0.0;
      if (i < r) {
        const int rho = perm[i];
        const int pidx = P.tabi[1 * RPs + rho];
        t = (pidx >= 0) ? ((pidx < P.npu) ? up[pidx] : yp[pidx - P.npu]) : rr3_target(P, RPs, rho, b, seed...);
        nbad += S.skip[b * S.s_stride + i] ? 1.0 : 0.0;
      }
      tv[i] = t; act[i] = 0; y2[i] = 0.0; bv[i] = 0.0;
    }
    if (tid == 0) flagw[3] = 0;
    if constexpr (SEEDED) { if (tid == 0) flagw[5] = 0; }      // [5] the seed holds an active component
    if (block_sum(nbad, tmp) != 0.0) st = 4;                 // (uniform) a pivot of K0 failed: not positive definite numerically
    if constexpr (SETPOINTS) {                               // (uniform) a refused setpoint: nothing is iterated
      const int refuse = rr3_setpoint_refusal(P, X, b, rr3_get_arg<Rr3Setpoint>(seed...));
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
        // (seeded) give the run in progress up: the empty set again, its beta on the trailing block (yv is kept), a fresh cap
        [[maybe_unused]] auto restart = [&]() {
          int ot = threadIdx.x;
          asm volatile("" : "+v"(ot));
          for (int i = ot; i < LD.VL; i += nthr) { act[i] = 0; y2[i] = yv[i]; }
          __syncthreads();
          rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);
          run0 = iter; phase = 2; k = 0;
        };
        for (;;) {
          ++iter;
          if (tid == 0) flagw[0] = 0;
          __syncthreads();
          int ot = threadIdx.x;
          asm volatile("" : "+v"(ot));     // (opaque per iteration: the table addresses are formed here, not kept alive across the kernel)
          // the violation test of rr3_solve_box_kernel, unchanged
          for (int s = ot; s < X.nbox; s += nthr) {
            const int i = X.ip[s], isy = X.ip[X.nbox + s];
            const int code = __hip_atomic_load(&act[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int cur = isy ? rr3_say(code) : rr3_sa(code);
            const double hat = fma(X.bd[(size_t)R3B_C * X.nbox + s], bv[i], rr3_box_a(P, X, s, b, seed...));
            const int upv = hat > X.bd[(size_t)R3B_HI * X.nbox + s], dnv = hat < X.bd[(size_t)R3B_LO * X.nbox + s];
            const int ns = cur > 0 ? upv : (cur < 0 ? -dnv : upv - dnv);
            if (ns != cur) { atomicAdd(&act[i], (ns - cur) * (isy ? 4 : 1)); flagw[0] = 1; }
          }
          __syncthreads();
          if (flagw[0] == 0) break;
          if constexpr (SEEDED) {
            const Rr3Seed sd = rr3_get_arg<Rr3Seed>(seed...);
            if (iter - run0 >= P.max_iter) {
              if (phase != 1 || sd.safeguard) { st = 4; break; }       // (a seeded run at the cap with the safeguard on: left to it)
              --iter;                                                  // (the test that found the cap followed a solve already counted)
              restart();
              continue;
            }
            if (phase == 0) {
              // the empty set's solution violates a bound: the seed, read component by component (a code outside the table's
              // components or outside -1 .. 1 is no seed), takes the place of what the test asked for -- unless it is empty
              phase = 2;
              const signed char* sset = sd.set + b * (long long)P.rE;
              for (int s = ot; s < X.nbox; s += nthr) {
                const int code = sset[perm[X.ip[s]]];
                const int a = X.ip[X.nbox + s] ? rr3_say(code) : rr3_sa(code);
                if (a == 1 || a == -1) flagw[5] = 1;
              }
              __syncthreads();
              if (flagw[5] != 0) {                                     // (uniform)
                phase = 1;
                for (int i = ot; i < LD.VL; i += nthr) act[i] = 0;
                __syncthreads();
                for (int s = ot; s < X.nbox; s += nthr) {
                  const int i = X.ip[s], isy = X.ip[X.nbox + s];
                  const int code = sset[perm[i]];
                  const int a = isy ? rr3_say(code) : rr3_sa(code);
                  if (a == 1 || a == -1) atomicAdd(&act[i], a * (isy ? 4 : 1));
                }
                __syncthreads();
              }
            }
          } else if (iter >= P.max_iter) {
            st = 4;
            break;
          }
          // the active components, ascending (deterministic column order)
          if (ot < 64) {
            int base = 0;
            for (int s0 = 0; s0 < X.nbox; s0 += 64) {
              const int s = s0 + (ot & 63);
              int a = 0, i = 0;
              if (s < X.nbox) { i = X.ip[s]; a = X.ip[X.nbox + s] ? rr3_say(act[i]) : rr3_sa(act[i]); }
              const unsigned long long mk = __ballot(a != 0);
              const int slot = base + __popcll(mk & ((1ull << (ot & 63)) - 1ull));
              if (a != 0 && slot < cap) {
                list[slot] = i; lcomp[slot] = s;
                lsh[slot] = rr3_box_shift(P, X, s, a > 0, b, seed...);
              }
              base += __popcll(mk);
            }
            if ((ot & 63) == 0) { flagw[1] = base; if (base > flagw[3]) flagw[3] = base; }
          }
          __syncthreads();
          k = flagw[1];
          if constexpr (SEEDED) {
            if (k > cap && phase == 1) { restart(); continue; }
          }
          if (k > cap) { st = 4; k = 0; break; }                          // more columns than W holds
          const int nblk = (k + 63) >> 6;
          for (int cb = 0; cb < nblk; ++cb)                               // W = L_TT^-1 E_T, 64 columns per pass
            rr3w_w_forward(G, m64, r, live, b0, n0, list + 64 * cb, (k - 64 * cb < 64) ? k - 64 * cb : 64, Wg + 64 * cb, cap, big);
          rr3w_gram(Wg, cap, nT, k, Sg);                                  // the tiles of -W'W
          w_apply(yv, y2, lsh);                                           // y + W shift
          w_times(y2);                                                    // hv = W'(y + W shift): no Gram tile needed
          if (ot < k) rr3w_tile(Sg, ot >> 6, ot >> 6)[(ot & 63) * 65] += X.bd[(size_t)R3B_INVD * X.nbox + lcomp[ot]];   // the component's own 1 / d_s
          __syncthreads();
          // blocked Cholesky of S, in place
          int bad = 0;
          for (int J = 0; J < nblk && !bad; ++J) {
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
          if constexpr (SEEDED) {
            if (bad && phase == 1) { restart(); continue; }
          }
          if (bad) { st = 4; k = 0; break; }
          s_solve();
          if (ot < k) ev[ot] += lsh[ot];                                  // y' = y + W (shift + cv) on the trailing block
          __syncthreads();
          w_apply(yv, y2, ev);
          rr3_trsv_bwd(G, m64, r, live, nb, b0, y2, bv, red, tmp);
        }
        if (st == 0) rr3_trsv_bwd(G, m64, r, live, b0, 0, y2, bv, red, tmp);   // the rows in front of the trailing block
      }
    }
    if (defer_outputs && st == 0) {
      // what the refinement launch needs: beta (both orders), t0, the active set (codes), the switched positions (W and the
      // tile factor of S are in global memory already)
      double* vx = Vb + (size_t)R3_X * S.VL;
      double* vbeta = Vb + (size_t)R3_BETA * S.VL;
      double* vt0 = Vb + (size_t)R3_T0 * S.VL;
      for (int i = tid; i < r; i += nthr) { vx[perm[i]] = bv[i]; vbeta[i] = bv[i]; vt0[i] = tv[i]; kq[4 + cap + i] = act[i]; }
      if (tid < k) kq[4 + tid] = list[tid];
    }
    if (tid == 0) {
      kq[0] = (st == 0) ? k : 0; kq[1] = st; kq[2] = iter; kq[3] = k;
      if constexpr (SEEDED) { if (st != 0) kq[2] = iter - run0; }        // (a failed instance: the count of its last run)
      const long long t_end = (long long)__builtin_amdgcn_s_memrealtime();
      kq[4 + cap + S.rv] = (int)(t_begin & 0x7fffffff); kq[4 + cap + S.rv + 1] = (int)(t_end - t_begin);   // (100 MHz ticks)
      kq[4 + cap + S.rv + 2] = flagw[3];                                  // the most components active in any iteration
    }
    if (!defer_outputs || st != 0) {
      __syncthreads();
      rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, st, iter, tmp, u_opt, cost, status, iters, beta_ws, act_ws, seed...);
    }
  } else {
    // ---- one pass of iterative refinement on the system of the final active set (as rr3_solve_box_kernel), then the outputs
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
        bb = vbeta[i]; t0 = vt0[i]; a = kq[4 + cap + i];
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
      w_times(yv);
      s_solve();
      w_apply(yv, yv, ev);
    }
    rr3_trsv_bwd(G, m64, r, live, nb, 0, yv, y2, red, tmp);                                                   // delta
    for (int i = tid; i < r; i += nthr) bv[i] += y2[i];
    __syncthreads();
    rr3_box_outputs(P, RPs, X, b, perm, tv, bv, act, 0, iter, tmp, u_opt, cost, status, iters, beta_ws, act_ws, seed...);
  }
}

// DDMPC_OPT_LARGE_BOX_WARM_START: behind the last launch of a solve, what the call finally reported becomes the seed of the next
// step -- the codes rr3_box_outputs left in act_ws (component order) for an instance with status 0 or 1, the empty set for any
// other (its codes were not written).  A buffer of its own: act_ws is the workspace ddmpc_get_solution reads, shared by every
// route of the handle.
__global__ void rr3_box_keep_seed_kernel(int r, int rE, const int* __restrict__ status, const signed char* __restrict__ act_ws,
                                         signed char* __restrict__ seed) {
  const long long b = blockIdx.x;
  const int st = status[b];
  for (int i = threadIdx.x; i < rE; i += blockDim.x)
    seed[b * (long long)rE + i] = (i < r && (st == 0 || st == 1)) ? act_ws[b * (long long)rE + i] : (signed char)0;
}

}  // namespace ddmpc
