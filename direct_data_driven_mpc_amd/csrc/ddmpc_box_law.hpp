// ddmpc_box_law.hpp -- input bounds u_min <= ubar <= u_max for ROBUST controllers on the register-resident sizes
// (ddmpc_set_input_bounds, (m+p)(L+n) <= 271): the primal-dual active-set iteration of the warm CONVEX path
// (ddmpc_aux_kernels.hpp, CwlLds / cwl_iterate) with a per-component description of the box instead of the slack box's
// symmetric +-bound.  Included by the API translation unit only.
//
// A free input row of the reduced system is z_i = t_i - lam D0_i beta_i, D0_i = 1 / w_i.  Holding it at a
// bound makes the row hard -- D1_i = 0, t_i = bound --, the same diagonal rank-k change of K0 the slack box makes:
//     K(A) = K0 - E_A diag(d_A) E_A',  d_s = lam (D0_s - D1_s)        t(A) = t0 + E_A shift_A
//     beta(A) = beta0 + M_A ev,   ev = shift_A + (diag(1/d_A) - M[A,A])^-1 (beta0[A] + M[A,A] shift_A)
// Boxed components s = 0 .. nbox-1 in ascending row order (the slack components of a CONVEX controller and the free input
// rows of the channels with a finite bound), shared by the batch and tabulated on the host:
//     tab = [box_rho (nbox) | box_of (r): s, or -1]
//     bd  = [a | c | lo | hi | 1/d], nbox doubles each:  hat_s = a_s + c_s beta_rho is the value the component takes when it
//           is released (for an active one beta_rho is the multiplier: mu_s = 2 w_s (hat_s - bound_s)).  From the empty set: an
//           inactive component becomes +1 if hat_s > hi_s, -1 if hat_s < lo_s; one at +1 stays while hat_s > hi_s, one at -1
//           while hat_s < lo_s, and is released otherwise (BoxTab::test);  shift_s = (hi_s or lo_s) - a_s.
//       slack:  a = 0,  c = -lam / lamb_sigma, lo / hi = -+ c_param eps_max, d = lam (D0 - D1)
//       input:  a = tb (= u_s), c = -lam D0,   lo / hi = u_min / u_max of the channel (either may be infinite), d = lam D0
//       output: a = tb (= y_s), c = -lam / q,  lo / hi = y_min / y_max of the channel,                   d = lam / q
// Output bounds (ddmpc_set_output_bounds, the YB instantiations): a K_WPRED row carries ybar AND sigma, so a CONVEX handle has
// two boxed components on such a row, the slack before the output; D_rho = [slack free] / lamb_sigma + [output free] / q, and
// with both active the row is hard.  Both change the same diagonal entry, so M keeps ONE column per boxed row: the table grows
//     tab = [box_rho (nbox) | box_of (r): the slack or input component | col (nbox): column of M | box_ofy (r): the output
//            component, or -1 | ncol | col_rho (ncol)]
// and the kernels run with max(r, nbox) threads rounded up to 64 (thread s looks at component s; nbox <= WARM_MAX_R).  The
// instantiations without YB never look beyond [box_rho | box_of]: col(s) = s there.
// The k x k system lives in LDS up to CWL_KLDS components and in the instance's slice of `sg` beyond; M = K0^-1 E_box is
// nbox * r doubles per instance (122 KB at L = 30, n = 4, m = p = 2, CONVEX, both channels bounded: 0.5 GB at 4096 instances).
//
// Per-instance bounds (ddmpc_set_instance_input_bounds, ddmpc_set_instance_output_bounds; slack NONE or the CONVEX slack box):
// the instantiations of the two kernels below with a BoxChannels element, whose bounds come from a per-instance channel table
// instead of the shared [lo | hi] columns of `bd`.  M = K0^-1 E_box, the law and the box list depend on WHICH rows are boxed,
// not on the bound values: the list is the union over the batch (a channel is listed when any instance has a finite bound on
// it) and stays shared.  The bound values enter the solve through BoxTab::lo / BoxTab::hi only -- the violation test, the
// shifts, the safeguard's ratios and the output stage's "held at its bound exactly".  The kernels keep blo[s] / bhi[s] in LDS by
// boxed component, filled once per launch (the loop kernel: once per instance, not per solve), and point their copy of the
// table at them: box_iterate, box_solve_set, box_safeguard, box_beta, box_component and box_component_y are used as they stand.
// An instance whose own bound on a listed component is infinite never activates it (hat > +inf and hat < -inf are false), so
// its shift is never formed.
//     chb [batch][lo (nch) | hi (nch)], inputs first, -+infinity where the instance has no bound on the channel;
//     a slack component (CONVEX) keeps -+ c eps_max from the shared `bd`; an input or output component takes its channel's entry.
// With the channel table the iteration always starts from the empty set (no instantiation takes a seed and a table).  beta and
// the signed active set are written as with shared bounds: ddmpc_get_solution reconstructs with the same channel table.
#pragma once
#include <type_traits>

#include "ddmpc_aux_kernels.hpp"

namespace ddmpc {

struct BoxTab {
  int nbox;
  const int *rho, *of;
  const double *a, *c, *lo, *hi, *invd;
  __device__ __forceinline__ BoxTab(int nbox_, const int* __restrict__ tab, const double* __restrict__ bd)
      : nbox(nbox_), rho(tab), of(tab + nbox_), a(bd), c(bd + nbox_), lo(bd + 2 * nbox_), hi(bd + 3 * nbox_), invd(bd + 4 * nbox_) {}
  // the side component j belongs on, given the beta of its row and the side it is on now: an inactive one goes to the bound
  // it violates; an active one stays while its multiplier has the right sign (hat beyond ITS bound) and is released otherwise
  // -- never moved to the other bound in one step, the rule of the full-space reference formulation (with a two-sided box
  // whose width is small against the unconstrained moves, jumping from bound to bound makes the iteration cycle)
  __device__ __forceinline__ int test(int j, double beta, int cur) const {
    const double hat = fma(c[j], beta, a[j]);
    const int up = hat > hi[j], dn = hat < lo[j];
    return cur > 0 ? up : (cur < 0 ? -dn : up - dn);
  }
  __device__ __forceinline__ double bound(int j, int act) const { return act > 0 ? hi[j] : lo[j]; }
  __device__ __forceinline__ double shift(int j, int act) const { return bound(j, act) - a[j]; }
};

// ... with output bounds: the column of M of every component, the output component of every row, the columns of M.
struct BoxTabY : BoxTab {
  const int *col, *ofy;
  int ncol;
  __device__ __forceinline__ BoxTabY(int nbox_, const int* __restrict__ tab, const double* __restrict__ bd, int r)
      : BoxTab(nbox_, tab, bd), col(tab + nbox_ + r), ofy(tab + 2 * nbox_ + r), ncol(tab[2 * (nbox_ + r)]) {}
};
template <bool YB> using BoxTabT = std::conditional_t<YB, BoxTabY, BoxTab>;
template <bool YB>
__device__ __forceinline__ BoxTabT<YB> box_table(int nbox, const int* __restrict__ tab, const double* __restrict__ bd, int r) {
  if constexpr (YB) return BoxTabY(nbox, tab, bd, r); else return BoxTab(nbox, tab, bd);
}
// the column of M of component j, and CwlLds::m / CwlLds::beta through it (the LDS slots are keyed by column)
template <bool YB>
__device__ __forceinline__ int box_col(const BoxTabT<YB>& T, int j) {
  if constexpr (YB) return T.col[j]; else return j;
}
template <bool YB>
__device__ __forceinline__ double box_beta(const CwlLds& s, const BoxTabT<YB>& T, const double* __restrict__ Mb, int r, double b0,
                                           int rho) {
  if constexpr (YB) {
    double v = b0;
    for (int i = 0; i < s.kfin; ++i) v += s.m(Mb, r, T.col[s.al[i]], rho) * s.ev[i];
    return v;
  } else {
    return s.beta(Mb, r, b0, rho);
  }
}

// The active-set iteration of one instance by the whole workgroup: cwl_iterate with the table (same control flow, same
// count of solves, status 4 at the cap or on a non-positive pivot of the k x k system; blockDim.x >= r and > nbox).  YB: two
// active components of one row share their column of M (box_col) and its LDS slot.
template <bool YB>
__device__ int box_iterate(const KParams& P, const BoxTabT<YB>& T, const double* __restrict__ Mb, double* __restrict__ Sg,
                           const double* b0, CwlLds& s, int* iters) {
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, r = P.r, nbox = T.nbox;
  for (int j = tid; j < nbox; j += nthr) { s.bc[j] = b0[T.rho[j]]; s.act[j] = 0; s.slot[j] = -1; }
  if (tid == 0) { s.kfin = 0; s.fail = 0; s.nslots = 0; }
  int iter = 1, st = 0;
  for (;;) {
    if (tid == 0) s.changed = 0;
    __syncthreads();
    for (int j = tid; j < nbox; j += nthr) {
      const int ns = T.test(j, s.bc[j], s.act[j]);
      if (ns != s.act[j]) { s.act[j] = (signed char)ns; s.changed = 1; }
    }
    __syncthreads();
    if (!s.changed) break;
    if (iter >= P.max_iter) { st = 4; break; }
    ++iter;
    // the active set in ascending order: one ballot per wave (nbox < blockDim.x: thread s looks at component s)
    const bool a = tid < nbox && s.act[tid] != 0;
    const unsigned long long mk = __ballot(a);
    if (lane == 0) s.wcnt[wave] = __popcll(mk);
    __syncthreads();
    int off = 0, k = 0;
    for (int w = 0; w < (nthr >> 6); ++w) { off += (w < wave) ? s.wcnt[w] : 0; k += s.wcnt[w]; }
    if (a) s.al[off + __popcll(mk & ((1ull << lane) - 1ull))] = tid;
    const int n0 = s.nslots;                                          // (read by all before thread 0 changes it)
    __syncthreads();
    if (tid == 0) {                                                   // LDS slots for columns that enter A for the first time
      int ns_ = n0;
      for (int i = 0; i < k && ns_ < CWL_CC; ++i) {
        const int j = box_col<YB>(T, s.al[i]);
        if (s.slot[j] < 0) { s.slot[j] = ns_; s.slotj[ns_] = j; ++ns_; }
      }
      s.nslots = ns_;
    }
    __syncthreads();
    const int n1 = s.nslots;
    for (int e = tid; e < (n1 - n0) * r; e += nthr) {                 // coalesced r-vectors
      const int sl = n0 + e / r, rho = e - (e / r) * r;
      s.Mc[sl][rho] = Mb[(long long)s.slotj[sl] * r + rho];
    }
    __syncthreads();
    // S = diag(1/d_A) - M[A,A] (lower triangle) and the right-hand side beta0[A] + M[A,A] shift_A
    double* Sp = (k <= CWL_KLDS) ? s.S : Sg;
    for (int e = tid; e < k * k; e += nthr) {
      const int i = e / k, l = e - i * k;
      if (l <= i) {
        const int ri = T.rho[s.al[i]];
        double v = -s.m(Mb, r, box_col<YB>(T, s.al[l]), ri);
        if (l == i) v += T.invd[s.al[i]];
        Sp[i * (i + 1) / 2 + l] = v;
      }
    }
    for (int i = tid; i < k; i += nthr) {
      const int ri = T.rho[s.al[i]];
      double g = b0[ri];
      for (int l = 0; l < k; ++l) g += s.m(Mb, r, box_col<YB>(T, s.al[l]), ri) * T.shift(s.al[l], s.act[s.al[l]]);
      s.ev[i] = g;
    }
    __syncthreads();
    // Cholesky, right-looking, one column per step
    for (int c = 0; c < k; ++c) {
      if (tid == 0) {
        const double pv = Sp[c * (c + 1) / 2 + c];
        if (!(pv > 0.0)) s.fail = 1; else Sp[c * (c + 1) / 2 + c] = sqrt(pv);
      }
      __syncthreads();
      if (s.fail) break;
      const double dc = Sp[c * (c + 1) / 2 + c];
      for (int i = c + 1 + tid; i < k; i += nthr) Sp[i * (i + 1) / 2 + c] /= dc;
      __syncthreads();
      const int nt = k - c - 1;
      for (int e = tid; e < nt * nt; e += nthr) {
        const int ii = e / nt, jj = e - ii * nt;
        if (jj <= ii) {
          const int i = c + 1 + ii, j = c + 1 + jj;
          Sp[i * (i + 1) / 2 + j] -= Sp[i * (i + 1) / 2 + c] * Sp[j * (j + 1) / 2 + c];
        }
      }
      __syncthreads();
    }
    if (s.fail) { if (tid == 0) s.kfin = 0; st = 4; __syncthreads(); break; }
    if (tid == 0) {                                                   // L y = g, L' x = y, ev = shift + x
      for (int i = 0; i < k; ++i) {
        double v = s.ev[i];
        for (int l = 0; l < i; ++l) v -= Sp[i * (i + 1) / 2 + l] * s.ev[l];
        s.ev[i] = v / Sp[i * (i + 1) / 2 + i];
      }
      for (int i = k - 1; i >= 0; --i) {
        double v = s.ev[i];
        for (int l = i + 1; l < k; ++l) v -= Sp[l * (l + 1) / 2 + i] * s.ev[l];
        s.ev[i] = v / Sp[i * (i + 1) / 2 + i];
      }
      for (int i = 0; i < k; ++i) s.ev[i] += T.shift(s.al[i], s.act[s.al[i]]);
      s.kfin = k;
    }
    __syncthreads();
    for (int j = tid; j < nbox; j += nthr) s.bc[j] = box_beta<YB>(s, T, Mb, r, b0[T.rho[j]], T.rho[j]);
  }
  *iters = iter;
  return st;
}

// LDS of the safeguard, in the box kernels' SAFE instantiations only (CwlLds is shared with the slack-only kernels and stays
// as it is): the primal iterate v by boxed component, and one (key, component) pair per wave for the two selections.
constexpr int BOX_NONE = 0x7fffffff;

struct BoxSafeLds {
  double v[WARM_MAX_R];
  double wkey[16];
  int widx[16];
};

// The smallest key over the workgroup, the lowest idx among equal keys, to every thread (idx = BOX_NONE: no candidate).
__device__ __forceinline__ void box_argmin(double& key, int& idx, BoxSafeLds& q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    const double k2 = __shfl_xor(key, o);
    const int i2 = __shfl_xor(idx, o);
    if (k2 < key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
  }
  if (lane == 0) { q.wkey[wave] = key; q.widx[wave] = idx; }
  __syncthreads();
  key = q.wkey[0]; idx = q.widx[0];
  for (int w = 1; w < nw; ++w) {
    const double k2 = q.wkey[w];
    const int i2 = q.widx[w];
    if (k2 < key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
  }
  __syncthreads();
}

// The solve of box_iterate's loop body for the signed set in s.act, by the whole workgroup (s.act settled by a barrier before
// the call): the set in ascending order (s.al), LDS slots for columns of M that enter it for the first time, the k x k system,
// its Cholesky factorisation, ev and s.kfin, then s.bc = the beta of every boxed component (no barrier after it).  True on a
// non-positive pivot (s.fail; s.kfin = 0: the beta of the empty set).  A twin of that loop body, not a part factored out of it:
// with the body in a function of its own the compiler allocates the registers of ddmpc_box_step_kernel differently and its
// default instantiation measured 1.2 % slower than before on [0, 2] at 4096 instances (outside the run-to-run spread), so
// box_iterate keeps its text and the kernels without the safeguard their code.
template <bool YB>
__device__ __forceinline__ bool box_solve_set(const KParams& P, const BoxTabT<YB>& T, const double* __restrict__ Mb,
                                              double* __restrict__ Sg, const double* b0, CwlLds& s) {
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, r = P.r, nbox = T.nbox;
  // the active set in ascending order: one ballot per wave (nbox < blockDim.x: thread s looks at component s)
  const bool a = tid < nbox && s.act[tid] != 0;
  const unsigned long long mk = __ballot(a);
  if (lane == 0) s.wcnt[wave] = __popcll(mk);
  __syncthreads();
  int off = 0, k = 0;
  for (int w = 0; w < (nthr >> 6); ++w) { off += (w < wave) ? s.wcnt[w] : 0; k += s.wcnt[w]; }
  if (a) s.al[off + __popcll(mk & ((1ull << lane) - 1ull))] = tid;
  const int n0 = s.nslots;                                          // (read by all before thread 0 changes it)
  __syncthreads();
  if (tid == 0) {                                                   // LDS slots for columns that enter A for the first time
    int ns_ = n0;
    for (int i = 0; i < k && ns_ < CWL_CC; ++i) {
      const int j = box_col<YB>(T, s.al[i]);
      if (s.slot[j] < 0) { s.slot[j] = ns_; s.slotj[ns_] = j; ++ns_; }
    }
    s.nslots = ns_;
  }
  __syncthreads();
  const int n1 = s.nslots;
  for (int e = tid; e < (n1 - n0) * r; e += nthr) {                 // coalesced r-vectors
    const int sl = n0 + e / r, rho = e - (e / r) * r;
    s.Mc[sl][rho] = Mb[(long long)s.slotj[sl] * r + rho];
  }
  __syncthreads();
  // S = diag(1/d_A) - M[A,A] (lower triangle) and the right-hand side beta0[A] + M[A,A] shift_A
  double* Sp = (k <= CWL_KLDS) ? s.S : Sg;
  for (int e = tid; e < k * k; e += nthr) {
    const int i = e / k, l = e - i * k;
    if (l <= i) {
      const int ri = T.rho[s.al[i]];
      double v = -s.m(Mb, r, box_col<YB>(T, s.al[l]), ri);
      if (l == i) v += T.invd[s.al[i]];
      Sp[i * (i + 1) / 2 + l] = v;
    }
  }
  for (int i = tid; i < k; i += nthr) {
    const int ri = T.rho[s.al[i]];
    double g = b0[ri];
    for (int l = 0; l < k; ++l) g += s.m(Mb, r, box_col<YB>(T, s.al[l]), ri) * T.shift(s.al[l], s.act[s.al[l]]);
    s.ev[i] = g;
  }
  __syncthreads();
  // Cholesky, right-looking, one column per step
  for (int c = 0; c < k; ++c) {
    if (tid == 0) {
      const double pv = Sp[c * (c + 1) / 2 + c];
      if (!(pv > 0.0)) s.fail = 1; else Sp[c * (c + 1) / 2 + c] = sqrt(pv);
    }
    __syncthreads();
    if (s.fail) break;
    const double dc = Sp[c * (c + 1) / 2 + c];
    for (int i = c + 1 + tid; i < k; i += nthr) Sp[i * (i + 1) / 2 + c] /= dc;
    __syncthreads();
    const int nt = k - c - 1;
    for (int e = tid; e < nt * nt; e += nthr) {
      const int ii = e / nt, jj = e - ii * nt;
      if (jj <= ii) {
        const int i = c + 1 + ii, j = c + 1 + jj;
        Sp[i * (i + 1) / 2 + j] -= Sp[i * (i + 1) / 2 + c] * Sp[j * (j + 1) / 2 + c];
      }
    }
    __syncthreads();
  }
  if (s.fail) { if (tid == 0) s.kfin = 0; __syncthreads(); return true; }
  if (tid == 0) {                                                   // L y = g, L' x = y, ev = shift + x
    for (int i = 0; i < k; ++i) {
      double v = s.ev[i];
      for (int l = 0; l < i; ++l) v -= Sp[i * (i + 1) / 2 + l] * s.ev[l];
      s.ev[i] = v / Sp[i * (i + 1) / 2 + i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double v = s.ev[i];
      for (int l = i + 1; l < k; ++l) v -= Sp[l * (l + 1) / 2 + i] * s.ev[l];
      s.ev[i] = v / Sp[i * (i + 1) / 2 + i];
    }
    for (int i = 0; i < k; ++i) s.ev[i] += T.shift(s.al[i], s.act[s.al[i]]);
    s.kfin = k;
  }
  __syncthreads();
  for (int j = tid; j < nbox; j += nthr) s.bc[j] = box_beta<YB>(s, T, Mb, r, b0[T.rho[j]], T.rho[j]);
  return false;
}

// DDMPC_OPT_BOX_SAFEGUARD: an instance whose iteration above ended at the max_iter cap is solved again by a primal active-set
// method on the same law, M and table, by the whole workgroup.  The bounded problem is a strictly convex box QP
// in the boxed values; box_solve_set is its equality-constrained subproblem for a signed working set W.  From the empty set's
// law (not from where the iteration stopped: the result does not depend on max_iter): v = clip(hat, lo, hi), W = the violated
// components.  Per solve, with v+ = hat(W) outside W: a component that would leave the box blocks at
// alpha = (bound - v) / (v+ - v); the smallest alpha (lowest s on ties) moves v by alpha (v+ - v), and that component joins W at
// its bound.  With none blocking v = v+, and the active component with the largest g = act (bound - hat) / |c| > 0 -- a
// multiplier of the wrong sign, lowest s on ties -- is released; none: W is optimal.  The cost falls with every move, so no set
// comes back.  Status 4 at 4 nbox + 16 solves or on a non-positive pivot.  *solves = the solves; s.act / s.al / s.ev / s.kfin
// describe the result as after box_iterate (thread s owns component s: blockDim.x > nbox).
template <bool YB>
__device__ int box_safeguard(const KParams& P, const BoxTabT<YB>& T, const double* __restrict__ Mb, double* __restrict__ Sg,
                             const double* b0, CwlLds& s, BoxSafeLds& q, int* solves) {
  const int tid = threadIdx.x, nbox = T.nbox, cap = 4 * nbox + 16;
  const bool own = tid < nbox;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  __syncthreads();                                                    // (everyone has read what box_iterate left)
  if (own) {
    const double beta = b0[T.rho[tid]];
    const int act = T.test(tid, beta, 0);
    s.act[tid] = (signed char)act;
    q.v[tid] = act ? T.bound(tid, act) : fma(T.c[tid], beta, T.a[tid]);
  }
  if (tid == 0) s.kfin = 0;
  int n = 0, st = 0;
  for (;;) {
    __syncthreads();
    if (n >= cap) { st = 4; break; }
    ++n;
    if (box_solve_set<YB>(P, T, Mb, Sg, b0, s)) { st = 4; break; }
    __syncthreads();
    const int act = own ? s.act[tid] : 0;
    const double hat = own ? fma(T.c[tid], s.bc[tid], T.a[tid]) : 0.0;
    const double vj = own ? q.v[tid] : 0.0;
    const int side = (own && act == 0) ? (hat > T.hi[tid]) - (hat < T.lo[tid]) : 0;
    double key = inf;
    int idx = BOX_NONE;
    if (side != 0) { key = fmax((T.bound(tid, side) - vj) / (hat - vj), 0.0); idx = tid; }
    box_argmin(key, idx, q);
    if (idx != BOX_NONE) {                                             // a blocking component: partial step, it joins W
      if (tid == idx) { s.act[tid] = (signed char)side; q.v[tid] = T.bound(tid, side); }
      else if (own && act == 0) q.v[tid] = fma(key, hat - vj, vj);
      continue;
    }
    if (own && act == 0) q.v[tid] = hat;
    key = inf;
    if (act != 0) {
      const double g = act * (T.bound(tid, act) - hat) / fabs(T.c[tid]);
      if (g > 0.0) { key = -g; idx = tid; }
    }
    box_argmin(key, idx, q);
    if (idx == BOX_NONE) break;                                        // every multiplier has the right sign
    if (tid == idx) s.act[tid] = 0;                                   // (v stays at the bound it leaves)
  }
  *solves = n;
  return st;
}

// DDMPC_OPT_BOX_WARM_START: the iteration from the signed set the last solve of the handle ended with, in the
// WARM instantiations of the box kernels only.  Called like box_iterate, after the law violated the box under the empty set,
// with the seed in s.act (settled by a barrier).  An empty seed: box_iterate as it is.  Otherwise the seed is solved for --
// solve number 2 -- and the test / solve loop of box_iterate goes on from there under the same cap (box_solve_set is that
// loop's body; BoxTab::test releases an active component whose multiplier has the wrong sign).  A seeded run that meets a
// non-positive pivot (K(A) is positive definite for every set, so that is the seed's doing) or ends at the cap starts again
// from the empty set with a fresh cap: box_iterate as it is, so the status is never worse than without the seed.  With SAFE a
// seeded run at the cap returns 4 with s.fail = 0 instead, and the caller goes to box_safeguard (which starts from the empty
// set's law: its result does not depend on the seed).  *iters = every solve made, the law counted once.
template <bool SAFE, bool YB>
__device__ int box_iterate_seeded(const KParams& P, const BoxTabT<YB>& T, const double* __restrict__ Mb, double* __restrict__ Sg,
                                  const double* b0, CwlLds& s, int* iters) {
  const int tid = threadIdx.x, nthr = blockDim.x, nbox = T.nbox;
  int any = 0;
  for (int j = tid; j < nbox; j += nthr) any |= s.act[j] != 0;
  int spent = 0;                                                      // solves of a seeded run that is given up
  if (__syncthreads_or(any)) {
    for (int j = tid; j < nbox; j += nthr) { s.bc[j] = b0[T.rho[j]]; s.slot[j] = -1; }
    if (tid == 0) { s.kfin = 0; s.fail = 0; s.nslots = 0; }
    __syncthreads();
    int iter = 1;
    bool done = false;
    for (;;) {
      if (iter >= P.max_iter) break;                                  // the cap
      ++iter;
      if (box_solve_set<YB>(P, T, Mb, Sg, b0, s)) break;              // a pivot
      if (tid == 0) s.changed = 0;
      __syncthreads();
      for (int j = tid; j < nbox; j += nthr) {
        const int ns = T.test(j, s.bc[j], s.act[j]);
        if (ns != s.act[j]) { s.act[j] = (signed char)ns; s.changed = 1; }
      }
      __syncthreads();
      if (!s.changed) { done = true; break; }
    }
    if (done) { *iters = iter; return 0; }
    if (SAFE && !s.fail) { *iters = iter; return 4; }
    spent = iter - 1;
    __syncthreads();                                                  // (everyone has read what the seeded run left)
  }
  int it;
  const int st = box_iterate<YB>(P, T, Mb, Sg, b0, s, &it);
  *iters = spent + it;
  return st;
}

// The seed, or the per-instance channel table, as a kernel argument.  The box kernels take it as a trailing parameter pack: empty
// in the instantiations launched with shared bounds and the option 0, whose signature, kernel arguments and code are then those of
// the kernels without either; one BoxSeed in the WARM ones, one BoxChannels in the INST ones (never both: DDMPC_OPT_BOX_WARM_START
// is not honoured on a handle with per-instance bounds).
struct BoxSeed {
  signed char* ws;            // [batch][nbox]: the signed set every instance's last solve ended with; written by every WARM launch
  int use;                    // 0: `ws` is not read (nothing valid in it) and every instance starts from the empty set
};
struct BoxChannels {
  const double* chb;          // [batch][lo (nch) | hi (nch)]: the bounds of every instance by channel (see the head of this file)
};
__device__ __forceinline__ BoxSeed box_seed_of() { return BoxSeed{nullptr, 0}; }
__device__ __forceinline__ BoxSeed box_seed_of(BoxSeed s) { return s; }
__device__ __forceinline__ BoxSeed box_seed_of(BoxChannels) { return BoxSeed{nullptr, 0}; }
__device__ __forceinline__ BoxChannels box_channels_of() { return BoxChannels{nullptr}; }
__device__ __forceinline__ BoxChannels box_channels_of(BoxSeed) { return BoxChannels{nullptr}; }
__device__ __forceinline__ BoxChannels box_channels_of(BoxChannels c) { return c; }

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

// Output stage of one component with its active flag (j: its place in the box list, or -1): cwl_component, and an input row
// held at a bound is that bound exactly (t = bound, D1 = 0); its cost term is the K_UFREE one.
__device__ __forceinline__ double box_component(const KParams& P, int RPs, const BoxTab& T, int rho, int j, double beta, int sa,
                                                const double* pv, double* z_out) {
  const int kind = P.tabi[0 * RPs + rho];
  const int pidx = P.tabi[1 * RPs + rho];
  const double D = sa ? P.tabd[1 * RPs + rho] : P.tabd[0 * RPs + rho];
  const double tb = P.tabd[2 * RPs + rho];
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

// ... of a K_WPRED row whose output component jy is held at its bound (say != 0; sa: its slack): ybar is that bound exactly,
// sigma = z - bound with the row's weight lamb_sigma, or +- c eps_max with both active (the row is hard).
__device__ __forceinline__ double box_component_y(const KParams& P, int RPs, const BoxTab& T, int rho, int jy, double beta, int sa,
                                                  int say, double* z_out) {
  const double tb = P.tabd[2 * RPs + rho];
  const double wq = P.tabd[3 * RPs + rho];
  const double yb = T.bound(jy, say);
  const double sg = (sa != 0) ? sa * P.bound : -P.lam * beta / P.lamb_sigma;
  const double z = yb + sg;
  const double dlt = yb - tb;
  *z_out = z;
  return P.lam * beta * z + wq * dlt * dlt + P.lamb_sigma * sg * sg;
}

// One control step of a bounded handle for the batch: grid = batch, block = r rounded up to 64 (the geometry of
// ddmpc_warm_step_kernel): law, violation test with the table, iteration, M_A ev correction, outputs.  Mcol [batch][nbox][r],
// sg [batch][nbox (nbox + 1) / 2] (used for k > CWL_KLDS only).  No cold hand-over: no cold kernel serves these handles.
// `refined` (may be null): instances whose law came from refining solves (ddmpc_prepare, AUTO); their M is the unrefined
// factor's, so a solve of theirs that ends with a non-empty active set is reported optimal_inaccurate.
// SAFE (DDMPC_OPT_BOX_SAFEGUARD = 1): an instance that ends at the max_iter cap is finished by box_safeguard; iters = max_iter +
// its solves.  The host launches <false> when the option is 0: that instantiation is the kernel as it was.
// YB (ddmpc_set_output_bounds): the table with the output components; block = max(r, nbox) rounded up to 64; the active-set
// workspace holds sa + 4 say per row (sa: slack or input, say: output).  Without YB the kernel is the one it was.
// Extra = BoxSeed (DDMPC_OPT_BOX_WARM_START = 1, "WARM"): box_iterate_seeded from the set in seed.ws when seed.use, and the set this
// solve ended with goes there (empty when nothing was iterated or the solve failed).  The host launches the empty pack when the
// option is 0: that instantiation is the kernel as it was.
// Extra = BoxChannels (per-instance bounds, "INST"): the same stages, statuses and iters with the instance's own bounds -- blo, bhi
// [WARM_MAX_R] in LDS (nbox <= WARM_MAX_R is checked by ddmpc_prepare), filled before the law, behind the table's lo / hi.
template <bool SAFE, bool YB, class... Extra>
__global__ void ddmpc_box_step_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                      const int* __restrict__ prep_status, const double* __restrict__ u_past,
                                      const double* __restrict__ y_past, double* __restrict__ u_opt, double* __restrict__ cost,
                                      int* __restrict__ status, int* __restrict__ iters, double* __restrict__ beta_ws,
                                      signed char* __restrict__ act_ws, int nbox, const int* __restrict__ tab,
                                      const double* __restrict__ bd, const double* __restrict__ Mcol, double* __restrict__ sg,
                                      const int* __restrict__ refined, Extra... extra) {
  constexpr bool WARM = (std::is_same_v<Extra, BoxSeed> || ...);
  constexpr bool INST = (std::is_same_v<Extra, BoxChannels> || ...);
  [[maybe_unused]] const BoxSeed seed = box_seed_of(extra...);
  [[maybe_unused]] const BoxChannels chan = box_channels_of(extra...);
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double red[32];
  __shared__ double bsh[WARM_MAX_R];
  __shared__ CwlLds s;
  const int r = P.r;
  BoxTabT<YB> T = box_table<YB>(nbox, tab, bd, r);
  const long long b = blockIdx.x;
  const int tid = threadIdx.x, nrhs = nf + 1;
  const int nyp = nf - P.npu;
  for (int f = tid; f < nf; f += blockDim.x)
    pv[f] = (f < P.npu) ? u_past[b * P.npu + f] : y_past[b * nyp + (f - P.npu)];
  if constexpr (INST) {
    __shared__ double blo[WARM_MAX_R];                // the bounds of this instance, by boxed component
    __shared__ double bhi[WARM_MAX_R];
    instance_box_fill<YB>(P, T, chan.chb + b * (long long)(2 * P.nch), blo, bhi);
    T.lo = blo;
    T.hi = bhi;
  }
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
    int dst;
    if constexpr (WARM) {
      for (int j = tid; j < nbox; j += blockDim.x) s.act[j] = seed.use ? seed.ws[b * nbox + j] : (signed char)0;
      __syncthreads();
      dst = box_iterate_seeded<SAFE, YB>(P, T, Mb, Sg, bsh, s, &it);
    } else {
      dst = box_iterate<YB>(P, T, Mb, Sg, bsh, s, &it);
    }
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
  if constexpr (WARM) {                                // the seed of the handle's next step: the set this solve ended with
    if (tid == 0) s.changed = iterate && st <= 1;      // (empty without an iteration and behind a failed solve)
    __syncthreads();
    const bool keep = s.changed != 0;
    for (int j = tid; j < nbox; j += blockDim.x) seed.ws[b * nbox + j] = keep ? s.act[j] : (signed char)0;
  }
}

// Whole closed loop of one instance of a bounded handle in one workgroup: the twin of ddmpc_closed_loop_convex_warm_kernel
// (same fixed-size arrays and the same checks of ddmpc_closed_loop behind them).  Per solve the law on the boxed rows and the
// n_mpc_step * m input rows in use, the iteration of ddmpc_box_step_kernel, the M_A ev correction of those rows, then the
// plant / FIFO steps of ddmpc_plant_kernel; everything on the last solve.  SAFE: as in ddmpc_box_step_kernel; an instance the
// safeguard finishes carries on with the loop.  YB: as in ddmpc_box_step_kernel.  Extra = BoxSeed: the set stays in s.act from one
// solve of the loop to the next; the first solve takes the handle's seed when seed.use, the last one leaves its set in seed.ws.
// Extra = BoxChannels: as in ddmpc_box_step_kernel; blo / bhi are filled once, before the first solve.
template <bool SAFE, bool YB, class... Extra>
__global__ void ddmpc_closed_loop_box_kernel(KParams P, int RPs, int nf, const double* __restrict__ gain,
                                             const int* __restrict__ prep_status, int ns, const double* __restrict__ pl,
                                             int n_steps, int n_mpc_step, double* __restrict__ x, double* __restrict__ u_past,
                                             double* __restrict__ y_past, const double* __restrict__ w, double* __restrict__ u_sys,
                                             double* __restrict__ y_sys, int* __restrict__ status_out, double* __restrict__ beta_ws,
                                             signed char* __restrict__ act_ws, int nbox, const int* __restrict__ tab,
                                             const double* __restrict__ bd, const double* __restrict__ Mcol, double* __restrict__ sg,
                                             const int* __restrict__ refined, double* __restrict__ lw_up, double* __restrict__ lw_yp,
                                             Extra... extra) {
  constexpr bool WARM = (std::is_same_v<Extra, BoxSeed> || ...);
  constexpr bool INST = (std::is_same_v<Extra, BoxChannels> || ...);
  [[maybe_unused]] const BoxSeed seed = box_seed_of(extra...);
  [[maybe_unused]] const BoxChannels chan = box_channels_of(extra...);
  __shared__ double pv[WARM_MAX_NF];
  __shared__ double uo[WARM_MAX_NF];      // the first n_mpc_step*m entries of optimal_u
  __shared__ double xs[16], xn[16];       // (ns <= 16 is checked by ddmpc_closed_loop)
  __shared__ double bsh[WARM_MAX_R];
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
  if constexpr (INST) {                               // (visible behind the barrier that opens the first solve)
    __shared__ double blo[WARM_MAX_R];                // the bounds of this instance, by boxed component
    __shared__ double bhi[WARM_MAX_R];
    instance_box_fill<YB>(P, T, chan.chb + b * (long long)(2 * P.nch), blo, bhi);
    T.lo = blo;
    T.hi = bhi;
  }
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
  if constexpr (WARM)                                 // the seed stays in s.act from one solve of the loop to the next
    for (int j = tid; j < nbox; j += blockDim.x) s.act[j] = seed.use ? seed.ws[b * nbox + j] : (signed char)0;
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
      int dst;
      if constexpr (WARM) dst = box_iterate_seeded<SAFE, YB>(P, T, Mb, Sg, bsh, s, &it);
      else dst = box_iterate<YB>(P, T, Mb, Sg, bsh, s, &it);
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
    if constexpr (WARM)                               // (an empty seed without an iteration and behind a failed solve)
      if (!iterate || st > 1)
        for (int j = tid; j < nbox; j += blockDim.x) s.act[j] = 0;
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
        for (int i = 0; i < p; ++i) yp[(n - 1) * p + i] = ys[i];      // (p is not bounded: no private copy of y)
      }
    }
  }
  __syncthreads();
  for (int f = tid; f < nf; f += blockDim.x) {
    if (f < P.npu) u_past[b * P.npu + f] = pv[f]; else y_past[b * nyp + (f - P.npu)] = pv[f];
  }
  if (tid < ns) x[b * ns + tid] = xs[tid];
  if (tid == 0) status_out[b] = stc;
  if constexpr (WARM)
    for (int j = tid; j < nbox; j += blockDim.x) seed.ws[b * nbox + j] = s.act[j];
}

}  // namespace ddmpc
