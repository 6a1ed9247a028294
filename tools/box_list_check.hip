// Host check of build_box_list and build_large_box (ddmpc_api.hip) under the address and undefined-behaviour sanitizers: no
// device is used.
//
//   python -m direct_data_driven_mpc_amd.build
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xarch_host -fsanitize=address,undefined -Idirect_data_driven_mpc_amd/csrc \
//         -c tools/box_list_check.hip -o tools/box_list_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined tools/box_list_check.o direct_data_driven_mpc_amd/_build/ddmpc_inst*.o \
//         -o tools/box_list_check && tools/box_list_check
//
// A 22-row (m = p = 1, L = 10, n = 1) and a 136-row (m = p = 2, L = 30, n = 4) table with the terminal constraint, with and
// without the CONVEX slack box, without input bounds, with one channel bounded and with all of them, each without output bounds
// and with every output channel bounded (two components on a predicted output row under the slack box, one column of M per
// boxed row).  The vectors have exactly the sizes ddmpc_prepare passes, so a read or write past them is reported.  Every case
// also goes through build_large_box (the "boxed last" order and the component table of the phase kernels beyond 271 rows):
// a permutation with its inverse, nA and the component count, positions ascending with the slack before the output on a row.
#include "../direct_data_driven_mpc_amd/csrc/ddmpc_api.hip"

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const int shapes[2][4] = {{1, 11, 1, 2}, {2, 34, 4, 9}};     // m (= p), L + n, n, tile rows NT
  int bad = 0;
  for (const auto& sh : shapes)
    for (int convex = 0; convex < 2; ++convex)
      for (int bounded = 0; bounded <= sh[0]; bounded += std::max(1, sh[0] - 1))     // channels with a finite bound: 0, 1, all
      for (int ybounded = 0; ybounded < 2; ++ybounded) {                             // output channels with one: none, all
        const int m = sh[0], nch = 2 * m, Ln = sh[1], n = sh[2], RP = 16 * sh[3], nfree = Ln - 2 * n;
        KParams k{};
        k.nch = nch; k.r = nch * Ln; k.convex = convex; k.lam = 0.04; k.sig_scale = -8e-5; k.bound = 0.002;
        std::vector<int> ti(3 * (size_t)RP, K_UFIX);
        std::vector<double> td(4 * (size_t)RP, 0.0);
        for (int rho = 0; rho < k.r; ++rho) {
          const int step = rho / nch, ch = rho % nch;
          const bool pred = step >= n, term = step >= Ln - n;
          ti[rho] = ch < m ? (pred && !term ? K_UFREE : K_UFIX) : (!pred ? K_WINT : term ? K_WTERM : K_WPRED);
          td[rho] = 2.0 + ch; td[RP + rho] = 0.5; td[2 * RP + rho] = 1.0;
        }
        std::vector<double> lo(m, -inf), hi(m, inf);
        for (int ch = 0; ch < bounded; ++ch) { lo[ch] = -4.0; hi[ch] = 6.0; }
        k.m = m;
        std::vector<double> ylo(m, 0.5), yhi(m, 1.5);
        const double* ul = bounded ? lo.data() : nullptr;
        const double* uh = bounded ? hi.data() : nullptr;
        const BoxList bl = ybounded ? build_box_list(k, RP, ti, td, ul, uh, ylo.data(), yhi.data())
                         : bounded ? build_box_list(k, RP, ti, td, ul, uh)
                                   : build_box_list(k, RP, ti, std::vector<double>(), nullptr, nullptr);
        const int want = (convex ? m * (Ln - n) : 0) + bounded * nfree + ybounded * m * nfree;
        const int wcol = (convex ? m * (Ln - n) : ybounded * m * nfree) + bounded * nfree;
        const bool bd = bounded || ybounded;
        bool ok = bl.nbox == want && bl.ncol == wcol && bl.bd.size() == (bd ? 5 * (size_t)want : 0) &&
                  bl.tab.size() == (ybounded ? 2 * (size_t)(want + k.r) + 1 + wcol : (size_t)(want + k.r));
        for (int s = 0; ok && s < bl.nbox; ++s) {
          const int rho = bl.tab[s];
          ok = (s == 0 || rho >= bl.tab[s - 1]) && (!bd || std::isfinite(bl.bd[4 * want + s]));
          if (!ybounded) { ok = ok && bl.tab[bl.nbox + rho] == s && (s == 0 || rho > bl.tab[s - 1]); continue; }
          const int* col = bl.tab.data() + want + k.r;
          const int* ofy = col + want;
          const int* crho = ofy + k.r + 1;
          ok = ok && ofy[k.r] == wcol && col[s] >= 0 && col[s] < wcol && crho[col[s]] == rho &&
               (bl.tab[bl.nbox + rho] == s || ofy[rho] == s) && (bl.tab[bl.nbox + rho] < 0 || ofy[rho] < 0 || ofy[rho] == bl.tab[bl.nbox + rho] + 1);
        }
        printf("%3d rows  convex %d  bounded channels %d  outputs %d: nbox %3d (want %3d) columns %3d (want %3d) %s\n", k.r, convex, bounded,
               ybounded, bl.nbox, want, bl.ncol, wcol, ok ? "ok" : "BAD");
        bad += !ok;
        // the same tables through build_large_box: the order "boxed last" and the component table of the phase kernels
        // beyond 271 rows (the builder does not look at the row count)
        k.p = m;
        const LargeBox lb = build_large_box(k, RP, ti, td, ul, uh, ybounded ? ylo.data() : nullptr, ybounded ? yhi.data() : nullptr);
        const int rv = (k.r + 1) & ~1;
        int rows = 0;
        for (int rho = 0; rho < k.r; ++rho)
          rows += (convex && (ti[rho] == K_WPRED || ti[rho] == K_WTERM)) || (ti[rho] == K_UFREE && rho % nch < bounded) ||
                  (ybounded && ti[rho] == K_WPRED);
        const int lwant = bd ? want : 0;
        bool lok = lb.nA == k.r - rows && lb.nbox == lwant && lb.pm.size() == 2 * (size_t)rv && lb.ip.size() == 2 * (size_t)lwant &&
                   lb.bd.size() == (bd ? (size_t)R3B_NV * lwant + 4 * (size_t)m : 0);
        std::vector<int> seen((size_t)k.r, 0);
        for (int i = 0; lok && i < k.r; ++i) {
          const int rho = lb.pm[i];
          lok = rho >= 0 && rho < k.r && !seen[rho]++ && lb.pm[rv + rho] == i;
        }
        for (int s = 0; lok && s < lb.nbox; ++s) {
          const int i = lb.ip[s], isy = lb.ip[lb.nbox + s];
          lok = i >= lb.nA && i < k.r && (s == 0 || i > lb.ip[s - 1] || (i == lb.ip[s - 1] && isy && !lb.ip[lb.nbox + s - 1])) &&
                std::isfinite(lb.bd[(size_t)R3B_INVD * lb.nbox + s]) && lb.bd[(size_t)R3B_INVD * lb.nbox + s] > 0.0 &&
                (!isy || ti[lb.pm[i]] == K_WPRED);
        }
        printf("          boxed last: nA %3d (want %3d) components %3d (want %3d) %s\n", lb.nA, k.r - rows, lb.nbox, lwant, lok ? "ok" : "BAD");
        bad += !lok;
      }
  return bad != 0;
}
