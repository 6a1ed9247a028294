// ddmpc_api.hip -- C ABI (include/ddmpc.h) over the gfx950 kernels in ddmpc_cold2.hpp, ddmpc_aux_kernels.hpp, ddmpc_box_law.hpp, ddmpc_setpoint_law.hpp, ddmpc_setpoint_box_law.hpp, ddmpc_workspace_kernels.hpp and the phase pipelines (ddmpc_rr2*.hpp, ddmpc_rr3.hpp, ddmpc_rr3_box.hpp).
// Host-side responsibilities: parameter validation with the reference's error
// conditions (direct_data_driven_mpc_controller.py:165-168,211-222,298-343,664-670),
// device buffer ownership, kernel-instance selection, launch.
#include "ddmpc_rr3_law.hpp"
#include "ddmpc_rr3_box_law.hpp"
#include "ddmpc_rr3_box.hpp"
#include "ddmpc_rr3_box_wide.hpp"
#include "ddmpc_rr3_box_safe.hpp"
#include "ddmpc_box_law.hpp"
#include "ddmpc_setpoint_law.hpp"
#include "ddmpc_setpoint_box_law.hpp"
#include "../../include/ddmpc.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace ddmpc;

// The kernels are instantiated in their own translation units (ddmpc_inst.hip).
namespace ddmpc {
#define DDMPC_INSTANCE(NT, W)                                                                              \
  extern template __global__ void ddmpc_cold_solve_kernel2<NT, W, false>(                                  \
      KParams, const double*, const double*, const double*, const double*, double*, double*, int*,        \
      int*, double*, signed char*, unsigned long long*, double*, double*, int*, const int*, long long, int*);   \
  extern template __global__ void ddmpc_cold_solve_kernel2<NT, W, true>(                                   \
      KParams, const double*, const double*, const double*, const double*, double*, double*, int*,        \
      int*, double*, signed char*, unsigned long long*, double*, double*, int*, const int*, long long, int*);   \
  extern template __global__ void ddmpc_cold_solve_kernel2<NT, W, false, true>(                            \
      KParams, const double*, const double*, const double*, const double*, double*, double*, int*,        \
      int*, double*, signed char*, unsigned long long*, double*, double*, int*, const int*, long long, int*);
#include "ddmpc_instances.inc"
#undef DDMPC_INSTANCE
}  // namespace ddmpc

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e__ = (expr);                                                            \
    if (e__ != hipSuccess)                                                              \
      return fail(DDMPC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                  __FILE__, __LINE__);                                                  \
  } while (0)

static int g_poison_byte = 0;      // ddmpc_debug_poison_allocations

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return DDMPC_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    HIP_TRY(hipMalloc(&p, need));
    bytes = need;
    // debugging aid (ddmpc_debug_poison_allocations): every fresh device buffer pre-filled with a byte pattern, so that a read
    // of something no kernel has written shows up in the results of one run instead of depending on what the allocator handed back
    if (g_poison_byte) HIP_TRY(hipMemset(p, g_poison_byte, need));
    return DDMPC_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct HostBuf {            // pinned host staging
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return DDMPC_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    HIP_TRY(hipHostMalloc(&p, need, hipHostMallocDefault));
    bytes = need;
    return DDMPC_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

typedef void (*cold_kernel2_t)(KParams, const double*, const double*, const double*, const double*, double*,
                               double*, int*, int*, double*, signed char*, unsigned long long*, double*, double*, int*, const int*, long long, int*);

struct KernelChoice {
  int NT, W;
  cold_kernel2_t fn2;        // cold-solve kernel (ddmpc_cold2.hpp)
  const char* name2;
  cold_kernel2_t fn2r;       // the same with the iterative-refinement loop compiled in
  cold_kernel2_t fn2c;       // the plain kernel with the rank-k treatment of the slack box (CONVEX controllers)
  int lds_fixed;             // Lds2<NT, W>::xs: doubles in front of the trajectory region
  int max_past;              // Lds2Limits: entries of [u_past; y_past] the prologue staging holds
  int scratch;               // Lds2Limits: doubles free for the residual check of AUTO refinement
};

// Instantiated (tile rows, waves) pairs.  A problem uses the smallest NT that
// holds rE+1 rows; larger problems are rejected as unsupported.
const KernelChoice kKernels[] = {
#define DDMPC_INSTANCE(NT, W) \
  {NT, W, &ddmpc_cold_solve_kernel2<NT, W, false>, "ddmpc_cold_solve_kernel2<" #NT "," #W ">", &ddmpc_cold_solve_kernel2<NT, W, true>, \
   &ddmpc_cold_solve_kernel2<NT, W, false, true>, Lds2<NT, W>::xs, Lds2Limits<NT, W>::max_past, Lds2Limits<NT, W>::scratch},
#include "ddmpc_instances.inc"
#undef DDMPC_INSTANCE
};

// Dynamic LDS beyond 64 KB is a per-function limit that has to be raised before the launch.  The limit is a property of the
// function, not of a handle: it is only ever RAISED here (a second controller with a smaller footprint must not lower it under
// the first one's launches), per device, behind a lock.
static hipError_t raise_lds_limit(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> limit;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  size_t& cur = limit[std::make_pair(fn, dev)];
  if (bytes <= cur) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}

// LDS doubles of a launch: the compile-time carve-up of the instance (Lds2<NT, W>::total) -- the same struct the kernel
// takes its offsets from.
size_t lds_doubles_for(const KernelChoice& kc, int xs_len) { return ((size_t)kc.lds_fixed + (size_t)xs_len + 1) & ~(size_t)1; }

}  // namespace

// The implementation that serves a handle's solves (select_route).
enum class Route {
  Cold,             // the register-resident cold kernels (trajectories beyond the LDS included) + the NOMINAL rescue kernel
  RobustPhases,     // ROBUST beyond the register-resident kernels: the phase kernels (ddmpc_rr3.hpp)
  RobustOneWg,      // ... the one-workgroup kernel (ddmpc_large_solve_kernel)
  NominalPhases,    // NOMINAL beyond the register-resident kernels: the phase kernels (ddmpc_rr2*.hpp)
  NominalOneWg,     // ... the one-workgroup kernel (ddmpc_nominal_rr_kernel)
  BoxLaw,           // ROBUST with input bounds (ddmpc_set_input_bounds), register-resident sizes: the active-set iteration on the
                    // law and M = K0^-1 E_box (ddmpc_box_law.hpp); the cold kernels serve its preparation only
};

// What steps the plant in a ddmpc_closed_loop (select_loop_path): one fused launch, or per control step a solve and
// ddmpc_plant_kernel.  kLoopKernel is what ddmpc_closed_loop_kernel_name reports.
enum class LoopPath {
  FusedAffine,      // affine law, no inequality: the whole loop of an instance inside one workgroup
  FusedConvex,      // ... with the slack box on the law (DDMPC_OPT_CONVEX_WARM_LAW, no refined law)
  FusedBox,         // ... with input bounds (Route::BoxLaw)
  StepPrepared,     // per step, step_on_route on what ddmpc_prepare kept
  SolvePerStep,     // per step, solve_on_route
};
static const char* const kLoopKernel[] = {"ddmpc_closed_loop_warm_kernel", "ddmpc_closed_loop_convex_warm_kernel",
                                          "ddmpc_closed_loop_box_kernel", "ddmpc_plant_kernel", "ddmpc_plant_kernel"};
static bool fused(LoopPath p) { return p == LoopPath::FusedAffine || p == LoopPath::FusedConvex || p == LoopPath::FusedBox; }

// What a launch of the global-workspace routes does: the whole solve, the data-dependent factors alone (ddmpc_prepare), or a
// solve on the factors ddmpc_prepare kept (ddmpc_step).  The values are the template argument of the one-workgroup kernels.
enum class Stage { Solve = 0, Factors = 1, OnFactors = 2 };

// What ddmpc_get_solution may read: the record of the last call that wrote solve outputs (ddmpc_solve, ddmpc_solve_from_host,
// ddmpc_step, ddmpc_closed_loop).  Each of them sets it whole (begin_solve ... end_solve); ddmpc_get_solution makes it current.
enum class BetaState {
  Written,          // beta / active set of the last solve are in the workspace
  ReSolveCold,      // a cold solve skipped them: solve once more at the same past window
  ReEvalLaw,        // a warm step skipped them: evaluate the affine law once more
};
enum class XState {
  Written,          // x = L^-T w of the NOMINAL rescue is in the workspace (or not needed)
  FromW,            // ... is still to be formed from the final w the phase solve kept
  ReSolveOnFactors, // a step on the NOMINAL affine law kept no w: solve once more on the route's factors
};
struct LastSolve {
  bool valid = false;
  Route route = Route::Cold;               // the route that served it (Cold until the first solve)
  const double *up = nullptr, *yp = nullptr;   // the past window of the reconstruction and of any re-solve
  BetaState beta = BetaState::Written;
  bool rescue = false;                     // z / x / flags of the NOMINAL rescue kernel are current
  XState x = XState::Written;
  int box_cap = RR3_KMAX;                  // Route::RobustPhases: columns of W of the kernel that wrote the per-instance record (its layout)
  bool box_seed = false;                   // Route::BoxLaw, DDMPC_OPT_BOX_WARM_START: d_box_seed holds the signed set that solve ended with
  bool large_seed = false;                 // Route::RobustPhases, DDMPC_OPT_LARGE_BOX_WARM_START: d_large_seed holds the set that solve ended with
  bool setpoint_call = false;              // not valid because ddmpc_step_setpoints / ddmpc_closed_loop_setpoints ran last (the message of ddmpc_get_solution)
};

// What ddmpc_prepare kept; it serves the route it was formed on only (prep_valid).
struct Prep {
  bool valid = false;
  Route route = Route::Cold;
  bool law = false;                        // beyond 271 rows: the affine law was formed (DDMPC_OPT_LARGE_AFFINE_LAW, DDMPC_OPT_LARGE_BOX_LAW)
  int r3_nolaw = 0;                        // ... ROBUST: instances whose law missed the refinement threshold (their steps take the filtered re-solve)
  int r3_nosp = 0;                         // ... DDMPC_OPT_LARGE_SETPOINTS: instances whose S missed it (their setpoint steps take the filtered re-solve)
  int cwl_nbox = 0;                        // DDMPC_OPT_CONVEX_WARM_LAW, Route::BoxLaw: boxed components
  int box_threads = 0;                     // Route::BoxLaw: block of the box kernels (max(r, nbox) rounded up to 64)
  int cwl_nref = 0;                        // ... instances whose law came from refining solves (their steps keep the filtered cold launch;
                                           //     BoxLaw: they iterate like the others and report optimal_inaccurate with a non-empty active set)
  int epoch = 0;                           // stamp of the flags recorded by the factor-export launch (AUTO)
  bool setpoint = false;                   // DDMPC_OPT_SETPOINT_LAW / _SETPOINT_BOX_LAW / _SETPOINT_CONVEX_LAW: S was formed next to the law (d_sgain)
};

struct ddmpc_handle {
  ddmpc_params prm{};
  std::vector<double> Qh, Rh, us_h, ys_h;
  int64_t batch = 0;
  int device = 0;
  KParams kp{};
  KernelChoice kc{};
  size_t lds_bytes = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t copy_stream = nullptr;      // uploads of ddmpc_solve_from_host, overlapped with the solves on `stream`
  bool have_data = false;
  LastSolve last;
  Prep prep;
  // parameter tables on device
  DevBuf d_tabd, d_tabi, d_dmat;
  // data (owned copies when the caller passed host memory)
  DevBuf d_ud, d_yd;
  const double* ud = nullptr;
  const double* yd = nullptr;
  // staging for host-memory solves + workspace for get_solution
  DevBuf d_up, d_yp, d_uopt, d_cost, d_status, d_iters, d_beta, d_act, d_out, d_stamps;
  DevBuf d_pl, d_x, d_w, d_usys, d_ysys, d_stacc;
  DevBuf d_lwup, d_lwyp;                   // ddmpc_closed_loop: the past window of the loop's last solve (what ddmpc_get_solution reads)
  // warm path: per-instance affine law (ddmpc_prepare)
  DevBuf d_lfac, d_lfacT, d_gain, d_prep_status, d_zero, d_need;
  // host-pointer solves: one packed device buffer and its pinned host mirror (two copies per solve instead of six)
  DevBuf d_io, d_rr, d_alpha;
  DevBuf d_rflag;                          // AUTO refinement: per-instance "refine me" flags of the plain cold kernel
  DevBuf d_zws, d_resc, d_xws;             // NOMINAL rescue kernel: z per component, a per-instance "rescued" flag and x = L^-T w (ddmpc_get_solution)
  DevBuf d_rrmeta;                         // ... pivot pattern + live column counts of the factors it leaves in d_rr (2 rv + 2 ints per instance)
  DevBuf d_rr2v, d_rr2zp, d_rr2sc, d_wz;   // ... vectors, Hankel partial sums and scalars of the solve (ddmpc_rr2_solve.hpp); weights / targets
  DevBuf d_gz, d_gres, d_zvirt;            // ... the affine law z(past) and the residuals of the dependent fixed rows (DDMPC_OPT_LARGE_AFFINE_LAW)
  int large_affine = 0;                    // DDMPC_OPT_LARGE_AFFINE_LAW
  DevBuf d_rr2mt;                          // ... Minv of every 64 x 64 diagonal block of the two factors (ddmpc_rr2.hpp)
  DevBuf d_rr3w, d_rr3k, d_rr_fb, d_rrmeta_fb;   // ROBUST beyond 271 rows on the phase kernels (ddmpc_rr3.hpp): W + the k x k factor, the per-instance
                                          // ints; workspace / record of the fall-back (ddmpc_large_solve_kernel on instances marked 5)
  int nA3 = 0;                            // ... first position of the boxed components (slack box, bounded inputs / outputs) in the "boxed last" order
  int nbox3 = 0;                          // ... bounded handles: components of the box table (Rr3Box)
  int large_bounds = 0;                   // DDMPC_OPT_LARGE_BOUNDS: ddmpc_set_input_bounds / ddmpc_set_output_bounds are accepted beyond 271 rows
  int large_box_cap = RR3_KMAX;           // DDMPC_OPT_LARGE_BOX_CAPACITY: columns of W per instance of a bounded handle (64: rr3_solve_box_kernel)
  int large_box_safeguard = 0;            // DDMPC_OPT_LARGE_BOX_SAFEGUARD: rr3_box_safeguard_kernel behind the solve launch of the wide kernels
  DevBuf d_r3bi, d_r3bd;                  // ... [position | output?] and [a | c | lo | hi | 1/d | shlo | shhi | bounds per channel] of that table
  std::vector<int> ti_h;                  // the parameter tables of upload_params on the host (the order and the box table are
  std::vector<double> td_h;               //   rebuilt from them when the bounds change)
  DevBuf d_r3y, d_r3res, d_r3zp, d_r3flag; // ... DDMPC_OPT_LARGE_AFFINE_LAW (ddmpc_rr3_law.hpp; the law itself in d_gz): substitution
                                          //   vectors, residuals and Hankel sums of a chunk of instances; [no law | re-solve | refine] flags,
                                          //   then the re-solve flags again as Rr2Solve::si (2 ints per instance)
  DevBuf d_gpre;                          // Gram tiles of ddmpc_gram_tiles_kernel (structured Gram, m + p != 4), see gram_pre_launch
  bool gram_pre = false, gpre_valid = false;
  int gram_launch = 0;                     // DDMPC_OPT_GRAM_LAUNCH: 0 streaming matrix-pipe kernel (rr2_gram_tiles*_kernel), 1 ddmpc_gram_tiles_kernel
  bool gram_stream_ok = false, gram_valu_ok = false;      // which of the two can serve this shape
  int ld_window = 0;                       // long_data: doubles of the trajectory window the refining variant stages chunk by chunk
  size_t ld_lds_bytes = 0;                 // ... and the LDS of such a launch
  bool long_data = false;                  // the trajectory does not fit the cold kernel's LDS: streaming Gram + gpre, no refinement (KParams::stage_xs = 0)
  DevBuf d_wd, d_rr2y;                     // dense weighting matrices of a NOMINAL controller beyond 271 rows: W of the free components (position
                                           //   order, shared by the batch); Y = W C per instance (rr2_wc_kernel)
  DevBuf d_rr2tol, d_rr2rank;              // ... per-instance pivot tolerance and [flag, accepted pivots] of the rank decision (+ one counter word)
  DevBuf d_rr2cand;                        // ... the pivot candidates of G's factorisation as they were met (Rr2Chol::cand)
  DevBuf d_perm, d_rr2d, d_rr2res;                   // phase kernels (ddmpc_rr2.hpp): fixed-first component order [perm | iperm]; per instance
                                           // [max diag of G | max diag of T | live chunks of G | live chunks of T]
  int nF = 0;                              // fixed components (hard constraints), nominal scheme
  int large_pipeline = DDMPC_PIPELINE_PHASES;   // DDMPC_OPT_LARGE_PIPELINE
  int convex_update = 1;                        // DDMPC_OPT_CONVEX_UPDATE: active-set iterations keep the first factor (rank-k update)
  int convex_warm = 0;                     // DDMPC_OPT_CONVEX_WARM_LAW: warm steps under the slack box run the active-set iteration on the law
  DevBuf d_mcol, d_cwl_tab, d_cwl_sg, d_cwl_ref;   // ... M = K0^-1 E_box [batch][nbox][r]; [box_rho | box_of]; k x k scratch; refined-law flags (+ count)
  int box_safeguard = 0;                   // DDMPC_OPT_BOX_SAFEGUARD: Route::BoxLaw instances at the max_iter cap are finished by box_safeguard
  int box_warm = 0;                        // DDMPC_OPT_BOX_WARM_START: Route::BoxLaw steps start their iteration from the last solve's set
  DevBuf d_box_seed;                       // ... that set, [batch][nbox] (written by the WARM instantiations of the box kernels)
  int large_box_warm = 0;                  // DDMPC_OPT_LARGE_BOX_WARM_START: steps of a bounded handle beyond 271 rows start from the last solve's set
  DevBuf d_large_seed;                     // ... that set, sa + 4 say per row, [batch][rE] (rr3_box_keep_seed_kernel)
  int large_box_law = 0;                   // DDMPC_OPT_LARGE_BOX_LAW: steps of a bounded handle beyond 271 rows on the affine law while inside the box
  int setpoint_law = 0;                    // DDMPC_OPT_SETPOINT_LAW: ddmpc_prepare also forms S = K0^-1 [1_c] (ddmpc_setpoint_law.hpp)
  DevBuf d_sgain, d_sptab;                 // ... S [batch][m+p][r]; the m + p table copies with a unit setpoint (refined columns)
  int setpoint_box_law = 0;                // DDMPC_OPT_SETPOINT_BOX_LAW: the same on a handle that may carry bounds (ddmpc_setpoint_box_law.hpp); it governs when both are on
  DevBuf d_chbnd;                          // ... [lo (m+p) | hi (m+p)] per channel, +-infinity without a bound (ddmpc_prepare on Route::BoxLaw)
  int setpoint_convex_law = 0;             // DDMPC_OPT_SETPOINT_CONVEX_LAW: the same under the CONVEX slack box, slack-only or bounded (the SLACK instantiations of ddmpc_setpoint_box_law.hpp);
                                           //   never on together with the two above (they refuse CONVEX, this one slack NONE)
  DevBuf d_sp, d_uref, d_yref;             // ... staging of host setpoints [u_s | y_s] (ddmpc_step_setpoints) and schedules (ddmpc_closed_loop_setpoints)
  const double *sp_us = nullptr, *sp_ys = nullptr;   // ... the device setpoints of the ddmpc_step_setpoints call in progress
  long long sp_su = 0, sp_sy = 0;          // ... DDMPC_OPT_LARGE_SETPOINTS: their per-instance strides (m, p; a schedule row: n_steps m, n_steps p)
  int large_setpoint_bounds = 0;           // DDMPC_OPT_LARGE_SETPOINT_BOUNDS: the setpoint calls on a bounded handle on Route::RobustPhases (the bounded phase kernels with the instance's setpoint)
  int large_setpoints = 0;                 // DDMPC_OPT_LARGE_SETPOINTS: the setpoint calls on Route::RobustPhases (a setpoint per instance on the kept factors)
  // input bounds (ddmpc_set_input_bounds) and output bounds (ddmpc_set_output_bounds): per channel, +-infinity = none; the
  // vectors are empty without a finite bound of their kind; `bounded` = some bound of either kind is finite (Route::BoxLaw)
  std::vector<double> umin_h, umax_h, ymin_h, ymax_h;
  bool bounded = false;
  DevBuf d_box_bd, d_ubnd, d_ybnd;         // ... [a | c | lo | hi | 1/d] of the box list (ddmpc_box_law.hpp); [u_min | u_max], [y_min | y_max] for the reconstruction
  // per-instance bounds (ddmpc_set_instance_input_bounds / _output_bounds, Route::BoxLaw at most 271 rows): [batch][m] / [batch][p]
  // rows, empty while the kind is shared or absent.  umin_h .. ymax_h above then hold, per channel, the smallest finite lower and
  // the largest finite upper bound of the batch (infinite where no instance has one): which channels are boxed -- all that
  // build_box_list and the shared [lo | hi] columns of d_box_bd are asked for on such a handle.  d_ibnd: the channel table
  // [batch][lo (m+p) | hi (m+p)] of ddmpc_box_law.hpp (BoxChannels), kept while either kind is per instance (the shared kind broadcast
  // into it, -+infinity without a bound).
  std::vector<double> iumin_h, iumax_h, iymin_h, iymax_h;
  DevBuf d_ibnd;
  int instance_setpoint_bounds = 0;        // DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS: per-instance bounds and DDMPC_OPT_SETPOINT_BOX_LAW / _CONVEX_LAW on one handle
                                           //   (the BoxChannels instantiations of ddmpc_setpoint_box_law.hpp read d_ibnd); 0: the two refuse each other
  DevBuf s_gain, s_prep_status, s_mcol, s_cwl_ref;   // ... the preparation of ddmpc_solve's own (solve_box): a kept ddmpc_prepare survives the solve
  int epoch = 0;                           // cold launches so far (KParams::epoch)
  int flag_epoch = 0;                      // latest stamp written into d_rflag
  HostBuf h_io;
  HostBuf h_flag;                          // one pinned word: the "factor again" count of the rank decision (launch_rr2_factors)
  hipEvent_t ev_flag = nullptr;            // ... and the event behind its copy
  int closed_loop_path = DDMPC_PATH_AUTO;
  const char* loop_kernel = "";           // the kernel that stepped the plant in the last ddmpc_closed_loop (ddmpc_closed_loop_kernel_name)
  bool closed_loop_graph = false;
  bool large = false;                      // r beyond the register-resident cold kernels: global-workspace kernels only
  bool large_nominal = false;              // ... NOMINAL (the rank-revealing kernels); else ROBUST
  int n_free = 0;                          // weighted (free) components, nominal scheme: rows of the reduced normal matrix
  bool stamps_on = false;                  // ddmpc_debug_stamps (the phase kernels carry no stamps)
};

// The one decision of which implementation serves a handle.  Beyond the register-resident kernels the phase kernels take
// batches up to 65535 (grid rows), up to 1024 rows (64-bit masks over 16-column chunks) and no diagnostic stamps
// (DDMPC_OPT_LARGE_PIPELINE selects them by default); the one-workgroup kernels serve everything else at that size.
static Route select_route(const ddmpc_handle* h) {
  if (!h->large) return h->bounded ? Route::BoxLaw : Route::Cold;
  const bool phases = h->large_pipeline == DDMPC_PIPELINE_PHASES && h->batch <= 65535 && !h->stamps_on && h->kp.r <= 1024;
  if (h->large_nominal) return phases ? Route::NominalPhases : Route::NominalOneWg;
  return phases ? Route::RobustPhases : Route::RobustOneWg;
}

// Bounds of either kind are per instance: the BoxChannels instantiations of ddmpc_box_law.hpp serve the handle's steps and fused loops.
static bool instance_bounds(const ddmpc_handle* h) { return !h->iumin_h.empty() || !h->iymin_h.empty(); }

static bool nominal_route(Route r) { return r == Route::NominalPhases || r == Route::NominalOneWg; }

// What ddmpc_prepare kept is the input of the route it was formed on only (the routes keep different things next to the factors).
static bool prep_valid(const ddmpc_handle* h) { return h->prep.valid && h->prep.route == select_route(h); }

// Forget what ddmpc_prepare kept (the data, the weights or an option it was formed with changed) -- and with it the seed of
// DDMPC_OPT_LARGE_BOX_WARM_START, which belongs to the kept factors, the order and the box table (every call that changes one
// of them comes through here: ddmpc_set_data, ddmpc_set_setpoints, both bounds calls, a new ddmpc_prepare).
static void forget_prep(ddmpc_handle* h) { h->prep = Prep{}; h->last.large_seed = false; }

// ddmpc_prepare forms S and the three setpoint calls are open: DDMPC_OPT_SETPOINT_LAW, _SETPOINT_BOX_LAW or _SETPOINT_CONVEX_LAW is on
// -- or, beyond 271 rows, DDMPC_OPT_LARGE_SETPOINTS (the calls run on the kept factors; S next to the law of DDMPC_OPT_LARGE_AFFINE_LAW)
// or DDMPC_OPT_LARGE_SETPOINT_BOUNDS (the same on a handle that may carry input / output bounds; no S).
static bool setpoint_on(const ddmpc_handle* h) {
  return h->setpoint_law != 0 || h->setpoint_box_law != 0 || h->setpoint_convex_law != 0 || h->large_setpoints != 0 || h->large_setpoint_bounds != 0;
}
// DDMPC_OPT_SETPOINT_CONVEX_LAW on a slack-only CONVEX handle (Route::Cold): ddmpc_prepare forms the slack box list with its
// [a | c | lo | hi | 1/d] table and M for the setpoint calls, whether or not DDMPC_OPT_CONVEX_WARM_LAW is on.
static bool setpoint_convex_slack_only(const ddmpc_handle* h) { return h->setpoint_convex_law != 0 && h->kp.convex && !h->large && !h->bounded; }

// An option that decides which kernels serve a bounded handle on Route::RobustPhases was set (DDMPC_OPT_LARGE_BOX_CAPACITY,
// _SAFEGUARD, _WARM_START, _LAW): the next solve may lay the per-instance record out differently, and setting one, to any value,
// drops the seed (the next step starts from the empty set).
static void forget_large_box_solve(ddmpc_handle* h) { h->last.valid = false; h->last.large_seed = false; }

// A call that writes solve outputs starts the record afresh (nothing of an earlier call survives) and makes it readable at its end.
static Route begin_solve(ddmpc_handle* h, Route route) { h->last = LastSolve{}; h->last.route = route; return route; }
static void end_solve(ddmpc_handle* h, const double* up, const double* yp) { h->last.up = up; h->last.yp = yp; h->last.valid = true; }

// DDMPC_OPT_BOX_WARM_START: the last solve of the handle left a seed the next step on Route::BoxLaw may read.  It lives with the
// record of that solve: whatever makes the record unreadable (new data, setpoints, bounds, a new ddmpc_prepare) drops the seed,
// so a seed indexed by another box table is never read.  Asked before begin_solve starts the next record.
static bool box_seed_valid(const ddmpc_handle* h) {
  return h->box_warm && h->last.valid && h->last.route == Route::BoxLaw && h->last.box_seed;
}

// DDMPC_OPT_LARGE_BOX_WARM_START: the last solve of the handle left a seed the next step on Route::RobustPhases may read.  Unlike
// box_seed_valid it does not ask for a finished record: the steps of the per-step closed loop follow each other inside one
// call.  What drops it clears the flag itself (forget_prep, forget_large_box_solve, option 12).  Asked before begin_solve.
static bool large_seed_valid(const ddmpc_handle* h) {
  return h->large_box_warm && h->last.route == Route::RobustPhases && h->last.large_seed;
}

// A parameter table of upload_params (d_tabi: 3 rows, d_tabd: 4 rows of 16 NT entries) read back to the host.  The blocking copy
// is also a synchronisation point: ddmpc_prepare without input bounds has no other one before it overwrites d_cwl_tab.
template <class T>
static int read_table(const DevBuf& d, size_t count, std::vector<T>* out) {
  out->resize(count);
  HIP_TRY(hipMemcpy(out->data(), d.p, count * sizeof(T), hipMemcpyDeviceToHost));
  return DDMPC_OK;
}

// The <SAFE, YB> template arguments of the bounded kernels from (DDMPC_OPT_BOX_SAFEGUARD, output bounds): f(std::bool_constant<SAFE>,
// std::bool_constant<YB>), a generic lambda that names the instantiation and launches it.  Every bounded launch goes through here.
template <class F>
static void with_safe_yb(bool safe, bool yb, F&& f) {
  if (safe) {
    if (yb) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{});
  } else {
    if (yb) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{});
  }
}

extern "C" {

int ddmpc_version(void) { return DDMPC_ABI_VERSION; }

const char* ddmpc_last_error(void) { return g_err.c_str(); }

int ddmpc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// Per-component tables of the reduced system, shared by the whole batch.
// Row rho = k*nch + ch of the internal ordering; see KParams in ddmpc_kernels.hpp.
//   ubar, internal window (controller.py:577) / terminal window (:612,620): hard value  -> D = 0
//   ubar, free prediction steps: penalty r (:709)                                       -> D = 1/r
//   w = ybar + sigma, internal window: sigma free, ybar = y_past (:578)                 -> D = 1/lamb_sigma
//   w, terminal window: ybar = y_s (:615,621), sigma = w - y_s boxed (:659,674)          -> D = 1/lamb_sigma | 0
//   w, free prediction steps: q (ybar - y_s)^2 + lamb_sigma sigma^2 (:710,716), boxed   -> D = 1/q + 1/lamb_sigma | 1/q
//   nominal scheme: no sigma (:536-538); ybar rows behave like ubar rows with weight q.
// Inverse of a symmetric positive definite n x n matrix (row-major) by Cholesky; false if not SPD -- numerically: a pivot
// below 1e-13 of the largest diagonal entry is a singular (or indefinite) matrix whose "inverse" would be rounding noise.
static bool spd_inverse(std::vector<double>& a, int n) {
  std::vector<double> l((size_t)n * n, 0.0);
  double dmax = 0.0;
  for (int j = 0; j < n; ++j) dmax = std::max(dmax, a[(size_t)j * n + j]);
  for (int j = 0; j < n; ++j) {
    double d = a[(size_t)j * n + j];
    for (int k = 0; k < j; ++k) d -= l[(size_t)j * n + k] * l[(size_t)j * n + k];
    if (!(d > 1e-13 * dmax)) return false;
    const double dj = std::sqrt(d);
    l[(size_t)j * n + j] = dj;
    for (int i = j + 1; i < n; ++i) {
      double v = a[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) v -= l[(size_t)i * n + k] * l[(size_t)j * n + k];
      l[(size_t)i * n + j] = v / dj;
    }
  }
  // T = L^-1 (lower), then A^-1 = T' T
  std::vector<double> t((size_t)n * n, 0.0);
  for (int c = 0; c < n; ++c) {
    t[(size_t)c * n + c] = 1.0 / l[(size_t)c * n + c];
    for (int i = c + 1; i < n; ++i) {
      double v = 0.0;
      for (int k = c; k < i; ++k) v -= l[(size_t)i * n + k] * t[(size_t)k * n + c];
      t[(size_t)i * n + c] = v / l[(size_t)i * n + i];
    }
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
      for (int k = i; k < n; ++k) v += t[(size_t)k * n + i] * t[(size_t)k * n + j];
      a[(size_t)i * n + j] = a[(size_t)j * n + i] = v;
    }
  return true;
}

// 1/w of an unweighted (w = 0) component: K_ii = lam * 1e25 makes its multiplier beta_i = (t_i - (G beta)_i) / (lam 1e25),
// zero to ~1e-25 relative, and z_i = t_i - lam D beta_i = (G beta)_i exactly as for a free component; every other
// pivot sees a perturbation of order G_ij^2 / 1e25.
static const double DDMPC_UNWEIGHTED = 1e25;
static inline double inv_weight(double w) { return w > 0.0 ? 1.0 / w : DDMPC_UNWEIGHTED; }

// ROBUST beyond the register-resident kernels on the phase kernels (ddmpc_rr3.hpp): the component order "boxed LAST" (time
// order inside both classes), so that every active-set iteration works on the trailing block of the factor, and -- with input
// or output bounds -- the table of boxed components the kernels test (Rr3Box).  The boxed class is the union of
// the slack rows (CONVEX: K_WPRED, K_WTERM), the free input rows of the channels with a finite input bound and the free output
// rows of the channels with a finite output bound.  Host arithmetic on the parameter tables (ti: 3 rows, td: 4 rows of RP
// entries), no handle; umin / umax [m], ymin / ymax [p], null = no bounds of that kind (then no table is formed).
struct LargeBox {
  std::vector<int> pm;          // [position -> component (rv) | component -> position (rv)]
  int nA = 0;                   // first boxed position
  int nbox = 0;                 // components of the table: ascending by position, the slack before the output on a shared row
  std::vector<int> ip;          // [position (nbox) | output component? (nbox) | setpoint channel, -1 for a slack (nbox) | terminal constraint? (1)]
  std::vector<double> bd;       // [a | c | lo | hi | 1/d | shlo | shhi], nbox each, then [u_min (m) | u_max (m) | y_min (p) | y_max (p)]
};
static LargeBox build_large_box(const KParams& k, int RP, const std::vector<int>& ti, const std::vector<double>& td,
                                const double* umin, const double* umax, const double* ymin, const double* ymax, int tec) {
  LargeBox lb;
  const size_t rv = ((size_t)k.r + 1) & ~(size_t)1;
  lb.pm.assign(2 * rv, 0);
  auto slack = [&](int rho) { return k.convex && (ti[rho] == K_WPRED || ti[rho] == K_WTERM); };
  auto input = [&](int rho) {
    const int ch = rho % k.nch;
    return umin != nullptr && ti[rho] == K_UFREE && ch < k.m && (std::isfinite(umin[ch]) || std::isfinite(umax[ch]));
  };
  auto output = [&](int rho) {
    const int cy = rho % k.nch - k.m;
    return ymin != nullptr && ti[rho] == K_WPRED && cy >= 0 && (std::isfinite(ymin[cy]) || std::isfinite(ymax[cy]));
  };
  int pos = 0;
  for (int cls = 0; cls < 2; ++cls) {
    for (int rho = 0; rho < k.r; ++rho) {
      const bool boxed = slack(rho) || input(rho) || output(rho);
      if ((boxed ? 1 : 0) == cls) { lb.pm[pos] = rho; lb.pm[rv + rho] = pos; ++pos; }
    }
    if (cls == 0) lb.nA = pos;
  }
  if (umin == nullptr && ymin == nullptr) return lb;
  std::vector<int> cpos, cy, cch;
  std::vector<double> cols[R3B_NV];
  auto add = [&](int i, int isy, int ch, double a, double c, double lo, double hi, double d) {
    cpos.push_back(i); cy.push_back(isy); cch.push_back(ch);
    const double v[R3B_NV] = {a, c, lo, hi, 1.0 / d, lo - a, hi - a};
    for (int q = 0; q < R3B_NV; ++q) cols[q].push_back(v[q]);
  };
  for (int i = lb.nA; i < k.r; ++i) {
    const int rho = lb.pm[i], ch = rho % k.nch;
    const double D0 = td[rho], D1 = td[(size_t)RP + rho], tb = td[2 * (size_t)RP + rho];
    if (slack(rho)) add(i, 0, -1, 0.0, k.sig_scale, -k.bound, k.bound, k.lam * (D0 - D1));        // sigma = -lam beta / lamb_sigma
    if (input(rho)) add(i, 0, ch, tb, -k.lam * D0, umin[ch], umax[ch], k.lam * D0);               // u = u_s - lam beta / r
    if (output(rho)) add(i, 1, ch, tb, -k.lam * D1, ymin[ch - k.m], ymax[ch - k.m], k.lam * D1);  // ybar = y_s - lam beta / q
  }
  lb.nbox = (int)cpos.size();
  lb.ip = cpos;
  lb.ip.insert(lb.ip.end(), cy.begin(), cy.end());
  lb.ip.insert(lb.ip.end(), cch.begin(), cch.end());         // (the setpoint instantiations of the bounded kernels: whose setpoint a_s is)
  lb.ip.push_back(tec ? 1 : 0);
  for (int q = 0; q < R3B_NV; ++q) lb.bd.insert(lb.bd.end(), cols[q].begin(), cols[q].end());
  const double inf = std::numeric_limits<double>::infinity();          // [u_min | u_max | y_min | y_max] for the output stage
  for (int side = 0; side < 2; ++side)
    for (int ch = 0; ch < k.m; ++ch) lb.bd.push_back(umin ? (side ? umax[ch] : umin[ch]) : (side ? inf : -inf));
  for (int side = 0; side < 2; ++side)
    for (int ch = 0; ch < k.p; ++ch) lb.bd.push_back(ymin ? (side ? ymax[ch] : ymin[ch]) : (side ? inf : -inf));
  return lb;
}

// The order and the box table of a ROBUST handle beyond 271 rows, from the tables upload_params kept and the handle's bounds.
static int upload_large_box(ddmpc_handle* h) {
  const LargeBox lb = build_large_box(h->kp, 16 * h->kc.NT, h->ti_h, h->td_h, h->umin_h.empty() ? nullptr : h->umin_h.data(),
                                      h->umin_h.empty() ? nullptr : h->umax_h.data(), h->ymin_h.empty() ? nullptr : h->ymin_h.data(),
                                      h->ymin_h.empty() ? nullptr : h->ymax_h.data(), h->prm.use_terminal_constraint);
  int rc;
  h->nA3 = lb.nA;
  h->nbox3 = lb.nbox;
  if ((rc = h->d_perm.ensure(lb.pm.size() * sizeof(int)))) return rc;
  HIP_TRY(hipMemcpy(h->d_perm.p, lb.pm.data(), lb.pm.size() * sizeof(int), hipMemcpyHostToDevice));
  if (lb.nbox == 0) return DDMPC_OK;
  if ((rc = h->d_r3bi.ensure(lb.ip.size() * sizeof(int))) || (rc = h->d_r3bd.ensure(lb.bd.size() * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpy(h->d_r3bi.p, lb.ip.data(), lb.ip.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->d_r3bd.p, lb.bd.data(), lb.bd.size() * sizeof(double), hipMemcpyHostToDevice));
  return DDMPC_OK;
}

static int upload_params(ddmpc_handle* h) {
  const ddmpc_params& p = h->prm;
  const KParams& k = h->kp;
  const int RP = 16 * h->kc.NT;
  std::vector<double> td(4 * (size_t)RP, 0.0);
  std::vector<int> ti(3 * (size_t)RP, -1);
  const bool robust = p.controller_type == DDMPC_ROBUST;
  const bool tec = p.use_terminal_constraint != 0;
  const bool diag = p.weight_kind == DDMPC_WEIGHT_DIAG;
  const bool dense = p.weight_kind == DDMPC_WEIGHT_DENSE;
  for (int rho = 0; rho < RP; ++rho) {
    double D0 = 0, D1 = 0, tb = 0, wq = 0;
    int kind = K_PAD, pidx = -1, oidx = -1;
    if (rho < k.r) {
      const int kk = rho / k.nch, ch = rho % k.nch;
      const int kp = kk - p.n;
      const bool is_int = kp < 0;
      const bool is_term = tec && kp >= p.L - p.n;
      if (ch < p.m) {
        tb = h->us_h[ch];
        if (is_int) { kind = K_UFIX; pidx = kk * p.m + ch; }
        else if (is_term) { kind = K_UFIX; }
        else if (dense) { kind = K_UFREE; }
        else { kind = K_UFREE; wq = diag ? h->Rh[kp * p.m + ch] : h->Rh[0]; D0 = D1 = inv_weight(wq); }
        if (!is_int) oidx = kp * p.m + ch;
      } else {
        const int cy = ch - p.m;
        tb = h->ys_h[cy];
        const double q = (is_int || dense) ? 0.0 : (diag ? h->Qh[kp * p.p + cy] : h->Qh[0]);
        wq = q;
        if (!robust) {
          if (is_int) { kind = K_YFIX; pidx = p.n * p.m + kk * p.p + cy; }
          else if (is_term) { kind = K_YFIX; }
          else { kind = K_YFREE; if (!dense) D0 = D1 = inv_weight(q); }
        } else {
          const double ils = 1.0 / p.lamb_sigma;
          if (is_int) { kind = K_WINT; pidx = p.n * p.m + kk * p.p + cy; D0 = D1 = ils; }
          else if (is_term) { kind = K_WTERM; D0 = ils; D1 = 0.0; }
          else if (dense) { kind = K_WPRED; D0 = ils; D1 = 0.0; }    // + Q_ff^-1 from the dense matrix
          else { kind = K_WPRED; D0 = inv_weight(q) + ils; D1 = inv_weight(q); }
        }
      }
    }
    td[0 * RP + rho] = D0; td[1 * RP + rho] = D1; td[2 * RP + rho] = tb; td[3 * RP + rho] = wq;
    ti[0 * RP + rho] = kind; ti[1 * RP + rho] = pidx; ti[2 * RP + rho] = oidx;
  }
  int rc;
  if ((rc = h->d_tabd.ensure(td.size() * sizeof(double)))) return rc;
  if ((rc = h->d_tabi.ensure(ti.size() * sizeof(int)))) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_tabd.p, td.data(), td.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_tabi.p, ti.data(), ti.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->kp.tabd = (const double*)h->d_tabd.p;
  h->kp.tabi = (const int*)h->d_tabi.p;
  h->n_free = 0;
  for (int rho = 0; rho < k.r; ++rho)
    if (ti[0 * RP + rho] == K_UFREE || ti[0 * RP + rho] == K_YFREE) ++h->n_free;
  if (h->large_nominal) {
    // the component order of the rank-revealing route (ddmpc_nominal_rr_kernel): fixed inputs, fixed outputs, free inputs,
    // free outputs, time order inside a class -- the same for every instance, so it is formed once here for the phase kernels
    const size_t rv = ((size_t)k.r + 1) & ~(size_t)1;
    std::vector<int> pm(2 * rv, 0);
    int pos = 0;
    h->nF = 0;
    for (int cls = 0; cls < 4; ++cls) {
      const int want = cls == 0 ? K_UFIX : cls == 1 ? K_YFIX : cls == 2 ? K_UFREE : K_YFREE;
      for (int rho = 0; rho < k.r; ++rho)
        if (ti[0 * RP + rho] == want) { pm[pos] = rho; pm[rv + rho] = pos; ++pos; }
      if (cls == 1) h->nF = pos;
    }
    if ((rc = h->d_perm.ensure(pm.size() * sizeof(int)))) return rc;
    HIP_TRY(hipMemcpy(h->d_perm.p, pm.data(), pm.size() * sizeof(int), hipMemcpyHostToDevice));
    std::vector<double> wz(2 * rv, 0.0);            // cost weight and target of the free components, position order
    for (int i = 0; i + h->nF < k.r; ++i) { wz[i] = td[3 * (size_t)RP + pm[h->nF + i]]; wz[rv + i] = td[2 * (size_t)RP + pm[h->nF + i]]; }
    if ((rc = h->d_wz.ensure(wz.size() * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(h->d_wz.p, wz.data(), wz.size() * sizeof(double), hipMemcpyHostToDevice));
    if (dense) {
      // W of the free components in position order (controller.py:708-710: R couples the inputs of the prediction steps, Q the
      // outputs, nothing couples the two), nR x nR row-major, shared by the batch
      const size_t nR = (size_t)k.r - (size_t)h->nF;
      std::vector<double> wd(nR * nR, 0.0);
      const int ml = p.m * p.L, pl = p.p * p.L;
      auto widx = [&](int rho, bool& is_u) -> int {                  // row of R (inputs) or Q (outputs) of component rho
        const int kk = rho / k.nch, ch = rho % k.nch, kp = kk - p.n;
        is_u = ch < p.m;
        return is_u ? kp * p.m + ch : kp * p.p + (ch - p.m);
      };
      for (size_t i = 0; i < nR; ++i) {
        bool ui; const int ai = widx(pm[h->nF + i], ui);
        for (size_t j = 0; j < nR; ++j) {
          bool uj; const int aj = widx(pm[h->nF + j], uj);
          if (ui == uj) wd[i * nR + j] = ui ? h->Rh[(size_t)ai * ml + aj] : h->Qh[(size_t)ai * pl + aj];
        }
      }
      if ((rc = h->d_wd.ensure(wd.size() * sizeof(double)))) return rc;
      HIP_TRY(hipMemcpy(h->d_wd.p, wd.data(), wd.size() * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  if (h->large && !h->large_nominal) {
    // ROBUST beyond the register-resident kernels on the phase kernels (ddmpc_rr3.hpp): the boxed components go LAST
    h->ti_h = ti;
    h->td_h = td;
    if ((rc = upload_large_box(h))) return rc;
  }
  h->kp.dense_w = 0;
  h->kp.dmat = nullptr;
  if (dense) {
    // lam * W^-1 as a full matrix.  Only the free prediction steps carry weights: the terminal steps are
    // fixed to the setpoint (controller.py:612-627), so their rows/columns of Q, R drop out of the cost.
    //   ubar free:            W = R_ff                      -> W^-1 = R_ff^-1
    //   ybar free (nominal):  W = Q_ff                      -> W^-1 = Q_ff^-1
    //   ybar+sigma free:      min over the split of q-form + lamb_sigma |sigma|^2 -> W^-1 = Q_ff^-1 + P_I/lamb_sigma,
    //                         P_I = the components whose sigma is NOT at its bound: the slack box only switches a diagonal term
    // Diagonal-only components (internal / terminal sigma) keep their tabd entries.
    const int nfree = tec ? p.L - p.n : p.L;
    std::vector<double> dm((size_t)RP * RP, 0.0);
    for (int pass = 0; pass < 2; ++pass) {
      const int nc = pass == 0 ? p.m : p.p, ld = nc * p.L, nn = nc * nfree;
      const std::vector<double>& W = pass == 0 ? h->Rh : h->Qh;
      std::vector<double> a((size_t)nn * nn);
      for (int i = 0; i < nn; ++i)
        for (int j = 0; j < nn; ++j) a[(size_t)i * nn + j] = 0.5 * (W[(size_t)i * ld + j] + W[(size_t)j * ld + i]);
      // Components whose row (= column) of the weighting matrix is entirely zero are unweighted, exactly like a zero on the
      // diagonal of a DIAG matrix (inv_weight): they leave the block that is inverted and get 1/w = DDMPC_UNWEIGHTED on the
      // diagonal.  This is the singular case that can be served with the Gram matrix in its own coordinates; a null space
      // that is NOT spanned by coordinate axes would need the Gram tiles rotated per instance (a penalty on a skew direction
      // cancels catastrophically in the Cholesky) and stays unsupported.
      std::vector<int> keep;
      for (int i = 0; i < nn; ++i) {
        bool any = false;
        for (int j = 0; j < nn && !any; ++j) any = a[(size_t)i * nn + j] != 0.0;
        if (any) keep.push_back(i);
      }
      const int nk = (int)keep.size();
      std::vector<double> ak((size_t)nk * nk);
      for (int i = 0; i < nk; ++i)
        for (int j = 0; j < nk; ++j) ak[(size_t)i * nk + j] = a[(size_t)keep[i] * nn + keep[j]];
      if (nk > 0 && !spd_inverse(ak, nk))
        return fail(DDMPC_ERR_UNSUPPORTED, "%s must be positive definite on the free prediction steps once its all-zero rows and "
                    "columns (unweighted components) are set aside (HIP path)", pass == 0 ? "R" : "Q");
      auto row_of = [&](int i) { return (p.n + i / nc) * k.nch + (pass == 0 ? 0 : p.m) + i % nc; };
      for (int i = 0; i < nn; ++i) { const int ri = row_of(i); dm[(size_t)ri * RP + ri] = DDMPC_UNWEIGHTED; }
      for (int i = 0; i < nk; ++i)
        for (int j = 0; j < nk; ++j)
          dm[(size_t)row_of(keep[i]) * RP + row_of(keep[j])] = ak[(size_t)i * nk + j];     // (robust y rows: + 1/lamb_sigma on the
                                                                  //  diagonal via tabd, switched off for a sigma at its bound)
    }
    if ((rc = h->d_dmat.ensure(dm.size() * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(h->d_dmat.p, dm.data(), dm.size() * sizeof(double), hipMemcpyHostToDevice));
    h->kp.dense_w = 1;
    h->kp.dmat = (const double*)h->d_dmat.p;
  }
  return DDMPC_OK;
}

int ddmpc_create(const ddmpc_params* params, int64_t batch, int device, ddmpc_handle** out) {
  if (!params || !out) return fail(DDMPC_ERR_INVALID, "params/out must not be null");
  *out = nullptr;
  if (params->struct_size != (int32_t)sizeof(ddmpc_params))
    return fail(DDMPC_ERR_INVALID, "ddmpc_params.struct_size mismatch (%d != %zu)", params->struct_size,
                sizeof(ddmpc_params));
  const ddmpc_params& p = *params;
  if (batch <= 0) return fail(DDMPC_ERR_INVALID, "batch must be positive");
  if (p.m <= 0 || p.p <= 0 || p.n <= 0 || p.L <= 0 || p.N <= 0)
    return fail(DDMPC_ERR_INVALID, "m, p, n, L, N must be positive");
  // controller.py:165-168
  if (p.controller_type != DDMPC_NOMINAL && p.controller_type != DDMPC_ROBUST)
    return fail(DDMPC_ERR_INVALID, "Unsupported controller type.");
  // controller.py:211-215
  if (p.slack_type != DDMPC_SLACK_NON_CONVEX && p.slack_type != DDMPC_SLACK_CONVEX &&
      p.slack_type != DDMPC_SLACK_NONE)
    return fail(DDMPC_ERR_INVALID, "Unsupported slack variable constraint type.");
  // controller.py:664-670 (raised while defining the constraints of a robust controller)
  if (p.controller_type == DDMPC_ROBUST && p.slack_type == DDMPC_SLACK_NON_CONVEX)
    return fail(DDMPC_ERR_UNSUPPORTED,
                "Robust Data-Driven MPC with a Non-Convex slack variable constraint is not currently "
                "implemented, since it cannot be efficiently solved.");
  // controller.py:316-325
  if (p.controller_type == DDMPC_NOMINAL && p.L < p.n)
    return fail(DDMPC_ERR_INVALID,
                "The prediction horizon (`L`) must be greater than or equal to the estimated system order `n`.");
  if (p.controller_type == DDMPC_ROBUST && p.L < 2 * p.n)
    return fail(DDMPC_ERR_INVALID,
                "The prediction horizon (`L`) must be greater than or equal to two times the estimated "
                "system order `n`.");
  if (p.N < p.L + p.n) return fail(DDMPC_ERR_INVALID, "N must be greater than or equal to L.");  // hankel_matrix.py:43-44
  if (!p.Q || !p.R || !p.u_s || !p.y_s) return fail(DDMPC_ERR_INVALID, "Q, R, u_s, y_s must not be null");
  if (p.weight_kind != DDMPC_WEIGHT_SCALAR && p.weight_kind != DDMPC_WEIGHT_DIAG && p.weight_kind != DDMPC_WEIGHT_DENSE)
    return fail(DDMPC_ERR_UNSUPPORTED, "weight_kind must be DDMPC_WEIGHT_SCALAR, _DIAG or _DENSE");
  const bool wdense = p.weight_kind == DDMPC_WEIGHT_DENSE;
  const size_t pl = (size_t)p.p * p.L, ml = (size_t)p.m * p.L;
  const size_t nq = wdense ? pl * pl : (p.weight_kind == DDMPC_WEIGHT_DIAG ? pl : 1);
  const size_t nr = wdense ? ml * ml : (p.weight_kind == DDMPC_WEIGHT_DIAG ? ml : 1);
  if (!wdense) {
    // scalar / diagonal weights may be positive SEMI-definite (controller.py:708-710 accepts any PSD matrix): a zero weight
    // leaves that component unpenalised, i.e. its multiplier is zero -- realised as 1/w = DDMPC_UNWEIGHTED (see upload_params)
    for (size_t i = 0; i < nq; ++i)
      if (!(p.Q[i] >= 0.0)) return fail(DDMPC_ERR_INVALID, "Q must be positive semi-definite (negative or NaN diagonal entry)");
    for (size_t i = 0; i < nr; ++i)
      if (!(p.R[i] >= 0.0)) return fail(DDMPC_ERR_INVALID, "R must be positive semi-definite (negative or NaN diagonal entry)");
  } else {
    for (int pass = 0; pass < 2; ++pass) {
      const double* W = pass ? p.R : p.Q;
      const size_t nn = pass ? ml : pl;
      double mx = 0.0;
      for (size_t i = 0; i < nn * nn; ++i) mx = std::fabs(W[i]) > mx ? std::fabs(W[i]) : mx;
      for (size_t i = 0; i < nn; ++i)
        for (size_t j = 0; j < i; ++j)
          if (std::fabs(W[i * nn + j] - W[j * nn + i]) > 1e-12 * mx)
            return fail(DDMPC_ERR_INVALID, "%s must be symmetric", pass ? "R" : "Q");
    }
  }
  if (p.controller_type == DDMPC_ROBUST) {
    if (!(p.eps_max > 0.0) || !(p.lamb_alpha > 0.0) || !(p.lamb_sigma > 0.0))
      return fail(DDMPC_ERR_INVALID, "robust controller needs eps_max, lamb_alpha, lamb_sigma > 0");
    if (p.slack_type == DDMPC_SLACK_CONVEX && !(p.c > 0.0))
      return fail(DDMPC_ERR_INVALID, "slack CONVEX needs c > 0");
  }
  if (ddmpc_device_count() <= 0) return fail(DDMPC_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
  if (device < 0 || device >= ddmpc_device_count()) return fail(DDMPC_ERR_NO_DEVICE, "device %d out of range", device);

  ddmpc_handle* h = new (std::nothrow) ddmpc_handle();
  if (!h) return fail(DDMPC_ERR_INVALID, "out of host memory");
  h->prm = p;
  h->Qh.assign(p.Q, p.Q + nq);
  h->Rh.assign(p.R, p.R + nr);
  h->us_h.assign(p.u_s, p.u_s + p.m);
  h->ys_h.assign(p.y_s, p.y_s + p.p);
  h->prm.Q = h->Qh.data();
  h->prm.R = h->Rh.data();
  h->prm.u_s = h->us_h.data();
  h->prm.y_s = h->ys_h.data();
  h->batch = batch;
  h->device = device;

  KParams& k = h->kp;
  k.N = p.N; k.m = p.m; k.p = p.p;
  k.nch = p.m + p.p;
  k.Ln = p.L + p.n;
  k.r = k.nch * k.Ln;
  k.rE = (k.r + 3) & ~3;
  k.c = p.N - k.Ln + 1;
  k.npu = p.n * p.m;
  const bool robust_ = p.controller_type == DDMPC_ROBUST;
  k.convex = robust_ && p.slack_type == DDMPC_SLACK_CONVEX;
  k.lam = robust_ ? p.lamb_alpha * p.eps_max : 0.0;
  k.lamb_sigma = robust_ ? p.lamb_sigma : 1.0;
  k.bound = k.convex ? p.c * p.eps_max : 0.0;
  k.sig_scale = -k.lam / k.lamb_sigma;
  k.box_cost = k.lamb_sigma * k.bound * k.bound;
  k.max_iter = p.max_iter > 0 ? p.max_iter : 50;
  k.refine = DDMPC_REFINE_AUTO;
  k.refine_max = 3;
  // AUTO: relative exact-Hankel residual above which an instance is re-solved with refinement.  Four-tank benchmark data:
  // <= ~1e-12 with errors ~1e-12 (never flagged); the random-plant sweep misses the cost bar from ~1.3e-10 on and errors
  // stay below ~30x the residual (tools/auto_flag_calib_cpu.py, profiles/r03_refine_calib.log)
  k.refine_res = std::pow(10.0, -0.1 * DDMPC_REFINE_RES_DEFAULT);
  if (p.gram_mode != DDMPC_GRAM_AUTO && p.gram_mode != DDMPC_GRAM_DENSE && p.gram_mode != DDMPC_GRAM_STRUCTURED) {
    delete h;
    return fail(DDMPC_ERR_INVALID, "unknown gram_mode %d", p.gram_mode);
  }
  // Structured Gram (AUTO / STRUCTURED): inside the cold-solve kernel for four channels, from ddmpc_gram_tiles_kernel ahead of
  // it for any other count (gram_pre below; the kernel's own fallback for those stays the dense product)
  // (two channels ride on the four-channel scheme inside the kernel: a SISO trajectory is two interleaved four-channel ones)
  k.gram_dense = (p.gram_mode == DDMPC_GRAM_DENSE || (k.nch != 4 && k.nch != 2)) ? 1 : 0;
  k.gpre = nullptr;
  k.gpre_stride = 0;

  const int rows_needed = k.rE + 1;
  const KernelChoice* kc = nullptr;
  for (const KernelChoice& cand : kKernels)
    if (16 * cand.NT >= rows_needed) { kc = &cand; break; }
  static const KernelChoice kLargeNominal = {0, 4, nullptr, "ddmpc_nominal_rr_kernel", nullptr, nullptr, 0, 0, 0};
  static const KernelChoice kLargeSolve = {0, 4, nullptr, "ddmpc_large_solve_kernel", nullptr, nullptr, 0, 0, 0};
  if (!kc) {
    // No register-resident kernel holds this many rows.  With scalar/diagonal weights the problem is served by the
    // global-workspace kernels (plain VALU code): ROBUST controllers by
    // ddmpc_large_solve_kernel, NOMINAL ones by the rank-revealing kernel (accurate only to the extent the Gram
    // route allows at that size).  Dense weights are unsupported here.
    // (dense weighting matrices of a NOMINAL controller at this size: phase kernels only -- rr2_wc_kernel / rr2_wapply_kernel --,
    //  the one-workgroup pipeline refuses them in ddmpc_set_option)
    {   // r-vectors and the Cholesky panel of the global-workspace kernels live in LDS (launch_cold / launch_nominal_rescue)
      // Up to 1024 rows: the phase kernels (64-bit masks over 16-column chunks) or the 512-thread one-workgroup kernels.  Beyond
      // (round 5): the 1024-thread instances of the one-workgroup kernels -- ROBUST (six r-vectors in LDS) up to 2048 rows, NOMINAL
      // (ten) up to 1524
      const bool rob = p.controller_type == DDMPC_ROBUST;
      const size_t rv = ((size_t)k.r + 1) & ~(size_t)1;
      const size_t lds = (rob ? 6 : 10) * rv * sizeof(double) + 4 * rv * sizeof(int) + (size_t)PSD_PAN * sizeof(double);
      const int rmax = PSD_RPT * 1024;                          // the blocked substitutions keep PSD_RPT entries per thread (1024 threads at most)
      if (lds + 1024 > 160 * 1024 || k.r > rmax) {
        delete h;
        return fail(DDMPC_ERR_UNSUPPORTED, "problem too large: (m+p)(L+n) = %d rows (the global-workspace kernels hold %d)", k.r, rmax);
      }
    }
    {   // the trajectory is streamed through the PSD_PAN doubles of LDS scratch in chunks of time steps: a chunk must hold
        // at least four of them next to the L+n steps of overlap (hankel_gram_packed, hankel_normal_times)
      const int tch = ((PSD_PAN / k.nch) - k.Ln) & ~3, tc = ((PSD_PAN - k.r) / (k.nch + 1)) & ~3;
      if (tch < 4 || tc < 4) {
        delete h;
        return fail(DDMPC_ERR_UNSUPPORTED, "problem shape not supported by the global-workspace kernels: m+p = %d channels with "
                    "L+n = %d", k.nch, k.Ln);
      }
    }
    h->large = true;
    h->large_nominal = (p.controller_type == DDMPC_NOMINAL);
    h->kc = h->large_nominal ? kLargeNominal : kLargeSolve;
    h->kc.NT = (rows_needed + 15) / 16;
  } else {
    h->kc = *kc;
  }
  if (h->large) {
    k.xs_len = 0;
    h->lds_bytes = 0;
    if (hipSetDevice(device) != hipSuccess) { delete h; return fail(DDMPC_ERR_HIP, "hipSetDevice(%d) failed", device); }
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
      delete h;
      return fail(DDMPC_ERR_HIP, "hipStreamCreate failed");
    }
    h->own_stream = true;
    int rcl = upload_params(h);
    if (rcl) { ddmpc_destroy(h); return rcl; }
    *out = h;
    return DDMPC_OK;
  }
  // dense-Gram operand reads reach (c+2)*nch + 16*NT; the structured walks read up to
  // x[c + 4*NT + 2]; everything past N*nch is zero padding (the residual check of AUTO refinement clamps its operand
  // addresses to the region: whatever it reads past the data meets a zero in the other operand)
  k.xs_len = ((p.N - k.Ln + 4) * k.nch + 16 * h->kc.NT + 8 + 64 + 1) & ~1;   // + lag groups past Ln in the 4x4x4 base loop
  if (k.xs_len < (p.N + 2) * k.nch) k.xs_len = ((p.N + 2) * k.nch + 1) & ~1;
  h->lds_bytes = lds_doubles_for(h->kc, k.xs_len) * sizeof(double);
  k.stage_xs = 1;
  if (h->lds_bytes > 160 * 1024) {
    // hankel_matrix.py:39-51 takes any N >= L.  A trajectory beyond the LDS is never staged: G = H H' comes from the streaming
    // Gram kernel of the phase pipeline (trajectory in chunks), written into the kernel's tiles (rr2_gram_tiles*_kernel), and the
    // cold kernel runs in its `gpre` mode with no trajectory region at all.  Refinement goes without the whole trajectory on
    // chip: AUTO's exact-Hankel residual check is streamed by the Hankel kernel of the phase pipeline (refine_flagged),
    // and the refining variant passes the trajectory through a window chunk by chunk (ld_window below).
    const int tch = ((RR2_XCAP / k.nch) - k.Ln - 3) & ~3;
    if (k.r > 1024 || tch < 4 || p.weight_kind == DDMPC_WEIGHT_DENSE) {
      const size_t need = h->lds_bytes;
      delete h;
      return fail(DDMPC_ERR_UNSUPPORTED, "trajectory too long for LDS staging (%zu bytes) and no streaming Gram for this shape", need);
    }
    h->long_data = true;
    k.stage_xs = 0;
    k.xs_len = 2;
    k.gram_dense = 0;
    h->lds_bytes = lds_doubles_for(h->kc, k.xs_len) * sizeof(double);
    // the refining variant passes the trajectory through a window of ~2048 doubles + the L + n rows of overlap, chunk by chunk
    const int wcols = (2048 / k.nch) > 64 ? (2048 / k.nch) : 64;
    h->ld_window = ((wcols + k.Ln - 1) * k.nch + 1) & ~1;
    h->ld_lds_bytes = lds_doubles_for(h->kc, h->ld_window) * sizeof(double);
  }
  // Structured Gram ahead of the kernel for plants of other than two or four channels: the streaming matrix-pipe launch
  // (rr2_gram_tiles*_kernel: a chunk of its LDS must hold four time steps next to the L + n of overlap) or the launch that stages
  // the whole trajectory (ddmpc_gram_tiles_kernel, DDMPC_OPT_GRAM_LAUNCH); shapes neither serves keep the dense product
  h->gram_stream_ok = (((RR2_XCAP / k.nch) - k.Ln - 3) & ~3) >= 4 && 16 * h->kc.NT <= 1024;
  h->gram_valu_ok = !h->long_data && gram_tiles_lds_doubles(k.xs_len, k.r, k.nch, h->kc.NT) * sizeof(double) <= 150 * 1024;
  // (measured, tools/gram_modes_time.py: up to five channels the staged launch is the faster one -- long walks, few lags --, from
  //  seven on the streaming one; DDMPC_OPT_GRAM_LAUNCH overrides)
  h->gram_launch = (!h->gram_stream_ok || (h->gram_valu_ok && k.nch <= 5)) ? 1 : 0;
  if (!h->gram_valu_ok) h->gram_launch = 0;
  h->gram_pre = h->long_data || (p.gram_mode != DDMPC_GRAM_DENSE && k.nch != 4 && k.nch != 2 && (h->gram_stream_ok || h->gram_valu_ok));
  if (p.gram_mode == DDMPC_GRAM_STRUCTURED && k.nch != 4 && k.nch != 2 && !h->gram_pre) {
    // AUTO falls back to the dense product silently; a caller who asked for STRUCTURED by name is told
    const int nch_ = k.nch;
    delete h;
    return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_GRAM_STRUCTURED cannot be served for this shape (m+p = %d channels: neither Gram launch "
                "holds it in LDS); use DDMPC_GRAM_AUTO or DDMPC_GRAM_DENSE", nch_);
  }
  if (p.n * k.nch > h->kc.max_past) {       // (implied by L >= n and the instance table; kept as a guard of the LDS aliasing)
    delete h;
    return fail(DDMPC_ERR_UNSUPPORTED, "past window of n (m+p) = %d entries exceeds the %d the kernel stages", p.n * k.nch, h->kc.max_past);
  }
  {   // AUTO refinement's residual check keeps alpha (c doubles) and, with four channels, at least one chunk of partial
      // sums (16 per block of four time offsets) in the LDS scratch region; shapes where that does not fit are refined
      // unconditionally
    const int cpad = (k.c + 1) & ~1, FB = (k.Ln + 3) / 4;
    k.res_fits = (h->kc.scratch >= cpad + (k.nch == 4 ? 16 * FB : 0)) ? 1 : 0;
    if (h->long_data) k.res_fits = 0;         // (no trajectory on chip: an instance the a-priori bound cannot dismiss is flagged, see launch_cold)
  }

  if (hipSetDevice(device) != hipSuccess) { delete h; return fail(DDMPC_ERR_HIP, "hipSetDevice(%d) failed", device); }
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(DDMPC_ERR_HIP, "hipStreamCreate failed");
  }
  h->own_stream = true;
  if (h->lds_bytes > 64 * 1024) {
    hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(h->kc.fn2), h->lds_bytes);
    if (e == hipSuccess)
      e = raise_lds_limit(reinterpret_cast<const void*>(h->kc.fn2r), h->lds_bytes);
    if (e == hipSuccess)
      e = raise_lds_limit(reinterpret_cast<const void*>(h->kc.fn2c), h->lds_bytes);
    if (e != hipSuccess) { ddmpc_destroy(h); return fail(DDMPC_ERR_HIP, "hipFuncSetAttribute(LDS=%zu) failed: %s", h->lds_bytes, hipGetErrorString(e)); }
  }
  if (h->ld_lds_bytes > 64 * 1024) {
    hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(h->kc.fn2r), h->ld_lds_bytes);
    if (e != hipSuccess) { ddmpc_destroy(h); return fail(DDMPC_ERR_HIP, "hipFuncSetAttribute(LDS=%zu) failed: %s", h->ld_lds_bytes, hipGetErrorString(e)); }
  }
  int rc = upload_params(h);
  if (rc) { ddmpc_destroy(h); return rc; }
  *out = h;
  return DDMPC_OK;
}

int ddmpc_destroy(ddmpc_handle* h) {
  if (!h) return DDMPC_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DevBuf* bufs[] = {&h->d_tabd, &h->d_tabi, &h->d_ud, &h->d_yd, &h->d_up, &h->d_yp, &h->d_uopt,
                    &h->d_cost, &h->d_status, &h->d_iters, &h->d_beta, &h->d_act, &h->d_out, &h->d_stamps,
                    &h->d_pl, &h->d_x, &h->d_w, &h->d_usys, &h->d_ysys, &h->d_stacc,
                    &h->d_lfac, &h->d_lfacT, &h->d_gain, &h->d_prep_status, &h->d_zero, &h->d_dmat, &h->d_need, &h->d_io, &h->d_rr, &h->d_alpha, &h->d_zws, &h->d_resc, &h->d_xws, &h->d_rflag, &h->d_rrmeta, &h->d_gpre, &h->d_perm, &h->d_rr2d, &h->d_rr2res, &h->d_rr2mt, &h->d_rr2v, &h->d_rr2zp, &h->d_rr2sc, &h->d_wz, &h->d_gz, &h->d_gres, &h->d_zvirt, &h->d_rr3w, &h->d_rr3k, &h->d_large_seed, &h->d_rr_fb, &h->d_rrmeta_fb, &h->d_rr2cand, &h->d_rr2tol, &h->d_rr2rank, &h->d_wd, &h->d_rr2y,
                    &h->d_mcol, &h->d_cwl_tab, &h->d_cwl_sg, &h->d_cwl_ref, &h->d_r3y, &h->d_r3res, &h->d_r3zp, &h->d_r3flag,
                    &h->d_box_bd, &h->d_ubnd, &h->d_ybnd, &h->d_r3bi, &h->d_r3bd, &h->s_gain, &h->s_prep_status, &h->s_mcol, &h->s_cwl_ref, &h->d_lwup, &h->d_lwyp,
                    &h->d_box_seed, &h->d_ibnd, &h->d_sgain, &h->d_sptab, &h->d_sp, &h->d_uref, &h->d_yref, &h->d_chbnd};
  for (DevBuf* b : bufs) b->release();
  h->h_io.release();
  h->h_flag.release();
  if (h->ev_flag) (void)hipEventDestroy(h->ev_flag);
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return DDMPC_OK;
}

int ddmpc_set_stream(ddmpc_handle* h, void* hip_stream) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (h->stream == (hipStream_t)hip_stream && !h->own_stream) return DDMPC_OK;     // unchanged: nothing to order
  (void)hipSetDevice(h->device);
  // work already queued on the old stream must precede what is queued on the new one: order the two streams with
  // an event on the device instead of blocking the host
  if (h->stream != (hipStream_t)hip_stream) {
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, h->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)hip_stream, ev, 0);
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) return fail(DDMPC_ERR_HIP, "ddmpc_set_stream: %s", hipGetErrorString(e));
  }
  if (h->own_stream && h->stream) {
    HIP_TRY(hipStreamSynchronize(h->stream));           // only the handle's own stream is destroyed (once)
    (void)hipStreamDestroy(h->stream);
  }
  h->stream = (hipStream_t)hip_stream;
  h->own_stream = false;
  return DDMPC_OK;
}

int ddmpc_synchronize(ddmpc_handle* h) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  (void)hipSetDevice(h->device);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return DDMPC_OK;
}

int ddmpc_set_data(ddmpc_handle* h, const double* u_d, const double* y_d, int mem) {
  if (!h || !u_d || !y_d) return fail(DDMPC_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(h->device));
  const size_t nu = (size_t)h->batch * h->prm.N * h->prm.m * sizeof(double);
  const size_t ny = (size_t)h->batch * h->prm.N * h->prm.p * sizeof(double);
  if (mem == DDMPC_MEM_HOST) {
    int rc;
    if ((rc = h->d_ud.ensure(nu))) return rc;
    if ((rc = h->d_yd.ensure(ny))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_ud.p, u_d, nu, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_yd.p, y_d, ny, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->ud = (const double*)h->d_ud.p;
    h->yd = (const double*)h->d_yd.p;
  } else if (mem == DDMPC_MEM_DEVICE) {
    h->ud = u_d;
    h->yd = y_d;
  } else {
    return fail(DDMPC_ERR_INVALID, "mem must be DDMPC_MEM_HOST or DDMPC_MEM_DEVICE");
  }
  h->have_data = true;
  h->last.valid = false;
  forget_prep(h);
  h->gpre_valid = false;
  return DDMPC_OK;
}

static unsigned large_threads(size_t r) {   // workgroup size of the global-workspace kernels: the packed Cholesky keeps
  return r <= 256 ? 256u : (r <= 1024 ? 512u : 1024u);           // r <= PSD_RPT * threads (blocked substitutions)
}

// Workgroup size of the warm-path kernels (the affine law): a thread per component, 1024 at most.
static unsigned warm_threads(int r) { return (unsigned)std::min(((r + 63) / 64) * 64, 1024); }

// Next launch stamp of the AUTO refinement flags (flag[b] == stamp <=> instance b was flagged by THIS launch; the counter word
// holds the largest stamp that flagged anything).  Stamps only grow, so nothing is cleared between launches -- except
// before the 32-bit stamp would wrap, when the flags and the counter are zeroed once and the stamps restart.
static int next_refine_epoch(ddmpc_handle* h) {
  if (h->epoch >= 0x3fffffff &&
      (!h->d_rflag.p || hipMemsetAsync(h->d_rflag.p, 0, h->d_rflag.bytes, h->stream) == hipSuccess))
    h->epoch = 0;
  return ++h->epoch;
}

// Structured Gram of the phase pipelines (rr2_gram_kernel; plants of at most eight channels: several lags per matrix tile).
static void launch_rr2_gram(hipStream_t st, const KParams& k, const double* ud, const double* yd, const int* iperm, double* ws, long long stride,
                            int n16, unsigned long long* dd, size_t nb) {
  const dim3 grid(rr2_gram_grid(k.Ln, k.nch), (unsigned)nb);
  if (k.nch <= 8) hipLaunchKernelGGL(rr2_gram_packed_kernel, grid, dim3(256), 0, st, k, ud, yd, iperm, ws, stride, n16, dd);
  else hipLaunchKernelGGL(rr2_gram_kernel, grid, dim3(256), 0, st, k, ud, yd, iperm, ws, stride, n16, dd);
}

// Structured Gram for channel counts other than four: the Gram tiles of `nb` instances (data at ud / yd) into slots b0 .. of
// the handle's buffer, and the pointers into `kq`.  cacheable: the data set is the handle's (h->ud / h->yd) -- one launch serves
// every cold-kernel launch until the data may have changed (ddmpc_set_data, ddmpc_solve, ddmpc_solve_from_host, ddmpc_prepare
// clear gpre_valid; ddmpc_step and ddmpc_get_solution work on the data ddmpc_prepare / the last solve saw).
static int gram_pre_launch(ddmpc_handle* h, KParams& kq, const double* ud, const double* yd, size_t nb, size_t b0, bool cacheable) {
  if (!h->gram_pre) return DDMPC_OK;
  const int NT = h->kc.NT;
  const long long stride = (long long)(NT * (NT + 1) / 2) * 256;
  int rc;
  if ((rc = h->d_gpre.ensure((size_t)h->batch * (size_t)stride * sizeof(double)))) return rc;
  kq.gpre = (const double*)h->d_gpre.p + (long long)b0 * stride;
  kq.gpre_stride = stride;
  if (cacheable && h->gpre_valid) return DDMPC_OK;
  if (h->long_data || h->gram_launch == 0) {
    // streaming Gram on the matrix pipe (trajectory in chunks through LDS, several lags per tile for plants of at most eight
    // channels), written straight into the tiles
    const dim3 grid(rr2_gram_grid(h->kp.Ln, h->kp.nch), (unsigned)nb);
    double* gp = (double*)h->d_gpre.p + (long long)b0 * stride;
    if (h->kp.nch == 4)                     // the four-tank plant of the reference's example: lag blocks on v_mfma_f64_4x4x4
      hipLaunchKernelGGL(rr2_gram_tiles_c4_kernel, dim3((unsigned)(((h->kp.Ln + 3) / 4 + 4 * RR2_C4_SL - 1) / (4 * RR2_C4_SL)), (unsigned)nb), dim3(256), 0,
                         h->stream, h->kp, ud, yd, gp, stride, 16 * NT);
    else if (h->kp.nch <= 8) hipLaunchKernelGGL(rr2_gram_tiles_packed_kernel, grid, dim3(256), 0, h->stream, h->kp, ud, yd, gp, stride, 16 * NT);
    else hipLaunchKernelGGL(rr2_gram_tiles_kernel, grid, dim3(256), 0, h->stream, h->kp, ud, yd, gp, stride, 16 * NT);
    HIP_TRY(hipGetLastError());
    if (cacheable) h->gpre_valid = true;
    return DDMPC_OK;
  }
  const size_t lds = gram_tiles_lds_doubles(h->kp.xs_len, h->kp.r, h->kp.nch, NT) * sizeof(double);
  if (lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)ddmpc_gram_tiles_kernel, lds));
  hipLaunchKernelGGL(ddmpc_gram_tiles_kernel, dim3((unsigned)nb), dim3(256), lds, h->stream, h->kp, NT, ud, yd,
                     (double*)h->d_gpre.p + (long long)b0 * stride, stride);
  HIP_TRY(hipGetLastError());
  if (cacheable) h->gpre_valid = true;
  return DDMPC_OK;
}

// The product H (H' v) of the phase pipelines: on the matrix pipe when the shape allows it (up to 16 channels, at most 8 tiles
// per half, LDS within reach), with as many workgroups per instance as leave >= 64 columns each; else the plain kernel (ng 0).
struct HankelLaunch { int ng = 0; size_t lds = 0; };
static int pick_hankel_launch(const KParams& k, HankelLaunch* hk) {
  if (k.nch > 16) return DDMPC_OK;
  for (int ng = RR2_NG; ng >= 1 && hk->ng == 0; --ng) {
    const Rr2HankelGeom G = rr2_hankel_geom(k.c, k.Ln, k.nch, ng);
    const size_t bytes = rr2_hankel_mfma_lds(G, k.Ln) * sizeof(double);
    if ((G.cg >= 64 || ng == 1) && bytes <= 80 * 1024 && G.ntA <= 8 && G.ntZ <= 8) { hk->ng = ng; hk->lds = bytes; }
  }
  if (hk->ng && hk->lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)rr2_hankel_mfma_kernel, hk->lds));
  return DDMPC_OK;
}
// (RR2_NG workgroups per instance whatever hk.ng is: the consumers sum RR2_NG partial results, and a workgroup past the last
//  column group writes the zeros they expect -- launched with hk.ng < RR2_NG workgroups, short trajectories summed whatever the
//  allocator had left in the other slots)
static void launch_hankel(const HankelLaunch& hk, hipStream_t st, unsigned nb, const Rr2Solve& S, const KParams& k,
                          const double* ud, const double* yd, int slot, int pass) {
  if (hk.ng) hipLaunchKernelGGL(rr2_hankel_mfma_kernel, dim3((unsigned)RR2_NG, nb), dim3(512), hk.lds, st, S, k, ud, yd, slot, pass, hk.ng);
  else hipLaunchKernelGGL(rr2_hankel_kernel, dim3((unsigned)RR2_NG, nb), dim3(512), 0, st, S, k, ud, yd, slot, pass);
}

// Doubles of the Minv blocks (64 x 64 diagonal blocks) of one instance's factor of n16 rows (ddmpc_rr2.hpp).
static long long rr2_m64(int n16) { return (long long)((n16 + RR2_NB - 1) / RR2_NB) * RR2_NB * RR2_NB; }
// Per-instance workspace slices of the phase pipelines (whole 16-row tiles): the packed factor of G (ROBUST), those of G and T
// (NOMINAL; the one-workgroup kernel keeps the same slices when they do not fit its LDS).
static long long rr3_ndbl(const ddmpc_handle* h) { return (long long)pk_size(((size_t)h->kp.r + 15) & ~(size_t)15); }
static long long rr2_ndbl(const ddmpc_handle* h) { return rr3_ndbl(h) + (long long)pk_size(((size_t)h->n_free + 15) & ~(size_t)15); }
// Per-instance workspace slice of ddmpc_large_solve_kernel (packed rows, then the lag sums or the Schur block of the components
// the slack box acts on), on a 128-byte boundary.
static size_t large_robust_stride(const KParams& k, const ddmpc_params& p) {
  const size_t nB = k.convex ? (size_t)p.p * p.L : 0, nlag = (size_t)k.Ln * k.nch * k.nch, sb = 2 * pk_size(nB);
  return (pk_size((size_t)k.r) + (nlag > sb ? nlag : sb) + 15) & ~(size_t)15;
}

// Lock-step Cholesky of the phase pipelines by 64-column panels: a panel launch, then the update of the row tiles below it.
static void launch_rr2_cholesky(hipStream_t st, const Rr2Chol& F, int n16, size_t B) {
  const int nt = n16 >> 4;
  for (int c0 = 0; c0 < n16; c0 += RR2_NB) {
    hipLaunchKernelGGL(rr2_chol_panel_kernel, dim3(1, (unsigned)B), dim3(256), 0, st, F, c0);
    const int nbelow = nt - (c0 >> 4) - 4;                 // row tiles below the diagonal block
    if (nbelow > 0)
      hipLaunchKernelGGL(rr2_chol_update_kernel<RR2_UT>, dim3((unsigned)((nbelow + 4 * RR2_UT - 1) / (4 * RR2_UT)), (unsigned)B),
                         dim3(256), 0, st, F, c0);
  }
}

// ---- ROBUST controllers beyond the register-resident kernels on the phase kernels (ddmpc_rr3.hpp) ----------------------------
// What depends on the data and the weights alone: G (boxed components last) + lam D0, its Cholesky factor with the Minv blocks.
static int launch_rr3_factors(ddmpc_handle* h) {
  const KParams& k = h->kp;
  const int r = k.r, n16 = (r + 15) & ~15, rv = (r + 1) & ~1;
  const long long ndbl = rr3_ndbl(h), mstride = 2 * (long long)rv + 2;
  const size_t B = (size_t)h->batch;
  const long long m64G = rr2_m64(n16);
  int rc;
  if ((rc = h->d_rr.ensure(B * (size_t)ndbl * sizeof(double))) || (rc = h->d_rrmeta.ensure(B * (size_t)mstride * sizeof(int))) ||
      (rc = h->d_rr2d.ensure(B * 4 * sizeof(unsigned long long))) || (rc = h->d_rr2mt.ensure(B * (size_t)m64G * sizeof(double))))
    return rc;
  HIP_TRY(hipMemsetAsync(h->d_rr2d.p, 0, B * 4 * sizeof(unsigned long long), h->stream));
  unsigned long long* dd = (unsigned long long*)h->d_rr2d.p;
  const int* perm = (const int*)h->d_perm.p;
  double* scratch = (double*)h->d_rr.p;
  launch_rr2_gram(h->stream, k, h->ud, h->yd, perm + rv, scratch, ndbl, n16, dd, B);
  hipLaunchKernelGGL(rr3_shift_kernel, dim3((unsigned)B), dim3(256), 0, h->stream, k, 16 * h->kc.NT, perm, scratch, ndbl);
  Rr2Chol FG{};
  FG.ws = scratch; FG.stride = ndbl; FG.off = 0; FG.n16 = n16; FG.n_inst = nullptr; FG.n_stride = 0;
  FG.dmax = dd + 0; FG.d_stride = 4; FG.tol_rel = 0.0; FG.skip = (int*)h->d_rrmeta.p; FG.s_stride = mstride; FG.nflag = r;
  FG.live = dd + 2; FG.l_stride = 4; FG.m64 = (double*)h->d_rr2mt.p; FG.m64_stride = m64G;
  FG.res = nullptr; FG.res_stride = 0; FG.dead = nullptr; FG.dead_stride = 0;
  launch_rr2_cholesky(h->stream, FG, n16, B);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// What fixes the kernels and the memory layout of one solve on the kept factors, decided here and nowhere else.
//   Plain    rr3_solve_kernel: no input / output bounds.  Instances it marks 5 go to the fall-back (launch_rr3_fallback).
//   Box      rr3_solve_box_kernel: the instantiations that test the component table, RR3_KMAX columns of W.  No fall-back kernel
//            knows the bounds (an instance beyond RR3_KMAX active components ends in status 4 inside the kernel).
//   BoxWide  rr3_solve_box_wide_kernel (ddmpc_rr3_box_wide.hpp), the twin with `capacity` columns of W and the tiled k x k system:
//            DDMPC_OPT_LARGE_BOX_CAPACITY above 64, DDMPC_OPT_LARGE_BOX_SAFEGUARD at every capacity (64 included: the safeguard
//            writes one layout of W, tiles and record) and DDMPC_OPT_LARGE_BOX_WARM_START (the seeded instantiation is that kernel's).
enum class Rr3Family { Plain, Box, BoxWide };
struct Rr3Plan {
  Rr3Family family;
  int cap;                     // columns of W per instance
  size_t lds;                  // dynamic LDS of every solve and safeguard launch, bytes
  int nA, ldw;                 // rows ahead of the trailing block; leading dimension of W
  long long wstride, kstride;  // per instance: doubles of W and the k x k system, ints of the record
  bool filtered;               // DDMPC_OPT_LARGE_BOX_LAW: the instantiations with the instance filter (Rr3Only)
  bool seed_read;              // DDMPC_OPT_LARGE_BOX_WARM_START with a valid seed: the seeded instantiation (without one, the kernel of the option 0)
  bool seed_kept;              // ... every call leaves its set in d_large_seed (rr3_box_keep_seed_kernel)
  bool safeguard;              // DDMPC_OPT_LARGE_BOX_SAFEGUARD: rr3_box_safeguard_kernel behind the solve launch
};

// Ints of the per-instance record: [k, state, iterations, k, switched positions (cap), active set (rv), start tick, ticks, peak k].
static long long rr3_kstride(int cap, int rv) { return 4 + cap + rv + 4; }

// setpoints: a call of DDMPC_OPT_LARGE_SETPOINT_BOUNDS, which honours neither the warm start nor the law (the kernels of a handle
// with both options 0).
static Rr3Plan rr3_plan(const ddmpc_handle* h, const KParams& kq, bool filtered = false, bool seeded = false, bool setpoints = false) {
  const int r = kq.r, rv = (r + 1) & ~1;
  const bool warm = h->large_box_warm != 0 && !setpoints;
  const bool wide = h->bounded && (h->large_box_cap > RR3_KMAX || h->large_box_safeguard != 0 || warm);
  Rr3Plan P{};
  P.family = wide ? Rr3Family::BoxWide : h->bounded ? Rr3Family::Box : Rr3Family::Plain;
  P.cap = wide ? h->large_box_cap : RR3_KMAX;
  P.lds = ((size_t)Rr3Lds::make(r).total + (wide ? (size_t)rr3w_lds_extra(P.cap) : h->bounded ? (size_t)RR3_BOX_LDS : 0)) * sizeof(double);
  P.nA = (kq.convex || h->bounded) ? h->nA3 : r;
  P.ldw = ((r - (P.nA & ~63)) + 63) & ~63;
  P.filtered = filtered;
  P.seed_read = wide && warm && seeded;
  P.seed_kept = wide && warm;
  P.safeguard = wide && h->large_box_safeguard;
  // W with cap columns, then the k x k system: one (RR3_KMAX + 1)-strided block, or the 64 x 64 tiles of the wide kernel -- and
  // behind them what rr3_box_safeguard_kernel keeps: the unfactored tiles, v, the entering column
  P.wstride = (long long)P.cap * P.ldw + (wide ? rr3w_tiles(P.cap) * 4096 : (long long)RR3_KMAX * (RR3_KMAX + 1));
  if (P.safeguard) P.wstride += rr3s_extra(P.cap, h->nbox3, P.ldw);
  P.kstride = rr3_kstride(P.cap, rv);
  return P;
}

// The table of boxed components of a bounded handle, as the kernels take it.
static Rr3Box rr3_box(const ddmpc_handle* h) {
  Rr3Box X{};
  X.nbox = h->nbox3; X.ip = (const int*)h->d_r3bi.p; X.bd = (const double*)h->d_r3bd.p;
  return X;
}

// The descriptor of the kept factors and of the solve's workspace (sized here, by the plan).
static int rr3_desc(ddmpc_handle* h, const KParams& kq, Rr3* out, bool setpoints = false) {
  const int r = kq.r, n16 = (r + 15) & ~15, rv = (r + 1) & ~1, VL = (r + 63) & ~63;
  const size_t B = (size_t)h->batch;
  const long long m64G = rr2_m64(n16);
  const Rr3Plan P = rr3_plan(h, kq, false, false, setpoints);
  int rc;
  if (P.seed_kept && (rc = h->d_large_seed.ensure(B * (size_t)kq.rE))) return rc;
  if ((rc = h->d_rr2v.ensure(B * (size_t)R3_NV * VL * sizeof(double))) || (rc = h->d_rr2zp.ensure(B * (size_t)RR2_NG * VL * sizeof(double))) ||
      (rc = h->d_rr3w.ensure(B * (size_t)P.wstride * sizeof(double))) || (rc = h->d_rr3k.ensure(B * (size_t)P.kstride * sizeof(int))) ||
      (rc = h->d_beta.ensure(B * (size_t)kq.rE * sizeof(double))) || (rc = h->d_act.ensure(B * (size_t)kq.rE)))
    return rc;
  Rr3& S = *out;
  S = Rr3{};
  S.ws = (const double*)h->d_rr.p; S.stride = rr3_ndbl(h);
  S.m64 = (const double*)h->d_rr2mt.p; S.m64_stride = m64G;
  S.skip = (const int*)h->d_rrmeta.p; S.s_stride = 2 * (long long)rv + 2;
  S.dd = (const unsigned long long*)h->d_rr2d.p;
  S.perm = (const int*)h->d_perm.p;
  S.rv = rv; S.r = r; S.nA = P.nA; S.n0 = P.nA & ~63;
  S.V = (double*)h->d_rr2v.p; S.vstride = (long long)R3_NV * VL; S.VL = VL;
  S.ZP = (double*)h->d_rr2zp.p;
  S.Wg = (double*)h->d_rr3w.p; S.wstride = P.wstride; S.ldw = P.ldw;
  S.kq = (int*)h->d_rr3k.p; S.kstride = P.kstride;
  return DDMPC_OK;
}

// Dynamic LDS of the one-workgroup kernels (ddmpc_large_solve_kernel, ddmpc_large_solve_wide_kernel), bytes.
static size_t large_solve_lds(size_t r) {
  const size_t rv = (r + 1) & ~(size_t)1;
  return 6 * rv * sizeof(double) + 4 * rv * sizeof(int) + (size_t)PSD_PAN * sizeof(double);
}

// Instances the unbounded phase solve marked 5 (more switched components than W holds, a failed pivot of the k x k system): the
// one-workgroup kernel of rounds 1-4 solves them from scratch in a workspace of its own; every other workgroup leaves at once.
static int launch_rr3_fallback(ddmpc_handle* h, const KParams& kq, const double* up, const double* yp, double* uo, double* cost,
                               int32_t* status, int32_t* iters) {
  const size_t B = (size_t)h->batch, r = (size_t)kq.r, stride = large_robust_stride(kq, h->prm);
  const size_t nfb = B < 8 ? B : 8;                         // (one slice of workspace per workgroup of the fall-back grid)
  int rc;
  if ((rc = h->d_rr_fb.ensure(nfb * stride * sizeof(double))) || (rc = h->d_rrmeta_fb.ensure(nfb * sizeof(int)))) return rc;
  const size_t lds = large_solve_lds(r);
  if (lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)ddmpc_large_solve_kernel<0>, lds));
  hipLaunchKernelGGL(ddmpc_large_solve_kernel<0>, dim3((unsigned)nfb), dim3(large_threads(r)), lds, h->stream, kq, 16 * h->kc.NT, h->ud, h->yd,
                     up, yp, uo, cost, (int*)status, (int*)iters, (double*)h->d_beta.p, (signed char*)h->d_act.p, (double*)h->d_rr_fb.p,
                     (long long)stride, (int*)h->d_rrmeta_fb.p, 5, (long long)B);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// The solve on those factors (what a control step repeats, controller.py:389-407).  only (nullptr: the whole batch): per-instance
// flags of the law step, the solve launches leave every other instance alone -- on a bounded handle (DDMPC_OPT_LARGE_BOX_LAW) by
// the filtered instantiations, the same launches for the instances the law step flagged.  seeded (DDMPC_OPT_LARGE_BOX_WARM_START
// = 1 on a bounded handle only): the iteration starts from the set in d_large_seed; with the option 1 every call leaves its set
// there.  sp (the setpoint calls beyond 271 rows): a setpoint per instance -- on a bounded handle the setpoint instantiations of
// the bounded kernels over the whole batch, from the empty set, no seed read or kept; else rr3_solve_kernel's.
static int launch_rr3_solve(ddmpc_handle* h, const KParams& kq, const double* up, const double* yp, double* uo, double* cost,
                            int32_t* status, int32_t* iters, const int* only = nullptr, int* only_si = nullptr, bool seeded = false,
                            const Rr3Setpoint* sp = nullptr) {
  const int r = kq.r;
  const unsigned B = (unsigned)h->batch;
  const Rr3Plan P = rr3_plan(h, kq, only != nullptr, seeded, sp != nullptr);
  Rr3 S;
  int rc;
  if ((rc = rr3_desc(h, kq, &S, sp != nullptr))) return rc;
  h->last.box_cap = P.cap;
  const int RPs = 16 * h->kc.NT;
  const bool refine = kq.refine != DDMPC_REFINE_OFF && kq.lam != 0.0;
  const Rr3Box X = rr3_box(h);
  const Rr3Only flt{only};
  const Rr3Seed seed{(const signed char*)h->d_large_seed.p, P.safeguard ? 1 : 0};
  auto launch = [&](auto kernel, int defer_outputs, auto... tail) -> int {
    if (P.lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)kernel, P.lds));
    hipLaunchKernelGGL(kernel, dim3(B), dim3(RR2_TS), P.lds, h->stream, S, kq, RPs, up, yp, uo, cost, (int*)status, (int*)iters,
                       (double*)h->d_beta.p, (signed char*)h->d_act.p, defer_outputs, tail...);
    return DDMPC_OK;
  };
  const bool wide = P.family == Rr3Family::BoxWide, box = P.family == Rr3Family::Box, F = P.filtered;
  const int defer = refine ? 1 : 0;
  if (sp && (wide || box) && F) return fail(DDMPC_ERR_UNSUPPORTED, "the bounded solve with setpoints takes no instance filter");
  if      (wide && sp)               rc = launch(rr3_solve_box_wide_kernel<false, Rr3Setpoint>, defer, X, P.cap, *sp);
  else if (box && sp)                rc = launch(rr3_solve_box_kernel<false, Rr3Setpoint>, defer, X, *sp);
  else if (wide && P.seed_read && F) rc = launch(rr3_solve_box_wide_kernel<false, Rr3Seed, Rr3Only>, defer, X, P.cap, seed, flt);
  else if (wide && P.seed_read)      rc = launch(rr3_solve_box_wide_kernel<false, Rr3Seed>, defer, X, P.cap, seed);
  else if (wide && F)                rc = launch(rr3_solve_box_wide_kernel<false, Rr3Only>, defer, X, P.cap, flt);
  else if (wide)                     rc = launch(rr3_solve_box_wide_kernel<false>, defer, X, P.cap);
  else if (box && F)                 rc = launch(rr3_solve_box_kernel<false, Rr3Only>, defer, X, flt);
  else if (box)                      rc = launch(rr3_solve_box_kernel<false>, defer, X);
  else if (sp)                       rc = launch(rr3_solve_kernel<false, Rr3Setpoint>, defer, only, *sp);   // (Plain: no finite bounds on the handle)
  else                               rc = launch(rr3_solve_kernel<false>, defer, only);
  if (rc) return rc;
  // the instances that reached max_iter are solved again by the primal method, before the Hankel products and the refinement
  // launch; every other workgroup leaves at once
  if (P.safeguard && sp) rc = launch(rr3_box_safeguard_kernel<Rr3Setpoint>, defer, X, P.cap, *sp);
  else if (P.safeguard && F) rc = launch(rr3_box_safeguard_kernel<Rr3Only>, defer, X, P.cap, flt);
  else if (P.safeguard) rc = launch(rr3_box_safeguard_kernel<>, defer, X, P.cap);
  if (rc) return rc;
  if (refine) {
    // H (H' beta) with exact products (the Hankel kernels of the NOMINAL pipeline: they read slot R3_X of the vectors)
    Rr2Solve H{};
    H.V = S.V; H.vstride = S.vstride; H.VL = S.VL; H.ZP = S.ZP; H.fdiv = 1; H.r = r;
    H.si = only_si;                                       // (the filtered re-solve: only the flagged instances, pass > 0 skips the rest)
    HankelLaunch hk;
    if ((rc = pick_hankel_launch(kq, &hk))) return rc;
    launch_hankel(hk, h->stream, B, H, kq, h->ud, h->yd, (int)R3_X, only_si != nullptr ? 1 : 0);
    if      (wide && sp) rc = launch(rr3_solve_box_wide_kernel<true, Rr3Setpoint>, 0, X, P.cap, *sp);
    else if (box && sp)  rc = launch(rr3_solve_box_kernel<true, Rr3Setpoint>, 0, X, *sp);
    else if (wide && F) rc = launch(rr3_solve_box_wide_kernel<true, Rr3Only>, 0, X, P.cap, flt);
    else if (wide)      rc = launch(rr3_solve_box_wide_kernel<true>, 0, X, P.cap);
    else if (box && F)  rc = launch(rr3_solve_box_kernel<true, Rr3Only>, 0, X, flt);
    else if (box)       rc = launch(rr3_solve_box_kernel<true>, 0, X);
    else if (sp)        rc = launch(rr3_solve_kernel<true, Rr3Setpoint>, 0, only, *sp);
    else                rc = launch(rr3_solve_kernel<true>, 0, only);
    if (rc) return rc;
  }
  if (P.seed_kept) {
    // the signed set the call finally reported (the solve, safeguard or refinement launch wrote it last) becomes the next step's seed
    hipLaunchKernelGGL(rr3_box_keep_seed_kernel, dim3(B), dim3(256), 0, h->stream, r, kq.rE, (const int*)status,
                       (const signed char*)h->d_act.p, (signed char*)h->d_large_seed.p);
    h->last.large_seed = true;
  }
  HIP_TRY(hipGetLastError());
  // (with setpoints: no fall-back, it solves from the shared table -- the kernel reported the instances it marked 5 as 4)
  return P.family == Rr3Family::Plain && !sp ? launch_rr3_fallback(h, kq, up, yp, uo, cost, status, iters) : DDMPC_OK;
}

// The per-instance flags of the law on Route::RobustPhases, d_r3flag (7 B ints): [no law | need | refine | si (2 B) | no setpoint
// law | refine S].
struct Rr3Flags {
  int *nolaw, *need, *rfl;     // the law missed the threshold; the step left the instance to the solve; the law build's refinement passes
  int* si;                     // [2 B]: need in the layout of Rr2Solve::si
  int *nosp, *rfs;             // DDMPC_OPT_LARGE_SETPOINTS: S missed the threshold (apart from nolaw: ddmpc_step does not read it); S's refinement passes
};
static Rr3Flags rr3_flags(const ddmpc_handle* h) {
  int* f = (int*)h->d_r3flag.p;
  const size_t B = (size_t)h->batch;
  return Rr3Flags{f, f + B, f + 2 * B, f + 3 * B, f + 5 * B, f + 6 * B};
}

// DDMPC_OPT_LARGE_AFFINE_LAW on Route::RobustPhases (ddmpc_rr3_law.hpp): the law beta(w) = g0 + G' w of every instance on the
// kept factor -- all n(m+p) + 1 right-hand sides by multi-column substitutions on the matrix pipe, then (refinement on) passes of
// exact-Hankel residuals and corrections through the same kernels.  Chunks of instances bound the virtual batch of the Hankel
// product (grid rows) and the scratch.  An instance whose law misses the threshold after refine_max passes is marked "no law".
static int launch_rr3_law_build(ddmpc_handle* h) {
  const KParams& k = h->kp;
  const int r = k.r, nf = h->prm.n * k.nch, nrhs = nf + 1, ncb = (nrhs + 63) / 64, VL = (r + 63) & ~63;
  if (nf > WARM_MAX_NF) return fail(DDMPC_ERR_UNSUPPORTED, "the affine law supports n*(m+p) <= %d", WARM_MAX_NF);
  const size_t B = (size_t)h->batch;
  const size_t Bc = std::min<size_t>(B, std::min<size_t>(32, (size_t)(65535 / nrhs)));
  const bool refine = k.refine != DDMPC_REFINE_OFF && k.lam != 0.0;
  const bool with_s = h->large_setpoints != 0 && h->large_affine != 0;    // DDMPC_OPT_LARGE_SETPOINTS: S next to the law
  Rr3 S;
  int rc;
  if ((rc = rr3_desc(h, k, &S))) return rc;
  if ((rc = h->d_gz.ensure((B * nrhs * (size_t)r + VL) * sizeof(double))) || (rc = h->d_r3flag.ensure(7 * B * sizeof(int))) ||
      (rc = h->d_r3y.ensure(Bc * ncb * (size_t)VL * 64 * sizeof(double))))
    return rc;
  if (with_s && (rc = h->d_sgain.ensure((B * k.nch * (size_t)r + VL) * sizeof(double)))) return rc;
  if (refine && ((rc = h->d_r3res.ensure(Bc * nrhs * (size_t)r * sizeof(double))) ||
                 (rc = h->d_r3zp.ensure(Bc * nrhs * (size_t)RR2_NG * VL * sizeof(double)))))
    return rc;
  HankelLaunch hk;
  if (refine && (rc = pick_hankel_launch(k, &hk))) return rc;
  const int RPs = 16 * h->kc.NT;
  double* Y = (double*)h->d_r3y.p;
  std::vector<int> fl(Bc);
  // One set of right-hand sides through the three kernels, chunk by chunk: the law (RR3_RHS_LAW: nf + 1 columns into d_gz, flags
  // nolaw / rfl), then -- apart from it, with flags of its own, so that the law's launches and the refinement decisions taken
  // on it are those of a handle without the option -- S (RR3_RHS_SETPOINT: m + p columns into d_sgain, flags nosp / rfs).  The
  // scratch (Y, residuals, Hankel sums) is sized by the law, which has the more columns.  *missed: instances above the threshold.
  auto build = [&](int kind, int ncol, double* dst, int* nol, int* rfl, int* missed) -> int {
    const int nfk = kind == RR3_RHS_SETPOINT ? ncol : ncol - 1;            // (the kernels' count: columns of S, or windows of the law)
    const int ncbk = (ncol + 63) / 64;
    HIP_TRY(hipMemsetAsync(nol, 0, B * sizeof(int), h->stream));
    for (size_t b0 = 0; b0 < B; b0 += Bc) {
      const size_t nb = std::min(Bc, B - b0);
      const dim3 grid((unsigned)ncbk, (unsigned)nb);
      hipLaunchKernelGGL(rr3_law_fwd_kernel<false>, grid, dim3(RR2_TS), 0, h->stream, S, k, RPs, (long long)b0, nfk, (const double*)nullptr,
                         (const int*)nullptr, Y, nol, kind);
      hipLaunchKernelGGL(rr3_law_bwd_kernel<false>, grid, dim3(RR2_TS), 0, h->stream, S, (long long)b0, nfk, (const int*)nullptr, Y, dst, nol, kind);
      HIP_TRY(hipGetLastError());
      if (!refine) continue;
      Rr2Solve H{};
      H.V = dst + b0 * ncol * (size_t)r; H.vstride = r; H.VL = VL; H.ZP = (double*)h->d_r3zp.p; H.fdiv = ncol; H.r = r;
      for (int pass = 0;; ++pass) {
        const bool last = pass == k.refine_max, force = pass == 0 && k.refine == DDMPC_REFINE_ALWAYS;
        HIP_TRY(hipMemsetAsync(rfl + b0, 0, nb * sizeof(int), h->stream));
        launch_hankel(hk, h->stream, (unsigned)(nb * ncol), H, k, h->ud + b0 * (size_t)k.N * k.m, h->yd + b0 * (size_t)k.N * k.p, 0, 0);
        hipLaunchKernelGGL(rr3_law_resid_kernel, dim3((unsigned)ncol, (unsigned)nb), dim3(256), 0, h->stream, k, RPs, (long long)b0, nfk,
                           (const double*)dst, (const double*)h->d_r3zp.p, VL, (double*)h->d_r3res.p, rfl, force ? 1 : 0,
                           last ? nol : nullptr, kind);
        HIP_TRY(hipGetLastError());
        if (last) break;
        HIP_TRY(hipMemcpyAsync(fl.data(), rfl + b0, nb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        bool any = false;
        for (size_t i = 0; i < nb; ++i) any = any || fl[i] != 0;
        if (!any) break;                                      // every column set of the chunk is within the threshold
        hipLaunchKernelGGL(rr3_law_fwd_kernel<true>, grid, dim3(RR2_TS), 0, h->stream, S, k, RPs, (long long)b0, nfk,
                           (const double*)h->d_r3res.p, (const int*)rfl, Y, nol, kind);
        hipLaunchKernelGGL(rr3_law_bwd_kernel<true>, grid, dim3(RR2_TS), 0, h->stream, S, (long long)b0, nfk, (const int*)rfl, Y, dst, nol, kind);
        HIP_TRY(hipGetLastError());
      }
    }
    std::vector<int> nl(B);
    HIP_TRY(hipMemcpyAsync(nl.data(), nol, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *missed = 0;
    for (size_t i = 0; i < B; ++i) *missed += nl[i] != 0;
    return DDMPC_OK;
  };
  const Rr3Flags F = rr3_flags(h);
  if ((rc = build(RR3_RHS_LAW, nrhs, (double*)h->d_gz.p, F.nolaw, F.rfl, &h->prep.r3_nolaw))) return rc;
  h->prep.law = true;
  if (with_s) {
    if ((rc = build(RR3_RHS_SETPOINT, k.nch, (double*)h->d_sgain.p, F.nosp, F.rfs, &h->prep.r3_nosp))) return rc;
    h->prep.setpoint = true;
  }
  return DDMPC_OK;
}

// DDMPC_OPT_LARGE_BOX_LAW: the law serves a bounded handle on Route::RobustPhases.
static bool rr3_box_law(const ddmpc_handle* h) { return h->large_box_law != 0 && h->large && !h->large_nominal && h->bounded; }

// The launch of a control step on that law over the batch: what the two step kernels share, box: that of a bounded handle, which
// takes the table and the capacity of the solve behind it.
static int launch_rr3_law_kernel(ddmpc_handle* h, bool box, const double* up, const double* yp, double* uo, double* cost,
                                 int32_t* status, int32_t* iters) {
  const KParams& k = h->kp;
  const Rr3Flags F = rr3_flags(h);
  Rr3 S;
  if (int rc = rr3_desc(h, k, &S)) return rc;
  auto launch = [&](auto kernel, auto... tail) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)h->batch), dim3(RR2_TS), 0, h->stream, S, k, 16 * h->kc.NT, h->prm.n * k.nch,
                       (const double*)h->d_gz.p, (const int*)F.nolaw, up, yp, uo, cost, (int*)status, (int*)iters, (double*)h->d_beta.p,
                       (signed char*)h->d_act.p, F.need, F.si, tail...);
  };
  if (box) launch(rr3_law_box_step_kernel, rr3_box(h), rr3_plan(h, k).cap);
  else launch(rr3_law_step_kernel);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// A control step on that law: one launch over the batch, then -- under the slack box, or when some instance has no law -- the solve
// on the kept factor restricted to the instances the step left to it.
static int launch_rr3_law_step(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                               int32_t* iters) {
  if (int rc = launch_rr3_law_kernel(h, false, up, yp, uo, cost, status, iters)) return rc;
  if (!h->kp.convex && h->prep.r3_nolaw == 0) return DDMPC_OK;
  return launch_rr3_solve(h, h->kp, up, yp, uo, cost, status, iters, rr3_flags(h).need, rr3_flags(h).si);
}

// DDMPC_OPT_LARGE_SETPOINTS with the law and S present: one launch of rr3_setpoint_law_step_kernel over the batch, then -- under the
// slack box, or when some instance has no law or no setpoint law -- the solve on the kept factor with the same setpoints,
// restricted to the instances the step left to it (queued without a read-back).
static int launch_rr3_setpoint_law_step(ddmpc_handle* h, const Rr3Setpoint& sp, const double* up, const double* yp, double* uo,
                                        double* cost, int32_t* status, int32_t* iters) {
  const KParams& k = h->kp;
  const Rr3Flags F = rr3_flags(h);
  Rr3 S;
  if (int rc = rr3_desc(h, k, &S)) return rc;
  hipLaunchKernelGGL(rr3_setpoint_law_step_kernel, dim3((unsigned)h->batch), dim3(RR2_TS), 0, h->stream, S, k, 16 * h->kc.NT,
                     h->prm.n * k.nch, (const double*)h->d_gz.p, (const int*)F.nolaw, up, yp, uo, cost, (int*)status, (int*)iters,
                     (double*)h->d_beta.p, (signed char*)h->d_act.p, F.need, F.si, (const double*)h->d_sgain.p, (const int*)F.nosp, sp);
  HIP_TRY(hipGetLastError());
  if (!k.convex && h->prep.r3_nolaw == 0 && h->prep.r3_nosp == 0) return DDMPC_OK;
  return launch_rr3_solve(h, k, up, yp, uo, cost, status, iters, F.need, F.si, false, &sp);
}

// DDMPC_OPT_LARGE_BOX_LAW (ddmpc_rr3_box_law.hpp): a control step of a bounded handle on that law -- one launch over the batch that
// serves the instances whose beta violates no component of the box table, then the bounded solve on the kept factor (the launches
// of the option 0) restricted to the instances the step left to it.  The solve launches are queued whatever the step found (no
// read-back between them): their workgroups leave at once for a served instance, and rr3_box_keep_seed_kernel behind them reads
// the empty set of a served instance like any other.
static int launch_rr3_law_box_step(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                                   int32_t* iters, bool seeded) {
  if (int rc = launch_rr3_law_kernel(h, true, up, yp, uo, cost, status, iters)) return rc;
  return launch_rr3_solve(h, h->kp, up, yp, uo, cost, status, iters, rr3_flags(h).need, rr3_flags(h).si, seeded);
}


// ROBUST controllers beyond the register-resident kernels (Route::RobustPhases, Route::RobustOneWg).
static int launch_large_robust(ddmpc_handle* h, Route route, Stage stage, const double* up, const double* yp, double* uo,
                               double* cost, int32_t* status, int32_t* iters, bool seeded = false) {
  int rc;
  if (route == Route::RobustPhases) {
    // lock-step factorisation of the whole batch, then one workgroup per instance that streams the factor twice and runs the
    // active-set iterations on its trailing block
    if (stage != Stage::OnFactors && (rc = launch_rr3_factors(h))) return rc;
    if (stage == Stage::OnFactors && h->large_affine && h->prep.law) return launch_rr3_law_step(h, up, yp, uo, cost, status, iters);
    if (stage == Stage::OnFactors && rr3_box_law(h) && h->prep.law) return launch_rr3_law_box_step(h, up, yp, uo, cost, status, iters, seeded);
    if (stage != Stage::Factors && (rc = launch_rr3_solve(h, h->kp, up, yp, uo, cost, status, iters, nullptr, nullptr, seeded))) return rc;
    return DDMPC_OK;
  }
  // the one-workgroup kernel: matrices in a per-instance slice of a global workspace
  const size_t r = (size_t)h->kp.r, stride = large_robust_stride(h->kp, h->prm);
  if ((rc = h->d_rr.ensure((size_t)h->batch * stride * sizeof(double))) ||
      (rc = h->d_beta.ensure((size_t)h->batch * h->kp.rE * sizeof(double))) || (rc = h->d_act.ensure((size_t)h->batch * h->kp.rE)))
    return rc;
  const size_t lds = large_solve_lds(r);
  if (lds + 1024 > 160 * 1024) return fail(DDMPC_ERR_UNSUPPORTED, "problem too large: %zu rows", r);
  if ((rc = h->d_rrmeta.ensure((size_t)h->batch * sizeof(int)))) return rc;
  auto launch = [&](auto fn) -> int {
    if (lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)fn, lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)h->batch), dim3(large_threads(r)), lds, h->stream, h->kp, 16 * h->kc.NT, h->ud, h->yd,
                       up, yp, uo, cost, (int*)status, (int*)iters, (double*)h->d_beta.p, (signed char*)h->d_act.p,
                       (double*)h->d_rr.p, (long long)stride, (int*)h->d_rrmeta.p, 0, (long long)h->batch);
    return DDMPC_OK;
  };
  auto staged = [&](auto k0, auto k1, auto k2) { return stage == Stage::Factors ? launch(k1) : stage == Stage::OnFactors ? launch(k2) : launch(k0); };
  if (r > 1024)                  // 1025 .. 2048 rows: the 1024-thread instance
    rc = staged(ddmpc_large_solve_wide_kernel<0>, ddmpc_large_solve_wide_kernel<1>, ddmpc_large_solve_wide_kernel<2>);
  else
    rc = staged(ddmpc_large_solve_kernel<0>, ddmpc_large_solve_kernel<1>, ddmpc_large_solve_kernel<2>);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// Pointer arguments of ddmpc_cold_solve_kernel2 (ddmpc_cold2.hpp), in its order.
struct ColdArgs {
  const double *ud, *yd, *up, *yp;
  double *uo, *cost;
  int32_t *status, *iters = nullptr;
  double* beta = nullptr; signed char* act = nullptr;     // beta / active-set workspace
  unsigned long long* stamps = nullptr;
  double *lfac = nullptr, *lfacT = nullptr;   // factor export (ddmpc_prepare)
  int *flag = nullptr, *count = nullptr;   // AUTO: per-instance flags of the plain kernel, and the counter word behind them
  const int* only = nullptr;               // filter: instances with only[b] == 0 are skipped
  long long nbatch = 0;                    // persistent grid: the instances it strides over
};

// The launches of the cold kernel.  Plain: fn2, or under the slack box fn2c, which keeps the first factor across active-set
// iterations (DDMPC_OPT_CONVEX_UPDATE = 0: fn2, which factors again).  Refine: the variant with the refinement loop, which on a
// trajectory beyond the LDS passes a window of it chunk by chunk.  Filtered: that variant on the instances flagged in d_rflag,
// a short persistent launch (3 workgroups per CU) that reads one counter word and leaves when nothing was flagged.
enum class ColdPass { Plain, Refine, Filtered };
static void enqueue_cold(ddmpc_handle* h, ColdPass pass, KParams k, ColdArgs a, size_t nb) {
  cold_kernel2_t fn = (k.convex && h->convex_update) ? h->kc.fn2c : h->kc.fn2;
  size_t lds = h->lds_bytes;
  if (pass != ColdPass::Plain) {
    fn = h->kc.fn2r;
    if (h->long_data) { k.xs_len = h->ld_window; lds = h->ld_lds_bytes; }
  }
  unsigned grid = (unsigned)nb;
  if (pass == ColdPass::Filtered) {
    k.refine = DDMPC_REFINE_ALWAYS;
    grid = (unsigned)(nb < 768 ? nb : 768);
    a.flag = nullptr; a.only = (const int*)h->d_rflag.p; a.nbatch = (long long)nb; a.count = (int*)h->d_rflag.p + h->batch;
  }
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * h->kc.W), lds, h->stream, k, a.ud, a.yd, a.up, a.yp, a.uo, a.cost, (int*)a.status,
                     (int*)a.iters, a.beta, a.act, a.stamps, a.lfac, a.lfacT, a.flag, a.only, a.nbatch, a.count);
}

// The beta / active-set workspace of the whole batch (what ddmpc_get_solution reconstructs from).
static int reserve_beta(ddmpc_handle* h) {
  const size_t n = (size_t)h->batch * h->kp.rE;
  if (int rc = h->d_beta.ensure(n * sizeof(double))) return rc;
  return h->d_act.ensure(n);
}

// What a handle's cold sequence writes besides its outputs, sized before it is enqueued (ddmpc_closed_loop: before a graph
// capture, inside which nothing may allocate or set an attribute): beta / active set (ws); under AUTO (flags) the flags + counter
// word, cleared when first allocated, and beyond the LDS the Hankel sums and Hankel kernel LDS of the streamed residual check.
static int reserve_cold(ddmpc_handle* h, bool ws, bool flags) {
  const size_t B = (size_t)h->batch, bytes = (B + 1) * sizeof(int);
  int rc;
  if (ws && (rc = reserve_beta(h))) return rc;
  if (!flags) return DDMPC_OK;
  const bool fresh = h->d_rflag.bytes < bytes;
  if ((rc = h->d_rflag.ensure(bytes))) return rc;
  if (fresh) HIP_TRY(hipMemsetAsync(h->d_rflag.p, 0, bytes, h->stream));
  if (!h->long_data) return DDMPC_OK;
  if ((rc = h->d_rr2zp.ensure(B * RR2_NG * (size_t)((h->kp.r + 63) & ~63) * sizeof(double)))) return rc;
  HankelLaunch hk;
  return pick_hankel_launch(h->kp, &hk);
}

// AUTO refinement once the plain launches have flagged the instances their residual check (on a trajectory beyond the LDS: their
// a-priori bound) could not dismiss.  Beyond the LDS, H (H' beta) of the whole batch by the streaming Hankel kernel of the phase
// pipeline first; its residual decides per flagged instance whether the flag stays.  Then the filtered refinement pass.
static int refine_flagged(ddmpc_handle* h, const KParams& kq, const ColdArgs& a) {
  if (h->long_data) {
    const int VL = (kq.r + 63) & ~63;
    Rr2Solve H{};
    H.V = (double*)h->d_beta.p; H.vstride = kq.rE; H.VL = VL; H.ZP = (double*)h->d_rr2zp.p; H.fdiv = 1; H.r = kq.r;
    HankelLaunch hk;
    if (int rc = pick_hankel_launch(kq, &hk)) return rc;
    launch_hankel(hk, h->stream, (unsigned)h->batch, H, kq, a.ud, a.yd, 0, 0);
    hipLaunchKernelGGL(ddmpc_flag_inaccurate_kernel, dim3((unsigned)h->batch), dim3(256), 0, h->stream, kq, 16 * h->kc.NT, kq.epoch,
                       (int*)h->d_rflag.p, a.up, a.yp, (const double*)h->d_beta.p, (const signed char*)h->d_act.p,
                       (const double*)h->d_rr2zp.p, (int)RR2_NG, VL, (int*)a.status);
    HIP_TRY(hipGetLastError());
  }
  enqueue_cold(h, ColdPass::Filtered, kq, a, (size_t)h->batch);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// What a caller of launch_cold chooses beyond the past window and the outputs: KParams in place of the handle's and the factor
// export (ddmpc_prepare), whether the beta / active-set workspace is written, a filter (the slack-box warm steps).
struct ColdSeq {
  const KParams* kp = nullptr;
  double *lfac = nullptr, *lfacT = nullptr;
  bool want_ws = true;
  const int* only = nullptr;
};

// The register-resident cold kernels (Route::Cold).  want_ws: also write the beta / active-set workspace (what
// ddmpc_get_solution, the gain kernel and the slack-box warm step read).  A plain cold solve skips it (1.2 KB of HBM writes per
// instance) and ddmpc_get_solution re-solves on demand.
static int launch_cold(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                       int32_t* iters, const ColdSeq& s = ColdSeq()) {
  int rc;
  const size_t B = (size_t)h->batch;
  const bool ws = s.want_ws || h->long_data;       // (the streamed residual check reads beta and the active set)
  // Refinement (DDMPC_OPT_REFINE).  OFF / factor export / nominal scheme (z = t does not depend on beta): plain kernel.
  // ALWAYS: the kernel variant with the refinement loop.  AUTO: plain kernel, which checks every instance's solve with
  // the exact-Hankel residual and flags the ones above the threshold; those alone are solved again (refine_flagged).  The
  // decision is taken per solve: nothing about a data set is remembered, so borrowed device data may change between solves.
  KParams kq = s.kp ? *s.kp : h->kp;
  const int mode = (s.lfac != nullptr || kq.lam == 0.0) ? DDMPC_REFINE_OFF : kq.refine;
  // factor export under AUTO: the plain kernel still records which instances AUTO would refine (ddmpc_prepare refines their law)
  const bool export_flags = s.lfac != nullptr && kq.lam != 0.0 && kq.refine == DDMPC_REFINE_AUTO && s.only == nullptr;
  if ((rc = gram_pre_launch(h, kq, h->ud, h->yd, B, 0, true))) return rc;
  if ((rc = reserve_cold(h, ws, mode == DDMPC_REFINE_AUTO || export_flags))) return rc;
  ColdArgs a{h->ud, h->yd, up, yp, uo, cost, status, iters};
  if (ws) { a.beta = (double*)h->d_beta.p; a.act = (signed char*)h->d_act.p; }
  if (h->stamps_on) a.stamps = (unsigned long long*)h->d_stamps.p;
  a.lfac = s.lfac; a.lfacT = s.lfacT; a.only = s.only;
  if (mode == DDMPC_REFINE_ALWAYS) {
    enqueue_cold(h, ColdPass::Refine, kq, a, B);
  } else if (mode == DDMPC_REFINE_AUTO) {
    if (s.only) HIP_TRY(hipMemsetAsync(h->d_rflag.p, 0, B * sizeof(int), h->stream));   // filtered-out instances: no flag
    kq.epoch = next_refine_epoch(h);
    a.flag = (int*)h->d_rflag.p; a.count = a.flag + B;
    enqueue_cold(h, ColdPass::Plain, kq, a, B);
    HIP_TRY(hipGetLastError());
    if ((rc = refine_flagged(h, kq, a))) return rc;
    h->flag_epoch = kq.epoch;                   // the flags now carry this stamp
  } else {
    if (export_flags) {
      a.flag = (int*)h->d_rflag.p; a.count = a.flag + B;
      kq.epoch = h->prep.epoch = h->flag_epoch = next_refine_epoch(h);
    }
    enqueue_cold(h, ColdPass::Plain, kq, a, B);
  }
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

static bool convex_warm_on(const ddmpc_handle* h) { return h->convex_warm && h->kp.convex && !h->large; }

// One evaluation of the affine law ddmpc_prepare kept.  keep: also write the beta / active-set workspace; need: under the slack
// box, where the kernel marks the instances whose law leaves it.
static void enqueue_warm_step(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                              int32_t* iters, bool keep, int* need) {
  hipLaunchKernelGGL(ddmpc_warm_step_kernel, dim3((unsigned)h->batch), dim3(warm_threads(h->kp.r)), 0, h->stream, h->kp,
                     16 * h->kc.NT, h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const int*)h->d_prep_status.p, up, yp, uo, cost,
                     (int*)status, (int*)iters, keep ? (double*)h->d_beta.p : (double*)nullptr,
                     keep ? (signed char*)h->d_act.p : (signed char*)nullptr, need);
}

static int launch_warm(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost,
                       int32_t* status, int32_t* iters) {
  int rc;
  if ((rc = reserve_beta(h))) return rc;
  const int nf = h->prm.n * h->kp.nch;
  const unsigned threads = warm_threads(h->kp.r);
  if (convex_warm_on(h)) {
    // DDMPC_OPT_CONVEX_WARM_LAW: the whole active-set iteration on the law and M; only instances whose law came from refining
    // solves and leaves the box go to the filtered cold launch (none unless ddmpc_prepare refined some)
    int* need = nullptr;
    if (h->prep.cwl_nref > 0) {
      if ((rc = h->d_need.ensure((size_t)h->batch * sizeof(int)))) return rc;
      need = (int*)h->d_need.p;
    }
    hipLaunchKernelGGL(ddmpc_warm_convex_step_kernel, dim3((unsigned)h->batch), dim3(threads), 0, h->stream, h->kp,
                       16 * h->kc.NT, nf, (const double*)h->d_gain.p, (const int*)h->d_prep_status.p, up, yp, uo, cost,
                       (int*)status, (int*)iters, (double*)h->d_beta.p, (signed char*)h->d_act.p, h->prep.cwl_nbox,
                       (const int*)h->d_cwl_tab.p, (const double*)h->d_mcol.p, (double*)h->d_cwl_sg.p,
                       need ? (const int*)h->d_cwl_ref.p : (const int*)nullptr, need);
    HIP_TRY(hipGetLastError());
    ColdSeq s; s.only = need;
    return need ? launch_cold(h, up, yp, uo, cost, status, iters, s) : DDMPC_OK;
  }
  int* need = nullptr;
  if (h->kp.convex) {
    if ((rc = h->d_need.ensure((size_t)h->batch * sizeof(int)))) return rc;
    need = (int*)h->d_need.p;
  }
  // beta / active set are only needed by ddmpc_get_solution (and by the filtered cold launch below): without the slack
  // box the step skips that 1.2 KB of writes per instance and ddmpc_get_solution re-evaluates the law on demand
  const bool keep = h->kp.convex != 0;
  enqueue_warm_step(h, up, yp, uo, cost, status, iters, keep, need);
  HIP_TRY(hipGetLastError());
  if (!keep) h->last.beta = BetaState::ReEvalLaw;
  // instances with an active slack bound: full active-set solve, same launch geometry, others exit at once
  ColdSeq s; s.only = need;
  return need ? launch_cold(h, up, yp, uo, cost, status, iters, s) : DDMPC_OK;
}

// Route::BoxLaw (input bounds): a control step on what ddmpc_prepare kept -- the law, M for the whole box list and the table.
// seeded (DDMPC_OPT_BOX_WARM_START = 1 only): the iteration starts from the set in d_box_seed; with the option 1 every launch
// leaves its set there.  Per-instance bounds (instance_bounds): the BoxChannels instantiations with the channel table;
// DDMPC_OPT_BOX_WARM_START is not honoured there -- from the empty set, no seed read or left.
static int launch_box_step(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                           int32_t* iters, bool seeded) {
  if (int rc = reserve_beta(h)) return rc;
  const bool inst = instance_bounds(h);
  const bool warm = h->box_warm != 0 && !inst;
  if (warm)
    if (int rc = h->d_box_seed.ensure((size_t)h->batch * (size_t)std::max(h->prep.cwl_nbox, 1))) return rc;
  // (DDMPC_OPT_BOX_SAFEGUARD = 0 launches the instantiation without the safeguard: its registers and LDS are the kernel's own)
  // (output bounds: the instantiations with the output components, block = max(r, nbox) rounded up to 64)
  const bool yb = !h->ymin_h.empty();
  // (DDMPC_OPT_BOX_WARM_START = 0 launches the instantiations without the seed argument: the kernels as they were)
  // (per-instance bounds launch the instantiations with the channel table as the trailing argument)
  auto launch = [&](auto... extra) {
    with_safe_yb(h->box_safeguard != 0, yb, [&](auto safe, auto ybt) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(ddmpc_box_step_kernel<safe(), ybt(), decltype(extra)...>), dim3((unsigned)h->batch),
                         dim3(yb ? (unsigned)h->prep.box_threads : warm_threads(h->kp.r)), 0, h->stream, h->kp,
                         16 * h->kc.NT, h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const int*)h->d_prep_status.p, up, yp, uo,
                         cost, (int*)status, (int*)iters, (double*)h->d_beta.p, (signed char*)h->d_act.p, h->prep.cwl_nbox,
                         (const int*)h->d_cwl_tab.p, (const double*)h->d_box_bd.p, (const double*)h->d_mcol.p, (double*)h->d_cwl_sg.p,
                         h->prep.cwl_nref > 0 ? (const int*)h->d_cwl_ref.p : (const int*)nullptr, extra...);
    });
  };
  if (inst) launch(BoxChannels{(const double*)h->d_ibnd.p});
  else if (warm) launch(BoxSeed{(signed char*)h->d_box_seed.p, seeded ? 1 : 0});
  else launch();
  HIP_TRY(hipGetLastError());
  h->last.box_seed = warm;
  return DDMPC_OK;
}

// ... and a cold solve: the trajectories are read anew and nothing derived from them is kept.  What ddmpc_prepare runs goes
// into a preparation of the solve's own (buffers apart from the kept one's, which a ddmpc_prepare before the call keeps valid,
// as on Route::Cold), the step kernel runs at the caller's window, and that preparation is dropped.
static int solve_box(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                     int32_t* iters) {
  auto swap_bufs = [&]() {
    std::swap(h->d_gain, h->s_gain); std::swap(h->d_prep_status, h->s_prep_status);
    std::swap(h->d_mcol, h->s_mcol); std::swap(h->d_cwl_ref, h->s_cwl_ref);
  };
  const Prep kept = h->prep;
  const int sp = h->setpoint_law, spb = h->setpoint_box_law, spc = h->setpoint_convex_law;   // (the solve's own preparation forms no S: the kept one stays)
  h->setpoint_law = h->setpoint_box_law = h->setpoint_convex_law = 0;
  swap_bufs();
  h->prep = Prep{};
  int rc = ddmpc_prepare(h);
  h->setpoint_law = sp; h->setpoint_box_law = spb; h->setpoint_convex_law = spc;
  if (!rc) {
    begin_solve(h, Route::BoxLaw);
    rc = launch_box_step(h, up, yp, uo, cost, status, iters, false);   // (cold contract: from the empty set; it leaves a seed)
  }
  swap_bufs();
  h->prep = kept;
  return rc;
}

// Nominal scheme: instances whose Gram matrix is singular (exact data) are re-solved by the rank-revealing
// kernel; it only touches instances the fast path marked SOLVER_ERROR.  Beyond the register-resident kernels (the NOMINAL
// routes) every instance is marked and this is the whole solve.
// stage (problems whose matrices live in the global workspace only): see Stage and ddmpc_nominal_rr_kernel.
static int launch_rr2_factors(ddmpc_handle* h, double* scratch, long long ndbl, double rank_tol);
static int launch_rr2_solve(ddmpc_handle* h, double* scratch, long long ndbl, const double* up, const double* yp, double* uo,
                            double* cost, int32_t* status, int32_t* iters, double feas_tol);
static int launch_nominal_rescue(ddmpc_handle* h, Route route, const double* up, const double* yp, double* uo, double* cost,
                                 int32_t* status, int32_t* iters, Stage stage = Stage::Solve) {
  if (h->prm.controller_type != DDMPC_NOMINAL || (h->prm.weight_kind == DDMPC_WEIGHT_DENSE && route == Route::Cold)) return DDMPC_OK;
  if (route != Route::Cold) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)status, 4, (size_t)h->batch, h->stream));   // (all SOLVER_ERROR)
  const size_t r = (size_t)h->kp.r, nR = (size_t)h->n_free;
  size_t ndbl = pk_size(r) + pk_size(nR);                         // packed rows on 128-byte boundaries (ddmpc_workspace_kernels.hpp)
  const size_t rv = (r + 1) & ~(size_t)1;
  const size_t vec_bytes = 10 * rv * sizeof(double) + 4 * rv * sizeof(int) +    // the kernel's r-vectors, always in LDS,
                           (size_t)PSD_PAN * sizeof(double);                        // and the scratch of its Cholesky / Gram
  size_t lds = vec_bytes + ndbl * sizeof(double);
  double* scratch = nullptr;
  if (lds + 1024 > 160 * 1024) {                              // matrices too big for LDS: per-instance slices of a global workspace
    ndbl = (size_t)rr2_ndbl(h);                               // (whole 16-row tiles: the phase kernels of ddmpc_rr2.hpp)
    int rc = h->d_rr.ensure((size_t)h->batch * ndbl * sizeof(double));
    if (rc) return rc;
    scratch = (double*)h->d_rr.p;
    lds = vec_bytes;
    if ((rc = h->d_rrmeta.ensure((size_t)h->batch * (2 * rv + 2) * sizeof(int)))) return rc;
  }
  if (!scratch) stage = Stage::Solve;
  if (lds + 1024 > 160 * 1024) return fail(DDMPC_ERR_UNSUPPORTED, "problem too large: %zu rows", r);
  {   // per instance: the r-vector w of the refinement passes
    int rca = h->d_alpha.ensure((size_t)h->batch * (size_t)h->kp.r * sizeof(double));
    if (rca) return rca;
  }
  {   // z per component + "rescued" flag per instance, read by ddmpc_get_solution
    int rcz = h->d_zws.ensure((size_t)h->batch * h->kp.rE * sizeof(double));
    if (!rcz) rcz = h->d_resc.ensure((size_t)h->batch * sizeof(int));
    if (!rcz) rcz = h->d_xws.ensure((size_t)h->batch * h->kp.rE * sizeof(double));
    if (rcz) return rcz;
    // (a factors-only launch writes neither z_ws, x_ws nor the flags: what the previous solve left there stays readable by
    //  ddmpc_get_solution, so the flags must not be cleared -- ddmpc_solve -> ddmpc_prepare -> ddmpc_get_solution)
    if (stage != Stage::Factors || !h->last.rescue)
      HIP_TRY(hipMemsetAsync(h->d_resc.p, 0, (size_t)h->batch * sizeof(int), h->stream));
  }
  // rank tolerance 1e-8 (relative to the largest diagonal entry of the Gram): with the fixed-first ordering the
  // pivots of dependent rows come out as rounding residue up to ~3e-10, genuine ones are >= ~5e-7 on exact
  // four-tank data (L = 10 .. 60)
  auto launch = [&](auto fn) -> int {
    if (lds > 64 * 1024) HIP_TRY(raise_lds_limit((const void*)fn, lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)h->batch), dim3(large_threads(r)), lds, h->stream, h->kp, 16 * h->kc.NT,
                       h->ud, h->yd, up, yp, uo, cost, (int*)status, (int*)iters, 1e-8, 1e-7, scratch, (long long)ndbl,
                       (double*)h->d_alpha.p,
                       (h->stamps_on && h->d_stamps.bytes >= (size_t)h->batch * 16 * sizeof(uint64_t)) ? (unsigned long long*)h->d_stamps.p
                                                                                                        : (unsigned long long*)nullptr,
                       (double*)h->d_zws.p, (int*)h->d_resc.p, (double*)h->d_xws.p,
                       scratch ? (int*)h->d_rrmeta.p : (int*)nullptr);
    HIP_TRY(hipGetLastError());
    return DDMPC_OK;
  };
  int rcl = DDMPC_OK;
  if (!scratch) rcl = launch(ddmpc_nominal_rr_kernel<0>);                 // matrices in LDS: one launch
  else {                                                                  // global workspace: factors, then the solve on them
    // (the one-workgroup kernel beyond 1024 rows: its 1024-thread instance)
    const bool wide = r > 1024;
    const bool phases = route == Route::NominalPhases;
    const bool wdense = h->prm.weight_kind == DDMPC_WEIGHT_DENSE;
    if (wdense && !phases)
      return fail(DDMPC_ERR_UNSUPPORTED, "dense weighting matrices of a NOMINAL controller beyond 271 rows run on the phase kernels only "
                  "(batches up to 65535, no diagnostic stamps)");
    if (stage != Stage::OnFactors) rcl = phases ? launch_rr2_factors(h, scratch, (long long)ndbl, 1e-8)
                                                : (wide ? launch(ddmpc_nominal_rr_wide_kernel<1>) : launch(ddmpc_nominal_rr_kernel<1>));
    if (!rcl && stage != Stage::Factors) {
      rcl = phases ? launch_rr2_solve(h, scratch, (long long)ndbl, up, yp, uo, cost, status, iters, 1e-7)
                   : (wide ? launch(ddmpc_nominal_rr_wide_kernel<2>) : launch(ddmpc_nominal_rr_kernel<2>));
      if (!rcl && phases && h->kp.refine_max > 1 && !wdense) rcl = launch(ddmpc_nominal_rr_kernel<2>);      // the instances the phase solve marked 4 (more passes)
    }
  }
  if (rcl) return rcl;
  if (stage != Stage::Factors) {          // (the phase solve keeps w: x = L^-T w is formed on demand)
    h->last.rescue = true;
    h->last.x = scratch && route == Route::NominalPhases ? XState::FromW : XState::Written;
  }
  return DDMPC_OK;
}

// The data-dependent half of a NOMINAL solve beyond the register-resident kernels as phase kernels over the whole batch
// (ddmpc_rr2.hpp): Gram -> lock-step Cholesky (64-column panels: update launch + panel launch) -> live counts -> C'WC ->
// its Cholesky.  Leaves in the workspace / meta exactly what ddmpc_nominal_rr_kernel<1> leaves.
static int launch_rr2_factors(ddmpc_handle* h, double* scratch, long long ndbl, double rank_tol) {
  const KParams& k = h->kp;
  const int r = k.r, n16 = (r + 15) & ~15, nR = h->n_free, nF = h->nF, nR16 = (nR + 15) & ~15;
  const int rv = (r + 1) & ~1;
  const long long mstride = 2 * (long long)rv + 2;
  const size_t B = (size_t)h->batch;
  const long long m64G = rr2_m64(n16), m64T = rr2_m64(nR16);       // Minv blocks of G's factor per instance, T's behind them
  int rc;
  const long long rstride = (long long)n16 + 2;              // per instance: two words of retired-tile bits, then the residual diagonal
  if ((rc = h->d_rr2d.ensure(B * 4 * sizeof(unsigned long long))) || (rc = h->d_rr2mt.ensure(B * (size_t)(m64G + m64T) * sizeof(double))) ||
      (rc = h->d_rr2res.ensure(B * (size_t)rstride * sizeof(double)))) return rc;
  HIP_TRY(hipMemsetAsync(h->d_rr2d.p, 0, B * 4 * sizeof(unsigned long long), h->stream));
  HIP_TRY(hipMemset2DAsync(h->d_rr2res.p, (size_t)rstride * sizeof(double), 0, 2 * sizeof(unsigned long long), B, h->stream));
  unsigned long long* dd = (unsigned long long*)h->d_rr2d.p;
  int* meta = (int*)h->d_rrmeta.p;
  const int* perm = (const int*)h->d_perm.p;
  const int* iperm = perm + rv;
  auto gram = [&]() {
    launch_rr2_gram(h->stream, k, h->ud, h->yd, iperm, scratch, ndbl, n16, dd, B);
  };
  gram();
  Rr2Chol FG{};
  FG.ws = scratch; FG.stride = ndbl; FG.off = 0; FG.n16 = n16; FG.n_inst = nullptr; FG.n_stride = 0;
  FG.dmax = dd + 0; FG.d_stride = 4; FG.tol_rel = rank_tol; FG.skip = meta; FG.s_stride = mstride; FG.nflag = r;
  FG.live = dd + 2; FG.l_stride = 4; FG.m64 = (double*)h->d_rr2mt.p; FG.m64_stride = m64G + m64T;
  FG.res = (double*)h->d_rr2res.p + 2; FG.res_stride = rstride; FG.dead = (unsigned long long*)h->d_rr2res.p; FG.dead_stride = rstride;
  if ((rc = h->d_rr2cand.ensure(B * (size_t)n16 * sizeof(double)))) return rc;
  FG.cand = (double*)h->d_rr2cand.p; FG.cand_stride = n16;
  launch_rr2_cholesky(h->stream, FG, n16, B);
  // what follows the factor of G: pivot counts, T = C'WC, its factor
  auto downstream = [&]() -> int {
    hipLaunchKernelGGL(rr2_meta_kernel, dim3((unsigned)B), dim3(256), 0, h->stream, meta, mstride, rv, r, nF, nR);
    if (nR > 0) {
      const int ldw = ((nR16 + 31) / 32) * 32 + 16;                         // LDS row of the C'WC kernel: 16 mod 32 doubles
      const size_t cwlds = ((size_t)(h->d_wd.p ? 32 : 16) * ldw + 16) * sizeof(double);
      if (cwlds > 64 * 1024)
        HIP_TRY(raise_lds_limit((const void*)rr2_cwc_kernel, cwlds));
      const double* Yd = nullptr;
      const long long ystride = (long long)nR16 * nR16;
      if (h->d_wd.p) {                                      // dense weighting matrices: Y = W C first
        int rcy = h->d_rr2y.ensure(B * (size_t)ystride * sizeof(double));
        if (rcy) return rcy;
        Yd = (const double*)h->d_rr2y.p;
        hipLaunchKernelGGL(rr2_wc_kernel, dim3((unsigned)(nR16 / 16), (unsigned)B), dim3(256), 0, h->stream, (const double*)h->d_wd.p, (const double*)scratch,
                           ndbl, (const int*)meta, mstride, rv, nF, nR, (double*)h->d_rr2y.p, ystride, nR16);
      }
      hipLaunchKernelGGL(rr2_cwc_kernel, dim3((unsigned)B), dim3(1024), cwlds, h->stream, k, 16 * h->kc.NT, perm, scratch, ndbl,
                         (long long)pk_size((size_t)n16), (const int*)meta, mstride, rv, nF, nR, dd + 1, ldw, Yd, ystride, nR16);
      Rr2Chol FT{};
      FT.ws = scratch; FT.stride = ndbl; FT.off = (long long)pk_size((size_t)n16); FT.n16 = nR16;
      FT.n_inst = meta + 2 * rv + 1; FT.n_stride = mstride;
      FT.dmax = dd + 1; FT.d_stride = 4; FT.tol_rel = 1e-14; FT.skip = meta + rv; FT.s_stride = mstride; FT.nflag = nR;
      FT.live = dd + 3; FT.l_stride = 4; FT.m64 = (double*)h->d_rr2mt.p + m64G; FT.m64_stride = m64G + m64T;
      if (nR16 <= 384)            // a few panels: one launch, one workgroup per instance walks them (rr2_chol_small_kernel)
        hipLaunchKernelGGL(rr2_chol_small_kernel<2>, dim3((unsigned)B), dim3(256), 0, h->stream, FT);
      else
        launch_rr2_cholesky(h->stream, FT, nR16, B);
    }
    HIP_TRY(hipGetLastError());
    return DDMPC_OK;
  };
  {
    // The rank decision, judged from the pivot candidates (rr2_rank_margin_kernel): an instance that accepted more pivots than
    // rank H can be gets a tolerance inside the gap behind the largest m (L + n) + n candidates and the batch is factored once
    // more with per-instance tolerances (every other instance keeps its tolerance: bit-identical factors); a decision without a
    // clear margin is flagged and the solve reports "optimal_inaccurate".  One 4-byte read-back per data set decides on the
    // second pass -- none on the benchmark configurations.
    if ((rc = h->d_rr2tol.ensure(2 * B * sizeof(double))) || (rc = h->d_rr2rank.ensure((2 * B + 1) * sizeof(int)))) return rc;
    const int bound = k.m * k.Ln + h->prm.n;
    const double safe = 20.0;
    int* rec = (int*)h->d_rr2rank.p;
    HIP_TRY(hipMemsetAsync(rec + 2 * B, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(rr2_rank_margin_kernel, dim3((unsigned)B), dim3(256), 0, h->stream, (const double*)h->d_rr2cand.p, (long long)n16, r, bound,
                       rank_tol, (const double*)nullptr, safe, 1, (double*)h->d_rr2tol.p, rec, rec + 2 * B, (double*)h->d_rr2tol.p + B);
    // ... read back WITHOUT draining the stream: the copy lands in a pinned word behind an event, everything downstream of the
    // factor (pivot counts, C'WC, its factor) is queued at once as if no instance needed the second pass -- the usual case -- and
    // the host waits for the event while the GPU works on that; a batch that does need it is factored again and the downstream
    // launches are repeated
    if ((rc = h->h_flag.ensure(sizeof(int)))) return rc;
    if (!h->ev_flag) HIP_TRY(hipEventCreateWithFlags(&h->ev_flag, hipEventDisableTiming));
    volatile int* nredo = (volatile int*)h->h_flag.p;
    *nredo = 0;
    HIP_TRY(hipMemcpyAsync(h->h_flag.p, rec + 2 * B, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipEventRecord(h->ev_flag, h->stream));
    if ((rc = downstream())) return rc;
    HIP_TRY(hipEventSynchronize(h->ev_flag));
    if (*nredo > 0) {
      HIP_TRY(hipMemsetAsync(h->d_rr2d.p, 0, B * 4 * sizeof(unsigned long long), h->stream));
      HIP_TRY(hipMemset2DAsync(h->d_rr2res.p, (size_t)rstride * sizeof(double), 0, 2 * sizeof(unsigned long long), B, h->stream));
      gram();
      FG.tol_inst = (const double*)h->d_rr2tol.p;
      launch_rr2_cholesky(h->stream, FG, n16, B);
      hipLaunchKernelGGL(rr2_rank_margin_kernel, dim3((unsigned)B), dim3(256), 0, h->stream, (const double*)h->d_rr2cand.p, (long long)n16, r, bound,
                         rank_tol, (const double*)h->d_rr2tol.p, safe, 0, (double*)h->d_rr2tol.p, rec, rec + 2 * B, (double*)h->d_rr2tol.p + B);
      if ((rc = downstream())) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// The solve on those factors (what a control step repeats, controller.py:389-407), as phase kernels (ddmpc_rr2_solve.hpp).
static int rr2_solve_desc(ddmpc_handle* h, double* scratch, long long ndbl, Rr2Solve* out, size_t vbatch = 0) {
  const KParams& k = h->kp;
  const int r = k.r, n16 = (r + 15) & ~15, nR = h->n_free, nF = h->nF, nR16 = (nR + 15) & ~15;
  const int rv = (r + 1) & ~1, VL = (r + 63) & ~63;
  const size_t B = vbatch ? vbatch : (size_t)h->batch;           // (the gain build runs the solve on a virtual batch)
  const long long m64G = rr2_m64(n16), m64T = rr2_m64(nR16);
  int rc;
  if ((rc = h->d_rr2v.ensure(B * (size_t)V_NV * VL * sizeof(double))) || (rc = h->d_rr2zp.ensure(B * (size_t)RR2_NG * VL * sizeof(double))) ||
      (rc = h->d_rr2sc.ensure(B * (4 * sizeof(double) + 2 * sizeof(int) + sizeof(unsigned long long)))))
    return rc;
  Rr2Solve S{};
  S.ws = scratch; S.stride = ndbl; S.toff = (long long)pk_size((size_t)n16);
  S.m64 = (const double*)h->d_rr2mt.p; S.m64_stride = m64G + m64T; S.m64T = m64G;
  S.meta = (const int*)h->d_rrmeta.p; S.mstride = 2 * (long long)rv + 2; S.rv = rv;
  S.dd = (const unsigned long long*)h->d_rr2d.p;
  S.perm = (const int*)h->d_perm.p;
  S.wz = (const double*)h->d_wz.p;
  S.wd = (const double*)h->d_wd.p;
  S.rankrec = (const int*)h->d_rr2rank.p;
  S.noise = h->d_rr2tol.p ? (const double*)h->d_rr2tol.p + h->batch : nullptr;
  S.V = (double*)h->d_rr2v.p; S.vstride = (long long)V_NV * VL; S.VL = VL;
  S.ZP = (double*)h->d_rr2zp.p;
  S.sc = (double*)h->d_rr2sc.p;
  S.resid = (unsigned long long*)(S.sc + 4 * B);
  S.si = (int*)(S.resid + B);
  S.r = r; S.nF = nF; S.nR = nR;
  S.fdiv = 1; S.unit = 0; S.ubase = 0;
  *out = S;
  return DDMPC_OK;
}

static int rr2_solve_sequence(ddmpc_handle* h, const Rr2Solve& S, unsigned B, const double* up, const double* yp, double* uo,
                              double* cost, int32_t* status, int32_t* iters, double* zws, int* resc, double feas_tol) {
  const KParams& k = h->kp;
  const int RPs = 16 * h->kc.NT, nF = S.nF, nR = S.nR;
  auto grp = [](int n, int per) { return (unsigned)((n + per - 1) / per < 1 ? 1 : (n + per - 1) / per); };
  hipStream_t st = h->stream;
  HankelLaunch hk;                                                        // H (H' x)
  const int rc = pick_hankel_launch(k, &hk);
  if (rc) return rc;
  auto hankel = [&](int slot, int pass) { launch_hankel(hk, st, B, S, k, h->ud, h->yd, slot, pass); };
  hipLaunchKernelGGL(rr2_s1_kernel, dim3(B), dim3(RR2_TS), 0, st, S, k, RPs, up, yp);
  hipLaunchKernelGGL(rr2_rows_kernel<0>, dim3(grp(nF + nR, 32), B), dim3(256), 0, st, S, k, RPs, (double*)nullptr, (double*)nullptr, 0);
  if (S.wd) hipLaunchKernelGGL(rr2_wapply_kernel<0>, dim3(B), dim3(RR2_TS), 0, st, S, 0);
  hipLaunchKernelGGL(rr2_cols_kernel<0>, dim3(grp(nR, 64), B), dim3(512), 0, st, S, 0);
  {
    // one refinement pass for everybody; an instance whose correction says another pass would still pay (rr2_s13_kernel: the
    // rule of ddmpc_nominal_rr_kernel) is marked and solved again, passes and all, by that kernel behind this sequence
    const int pass = 0;
    hipLaunchKernelGGL(rr2_s4_kernel, dim3(B), dim3(RR2_TS), 0, st, S, pass);
    hankel((int)V_X, pass);
    hipLaunchKernelGGL(rr2_rows_kernel<1>, dim3(grp(nR, 32), B), dim3(256), 0, st, S, k, RPs, (double*)nullptr, (double*)nullptr, pass);
    if (S.wd) hipLaunchKernelGGL(rr2_wapply_kernel<1>, dim3(B), dim3(RR2_TS), 0, st, S, pass);
    hipLaunchKernelGGL(rr2_cols_kernel<1>, dim3(grp(nF, 64), B), dim3(512), 0, st, S, pass);
    hipLaunchKernelGGL(rr2_s8_kernel, dim3(B), dim3(RR2_TS), 0, st, S, pass);
    hankel((int)V_VC, pass);
    hipLaunchKernelGGL(rr2_rows_kernel<2>, dim3(grp(nR, 32), B), dim3(256), 0, st, S, k, RPs, (double*)nullptr, (double*)nullptr, pass);
    hipLaunchKernelGGL(rr2_s11_kernel, dim3(B), dim3(RR2_TS), 0, st, S, pass);
    if (S.wd) hipLaunchKernelGGL(rr2_wapply_kernel<2>, dim3(B), dim3(RR2_TS), 0, st, S, pass);
    hipLaunchKernelGGL(rr2_cols_kernel<2>, dim3(grp(nR, 64), B), dim3(512), 0, st, S, pass);
    // (dense weighting matrices: no instance is handed to ddmpc_nominal_rr_kernel<2> for further passes -- that kernel knows
    //  diagonal weights only)
    hipLaunchKernelGGL(rr2_s13_kernel, dim3(B), dim3(RR2_TS), 0, st, S, pass, S.wd ? 1 : k.refine_max);
  }
  hipLaunchKernelGGL(rr2_rows_kernel<3>, dim3(grp(nR, 32), B), dim3(256), 0, st, S, k, RPs, uo, zws, 0);
  if (S.wd) hipLaunchKernelGGL(rr2_wapply_kernel<3>, dim3(B), dim3(RR2_TS), 0, st, S, 0);
  hipLaunchKernelGGL(rr2_s15_kernel, dim3(B), dim3(RR2_TS), 0, st, S, k, RPs, feas_tol, uo, cost, (int*)status, (int*)iters, zws, resc);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

static int launch_rr2_solve(ddmpc_handle* h, double* scratch, long long ndbl, const double* up, const double* yp, double* uo,
                            double* cost, int32_t* status, int32_t* iters, double feas_tol) {
  Rr2Solve S;
  int rc = rr2_solve_desc(h, scratch, ndbl, &S);
  if (rc) return rc;
  return rr2_solve_sequence(h, S, (unsigned)h->batch, up, yp, uo, cost, status, iters, (double*)h->d_zws.p, (int*)h->d_resc.p, feas_tol);
}

// DDMPC_OPT_LARGE_AFFINE_LAW: the affine law z(past) of every instance (ddmpc_rr2_solve.hpp), formed by ddmpc_prepare from solves at
// the zero window and the n(m+p) unit windows on a virtual batch, RR2_GAIN_CHUNK windows at a time.
constexpr int RR2_GAIN_CHUNK = 16;
static int launch_rr2_gain_build(ddmpc_handle* h, double* scratch, long long ndbl) {
  const KParams& k = h->kp;
  const int nf = h->prm.n * k.nch, nrhs = nf + 1, nFp = (h->nF + 63) & ~63;
  if (nf > WARM_MAX_NF) return fail(DDMPC_ERR_UNSUPPORTED, "the affine law supports n*(m+p) <= %d", WARM_MAX_NF);
  const size_t B = (size_t)h->batch, Bv = B * RR2_GAIN_CHUNK;
  if (Bv > 65535) return fail(DDMPC_ERR_UNSUPPORTED, "batch too large for the affine law at this size (%zu instances x %d windows per launch)", B, RR2_GAIN_CHUNK);
  int rc;
  if ((rc = h->d_gz.ensure(B * (size_t)nrhs * k.r * sizeof(double))) || (rc = h->d_gres.ensure(B * (size_t)nrhs * nFp * sizeof(double))) ||
      (rc = h->d_zvirt.ensure(Bv * (size_t)k.rE * sizeof(double))))
    return rc;
  if (h->last.x == XState::FromW) {
    // the virtual-batch solves below reuse (and re-size) the vectors the last solve kept for the on-demand x = L^-T w of
    // ddmpc_get_solution(ALPHA): form x now (ddmpc_solve -> ddmpc_prepare -> ddmpc_get_solution)
    Rr2Solve S0;
    if ((rc = rr2_solve_desc(h, scratch, ndbl, &S0))) return rc;
    if ((rc = h->d_xws.ensure(B * (size_t)k.rE * sizeof(double)))) return rc;
    hipLaunchKernelGGL(rr2_xws_kernel, dim3((unsigned)B), dim3(RR2_TS), 0, h->stream, S0, k, (double*)h->d_xws.p);
    HIP_TRY(hipGetLastError());
    h->last.x = XState::Written;
  }
  Rr2Solve S;
  if ((rc = rr2_solve_desc(h, scratch, ndbl, &S, Bv))) return rc;
  S.fdiv = RR2_GAIN_CHUNK; S.unit = 1;
  for (int j0 = 0; j0 < nrhs; j0 += RR2_GAIN_CHUNK) {
    S.ubase = j0;
    if ((rc = rr2_solve_sequence(h, S, (unsigned)Bv, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (double*)h->d_zvirt.p, nullptr, 1e-7)))
      return rc;
    hipLaunchKernelGGL(rr2_gain_collect_kernel, dim3((unsigned)Bv), dim3(256), 0, h->stream, S, k, (const double*)h->d_zvirt.p, nrhs, nFp,
                       (double*)h->d_gz.p, (double*)h->d_gres.p);
  }
  const long long tz = (long long)B * nf * k.r, tr = (long long)B * nf * nFp;
  hipLaunchKernelGGL(rr2_gain_finish_kernel, dim3((unsigned)((tz + 255) / 256)), dim3(256), 0, h->stream, (long long)B, nrhs, k.r, (double*)h->d_gz.p);
  hipLaunchKernelGGL(rr2_gain_finish_kernel, dim3((unsigned)((tr + 255) / 256)), dim3(256), 0, h->stream, (long long)B, nrhs, nFp, (double*)h->d_gres.p);
  HIP_TRY(hipGetLastError());
  h->prep.law = true;
  return DDMPC_OK;
}

// NOMINAL controller beyond the register-resident kernels, warm: a solve on the factors ddmpc_prepare left in the workspace
static int launch_large_nominal_warm(ddmpc_handle* h, Route route, const double* up, const double* yp, double* uo, double* cost,
                                     int32_t* status, int32_t* iters) {
  if (h->prep.law && h->large_affine) {                                // the affine law of ddmpc_prepare: one HBM-bound launch
    const KParams& k = h->kp;
    const int nf = h->prm.n * k.nch, nFp = (h->nF + 63) & ~63;
    int rcz = h->d_zws.ensure((size_t)h->batch * k.rE * sizeof(double));
    if (!rcz) rcz = h->d_resc.ensure((size_t)h->batch * sizeof(int));
    if (rcz) return rcz;
    hipLaunchKernelGGL(rr2_gain_step_kernel, dim3((unsigned)h->batch), dim3(512), 0, h->stream, k, 16 * h->kc.NT, h->nF, nFp, nf + 1,
                       (const double*)h->d_gz.p, (const double*)h->d_gres.p, up, yp, uo, cost, (int*)status, (int*)iters,
                       (double*)h->d_zws.p, (int*)h->d_resc.p, 1e-7);
    HIP_TRY(hipGetLastError());
    h->last.rescue = true;
    h->last.x = XState::ReSolveOnFactors;
    return DDMPC_OK;
  }
  return launch_nominal_rescue(h, route, up, yp, uo, cost, status, iters, Stage::OnFactors);
}

// A cold solve of the whole batch on the handle's route (ddmpc_solve, the cold closed loop).
static int solve_on_route(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                          int32_t* iters) {
  if (select_route(h) == Route::BoxLaw) return solve_box(h, up, yp, uo, cost, status, iters);
  const Route route = begin_solve(h, select_route(h));
  if (route != h->prep.route) forget_prep(h);                   // (its workspace is the one ddmpc_prepare kept things in)
  if (route == Route::RobustPhases || route == Route::RobustOneWg)
    return launch_large_robust(h, route, Stage::Solve, up, yp, uo, cost, status, iters);
  int rc = DDMPC_OK;
  if (route == Route::Cold) {           // (beyond 271 rows no cold kernel: the rescue is the solve)
    ColdSeq s; s.want_ws = false;
    rc = launch_cold(h, up, yp, uo, cost, status, iters, s);
    if (!h->long_data) h->last.beta = BetaState::ReSolveCold;   // (beyond the LDS the streamed residual check wrote them)
  }
  return rc ? rc : launch_nominal_rescue(h, route, up, yp, uo, cost, status, iters);
}

// A control step on what ddmpc_prepare kept (ddmpc_step, the per-step closed loop): the callers have prepared on this route.
static int step_on_route(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                         int32_t* iters) {
  const bool seeded = box_seed_valid(h), large_seeded = large_seed_valid(h);
  const Route route = begin_solve(h, select_route(h));
  if (route == Route::BoxLaw) return launch_box_step(h, up, yp, uo, cost, status, iters, seeded);
  if (route == Route::RobustPhases || route == Route::RobustOneWg)
    return launch_large_robust(h, route, Stage::OnFactors, up, yp, uo, cost, status, iters, large_seeded);
  if (route != Route::Cold) return launch_large_nominal_warm(h, route, up, yp, uo, cost, status, iters);
  const int rc = launch_warm(h, up, yp, uo, cost, status, iters);
  return rc ? rc : launch_nominal_rescue(h, route, up, yp, uo, cost, status, iters);
}

typedef int (*launch_fn)(ddmpc_handle*, const double*, const double*, double*, double*, int32_t*, int32_t*);

static int solve_impl(ddmpc_handle* h, const double* u_past, const double* y_past, double* u_opt, double* cost,
                      int32_t* status, int32_t* iters, int mem, launch_fn launch) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (!h->have_data) return fail(DDMPC_ERR_NOT_READY, "ddmpc_set_data must be called before ddmpc_solve");
  if (!u_past || !y_past || !u_opt || !cost || !status) return fail(DDMPC_ERR_INVALID, "null argument");
  if (h->batch > 0x7fffffffLL) return fail(DDMPC_ERR_INVALID, "batch too large for one launch");
  HIP_TRY(hipSetDevice(h->device));
  const ddmpc_params& p = h->prm;
  const size_t n_up = (size_t)h->batch * p.n * p.m * sizeof(double);
  const size_t n_yp = (size_t)h->batch * p.n * p.p * sizeof(double);
  const size_t n_uo = (size_t)h->batch * p.L * p.m * sizeof(double);
  int rc;
  if (mem == DDMPC_MEM_DEVICE) {
    if ((rc = launch(h, u_past, y_past, u_opt, cost, status, iters))) return rc;
    end_solve(h, u_past, y_past);
    return DDMPC_OK;
  }
  if (mem != DDMPC_MEM_HOST) return fail(DDMPC_ERR_INVALID, "mem must be DDMPC_MEM_HOST or DDMPC_MEM_DEVICE");
  // packed staging: [u_past | y_past | u_opt | cost | status | iters], every section 16-byte aligned
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t B = (size_t)h->batch;
  const size_t o_up = 0, o_yp = al(o_up + n_up), o_uo = al(o_yp + n_yp), o_cost = al(o_uo + n_uo),
               o_st = al(o_cost + B * sizeof(double)), o_it = al(o_st + B * sizeof(int32_t)),
               total = al(o_it + B * sizeof(int32_t));
  if ((rc = h->d_io.ensure(total)) || (rc = h->h_io.ensure(total))) return rc;
  char* hb = (char*)h->h_io.p;
  char* db = (char*)h->d_io.p;
  memcpy(hb + o_up, u_past, n_up);
  memcpy(hb + o_yp, y_past, n_yp);
  HIP_TRY(hipMemcpyAsync(db, hb, o_uo, hipMemcpyHostToDevice, h->stream));                 // both inputs, one copy
  if ((rc = launch(h, (const double*)(db + o_up), (const double*)(db + o_yp), (double*)(db + o_uo),
                   (double*)(db + o_cost), (int32_t*)(db + o_st), (int32_t*)(db + o_it))))
    return rc;
  HIP_TRY(hipMemcpyAsync(hb + o_uo, db + o_uo, total - o_uo, hipMemcpyDeviceToHost, h->stream));   // all outputs, one copy
  HIP_TRY(hipStreamSynchronize(h->stream));
  memcpy(u_opt, hb + o_uo, n_uo);
  memcpy(cost, hb + o_cost, B * sizeof(double));
  memcpy(status, hb + o_st, B * sizeof(int32_t));
  if (iters) memcpy(iters, hb + o_it, B * sizeof(int32_t));
  end_solve(h, (const double*)(db + o_up), (const double*)(db + o_yp));
  return DDMPC_OK;
}

int ddmpc_solve(ddmpc_handle* h, const double* u_past, const double* y_past, double* u_opt, double* cost,
                int32_t* status, int32_t* iters, int mem) {
  if (h) h->gpre_valid = false;           // (borrowed device data may have changed since the last call)
  return solve_impl(h, u_past, y_past, u_opt, cost, status, iters, mem, &solve_on_route);
}

int ddmpc_solve_from_host(ddmpc_handle* h, const double* u_d, const double* y_d, const double* u_past,
                          const double* y_past, double* u_opt, double* cost, int32_t* status, int32_t* iters) {
  if (!h || !u_d || !y_d || !u_past || !y_past || !u_opt || !cost || !status)
    return fail(DDMPC_ERR_INVALID, "null argument");
  if (h->batch > 0x7fffffffLL) return fail(DDMPC_ERR_INVALID, "batch too large for one launch");
  if (h->bounded && h->umin_h.empty())
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_solve_from_host does not serve a handle with output bounds (ddmpc_set_output_bounds): "
                "use ddmpc_set_data + ddmpc_solve");
  if (h->bounded)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_solve_from_host does not serve a handle with input bounds (ddmpc_set_input_bounds): "
                "use ddmpc_set_data + ddmpc_solve");
  h->gpre_valid = false;
  if (select_route(h) != Route::Cold) {   // no chunked cold launches beyond the register-resident kernels: plain upload + solve
    int rcs = ddmpc_set_data(h, u_d, y_d, DDMPC_MEM_HOST);
    return rcs ? rcs : ddmpc_solve(h, u_past, y_past, u_opt, cost, status, iters, DDMPC_MEM_HOST);
  }
  HIP_TRY(hipSetDevice(h->device));
  const ddmpc_params& p = h->prm;
  const size_t B = (size_t)h->batch;
  const size_t su = (size_t)p.N * p.m, sy = (size_t)p.N * p.p;                 // doubles per instance
  const size_t sup = (size_t)p.n * p.m, syp = (size_t)p.n * p.p, suo = (size_t)p.L * p.m;
  int rc;
  if ((rc = h->d_ud.ensure(B * su * sizeof(double))) || (rc = h->d_yd.ensure(B * sy * sizeof(double))) ||
      (rc = h->d_up.ensure(B * sup * sizeof(double))) || (rc = h->d_yp.ensure(B * syp * sizeof(double))) ||
      (rc = h->d_uopt.ensure(B * suo * sizeof(double))) || (rc = h->d_cost.ensure(B * sizeof(double))) ||
      (rc = h->d_status.ensure(B * sizeof(int32_t))) || (rc = h->d_iters.ensure(B * sizeof(int32_t))))
    return rc;
  if (!h->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  double *dud = (double*)h->d_ud.p, *dyd = (double*)h->d_yd.p, *dup = (double*)h->d_up.p, *dyp = (double*)h->d_yp.p;
  double *duo = (double*)h->d_uopt.p, *dco = (double*)h->d_cost.p;
  int32_t *dst = (int32_t*)h->d_status.p, *dit = (int32_t*)h->d_iters.p;
  {   // earlier asynchronous work on the compute stream may still read the buffers the uploads overwrite
    hipEvent_t ev0;
    HIP_TRY(hipEventCreateWithFlags(&ev0, hipEventDisableTiming));
    hipError_t e0 = hipEventRecord(ev0, h->stream);
    if (e0 == hipSuccess) e0 = hipStreamWaitEvent(h->copy_stream, ev0, 0);
    (void)hipEventDestroy(ev0);
    if (e0 != hipSuccess) return fail(DDMPC_ERR_HIP, "ddmpc_solve_from_host: %s", hipGetErrorString(e0));
  }
  begin_solve(h, Route::Cold);
  HIP_TRY(hipMemcpyAsync(dup, u_past, B * sup * sizeof(double), hipMemcpyHostToDevice, h->copy_stream));
  HIP_TRY(hipMemcpyAsync(dyp, y_past, B * syp * sizeof(double), hipMemcpyHostToDevice, h->copy_stream));
  // chunks of instances: upload chunk k+1 on the copy stream while chunk k is being solved on the compute stream
  const size_t nchunks = B >= 2048 ? 8 : (B >= 256 ? 4 : 1);
  hipEvent_t ev[8];
  for (size_t k = 0; k < nchunks; ++k) HIP_TRY(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
  // refinement (see launch_cold): ALWAYS -> the refining kernel variant per chunk; AUTO -> the chunks flag the instances
  // that need it and refine_flagged follows the last chunk.  Trajectories beyond the LDS: the chunks write beta / the active
  // set for the streamed residual check.
  const bool refinable = h->kp.lam != 0.0;
  const bool always = refinable && h->kp.refine == DDMPC_REFINE_ALWAYS, autoref = refinable && h->kp.refine == DDMPC_REFINE_AUTO;
  if ((rc = reserve_cold(h, h->long_data, autoref))) return rc;
  if (!h->long_data) h->last.beta = BetaState::ReSolveCold;
  KParams kchunk = h->kp;
  kchunk.epoch = next_refine_epoch(h);
  h->flag_epoch = kchunk.epoch;
  int rcl = DDMPC_OK;
  for (size_t k = 0; k < nchunks && rcl == DDMPC_OK; ++k) {
    const size_t b0 = B * k / nchunks, b1 = B * (k + 1) / nchunks, nb = b1 - b0;
    if (hipMemcpyAsync(dud + b0 * su, u_d + b0 * su, nb * su * sizeof(double), hipMemcpyHostToDevice, h->copy_stream) != hipSuccess ||
        hipMemcpyAsync(dyd + b0 * sy, y_d + b0 * sy, nb * sy * sizeof(double), hipMemcpyHostToDevice, h->copy_stream) != hipSuccess ||
        hipEventRecord(ev[k], h->copy_stream) != hipSuccess || hipStreamWaitEvent(h->stream, ev[k], 0) != hipSuccess) {
      rcl = fail(DDMPC_ERR_HIP, "ddmpc_solve_from_host: upload of chunk %zu failed", k);
      break;
    }
    KParams kck = kchunk;
    ColdArgs a{dud + b0 * su, dyd + b0 * sy, dup + b0 * sup, dyp + b0 * syp, duo + b0 * suo, dco + b0, dst + b0, dit + b0};
    if ((rcl = gram_pre_launch(h, kck, a.ud, a.yd, nb, b0, false))) break;
    if (h->long_data) { a.beta = (double*)h->d_beta.p + b0 * h->kp.rE; a.act = (signed char*)h->d_act.p + b0 * h->kp.rE; }
    if (autoref) { a.flag = (int*)h->d_rflag.p + b0; a.count = (int*)h->d_rflag.p + B; }
    enqueue_cold(h, always ? ColdPass::Refine : ColdPass::Plain, kck, a, nb);
    if (hipGetLastError() != hipSuccess) rcl = fail(DDMPC_ERR_HIP, "ddmpc_solve_from_host: launch of chunk %zu failed", k);
  }
  if (rcl == DDMPC_OK && h->gram_pre) {           // every chunk's Gram tiles are in place: they serve the launches below
    h->gpre_valid = true;
    h->ud = dud; h->yd = dyd;
    rcl = gram_pre_launch(h, kchunk, dud, dyd, B, 0, true);
  }
  if (rcl == DDMPC_OK && autoref) {
    ColdArgs a{dud, dyd, dup, dyp, duo, dco, dst, dit};
    // the chunks wrote beta / active set: the refining pass corrects those of the instances it refines (as in launch_cold)
    if (h->last.beta == BetaState::Written) { a.beta = (double*)h->d_beta.p; a.act = (signed char*)h->d_act.p; }
    rcl = refine_flagged(h, kchunk, a);
  }
  if (rcl == DDMPC_OK) {            // NOMINAL on exact data: same rank-revealing rescue as ddmpc_solve (all chunks are uploaded
    h->ud = dud; h->yd = dyd;       // and solved by now in stream order)
    rcl = launch_nominal_rescue(h, Route::Cold, dup, dyp, duo, dco, dst, dit);
  }
  if (rcl == DDMPC_OK) {
    if (hipMemcpyAsync(u_opt, duo, B * suo * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(cost, dco, B * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(status, dst, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        (iters && hipMemcpyAsync(iters, dit, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess))
      rcl = fail(DDMPC_ERR_HIP, "ddmpc_solve_from_host: download failed");
  }
  (void)hipStreamSynchronize(h->copy_stream);
  (void)hipStreamSynchronize(h->stream);
  for (size_t k = 0; k < nchunks; ++k) (void)hipEventDestroy(ev[k]);
  if (rcl != DDMPC_OK) return rcl;
  h->ud = dud; h->yd = dyd;
  h->have_data = true;
  forget_prep(h);
  end_solve(h, dup, dyp);
  return DDMPC_OK;
}

// ---- ddmpc_prepare on the register-resident routes (Route::Cold, Route::BoxLaw), step by step ----

// AUTO decides from the exact-Hankel residual of a solve, which depends on the right-hand side -- and the factor-export
// solve of ddmpc_prepare runs at the ZERO past window (with zero setpoints its right-hand side vanishes: beta = 0, residual 0,
// nothing would ever be flagged).  So the data sets are probed once more with a plain solve at the window a controller
// starts from, the last n steps of its own data (controller.py:184-185), and the two sets of flags are joined.
static int prep_probe_tail(ddmpc_handle* h, const KParams& k0) {
  const ddmpc_params& p = h->prm;
  const size_t B = (size_t)h->batch;
  const int npu = p.n * p.m, npy = p.n * p.p;
  int rc;
  if ((rc = h->d_status.ensure(B * sizeof(int32_t))) || (rc = h->d_need.ensure((B + 1) * sizeof(int)))) return rc;
  double* pu = (double*)h->d_zero.p;
  double* py = pu + B * (size_t)npu;
  hipLaunchKernelGGL(ddmpc_tail_past_kernel, dim3((unsigned)((B * (size_t)(npu + npy) + 255) / 256)), dim3(256), 0, h->stream,
                     (long long)B, p.N, p.m, p.p, p.n, h->ud, h->yd, pu, py);
  HIP_TRY(hipMemsetAsync(h->d_need.p, 0, (B + 1) * sizeof(int), h->stream));
  KParams kprobe = k0;
  kprobe.epoch = h->prep.epoch;
  if ((rc = gram_pre_launch(h, kprobe, h->ud, h->yd, B, 0, true))) return rc;
  ColdArgs a{h->ud, h->yd, pu, py, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_status.p};
  a.flag = (int*)h->d_need.p; a.count = a.flag + B;
  enqueue_cold(h, ColdPass::Plain, kprobe, a, B);       // (k0: no slack box, so the plain kernel fn2)
  hipLaunchKernelGGL(ddmpc_or_flags_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, (long long)B,
                     h->prep.epoch, (const int*)h->d_need.p, (int*)h->d_rflag.p);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// DDMPC_OPT_CONVEX_WARM_LAW: the boxed components, whose columns M = K0^-1 E_box are nbox more right-hand sides of the gain
// kernel.  Route::BoxLaw (umin / umax given): the same for its whole box list, the slack components (CONVEX) and the free input
// rows of the channels with a finite bound in ascending row order, with the table of ddmpc_box_law.hpp.  Host arithmetic on the
// parameter tables (ti: 3 rows, td: 4 rows of RP entries; td is read under bounds only).  Output bounds (ymin / ymax given) add
// the K_WPRED rows of the channels with a finite bound as components of a third kind, after the slack component of the same
// row where there is one; the two share their column of M, so M is keyed by boxed row (ncol <= nbox columns) and the table
// grows by [col | box_ofy | ncol | col_rho] (ddmpc_box_law.hpp).  Without them the list is the one it was.
struct BoxList {
  int nbox = 0;
  int ncol = 0;                // columns of M: the boxed rows (= nbox without output bounds)
  std::vector<int> tab;        // [rows of the boxed components | per row its place in the list, or -1]  (+ the output part)
  std::vector<double> bd;      // Route::BoxLaw: [a | c | lo | hi | 1/d] per boxed component
};
static BoxList build_box_list(const KParams& k, int RP, const std::vector<int>& ti, const std::vector<double>& td,
                              const double* umin, const double* umax, const double* ymin = nullptr, const double* ymax = nullptr,
                              bool slack_bd = false) {
  const bool box = umin != nullptr || ymin != nullptr || slack_bd;     // (slack_bd: the table of a slack-only list, DDMPC_OPT_SETPOINT_CONVEX_LAW)
  BoxList bl;
  std::vector<int>& tab = bl.tab;
  std::vector<int> box_of((size_t)k.r, -1), box_ofy, col, col_rho;
  std::vector<char> outp;      // per component: the output of its row
  if (ymin) box_ofy.assign((size_t)k.r, -1);
  auto bounded_row = [&](int rho) {
    const int ch = rho % k.nch;
    return umin != nullptr && ti[rho] == K_UFREE && (std::isfinite(umin[ch]) || std::isfinite(umax[ch]));
  };
  auto bounded_output = [&](int rho) {
    const int cy = rho % k.nch - k.m;
    return ymin != nullptr && ti[rho] == K_WPRED && (std::isfinite(ymin[cy]) || std::isfinite(ymax[cy]));
  };
  for (int rho = 0; rho < k.r; ++rho) {
    const bool first = (k.convex && (ti[rho] == K_WPRED || ti[rho] == K_WTERM)) || bounded_row(rho), second = bounded_output(rho);
    if (first) { box_of[rho] = (int)tab.size(); tab.push_back(rho); outp.push_back(0); col.push_back((int)col_rho.size()); }
    if (second) { box_ofy[rho] = (int)tab.size(); tab.push_back(rho); outp.push_back(1); col.push_back((int)col_rho.size()); }
    if (first || second) col_rho.push_back(rho);
  }
  const int nbox = bl.nbox = (int)tab.size();
  bl.ncol = (int)col_rho.size();
  if (box) {
    bl.bd.resize(5 * (size_t)nbox);
    for (int s = 0; s < nbox; ++s) {
      const int rho = tab[s], ch = rho % k.nch;
      const double D0 = td[rho], D1 = td[RP + rho];
      const bool inp = ti[rho] == K_UFREE;
      if (outp[s]) {           // hat = y_s - lam beta / q, held at y_min / y_max: d = lam / q (D1 = 1 / q on a K_WPRED row)
        bl.bd[0 * nbox + s] = td[2 * RP + rho];
        bl.bd[1 * nbox + s] = -k.lam * D1;
        bl.bd[2 * nbox + s] = ymin[ch - k.m];
        bl.bd[3 * nbox + s] = ymax[ch - k.m];
        bl.bd[4 * nbox + s] = 1.0 / (k.lam * D1);
        continue;
      }
      bl.bd[0 * nbox + s] = inp ? td[2 * RP + rho] : 0.0;
      bl.bd[1 * nbox + s] = inp ? -k.lam * D0 : k.sig_scale;
      bl.bd[2 * nbox + s] = inp ? umin[ch] : -k.bound;
      bl.bd[3 * nbox + s] = inp ? umax[ch] : k.bound;
      bl.bd[4 * nbox + s] = 1.0 / (k.lam * (inp ? D0 : D0 - D1));
    }
  }
  tab.insert(tab.end(), box_of.begin(), box_of.end());
  if (ymin) {
    tab.insert(tab.end(), col.begin(), col.end());
    tab.insert(tab.end(), box_ofy.begin(), box_ofy.end());
    tab.push_back(bl.ncol);
    tab.insert(tab.end(), col_rho.begin(), col_rho.end());
  }
  return bl;
}

// ... its tables on the device, room for M and the k x k scratch beyond the LDS, and the refined-law flags (+ count) cleared.
static int upload_box_list(ddmpc_handle* h, const BoxList& bl, bool box) {
  const size_t B = (size_t)h->batch;
  int rc;
  if (box) {
    if ((rc = h->d_box_bd.ensure(bl.bd.size() * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpy(h->d_box_bd.p, bl.bd.data(), bl.bd.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if ((rc = h->d_cwl_tab.ensure(bl.tab.size() * sizeof(int))) || (rc = h->d_mcol.ensure(B * (size_t)bl.ncol * h->kp.r * sizeof(double))) ||
      (rc = h->d_cwl_ref.ensure((B + 1) * sizeof(int))))
    return rc;
  if (bl.nbox > CWL_KLDS && (rc = h->d_cwl_sg.ensure(B * (size_t)(bl.nbox * (bl.nbox + 1) / 2) * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpy(h->d_cwl_tab.p, bl.tab.data(), bl.tab.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(h->d_cwl_ref.p, 0, (B + 1) * sizeof(int), h->stream));
  return DDMPC_OK;
}

// The affine law (and M for nbox boxed components) by substitutions through the exported factor.
static int enqueue_gain(ddmpc_handle* h, int nf, int nbox, const int* box_rho) {
  const int NT = h->kc.NT;
  bool launched = false;
#define DDMPC_INSTANCE(NT_, W_)                                                                              \
  if (!launched && NT == NT_) {                                                                               \
    const size_t glds = (size_t)(2 * NT_ * 256 + 32) * sizeof(double);                                        \
    if (glds > 64 * 1024)                                                                                     \
      HIP_TRY(raise_lds_limit((const void*)ddmpc_gain_kernel<NT_>, glds)); \
    hipLaunchKernelGGL(ddmpc_gain_kernel<NT_>, dim3((unsigned)h->batch), dim3(256), glds, h->stream, h->kp, 16 * NT, nf, \
                       (const double*)h->d_lfac.p, (const double*)h->d_lfacT.p, (const double*)h->d_beta.p,  \
                       (double*)h->d_gain.p, nbox, box_rho, (double*)h->d_mcol.p);                            \
    launched = true;                                                                                          \
  }
#include "ddmpc_instances.inc"
#undef DDMPC_INSTANCE
  if (!launched) return fail(DDMPC_ERR_UNSUPPORTED, "no gain kernel for %d tile rows", NT);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// The substitutions of the gain kernel went through the unrefined factor, whose error is the Gram route's (cond(H) squared).
// Replace columns of the law by refining cold solves: beta is affine in the past window, so column 1 + f =
// beta(e_f) - beta(0).  nf + 1 launches of the refining kernel variant, once per data set -- ALWAYS: for every
// instance; AUTO: a filtered launch that only works on the instances the factor-export launch flagged (it reads one
// word per workgroup and leaves when there is none: the benchmark data).
static int prep_refine_columns(ddmpc_handle* h, const KParams& k0) {
  const ddmpc_params& p = h->prm;
  const KParams& k = h->kp;
  const size_t B = (size_t)h->batch;
  const int nrhs = p.n * k.nch + 1;
  const bool flagged_only = k.refine == DDMPC_REFINE_AUTO;
  const int npu = p.n * p.m, npy = p.n * p.p;
  double* pu = (double*)h->d_zero.p;               // the zero past window of the factor export becomes e_f (its own buffer:
  double* py = pu + B * (size_t)npu;               // the handle's staging buffers may hold a caller's window)
  KParams kr = k0;
  kr.refine = DDMPC_REFINE_ALWAYS;
  ColdSeq sr; sr.kp = &kr;
  ColdArgs a{h->ud, h->yd, pu, py, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_prep_status.p};
  a.beta = (double*)h->d_beta.p; a.act = (signed char*)h->d_act.p;
  const unsigned gp = (unsigned)((B * (size_t)(npu + npy) + 255) / 256), gg = (unsigned)((B * (size_t)k.r + 255) / 256);
  for (int j = 0; j < nrhs; ++j) {
    hipLaunchKernelGGL(ddmpc_unit_past_kernel, dim3(gp), dim3(256), 0, h->stream, (long long)B, npu, npy, j - 1,
                       pu, py);
    if (!flagged_only) {
      if (int rc = launch_cold(h, pu, py, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_prep_status.p, nullptr, sr))
        return rc;
    } else {
      // (trajectory beyond the LDS: the flags are those of the a-priori bound alone, no streamed check)
      kr.epoch = h->prep.epoch;
      if (int rc = gram_pre_launch(h, kr, h->ud, h->yd, B, 0, true)) return rc;
      enqueue_cold(h, ColdPass::Filtered, kr, a, B);
    }
    hipLaunchKernelGGL(ddmpc_gain_column_kernel, dim3(gg), dim3(256), 0, h->stream, (long long)B, k.r, k.rE, nrhs, j,
                       (const double*)h->d_beta.p, (double*)h->d_gain.p,
                       flagged_only ? (const int*)h->d_rflag.p : (const int*)nullptr, h->prep.epoch);
  }
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// DDMPC_OPT_SETPOINT_LAW: S = K0^-1 [1_0 .. 1_{m+p-1}] by substitutions through the exported factor (queued behind enqueue_gain,
// while d_lfac / d_lfacT are alive).
static int enqueue_setpoint_gain(ddmpc_handle* h) {
  const int NT = h->kc.NT;
  bool launched = false;
#define DDMPC_INSTANCE(NT_, W_)                                                                              \
  if (!launched && NT == NT_) {                                                                               \
    const size_t glds = (size_t)(2 * NT_ * 256 + 32) * sizeof(double);                                        \
    if (glds > 64 * 1024)                                                                                     \
      HIP_TRY(raise_lds_limit((const void*)ddmpc_setpoint_gain_kernel<NT_>, glds));                           \
    hipLaunchKernelGGL(ddmpc_setpoint_gain_kernel<NT_>, dim3((unsigned)h->batch), dim3(256), glds, h->stream, h->kp, 16 * NT, \
                       (const double*)h->d_lfac.p, (const double*)h->d_lfacT.p, (double*)h->d_sgain.p);      \
    launched = true;                                                                                          \
  }
#include "ddmpc_instances.inc"
#undef DDMPC_INSTANCE
  if (!launched) return fail(DDMPC_ERR_UNSUPPORTED, "no setpoint gain kernel for %d tile rows", NT);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// ... and, like the columns of the law (prep_refine_columns: same launches, same flag filter), replaced by refining cold solves:
// column c is the beta of a solve at the zero past window whose KParams copy points `tabd` at a scratch copy of the tables with
// the unit setpoint e_c in row 2 -- its right-hand side is 1_c, so there is no offset to subtract.  The handle's tables are
// only read.  m + p launches of the refining kernel variant, once per data set.
static int prep_refine_setpoint_columns(ddmpc_handle* h, const KParams& k0) {
  const ddmpc_params& p = h->prm;
  const KParams& k = h->kp;
  const size_t B = (size_t)h->batch;
  const int RP = 16 * h->kc.NT, nch = k.nch;
  const bool flagged_only = k.refine == DDMPC_REFINE_AUTO;
  const int npu = p.n * p.m, npy = p.n * p.p;
  if (int rc = h->d_sptab.ensure((size_t)nch * 4 * RP * sizeof(double))) return rc;
  double* pu = (double*)h->d_zero.p;               // (prep_refine_columns left a unit window there)
  double* py = pu + B * (size_t)npu;
  const unsigned gp = (unsigned)((B * (size_t)(npu + npy) + 255) / 256), gg = (unsigned)((B * (size_t)k.r + 255) / 256);
  hipLaunchKernelGGL(ddmpc_unit_past_kernel, dim3(gp), dim3(256), 0, h->stream, (long long)B, npu, npy, -1, pu, py);
  hipLaunchKernelGGL(ddmpc_setpoint_tables_kernel, dim3((unsigned)((nch * 4 * RP + 255) / 256)), dim3(256), 0, h->stream, RP, nch,
                     k.tabd, (double*)h->d_sptab.p);
  KParams kr = k0;
  kr.refine = DDMPC_REFINE_ALWAYS;
  ColdSeq sr; sr.kp = &kr;
  ColdArgs a{h->ud, h->yd, pu, py, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_prep_status.p};
  a.beta = (double*)h->d_beta.p; a.act = (signed char*)h->d_act.p;
  for (int c = 0; c < nch; ++c) {
    kr.tabd = (const double*)h->d_sptab.p + (size_t)c * 4 * RP;
    if (!flagged_only) {
      if (int rc = launch_cold(h, pu, py, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_prep_status.p, nullptr, sr))
        return rc;
    } else {
      kr.epoch = h->prep.epoch;
      if (int rc = gram_pre_launch(h, kr, h->ud, h->yd, B, 0, true)) return rc;
      enqueue_cold(h, ColdPass::Filtered, kr, a, B);
    }
    hipLaunchKernelGGL(ddmpc_setpoint_gain_column_kernel, dim3(gg), dim3(256), 0, h->stream, (long long)B, k.r, k.rE, nch, c,
                       (const double*)h->d_beta.p, (double*)h->d_sgain.p,
                       flagged_only ? (const int*)h->d_rflag.p : (const int*)nullptr, h->prep.epoch);
  }
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// Factor export, AUTO probe, box list, gain launch, refined columns, refined-instance mark and its count, in this order.
static int prepare_register_resident(ddmpc_handle* h, bool box) {
  const ddmpc_params& p = h->prm;
  const KParams& k = h->kp;
  const int nf = p.n * k.nch, nrhs = nf + 1, NT = h->kc.NT;
  if (nf > WARM_MAX_NF) return fail(DDMPC_ERR_UNSUPPORTED, "warm path supports n*(m+p) <= %d", WARM_MAX_NF);
  const size_t B = (size_t)h->batch;
  const size_t lf_bytes = B * (size_t)(NT * (NT + 1) / 2) * 256 * sizeof(double);
  h->last.valid = false;                           // (the launches below overwrite the outputs and the workspace of the last solve)
  int rc;
  if ((rc = h->d_lfac.ensure(lf_bytes)) || (rc = h->d_lfacT.ensure(lf_bytes)) || (rc = h->d_gain.ensure(B * nrhs * k.r * sizeof(double))) ||
      (rc = h->d_prep_status.ensure(B * sizeof(int32_t))) || (rc = h->d_zero.ensure(B * nf * sizeof(double))) ||
      (rc = h->d_uopt.ensure(B * p.L * p.m * sizeof(double))) || (rc = h->d_cost.ensure(B * sizeof(double))))
    return rc;
  HIP_TRY(hipMemsetAsync(h->d_zero.p, 0, B * nf * sizeof(double), h->stream));
  const double* z = (const double*)h->d_zero.p;
  // one cold factorisation with the factor exported (its solution for a zero past window is discarded)
  KParams k0 = h->kp;                              // slack box: factor of the EMPTY active set (one iteration)
  k0.convex = 0;
  ColdSeq s0; s0.kp = &k0; s0.lfac = (double*)h->d_lfac.p; s0.lfacT = (double*)h->d_lfacT.p;
  if ((rc = launch_cold(h, z, z + B * p.n * p.m, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_prep_status.p, nullptr, s0)))
    return rc;
  const bool refinable = k.lam != 0.0;
  if (refinable && k.refine == DDMPC_REFINE_AUTO && (rc = prep_probe_tail(h, k0))) return rc;
  if (B * (size_t)(NT * (NT + 1) / 2) > 0x7fffffffULL) return fail(DDMPC_ERR_INVALID, "batch too large for ddmpc_prepare");
  const bool spc = !box && setpoint_convex_slack_only(h);   // (the slack-only list with its table, for the setpoint calls alone)
  const bool cwl = convex_warm_on(h) || box || spc;
  int nbox = 0, ncol = 0;
  const int* col_rho = nullptr;                    // output bounds: the rows of M's columns (the end of the table)
  if (cwl) {
    const int RP = 16 * NT;
    std::vector<int> ti;
    std::vector<double> td;
    if (box) HIP_TRY(hipStreamSynchronize(h->stream));     // (a step in flight may still read the tables written below)
    if (spc) HIP_TRY(hipStreamSynchronize(h->stream));     // (a setpoint step in flight may still read d_box_bd)
    if ((rc = read_table(h->d_tabi, 3 * (size_t)RP, &ti)) || ((box || spc) && (rc = read_table(h->d_tabd, 4 * (size_t)RP, &td)))) return rc;
    const bool ub = box && !h->umin_h.empty(), yb = box && !h->ymin_h.empty();
    const BoxList bl = build_box_list(k, RP, ti, td, ub ? h->umin_h.data() : nullptr, ub ? h->umax_h.data() : nullptr,
                                      yb ? h->ymin_h.data() : nullptr, yb ? h->ymax_h.data() : nullptr, spc);
    // (thread s of the box kernels looks at component s, and the LDS arrays by component hold WARM_MAX_R entries)
    if (bl.nbox > WARM_MAX_R)
      return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: the box list has %d components (slack, input and output), the kernels hold %d",
                  bl.nbox, WARM_MAX_R);
    if ((rc = upload_box_list(h, bl, box || spc))) return rc;
    nbox = bl.nbox;
    ncol = bl.ncol;
    if (yb) col_rho = (const int*)h->d_cwl_tab.p + 2 * (nbox + k.r) + 1;
    h->prep.box_threads = (int)warm_threads(std::max(k.r, nbox));
  }
  h->prep.cwl_nbox = nbox;
  if ((rc = enqueue_gain(h, nf, ncol, col_rho ? col_rho : (const int*)h->d_cwl_tab.p))) return rc;
  // DDMPC_OPT_SETPOINT_LAW / _SETPOINT_BOX_LAW / _SETPOINT_CONVEX_LAW (ROBUST, refinable): S comes from k0, the empty set's system, and knows no bounds
  const bool setpoint = setpoint_on(h);
  if (setpoint && (box || spc)) {                  // the bounds per channel, for the per-instance refusal of ddmpc_setpoint_box_law.hpp
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> cb(2 * (size_t)k.nch);
    for (int c = 0; c < k.nch; ++c) {
      const std::vector<double>& lo = c < k.m ? h->umin_h : h->ymin_h;
      const std::vector<double>& hi = c < k.m ? h->umax_h : h->ymax_h;
      const int ch = c < k.m ? c : c - k.m;
      cb[c] = lo.empty() ? -inf : lo[ch];
      cb[k.nch + c] = hi.empty() ? inf : hi[ch];
    }
    if ((rc = h->d_chbnd.ensure(cb.size() * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_chbnd.p, cb.data(), cb.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));      // (cb is pageable host memory: the copy has left it)
  }
  if (setpoint && ((rc = h->d_sgain.ensure(B * (size_t)k.nch * k.r * sizeof(double))) || (rc = enqueue_setpoint_gain(h)))) return rc;
  if (refinable && (k.refine == DDMPC_REFINE_ALWAYS || k.refine == DDMPC_REFINE_AUTO) && (rc = prep_refine_columns(h, k0))) return rc;
  if (setpoint && refinable && (k.refine == DDMPC_REFINE_ALWAYS || k.refine == DDMPC_REFINE_AUTO) &&
      (rc = prep_refine_setpoint_columns(h, k0)))
    return rc;
  h->prep.setpoint = setpoint;
  if (cwl) {
    // M comes from the unrefined factor: instances whose law was refined keep the filtered cold launch for their box
    // (ddmpc_step), and their presence sends ddmpc_closed_loop to the per-step path
    const int mode = refinable ? k.refine : DDMPC_REFINE_OFF;
    hipLaunchKernelGGL(ddmpc_cwl_mark_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, (long long)B, mode,
                       h->prep.epoch, (const int*)h->d_rflag.p, (int*)h->d_cwl_ref.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->prep.cwl_nref = 0;
  if (cwl) HIP_TRY(hipMemcpy(&h->prep.cwl_nref, (const int*)h->d_cwl_ref.p + B, sizeof(int), hipMemcpyDeviceToHost));
  h->d_lfac.release();                           // the factor is only needed to form the gain
  h->d_lfacT.release();
  h->prep.valid = true;
  return DDMPC_OK;
}

int ddmpc_prepare(ddmpc_handle* h) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (!h->have_data) return fail(DDMPC_ERR_NOT_READY, "ddmpc_set_data must be called before ddmpc_prepare");
  if (h->batch > 0x7fffffffLL) return fail(DDMPC_ERR_INVALID, "batch too large for one launch");
  if (prep_valid(h)) return DDMPC_OK;
  h->gpre_valid = false;
  const Route route = select_route(h);
  forget_prep(h);                         // (until the route's preparation below has been queued in full)
  h->prep.route = route;
  HIP_TRY(hipSetDevice(h->device));
  if (nominal_route(route)) {
    // no affine law at this size, but everything that depends on the data alone -- Gram, its rank-revealing factor, the
    // reduced normal matrix and its factor, 70 % of a solve -- is formed once and kept in the workspace; ddmpc_step and
    // the per-step closed loop then only redo the substitutions and the refinement passes
    int rc = h->d_prep_status.ensure((size_t)h->batch * sizeof(int32_t));
    if (!rc) rc = launch_nominal_rescue(h, route, h->ud, h->yd, nullptr, nullptr, (int32_t*)h->d_prep_status.p, nullptr, Stage::Factors);
    if (!rc && h->large_affine && route == Route::NominalPhases && h->d_rr.p) rc = launch_rr2_gain_build(h, (double*)h->d_rr.p, rr2_ndbl(h));
    h->prep.valid = rc == DDMPC_OK;
    return rc;
  }
  const bool box = route == Route::BoxLaw;
  if (route != Route::Cold && !box) {     // ROBUST at this size: Gram + lam D, the factor of the columns outside the slack box and
                                          // the Schur complement of the boxed block are formed once and kept
    int rc = launch_large_robust(h, route, Stage::Factors, h->ud, h->yd, nullptr, nullptr, nullptr, nullptr);
    if (!rc && (h->large_affine || rr3_box_law(h)) && route == Route::RobustPhases) rc = launch_rr3_law_build(h);   // ... and the affine law on that factor
    h->prep.valid = rc == DDMPC_OK;
    return rc;
  }
  return prepare_register_resident(h, box);
}

int ddmpc_step(ddmpc_handle* h, const double* u_past, const double* y_past, double* u_opt, double* cost,
               int32_t* status, int32_t* iters, int mem) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (!h->have_data) return fail(DDMPC_ERR_NOT_READY, "ddmpc_set_data must be called before ddmpc_step");
  if (!prep_valid(h)) {
    int rc = ddmpc_prepare(h);
    if (rc) return rc;
  }
  return solve_impl(h, u_past, y_past, u_opt, cost, status, iters, mem, &step_on_route);
}

int ddmpc_get_gain(ddmpc_handle* h, double* out, int mem) {
  if (!h || !out) return fail(DDMPC_ERR_INVALID, "null argument");
  if (h->large && !h->large_affine && !(rr3_box_law(h) && select_route(h) == Route::RobustPhases))
    return fail(DDMPC_ERR_UNSUPPORTED, "no affine law at this problem size without DDMPC_OPT_LARGE_AFFINE_LAW");
  if (!prep_valid(h) || (h->large && !h->prep.law)) return fail(DDMPC_ERR_NOT_READY, "ddmpc_prepare must be called before ddmpc_get_gain");
  HIP_TRY(hipSetDevice(h->device));
  // (beyond the register-resident kernels, NOMINAL: z = [ubar; ybar] (component order) = gain[:,0] + gain[:,1:]' [u_past; y_past];
  //  ROBUST: beta of the empty active set (component order) = gain[:,0] + gain[:,1:]' [u_past; y_past], as below 272 rows)
  const size_t bytes = (size_t)h->batch * (h->prm.n * h->kp.nch + 1) * h->kp.r * sizeof(double);
  HIP_TRY(hipMemcpyAsync(out, h->large ? h->d_gz.p : h->d_gain.p, bytes, mem == DDMPC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                         h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return DDMPC_OK;
}

// DDMPC_OPT_SETPOINT_LAW: one evaluation of the law and S with the setpoints of the call in progress (h->sp_us / h->sp_ys).
// DDMPC_OPT_SETPOINT_BOX_LAW on a handle with finite bounds (Route::BoxLaw): one launch of ddmpc_setpoint_box_step_kernel, from the
// empty set (DDMPC_OPT_BOX_WARM_START is not honoured, and the caller drops the seed with the record of the last solve).
// DDMPC_OPT_LARGE_SETPOINTS (Route::RobustPhases): the solve on the kept factors with the instance's setpoint.
// DDMPC_OPT_LARGE_SETPOINT_BOUNDS (the same route, with or without finite bounds): that solve, never the law or S.
static int setpoint_step_on_route(ddmpc_handle* h, const double* up, const double* yp, double* uo, double* cost, int32_t* status,
                                  int32_t* iters) {
  if (h->large_setpoints) {
    begin_solve(h, Route::RobustPhases);
    const Rr3Setpoint sp{h->sp_us, h->sp_ys, h->sp_su, h->sp_sy};
    if (h->large_affine && h->prep.law && h->prep.setpoint) return launch_rr3_setpoint_law_step(h, sp, up, yp, uo, cost, status, iters);
    return launch_rr3_solve(h, h->kp, up, yp, uo, cost, status, iters, nullptr, nullptr, false, &sp);
  }
  if (h->large_setpoint_bounds) {
    // (a bounded handle has a table: a ROBUST controller has L >= 2 n, so a finite bound of a channel boxes >= n free steps)
    begin_solve(h, Route::RobustPhases);
    const Rr3Setpoint sp{h->sp_us, h->sp_ys, h->sp_su, h->sp_sy};
    return launch_rr3_solve(h, h->kp, up, yp, uo, cost, status, iters, nullptr, nullptr, false, &sp);
  }
  const Route route = select_route(h);
  if (h->setpoint_convex_law || route == Route::BoxLaw) {
    // ddmpc_setpoint_box_step_kernel on the box list ddmpc_prepare kept.  DDMPC_OPT_SETPOINT_CONVEX_LAW: its SLACK instantiations --
    // the slack components alone (Route::Cold; no safeguard: the slack box does not cycle) or next to the bounded inputs / outputs
    begin_solve(h, route);
    // Per-instance bounds (instance_bounds, DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1): the BoxChannels instantiations with the channel table.
    const bool yb = !h->ymin_h.empty(), safe = route == Route::BoxLaw && h->box_safeguard;
    auto launch = [&](auto slack, auto... extra) {
      with_safe_yb(safe, yb, [&](auto safet, auto ybt) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ddmpc_setpoint_box_step_kernel<safet(), ybt(), slack(), decltype(extra)...>), dim3((unsigned)h->batch),
                           dim3(yb ? (unsigned)h->prep.box_threads : warm_threads(h->kp.r)), 0, h->stream, h->kp, 16 * h->kc.NT,
                           h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const double*)h->d_sgain.p,
                           (const int*)h->d_prep_status.p, up, yp, h->sp_us, h->sp_ys, uo, cost, (int*)status, (int*)iters,
                           h->prep.cwl_nbox, (const int*)h->d_cwl_tab.p, (const double*)h->d_box_bd.p, (const double*)h->d_mcol.p,
                           (double*)h->d_cwl_sg.p, h->prep.cwl_nref > 0 ? (const int*)h->d_cwl_ref.p : (const int*)nullptr,
                           (const double*)h->d_chbnd.p, (int)(h->prm.use_terminal_constraint != 0), extra...);
      });
    };
    if (instance_bounds(h)) {
      const BoxChannels chan{(const double*)h->d_ibnd.p};
      if (h->setpoint_convex_law) launch(std::true_type{}, chan); else launch(std::false_type{}, chan);
    } else {
      if (h->setpoint_convex_law) launch(std::true_type{}); else launch(std::false_type{});
    }
    HIP_TRY(hipGetLastError());
    return DDMPC_OK;
  }
  begin_solve(h, Route::Cold);
  hipLaunchKernelGGL(ddmpc_setpoint_step_kernel, dim3((unsigned)h->batch), dim3(warm_threads(h->kp.r)), 0, h->stream, h->kp,
                     16 * h->kc.NT, h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const double*)h->d_sgain.p,
                     (const int*)h->d_prep_status.p, up, yp, h->sp_us, h->sp_ys, uo, cost, (int*)status, (int*)iters);
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

int ddmpc_step_setpoints(ddmpc_handle* h, const double* u_past, const double* y_past, const double* u_s, const double* y_s,
                         double* u_opt, double* cost, int32_t* status, int32_t* iters, int mem) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (!setpoint_on(h))
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_step_setpoints needs DDMPC_OPT_SETPOINT_LAW = 1 (or DDMPC_OPT_SETPOINT_BOX_LAW = 1, or DDMPC_OPT_SETPOINT_CONVEX_LAW = 1 under the CONVEX slack box), or beyond 271 rows DDMPC_OPT_LARGE_SETPOINTS = 1 (on a handle with input or output bounds there: DDMPC_OPT_LARGE_SETPOINT_BOUNDS = 1)");
  if (h->bounded && !h->setpoint_box_law && !h->setpoint_convex_law && !h->large_setpoint_bounds)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_step_setpoints on a handle with input or output bounds needs DDMPC_OPT_SETPOINT_BOX_LAW = 1");
  if (!h->have_data) return fail(DDMPC_ERR_NOT_READY, "ddmpc_set_data must be called before ddmpc_step_setpoints");
  if (!u_s || !y_s) return fail(DDMPC_ERR_INVALID, "null argument");
  if (mem != DDMPC_MEM_HOST && mem != DDMPC_MEM_DEVICE) return fail(DDMPC_ERR_INVALID, "mem must be DDMPC_MEM_HOST or DDMPC_MEM_DEVICE");
  if (!prep_valid(h))
    if (int rc = ddmpc_prepare(h)) return rc;
  HIP_TRY(hipSetDevice(h->device));
  h->sp_us = u_s; h->sp_ys = y_s; h->sp_su = h->prm.m; h->sp_sy = h->prm.p;
  if (mem == DDMPC_MEM_HOST) {
    const size_t B = (size_t)h->batch, nu = B * h->prm.m, ny = B * h->prm.p;
    if (int rc = h->d_sp.ensure((nu + ny) * sizeof(double))) return rc;
    double* d = (double*)h->d_sp.p;
    HIP_TRY(hipMemcpyAsync(d, u_s, nu * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d + nu, y_s, ny * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->sp_us = d; h->sp_ys = d + nu;
  }
  const int rc = solve_impl(h, u_past, y_past, u_opt, cost, status, iters, mem, &setpoint_step_on_route);
  h->last = LastSolve{};               // nothing ddmpc_get_solution could reconstruct: its kernel reads the shared setpoint table
  h->last.setpoint_call = true;
  h->sp_us = h->sp_ys = nullptr;
  return rc;
}

int ddmpc_get_setpoint_gain(ddmpc_handle* h, double* out, int mem) {
  if (!h || !out) return fail(DDMPC_ERR_INVALID, "null argument");
  if (!setpoint_on(h))
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_get_setpoint_gain needs DDMPC_OPT_SETPOINT_LAW = 1 (or DDMPC_OPT_SETPOINT_BOX_LAW = 1, or DDMPC_OPT_SETPOINT_CONVEX_LAW = 1 under the CONVEX slack box), or beyond 271 rows DDMPC_OPT_LARGE_SETPOINTS = 1");
  if (h->large_setpoint_bounds && !h->large_setpoints)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_get_setpoint_gain: DDMPC_OPT_LARGE_SETPOINT_BOUNDS = 1 forms no S (beyond 271 rows there is no S on a "
                "bounded handle: its setpoint calls solve on the kept factors)");
  if (h->large_setpoints && (!prep_valid(h) || !h->prep.setpoint))
    return fail(DDMPC_ERR_NOT_READY, "ddmpc_get_setpoint_gain beyond 271 rows: S is formed next to the affine law only -- ddmpc_prepare with "
                "DDMPC_OPT_LARGE_AFFINE_LAW = 1 (and DDMPC_OPT_LARGE_SETPOINTS = 1) must be called before it");
  if (!prep_valid(h) || !h->prep.setpoint)
    return fail(DDMPC_ERR_NOT_READY, "ddmpc_prepare with DDMPC_OPT_SETPOINT_LAW = 1 (or DDMPC_OPT_SETPOINT_BOX_LAW = 1) must be called before "
                "ddmpc_get_setpoint_gain");
  HIP_TRY(hipSetDevice(h->device));
  const size_t bytes = (size_t)h->batch * h->kp.nch * h->kp.r * sizeof(double);
  HIP_TRY(hipMemcpyAsync(out, h->d_sgain.p, bytes, mem == DDMPC_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return DDMPC_OK;
}

int ddmpc_set_option(ddmpc_handle* h, int option, int value) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  switch (option) {
    case DDMPC_OPT_CLOSED_LOOP_PATH:
      if (value != DDMPC_PATH_AUTO && value != DDMPC_PATH_COLD && value != DDMPC_PATH_WARM)
        return fail(DDMPC_ERR_INVALID, "closed-loop path must be DDMPC_PATH_AUTO, _COLD or _WARM");
      h->closed_loop_path = value;
      return DDMPC_OK;
    case DDMPC_OPT_CLOSED_LOOP_GRAPH:
      h->closed_loop_graph = value != 0;
      return DDMPC_OK;
    case DDMPC_OPT_REFINE:
      if (value != DDMPC_REFINE_OFF && value != DDMPC_REFINE_AUTO && value != DDMPC_REFINE_ALWAYS)
        return fail(DDMPC_ERR_INVALID, "refinement mode must be DDMPC_REFINE_OFF, _AUTO or _ALWAYS");
      if (value == DDMPC_REFINE_ALWAYS && h->bounded && !h->large && h->umin_h.empty())
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_REFINE_ALWAYS is not available on a handle with output bounds (ddmpc_set_output_bounds)");
      if (value == DDMPC_REFINE_ALWAYS && h->bounded && !h->large)       // (M comes from the unrefined factor: no refined iteration on it)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_REFINE_ALWAYS is not available on a handle with input bounds (ddmpc_set_input_bounds)");
      h->kp.refine = value;
      forget_prep(h);                   // the affine law is formed from a refined solve of the offset column
      return DDMPC_OK;
    case DDMPC_OPT_REFINE_MAX:
      if (value < 1 || value > 10) return fail(DDMPC_ERR_INVALID, "refinement passes must be within [1, 10]");
      h->kp.refine_max = value;
      if (h->large_affine || h->large_box_law) forget_prep(h);   // the ROBUST law beyond 271 rows marks "no law" after refine_max passes
      return DDMPC_OK;
    case DDMPC_OPT_REFINE_RES_LOG10:
      if (value < 0 || value > 3000)
        return fail(DDMPC_ERR_INVALID, "refinement threshold (tenths of a decade below 1) must be within [0, 3000]");
      h->kp.refine_res = std::pow(10.0, -0.1 * (double)value);
      forget_prep(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_AFFINE_LAW:
      // (the law's step kernel evaluates the cost with the diagonal weights, and the law is built by the phase kernels: 1024 rows)
      if (value != 0 && h->large_nominal && (h->prm.weight_kind == DDMPC_WEIGHT_DENSE || h->kp.r > 1024))
        return fail(DDMPC_ERR_UNSUPPORTED, "the affine law of NOMINAL controllers beyond 271 rows takes scalar / diagonal weights and at most 1024 rows");
      // (ROBUST: the law step evaluates z with the diagonal weights, the law is built on the phase kernels, its step stages the window in LDS)
      if (value != 0 && h->large && !h->large_nominal &&
          (h->prm.weight_kind == DDMPC_WEIGHT_DENSE || h->kp.r > 1024 || h->prm.n * h->kp.nch > WARM_MAX_NF))
        return fail(DDMPC_ERR_UNSUPPORTED, "the affine law of ROBUST controllers beyond 271 rows takes scalar / diagonal weights, at most 1024 rows "
                    "and n*(m+p) <= %d", WARM_MAX_NF);
      if (value != 0 && h->large && h->bounded)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_AFFINE_LAW is not available on a handle with input or output bounds beyond 271 rows "
                    "(the law step knows no bounds)");
      h->large_affine = value != 0;
      forget_prep(h);
      return DDMPC_OK;
    case DDMPC_OPT_CONVEX_UPDATE:
      h->convex_update = value != 0;
      return DDMPC_OK;
    case DDMPC_OPT_CONVEX_WARM_LAW:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_CONVEX_WARM_LAW must be 0 or 1");
      if (value == 1 && h->kp.convex) {
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_CONVEX_WARM_LAW: dense weighting matrices are not supported with the slack box");
        if (h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_CONVEX_WARM_LAW: %d rows, the option covers the register-resident kernels "
                      "((m+p)(L+n) <= 271)", h->kp.r);
        // every boxed component must change its diagonal entry when its slack reaches the bound (d_s > 0): a zero output
        // weight makes 1/q swallow 1/lamb_sigma
        const int RP = 16 * h->kc.NT;
        std::vector<double> td;
        std::vector<int> ti;
        if (int rc = read_table(h->d_tabd, 4 * (size_t)RP, &td)) return rc;
        if (int rc = read_table(h->d_tabi, 3 * (size_t)RP, &ti)) return rc;
        for (int rho = 0; rho < h->kp.r; ++rho)
          if ((ti[rho] == K_WPRED || ti[rho] == K_WTERM) && !(td[rho] - td[RP + rho] > 0.0))
            return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_CONVEX_WARM_LAW: a boxed output component has no weight (Q entry 0)");
      }
      h->convex_warm = value;
      forget_prep(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_BOUNDS:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_BOUNDS must be 0 or 1");
      if (value == 0 && h->large && h->bounded)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_BOUNDS = 0 on a handle with input or output bounds beyond 271 rows: remove the "
                    "bounds first");
      h->large_bounds = value;            // (which calls are accepted: nothing prepared depends on it)
      h->last.large_seed = false;         // (DDMPC_OPT_LARGE_BOX_WARM_START: the next step starts from the empty set)
      return DDMPC_OK;
    case DDMPC_OPT_BOX_SAFEGUARD:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_BOX_SAFEGUARD must be 0 or 1");
      h->box_safeguard = value;           // (which instantiation of the box kernels is launched: nothing prepared depends on it)
      return DDMPC_OK;
    case DDMPC_OPT_BOX_WARM_START:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_BOX_WARM_START must be 0 or 1");
      h->box_warm = value;                // (which instantiation of the box kernels is launched: nothing prepared depends on it)
      h->last.box_seed = false;           // (setting it, to either value, drops the seed: the next step starts from the empty set)
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_BOX_CAPACITY:
      if (value != 64 && value != 128 && value != 192 && value != 256)
        return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_BOX_CAPACITY must be 64, 128, 192 or 256");
      h->large_box_cap = value;           // (which bounded phase kernel is launched and how its workspace is sized: the factors do not depend on it)
      forget_large_box_solve(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_BOX_SAFEGUARD:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_BOX_SAFEGUARD must be 0 or 1");
      h->large_box_safeguard = value;     // (which kernels serve a bounded handle beyond 271 rows and how their workspace is sized: the factors do not depend on it)
      forget_large_box_solve(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_BOX_WARM_START:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_BOX_WARM_START must be 0 or 1");
      h->large_box_warm = value;          // (with 1 the wide kernels serve a bounded handle beyond 271 rows at every capacity: the factors do not depend on it)
      forget_large_box_solve(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_BOX_LAW:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_BOX_LAW must be 0 or 1");
      // (the law is built on the phase kernels and its step stages the window in LDS: a shape check, whatever the bounds)
      if (value == 1 && h->large && h->prm.n * h->kp.nch > WARM_MAX_NF)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_LARGE_BOX_LAW: n*(m+p) = %d, the affine law beyond 271 rows supports n*(m+p) <= %d",
                    h->prm.n * h->kp.nch, WARM_MAX_NF);
      h->large_box_law = value;           // (ddmpc_prepare forms the law next to the factors: it is part of what is kept)
      forget_prep(h);
      forget_large_box_solve(h);
      return DDMPC_OK;
    case DDMPC_OPT_SETPOINT_LAW:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_SETPOINT_LAW must be 0 or 1");
      if (value == 1) {
        const char* pre = "DDMPC_OPT_SETPOINT_LAW";
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one fixes its outputs to the setpoint as hard rows)", pre);
        if (h->kp.convex)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: not with the CONVEX slack box (slack NONE only: the setpoint step runs no active-set iteration)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (h->prm.n * h->kp.nch > WARM_MAX_NF)     // (asked before the row count: L >= 2 n puts every such ROBUST handle beyond 271 rows)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: n*(m+p) = %d, the affine law of ddmpc_prepare holds %d", pre, h->prm.n * h->kp.nch, WARM_MAX_NF);
        if (h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels)", pre, h->kp.r);
        if (h->long_data)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: N = %d, the trajectory does not fit the LDS of the cold kernel (no refined columns there)", pre,
                      h->prm.N);
        if (h->bounded && !h->setpoint_box_law)     // (with DDMPC_OPT_SETPOINT_BOX_LAW = 1 that option governs)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s is not available on a handle with input or output bounds (the setpoint step knows no bounds)", pre);
      }
      if (h->setpoint_law != value) forget_prep(h);     // (S is part of what ddmpc_prepare keeps)
      h->setpoint_law = value;
      return DDMPC_OK;
    case DDMPC_OPT_SETPOINT_BOX_LAW:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_SETPOINT_BOX_LAW must be 0 or 1");
      if (value == 1) {                                 // (the refusals of DDMPC_OPT_SETPOINT_LAW but the one of bounds)
        const char* pre = "DDMPC_OPT_SETPOINT_BOX_LAW";
        if (instance_bounds(h) && !h->instance_setpoint_bounds)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: not on a handle with per-instance bounds (ddmpc_set_instance_input_bounds / "
                      "_output_bounds: the setpoint kernels read the bounds shared by the batch)", pre);
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one fixes its outputs to the setpoint as hard rows)", pre);
        if (h->kp.convex)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: not with the CONVEX slack box (slack NONE only: a slack-only CONVEX handle runs on other kernels, "
                      "and the offsets of its slack components are not setpoints)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (h->prm.n * h->kp.nch > WARM_MAX_NF)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: n*(m+p) = %d, the affine law of ddmpc_prepare holds %d", pre, h->prm.n * h->kp.nch, WARM_MAX_NF);
        if (h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels: beyond them the phase "
                      "kernels have no M)", pre, h->kp.r);
        if (h->long_data)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: N = %d, the trajectory does not fit the LDS of the cold kernel (no refined columns there)", pre,
                      h->prm.N);
      }
      if (h->setpoint_box_law != value) forget_prep(h);   // (S is part of what ddmpc_prepare keeps)
      h->setpoint_box_law = value;
      return DDMPC_OK;
    case DDMPC_OPT_SETPOINT_CONVEX_LAW:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_SETPOINT_CONVEX_LAW must be 0 or 1");
      if (value == 1) {                                 // (CONVEX only, so never on together with options 18 / 19, which refuse it)
        const char* pre = "DDMPC_OPT_SETPOINT_CONVEX_LAW";
        if (instance_bounds(h) && !h->instance_setpoint_bounds)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: not on a handle with per-instance bounds (ddmpc_set_instance_input_bounds / "
                      "_output_bounds: the setpoint kernels read the bounds shared by the batch)", pre);
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one fixes its outputs to the setpoint as hard rows)", pre);
        if (!h->kp.convex)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the CONVEX slack box only (slack NONE: DDMPC_OPT_SETPOINT_LAW, or DDMPC_OPT_SETPOINT_BOX_LAW "
                      "with input / output bounds)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (h->prm.n * h->kp.nch > WARM_MAX_NF)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: n*(m+p) = %d, the affine law of ddmpc_prepare holds %d", pre, h->prm.n * h->kp.nch, WARM_MAX_NF);
        if (h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels: beyond them the phase "
                      "kernels have no M)", pre, h->kp.r);
        if (h->long_data)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: N = %d, the trajectory does not fit the LDS of the cold kernel (no refined columns there)", pre,
                      h->prm.N);
        // every slack component must change its diagonal entry at the bound (d_s > 0), the rule of DDMPC_OPT_CONVEX_WARM_LAW
        const int RP = 16 * h->kc.NT;
        std::vector<double> td;
        std::vector<int> ti;
        if (int rc = read_table(h->d_tabd, 4 * (size_t)RP, &td)) return rc;
        if (int rc = read_table(h->d_tabi, 3 * (size_t)RP, &ti)) return rc;
        for (int rho = 0; rho < h->kp.r; ++rho)
          if ((ti[rho] == K_WPRED || ti[rho] == K_WTERM) && !(td[rho] - td[RP + rho] > 0.0))
            return fail(DDMPC_ERR_UNSUPPORTED, "%s: a boxed output component has no weight (Q entry 0)", pre);
      }
      if (h->setpoint_convex_law != value) forget_prep(h);   // (S, and on a slack-only handle the box list and M, are part of what ddmpc_prepare keeps)
      h->setpoint_convex_law = value;
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_SETPOINTS:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_SETPOINTS must be 0 or 1");
      if (value == 1) {
        const char* pre = "DDMPC_OPT_LARGE_SETPOINTS";
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one fixes its outputs to the setpoint as hard rows)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (!h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the option serves 272 .. 1024 rows (up to 271 rows: DDMPC_OPT_SETPOINT_LAW, "
                      "DDMPC_OPT_SETPOINT_BOX_LAW, DDMPC_OPT_SETPOINT_CONVEX_LAW)", pre, h->kp.r);
        if (h->kp.r > 1024)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 1024 (the phase kernels)", pre, h->kp.r);
        if (h->large_pipeline != DDMPC_PIPELINE_PHASES)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only, and DDMPC_OPT_LARGE_PIPELINE selects the one-workgroup kernel", pre);
        if (h->stamps_on)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only, and ddmpc_debug_stamps selects the one-workgroup kernel", pre);
        if (h->batch > 65535)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only: batch %lld, the limit is 65535", pre, (long long)h->batch);
        if (h->prm.n * h->kp.nch > WARM_MAX_NF)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: n*(m+p) = %d, the limit is %d", pre, h->prm.n * h->kp.nch, WARM_MAX_NF);
        if (h->bounded)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s is not available on a handle with input or output bounds (beyond 271 rows the setpoint step "
                      "knows no bounds)", pre);
      }
      if (h->large_setpoints != value) forget_prep(h);   // (S is part of what ddmpc_prepare keeps, as DDMPC_OPT_SETPOINT_LAW)
      h->large_setpoints = value;
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_SETPOINT_BOUNDS:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_LARGE_SETPOINT_BOUNDS must be 0 or 1");
      if (value == 1) {                                 // (the refusals of DDMPC_OPT_LARGE_SETPOINTS but the one of bounds)
        const char* pre = "DDMPC_OPT_LARGE_SETPOINT_BOUNDS";
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one fixes its outputs to the setpoint as hard rows)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (!h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the option serves 272 .. 1024 rows (up to 271 rows: DDMPC_OPT_SETPOINT_BOX_LAW, "
                      "DDMPC_OPT_SETPOINT_CONVEX_LAW)", pre, h->kp.r);
        if (h->kp.r > 1024)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 1024 (the phase kernels)", pre, h->kp.r);
        if (h->large_pipeline != DDMPC_PIPELINE_PHASES)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only, and DDMPC_OPT_LARGE_PIPELINE selects the one-workgroup kernel", pre);
        if (h->stamps_on)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only, and ddmpc_debug_stamps selects the one-workgroup kernel", pre);
        if (h->batch > 65535)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: the phase kernels serve it only: batch %lld, the limit is 65535", pre, (long long)h->batch);
        if (h->prm.n * h->kp.nch > WARM_MAX_NF)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: n*(m+p) = %d, the limit is %d", pre, h->prm.n * h->kp.nch, WARM_MAX_NF);
      }
      h->large_setpoint_bounds = value;   // (which calls are accepted: the kept factor does not depend on the setpoint, nothing prepared differs)
      return DDMPC_OK;
    case DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS must be 0 or 1");
      if (value == 1) {
        const char* pre = "DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS";
        if (h->prm.controller_type != DDMPC_ROBUST)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: ROBUST controllers only (a NOMINAL one has neither bounds nor the setpoint law)", pre);
        if (h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)", pre);
        if (h->large)
          return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels; beyond them the "
                      "bounds stay shared by the batch)", pre, h->kp.r);
      } else if (instance_bounds(h) && (h->setpoint_box_law || h->setpoint_convex_law)) {
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 0: the handle carries per-instance bounds and %s = 1 together; remove "
                    "the per-instance bounds (ddmpc_set_instance_input_bounds / _output_bounds with null) or set %s = 0 first",
                    h->setpoint_box_law ? "DDMPC_OPT_SETPOINT_BOX_LAW" : "DDMPC_OPT_SETPOINT_CONVEX_LAW",
                    h->setpoint_box_law ? "DDMPC_OPT_SETPOINT_BOX_LAW" : "DDMPC_OPT_SETPOINT_CONVEX_LAW");
      }
      h->instance_setpoint_bounds = value;   // (which calls are accepted and which instantiation is launched: the law, S, the box list and M do not depend on it)
      return DDMPC_OK;
    case DDMPC_OPT_GRAM_LAUNCH:
      if (value != 0 && value != 1) return fail(DDMPC_ERR_INVALID, "Gram launch must be 0 (matrix pipe) or 1 (ddmpc_gram_tiles_kernel)");
      if (value == 1 && !h->gram_valu_ok) return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_gram_tiles_kernel stages the whole trajectory in LDS: not at this shape");
      if (value == 0 && !h->gram_stream_ok) return fail(DDMPC_ERR_UNSUPPORTED, "the streaming Gram launch does not hold this shape");
      h->gram_launch = value;
      h->gpre_valid = false;
      forget_prep(h);
      return DDMPC_OK;
    case DDMPC_OPT_LARGE_PIPELINE:
      if (value != DDMPC_PIPELINE_ONE_WORKGROUP && value != DDMPC_PIPELINE_PHASES)
        return fail(DDMPC_ERR_INVALID, "pipeline must be DDMPC_PIPELINE_ONE_WORKGROUP or DDMPC_PIPELINE_PHASES");
      if (value == DDMPC_PIPELINE_ONE_WORKGROUP && h->large_nominal && h->prm.weight_kind == DDMPC_WEIGHT_DENSE)
        return fail(DDMPC_ERR_UNSUPPORTED, "dense weighting matrices of a NOMINAL controller beyond 271 rows run on the phase kernels only");
      if (value == DDMPC_PIPELINE_ONE_WORKGROUP && h->large_setpoints)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_PIPELINE_ONE_WORKGROUP is not available with DDMPC_OPT_LARGE_SETPOINTS = 1: the phase kernels "
                    "serve the setpoint calls only");
      if (value == DDMPC_PIPELINE_ONE_WORKGROUP && h->large_setpoint_bounds)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_PIPELINE_ONE_WORKGROUP is not available with DDMPC_OPT_LARGE_SETPOINT_BOUNDS = 1: the phase "
                    "kernels serve the setpoint calls only");
      if (value == DDMPC_PIPELINE_ONE_WORKGROUP && h->large && h->bounded)
        return fail(DDMPC_ERR_UNSUPPORTED, "DDMPC_PIPELINE_ONE_WORKGROUP is not available on a handle with input or output bounds: beyond 271 rows "
                    "the phase kernels serve them only");
      h->large_pipeline = value;
      return DDMPC_OK;
    default: return fail(DDMPC_ERR_INVALID, "unknown option %d", option);
  }
}

// Bounds beyond 271 rows are served by the bounded instantiations of the phase kernels (ddmpc_rr3.hpp) only: why this handle
// cannot have them, or null.  `what`: "input bounds" / "output bounds".
static int large_bounds_refusal(const ddmpc_handle* h, const char* what) {
  if (h->large_setpoints)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: not with DDMPC_OPT_LARGE_SETPOINTS = 1 (beyond 271 rows the setpoint step knows no bounds)", what);
  if (!h->large_bounds)     // (opt-in: without the option a handle beyond 271 rows refuses bounds as it always did)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels) unless "
                "DDMPC_OPT_LARGE_BOUNDS = 1 (the phase kernels, 272 .. 1024 rows)", what, h->kp.r);
  if (h->kp.r > 1024)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 1024 (the phase kernels)", what, h->kp.r);
  if (h->large_pipeline != DDMPC_PIPELINE_PHASES)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: beyond 271 rows the phase kernels serve them only, and DDMPC_OPT_LARGE_PIPELINE selects the "
                "one-workgroup kernel", what);
  if (h->stamps_on)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: beyond 271 rows the phase kernels serve them only, and ddmpc_debug_stamps selects the "
                "one-workgroup kernel", what);
  if (h->batch > 65535)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: beyond 271 rows the phase kernels serve them only: batch %lld, the limit is 65535", what,
                (long long)h->batch);
  if (h->large_affine)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: not with DDMPC_OPT_LARGE_AFFINE_LAW = 1 (the law step knows no bounds)", what);
  return DDMPC_OK;
}

// With the terminal constraint the last n predicted inputs are fixed to u_s: outside the input bounds the QP is infeasible.
static const char* setpoint_outside_bounds(const ddmpc_handle* h, const double* u_s, const double* u_min, const double* u_max) {
  if (!h->prm.use_terminal_constraint) return nullptr;
  for (int ch = 0; ch < h->prm.m; ++ch)
    if (u_s[ch] < u_min[ch] || u_s[ch] > u_max[ch]) return "u_s lies outside [u_min, u_max] and the terminal constraint fixes the last n inputs to it";
  return nullptr;
}

static int apply_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max, bool any);
static int apply_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max, bool any);

// The channel table of ddmpc_box_law.hpp (BoxChannels) from the handle's bounds of both kinds: [batch][lo (m+p) | hi (m+p)], inputs
// first, a shared kind broadcast, -+infinity without a bound.  Released when neither kind is per instance.  Every bounds call ends
// here (behind its stream synchronisation: nothing in flight reads the table).
static int upload_instance_bounds(ddmpc_handle* h) {
  if (!instance_bounds(h)) { h->d_ibnd.release(); return DDMPC_OK; }
  const int m = h->prm.m, pp = h->prm.p, nch = m + pp;
  const size_t B = (size_t)h->batch;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> t(B * 2 * (size_t)nch);
  for (size_t b = 0; b < B; ++b) {
    double* lo = t.data() + b * 2 * (size_t)nch;
    double* hi = lo + nch;
    for (int c = 0; c < m; ++c) {
      lo[c] = !h->iumin_h.empty() ? h->iumin_h[b * m + c] : (h->umin_h.empty() ? -inf : h->umin_h[c]);
      hi[c] = !h->iumin_h.empty() ? h->iumax_h[b * m + c] : (h->umin_h.empty() ? inf : h->umax_h[c]);
    }
    for (int c = 0; c < pp; ++c) {
      lo[m + c] = !h->iymin_h.empty() ? h->iymin_h[b * pp + c] : (h->ymin_h.empty() ? -inf : h->ymin_h[c]);
      hi[m + c] = !h->iymin_h.empty() ? h->iymax_h[b * pp + c] : (h->ymin_h.empty() ? inf : h->ymax_h[c]);
    }
  }
  int rc = h->d_ibnd.ensure(t.size() * sizeof(double));
  if (!rc && hipMemcpy(h->d_ibnd.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(DDMPC_ERR_HIP, "per-instance bounds: the copy of the channel table failed");
  if (rc) {                             // (no table: no launch may ask for it -- the handle keeps the per-channel summary as shared bounds)
    h->iumin_h.clear(); h->iumax_h.clear(); h->iymin_h.clear(); h->iymax_h.clear();
    h->d_ibnd.release();
  }
  return rc;
}

// With the terminal constraint: the handle's setpoint of one kind (`nm`: "u" / "y", nc channels) against every row of the
// per-instance bounds of that kind.
static int instance_setpoint_outside(const ddmpc_handle* h, const double* sp, const double* lo, const double* hi, int nc, const char* nm) {
  if (!h->prm.use_terminal_constraint) return DDMPC_OK;
  for (int64_t b = 0; b < h->batch; ++b)
    for (int ch = 0; ch < nc; ++ch)
      if (sp[ch] < lo[b * nc + ch] || sp[ch] > hi[b * nc + ch])
        return fail(DDMPC_ERR_INVALID, "instance %lld, channel %d: %s_s lies outside [%s_min, %s_max] of that instance and the terminal constraint "
                    "fixes the last n %s to it", (long long)b, ch, nm, nm, nm, nm[0] == 'u' ? "inputs" : "outputs");
  return DDMPC_OK;
}

// The rows of a per-instance bounds call checked (nm: "u" / "y", nc channels), and their per-channel summary for the box list:
// the smallest finite lower and the largest finite upper bound of the batch, infinite where no instance has one.
static int check_instance_bounds(const ddmpc_handle* h, const double* lo, const double* hi, int nc, const char* nm,
                                 std::vector<double>* slo, std::vector<double>* shi, bool* any) {
  const double inf = std::numeric_limits<double>::infinity();
  slo->assign((size_t)nc, -inf);
  shi->assign((size_t)nc, inf);
  *any = false;
  for (int64_t b = 0; b < h->batch; ++b)
    for (int ch = 0; ch < nc; ++ch) {
      const double l = lo[b * nc + ch], u = hi[b * nc + ch];
      if (l != l) return fail(DDMPC_ERR_INVALID, "%s_min is NaN at instance %lld, channel %d", nm, (long long)b, ch);
      if (u != u) return fail(DDMPC_ERR_INVALID, "%s_max is NaN at instance %lld, channel %d", nm, (long long)b, ch);
      if (l >= u)
        return fail(DDMPC_ERR_INVALID, "%s_min >= %s_max at instance %lld, channel %d: the box is empty or a point", nm, nm, (long long)b, ch);
      if (std::isfinite(l)) { (*slo)[ch] = std::isfinite((*slo)[ch]) ? std::min((*slo)[ch], l) : l; *any = true; }
      if (std::isfinite(u)) { (*shi)[ch] = std::isfinite((*shi)[ch]) ? std::max((*shi)[ch], u) : u; *any = true; }
    }
  return DDMPC_OK;
}

// What per-instance bounds refuse beyond the refusals of the shared calls (`what`: "per-instance input bounds" / "... output bounds").
static int instance_bounds_refusal(const ddmpc_handle* h, const char* what) {
  if (h->large)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: (m+p)(L+n) = %d rows, the limit is 271 (the register-resident kernels; beyond them the "
                "phase kernels read the bounds shared by the batch, also with DDMPC_OPT_LARGE_BOUNDS = 1)", what, h->kp.r);
  if ((h->setpoint_box_law || h->setpoint_convex_law) && !h->instance_setpoint_bounds)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: not with %s = 1 (the setpoint kernels read the bounds shared by the batch)", what,
                h->setpoint_box_law ? "DDMPC_OPT_SETPOINT_BOX_LAW" : "DDMPC_OPT_SETPOINT_CONVEX_LAW");
  return DDMPC_OK;
}

int ddmpc_set_instance_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if ((u_min == nullptr) != (u_max == nullptr))
    return fail(DDMPC_ERR_INVALID, "%s is null: pass both u_min and u_max, or neither to remove the bounds", u_min ? "u_max" : "u_min");
  if (!u_min) return ddmpc_set_input_bounds(h, nullptr, nullptr);
  const int m = h->prm.m;
  std::vector<double> slo, shi;
  bool any = false;
  if (int rc = check_instance_bounds(h, u_min, u_max, m, "u", &slo, &shi, &any)) return rc;
  if (!any) return ddmpc_set_input_bounds(h, nullptr, nullptr);      // (no finite bound in the batch: a removal)
  if (int rc = instance_setpoint_outside(h, h->us_h.data(), u_min, u_max, m, "u")) return rc;
  if (int rc = instance_bounds_refusal(h, "per-instance input bounds")) return rc;
  if (int rc = apply_input_bounds(h, slo.data(), shi.data(), true)) return rc;
  h->iumin_h.assign(u_min, u_min + (size_t)h->batch * m);
  h->iumax_h.assign(u_max, u_max + (size_t)h->batch * m);
  return upload_instance_bounds(h);
}

int ddmpc_set_instance_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if ((y_min == nullptr) != (y_max == nullptr))
    return fail(DDMPC_ERR_INVALID, "%s is null: pass both y_min and y_max, or neither to remove the bounds", y_min ? "y_max" : "y_min");
  if (!y_min) return ddmpc_set_output_bounds(h, nullptr, nullptr);
  const int pp = h->prm.p;
  std::vector<double> slo, shi;
  bool any = false;
  if (int rc = check_instance_bounds(h, y_min, y_max, pp, "y", &slo, &shi, &any)) return rc;
  if (!any) return ddmpc_set_output_bounds(h, nullptr, nullptr);     // (no finite bound in the batch: a removal)
  if (int rc = instance_setpoint_outside(h, h->ys_h.data(), y_min, y_max, pp, "y")) return rc;
  if (int rc = instance_bounds_refusal(h, "per-instance output bounds")) return rc;
  if (int rc = apply_output_bounds(h, slo.data(), shi.data(), true)) return rc;
  h->iymin_h.assign(y_min, y_min + (size_t)h->batch * pp);
  h->iymax_h.assign(y_max, y_max + (size_t)h->batch * pp);
  return upload_instance_bounds(h);
}

int ddmpc_set_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if ((u_min == nullptr) != (u_max == nullptr))
    return fail(DDMPC_ERR_INVALID, "%s is null: pass both u_min and u_max, or neither to remove the bounds", u_min ? "u_max" : "u_min");
  const ddmpc_params& p = h->prm;
  bool any = false;
  if (u_min) {
    for (int ch = 0; ch < p.m; ++ch) {
      if (u_min[ch] != u_min[ch]) return fail(DDMPC_ERR_INVALID, "u_min[%d] is NaN", ch);
      if (u_max[ch] != u_max[ch]) return fail(DDMPC_ERR_INVALID, "u_max[%d] is NaN", ch);
      if (u_min[ch] >= u_max[ch]) return fail(DDMPC_ERR_INVALID, "u_min[%d] >= u_max[%d]: the box is empty or a point", ch, ch);
      any = any || std::isfinite(u_min[ch]) || std::isfinite(u_max[ch]);
    }
  }
  if (any)
    if (const char* msg = setpoint_outside_bounds(h, h->us_h.data(), u_min, u_max)) return fail(DDMPC_ERR_INVALID, "u_min / u_max: %s", msg);
  if (int rc = apply_input_bounds(h, u_min, u_max, any)) return rc;
  h->iumin_h.clear();                   // (the last call wins: the input bounds are shared now)
  h->iumax_h.clear();
  return upload_instance_bounds(h);
}

// ... what the call does once its values are accepted: the refusals that depend on which channels are bounded (`any`: some
// bound is finite), then the handle's state.  ddmpc_set_instance_input_bounds comes here with the per-channel summary of its rows.
static int apply_input_bounds(ddmpc_handle* h, const double* u_min, const double* u_max, bool any) {
  const ddmpc_params& p = h->prm;
  if (any) {
    if (h->setpoint_law && !h->setpoint_box_law)
      return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: not with DDMPC_OPT_SETPOINT_LAW = 1 (the setpoint step knows no bounds)");
    if (p.controller_type != DDMPC_ROBUST)
      return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: ROBUST controllers only (a NOMINAL one has no regularised reduced system to iterate on)");
    if (p.weight_kind == DDMPC_WEIGHT_DENSE)
      return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)");
    if (h->large) {           // (the kept factor plus one refinement pass is the normal solve there: every refinement mode)
      if (int rc = large_bounds_refusal(h, "input bounds")) return rc;
    } else {
      if (p.n * h->kp.nch > WARM_MAX_NF)
        return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: n*(m+p) = %d, the affine law of ddmpc_prepare holds %d", p.n * h->kp.nch, WARM_MAX_NF);
      if (h->kp.refine == DDMPC_REFINE_ALWAYS)
        return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: not with DDMPC_REFINE_ALWAYS (DDMPC_OPT_REFINE must be OFF or AUTO)");
    }
    const int nfree = p.use_terminal_constraint ? p.L - p.n : p.L;
    const bool diag = p.weight_kind == DDMPC_WEIGHT_DIAG;
    for (int ch = 0; ch < p.m; ++ch) {
      if (!std::isfinite(u_min[ch]) && !std::isfinite(u_max[ch])) continue;
      for (int kp = 0; kp < nfree; ++kp)
        if (!((diag ? h->Rh[(size_t)kp * p.m + ch] : h->Rh[0]) > 0.0))
          return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: channel %d is bounded and has an R entry of 0 on a free prediction step (limit: R > 0 there)", ch);
    }
    if (h->kp.convex)        // (the slack components join the box list: each must change its diagonal entry at the bound)
      for (int i = 0; i < (diag ? nfree * p.p : 1); ++i)
        if (!(h->Qh[(size_t)i] > 0.0))
          return fail(DDMPC_ERR_UNSUPPORTED, "input bounds: with the CONVEX slack box every Q entry of a free prediction step must be positive (limit: Q > 0 there)");
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->last.valid = false;
  forget_prep(h);
  h->bounded = any || !h->ymin_h.empty();
  const bool order = h->large && !h->large_nominal;          // (beyond 271 rows the bounded rows join the "boxed last" class)
  if (!any) { h->umin_h.clear(); h->umax_h.clear(); return order ? upload_large_box(h) : DDMPC_OK; }
  h->umin_h.assign(u_min, u_min + p.m);
  h->umax_h.assign(u_max, u_max + p.m);
  std::vector<double> ub(h->umin_h);
  ub.insert(ub.end(), h->umax_h.begin(), h->umax_h.end());
  int rc;
  if ((rc = h->d_ubnd.ensure(ub.size() * sizeof(double)))) { h->umin_h.clear(); h->umax_h.clear(); h->bounded = !h->ymin_h.empty(); return rc; }
  HIP_TRY(hipMemcpy(h->d_ubnd.p, ub.data(), ub.size() * sizeof(double), hipMemcpyHostToDevice));
  return order ? upload_large_box(h) : DDMPC_OK;
}

// With the terminal constraint the last n predicted outputs are fixed to y_s (the bounds act on the free steps, but a setpoint
// the free steps may not reach makes the QP infeasible under the CONVEX slack box, and pointless otherwise).
static const char* output_setpoint_outside_bounds(const ddmpc_handle* h, const double* y_s, const double* y_min, const double* y_max) {
  if (!h->prm.use_terminal_constraint) return nullptr;
  for (int ch = 0; ch < h->prm.p; ++ch)
    if (y_s[ch] < y_min[ch] || y_s[ch] > y_max[ch]) return "y_s lies outside [y_min, y_max] and the terminal constraint fixes the last n outputs to it";
  return nullptr;
}

int ddmpc_set_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if ((y_min == nullptr) != (y_max == nullptr))
    return fail(DDMPC_ERR_INVALID, "%s is null: pass both y_min and y_max, or neither to remove the bounds", y_min ? "y_max" : "y_min");
  const ddmpc_params& p = h->prm;
  bool any = false;
  if (y_min) {
    for (int ch = 0; ch < p.p; ++ch) {
      if (y_min[ch] != y_min[ch]) return fail(DDMPC_ERR_INVALID, "y_min[%d] is NaN", ch);
      if (y_max[ch] != y_max[ch]) return fail(DDMPC_ERR_INVALID, "y_max[%d] is NaN", ch);
      if (y_min[ch] >= y_max[ch]) return fail(DDMPC_ERR_INVALID, "y_min[%d] >= y_max[%d]: the box is empty or a point", ch, ch);
      any = any || std::isfinite(y_min[ch]) || std::isfinite(y_max[ch]);
    }
  }
  if (any)
    if (const char* msg = output_setpoint_outside_bounds(h, h->ys_h.data(), y_min, y_max)) return fail(DDMPC_ERR_INVALID, "y_min / y_max: %s", msg);
  if (int rc = apply_output_bounds(h, y_min, y_max, any)) return rc;
  h->iymin_h.clear();                   // (the last call wins: the output bounds are shared now)
  h->iymax_h.clear();
  return upload_instance_bounds(h);
}

// ... what the call does once its values are accepted (as apply_input_bounds).
static int apply_output_bounds(ddmpc_handle* h, const double* y_min, const double* y_max, bool any) {
  const ddmpc_params& p = h->prm;
  if (any) {
    if (h->setpoint_law && !h->setpoint_box_law)
      return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: not with DDMPC_OPT_SETPOINT_LAW = 1 (the setpoint step knows no bounds)");
    if (p.controller_type != DDMPC_ROBUST)
      return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: ROBUST controllers only (a NOMINAL one has no regularised reduced system to iterate on)");
    if (p.weight_kind == DDMPC_WEIGHT_DENSE)
      return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: DDMPC_WEIGHT_DENSE is not supported (scalar / diagonal weights only)");
    if (h->large) {
      if (int rc = large_bounds_refusal(h, "output bounds")) return rc;
    } else {
      if (p.n * h->kp.nch > WARM_MAX_NF)
        return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: n*(m+p) = %d, the affine law of ddmpc_prepare holds %d", p.n * h->kp.nch, WARM_MAX_NF);
      if (h->kp.refine == DDMPC_REFINE_ALWAYS)
        return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: not with DDMPC_REFINE_ALWAYS (DDMPC_OPT_REFINE must be OFF or AUTO)");
    }
    const int nfree = p.use_terminal_constraint ? p.L - p.n : p.L;
    const bool diag = p.weight_kind == DDMPC_WEIGHT_DIAG;
    int nout = 0;
    for (int ch = 0; ch < p.p; ++ch) {
      if (!std::isfinite(y_min[ch]) && !std::isfinite(y_max[ch])) continue;
      nout += nfree;
      for (int kp = 0; kp < nfree; ++kp)
        if (!((diag ? h->Qh[(size_t)kp * p.p + ch] : h->Qh[0]) > 0.0))
          return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: channel %d is bounded and has a Q entry of 0 on a free prediction step (limit: Q > 0 there)", ch);
    }
    if (h->kp.convex)        // (the slack components join the box list: each must change its diagonal entry at the bound)
      for (int i = 0; i < (diag ? nfree * p.p : 1); ++i)
        if (!(h->Qh[(size_t)i] > 0.0))
          return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: with the CONVEX slack box every Q entry of a free prediction step must be positive (limit: Q > 0 there)");
    // the box list: the slack components (CONVEX: every predicted step), the bounded inputs and the bounded outputs of the free steps
    int nin = 0;
    for (int ch = 0; ch < p.m && !h->umin_h.empty(); ++ch)
      if (std::isfinite(h->umin_h[ch]) || std::isfinite(h->umax_h[ch])) nin += nfree;
    const int nlist = (h->kp.convex ? p.L * p.p : 0) + nin + nout;
    if (!h->large && nlist > WARM_MAX_R)      // (beyond 271 rows nothing is indexed by component in LDS but the RR3_KMAX active ones)
      return fail(DDMPC_ERR_UNSUPPORTED, "output bounds: the box list has %d components (slack, input and output), the kernels hold %d", nlist,
                  WARM_MAX_R);
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->last.valid = false;
  forget_prep(h);
  h->bounded = any || !h->umin_h.empty();
  const bool order = h->large && !h->large_nominal;
  if (!any) { h->ymin_h.clear(); h->ymax_h.clear(); return order ? upload_large_box(h) : DDMPC_OK; }
  h->ymin_h.assign(y_min, y_min + p.p);
  h->ymax_h.assign(y_max, y_max + p.p);
  std::vector<double> yb(h->ymin_h);
  yb.insert(yb.end(), h->ymax_h.begin(), h->ymax_h.end());
  int rc;
  if ((rc = h->d_ybnd.ensure(yb.size() * sizeof(double)))) { h->ymin_h.clear(); h->ymax_h.clear(); h->bounded = !h->umin_h.empty(); return rc; }
  HIP_TRY(hipMemcpy(h->d_ybnd.p, yb.data(), yb.size() * sizeof(double), hipMemcpyHostToDevice));
  return order ? upload_large_box(h) : DDMPC_OK;
}

int ddmpc_set_setpoints(ddmpc_handle* h, const double* u_s, const double* y_s) {
  if (!h || !u_s || !y_s) return fail(DDMPC_ERR_INVALID, "null argument");
  if (!h->iumin_h.empty()) {            // (per-instance bounds: against every row)
    if (int rc = instance_setpoint_outside(h, u_s, h->iumin_h.data(), h->iumax_h.data(), h->prm.m, "u")) return rc;
  } else if (!h->umin_h.empty()) {
    if (const char* msg = setpoint_outside_bounds(h, u_s, h->umin_h.data(), h->umax_h.data())) return fail(DDMPC_ERR_INVALID, "%s", msg);
  }
  if (!h->iymin_h.empty()) {
    if (int rc = instance_setpoint_outside(h, y_s, h->iymin_h.data(), h->iymax_h.data(), h->prm.p, "y")) return rc;
  } else if (!h->ymin_h.empty()) {
    if (const char* msg = output_setpoint_outside_bounds(h, y_s, h->ymin_h.data(), h->ymax_h.data())) return fail(DDMPC_ERR_INVALID, "%s", msg);
  }
  HIP_TRY(hipSetDevice(h->device));
  h->us_h.assign(u_s, u_s + h->prm.m);
  h->ys_h.assign(y_s, y_s + h->prm.p);
  h->prm.u_s = h->us_h.data();
  h->prm.y_s = h->ys_h.data();
  h->last.valid = false;
  forget_prep(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return upload_params(h);
}

int ddmpc_get_solution(ddmpc_handle* h, int what, double* out, int mem) {
  if (!h || !out) return fail(DDMPC_ERR_INVALID, "null argument");
  LastSolve& l = h->last;
  if (!l.valid && l.setpoint_call)      // (ddmpc_reconstruct_kernel reads the shared setpoint table: it cannot rebuild that solve)
    return fail(DDMPC_ERR_NOT_READY, "no solution to read after ddmpc_step_setpoints / ddmpc_closed_loop_setpoints: the reconstruction knows "
                "the handle's shared setpoints only (a ddmpc_solve or ddmpc_step makes it readable again)");
  if (!l.valid) return fail(DDMPC_ERR_NOT_READY, "no solve to read a solution from");
  const KParams& k = h->kp;
  size_t per = 0;
  switch (what) {
    case DDMPC_SOL_ALPHA: per = k.c; break;
    case DDMPC_SOL_UBAR: per = (size_t)k.Ln * k.m; break;
    case DDMPC_SOL_YBAR: per = (size_t)k.Ln * k.p; break;
    case DDMPC_SOL_SIGMA:
      if (h->prm.controller_type != DDMPC_ROBUST) return fail(DDMPC_ERR_INVALID, "sigma exists only for a robust controller");
      per = (size_t)k.Ln * k.p;
      break;
    default: return fail(DDMPC_ERR_INVALID, "unknown solution selector %d", what);
  }
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)h->batch;
  const bool resolve_x = what == DDMPC_SOL_ALPHA && l.x == XState::ReSolveOnFactors;
  int rc;
  // make the record current: beta first, then (alpha only) x; a re-solve writes its outputs into the handle's own buffers
  if ((l.beta != BetaState::Written || resolve_x) &&
      ((rc = h->d_uopt.ensure(B * h->prm.L * k.m * sizeof(double))) || (rc = h->d_cost.ensure(B * sizeof(double))) ||
       (rc = h->d_status.ensure(B * sizeof(int32_t))) || (rc = h->d_iters.ensure(B * sizeof(int32_t)))))
    return rc;
  double *uo = (double*)h->d_uopt.p, *co = (double*)h->d_cost.p;
  int32_t *st = (int32_t*)h->d_status.p, *it = (int32_t*)h->d_iters.p;
  switch (l.beta) {
    case BetaState::Written: break;
    case BetaState::ReSolveCold:     // solve once more at the same past window, keeping beta / active set (and the rescue's output)
      if ((rc = launch_cold(h, l.up, l.yp, uo, co, st, it))) return rc;
      break;
    case BetaState::ReEvalLaw:       // evaluate the affine law once more, keeping beta / active set
      if ((rc = reserve_beta(h))) return rc;
      enqueue_warm_step(h, l.up, l.yp, uo, co, st, it, true, nullptr);
      HIP_TRY(hipGetLastError());
      break;
  }
  l.beta = BetaState::Written;
  const size_t bytes = per * B * sizeof(double);
  double* dst = out;
  if (mem == DDMPC_MEM_HOST) {
    if ((rc = h->d_out.ensure(bytes))) return rc;
    dst = (double*)h->d_out.p;
  }
  // instances solved by the NOMINAL rescue kernel have no beta: ubar / ybar come from the z it exported, alpha = H' x from
  // the vector x it exported
  if (resolve_x &&                   // solve once more on the route's factors at the same past window (on the phase route: x from w)
      (rc = launch_nominal_rescue(h, l.route, l.up, l.yp, uo, co, st, it, Stage::OnFactors)))
    return rc;
  const bool resc = l.rescue && h->d_resc.p && h->d_zws.p;
  if (h->large_nominal && !resc) return fail(DDMPC_ERR_NOT_READY, "no solve to read a solution from");
  if (what == DDMPC_SOL_ALPHA && l.x == XState::FromW) {    // x = L_I^-T w (alpha = H' x) from the final w the phase solve kept
    Rr2Solve S;
    if ((rc = rr2_solve_desc(h, (double*)h->d_rr.p, rr2_ndbl(h), &S))) return rc;
    hipLaunchKernelGGL(rr2_xws_kernel, dim3((unsigned)B), dim3(RR2_TS), 0, h->stream, S, k, (double*)h->d_xws.p);
    HIP_TRY(hipGetLastError());
    l.x = XState::Written;
  }
  const bool inst = instance_bounds(h);         // (per-instance bounds: both kinds are read from the channel table)
  const double* ibnd = (const double*)h->d_ibnd.p;
  hipLaunchKernelGGL(ddmpc_reconstruct_kernel, dim3((unsigned)h->batch), dim3(256), 0, h->stream, k, 16 * h->kc.NT, what, h->ud,
                     h->yd, l.up, l.yp, (const double*)h->d_beta.p, (const signed char*)h->d_act.p, dst,
                     resc ? (const double*)h->d_zws.p : (const double*)nullptr, resc ? (const int*)h->d_resc.p : (const int*)nullptr,
                     resc ? (const double*)h->d_xws.p : (const double*)nullptr,
                     !h->umin_h.empty() ? (inst ? ibnd : (const double*)h->d_ubnd.p) : (const double*)nullptr,
                     !h->ymin_h.empty() ? (inst ? ibnd + k.m : (const double*)h->d_ybnd.p) : (const double*)nullptr,
                     inst ? 2LL * k.nch : 0LL);
  HIP_TRY(hipGetLastError());
  if (mem == DDMPC_MEM_HOST) {
    HIP_TRY(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return DDMPC_OK;
}

int ddmpc_hankel(const double* X, int64_t batch, int32_t N, int32_t nch, int32_t L, double* H, int mem,
                 int device) {
  if (!X || !H) return fail(DDMPC_ERR_INVALID, "null argument");
  if (batch <= 0 || N <= 0 || nch <= 0 || L <= 0) return fail(DDMPC_ERR_INVALID, "sizes must be positive");
  if (N < L) return fail(DDMPC_ERR_INVALID, "N must be greater than or equal to L.");   // hankel_matrix.py:43-44
  if (ddmpc_device_count() <= 0) return fail(DDMPC_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
  HIP_TRY(hipSetDevice(device));
  const size_t nx = (size_t)batch * N * nch * sizeof(double);
  const size_t nh = (size_t)batch * L * nch * (N - L + 1) * sizeof(double);
  const long long total = (long long)(nh / sizeof(double));
  unsigned blocks = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
  if (mem == DDMPC_MEM_DEVICE) {
    hipLaunchKernelGGL(ddmpc_hankel_kernel, dim3(blocks), dim3(256), 0, 0, X, H, N, nch, L, (long long)batch);
    HIP_TRY(hipGetLastError());
    return DDMPC_OK;
  }
  double *dX = nullptr, *dH = nullptr;
  HIP_TRY(hipMalloc((void**)&dX, nx));
  if (hipMalloc((void**)&dH, nh) != hipSuccess) { (void)hipFree(dX); return fail(DDMPC_ERR_HIP, "hipMalloc(%zu) failed", nh); }
  hipError_t e = hipMemcpy(dX, X, nx, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ddmpc_hankel_kernel, dim3(blocks), dim3(256), 0, 0, dX, dH, N, nch, L, (long long)batch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(H, dH, nh, hipMemcpyDeviceToHost);
  (void)hipFree(dX);
  (void)hipFree(dH);
  if (e != hipSuccess) return fail(DDMPC_ERR_HIP, "ddmpc_hankel: %s", hipGetErrorString(e));
  return DDMPC_OK;
}

int ddmpc_pe_guard(const double* u_d, int64_t batch, int32_t N, int32_t m, int32_t order, double* ratio_lb,
                   int mem, int device) {
  if (!u_d || !ratio_lb) return fail(DDMPC_ERR_INVALID, "null argument");
  if (batch <= 0 || N <= 0 || m <= 0 || order <= 0) return fail(DDMPC_ERR_INVALID, "sizes must be positive");
  if (N < order) return fail(DDMPC_ERR_INVALID, "N must be greater than or equal to L.");   // hankel_matrix.py:43-44
  if (batch > 0x7fffffffLL) return fail(DDMPC_ERR_INVALID, "batch too large for one launch");
  if (mem != DDMPC_MEM_HOST && mem != DDMPC_MEM_DEVICE)
    return fail(DDMPC_ERR_INVALID, "mem must be DDMPC_MEM_HOST or DDMPC_MEM_DEVICE");
  if (ddmpc_device_count() <= 0) return fail(DDMPC_ERR_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
  const long long r = (long long)m * order;
  const size_t ndbl = (size_t)(r * (r + 1) / 2 + r + 64);
  size_t lds = ndbl * sizeof(double);
  HIP_TRY(hipSetDevice(device));
  double* scratch = nullptr;                                  // packed matrix too large for LDS: global workspace
  if (lds > 160 * 1024 - 64) {
    HIP_TRY(hipMalloc((void**)&scratch, (size_t)batch * ndbl * sizeof(double)));
    lds = 0;
  }
  if (lds > 64 * 1024)
    HIP_TRY(raise_lds_limit((const void*)ddmpc_pe_guard_kernel, lds));
  hipError_t e = hipSuccess;
  double *dX = nullptr, *dR = nullptr;
  const size_t nx = (size_t)batch * N * m * sizeof(double);
  if (mem == DDMPC_MEM_DEVICE) {
    hipLaunchKernelGGL(ddmpc_pe_guard_kernel, dim3((unsigned)batch), dim3(256), lds, 0, u_d, N, m, order, ratio_lb, scratch,
                       (long long)ndbl);
    e = hipGetLastError();
    if (e == hipSuccess && scratch) e = hipDeviceSynchronize();          // the workspace is released below
  } else {
    e = hipMalloc((void**)&dX, nx);
    if (e == hipSuccess) e = hipMalloc((void**)&dR, (size_t)batch * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(dX, u_d, nx, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(ddmpc_pe_guard_kernel, dim3((unsigned)batch), dim3(256), lds, 0, dX, N, m, order, dR, scratch,
                         (long long)ndbl);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(ratio_lb, dR, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost);
  }
  if (dX) (void)hipFree(dX);
  if (dR) (void)hipFree(dR);
  if (scratch) (void)hipFree(scratch);
  if (e != hipSuccess) return fail(DDMPC_ERR_HIP, "ddmpc_pe_guard: %s", hipGetErrorString(e));
  return DDMPC_OK;
}

// ---- ddmpc_closed_loop ----

// Arguments the three fused closed-loop kernels share, in their order (after the law, around each kernel's own tail); the
// per-step loop works on the same buffers.
struct LoopArgs {
  int ns; const double* pl; int n_steps, n_mpc_step;      // plant [A | B | C | D] and steps
  double *x, *up, *yp;                                     // state and past windows, moved on in place
  const double* w;
  double *usys, *ysys;
  int* stacc;                                              // status accumulator
  double* beta = nullptr; signed char* act = nullptr;      // beta / active set of the last solve (launch_fused_loop)
  double *lwup = nullptr, *lwyp = nullptr;                 // the past window of the last solve
  const double *uref = nullptr, *yref = nullptr;           // DDMPC_OPT_LARGE_SETPOINTS: the schedules [batch][n_steps][m], [batch][n_steps][p] (run_step_loop)
};
struct LoopBytes { size_t x, up, yp, w, us; };             // state, windows, w (= y_sys) and u_sys of the whole batch

// The one decision of what steps the plant.  It may call ddmpc_prepare: the prep_status of a NOMINAL handle and the refined
// laws under the slack box (prep.cwl_nref) are known after it only.  "fits": the fused loops keep the window and the inputs in
// use in LDS arrays of WARM_MAX_NF doubles, n_mpc_step * m <= WARM_MAX_NF and n (m + p) <= WARM_MAX_NF (ddmpc_plant_kernel sizes
// nothing by m, p, n or n_mpc_step).  First match:
//
//   DDMPC_PATH_COLD                                                     SolvePerStep   no ddmpc_prepare
//   beyond 271 rows                                                     StepPrepared   ddmpc_prepare
//   does not fit                                                        SolvePerStep   no ddmpc_prepare
//   input bounds (Route::BoxLaw)                                        FusedBox       ddmpc_prepare
//   slack box, DDMPC_OPT_CONVEX_WARM_LAW and no law refined             FusedConvex    ddmpc_prepare
//   slack box otherwise (affine iterate + filtered cold re-solve)       StepPrepared   ddmpc_prepare
//   NOMINAL, an instance with a singular Gram matrix (exact data)       SolvePerStep   ddmpc_prepare (its solves go through the
//                                                                                      rank-revealing rescue kernel: no law)
//   no inequality otherwise                                             FusedAffine    ddmpc_prepare
//
// DDMPC_PATH_WARM and DDMPC_PATH_AUTO choose alike.
static int select_loop_path(ddmpc_handle* h, int n_mpc_step, LoopPath* path) {
  const ddmpc_params& p = h->prm;
  *path = LoopPath::SolvePerStep;
  if (h->closed_loop_path == DDMPC_PATH_COLD) return DDMPC_OK;
  const bool fits = (size_t)n_mpc_step * p.m <= (size_t)WARM_MAX_NF && p.n * h->kp.nch <= WARM_MAX_NF;
  if (!h->large && !fits) return DDMPC_OK;
  if (int rc = ddmpc_prepare(h)) return rc;
  if (h->large) {
    *path = LoopPath::StepPrepared;
  } else if (select_route(h) == Route::BoxLaw) {
    *path = LoopPath::FusedBox;
  } else if (h->kp.convex) {
    *path = convex_warm_on(h) && h->prep.cwl_nref == 0 ? LoopPath::FusedConvex : LoopPath::StepPrepared;
  } else {
    if (p.controller_type == DDMPC_NOMINAL) {
      std::vector<int32_t> ps((size_t)h->batch);
      HIP_TRY(hipMemcpy(ps.data(), h->d_prep_status.p, ps.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int32_t st : ps)
        if (st != 0) return DDMPC_OK;
    }
    *path = LoopPath::FusedAffine;
  }
  return DDMPC_OK;
}

// The fused loop of `path`: the whole loop of an instance runs inside one workgroup, active-set iterations included.
static int launch_fused_loop(ddmpc_handle* h, LoopPath path, LoopArgs a) {
  if (int rc = reserve_beta(h)) return rc;
  a.beta = (double*)h->d_beta.p; a.act = (signed char*)h->d_act.p;
  const bool inst = path == LoopPath::FusedBox && instance_bounds(h);     // per-instance bounds: the channel table, as launch_box_step
  const bool warm = path == LoopPath::FusedBox && h->box_warm != 0 && !inst;   // DDMPC_OPT_BOX_WARM_START, as launch_box_step
  const int seeded = (warm && box_seed_valid(h)) ? 1 : 0;
  if (warm)
    if (int rc = h->d_box_seed.ensure((size_t)h->batch * (size_t)std::max(h->prep.cwl_nbox, 1))) return rc;
  begin_solve(h, path == LoopPath::FusedBox ? Route::BoxLaw : Route::Cold);
  const bool yb = path == LoopPath::FusedBox && !h->ymin_h.empty();
  const unsigned threads = yb ? (unsigned)h->prep.box_threads : warm_threads(h->kp.r);
  auto launch = [&](auto kernel, auto... tail) {       // (tail: what the kernel takes behind the beta / active-set workspace)
    hipLaunchKernelGGL(kernel, dim3((unsigned)h->batch), dim3(threads), 0, h->stream, h->kp, 16 * h->kc.NT,
                       h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const int*)h->d_prep_status.p, a.ns, a.pl, a.n_steps,
                       a.n_mpc_step, a.x, a.up, a.yp, a.w, a.usys, a.ysys, a.stacc, a.beta, a.act, tail...);
  };
  const int nbox = h->prep.cwl_nbox;
  const int* tab = (const int*)h->d_cwl_tab.p;
  const double* mcol = (const double*)h->d_mcol.p;
  double* sg = (double*)h->d_cwl_sg.p;
  if (path == LoopPath::FusedAffine) {
    launch(ddmpc_closed_loop_warm_kernel, a.lwup, a.lwyp);
  } else if (path == LoopPath::FusedConvex) {
    launch(ddmpc_closed_loop_convex_warm_kernel, nbox, tab, mcol, sg, a.lwup, a.lwyp);
  } else {    // (DDMPC_OPT_BOX_SAFEGUARD = 0 launches the instantiation without the safeguard, as launch_box_step)
    const double* bd = (const double*)h->d_box_bd.p;
    const int* ref = h->prep.cwl_nref > 0 ? (const int*)h->d_cwl_ref.p : (const int*)nullptr;
    auto launch_box = [&](auto... extra) {   // (the seed or the channel table follows the window of the last solve)
      with_safe_yb(h->box_safeguard != 0, yb, [&](auto safe, auto ybt) {
        launch(ddmpc_closed_loop_box_kernel<safe(), ybt(), decltype(extra)...>, nbox, tab, bd, mcol, sg, ref, a.lwup, a.lwyp, extra...);
      });
    };
    if (inst) launch_box(BoxChannels{(const double*)h->d_ibnd.p});
    else if (warm) launch_box(BoxSeed{(signed char*)h->d_box_seed.p, seeded});
    else launch_box();
    h->last.box_seed = warm;
  }
  HIP_TRY(hipGetLastError());
  return DDMPC_OK;
}

// The per-step paths are loops of two or three small launches per control step.  Optionally
// (DDMPC_OPT_CLOSED_LOOP_GRAPH) they are recorded into a HIP graph and replayed with a single launch; all
// buffers the loop touches are sized before the capture starts.  Off by default: measured on MI355X the
// asynchronous launches already keep the GPU busy (14.8 us per launch, 4096 x 401 one-step loop in 17.8 ms),
// while instantiating the ~1200-node graph costs more than it saves (25.2 ms) -- it only pays if a graph is
// replayed many times, which a closed loop with new data is not.
static int run_step_loop(ddmpc_handle* h, LoopPath path, const LoopArgs& a, const LoopBytes& nb) {
  const ddmpc_params& p = h->prm;
  const size_t B = (size_t)h->batch;
  const Route route = select_route(h);
  const int n_solves = (a.n_steps + a.n_mpc_step - 1) / a.n_mpc_step;
  bool use_graph = h->closed_loop_graph && n_solves >= 4 &&
                   !h->large && p.controller_type != DDMPC_NOMINAL && route != Route::BoxLaw;   // those paths size workspaces / set attributes per launch
  int rc;
  if ((rc = reserve_beta(h))) return rc;
  if (path == LoopPath::StepPrepared && !h->large && (rc = h->d_need.ensure(B * sizeof(int)))) return rc;   // (the slack box: launch_warm)
  // what launch_cold allocates or sets: sized before a capture starts
  if (route == Route::Cold && (rc = reserve_cold(h, true, true))) return rc;
  if (use_graph && hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();                          // e.g. a caller-provided legacy stream: launch the steps directly
    use_graph = false;
  }
  auto enqueue_steps = [&]() -> int {
    const unsigned pblocks = (unsigned)((B + 127) / 128);
    for (int t = 0; t < a.n_steps; t += a.n_mpc_step) {
      if (t + a.n_mpc_step >= a.n_steps) {            // the last solve: keep its window
        HIP_TRY(hipMemcpyAsync(a.lwup, a.up, nb.up, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(a.lwyp, a.yp, nb.yp, hipMemcpyDeviceToDevice, h->stream));
      }
      launch_fn solve = path == LoopPath::StepPrepared ? step_on_route : solve_on_route;
      if (a.uref) {       // the solve at step t reads row t of the schedules in place (the instance stride spans the schedule)
        h->sp_us = a.uref + (size_t)t * p.m; h->sp_ys = a.yref + (size_t)t * p.p;
        h->sp_su = (long long)a.n_steps * p.m; h->sp_sy = (long long)a.n_steps * p.p;
        solve = setpoint_step_on_route;
      }
      int rcs = solve(h, a.up, a.yp, (double*)h->d_uopt.p, (double*)h->d_cost.p, (int32_t*)h->d_status.p, nullptr);
      h->sp_us = h->sp_ys = nullptr;
      if (rcs) return rcs;
      const int nsub = (t + a.n_mpc_step <= a.n_steps) ? a.n_mpc_step : a.n_steps - t;
      hipLaunchKernelGGL(ddmpc_plant_kernel, dim3(pblocks), dim3(128), 0, h->stream, (long long)B, a.ns, p.m, p.p, p.n,
                         p.L * p.m, a.pl, t, nsub, a.n_steps, (const double*)h->d_uopt.p,
                         (const int*)h->d_status.p, a.stacc, a.x, a.up, a.yp, a.w, a.usys, a.ysys);
      HIP_TRY(hipGetLastError());
    }
    return DDMPC_OK;
  };
  rc = enqueue_steps();
  hipGraph_t graph = nullptr;
  if (rc) {
    if (use_graph) {                                  // leave the stream usable: close and drop the partial capture
      (void)hipStreamEndCapture(h->stream, &graph);
      if (graph) (void)hipGraphDestroy(graph);
    }
    return rc;
  }
  if (use_graph) {
    hipGraphExec_t exec = nullptr;
    HIP_TRY(hipStreamEndCapture(h->stream, &graph));
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e == hipSuccess) e = hipGraphLaunch(exec, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (exec) (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(DDMPC_ERR_HIP, "closed-loop graph: %s", hipGetErrorString(e));
  }
  return DDMPC_OK;
}

// mem == DDMPC_MEM_HOST: the loop runs on the handle's own buffers, the caller's inputs (user) copied in ...
static int stage_loop_inputs(ddmpc_handle* h, const LoopBytes& nb, const LoopArgs& user, LoopArgs* a) {
  int rc;
  if ((rc = h->d_x.ensure(nb.x)) || (rc = h->d_up.ensure(nb.up)) || (rc = h->d_yp.ensure(nb.yp)) ||
      (rc = h->d_w.ensure(nb.w)) || (rc = h->d_usys.ensure(nb.us)) || (rc = h->d_ysys.ensure(nb.w)))
    return rc;
  HIP_TRY(hipMemcpyAsync(h->d_x.p, user.x, nb.x, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_up.p, user.up, nb.up, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_yp.p, user.yp, nb.yp, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_w.p, user.w, nb.w, hipMemcpyHostToDevice, h->stream));
  a->x = (double*)h->d_x.p; a->up = (double*)h->d_up.p; a->yp = (double*)h->d_yp.p; a->w = (const double*)h->d_w.p;
  a->usys = (double*)h->d_usys.p; a->ysys = (double*)h->d_ysys.p;
  return DDMPC_OK;
}

// ... and its outputs copied out; the accumulated statuses go to the caller's memory either way.
static int copy_loop_outputs(ddmpc_handle* h, int mem, const LoopBytes& nb, const LoopArgs& a, const LoopArgs& user, int32_t* status) {
  const bool host = mem == DDMPC_MEM_HOST;
  if (host) {
    HIP_TRY(hipMemcpyAsync(user.x, a.x, nb.x, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(user.up, a.up, nb.up, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(user.yp, a.yp, nb.yp, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(user.usys, a.usys, nb.us, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(user.ysys, a.ysys, nb.w, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipMemcpyAsync(status, a.stacc, (size_t)h->batch * sizeof(int32_t), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
  if (host) HIP_TRY(hipStreamSynchronize(h->stream));
  return DDMPC_OK;
}

// DDMPC_OPT_SETPOINT_LAW: the fused loop with a setpoint schedule (a.ns .. a.stacc as for the other fused loops; u_ref / y_ref on
// the device).  The loop's last solve leaves nothing ddmpc_get_solution could reconstruct.
// DDMPC_OPT_SETPOINT_BOX_LAW on a handle with finite bounds (Route::BoxLaw): ddmpc_closed_loop_setpoint_box_kernel, from the empty set.
static int launch_setpoint_loop(ddmpc_handle* h, const LoopArgs& a, const double* u_ref, const double* y_ref) {
  const Route route = select_route(h);
  if (h->setpoint_convex_law || route == Route::BoxLaw) {
    // (DDMPC_OPT_SETPOINT_CONVEX_LAW: the SLACK instantiations, slack-only (Route::Cold) or bounded (Route::BoxLaw), as setpoint_step_on_route)
    begin_solve(h, route);
    const bool yb = !h->ymin_h.empty(), safe = route == Route::BoxLaw && h->box_safeguard;
    auto launch = [&](auto slack, auto... extra) {
      with_safe_yb(safe, yb, [&](auto safet, auto ybt) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ddmpc_closed_loop_setpoint_box_kernel<safet(), ybt(), slack(), decltype(extra)...>), dim3((unsigned)h->batch),
                           dim3(yb ? (unsigned)h->prep.box_threads : warm_threads(h->kp.r)), 0, h->stream, h->kp, 16 * h->kc.NT,
                           h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const double*)h->d_sgain.p,
                           (const int*)h->d_prep_status.p, a.ns, a.pl, a.n_steps, a.n_mpc_step, a.x, a.up, a.yp, a.w, u_ref, y_ref,
                           a.usys, a.ysys, a.stacc, h->prep.cwl_nbox, (const int*)h->d_cwl_tab.p, (const double*)h->d_box_bd.p,
                           (const double*)h->d_mcol.p, (double*)h->d_cwl_sg.p,
                           h->prep.cwl_nref > 0 ? (const int*)h->d_cwl_ref.p : (const int*)nullptr, (const double*)h->d_chbnd.p,
                           (int)(h->prm.use_terminal_constraint != 0), extra...);
      });
    };
    if (instance_bounds(h)) {      // (DDMPC_OPT_INSTANCE_SETPOINT_BOUNDS = 1: the BoxChannels instantiations, as setpoint_step_on_route)
      const BoxChannels chan{(const double*)h->d_ibnd.p};
      if (h->setpoint_convex_law) launch(std::true_type{}, chan); else launch(std::false_type{}, chan);
    } else {
      if (h->setpoint_convex_law) launch(std::true_type{}); else launch(std::false_type{});
    }
    HIP_TRY(hipGetLastError());
    h->last.setpoint_call = true;
    return DDMPC_OK;
  }
  begin_solve(h, Route::Cold);
  hipLaunchKernelGGL(ddmpc_closed_loop_setpoint_kernel, dim3((unsigned)h->batch), dim3(warm_threads(h->kp.r)), 0, h->stream, h->kp,
                     16 * h->kc.NT, h->prm.n * h->kp.nch, (const double*)h->d_gain.p, (const double*)h->d_sgain.p,
                     (const int*)h->d_prep_status.p, a.ns, a.pl, a.n_steps, a.n_mpc_step, a.x, a.up, a.yp, a.w, u_ref, y_ref, a.usys,
                     a.ysys, a.stacc);
  HIP_TRY(hipGetLastError());
  h->last.setpoint_call = true;
  return DDMPC_OK;
}

// ddmpc_closed_loop (u_ref = y_ref = null) and ddmpc_closed_loop_setpoints (`what` names the call in messages).
static int closed_loop_impl(ddmpc_handle* h, const char* what, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step,
                            double* x, double* u_past, double* y_past, const double* w, const double* u_ref, const double* y_ref,
                            double* u_sys, double* y_sys, int32_t* status, int mem);

int ddmpc_closed_loop(ddmpc_handle* h, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step, double* x,
                      double* u_past, double* y_past, const double* w, double* u_sys, double* y_sys,
                      int32_t* status, int mem) {
  return closed_loop_impl(h, "ddmpc_closed_loop", plant, n_steps, n_mpc_step, x, u_past, y_past, w, nullptr, nullptr, u_sys, y_sys,
                          status, mem);
}

int ddmpc_closed_loop_setpoints(ddmpc_handle* h, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step, double* x,
                                double* u_past, double* y_past, const double* w, const double* u_ref, const double* y_ref,
                                double* u_sys, double* y_sys, int32_t* status, int mem) {
  if (!h || !u_ref || !y_ref) return fail(DDMPC_ERR_INVALID, "null argument");
  if (!setpoint_on(h))
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_closed_loop_setpoints needs DDMPC_OPT_SETPOINT_LAW = 1 (or DDMPC_OPT_SETPOINT_BOX_LAW = 1, or DDMPC_OPT_SETPOINT_CONVEX_LAW = 1 under the CONVEX slack box), or beyond 271 rows DDMPC_OPT_LARGE_SETPOINTS = 1 (on a handle with input or output bounds there: DDMPC_OPT_LARGE_SETPOINT_BOUNDS = 1)");
  if (h->bounded && !h->setpoint_box_law && !h->setpoint_convex_law && !h->large_setpoint_bounds)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_closed_loop_setpoints on a handle with input or output bounds needs DDMPC_OPT_SETPOINT_BOX_LAW = 1");
  return closed_loop_impl(h, "ddmpc_closed_loop_setpoints", plant, n_steps, n_mpc_step, x, u_past, y_past, w, u_ref, y_ref, u_sys,
                          y_sys, status, mem);
}

static int closed_loop_impl(ddmpc_handle* h, const char* what, const ddmpc_plant* plant, int32_t n_steps, int32_t n_mpc_step,
                            double* x, double* u_past, double* y_past, const double* w, const double* u_ref, const double* y_ref,
                            double* u_sys, double* y_sys, int32_t* status, int mem) {
  if (!h || !plant || !x || !u_past || !y_past || !w || !u_sys || !y_sys || !status)
    return fail(DDMPC_ERR_INVALID, "null argument");
  if (!h->have_data) return fail(DDMPC_ERR_NOT_READY, "ddmpc_set_data must be called before %s", what);
  if (!prep_valid(h)) h->gpre_valid = false;    // (borrowed device data may have changed since the last solve; a kept law pins it)
  if (n_steps <= 0 || n_mpc_step <= 0) return fail(DDMPC_ERR_INVALID, "n_steps and n_mpc_step must be positive");
  const ddmpc_params& p = h->prm;
  if (n_mpc_step > p.L) return fail(DDMPC_ERR_INVALID, "n_mpc_step must not exceed the prediction horizon L");
  if (plant->ns <= 0 || plant->ns > 16 || !plant->A || !plant->B || !plant->C || !plant->D)
    return fail(DDMPC_ERR_INVALID, "plant: need 1 <= ns <= 16 and A, B, C, D");
  if (mem != DDMPC_MEM_HOST && mem != DDMPC_MEM_DEVICE)
    return fail(DDMPC_ERR_INVALID, "mem must be DDMPC_MEM_HOST or DDMPC_MEM_DEVICE");
  HIP_TRY(hipSetDevice(h->device));
  const int ns = plant->ns, m = p.m, pp = p.p, n = p.n;
  const size_t B = (size_t)h->batch;
  int rc;
  // plant matrices -> device
  std::vector<double> pl;
  pl.insert(pl.end(), plant->A, plant->A + ns * ns);
  pl.insert(pl.end(), plant->B, plant->B + ns * m);
  pl.insert(pl.end(), plant->C, plant->C + pp * ns);
  pl.insert(pl.end(), plant->D, plant->D + pp * m);
  if ((rc = h->d_pl.ensure(pl.size() * sizeof(double)))) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_pl.p, pl.data(), pl.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if ((rc = h->d_uopt.ensure(B * p.L * m * sizeof(double)))) return rc;
  if ((rc = h->d_cost.ensure(B * sizeof(double)))) return rc;
  if ((rc = h->d_status.ensure(B * sizeof(int32_t)))) return rc;
  if ((rc = h->d_stacc.ensure(B * sizeof(int32_t)))) return rc;
  HIP_TRY(hipMemsetAsync(h->d_stacc.p, 0, B * sizeof(int32_t), h->stream));
  const LoopBytes nb{B * ns * sizeof(double), B * n * m * sizeof(double), B * n * pp * sizeof(double),
                     B * (size_t)n_steps * pp * sizeof(double), B * (size_t)n_steps * m * sizeof(double)};
  const LoopArgs user{ns, (const double*)h->d_pl.p, n_steps, n_mpc_step, x, u_past, y_past, w, u_sys, y_sys, (int*)h->d_stacc.p};
  LoopArgs a = user;
  if (mem == DDMPC_MEM_HOST && (rc = stage_loop_inputs(h, nb, user, &a))) return rc;
  // the record of the loop is its last solve, at the window that solve saw (the `.value`s the reference holds after its loop):
  // the plant steps that follow it move u_past / y_past on, so that window is kept apart
  if ((rc = h->d_lwup.ensure(nb.up)) || (rc = h->d_lwyp.ensure(nb.yp))) return rc;
  a.lwup = (double*)h->d_lwup.p; a.lwyp = (double*)h->d_lwyp.p;
  // the fused loops of DDMPC_OPT_SETPOINT_LAW / _BOX_LAW / _CONVEX_LAW hold n_mpc_step * m inputs per solve in LDS (checked before
  // anything is staged); the per-step path of DDMPC_OPT_LARGE_SETPOINTS has no such limit
  if (u_ref && !h->large_setpoints && !h->large_setpoint_bounds && (size_t)n_mpc_step * m > (size_t)WARM_MAX_NF)
    return fail(DDMPC_ERR_UNSUPPORTED, "%s: n_mpc_step * m = %d, the fused loop holds %d inputs per solve", what, n_mpc_step * m, WARM_MAX_NF);
  if (u_ref) {                       // both setpoint loops: the schedules on the device, the preparation in place
    if (mem == DDMPC_MEM_HOST) {     // the schedules are [batch, n_steps, m] and [batch, n_steps, p]: the sizes of u_sys and y_sys
      if ((rc = h->d_uref.ensure(nb.us)) || (rc = h->d_yref.ensure(nb.w))) return rc;
      HIP_TRY(hipMemcpyAsync(h->d_uref.p, u_ref, nb.us, hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipMemcpyAsync(h->d_yref.p, y_ref, nb.w, hipMemcpyHostToDevice, h->stream));
      u_ref = (const double*)h->d_uref.p; y_ref = (const double*)h->d_yref.p;
    }
    if (!prep_valid(h) && (rc = ddmpc_prepare(h))) return rc;
  }
  if (u_ref && (h->large_setpoints || h->large_setpoint_bounds)) {
    // DDMPC_OPT_LARGE_SETPOINTS / _LARGE_SETPOINT_BOUNDS: the per-step path on what ddmpc_prepare kept (no fused kernel at this size, so no limit on
    // n_mpc_step * m; DDMPC_OPT_CLOSED_LOOP_PATH is not looked at: the cold solve knows the shared setpoints only)
    h->loop_kernel = kLoopKernel[(int)LoopPath::StepPrepared];
    a.uref = u_ref; a.yref = y_ref;
    rc = run_step_loop(h, LoopPath::StepPrepared, a, nb);
    h->last = LastSolve{};             // (as ddmpc_step_setpoints: nothing ddmpc_get_solution could reconstruct)
    h->last.setpoint_call = true;
    return rc ? rc : copy_loop_outputs(h, mem, nb, a, user, status);
  }
  if (u_ref) {
    // DDMPC_OPT_SETPOINT_LAW: one fused launch, no per-step fall-back (DDMPC_OPT_CLOSED_LOOP_PATH / _GRAPH are not looked at)
    // (the names are labels of the path: "..._setpoint_convex_kernel" is the SLACK instantiation of ddmpc_closed_loop_setpoint_box_kernel)
    // ("ddmpc_closed_loop_instance_setpoint_box_kernel" / "..._instance_setpoint_convex_kernel": its BoxChannels instantiations)
    const bool inst = instance_bounds(h);
    h->loop_kernel = h->setpoint_convex_law ? (inst ? "ddmpc_closed_loop_instance_setpoint_convex_kernel" : "ddmpc_closed_loop_setpoint_convex_kernel")
                     : select_route(h) == Route::BoxLaw ? (inst ? "ddmpc_closed_loop_instance_setpoint_box_kernel" : "ddmpc_closed_loop_setpoint_box_kernel")
                                                         : "ddmpc_closed_loop_setpoint_kernel";
    if ((rc = launch_setpoint_loop(h, a, u_ref, y_ref))) return rc;
    return copy_loop_outputs(h, mem, nb, a, user, status);
  }
  LoopPath path;
  if ((rc = select_loop_path(h, n_mpc_step, &path))) return rc;
  // ("ddmpc_closed_loop_instance_box_kernel" labels the channel-bounds (BoxChannels) instantiation of ddmpc_closed_loop_box_kernel)
  h->loop_kernel = (path == LoopPath::FusedBox && instance_bounds(h)) ? "ddmpc_closed_loop_instance_box_kernel" : kLoopKernel[(int)path];
  if ((rc = fused(path) ? launch_fused_loop(h, path, a) : run_step_loop(h, path, a, nb))) return rc;
  end_solve(h, a.lwup, a.lwyp);    // (the last solve's window: the per-step cold path re-solves there, the other paths wrote its beta)
  return copy_loop_outputs(h, mem, nb, a, user, status);
}

int ddmpc_cost_model(ddmpc_handle* h, double* flops_per_solve, double* bytes_per_solve) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  const KParams& k = h->kp;
  const double r = k.r, c = k.c;
  // Gram + Cholesky of the r x r reduced system + forward/back substitution
  // (DESIGN.md "Roofline accounting").  Dense Gram: symmetric H H', multiply-add = 2
  // flops, half the entries.  Structured Gram: nch^2*(L+n) base dot products of length c
  // plus the 4-flop sliding-window update of every entry of the lower triangle.
  const double gram = (k.gram_dense && !h->gram_pre) ? r * r * c : 2.0 * k.nch * k.nch * (double)k.Ln * c + 4.0 * r * r / 2.0;
  if (flops_per_solve) *flops_per_solve = gram + r * r * r / 3.0 + 2.0 * r * r;
  // compulsory HBM traffic: trajectories in, past window in, optimal_u + cost + status out
  if (bytes_per_solve)
    *bytes_per_solve = 8.0 * ((double)k.N * k.nch + (double)h->prm.n * k.nch + (double)h->prm.L * k.m + 1.0) + 4.0;
  return DDMPC_OK;
}

const char* ddmpc_kernel_name(ddmpc_handle* h) { return h ? h->kc.name2 : ""; }

const char* ddmpc_closed_loop_kernel_name(ddmpc_handle* h) { return h ? h->loop_kernel : ""; }

int ddmpc_debug_stamps(ddmpc_handle* h, int enable, uint64_t* out) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  if (enable && h->large_setpoints)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_debug_stamps is not available with DDMPC_OPT_LARGE_SETPOINTS = 1: stamps select the "
                "one-workgroup kernel, and the phase kernels serve the setpoint calls only");
  if (enable && h->large_setpoint_bounds)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_debug_stamps is not available with DDMPC_OPT_LARGE_SETPOINT_BOUNDS = 1: stamps select the "
                "one-workgroup kernel, and the phase kernels serve the setpoint calls only");
  if (enable && h->large && h->bounded)
    return fail(DDMPC_ERR_UNSUPPORTED, "ddmpc_debug_stamps is not available on a handle with input or output bounds beyond 271 rows: stamps "
                "select the one-workgroup kernel, and the phase kernels serve the bounds only");
  HIP_TRY(hipSetDevice(h->device));
  const size_t bytes = (size_t)h->batch * 16 * sizeof(uint64_t);
  if (out) {
    if (!h->stamps_on || !h->d_stamps.p) return fail(DDMPC_ERR_NOT_READY, "stamps were not enabled");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->d_stamps.p, bytes, hipMemcpyDeviceToHost));
  }
  if (enable) {
    int rc = h->d_stamps.ensure(bytes);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->d_stamps.p, 0, bytes, h->stream));
  }
  h->stamps_on = enable != 0;          // (beyond 271 rows this selects the route: select_route, prep_valid)
  return DDMPC_OK;
}

int ddmpc_debug_poison_allocations(int byte) {
  const int prev = g_poison_byte;
  g_poison_byte = byte & 0xff;
  return prev;
}

int ddmpc_debug_workspace(ddmpc_handle* h, int64_t b, double* ws_out, int64_t ws_count, int32_t* meta_out, int64_t meta_count,
                          int64_t* ws_avail, int64_t* meta_avail) {
  if (!h) return fail(DDMPC_ERR_INVALID, "null handle");
  // what the last solve left, read on the route that served it
  if (h->last.route == Route::RobustPhases && h->d_rr3k.p) {
    // ROBUST on the phase kernels (ddmpc_rr3.hpp): the per-instance record of the last solve --
    // [k, state, iterations, k, switched positions (capacity: RR3_KMAX, or DDMPC_OPT_LARGE_BOX_CAPACITY of the solve that wrote
    // it), active set (rv), start tick, ticks, peak k] -- into meta_out
    const long long kstride = rr3_kstride(h->last.box_cap, (h->kp.r + 1) & ~1);
    if (meta_avail) *meta_avail = kstride;
    if (ws_avail) *ws_avail = 0;
    if (b < 0 || b >= h->batch) return fail(DDMPC_ERR_INVALID, "instance out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (meta_out && meta_count > 0)
      HIP_TRY(hipMemcpy(meta_out, (const int*)h->d_rr3k.p + b * kstride, (size_t)(meta_count < kstride ? meta_count : kstride) * sizeof(int), hipMemcpyDeviceToHost));
    return DDMPC_OK;
  }
  if (!nominal_route(h->last.route) || !h->d_rr.p || !h->d_rrmeta.p) return fail(DDMPC_ERR_NOT_READY, "no global workspace to read");
  if (ws_count < 0 && h->d_rr2cand.p) {
    // diagnostics: the pivot candidates of G's factorisation (phase kernels), n16 doubles, relative to nothing (dmax is meta's business)
    const int n16 = (h->kp.r + 15) & ~15;
    if (ws_avail) *ws_avail = n16;
    if (b < 0 || b >= h->batch) return fail(DDMPC_ERR_INVALID, "instance out of range");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (ws_out) HIP_TRY(hipMemcpy(ws_out, (const double*)h->d_rr2cand.p + b * n16, (size_t)n16 * sizeof(double), hipMemcpyDeviceToHost));
    return DDMPC_OK;
  }
  if (b < 0 || b >= h->batch) return fail(DDMPC_ERR_INVALID, "instance out of range");
  HIP_TRY(hipSetDevice(h->device));
  const size_t rv = ((size_t)h->kp.r + 1) & ~(size_t)1;
  const size_t ndbl = (size_t)rr2_ndbl(h), nmeta = 2 * rv + 2;
  if (ws_avail) *ws_avail = (int64_t)ndbl;
  if (meta_avail) *meta_avail = (int64_t)nmeta;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ws_out && ws_count > 0)
    HIP_TRY(hipMemcpy(ws_out, (const double*)h->d_rr.p + (size_t)b * ndbl, sizeof(double) * (size_t)(ws_count < (int64_t)ndbl ? ws_count : (int64_t)ndbl),
                      hipMemcpyDeviceToHost));
  if (meta_out && meta_count > 0)
    HIP_TRY(hipMemcpy(meta_out, (const int*)h->d_rrmeta.p + (size_t)b * nmeta, sizeof(int) * (size_t)(meta_count < (int64_t)nmeta ? meta_count : (int64_t)nmeta),
                      hipMemcpyDeviceToHost));
  return DDMPC_OK;
}

int ddmpc_debug_large_box_order(int32_t m, int32_t p, int32_t n, int32_t L, int32_t use_terminal_constraint, int32_t convex,
                                const double* u_min, const double* u_max, const double* y_min, const double* y_max,
                                int32_t* perm_out, int32_t* n_a, int32_t* comp_out, int64_t comp_count, int32_t* nbox) {
  if (m <= 0 || p <= 0 || n <= 0 || L <= 0) return fail(DDMPC_ERR_INVALID, "sizes must be positive");
  if ((u_min == nullptr) != (u_max == nullptr) || (y_min == nullptr) != (y_max == nullptr))
    return fail(DDMPC_ERR_INVALID, "pass both arrays of a kind of bounds, or neither");
  // the kinds of a ROBUST controller's rows as upload_params sets them; weights of 1 (the order does not depend on them)
  KParams k{};
  k.m = m; k.p = p; k.nch = m + p; k.r = k.nch * (L + n); k.convex = convex != 0; k.lam = 1.0; k.sig_scale = -1.0; k.bound = 1.0;
  const int RP = (k.r + 15) & ~15;
  std::vector<int> ti(3 * (size_t)RP, -1);
  std::vector<double> td(4 * (size_t)RP, 0.0);
  for (int rho = 0; rho < k.r; ++rho) {
    const int kk = rho / k.nch, ch = rho % k.nch, kp = kk - n;
    const bool is_int = kp < 0, is_term = use_terminal_constraint != 0 && kp >= L - n;
    ti[rho] = ch < m ? ((is_int || is_term) ? K_UFIX : K_UFREE) : (is_int ? K_WINT : is_term ? K_WTERM : K_WPRED);
    td[rho] = 2.0; td[(size_t)RP + rho] = 1.0;
  }
  const LargeBox lb = build_large_box(k, RP, ti, td, u_min, u_max, y_min, y_max, use_terminal_constraint);
  if (perm_out) for (int i = 0; i < k.r; ++i) perm_out[i] = lb.pm[i];
  if (n_a) *n_a = lb.nA;
  if (nbox) *nbox = lb.nbox;
  for (int64_t s = 0; comp_out && s < comp_count && s < lb.nbox; ++s) { comp_out[s] = lb.ip[s]; comp_out[comp_count + s] = lb.ip[lb.nbox + s]; }
  return DDMPC_OK;
}

}  // extern "C"
