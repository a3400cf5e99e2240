// Host side of libaehmc_hip.so: the C-ABI of include/aehmc_hip.h over the gfx950 kernels
// in engine.cuh / gemm_f64.cuh / hmc_fused.cuh.  No torch types, no CPU fallback: every
// entry point launches HIP kernels or fails with an error code.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/aehmc_hip.h"
#include "tu.h"
#include "engine.cuh"
#include "gemm_f64.cuh"
#include "hmc_fused.cuh"
#include "hmc_linreg.cuh"
#include "nuts_linreg.cuh"
#include "nuts_block.cuh"
#include "nuts_block_reg.cuh"
#include "nuts_block_roll.cuh"
#include "nuts_resident.cuh"
#include "nuts_wide.cuh"
#include "nuts_pc_dense.cuh"
#include "pooled_adapt.cuh"
#include "chees.cuh"
#include "ghmc_fused.cuh"
#include "meads.cuh"
#include "pointwise.cuh"

using namespace aehmc;

#ifndef AEHMC_GPU_ARCH
#define AEHMC_GPU_ARCH "gfx950"  /* csrc/Makefile passes its ARCH */
#endif

namespace {
constexpr int NRING = 4;       // pinned "chains still active" slots
constexpr int STEP_BATCH = 8;  // lock-step leapfrogs between two polls
constexpr size_t PROF_POOL = 8192;
}  // namespace

// ---- run-time compiled programs (hipRTC; "user-defined targets" below).  One row per program: the target mode its
// source is compiled in, the family headers included after engine.cuh, and the kernels compiled together -- or none:
// one instantiation per program, named by the launch.  A new run-time compiled route registers here, and builds the
// name of its instantiation beside the plan in its family header (KernelLaunch, engine.cuh).
enum RtcProg { RTC_BASE, RTC_GLM, RTC_JBASE, RTC_JTWG, RTC_JWG, RTC_NUTS, RTC_JNUTS, RTC_WIDE, RTC_JWIDE, RTC_BLOCK, RTC_HMC,
               RTC_JHMCF, RTC_JHMC, RTC_GLMK, RTC_GHMC, RTC_JGHMC, RTC_PW };
struct RtcRow {
  const char *mode;                  // "AEHMC_CUSTOM_TARGET" (engine.cuh: target_elem calls aehmc_custom_elem), "AEHMC_JOINT_TARGET"
                                     // (leap_small_dense calls aehmc_logp through dual.cuh), or none: the GLM kernels
  std::vector<const char *> headers;
  std::vector<std::string> names;    // (a launch asks for one of them by the name written here: rtc_function fails otherwise)
  bool engine = true;                // engine.cuh ahead of the family headers (not for a pointwise program: no target in it)
};
static const RtcRow RTC_TABLE[] = {
    // RTC_BASE: the lock-step engine's target-dependent kernels (+ new_state): what LAUNCH_T can ask for
    {"AEHMC_CUSTOM_TARGET", {},
     {"aehmc::k_new_state_elem", "aehmc::k_step<true, true, true, false, true>", "aehmc::k_step<true, true, true, false, false>",
      "aehmc::k_step<false, true, true, true, false>", "aehmc::k_step_linear<12, false>", "aehmc::k_step_linear<15, true>"}},
    /* RTC_GLM */ {nullptr, {"glm_rows.cuh"}, {"aehmc::k_glm_rows", "aehmc::k_glm_finish"}},
    /* RTC_JBASE */ {"AEHMC_JOINT_TARGET", {},
     {"aehmc::k_new_state_joint", "aehmc::k_target_joint_rows", "aehmc::k_nuts_joint_rows", "aehmc::k_hmc_joint_rows"}},
    // RTC_JTWG: above JOINT_ROWS_MAX_D (a density with its reverse-mode program only): U and dU/dq a workgroup per chain --
    // new_state and the lock-step path's target evaluation; RTC_JBASE's kernels would need four chains' rows in LDS
    {"AEHMC_JOINT_TARGET", {}, {"aehmc::k_target_joint_wg<8>"}},
    // RTC_JWG: a workgroup of 8 wavefronts per chain (engine.cuh: k_nuts_joint_wg): traced densities with long data sweeps, few chains
    {"AEHMC_JOINT_TARGET", {}, {"aehmc::k_nuts_joint_wg<8>", "aehmc::k_hmc_joint_wg<8>"}},  // (this order: RTC_JWG_NUTS / _HMC below)
    /* RTC_NUTS */ {"AEHMC_CUSTOM_TARGET", {"nuts_resident.cuh"}, {}},
    /* RTC_JNUTS */ {"AEHMC_JOINT_TARGET", {"nuts_resident.cuh"}, {}},
    /* RTC_WIDE */ {"AEHMC_CUSTOM_TARGET", {"nuts_wide.cuh"}, {}},
    /* RTC_JWIDE */ {"AEHMC_JOINT_TARGET", {"nuts_wide.cuh", "hmc_fused.cuh"}, {}},
    /* RTC_BLOCK */ {"AEHMC_CUSTOM_TARGET", {"nuts_block_reg.cuh"}, {}},
    /* RTC_HMC */ {"AEHMC_CUSTOM_TARGET", {"hmc_fused.cuh"}, {}},
    /* RTC_JHMCF */ {"AEHMC_JOINT_TARGET", {"hmc_fused.cuh"}, {}},
    /* RTC_JHMC */ {"AEHMC_JOINT_TARGET", {}, {}},
    /* RTC_GLMK */ {nullptr, {"glm_rows.cuh"}, {}},  // (one instantiation of the one-launch GLM kernels)
    /* RTC_GHMC */ {"AEHMC_CUSTOM_TARGET", {"ghmc_fused.cuh"}, {}},
    /* RTC_JGHMC */ {"AEHMC_JOINT_TARGET", {"ghmc_fused.cuh"}, {}},
    // RTC_PW: a pointwise program (pointwise.cuh: k_pointwise<FOLD, STAGE>), compiled against the POINTWISE binding -- never
    // the target's; one instantiation per program
    {"AEHMC_POINTWISE_TARGET", {"pointwise.cuh"}, {}, false},
};
static_assert(sizeof(RTC_TABLE) / sizeof(RTC_TABLE[0]) == RTC_PW + 1, "one row per RtcProg, in its order");
static const std::string &RTC_JWG_NUTS = RTC_TABLE[RTC_JWG].names[0], &RTC_JWG_HMC = RTC_TABLE[RTC_JWG].names[1];  // (nuts_run / hmc_run spell no template arguments)
// a program and the wavefronts per SIMD its workgroup-per-chain kernels are compiled for (AEHMC_WG_MIN_WAVES 3 / 4:
// RTC_GLMK and RTC_JWG, see wg_program; 0: not defined)
struct RtcId {
  RtcProg prog;
  int waves;
  RtcId(RtcProg p, int w = 0) : prog(p), waves(w) {}
};
struct RtcProgram {
  hipModule_t mod = nullptr;
  std::map<std::string, hipFunction_t> fn;
};
// What a bound user-defined target owns: its source, the kernels compiled against it (hipRTC code objects keyed by
// program, waves and -- one instantiation per program -- kernel, kept while the source is bound), wg_program's picks
// among them, the device array of its parameter arrays, and what the source says about itself (read once, at bind)
struct CustomBinding {
  std::string src, inc;
  std::map<std::tuple<int, int, std::string>, RtcProgram> rtc;
  std::map<std::pair<int, std::string>, int> wg_choice;  // (wg_program: program, kernel -> the waves that were picked)
  const double **d_cparams = nullptr;
  int n_cparams = 0;
  bool has_grad = false, grad_small = false;  // "#define AEHMC_JOINT_GRAD" (a prefix of the next), "#define AEHMC_JOINT_GRAD_SMALL"
  bool has_sweep = false;  // "#define AEHMC_JOINT_SWEEP_TERMS n" (the tracer writes it, also with n = 0)
  long long sweep_terms = 0;
};
static void custom_release(CustomBinding &b) {
  for (auto &kv : b.rtc)
    if (kv.second.mod) (void)hipModuleUnload(kv.second.mod);
  b.rtc.clear();
  if (b.d_cparams) (void)hipFree(b.d_cparams);
  b.d_cparams = nullptr;
}

struct aehmc_ctx {
  int device = 0;
  std::string err;
  aehmc_target tgt{};
  bool has_tgt = false;
  aehmc_metric met{};
  bool has_met = false;
  double *log_sigma = nullptr;
  double *own_sqrt_mass = nullptr;  // computed by aehmc_set_metric when the caller passes none
  int64_t own_sqrt_mass_n = 0;
  const double *eps_c = nullptr;  // per-chain step sizes (aehmc_set_step_sizes)
  int64_t eps_n = 0;
  void *ws = nullptr;
  int64_t ws_bytes = 0;
  int *h_active = nullptr;  // pinned, device-visible
  int *d_active = nullptr;
  hipEvent_t ev[NRING] = {};
  bool opt_fused_hmc = true;
  int opt_resident_min_team = 0;  // tests: always use the smallest team that holds the chain
  int opt_resident_nuts = 2;      // register-resident single-launch NUTS: 0 off, 1 on, 2 auto
  bool opt_fused_nuts = false;   // whole NUTS transition in one launch (diag metric, coordinate-wise target)
  bool opt_dense_linear = true;  // one metric GEMM per leapfrog (v carried by linearity)
  bool opt_dense_whiten = true;  // dense MVN, shared dense metric, D > 512, lock-step: leapfrog in whitened coordinates
  bool opt_compact = true;       // finished chains drop out of the GEMMs
  int opt_block_roll = 0;        // block-resident NUTS: waiting chains that trigger a begin round (0: kernel default)
  int opt_joint_wg = 1;          // traced joint densities with long sweeps: a workgroup per chain (0 never, 1 when it pays, 2 always)
  int opt_wg_waves = 0;          // wavefronts per SIMD the workgroup-per-chain kernels are compiled for (0: four unless the program then spills, see wg_program; 3; 4)
  int opt_joint_wide = 1;      // traced joint densities, scalar / diagonal metric: the workgroup-per-chain kernels (0 never, 1 above 2048 coordinates, 2 also from 513 on)
  int opt_joint_resident = 1;  // joint densities with a reverse-mode program, D <= 512: the register-resident NUTS kernel (0 never, 1 from 17 coordinates on or with long reductions, 2 always)
  bool opt_pc_dense = true;      // per-chain dense metrics, 64 < D <= 512: NUTS in one launch, a wavefront per chain streams its matrix
  int opt_block_dense = 1;       // mid-size dense problems (64 < D <= 512): one workgroup per 16 chains, whole call in one launch
                                 // (1: chain state in registers up to D = 256, in L2-resident work rows above; 2: always work rows)
  bool opt_fp_contract = false;  // fast arithmetic in the leapfrog bodies of the register-resident kernels (1e-6, not bit parity)
  // profiling of the dominant (GEMM / fused) kernel with HIP events on the launch stream
  bool prof = false;
  std::vector<hipEvent_t> prof_ev;
  size_t prof_used = 0;
  double prof_ms = 0.0;
  int64_t prof_n = 0;
  unsigned long long *d_flops = nullptr;  // algorithmic flops of the profiled launches
  // stream-K GEMM: persistent grid, partial-accumulator hand-off buffers
  int opt_gemm_small = 1;  // mid-size products on small tiles: 1 auto, 0 off, 2 / 3 / 4: force 64x64 / 64x128 / 32x64
  int opt_streamk = 2;  // 0 off, 1 = 128x128 tiles (2 workgroups/CU), 2 = 128x256 tiles, software-pipelined (1 workgroup/CU)
  int sk_grid = 0, sk_grid_wide = 0;
  int64_t rows_hint = 0;  // > 0: upper bound on the live-row count of compacted GEMMs (from the last poll)
  double *sk_partial = nullptr;
  int *sk_flags = nullptr;
  int sk_epoch = 0;
  // pinned, device-visible error words: [0] a bounded stream-K spin expired, [1] a per-chain
  // matrix was not positive definite (separate words: one must not erase the other)
  int *h_err = nullptr, *d_err = nullptr;
  double prof_flops = 0.0;
  bool fuse_pre = false, pre_done = false;  // NUTS lock-step loop, dense-linear mode: see launch_leapfrog
  int *d_sched = nullptr;  // warm-up schedule on the device: stage [n], is_window_end [n]
  int64_t d_sched_n = 0;
  double *pc_work = nullptr;  // scratch of aehmc_metric_sqrt_per_chain above D = 64 (kept, grown on demand)
  size_t pc_work_bytes = 0;
  double *fd_ws = nullptr;  // small-dense kernels, per-chain metrics: the chains' transposed matrices (kept, grown)
  size_t fd_ws_bytes = 0;
  double *pool_work = nullptr;  // pooled window adaptation: partial column sums, batch mean, delta (kept, grown)
  size_t pool_work_bytes = 0;
  double *chees_work = nullptr;  // ChEES warm-up: partial column sums, the two means, the per-chain criterion (kept, grown)
  size_t chees_work_bytes = 0;
  double *chees_loop = nullptr;  // aehmc_chees_warmup: the positions before a transition [C,D], momentum . imm [C,D] (kept, grown)
  size_t chees_loop_bytes = 0;
  double *meads_work = nullptr;  // MEADS update: column sums, m, sd, row norms, Frobenius rows, the two [D,D] products (kept, grown)
  size_t meads_work_bytes = 0;
  double *ghmc_cell = nullptr;  // aehmc_ghmc_sample with host parameters: eps, alpha, delta [3]
  size_t ghmc_cell_bytes = 0;
  double *hmc_lens = nullptr;  // aehmc_hmc_sample_lengths: the call's trajectory lengths, int64 [num_samples] (kept, grown)
  size_t hmc_lens_bytes = 0;
  double *syrk_work = nullptr;  // symmetric rank-C update of a mid-size D: the parts of the chain range (kept, grown)
  size_t syrk_work_bytes = 0;
  double *blk_pack = nullptr;  // block-resident dense kernels: the launch's matrices zero-padded to [Dp][Dp] (kept, grown)
  size_t blk_pack_bytes = 0;
  CustomBinding bound;  // the user-defined target (aehmc_set_custom_target and its kin)
  // the pointwise program (aehmc_set_pointwise): a binding of its own -- summary.run samples with the target while it
  // folds --, what it said about itself, and the parts of a fold [parts][4][n_out] (kept, grown)
  CustomBinding pw;
  int64_t pw_D = 0, pw_n_out = 0;
  int pw_n_head = 0;
  double *pw_work = nullptr;
  size_t pw_work_bytes = 0;
  std::string rtc_cache_dir;  // compiled code objects of user-defined targets, kept across processes (aehmc_set_rtc_cache)
  int64_t rtc_compiled = 0, rtc_loaded = 0;  // programs compiled by hipRTC / taken from rtc_cache_dir (aehmc_rtc_stats)
  // user-defined row-reduction target: data matrix X [N,D], its transpose (owned), responses, [C,N] / [C] work arrays (owned)
  const double *glm_X = nullptr, *glm_y = nullptr;
  double *glm_XT = nullptr, *glm_z = nullptr, *glm_lsum = nullptr;
  int64_t glm_N = 0;
  size_t glm_z_bytes = 0, glm_lsum_bytes = 0;
  // whitened dense MVN (white_prepare): imm = L L^T, z = L^-1 (q - mu), r = L^T p; the problem is then a Gaussian of
  // precision H = L^T P L under the identity metric.  Formed from the bound arrays on first use, dropped on every
  // aehmc_set_target / aehmc_set_metric
  bool wh_ready = false;
  double *wh_L = nullptr, *wh_Linv = nullptr, *wh_H = nullptr;  // [D, D] row-major: L, L^-1 = sqrt_mass^T, H
  double *wh_zero = nullptr, *wh_one = nullptr;                 // mu of the whitened target [D] (zeros); the metric 1.0
  double *wh_mu = nullptr;                                      // the target's mu as it was when the operator was formed
  bool wh_tri = false;  // sqrt_mass is upper triangular to the bit (white_prepare): its products take the triangular hint
  // whitened carry ("dense_whiten_carry"): after white_end the workspace vectors z, hz, qn, gn (and Un) hold,
  // per chain, the returned (q, g, U) and the whitened pair (z, H z) it came from.  white_begin keeps the pair of every
  // chain whose incoming state is that record, bit for bit.  Dropped (carry_drop) by whatever may write those vectors
  // or change what they mean.
  bool opt_dense_whiten_carry = true;
  // whitened NUTS lock-step: the next half step is formed inside the bookkeeping pass (k_step_white_ahead)
  bool opt_dense_whiten_ahead = true;
  struct {
    bool valid = false;
    int64_t C = 0, D = 0;
    const double *z = nullptr, *hz = nullptr, *qn = nullptr, *gn = nullptr;
    // aehmc_set_target / aehmc_set_metric with a valid record: the operator it was made with is kept aside (`old_*`)
    // instead of freed, and the record is `pending`.  When the next whitened call has formed the new binding's operator,
    // the record counts again if L, L^-1, H and mu are the old ones bit for bit -- results follow the CONTENT of the
    // bound arrays, not which arrays hold it (a caller who passes a fresh copy of the same matrix every call gets what
    // one binding gives) -- and is dropped otherwise.
    bool pending = false;
    double *old_L = nullptr, *old_Linv = nullptr, *old_H = nullptr, *old_mu = nullptr;
    bool eig = false;  // the record's z is the eigen route's y
  } carry;
  // eigen route of the whitened mode ("dense_eigen"): H = V diag(lam) V^T, formed by white_basis on the first
  // NUTS call that wants it.  Vt = V^T, Tin = V^T L^-1, Tout = L V, Tp = L^-T V, all [D, D] row-major: the B operand of
  // A B^T in s = V^T r, y = Tin (q - mu), q - mu = Tout y, p = Tp s
  int opt_dense_eigen = 1;         // 0 off, 1 where the whitened mode applies and D >= EIGEN_MIN_D, 2 wherever it applies
  int opt_dense_eigen_wide = 1;    // the route's NUTS loop: 1 one k_nuts_wide launch where 512 < D <= 10176, 0 the lock-step stage
  bool opt_eigen_solver = true;    // false (tests): the solver's symbols are not found
  struct {
    bool tried = false, ready = false;  // tried: white_basis has decided for this operator (state says what)
    int state = 0;                      // aehmc_white_basis_info
    double orth = -1.0, resid = -1.0, solver_ms = 0.0;
    double *Vt = nullptr, *lam = nullptr, *Tin = nullptr, *Tout = nullptr, *Tp = nullptr;
    double *sup_V = nullptr, *sup_lam = nullptr;  // aehmc_set_white_basis: the caller's V and lam (copies)
    int64_t sup_D = 0, D = 0;  // (D: the size of the basis in use)
    // aehmc_set_target / aehmc_set_metric with a basis in use: it is kept aside with a copy of its H, and the next
    // white_basis takes it back if the new binding's H has those bits (the solver is not paid again by a caller who
    // binds fresh copies of the same matrices)
    double *keep_H = nullptr, *keep_Vt = nullptr, *keep_lam = nullptr;
    int64_t keep_D = 0;
  } eig;
};

#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);                      \
      return -1;                                                                         \
    }                                                                                    \
  } while (0)
#define FAIL(msg)        \
  do {                   \
    ctx->err = (msg);    \
    return -2;           \
  } while (0)

// a buffer kept with the ctx and grown on demand (hipFree waits for earlier launches that use it)
static int grow(aehmc_ctx *ctx, double **buf, size_t *have, size_t need) {
  if (*have >= need) return 0;
  if (*buf) HIPCHK(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  HIPCHK(hipMalloc((void **)buf, need));
  *have = need;
  return 0;
}
static inline dim3 chain_grid(int64_t C) { return dim3((unsigned)((C + 3) / 4)); }
static void carry_free_old(aehmc_ctx *ctx) {
  for (double **p : {&ctx->carry.old_L, &ctx->carry.old_Linv, &ctx->carry.old_H, &ctx->carry.old_mu}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}
static inline void carry_drop(aehmc_ctx *ctx) {
  ctx->carry.valid = ctx->carry.pending = false;
  if (ctx->carry.old_L) carry_free_old(ctx);
}
// drops the whitened operator (hipFree waits for the launches that still read it)
// `rebind` (aehmc_set_target, aehmc_set_metric on a dense-MVN binding): a valid carry record becomes pending, see
// aehmc_ctx::carry
static void eigen_free_keep(aehmc_ctx *ctx) {
  for (double **p : {&ctx->eig.keep_H, &ctx->eig.keep_Vt, &ctx->eig.keep_lam}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  ctx->eig.keep_D = 0;
}
// drops the basis of the bound operator; `keep`: V^T and lam are kept aside with a copy of H (aehmc_ctx::eig)
static void eigen_release(aehmc_ctx *ctx, bool keep) {
  auto &e = ctx->eig;
  if (keep && e.ready && ctx->wh_H) {
    eigen_free_keep(ctx);
    const int64_t D = e.D;
    if (hipMalloc((void **)&e.keep_H, (size_t)D * D * sizeof(double)) == hipSuccess &&
        hipMemcpy(e.keep_H, ctx->wh_H, (size_t)D * D * sizeof(double), hipMemcpyDeviceToDevice) == hipSuccess) {
      e.keep_Vt = e.Vt; e.keep_lam = e.lam; e.keep_D = D;
      e.Vt = e.lam = nullptr;
    } else {
      (void)hipGetLastError();
      eigen_free_keep(ctx);
    }
  }
  for (double **p : {&e.Vt, &e.lam, &e.Tin, &e.Tout, &e.Tp}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  e.tried = e.ready = false;
}
static void white_release(aehmc_ctx *ctx, bool rebind = false) {
  eigen_release(ctx, rebind);  // (a basis kept aside by an earlier re-binding waits for the next white_basis)
  if (!rebind) eigen_free_keep(ctx);
  const bool set_aside = rebind && ctx->carry.valid && ctx->wh_ready && ctx->wh_mu;
  const bool keep = set_aside || (rebind && ctx->carry.pending && !ctx->wh_ready);
  if (set_aside) {
    carry_free_old(ctx);
    ctx->carry.old_L = ctx->wh_L; ctx->carry.old_Linv = ctx->wh_Linv; ctx->carry.old_H = ctx->wh_H;
    ctx->carry.old_mu = ctx->wh_mu;
    ctx->wh_L = ctx->wh_Linv = ctx->wh_H = ctx->wh_mu = nullptr;
  }
  for (double **p : {&ctx->wh_L, &ctx->wh_Linv, &ctx->wh_H, &ctx->wh_zero, &ctx->wh_one, &ctx->wh_mu}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  ctx->wh_ready = ctx->wh_tri = false;
  if (keep) {
    ctx->carry.valid = false;
    ctx->carry.pending = true;
  } else {
    carry_drop(ctx);
  }
}
constexpr int LINREG_SMAX = 32;
// row slices per chain group: enough workgroups (~2048) to fill the GPU
static inline int linreg_slices(int64_t C) {
  const int64_t groups = (C + LINREG_CPB - 1) / LINREG_CPB;
  int64_t s = (2048 + groups - 1) / groups;
  return (int)(s < 1 ? 1 : (s > LINREG_SMAX ? LINREG_SMAX : s));
}
static int launch_linreg(aehmc_ctx *ctx, const EngineArgs &a, const double *q, double *g, double *U, int to_ctl,
                         hipStream_t st) {
  const int S = linreg_slices(a.C);
  const unsigned groups = (unsigned)((a.C + LINREG_CPB - 1) / LINREG_CPB);
  hipLaunchKernelGGL(k_target_linreg, dim3(groups * S), dim3(256), 0, st, a, q, a.linreg_part, S, to_ctl);
  hipLaunchKernelGGL(k_linreg_finish, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, st, a, q, g, U,
                     (const double *)a.linreg_part, S, to_ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ ctx ------------
extern "C" int aehmc_create(aehmc_ctx **out, int device) {
  if (!out) return -2;
  aehmc_ctx *ctx = new aehmc_ctx();
  ctx->device = device;
  *out = ctx;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipHostMalloc((void **)&ctx->h_active, NRING * sizeof(int), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer((void **)&ctx->d_active, ctx->h_active, 0));
  for (int i = 0; i < NRING; i++) HIPCHK(hipEventCreateWithFlags(&ctx->ev[i], hipEventDisableTiming));
  {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    int per_cu = 0;
    HIPCHK(tu::gemm_streamk_occupancy(&per_cu));
    if (per_cu > 2) per_cu = 2;
    ctx->sk_grid = (prop.multiProcessorCount * per_cu / 8) * 8;  // all workgroups co-resident
    ctx->sk_grid_wide = (prop.multiProcessorCount / 8) * 8;       // 128 x 256 tiles: one workgroup per CU
    if (ctx->sk_grid > 0) {
      HIPCHK(hipMalloc((void **)&ctx->sk_partial, (size_t)ctx->sk_grid * 64 * 256 * sizeof(double)));
      HIPCHK(hipMalloc((void **)&ctx->sk_flags, ctx->sk_grid * sizeof(int)));
      HIPCHK(hipMemset(ctx->sk_flags, 0, ctx->sk_grid * sizeof(int)));
    }
    HIPCHK(hipHostMalloc((void **)&ctx->h_err, 2 * sizeof(int), hipHostMallocMapped));
    ctx->h_err[0] = ctx->h_err[1] = 0;
    HIPCHK(hipHostGetDevicePointer((void **)&ctx->d_err, ctx->h_err, 0));
  }
  HIPCHK(hipMalloc((void **)&ctx->d_flops, sizeof(unsigned long long)));
  HIPCHK(hipMemset(ctx->d_flops, 0, sizeof(unsigned long long)));
  return 0;
}

extern "C" int aehmc_destroy(aehmc_ctx *ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  if (ctx->log_sigma) (void)hipFree(ctx->log_sigma);
  if (ctx->own_sqrt_mass) (void)hipFree(ctx->own_sqrt_mass);
  if (ctx->h_active) (void)hipHostFree(ctx->h_active);
  if (ctx->d_flops) (void)hipFree(ctx->d_flops);
  if (ctx->sk_partial) (void)hipFree(ctx->sk_partial);
  if (ctx->sk_flags) (void)hipFree(ctx->sk_flags);
  if (ctx->h_err) (void)hipHostFree(ctx->h_err);
  if (ctx->d_sched) (void)hipFree(ctx->d_sched);
  if (ctx->pc_work) (void)hipFree(ctx->pc_work);
  if (ctx->fd_ws) (void)hipFree(ctx->fd_ws);
  if (ctx->blk_pack) (void)hipFree(ctx->blk_pack);
  if (ctx->pool_work) (void)hipFree(ctx->pool_work);
  if (ctx->chees_work) (void)hipFree(ctx->chees_work);
  if (ctx->chees_loop) (void)hipFree(ctx->chees_loop);
  if (ctx->meads_work) (void)hipFree(ctx->meads_work);
  if (ctx->ghmc_cell) (void)hipFree(ctx->ghmc_cell);
  if (ctx->hmc_lens) (void)hipFree(ctx->hmc_lens);
  if (ctx->syrk_work) (void)hipFree(ctx->syrk_work);
  if (ctx->glm_XT) (void)hipFree(ctx->glm_XT);
  if (ctx->glm_z) (void)hipFree(ctx->glm_z);
  if (ctx->glm_lsum) (void)hipFree(ctx->glm_lsum);
  white_release(ctx);
  if (ctx->eig.sup_V) (void)hipFree(ctx->eig.sup_V);
  if (ctx->eig.sup_lam) (void)hipFree(ctx->eig.sup_lam);
  custom_release(ctx->bound);
  custom_release(ctx->pw);
  if (ctx->pw_work) (void)hipFree(ctx->pw_work);
  for (int i = 0; i < NRING; i++)
    if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
  for (auto e : ctx->prof_ev) (void)hipEventDestroy(e);
  delete ctx;
  return 0;
}

extern "C" const char *aehmc_last_error(const aehmc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

extern "C" int aehmc_set_target(aehmc_ctx *ctx, const aehmc_target *t) {
  if (!ctx || !t) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (t->D <= 0) FAIL("target: D must be positive");
  switch (t->kind) {
    case AEHMC_T_STD_NORMAL:
    case AEHMC_T_ISO_GAUSSIAN:
      break;
    case AEHMC_T_DIAG_GAUSSIAN:
      if (!t->mu || !t->sigma) FAIL("diag gaussian target needs mu and sigma");
      break;
    case AEHMC_T_DENSE_MVN:
      if (!t->mu || !t->prec) FAIL("dense MVN target needs mu and prec");
      break;
    case AEHMC_T_LINREG:
      if (!t->X || !t->y || t->N <= 0 || t->D != 2) FAIL("linreg target needs X, y, N and D == 2");
      if ((((uintptr_t)t->X) | ((uintptr_t)t->y)) & 15) FAIL("linreg target: X and y must be 16-byte aligned");
      break;
    default:
      FAIL("unknown target kind");
  }
  white_release(ctx, t->kind == AEHMC_T_DENSE_MVN);
  ctx->tgt = *t;
  ctx->has_tgt = true;
  if (ctx->log_sigma) {
    HIPCHK(hipFree(ctx->log_sigma));
    ctx->log_sigma = nullptr;
  }
  if (t->kind == AEHMC_T_DIAG_GAUSSIAN) {
    HIPCHK(hipMalloc((void **)&ctx->log_sigma, t->D * sizeof(double)));
    hipLaunchKernelGGL(k_log, dim3((unsigned)((t->D + 255) / 256)), dim3(256), 0, 0, t->sigma,
                       ctx->log_sigma, (long long)t->D);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
  }
  return 0;
}

// ------------------------------------------------------------------ user-defined targets (hipRTC)
// The kernels that evaluate the target are templates / inline functions of engine.cuh and the family headers; for a
// user-defined target they are compiled at run time against the user's aehmc_custom_elem (engine.cuh: target_elem's
// AEHMC_T_CUSTOM case) or joint density.  One hipRTC program per RTC_TABLE row (and instantiation), compiled on first use.
static const char *RTC_PROLOGUE =
    "typedef signed int int32_t; typedef unsigned int uint32_t; typedef long long int64_t;\n"
    "typedef unsigned long long uint64_t; typedef unsigned long long uintptr_t; typedef unsigned long size_t;\n"
    "#define INFINITY __builtin_huge_val()\n";
// ---- code objects of run-time compiled programs on disk (aehmc_set_rtc_cache): a second process that binds the same
// user-defined target starts without recompiling.  File = the code object + the lowered names of its kernels; its name
// is a hash of everything the compiler saw (source, options, kernel names); the DIRECTORY is chosen by the caller and
// carries the hash of the library's own sources (the headers the program includes), see aehmc_amd/engine.py.
static uint64_t fnv1a64(const std::string &s, uint64_t h = 1469598103934665603ULL) {
  for (unsigned char ch : s) {
    h ^= ch;
    h *= 1099511628211ULL;
  }
  return h;
}
static bool rtc_cache_load(const std::string &path, const std::vector<std::string> &names, std::vector<char> &code,
                           std::vector<std::string> &lowered) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  bool ok = false;
  uint64_t head[3];
  if (fread(head, sizeof(uint64_t), 3, f) == 3 && head[0] == 0x61656863724b4f31ULL && head[1] == names.size()) {
    lowered.clear();
    ok = true;
    for (size_t k = 0; ok && k < names.size(); k++) {
      uint64_t n = 0;
      ok = fread(&n, sizeof(n), 1, f) == 1 && n < 4096;
      std::string low(ok ? n : 0, '\0');
      ok = ok && (n == 0 || fread(&low[0], 1, n, f) == n);
      lowered.push_back(low);
    }
    code.resize(ok ? head[2] : 0);
    ok = ok && head[2] > 0 && fread(code.data(), 1, head[2], f) == head[2];
  }
  fclose(f);
  return ok;
}
static void rtc_cache_store(const std::string &path, const std::vector<std::string> &lowered, const std::vector<char> &code) {
  const std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return;  // (an unwritable cache is not an error)
  const uint64_t head[3] = {0x61656863724b4f31ULL, lowered.size(), code.size()};
  bool ok = fwrite(head, sizeof(uint64_t), 3, f) == 3;
  for (const auto &low : lowered) {
    const uint64_t n = low.size();
    ok = ok && fwrite(&n, sizeof(n), 1, f) == 1 && (n == 0 || fwrite(low.data(), 1, n, f) == n);
  }
  ok = ok && fwrite(code.data(), 1, code.size(), f) == code.size();
  ok = (fclose(f) == 0) && ok;
  if (ok) ok = rename(tmp.c_str(), path.c_str()) == 0;  // (atomic: a concurrent reader sees the old file or the new one)
  if (!ok) remove(tmp.c_str());
}
extern "C" int aehmc_set_rtc_cache(aehmc_ctx *ctx, const char *dir) {
  if (!ctx) return -2;
  ctx->rtc_cache_dir = dir ? dir : "";
  return 0;
}
extern "C" int aehmc_rtc_stats(const aehmc_ctx *ctx, int64_t *compiled, int64_t *loaded_from_cache) {
  if (!ctx) return -2;
  if (compiled) *compiled = ctx->rtc_compiled;
  if (loaded_from_cache) *loaded_from_cache = ctx->rtc_loaded;
  return 0;
}

// `b`: the binding whose source the program is compiled against and which keeps the code object (the target's, or the
// pointwise program's)
static int rtc_function(aehmc_ctx *ctx, CustomBinding &b, RtcId id, const std::string &want, hipFunction_t *out) {
  const RtcRow &row = RTC_TABLE[id.prog];
  const bool one = row.names.empty();  // one instantiation per program
  const std::tuple<int, int, std::string> key(id.prog, id.waves, one ? want : std::string());
  auto it = b.rtc.find(key);
  if (it == b.rtc.end()) {
    const std::vector<std::string> names = one ? std::vector<std::string>{want} : row.names;
    if (b.src.empty()) FAIL("internal: no user-defined source");
    std::string src = RTC_PROLOGUE;
    if (id.waves) src += "#define AEHMC_WG_MIN_WAVES " + std::to_string(id.waves) + "\n";
    if (row.mode) src += std::string("#define ") + row.mode + " 1\n";
    src += "#line 1 \"custom_target\"\n" + b.src + "\n";
    if (row.engine) src += "#include \"engine.cuh\"\n";
    for (const char *h : row.headers) src += std::string("#include \"") + h + "\"\n";
    const std::string inc = "-I" + b.inc;
    const char *opts[] = {"--offload-arch=" AEHMC_GPU_ARCH, "-O3", "-std=c++17", "-ffp-contract=off", inc.c_str(),
                          "-mllvm", "-disable-machine-licm"};  // (the flags of csrc/Makefile)
    std::vector<char> code;
    std::vector<std::string> lowered;
    std::string cache_path;
    if (!ctx->rtc_cache_dir.empty()) {
      std::string all = src;
      for (const char *o : opts)
        if (o != inc.c_str()) all += std::string("\n") + o;
      for (const auto &n : names) all += "\n" + n;
      char name[40];
      snprintf(name, sizeof(name), "/%016llx.aehmcco", (unsigned long long)fnv1a64(all));
      cache_path = ctx->rtc_cache_dir + name;
    }
    const bool cached = !cache_path.empty() && rtc_cache_load(cache_path, names, code, lowered);
    if (!cached) {
      hiprtcProgram prog;
      if (hiprtcCreateProgram(&prog, src.c_str(), "aehmc_custom.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        FAIL("hiprtcCreateProgram failed");
      for (const auto &n : names) hiprtcAddNameExpression(prog, n.c_str());
      const hiprtcResult rc = hiprtcCompileProgram(prog, 7, opts);
      if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        ctx->err = std::string("user-defined target: compilation failed (") + hiprtcGetErrorString(rc) + ")\n" + log;
        return -3;
      }
      size_t cs = 0;
      hiprtcGetCodeSize(prog, &cs);
      code.resize(cs);
      hiprtcGetCode(prog, code.data());
      lowered.clear();
      for (const auto &n : names) {
        const char *low = nullptr;
        if (hiprtcGetLoweredName(prog, n.c_str(), &low) != HIPRTC_SUCCESS || !low) {
          hiprtcDestroyProgram(&prog);
          FAIL("user-defined target: kernel " + n + " not found in the compiled program");
        }
        lowered.push_back(low);
      }
      hiprtcDestroyProgram(&prog);
      if (!cache_path.empty()) rtc_cache_store(cache_path, lowered, code);
      ctx->rtc_compiled++;
    } else {
      ctx->rtc_loaded++;
    }
    RtcProgram rp;
    if (hipModuleLoadData(&rp.mod, code.data()) != hipSuccess) {
      if (cached) remove(cache_path.c_str());  // (a damaged file: compiled afresh by the next call)
      FAIL("user-defined target: hipModuleLoadData failed");
    }
    for (size_t k = 0; k < names.size(); k++) {
      hipFunction_t f = nullptr;
      if (hipModuleGetFunction(&f, rp.mod, lowered[k].c_str()) != hipSuccess) {
        (void)hipModuleUnload(rp.mod);
        if (cached) remove(cache_path.c_str());
        FAIL("user-defined target: kernel " + names[k] + " not found in the code object");
      }
      rp.fn[names[k]] = f;
    }
    it = b.rtc.emplace(key, rp).first;
  }
  auto f = it->second.fn.find(want);
  if (f == it->second.fn.end()) FAIL("internal: kernel " + want + " was not compiled");
  *out = f->second;
  return 0;
}
template <class... Args>
static int rtc_launch_on(aehmc_ctx *ctx, CustomBinding &b, RtcId id, const std::string &want, dim3 grid, dim3 block, size_t dyn,
                         hipStream_t st, Args... args) {
  hipFunction_t f = nullptr;
  if (int rc = rtc_function(ctx, b, id, want, &f)) return rc;
  void *params[] = {(void *)&args...};
  {  // a code object whose register count does not fit the workgroup aborts the PROCESS when it is launched
     // (HSA_STATUS_ERROR_INVALID_ISA): an error return instead
    int max_threads = 0, regs = 0;
    (void)hipFuncGetAttribute(&max_threads, HIP_FUNC_ATTRIBUTE_MAX_THREADS_PER_BLOCK, f);
    (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, f);
    // (gfx950: 512 registers per lane and SIMD, four SIMDs per CU: a workgroup fits if its wavefronts per SIMD do)
    if (regs > 0 && regs <= 512) {
      const int by_regs = (512 / ((regs + 7) & ~7)) * 4 * 64;
      if (max_threads <= 0 || by_regs < max_threads) max_threads = by_regs;
    }
    if (max_threads > 0 && (int)(block.x * block.y * block.z) > max_threads) {
      FAIL("user-defined target: the kernel " + want + " compiled against it uses " + std::to_string(regs) +
           " registers per lane and can run workgroups of at most " + std::to_string(max_threads) + " threads (" +
           std::to_string(block.x * block.y * block.z) + " needed): simplify the density (long unrolled loop bodies), or "
           "use the lock-step path (set_option resident_nuts 0 / fused_hmc 0)");
    }
  }
  if (dyn >= 49152)  // (with the kernel's static LDS more than the default limit: allowed per function)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(f), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  HIPCHK(hipModuleLaunchKernel(f, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)dyn, st, params, nullptr));
  return 0;
}
template <class... Args>  // (against the bound target)
static int rtc_launch(aehmc_ctx *ctx, RtcId id, const std::string &want, dim3 grid, dim3 block, size_t dyn, hipStream_t st,
                      Args... args) {
  return rtc_launch_on(ctx, ctx->bound, id, want, grid, block, dyn, st, args...);
}
template <class... Args>  // (a launch as its family header describes it)
static int rtc_launch(aehmc_ctx *ctx, RtcId id, const KernelLaunch &k, hipStream_t st, Args... args) {
  return rtc_launch(ctx, id, k.name, k.grid, k.block, k.dyn, st, args...);
}

// The workgroup-per-chain kernels (512 threads) are compiled for FOUR wavefronts per SIMD -- 128 registers per lane, two
// workgroups per CU -- unless the program then keeps more than WG_SCRATCH_MAX bytes per lane in scratch (a density with
// many per-lane accumulators: its sweep would spill): three (168 registers, one workgroup per CU) in that case.  Logistic
// regression N = 1e5, D = 8, 1024 chains, NUTS: 28.8 -> 22.9 ms per transition (profiles/r6/INDEX.md).  "wg_waves" option:
// 3 / 4 force one.
constexpr int WG_SCRATCH_MAX = 320;
static int wg_program(aehmc_ctx *ctx, RtcProg prog, const std::string &want, int *waves) {
  if (ctx->opt_wg_waves == 3 || ctx->opt_wg_waves == 4) {
    *waves = ctx->opt_wg_waves;
    return 0;
  }
  auto it = ctx->bound.wg_choice.find({prog, want});
  if (it == ctx->bound.wg_choice.end()) {
    hipFunction_t f = nullptr;
    if (int rc = rtc_function(ctx, ctx->bound, {prog, 4}, want, &f)) return rc;
    int scratch = 0;
    (void)hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f);
    it = ctx->bound.wg_choice.emplace(std::make_pair((int)prog, want), scratch > WG_SCRATCH_MAX ? 3 : 4).first;
  }
  *waves = it->second;
  return 0;
}

__global__ void k_transpose_rect(const double *src, double *dst, long long rows, long long cols) {  // dst [cols, rows]
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < rows * cols) dst[(e % cols) * rows + e / cols] = src[e];
}
// Binding a user-defined target is a transaction: the new source is compiled and the new parameter table uploaded
// BESIDE what is bound, and only when every step has succeeded do they replace it (round 5; until then a failed compile
// left the new source and parameter table in place under the old target: the next step of the old target then
// recompiled the bad source, or read freed parameter arrays).
// the first step of a bind: the new binding's source, and the markers in it, read here and nowhere else
static CustomBinding custom_source(const char *source, const char *include_dir) {
  CustomBinding nb;
  nb.src = source;
  nb.inc = include_dir;
  nb.has_grad = nb.src.find("#define AEHMC_JOINT_GRAD") != std::string::npos;
  nb.grad_small = nb.src.find("#define AEHMC_JOINT_GRAD_SMALL") != std::string::npos;
  static const char sweep_key[] = "#define AEHMC_JOINT_SWEEP_TERMS ";
  const size_t at = nb.src.find(sweep_key);
  nb.has_sweep = at != std::string::npos;
  nb.sweep_terms = nb.has_sweep ? atoll(nb.src.c_str() + at + sizeof(sweep_key) - 1) : 0;
  return nb;
}
// installs `nb` (custom_source) with `params` in `slot` (the ctx's target binding or its pointwise binding) and compiles
// kernel `want` of program `prog`; on failure the previous binding is back in place.  The other slot is never touched
static int custom_bind(aehmc_ctx *ctx, CustomBinding &slot, CustomBinding nb, const double *const *params, int32_t n_params,
                       RtcProg prog, const std::string &want) {
  if (n_params < 0 || (n_params > 0 && !params)) FAIL("custom target: bad parameter list");
  nb.n_cparams = n_params;
  HIPCHK(hipMalloc((void **)&nb.d_cparams, (size_t)(n_params > 0 ? n_params : 1) * sizeof(double *)));
  if (n_params > 0 &&
      hipMemcpy(nb.d_cparams, params, (size_t)n_params * sizeof(double *), hipMemcpyHostToDevice) != hipSuccess) {
    custom_release(nb);
    FAIL("custom target: parameter table upload failed");
  }
  // the same function: its code objects and wg_program's picks among them stay
  const bool same_source = slot.src == nb.src && slot.inc == nb.inc;
  const auto keep_programs = [&] {
    if (!same_source) return;
    std::swap(nb.rtc, slot.rtc);
    std::swap(nb.wg_choice, slot.wg_choice);
  };
  keep_programs();
  std::swap(slot, nb);  // ctx: new binding; nb: the previous one
  hipFunction_t f = nullptr;  // compile now: errors in the user's source surface here, not in the first step
  if (int rc = rtc_function(ctx, slot, prog, want, &f)) {
    const std::string err = ctx->err;
    std::swap(slot, nb);  // ctx: the previous binding again; nb: the failed one
    keep_programs();
    custom_release(nb);
    ctx->err = err;
    return rc;
  }
  custom_release(nb);
  return 0;
}
// the bound source becomes the target: a record of its kind and D alone
static int custom_target(aehmc_ctx *ctx, aehmc_target_kind kind, int64_t D) {
  aehmc_target t{};
  t.kind = kind;
  t.D = D;
  white_release(ctx);
  ctx->tgt = t;
  ctx->has_tgt = true;
  return 0;
}
extern "C" int aehmc_set_custom_glm_target(aehmc_ctx *ctx, const char *source, int64_t D, int64_t N, const double *X,
                                           const double *y, const double *const *params, int32_t n_params,
                                           const char *include_dir) {
  if (!ctx || !source || !include_dir) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (D <= 0 || N <= 0 || !X || !y) FAIL("GLM target needs D, N, X [N,D] and y [N]");
  double *XT = nullptr;  // (allocated before anything is replaced)
  HIPCHK(hipMalloc((void **)&XT, (size_t)N * D * sizeof(double)));
  if (int rc = custom_bind(ctx, ctx->bound, custom_source(source, include_dir), params, n_params, RTC_GLM, RTC_TABLE[RTC_GLM].names[0])) {
    (void)hipFree(XT);
    return rc;
  }
  if (ctx->glm_XT) (void)hipFree(ctx->glm_XT);
  ctx->glm_XT = XT;
  hipLaunchKernelGGL(k_transpose_rect, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, 0, X, ctx->glm_XT,
                     (long long)N, (long long)D);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  ctx->glm_X = X; ctx->glm_y = y; ctx->glm_N = N;
  return custom_target(ctx, AEHMC_T_GLM, D);
}

// a traced joint density with long data sweeps and few chains on a workgroup of 8 wavefronts per chain (RTC_JWG)
static bool joint_wg_wanted(const aehmc_ctx *ctx, int64_t C) {
  if (!ctx->opt_joint_wg || !ctx->bound.has_sweep) return false;
  // (a wavefront per chain fills the GPU's 1024 SIMDs twice over at 2048 chains; a sweep of < 8192 terms is < 128 trips of a wavefront)
  return ctx->opt_joint_wg > 1 || (ctx->bound.sweep_terms >= 8192 && C <= 2048);
}
// a traced joint density on the workgroup-per-chain NUTS / HMC kernels (k_nuts_wide / k_hmc_wide, AEHMC_T_JOINT): above
// JOINT_ROWS_MAX_D by default ("joint_wide" 1), also from 513 coordinates on with "joint_wide" 2 (cross-checks), never with 0
static bool joint_wide_wanted(const aehmc_ctx *ctx) {
  const int64_t D = ctx->tgt.D;
  if (ctx->tgt.kind != AEHMC_T_JOINT || !ctx->opt_joint_wide || ctx->met.ndim >= 2 || D > JOINT_WIDE_MAX_D || !ctx->bound.has_grad)
    return false;
  // (option 2 only where the workspace rows are padded for k_nuts_wide: ws_layout, wide_rows_padded)
  return D > JOINT_ROWS_MAX_D || (ctx->opt_joint_wide == 2 && wide_rows_padded(D));
}
// LDS of a workgroup that holds ONE chain's position and gradient rows (`row` doubles each: D + 1 for the wide kernels,
// D for k_target_joint_wg) next to the kernel's static arrays (`f`: the compiled kernel), against the CU's 160 KiB
constexpr size_t CU_LDS_BYTES = 163840;
// rtc_launch of such a kernel, after that budget check
template <class... Args>
static int joint_rows_launch(aehmc_ctx *ctx, RtcProg prog, const std::string &want, int64_t row, dim3 grid, dim3 block,
                             hipStream_t st, Args... args) {
  hipFunction_t f = nullptr;
  if (int rc = rtc_function(ctx, ctx->bound, prog, want, &f)) return rc;
  int stat = 0;
  if (hipFuncGetAttribute(&stat, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, f) != hipSuccess || stat < 0)
    FAIL("joint target: the static LDS size of the compiled kernel could not be read");
  const size_t dyn = (size_t)2 * row * sizeof(double);
  if (dyn + (size_t)stat > CU_LDS_BYTES)
    FAIL("joint target: D = " + std::to_string(ctx->tgt.D) + " needs " + std::to_string(dyn + stat) +
         " bytes of LDS for one chain's position and gradient rows, the CU has " + std::to_string(CU_LDS_BYTES));
  return rtc_launch(ctx, prog, want, grid, block, dyn, st, args...);
}
extern "C" int aehmc_set_custom_joint_target(aehmc_ctx *ctx, const char *source, int64_t D, const double *const *params,
                                             int32_t n_params, const char *include_dir) {
  if (!ctx || !source || !include_dir) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  // (D <= 64: one coordinate per lane, the single-launch kernels; above: the position row in LDS -- four chains' rows per
  //  workgroup up to JOINT_ROWS_MAX_D, one chain's above, which takes the density's reverse-mode program)
  CustomBinding nb = custom_source(source, include_dir);
  const bool grad = nb.has_grad;
  const int64_t dmax = grad ? JOINT_WIDE_MAX_D : JOINT_ROWS_MAX_D;
  if (D <= 0 || D > dmax)
    FAIL("joint target: D must be in [1, " + std::to_string(dmax) + "]" +
         (grad ? std::string() : " without a reverse-mode program (AEHMC_JOINT_GRAD: up to " + std::to_string(JOINT_WIDE_MAX_D) + ")"));
  const RtcProg prog = D > JOINT_ROWS_MAX_D ? RTC_JTWG : RTC_JBASE;
  if (int rc = custom_bind(ctx, ctx->bound, std::move(nb), params, n_params, prog, RTC_TABLE[prog].names[0])) return rc;
  return custom_target(ctx, AEHMC_T_JOINT, D);
}

extern "C" int aehmc_set_custom_target(aehmc_ctx *ctx, const char *source, int64_t D, const double *const *params,
                                       int32_t n_params, const char *include_dir) {
  if (!ctx || !source || !include_dir) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (D <= 0) FAIL("target: D must be positive");
  if (int rc = custom_bind(ctx, ctx->bound, custom_source(source, include_dir), params, n_params, RTC_BASE, RTC_TABLE[RTC_BASE].names[0])) return rc;
  return custom_target(ctx, AEHMC_T_CUSTOM, D);
}

static int gemm(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                const double *B, int64_t ldb, double *Cm, int64_t ldc, hipStream_t st,
                const int *row_idx = nullptr, const int *n_rows = nullptr, int mode = 0, int tri = 0,
                bool carry_in = false, bool in_place = false);

// Blocked (64-wide) right-looking Cholesky of Lw [D,D] in place (lower triangle; the upper one keeps the input);
// `inv`, `invT`: [NB,NB] scratch each, `info`: the first failed pivot
static int dense_cholesky(aehmc_ctx *ctx, double *Lw, int64_t D, double *inv, double *invT, int *info, hipStream_t st) {
  const int NB = FACT_NB;
  int rc = 0;
  for (int64_t j0 = 0; j0 < D && !rc; j0 += NB) {
    const int nb = (int)((D - j0 < NB) ? D - j0 : NB);
    const int64_t M = D - j0 - nb;
    hipLaunchKernelGGL(k_potrf_trtri, dim3(1), dim3(256), 0, st, Lw + j0 * D + j0, (long long)D, nb, 1, inv,
                       invT, info, (int)j0);
    if (M > 0) {
      double *panel = Lw + (j0 + nb) * D + j0;
      // L21 = A21 L11^-T, in place: only on kernels whose workgroups own complete rows (launch_gemm_nt_f64: in_place)
      rc = gemm(ctx, M, nb, nb, panel, D, inv, NB, panel, D, st, nullptr, nullptr, 0, 0, false, true);
      if (!rc) rc = gemm(ctx, M, M, nb, panel, D, panel, D, Lw + (j0 + nb) * D + (j0 + nb), D, st, nullptr,
                         nullptr, 1);                                                   // A22 -= L21 L21^T
    }
  }
  return rc;
}

// metrics.py:56-58: L = cholesky(imm); mass_matrix_sqrt = solve_triangular(L, I, lower, trans)
// = L^-T.  Blocked (64-wide) right-looking Cholesky and blocked triangular inverse; the
// O(D^3) work is in the fp64 MFMA GEMM.  `out` [D,D] receives L^-T.
// `pd_is_data`: a matrix that is not positive definite is no error -- `out` is filled with NaNs (pooled warm-up: an
// estimate, as the per-chain warm-up kernel leaves them)
static int dense_sqrt_mass(aehmc_ctx *ctx, const double *imm, int64_t D, double *out, hipStream_t st,
                           bool pd_is_data = false) {
  const int NB = FACT_NB;
  double *Lw = nullptr, *Li = nullptr, *small = nullptr, *Tt = nullptr;
  int *info = nullptr;
  HIPCHK(hipMalloc((void **)&Lw, (size_t)D * D * sizeof(double)));
  HIPCHK(hipMalloc((void **)&Li, (size_t)D * D * sizeof(double)));
  HIPCHK(hipMalloc((void **)&small, (size_t)2 * NB * NB * sizeof(double)));
  HIPCHK(hipMalloc((void **)&Tt, (size_t)NB * D * sizeof(double)));
  HIPCHK(hipMalloc((void **)&info, sizeof(int)));
  double *inv = small, *invT = small + NB * NB;
  int rc = 0, h_info = 0;
  auto done = [&](int r) {
    (void)hipFree(Lw); (void)hipFree(Li); (void)hipFree(small); (void)hipFree(Tt); (void)hipFree(info);
    return r;
  };
  if (hipMemcpyAsync(Lw, imm, (size_t)D * D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemsetAsync(Li, 0, (size_t)D * D * sizeof(double), st) != hipSuccess ||
      hipMemsetAsync(info, 0, sizeof(int), st) != hipSuccess) {
    ctx->err = "dense metric: device copy failed";
    return done(-1);
  }
  rc = dense_cholesky(ctx, Lw, D, inv, invT, info, st);
  const int64_t nblk = (D + NB - 1) / NB;
  for (int64_t kb = nblk - 1; kb >= 0 && !rc; kb--) {  // L^-1, block column by block column
    const int64_t j0 = kb * NB;
    const int nb = (int)((D - j0 < NB) ? D - j0 : NB);
    const int64_t M = D - j0 - nb;
    hipLaunchKernelGGL(k_potrf_trtri, dim3(1), dim3(256), 0, st, Lw + j0 * D + j0, (long long)D, nb, 0, inv,
                       invT, info, (int)j0);
    hipLaunchKernelGGL(k_copy_block, dim3(16), dim3(256), 0, st, (const double *)inv, (long long)NB,
                       Li + j0 * D + j0, (long long)D, nb, nb);
    if (M > 0) {
      // T^T = L11^-T L21^T  ([nb, M]);  L^-1[>k, k] = - L^-1[>k, >k] T
      rc = gemm(ctx, nb, M, nb, invT, NB, Lw + (j0 + nb) * D + j0, D, Tt, M, st);
      if (!rc) rc = gemm(ctx, M, nb, M, Li + (j0 + nb) * D + (j0 + nb), D, Tt, M, Li + (j0 + nb) * D + j0, D, st,
                         nullptr, nullptr, 2);
    }
  }
  if (!rc) {
    dim3 grid((unsigned)((D + 31) / 32), (unsigned)((D + 31) / 32)), block(32, 8);
    hipLaunchKernelGGL(k_transpose, grid, block, 0, st, (const double *)Li, out, (long long)D);
    // (on the caller's stream: an `imm` produced there is complete before it is read, and the factor before return)
    if (hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
      ctx->err = "dense metric: factorisation kernels failed";
      rc = -1;
    } else if (h_info && pd_is_data) {
      if (hipMemsetAsync(out, 0xFF, (size_t)D * D * sizeof(double), st) != hipSuccess) {  // (all bits set: a NaN)
        ctx->err = "dense metric: device fill failed";
        rc = -1;
      }
    } else if (h_info) {
      ctx->err = "dense inverse mass matrix is not positive definite (pivot " + std::to_string(h_info) + ")";
      rc = -2;
    }
  }
  return done(rc);
}

extern "C" int aehmc_set_metric(aehmc_ctx *ctx, const aehmc_metric *m) {
  if (!ctx || !m) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (m->ndim < 0 || m->ndim > 2)  // metrics.py:60-63
    FAIL("Expected a mass matrix of dimension 1 (diagonal) or 2, got " + std::to_string(m->ndim));
  if (!m->imm || m->D <= 0) FAIL("metric needs imm and D");
  if (m->per_chain && m->ndim == 2 && m->D > AEHMC_PC_DENSE_MAX_D)
    FAIL("per-chain dense mass matrices are supported up to D = " + std::to_string(AEHMC_PC_DENSE_MAX_D));
  if (m->per_chain && !m->sqrt_mass)
    FAIL("per-chain metrics need sqrt_mass (dense: aehmc_metric_sqrt_per_chain)");
  if (m->per_chain && m->n_chains <= 0) FAIL("per-chain metrics need n_chains");
  aehmc_metric met = *m;
  if (!met.sqrt_mass) {  // metrics.py:45,49,56-58 computed here
    const int64_t n = m->ndim == 0 ? 1 : (m->ndim == 1 ? m->D : m->D * m->D);
    if (ctx->own_sqrt_mass_n < n) {
      if (ctx->own_sqrt_mass) HIPCHK(hipFree(ctx->own_sqrt_mass));
      ctx->own_sqrt_mass = nullptr;
      HIPCHK(hipMalloc((void **)&ctx->own_sqrt_mass, n * sizeof(double)));
      ctx->own_sqrt_mass_n = n;
    }
    HIPCHK(hipDeviceSynchronize());  // (no stream argument here: whatever produced `imm`, on any stream, is complete)
    if (m->ndim < 2) {
      hipLaunchKernelGGL(k_sqrt_recip, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, m->imm,
                         ctx->own_sqrt_mass, (long long)n);
      HIPCHK(hipGetLastError());
      HIPCHK(hipDeviceSynchronize());
    } else if (int rc = dense_sqrt_mass(ctx, m->imm, m->D, ctx->own_sqrt_mass, 0)) {
      return rc;
    }
    met.sqrt_mass = ctx->own_sqrt_mass;
  }
  white_release(ctx, met.ndim == 2 && !met.per_chain);
  ctx->met = met;
  ctx->has_met = true;
  return 0;
}

extern "C" int aehmc_metric_sqrt(aehmc_ctx *ctx, int32_t ndim, int64_t D, const double *imm, double *sqrt_mass,
                                 void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (ndim < 0 || ndim > 2)
    FAIL("Expected a mass matrix of dimension 1 (diagonal) or 2, got " + std::to_string(ndim));
  if (!imm || !sqrt_mass || D <= 0) FAIL("metric_sqrt: bad arguments");
  // on the caller's stream (ordered behind whatever produced `imm` there) and complete on return
  hipStream_t st = (hipStream_t)stream;
  if (ndim < 2) {
    const int64_t n = ndim == 0 ? 1 : D;
    hipLaunchKernelGGL(k_sqrt_recip, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, imm, sqrt_mass, (long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  return dense_sqrt_mass(ctx, imm, D, sqrt_mass, st);
}

extern "C" int aehmc_metric_sqrt_per_chain(aehmc_ctx *ctx, int64_t C, int64_t D, const double *imm,
                                           double *sqrt_mass, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (!imm || !sqrt_mass || C <= 0 || D <= 0) FAIL("metric_sqrt_per_chain: bad arguments");
  if (D > AEHMC_PC_DENSE_MAX_D)
    FAIL("per-chain dense mass matrices are supported up to D = " + std::to_string(AEHMC_PC_DENSE_MAX_D));
  ctx->h_err[1] = 0;
  const bool in_lds = D <= AEHMC_PC_LDS_MAX_D;
  const size_t dyn = in_lds ? (size_t)2 * D * D * sizeof(double) : 0;
  double *work = nullptr;
  if (!in_lds) {  // the factor is formed in a scratch copy: kept with the ctx, not allocated per call
    if (int rc = grow(ctx, &ctx->pc_work, &ctx->pc_work_bytes, (size_t)C * D * D * sizeof(double))) return rc;
    work = ctx->pc_work;
  }
  if (dyn)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_chol_inv_pc),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  hipLaunchKernelGGL(k_chol_inv_pc, dim3((unsigned)C), dim3(64), dyn, (hipStream_t)stream, imm, sqrt_mass,
                     (long long)C, (int)D, ctx->d_err + 1, work);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (ctx->h_err[1]) {
    ctx->h_err[1] = 0;
    FAIL("inverse mass matrix of some chain is not positive definite");
  }
  return 0;
}

extern "C" int aehmc_set_step_sizes(aehmc_ctx *ctx, const double *step_sizes, int64_t n) {
  if (!ctx) return -2;
  if (step_sizes && n <= 0) FAIL("set_step_sizes: n must be the number of chains");
  ctx->eps_c = step_sizes;
  ctx->eps_n = step_sizes ? n : 0;
  return 0;
}

static int adapt_args(aehmc_ctx *ctx, int64_t C, int64_t D, const aehmc_adapt_state *s, AdaptArgs &a) {
  if (!s || C <= 0 || D <= 0) FAIL("adaptation: bad arguments");
  if (!s->da_step || !s->da_x || !s->da_x_avg || !s->da_g_avg || !s->da_mu || !s->wc_mean ||
      !s->wc_m2 || !s->wc_n || !s->step_size || !s->imm || !s->sqrt_mass)
    FAIL("adaptation: state arrays missing");
  memset(&a, 0, sizeof(a));
  a.C = C; a.D = D; a.s = *s;
  a.gamma = 0.05; a.t0 = 10; a.kappa = 0.75;  // step_size.py:9-14
  return 0;
}
extern "C" int aehmc_adapt_init(aehmc_ctx *ctx, int64_t C, int64_t D, double initial_step_size,
                                const aehmc_adapt_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  AdaptArgs a;
  if (int rc = adapt_args(ctx, C, D, state, a)) return rc;
  if (state->full && D > AEHMC_PC_DENSE_MAX_D)
    FAIL("full mass-matrix adaptation is supported up to D = " + std::to_string(AEHMC_PC_DENSE_MAX_D));
  hipLaunchKernelGGL(k_adapt_init, chain_grid(C), dim3(256), 0, (hipStream_t)stream, a, initial_step_size);
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aehmc_adapt_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t stage,
                                  int32_t is_window_end, int32_t is_last, double target,
                                  const double *p_accept, const double *position,
                                  const aehmc_adapt_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  AdaptArgs a;
  if (int rc = adapt_args(ctx, C, D, state, a)) return rc;
  if (!p_accept || !position) FAIL("adaptation: acceptance_probability / position missing");
  a.stage = stage; a.window_end = is_window_end; a.last = is_last; a.target = target;
  a.p_accept = p_accept; a.position = position;
  if (state->full) {  // one wavefront per workgroup: delta vectors (and, D <= 64, the window-end factorisation) in LDS
    if (D > AEHMC_PC_DENSE_MAX_D)
      FAIL("full mass-matrix adaptation is supported up to D = " + std::to_string(AEHMC_PC_DENSE_MAX_D));
    if (D > AEHMC_PC_LDS_MAX_D && !state->work) FAIL("full mass-matrix adaptation with D > 64 needs state->work [C,D,D]");
    const size_t dyn = (size_t)(2 * D + (D <= AEHMC_PC_LDS_MAX_D ? 2 * D * D : 0)) * sizeof(double);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_adapt_update),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(k_adapt_update, dim3((unsigned)C), dim3(64), dyn, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(k_adapt_update, chain_grid(C), dim3(256), 0, (hipStream_t)stream, a);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- pooled window adaptation (pooled_adapt.cuh, syrk_f64.cuh) ----
static int pool_args(aehmc_ctx *ctx, int64_t C, int64_t D, const aehmc_pooled_adapt_state *s, PoolArgs &a) {
  if (!s || C <= 0 || D <= 0) FAIL("pooled adaptation: bad arguments");
  if (!s->da_step || !s->da_x || !s->da_x_avg || !s->da_g_avg || !s->da_mu || !s->wc_mean || !s->wc_m2 || !s->wc_n ||
      !s->step_size || !s->imm || !s->sqrt_mass)
    FAIL("pooled adaptation: state arrays missing");
  memset(&a, 0, sizeof(a));
  a.C = C; a.D = D; a.s = *s;
  a.gamma = 0.05; a.t0 = 10; a.kappa = 0.75;  // step_size.py:9-14
  pool_parts(C, D, a.P, a.rows_per);
  if (int rc = grow(ctx, &ctx->pool_work, &ctx->pool_work_bytes, pool_work_doubles(C, D) * sizeof(double))) return rc;
  a.part = ctx->pool_work;
  a.b = a.part + (size_t)a.P * (D + 1);
  a.delta = a.b + D;
  a.sc = a.delta + D;
  return 0;
}
static int syrk(aehmc_ctx *ctx, int64_t C, int64_t D, const double *X, int64_t ldx, const double *centre, double w,
                const double *w_dev, const double *delta, double *S, int64_t lds_, hipStream_t st) {
  if (int rc = grow(ctx, &ctx->syrk_work, &ctx->syrk_work_bytes, tu::syrk_partial_doubles(C, D) * sizeof(double)))
    return rc;
  HIPCHK(tu::syrk_tn(C, D, X, ldx, centre, w, w_dev, delta, S, lds_, ctx->syrk_work, st));
  return 0;
}
extern "C" int aehmc_syrk_tn(aehmc_ctx *ctx, int64_t C, int64_t D, const double *X, int64_t ldx, const double *centre,
                             double w, const double *delta, double *S, int64_t lds_, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (C <= 0 || D <= 0 || !X || !S || ldx < D || lds_ < D) FAIL("syrk_tn: bad arguments");
  return syrk(ctx, C, D, X, ldx, centre, w, nullptr, delta, S, lds_, (hipStream_t)stream);
}
extern "C" int aehmc_pooled_adapt_init(aehmc_ctx *ctx, int64_t C, int64_t D, double initial_step_size,
                                       const aehmc_pooled_adapt_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  PoolArgs a;
  if (int rc = pool_args(ctx, C, D, state, a)) return rc;
  HIPCHK(tu::pool_init(a, initial_step_size, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_pooled_adapt_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t stage, int32_t is_window_end,
                                         int32_t is_last, double target, const double *p_accept,
                                         const double *position, const aehmc_pooled_adapt_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  PoolArgs a;
  if (int rc = pool_args(ctx, C, D, state, a)) return rc;
  if (!p_accept || !position) FAIL("pooled adaptation: acceptance_probability / position missing");
  if (is_window_end && stage == 0) FAIL("pooled adaptation: a window ends in a slow stage");
  a.stage = stage; a.window_end = is_window_end; a.last = is_last; a.target = target;
  a.p_accept = p_accept; a.position = position;
  HIPCHK(tu::pool_sums(a, st));
  if (state->full && stage != 0) {
    if (int rc = syrk(ctx, C, D, position, D, a.b, 0.0, a.sc, a.delta, state->wc_m2, D, st)) return rc;
    if (is_window_end) {
      HIPCHK(tu::pool_imm(a, st));
      if (int rc = dense_sqrt_mass(ctx, state->imm, D, state->sqrt_mass, st, true)) return rc;
    }
  }
  HIPCHK(tu::pool_scalars(a, st));
  return 0;
}

// ---- ChEES warm-up: trajectory length and step size from all chains (chees.cuh) ----
static int chees_args(aehmc_ctx *ctx, int64_t C, int64_t D, const aehmc_chees_state *s, CheesArgs &a) {
  if (!s || C <= 0 || D <= 0) FAIL("chees: bad arguments");
  if (!s->step || !s->log_T || !s->log_T_avg || !s->adam_m || !s->adam_v || !s->h || !s->num_steps || !s->da_step ||
      !s->da_x || !s->da_x_avg || !s->da_g_avg || !s->da_mu || !s->step_size)
    FAIL("chees: state arrays missing");
  memset(&a, 0, sizeof(a));
  a.C = C; a.D = D; a.s = *s;
  chees_parts(C, D, a.P, a.rows_per);
  if (int rc = grow(ctx, &ctx->chees_work, &ctx->chees_work_bytes, chees_work_doubles(C, D) * sizeof(double))) return rc;
  a.part = ctx->chees_work;
  a.m0 = a.part + (size_t)a.P * (2 * D + 2);
  a.m1 = a.m0 + D;
  a.sc = a.m1 + D;
  return 0;
}
extern "C" int aehmc_chees_init(aehmc_ctx *ctx, int64_t C, double initial_step_size, double initial_trajectory_length,
                                const aehmc_chees_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  CheesArgs a;
  if (int rc = chees_args(ctx, C, 1, state, a)) return rc;
  if (!(initial_step_size > 0) || !(initial_trajectory_length > 0))
    FAIL("chees: initial_step_size and initial_trajectory_length must be positive");
  a.max_steps = (long long)1 << 62;  // (the cap comes with the first update)
  HIPCHK(tu::chees_init(a, initial_step_size, initial_trajectory_length, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_chees_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t is_last, double target_acceptance_rate,
                                  double learning_rate, int64_t max_num_steps, const double *position_before,
                                  const double *position_after, const double *velocity_or_momentum,
                                  const double *inverse_mass_diag, double inverse_mass_scalar, const int32_t *accepted,
                                  const double *acceptance_probability, const aehmc_chees_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  CheesArgs a;
  if (int rc = chees_args(ctx, C, D, state, a)) return rc;
  if (!position_before || !position_after || !velocity_or_momentum || !accepted || !acceptance_probability)
    FAIL("chees: positions / momentum / accept flags / acceptance_probability missing");
  if (max_num_steps < 1) FAIL("chees: max_num_steps must be at least 1");
  a.last = is_last; a.target = target_acceptance_rate; a.lr = learning_rate; a.max_steps = max_num_steps;
  a.q0 = position_before; a.q1 = position_after; a.mom = velocity_or_momentum;
  a.imm = inverse_mass_diag; a.imm_scalar = inverse_mass_scalar;
  a.accepted = accepted; a.p_accept = acceptance_probability;
  HIPCHK(tu::chees_update(a, (hipStream_t)stream));
  return 0;
}

extern "C" int aehmc_dual_averaging_update(aehmc_ctx *ctx, int64_t C, double target_acceptance_rate, double gamma,
                                           double t0, double kappa, const double *acceptance_probability,
                                           int64_t *step, double *iterates, double *iterates_avg,
                                           double *gradient_avg, const double *shrinkage_pts,
                                           double *step_size_out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (C <= 0 || !acceptance_probability || !step || !iterates || !iterates_avg || !gradient_avg || !shrinkage_pts)
    FAIL("dual_averaging_update: bad arguments");
  hipLaunchKernelGGL(k_dual_averaging, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (long long)C, target_acceptance_rate, gamma, t0, kappa, acceptance_probability,
                     (long long *)step, iterates, iterates_avg, gradient_avg, shrinkage_pts, step_size_out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aehmc_welford_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t full, const double *value,
                                    double *mean, double *m2, int64_t *sample_size, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (C <= 0 || D <= 0 || !value || !mean || !m2 || !sample_size) FAIL("welford_update: bad arguments");
  const size_t dyn = full ? (size_t)2 * D * sizeof(double) : 0;
  if (dyn > 64 * 1024) FAIL("welford_update: full covariance is supported up to D = 4096");
  hipLaunchKernelGGL(k_welford_update, dim3((unsigned)C), dim3(64), dyn, (hipStream_t)stream, (long long)C, (long long)D,
                     (int)full, value, mean, m2, (long long *)sample_size);
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aehmc_covariance_final(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t full, int32_t shrink,
                                      const double *m2, const int64_t *sample_size, double *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (C <= 0 || D <= 0 || !m2 || !sample_size || !out) FAIL("covariance_final: bad arguments");
  const long long per = full ? D * D : D;
  hipLaunchKernelGGL(k_covariance_final, dim3((unsigned)((C * per + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (long long)C, per, (long long)D, (int)full, (int)shrink, m2, (const long long *)sample_size, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// Posterior summaries (summary.cuh): caller-owned buffers only -- no workspace, no EngineArgs, nothing the whitened
// carry record depends on.
static int summary_shape(aehmc_ctx *ctx, const char *what, int64_t N, int64_t C, int64_t D, int32_t S) {
  if (N <= 0 || C <= 0 || D <= 0 || (S != 1 && S != 2)) FAIL(std::string(what) + ": bad arguments");
  if (N / S < 2) FAIL(std::string(what) + ": a segment needs at least two draws");
  if (C * D > (int64_t)1 << 38) FAIL(std::string(what) + ": C * D is too large");
  return 0;
}
extern "C" int aehmc_summary_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws,
                                    int32_t n_segments, const double *samples, double *mean, double *m2, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = summary_shape(ctx, "summary_update", num_draws, C, D, n_segments)) return rc;
  if (T <= 0 || t0 < 0 || t0 + T > num_draws || !samples || !mean || !m2) FAIL("summary_update: bad arguments");
  HIPCHK(tu::summary_update(samples, T, C * D, t0, num_draws, n_segments, mean, m2, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_autocov(aehmc_ctx *ctx, int64_t num_draws, int64_t C, int64_t D, int32_t n_segments,
                                     int64_t K, int64_t G, const double *samples, const double *mean, double *work,
                                     double *acov, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = summary_shape(ctx, "summary_autocov", num_draws, C, D, n_segments)) return rc;
  const int64_t n = num_draws / n_segments;
  if (!samples || !mean || !work || !acov || G < 1 || G > n_segments * C || G > 65535)
    FAIL("summary_autocov: bad arguments");
  if (K < 2 || K > n) FAIL("summary_autocov: the number of lags K must be in [2, segment length]");
  if (n + K > AEHMC_SUMMARY_MAX_ROWS)
    FAIL("summary_autocov: segment length + lags is " + std::to_string(n + K) + ", supported up to " +
         std::to_string(AEHMC_SUMMARY_MAX_ROWS) + " (use fewer lags)");
  HIPCHK(tu::summary_acov(samples, mean, work, acov, num_draws, C, D, n_segments, K, (int)G, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_final(aehmc_ctx *ctx, int64_t num_draws, int64_t C, int64_t D, int32_t n_segments,
                                   int64_t K, const double *mean, const double *m2, const double *acov, double *out,
                                   int32_t *lag_truncated, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = summary_shape(ctx, "summary_final", num_draws, C, D, n_segments)) return rc;
  if (!mean || !m2 || !out) FAIL("summary_final: bad arguments");
  if (acov && (!lag_truncated || K < 2)) FAIL("summary_final: acov needs lag_truncated and K >= 2");
  HIPCHK(tu::summary_final(mean, m2, acov, out, lag_truncated, num_draws / n_segments, (int64_t)n_segments * C, D, K,
                           (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_lag_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws,
                                        int32_t n_segments, int64_t K, const double *samples, double *shift,
                                        double *sums, double *ring, double *head, double *work, double *acov,
                                        void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = summary_shape(ctx, "summary_lag_update", num_draws, C, D, n_segments)) return rc;
  if (T <= 0 || t0 < 0 || t0 + T > num_draws || !samples || !shift || !sums || !ring || !head || !work || !acov)
    FAIL("summary_lag_update: bad arguments");
  if (K < 2 || K > num_draws / n_segments)
    FAIL("summary_lag_update: the number of lags K must be in [2, segment length]");
  const int cg = tu::summary_lag_group(K);
  if ((C + cg - 1) / cg > 65535) FAIL("summary_lag_update: more than 65535 groups of chains");
  HIPCHK(tu::summary_lag_update(samples, T, C, D, t0, num_draws, n_segments, K, cg, shift, sums, ring, head, work, acov,
                                (hipStream_t)stream));
  return 0;
}
extern "C" int64_t aehmc_summary_lag_group(int64_t K) { return K < 2 ? 0 : tu::summary_lag_group(K); }

// Nested R-hat of many short chains (nested.cuh): caller-owned buffers only, as the summaries above.  Its own shape
// check: a window may be a single draw, which summary_shape refuses.
extern "C" int aehmc_nested_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws,
                                   int64_t window, int64_t chains_per_superchain, const double *samples, double *mean,
                                   double *m2, double *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t M = chains_per_superchain;
  if (num_draws <= 0 || C <= 0 || D <= 0 || T <= 0 || t0 < 0 || t0 + T > num_draws || !samples || !mean || !m2 || !out)
    FAIL("nested_update: bad arguments");
  if (window < 1 || num_draws % window) FAIL("nested_update: num_draws must be a multiple of window >= 1");
  if (M < 1 || C % M || C / M < 2) FAIL("nested_update: C must be at least 2 superchains of chains_per_superchain chains");
  if (window == 1 && M == 1)
    FAIL("nested_update: a window of one draw with one chain per superchain leaves nothing to estimate inside a superchain");
  if (C * D > (int64_t)1 << 38) FAIL("nested_update: C * D is too large");
  const int64_t nwin = (t0 + T) / window - t0 / window;
  if (nwin * tu::nested_blocks(D) >= (int64_t)1 << 31)
    FAIL("nested_update: more than 2^31 workgroups, fold fewer windows a call");
  HIPCHK(tu::nested_update(samples, T, C, D, t0, window, M, mean, m2, out, (hipStream_t)stream));
  return 0;
}

// Order statistics and quantiles of the stored draws (quantile.cuh): the same conventions -- caller-owned buffers only.
static int quantile_shape(aehmc_ctx *ctx, const char *what, int64_t R, int64_t D, int64_t M, const void *samples,
                          const void *host, const void *out, const void *work, int64_t work_bytes) {
  if (R < 1 || D < 1 || M < 1 || !samples || !host || !out || !work) FAIL(std::string(what) + ": bad arguments");
  if ((uintptr_t)work % 256) FAIL(std::string(what) + ": work must be 256-byte aligned");
  if (R >= (int64_t)1 << 31) FAIL(std::string(what) + ": the counts are 32-bit, R must be below 2^31");
  if (D >= (int64_t)1 << 31) FAIL(std::string(what) + ": D is too large");
  if (M > AEHMC_SUMMARY_QUANTILE_MAX)
    FAIL(std::string(what) + ": at most " + std::to_string(AEHMC_SUMMARY_QUANTILE_MAX) + " ranks or probabilities a call");
  if (work_bytes < (int64_t)tu::quantile_work_bytes(D, M))
    FAIL(std::string(what) + ": work holds " + std::to_string(work_bytes) + " bytes, aehmc_summary_quantile_work gives " +
         std::to_string(tu::quantile_work_bytes(D, M)));
  return 0;
}
// the distinct ranks, ascending, and for every entry of `want` its row among them
static std::vector<long long> quantile_rows(const std::vector<long long> &want, std::vector<int> &row) {
  std::vector<long long> u(want);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  row.resize(want.size());
  for (size_t i = 0; i < want.size(); ++i) row[i] = (int)(std::lower_bound(u.begin(), u.end(), want[i]) - u.begin());
  return u;
}
// numpy's "linear" rule over R pooled draws: per probability the virtual index h = p (R - 1), its floor and the gap g;
// u: the distinct ranks floor(h), min(floor(h) + 1, R - 1) of all probabilities, ascending; lo / hi: their rows in u
static int quantile_ranks(aehmc_ctx *ctx, const char *what, int64_t R, int64_t Q, const double *probs,
                          std::vector<long long> &u, std::vector<int> &lo, std::vector<int> &hi, std::vector<double> &g) {
  std::vector<long long> want(2 * Q);
  g.resize(Q);
  for (int64_t i = 0; i < Q; ++i) {
    const double p = probs[i];
    if (!(p >= 0.0 && p <= 1.0))
      FAIL(std::string(what) + ": probability " + std::to_string(p) + " is outside [0, 1]");
    const double h = p * (double)(R - 1), fl = std::floor(h);
    const long long k = (long long)fl;
    g[i] = h - fl;
    want[2 * i] = k;
    want[2 * i + 1] = k + 1 < R ? k + 1 : R - 1;
  }
  std::vector<int> row;
  u = quantile_rows(want, row);
  lo.resize(Q);
  hi.resize(Q);
  for (int64_t i = 0; i < Q; ++i) {
    lo[i] = row[2 * i];
    hi[i] = row[2 * i + 1];
  }
  return 0;
}
extern "C" int64_t aehmc_summary_quantile_work(int64_t R, int64_t D, int64_t M) {
  if (R < 1 || D < 1 || M < 1 || M > AEHMC_SUMMARY_QUANTILE_MAX || D >= (int64_t)1 << 31) return 0;
  return (int64_t)tu::quantile_work_bytes(D, M);
}
extern "C" int aehmc_summary_order_stats(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t M, const double *samples,
                                         const int64_t *ranks, double *out, void *work, int64_t work_bytes,
                                         void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = quantile_shape(ctx, "summary_order_stats", R, D, M, samples, ranks, out, work, work_bytes)) return rc;
  std::vector<long long> want(M);
  for (int64_t i = 0; i < M; ++i) {
    if (ranks[i] < 0 || ranks[i] >= R)
      FAIL("summary_order_stats: rank " + std::to_string(ranks[i]) + " is outside [0, " + std::to_string(R) + ")");
    want[i] = ranks[i];
  }
  std::vector<int> row;
  const std::vector<long long> u = quantile_rows(want, row);
  HIPCHK(tu::quantile_stats(samples, R, D, (int)u.size(), u.data(), work, M, (hipStream_t)stream));
  HIPCHK(tu::quantile_out(work, D, M, (int)M, row.data(), nullptr, nullptr, out, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_quantiles(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t Q, const double *samples,
                                       const double *probs, double *out, void *work, int64_t work_bytes, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = quantile_shape(ctx, "summary_quantiles", R, D, Q, samples, probs, out, work, work_bytes)) return rc;
  std::vector<int> lo, hi;
  std::vector<double> g;
  std::vector<long long> u;
  if (int rc = quantile_ranks(ctx, "summary_quantiles", R, Q, probs, u, lo, hi, g)) return rc;
  HIPCHK(tu::quantile_stats(samples, R, D, (int)u.size(), u.data(), work, Q, (hipStream_t)stream));
  HIPCHK(tu::quantile_out(work, D, Q, (int)Q, lo.data(), hi.data(), g.data(), out, (hipStream_t)stream));
  return 0;
}

// Streaming quantiles (sketch.cuh): a fixed-grid histogram per coordinate, the same conventions.
static int sketch_shape(aehmc_ctx *ctx, const char *what, int64_t D, int64_t B) {
  if (D < 1) FAIL(std::string(what) + ": bad arguments");
  if (D >= (int64_t)1 << 31) FAIL(std::string(what) + ": D is too large");
  if (B < AEHMC_SUMMARY_SKETCH_MIN_BINS || B > AEHMC_SUMMARY_SKETCH_MAX_BINS || (B & (B - 1)))
    FAIL(std::string(what) + ": the number of bins must be a power of two in [" +
         std::to_string(AEHMC_SUMMARY_SKETCH_MIN_BINS) + ", " + std::to_string(AEHMC_SUMMARY_SKETCH_MAX_BINS) + "], got " +
         std::to_string(B));
  return 0;
}
extern "C" int aehmc_summary_sketch_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t B,
                                           const double *samples, const double *lo, const double *inv_width,
                                           int64_t *counts, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = sketch_shape(ctx, "summary_sketch_update", D, B)) return rc;
  if (T < 1 || C < 1 || !samples || !lo || !inv_width || !counts) FAIL("summary_sketch_update: bad arguments");
  if (T >= (int64_t)1 << 31 || C >= (int64_t)1 << 31 || T * C >= (int64_t)1 << 31)
    FAIL("summary_sketch_update: a workgroup counts in 32 bits, T * C must be below 2^31");
  HIPCHK(tu::sketch_update(samples, T * C, D, (int)B, lo, inv_width, (unsigned long long *)counts, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_sketch_quantiles(aehmc_ctx *ctx, int64_t D, int64_t B, int64_t Q, const double *probs,
                                              const int64_t *counts, const double *lo, const double *width,
                                              double *estimate, int32_t *resolved, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = sketch_shape(ctx, "summary_sketch_quantiles", D, B)) return rc;
  if (Q < 1 || !probs || !counts || !lo || !width || !estimate || !resolved)
    FAIL("summary_sketch_quantiles: bad arguments");
  if (Q > AEHMC_SUMMARY_QUANTILE_MAX)
    FAIL("summary_sketch_quantiles: at most " + std::to_string(AEHMC_SUMMARY_QUANTILE_MAX) + " probabilities a call");
  // the ranks need the number of pooled draws: every coordinate has counted the same, the first one's counters say it
  std::vector<unsigned long long> first(B + 3);
  HIPCHK(hipMemcpyAsync(first.data(), counts, first.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long total = 0;
  for (unsigned long long n : first) total += n;
  if (total < 1) FAIL("summary_sketch_quantiles: no draw has been counted");
  if (total >= 1ULL << 53) FAIL("summary_sketch_quantiles: the ranks are computed in fp64, the count must be below 2^53");
  std::vector<int> lo_row, hi_row;
  std::vector<double> g;
  std::vector<long long> u;
  if (int rc = quantile_ranks(ctx, "summary_sketch_quantiles", (int64_t)total, Q, probs, u, lo_row, hi_row, g)) return rc;
  HIPCHK(tu::sketch_quantiles((const unsigned long long *)counts, lo, width, D, (int)B, (int)Q, (int)u.size(), u.data(),
                              lo_row.data(), hi_row.data(), g.data(), estimate, resolved, (hipStream_t)stream));
  return 0;
}

// Constrained draws (constrain.cuh): x [R, D_in] into y [R, D_out] through the per-output table; out of place.
extern "C" int aehmc_constrain(aehmc_ctx *ctx, int64_t R, int64_t D_in, int64_t D_out, const double *x,
                               const aehmc_constrain_entry *table, double *y, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (R < 1 || D_in < 1 || D_out < 1 || !x || !table || !y) FAIL("constrain: bad arguments");
  if (D_in >= (int64_t)1 << 31 || D_out >= (int64_t)1 << 31) FAIL("constrain: D_in and D_out must be below 2^31");
  if (R > INT64_MAX / 8 / D_in || R > INT64_MAX / 8 / D_out) FAIL("constrain: R is too large");
  const uintptr_t xb = (uintptr_t)x, yb = (uintptr_t)y;
  const uintptr_t xe = xb + (uintptr_t)(R * D_in * 8), ye = yb + (uintptr_t)(R * D_out * 8);
  if (xb < ye && yb < xe) FAIL("constrain: x and y overlap; the map is out of place");
  HIPCHK(tu::constrain(x, R, D_in, D_out, table, y, (hipStream_t)stream));
  return 0;
}

// ------------------------------------------------------------------ pointwise programs and streaming WAIC (pointwise.cuh)
static std::string pw_kernel(bool fold, bool stage) {
  return std::string("aehmc::k_pointwise<") + (fold ? "true" : "false") + ", " + (stage ? "true" : "false") + ">";
}
// Binds a pointwise program (tracing.trace_pointwise) BESIDE the target: a transaction like aehmc_set_custom_target -- a
// failed compile leaves the previous pointwise binding in place -- that never touches the target's binding.
extern "C" int aehmc_set_pointwise(aehmc_ctx *ctx, const char *source, int64_t D, int64_t n_out, int32_t n_head,
                                   const double *const *params, int32_t n_params, const char *include_dir) {
  if (!ctx || !source || !include_dir) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (D < 1 || D > JOINT_WIDE_MAX_D) FAIL("pointwise: D must be in [1, " + std::to_string(JOINT_WIDE_MAX_D) + "]");
  if (n_out < 1 || (n_out + PW_TILE - 1) / PW_TILE > 65535) FAIL("pointwise: n_out must be in [1, " + std::to_string(65535LL * PW_TILE) + "]");
  if (n_head < 0) FAIL("pointwise: n_head must not be negative");
  const PwPlan plan = pw_plan(D, n_head);
  if (plan.batch < 1) FAIL("pointwise: " + std::to_string(n_head) + " head values per row do not fit in LDS");
  if (int rc = custom_bind(ctx, ctx->pw, custom_source(source, include_dir), params, n_params, RTC_PW, pw_kernel(false, plan.stage)))
    return rc;
  ctx->pw_D = D; ctx->pw_n_out = n_out; ctx->pw_n_head = n_head;
  return 0;
}
static int pw_launch(aehmc_ctx *ctx, bool fold, int64_t R, const double *x, double *out, hipStream_t st) {
  const PwPlan plan = pw_plan(ctx->pw_D, ctx->pw_n_head);
  PwArgs a{};
  a.x = x; a.out = out; a.prm = ctx->pw.d_cparams;
  a.R = R; a.D = ctx->pw_D; a.n_out = ctx->pw_n_out; a.n_head = ctx->pw_n_head; a.batch = plan.batch;
  const dim3 grid((unsigned)pw_parts(R), (unsigned)((ctx->pw_n_out + PW_TILE - 1) / PW_TILE));
  return rtc_launch_on(ctx, ctx->pw, RTC_PW, pw_kernel(fold, plan.stage), grid, dim3(PW_TILE), plan.lds, st, a);
}
static int pw_check_rows(aehmc_ctx *ctx, const char *what, int64_t R, int64_t width) {
  if (R < 1 || pw_parts(R) > 2147483647LL) FAIL(std::string(what) + ": R must be in [1, " + std::to_string(2147483647LL * PW_PART) + "]");
  if (R > INT64_MAX / 8 / width) FAIL(std::string(what) + ": R is too large");
  return 0;
}
extern "C" int aehmc_pointwise_eval(aehmc_ctx *ctx, int64_t R, const double *x, double *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->pw.src.empty()) FAIL("pointwise_eval: no pointwise program is bound (aehmc_set_pointwise)");
  if (!x || !out) FAIL("pointwise_eval: bad arguments");
  if (int rc = pw_check_rows(ctx, "pointwise_eval", R, std::max(ctx->pw_D, ctx->pw_n_out))) return rc;
  return pw_launch(ctx, false, R, x, out, (hipStream_t)stream);
}
static int waic_state_check(aehmc_ctx *ctx, const char *what, const double *state, int64_t n_state) {
  if (!state || n_state < 0) FAIL(std::string(what) + ": bad state");
  if (n_state >= (int64_t)1 << 53) FAIL(std::string(what) + ": the draw count must stay below 2^53");
  return 0;
}
extern "C" int aehmc_pointwise_waic_fold(aehmc_ctx *ctx, int64_t R, const double *x, double *state, int64_t n_state,
                                         void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (ctx->pw.src.empty()) FAIL("pointwise_waic_fold: no pointwise program is bound (aehmc_set_pointwise)");
  if (!x) FAIL("pointwise_waic_fold: bad arguments");
  if (int rc = waic_state_check(ctx, "pointwise_waic_fold", state, n_state)) return rc;
  if (int rc = pw_check_rows(ctx, "pointwise_waic_fold", R, std::max(ctx->pw_D, 4 * ctx->pw_n_out))) return rc;
  if (int rc = grow(ctx, &ctx->pw_work, &ctx->pw_work_bytes, pw_work_doubles(R, ctx->pw_n_out) * sizeof(double))) return rc;
  if (int rc = pw_launch(ctx, true, R, x, ctx->pw_work, (hipStream_t)stream)) return rc;
  HIPCHK(tu::waic_merge(ctx->pw_work, pw_parts(R), PW_PART, R, state, (double)n_state, ctx->pw_n_out, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_waic_fold(aehmc_ctx *ctx, int64_t R, int64_t n_obs, const double *x, double *state, int64_t n_state,
                               void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (!x || n_obs < 1 || (n_obs + PW_TILE - 1) / PW_TILE > 65535) FAIL("waic_fold: bad arguments (1 <= n_obs <= " + std::to_string(65535LL * PW_TILE) + ")");
  if (int rc = waic_state_check(ctx, "waic_fold", state, n_state)) return rc;
  if (int rc = pw_check_rows(ctx, "waic_fold", R, 4 * n_obs)) return rc;
  if (int rc = grow(ctx, &ctx->pw_work, &ctx->pw_work_bytes, pw_work_doubles(R, n_obs) * sizeof(double))) return rc;
  HIPCHK(tu::waic_fold_stored(x, R, n_obs, ctx->pw_work, (hipStream_t)stream));
  HIPCHK(tu::waic_merge(ctx->pw_work, pw_parts(R), PW_PART, R, state, (double)n_state, n_obs, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_waic_merge(aehmc_ctx *ctx, int64_t n_obs, double *state, int64_t n_state, const double *other,
                                int64_t n_other, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (n_obs < 1 || !other || n_other < 1 || other == state) FAIL("waic_merge: bad arguments");
  if (int rc = waic_state_check(ctx, "waic_merge", state, n_state)) return rc;
  if (n_other >= (int64_t)1 << 53) FAIL("waic_merge: the draw count must stay below 2^53");
  HIPCHK(tu::waic_merge(other, 1, n_other, n_other, state, (double)n_state, n_obs, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_waic_final(aehmc_ctx *ctx, int64_t n_obs, const double *state, int64_t n_state, double *lppd,
                                double *p, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (n_obs < 1 || !state || n_state < 1 || !lppd || !p) FAIL("waic_final: bad arguments (at least one draw)");
  HIPCHK(tu::waic_final(state, (double)n_state, n_obs, lppd, p, (hipStream_t)stream));
  return 0;
}

// Average ranks and normal scores of the stored draws (rank.cuh): the same conventions.  The scratch decides the tile:
// as many coordinates as it holds are sorted at a time, and the result does not depend on how many that is.
extern "C" int64_t aehmc_summary_rank_work(int64_t R, int64_t D) {
  if (R < 1 || D < 1 || R >= (int64_t)1 << 31 || D >= (int64_t)1 << 31) return 0;
  return (int64_t)tu::rank_work_bytes(R, tu::rank_default_tile(R, D));
}
extern "C" int aehmc_summary_rank(aehmc_ctx *ctx, int64_t R, int64_t D, const double *samples, const double *center,
                                  int mode, double *out, void *work, int64_t work_bytes, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (R < 1 || D < 1 || !samples || !out || !work) FAIL("summary_rank: bad arguments");
  if (mode != 0 && mode != 1) FAIL("summary_rank: mode must be 0 (ranks) or 1 (normal scores), got " + std::to_string(mode));
  if ((uintptr_t)work % 256) FAIL("summary_rank: work must be 256-byte aligned");
  if (R >= (int64_t)1 << 31) FAIL("summary_rank: the counts are 32-bit, R must be below 2^31");
  if (D >= (int64_t)1 << 31) FAIL("summary_rank: D is too large");
  const int64_t T = work_bytes > 0 ? tu::rank_tile_width(R, D, (size_t)work_bytes) : 0;
  if (T < 1)
    FAIL("summary_rank: work holds " + std::to_string(work_bytes) + " bytes, one coordinate needs " +
         std::to_string(tu::rank_work_bytes(R, 1)) + " (aehmc_summary_rank_work gives " +
         std::to_string(aehmc_summary_rank_work(R, D)) + ")");
  HIPCHK(tu::rank(samples, center, R, D, mode, out, work, T, (hipStream_t)stream));
  return 0;
}

// Highest-density intervals and the MCSE of quantiles (posterior.cuh): consumers of the same sorted columns, with the
// scratch, the tiles and the refusals of aehmc_summary_rank.  tile: the coordinates a tile holds, or the refusal.
static int posterior_shape(aehmc_ctx *ctx, const char *what, int64_t R, int64_t D, const void *work, int64_t work_bytes,
                           int64_t *tile) {
  if ((uintptr_t)work % 256) FAIL(std::string(what) + ": work must be 256-byte aligned");
  if (R >= (int64_t)1 << 31) FAIL(std::string(what) + ": the counts are 32-bit, R must be below 2^31");
  if (D >= (int64_t)1 << 31) FAIL(std::string(what) + ": D is too large");
  *tile = work_bytes > 0 ? tu::rank_tile_width(R, D, (size_t)work_bytes) : 0;
  if (*tile < 1)
    FAIL(std::string(what) + ": work holds " + std::to_string(work_bytes) + " bytes, one coordinate needs " +
         std::to_string(tu::rank_work_bytes(R, 1)) + " (aehmc_summary_rank_work gives " +
         std::to_string(aehmc_summary_rank_work(R, D)) + ")");
  return 0;
}
extern "C" int aehmc_summary_hdi(aehmc_ctx *ctx, int64_t R, int64_t D, const double *samples, double prob,
                                 double *lower, double *upper, int64_t *index, void *work, int64_t work_bytes,
                                 void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (R < 1 || D < 1 || !samples || !lower || !upper || !work) FAIL("summary_hdi: bad arguments");
  if (!(prob > 0.0 && prob <= 1.0)) FAIL("summary_hdi: prob must be within (0, 1], got " + std::to_string(prob));
  int64_t T = 0;
  if (int rc = posterior_shape(ctx, "summary_hdi", R, D, work, work_bytes, &T)) return rc;
  // the window in order statistics, numpy's floor(prob * n), held to R - 1 so that prob = 1 is (min, max)
  int64_t m = (int64_t)std::floor(prob * (double)R);
  if (m > R - 1) m = R - 1;
  static_assert(sizeof(long long) == sizeof(int64_t), "index is written as long long");
  HIPCHK(tu::hdi(samples, R, D, m, lower, upper, (long long *)index, work, T, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_summary_quantile_mcse(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t Q, const double *samples,
                                           const double *probs, const double *ess, double *out, int64_t *ranks,
                                           void *work, int64_t work_bytes, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (R < 1 || D < 1 || Q < 1 || !samples || !probs || !ess || !out || !work)
    FAIL("summary_quantile_mcse: bad arguments");
  if (Q > AEHMC_SUMMARY_QUANTILE_MAX)
    FAIL("summary_quantile_mcse: at most " + std::to_string(AEHMC_SUMMARY_QUANTILE_MAX) + " probabilities a call");
  for (int64_t i = 0; i < Q; ++i)
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
      FAIL("summary_quantile_mcse: probability " + std::to_string(probs[i]) + " is outside [0, 1]");
  int64_t T = 0;
  if (int rc = posterior_shape(ctx, "summary_quantile_mcse", R, D, work, work_bytes, &T)) return rc;
  HIPCHK(tu::quantile_mcse(samples, R, D, (int)Q, probs, ess, out, (long long *)ranks, work, T, (hipStream_t)stream));
  return 0;
}
// Pareto-smoothed importance sampling (psis.cuh): one more consumer of the sorted columns.  Without log_ratios the
// ratios are -log_values, the leave-one-out case: no negated copy of the log-likelihood has to exist.
extern "C" int aehmc_summary_psis(aehmc_ctx *ctx, int64_t R, int64_t D, const double *log_ratios, const double *reff,
                                  const double *log_values, double *log_weights, double *pareto_k, int64_t *tail_len,
                                  double *log_mean, void *work, int64_t work_bytes, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (R < 1 || D < 1 || (!log_ratios && !log_values) || !pareto_k || !work) FAIL("summary_psis: bad arguments");
  if ((log_values != nullptr) != (log_mean != nullptr))
    FAIL("summary_psis: log_values and log_mean go together, one of them is null");
  int64_t T = 0;
  if (int rc = posterior_shape(ctx, "summary_psis", R, D, work, work_bytes, &T)) return rc;
  const bool neg = !log_ratios;
  HIPCHK(tu::psis(neg ? log_values : log_ratios, neg, reff, log_values, log_weights, pareto_k, (long long *)tail_len,
                  log_mean, R, D, work, T, (hipStream_t)stream));
  return 0;
}
extern "C" int aehmc_beta_quantile(aehmc_ctx *ctx, int64_t n, const double *p, const double *a, const double *b,
                                   double *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (n < 1 || !p || !a || !b || !out) FAIL("beta_quantile: bad arguments");
  if (n >= (int64_t)1 << 37) FAIL("beta_quantile: n is too large");
  HIPCHK(tu::beta_quantile(n, p, a, b, out, (hipStream_t)stream));
  return 0;
}

extern "C" int aehmc_set_option(aehmc_ctx *ctx, const char *name, int64_t value) {
  if (!ctx || !name) return -2;
  if (!strcmp(name, "fused_hmc")) {
    ctx->opt_fused_hmc = value != 0;
    return 0;
  }
  if (!strcmp(name, "resident_min_team")) {
    ctx->opt_resident_min_team = value != 0;
    return 0;
  }
  if (!strcmp(name, "resident_nuts")) {
    ctx->opt_resident_nuts = (int)value;
    return 0;
  }
  if (!strcmp(name, "fused_nuts")) {
    ctx->opt_fused_nuts = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_linear")) {
    if (ctx->opt_dense_linear != (value != 0)) carry_drop(ctx);
    ctx->opt_dense_linear = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_whiten")) {
    if (ctx->opt_dense_whiten != (value != 0)) carry_drop(ctx);
    ctx->opt_dense_whiten = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_whiten_carry")) {
    if (ctx->opt_dense_whiten_carry != (value != 0)) carry_drop(ctx);
    ctx->opt_dense_whiten_carry = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_whiten_ahead")) {
    if (ctx->opt_dense_whiten_ahead != (value != 0)) carry_drop(ctx);
    ctx->opt_dense_whiten_ahead = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_eigen")) {
    if (value < 0 || value > 2) FAIL("dense_eigen: 0 (off), 1 (default: D >= 2048), 2 (wherever the whitened mode applies)");
    if (ctx->opt_dense_eigen != (int)value) carry_drop(ctx);
    ctx->opt_dense_eigen = (int)value;
    return 0;
  }
  if (!strcmp(name, "dense_eigen_wide")) {
    if (ctx->opt_dense_eigen_wide != (value != 0)) carry_drop(ctx);
    ctx->opt_dense_eigen_wide = value != 0;
    return 0;
  }
  if (!strcmp(name, "dense_eigen_solver")) {
    if (ctx->opt_eigen_solver != (value != 0)) {
      carry_drop(ctx);
      eigen_release(ctx, false);
      eigen_free_keep(ctx);
    }
    ctx->opt_eigen_solver = value != 0;
    return 0;
  }
  if (!strcmp(name, "gemm_small_tiles")) {
    ctx->opt_gemm_small = (int)value;
    return 0;
  }
  if (!strcmp(name, "streamk")) {
    ctx->opt_streamk = (int)value;
    return 0;
  }
  if (!strcmp(name, "compact")) {
    ctx->opt_compact = value != 0;
    return 0;
  }
  if (!strcmp(name, "block_dense")) {
    ctx->opt_block_dense = (int)value;
    return 0;
  }
  if (!strcmp(name, "pc_dense")) {
    ctx->opt_pc_dense = value != 0;
    return 0;
  }
  if (!strcmp(name, "block_roll")) {
    if (value < 0 || value > 16) FAIL("block_roll: 0 (default) ... 16");
    ctx->opt_block_roll = (int)value;
    return 0;
  }
  if (!strcmp(name, "fp_contract")) {
    ctx->opt_fp_contract = value != 0;
    return 0;
  }
  if (!strcmp(name, "joint_resident")) {
    ctx->opt_joint_resident = (int)value;
    return 0;
  }
  if (!strcmp(name, "joint_wide")) {
    if (value < 0 || value > 2) FAIL("joint_wide: 0 (never), 1 (default: above 2048 coordinates), 2 (also from 513 on)");
    ctx->opt_joint_wide = (int)value;
    return 0;
  }
  if (!strcmp(name, "joint_wg")) {
    if (value < 0 || value > 2) FAIL("joint_wg: 0 (never), 1 (default: when it pays), 2 (always)");
    ctx->opt_joint_wg = (int)value;
    return 0;
  }
  if (!strcmp(name, "wg_waves")) {
    if (value != 0 && value != 3 && value != 4) FAIL("wg_waves: 0 (default: four unless the program spills), 3, 4");
    ctx->opt_wg_waves = (int)value;
    return 0;
  }
  FAIL(std::string("unknown option ") + name);
}

extern "C" int aehmc_set_white_basis(aehmc_ctx *ctx, int64_t D, const double *V, const double *lam, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if ((V == nullptr) != (lam == nullptr)) FAIL("set_white_basis: V and lam go together");
  if (V && D < 1) FAIL("set_white_basis: D must be positive");
  auto &e = ctx->eig;
  carry_drop(ctx);
  eigen_release(ctx, false);
  eigen_free_keep(ctx);
  for (double **p : {&e.sup_V, &e.sup_lam}) {
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
  }
  e.sup_D = 0;
  e.state = 0;
  if (!V) return 0;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMalloc((void **)&e.sup_V, (size_t)D * D * sizeof(double)));
  HIPCHK(hipMalloc((void **)&e.sup_lam, D * sizeof(double)));
  e.sup_D = D;
  HIPCHK(hipMemcpyAsync(e.sup_V, V, (size_t)D * D * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(e.sup_lam, lam, D * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
extern "C" int aehmc_white_basis_info(aehmc_ctx *ctx, int32_t *state, double *orth, double *resid, double *solver_ms) {
  if (!ctx) return -2;
  if (state) *state = ctx->eig.state;
  if (orth) *orth = ctx->eig.orth;
  if (resid) *resid = ctx->eig.resid;
  if (solver_ms) *solver_ms = ctx->eig.solver_ms;
  return 0;
}

// ------------------------------------------------------------------ workspace ------
static int64_t ws_layout(const aehmc_ctx *ctx, int64_t C, int64_t E, char *base, EngineArgs *a) {
  const bool md = ctx->has_met && ctx->met.ndim == 2;
  const int64_t D = ctx->has_tgt ? ctx->tgt.D : (ctx->has_met ? ctx->met.D : 0);
  // (rows padded to nuts_wide_ld(D) where the workgroup-per-chain NUTS kernel may run: D > 512)
  const int64_t ldmax = wide_rows_padded(D) ? nuts_wide_ld(D) : D;
  const size_t vec = (((size_t)C * ldmax * sizeof(double)) + 255) & ~(size_t)255;
  size_t off = 0;
  auto take = [&](size_t n) -> double * {
    double *p = base ? reinterpret_cast<double *>(base + off) : nullptr;
    off += n;
    return p;
  };
  EngineArgs tmp{};
  EngineArgs &r = a ? *a : tmp;
  r.cur_q = take(vec); r.cur_p = take(vec); r.cur_g = take(vec);
  for (int e = 0; e < 2; e++) { r.end_q[e] = take(vec); r.end_p[e] = take(vec); r.end_g[e] = take(vec); }
  for (int s = 0; s < 2; s++) { r.slot_q[s] = take(vec); r.slot_p[s] = take(vec); r.slot_g[s] = take(vec); }
  r.psum = take(vec); r.psub = take(vec);
  r.ckp = take(vec * E); r.cks = take(vec * E);
  r.vhalf = take(vec); r.rbuf = take(vec); r.zbuf = take(vec);
  if (md) {
    r.cur_v = take(vec);
    r.end_v[0] = take(vec); r.end_v[1] = take(vec);
    r.ckv = take(vec * E);
    r.cur_w = take(vec);
    r.end_w[0] = take(vec); r.end_w[1] = take(vec);
  }
  r.linreg_part = take((((size_t)(C + LINREG_CPB - 1) / LINREG_CPB) * LINREG_SMAX * 2 * LINREG_CPB * sizeof(double) + 255) & ~(size_t)255);
  r.row_idx = reinterpret_cast<int *>(take(((size_t)C * sizeof(int) + 255) & ~(size_t)255));
  r.n_rows = reinterpret_cast<int *>(take(256));
  r.ctl = reinterpret_cast<ChainCtl *>(take(((size_t)C * sizeof(ChainCtl) + 255) & ~(size_t)255));
  return (int64_t)off;
}

extern "C" int64_t aehmc_workspace_bytes(const aehmc_ctx *ctx, int64_t C, int64_t max_num_expansions) {
  if (!ctx || !ctx->has_tgt || !ctx->has_met) return -2;
  if (max_num_expansions < 1) max_num_expansions = 1;
  return ws_layout(ctx, C, max_num_expansions, nullptr, nullptr);
}
extern "C" int aehmc_set_workspace(aehmc_ctx *ctx, void *ws, int64_t bytes) {
  if (!ctx) return -2;
  if (((uintptr_t)ws) % 256 != 0) FAIL("workspace must be 256-byte aligned");
  ctx->ws = ws;
  ctx->ws_bytes = bytes;
  carry_drop(ctx);
  return 0;
}

// per-chain parameters are indexed [c] for c < C: a different length would read out of bounds
static int check_per_chain(aehmc_ctx *ctx, int64_t C) {
  if (ctx->eps_c && ctx->eps_n != C)
    FAIL("per-chain step sizes have " + std::to_string(ctx->eps_n) + " entries, the call has " +
         std::to_string(C) + " chains");
  if (ctx->has_met && ctx->met.per_chain && ctx->met.n_chains != C)
    FAIL("per-chain inverse mass matrix has " + std::to_string(ctx->met.n_chains) + " rows, the call has " +
         std::to_string(C) + " chains");
  return 0;
}
// Every caller may write the workspace's vectors, so the whitened carry record is dropped here; nuts_run and hmc_run
// (`keep_carry`) decide for themselves once they know their route.
static int fill_args(aehmc_ctx *ctx, int64_t C, int64_t E, EngineArgs &a, bool uses_params = true, bool keep_carry = false) {
  if (!keep_carry) carry_drop(ctx);
  if (!ctx->has_tgt || !ctx->has_met) FAIL("set_target and set_metric must be called first");
  if (ctx->tgt.D != ctx->met.D) FAIL("target and metric dimensions differ");
  if (C <= 0) FAIL("C must be positive");
  if (uses_params)  // (new_state evaluates the target only: stale per-chain parameters are not read)
    if (int rc = check_per_chain(ctx, C)) return rc;
  memset(&a, 0, sizeof(a));
  int64_t need = ws_layout(ctx, C, E, (char *)ctx->ws, &a);
  if (!ctx->ws || need > ctx->ws_bytes)
    FAIL("workspace too small: need " + std::to_string(need) + " bytes");
  a.C = C;
  a.D = ctx->tgt.D;
  a.ldw = a.D;
  a.max_exp = (int)E;
  a.met_ndim = ctx->met.ndim;
  a.imm = ctx->met.imm;
  a.sqrt_mass = ctx->met.sqrt_mass;
  a.imm_cs = ctx->met.per_chain ? (ctx->met.ndim == 0 ? 1 : ctx->met.D) : 0;
  a.eps_c = ctx->eps_c;
  a.tkind = ctx->tgt.kind;
  a.mu = ctx->tgt.mu;
  a.sigma = ctx->tgt.sigma;
  a.log_sigma = ctx->log_sigma;
  a.X = ctx->tgt.X; a.y = ctx->tgt.y; a.N = ctx->tgt.N;
  a.cparams = ctx->bound.d_cparams;
  a.linear = (a.met_ndim == 2 && ctx->opt_dense_linear) ? 1 : 0;
  return 0;
}

// ------------------------------------------------------------------ GEMM + profiling
// HIP-event pairs around the dominant kernel's launches.  When the pool is used up the finished
// pairs are folded into the totals and the pool is reused, so long runs are covered completely.
static int prof_drain(aehmc_ctx *ctx) {
  for (size_t i = 0; i + 1 < ctx->prof_used; i += 2) {
    HIPCHK(hipEventSynchronize(ctx->prof_ev[i + 1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->prof_ev[i], ctx->prof_ev[i + 1]));
    ctx->prof_ms += ms;
    ctx->prof_n += 1;
  }
  ctx->prof_used = 0;
  return 0;
}
// `launch` (a callable: int(bool profiled), 0 on success) between the two events of a pair.  When it fails its error
// is returned at once: the end event is not recorded and the pair is not counted.
template <class Launch>
static int profiled(aehmc_ctx *ctx, hipStream_t st, Launch launch) {
  const bool on = ctx->prof && !ctx->prof_ev.empty();
  if (on) {
    if (ctx->prof_used + 2 > ctx->prof_ev.size())
      if (int rc = prof_drain(ctx)) return rc;
    HIPCHK(hipEventRecord(ctx->prof_ev[ctx->prof_used], st));
  }
  if (int rc = launch(on)) return rc;
  if (on) {
    HIPCHK(hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], st));
    ctx->prof_used += 2;
  }
  return 0;
}
// A stream-K hand-off that timed out leaves garbage partial sums: every entry point that waits
// for the device (lagging poll, profile_read, aehmc_synchronize) and every GEMM launch reports it.
static int check_device_errors(aehmc_ctx *ctx) {
  if (ctx->h_err && ctx->h_err[0]) {
    // reported once: the ctx stays usable (e.g. after set_option("streamk", 0)); the lock-step loop's
    // per-call state is reset because the call that saw the failure returns from the middle of it
    ctx->h_err[0] = 0;
    ctx->rows_hint = 0;
    carry_drop(ctx);
    ctx->fuse_pre = ctx->pre_done = false;
    FAIL("stream-K GEMM: a workgroup hand-off timed out (results invalid)");
  }
  return 0;
}
extern "C" int aehmc_synchronize(aehmc_ctx *ctx, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return check_device_errors(ctx);
}
static int gemm(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                const double *B, int64_t ldb, double *Cm, int64_t ldc, hipStream_t st,
                const int *row_idx, const int *n_rows, int mode, int tri, bool carry_in, bool in_place) {
  // tri: triangular hint for B (gemm_f64.cuh).  carry_in: one of white_begin's two input products on the rows that
  // could not be carried -- often none, so it is kept out of the timed launch pairs (its flops are still counted), and
  // its rows are not bounded by rows_hint, which belongs to the lock-step loop
  auto launch = [&](bool p) -> int {
    if (int rc = check_device_errors(ctx)) return rc;
    GemmStreamK sk{ctx->sk_partial, ctx->sk_flags, ctx->d_err, ++ctx->sk_epoch};
    const bool use_sk = ctx->opt_streamk && ctx->sk_grid > 0;
    // the kernels read the exact row count on the device; the host only picks the kernel and the
    // grid, from an upper bound: live chains never increase within a transition, so the count seen
    // at the last poll bounds every later launch (few rows left: smaller tiles, no persistent grid)
    if (!carry_in && n_rows && ctx->rows_hint > 0 && ctx->rows_hint < M) M = ctx->rows_hint;
    HIPCHK(tu::gemm_nt_f64(M, N, K, A, lda, B, ldb, Cm, ldc, st, row_idx, n_rows,
                           p ? ctx->d_flops : nullptr, (use_sk && mode == 0) ? &sk : nullptr, ctx->sk_grid,
                           mode, ctx->opt_streamk == 2 ? ctx->sk_grid_wide : 0, ctx->opt_gemm_small, tri, in_place));
    return 0;
  };
  if (carry_in) return launch(ctx->prof && !ctx->prof_ev.empty());
  return profiled(ctx, st, launch);
}

// X [C,D] times the metric matrix `mat` (imm or sqrt_mass): one GEMM over all chains when the
// matrix is shared, per-chain mat-vecs when every chain has its own (is_mass_matrix_full)
static int metric_mul(aehmc_ctx *ctx, int64_t C, const double *X, const double *mat, double *out,
                      hipStream_t st, const int *row_idx = nullptr, const int *n_rows = nullptr, int tri = 0) {
  const int64_t D = ctx->met.D;
  if (ctx->met.per_chain) {
    if (D <= AEHMC_PC_LDS_MAX_D)
      hipLaunchKernelGGL(k_matvec_pc, chain_grid(C), dim3(256), 0, st, mat, X, out, (long long)C, (long long)D,
                         row_idx, n_rows);
    else
      hipLaunchKernelGGL(k_matvec_pc_rows, dim3((unsigned)(((D + 63) / 64) * C)), dim3(256), 0, st, mat, X,
                         out, (long long)C, (long long)D, row_idx, n_rows);
    HIPCHK(hipGetLastError());
    return 0;
  }
  return gemm(ctx, C, D, D, X, D, mat, D, out, D, st, row_idx, n_rows, 0, tri);
}

extern "C" int aehmc_profile_enable(aehmc_ctx *ctx, int enable) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (enable && ctx->prof_ev.empty()) {
    ctx->prof_ev.resize(PROF_POOL);
    for (auto &e : ctx->prof_ev) HIPCHK(hipEventCreate(&e));
  }
  ctx->prof = enable != 0;
  ctx->prof_used = 0;
  ctx->prof_ms = 0.0;
  ctx->prof_n = 0;
  ctx->prof_flops = 0.0;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(ctx->d_flops, 0, sizeof(unsigned long long)));
  return 0;
}
extern "C" int aehmc_profile_read(aehmc_ctx *ctx, double *ms_total, int64_t *launches,
                                  double *flops_total) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = prof_drain(ctx)) return rc;
  unsigned long long fl = 0;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&fl, ctx->d_flops, sizeof(fl), hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(ctx->d_flops, 0, sizeof(unsigned long long)));
  ctx->prof_flops += (double)fl;
  if (ms_total) *ms_total = ctx->prof_ms;
  if (launches) *launches = ctx->prof_n;
  if (flops_total) *flops_total = ctx->prof_flops;
  return check_device_errors(ctx);
}

extern "C" int aehmc_gemm_nt(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A,
                             int64_t lda, const double *B, int64_t ldb, double *Cm, int64_t ldc,
                             void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  return gemm(ctx, M, N, K, A, lda, B, ldb, Cm, ldc, (hipStream_t)stream);
}
extern "C" int aehmc_gemm_nt_tri(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                                 const double *B, int64_t ldb, double *Cm, int64_t ldc, int32_t tri,
                                 const int32_t *row_idx, const int32_t *n_rows, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (tri < 0 || tri > 2) FAIL("gemm_nt_tri: tri is 0 (none), 1 (B lower triangular) or 2 (B upper triangular)");
  if ((row_idx == nullptr) != (n_rows == nullptr)) FAIL("gemm_nt_tri: row_idx and n_rows go together");
  return gemm(ctx, M, N, K, A, lda, B, ldb, Cm, ldc, (hipStream_t)stream, row_idx, n_rows, 0, tri);
}

// user-defined row-reduction target at the positions q [C,D]: Z = Q X^T (GEMM) -> dloss/dz in place + the loss sums
// (run-time compiled) -> G = dLoss X (GEMM) -> + the prior's terms, U (run-time compiled)
static int launch_glm(aehmc_ctx *ctx, const EngineArgs &a, const double *q, double *g, double *U, int to_ctl,
                      hipStream_t st, const int *ri, const int *nr) {
  const int64_t C = a.C, D = a.D, N = ctx->glm_N;
  if (int rc = grow(ctx, &ctx->glm_z, &ctx->glm_z_bytes, (size_t)C * N * sizeof(double))) return rc;
  if (int rc = grow(ctx, &ctx->glm_lsum, &ctx->glm_lsum_bytes, (size_t)C * sizeof(double))) return rc;
  if (int rc = gemm(ctx, C, N, D, q, D, ctx->glm_X, D, ctx->glm_z, N, st, ri, nr)) return rc;
  if (int rc = rtc_launch(ctx, RTC_GLM, "aehmc::k_glm_rows", chain_grid(C), dim3(256), 0, st, (long long)C,
                          (long long)N, ctx->glm_y, (const double *const *)ctx->bound.d_cparams, ctx->glm_z, ctx->glm_lsum, ri, nr))
    return rc;
  if (int rc = gemm(ctx, C, D, N, ctx->glm_z, N, ctx->glm_XT, N, g, D, st, ri, nr)) return rc;
  return rtc_launch(ctx, RTC_GLM, "aehmc::k_glm_finish", chain_grid(C), dim3(256), 0, st, a, q, g, U,
                    (const double *)ctx->glm_lsum, to_ctl);
}

// ------------------------------------------------------------------ leapfrog driver
#define LAUNCH(kern, C, st, ...)                                                      \
  do {                                                                                \
    hipLaunchKernelGGL(kern, chain_grid(C), dim3(256), 0, st, __VA_ARGS__);           \
    HIPCHK(hipGetLastError());                                                        \
  } while (0)

// joint user-defined target on the lock-step path: U and dU/dq of the (live) chains from their position rows
static int launch_joint_rows(aehmc_ctx *ctx, const EngineArgs &a, const double *q, double *g, double *U, int to_ctl,
                             hipStream_t st, const int *ri, const int *nr) {
  if (a.D > JOINT_ROWS_MAX_D)  // a workgroup per chain (k_target_joint_wg)
    return joint_rows_launch(ctx, RTC_JTWG, "aehmc::k_target_joint_wg<8>", a.D, dim3((unsigned)a.C), dim3(512), st, a, q, g, U, to_ctl, ri, nr);
  return rtc_launch(ctx, RTC_JBASE, "aehmc::k_target_joint_rows", chain_grid(a.C), dim3(256), (size_t)8 * a.D * sizeof(double), st, a, q, g, U,
                    to_ctl, ri, nr);
}

// kernels that evaluate a coordinate-wise target: the library's own instantiation, or -- user-defined target -- the
// run-time compiled one of the same name
// (the kernel token as it is written is the name hipRTC is asked for: RTC_BASE's list holds every one written below)
#define LAUNCH_T(C, st, a, ...)                                                                         \
  do {                                                                                                  \
    if (ctx->tgt.kind == AEHMC_T_CUSTOM) {                                                              \
      if (int rc_ = rtc_launch(ctx, RTC_BASE, "aehmc::" #__VA_ARGS__, chain_grid(C), dim3(256), 0, st, a)) return rc_; \
    } else {                                                                                            \
      LAUNCH((__VA_ARGS__), C, st, a);                                                                  \
    }                                                                                                   \
  } while (0)

// ---- whitened dense MVN ("dense_whiten").  NUTS and HMC are equivariant under q = mu + L z, p = L^-T r
// with imm = L L^T: in (z, r) the target is a Gaussian of precision H = L^T P L, the metric the identity, the kinetic
// energy r.r / 2, and the momentum draw r = the raw normals.  A leapfrog then needs ONE chain-batched product (H z')
// instead of two (P q', imm g').  Every transition maps in and out on its own.
static bool white_wanted(const aehmc_ctx *ctx, const EngineArgs &a) {
  return ctx->opt_dense_whiten && a.linear && a.tkind == AEHMC_T_DENSE_MVN && a.met_ndim == 2 && !ctx->met.per_chain &&
         a.D > 512;
}
// L from a Cholesky of imm (the factor whose L^-T the bound sqrt_mass is: metrics.py:56-58), L^-1 = sqrt_mass^T, and
// H = (L^T P) L by two GEMMs, symmetrised.  Once per (target, metric) binding, from the bound arrays, on the stream of
// the first call that needs it.  (Not a factorisation of the caller's metric: aehmc_metric_sqrt is that.)
static int white_prepare(aehmc_ctx *ctx, hipStream_t st) {
  if (ctx->wh_ready) return 0;
  white_release(ctx, true);  // (a pending carry record waits for the operator formed here)
  const int64_t D = ctx->tgt.D;
  if (ctx->carry.pending && ctx->carry.D != D) carry_drop(ctx);  // (the old operator is of another size)
  const size_t mb = (size_t)D * D * sizeof(double);
  const int NB = FACT_NB;
  double *Lw = nullptr, *Lt = nullptr, *M = nullptr, *small = nullptr;
  int *info = nullptr;
  const bool prof = ctx->prof;  // (the formation's GEMMs are not the profiled workload's)
  auto done = [&](int r) {
    (void)hipFree(Lw); (void)hipFree(Lt); (void)hipFree(M); (void)hipFree(small); (void)hipFree(info);
    ctx->prof = prof;
    if (r) white_release(ctx);
    return r;
  };
  if (hipMalloc((void **)&ctx->wh_L, mb) != hipSuccess || hipMalloc((void **)&ctx->wh_Linv, mb) != hipSuccess ||
      hipMalloc((void **)&ctx->wh_H, mb) != hipSuccess || hipMalloc((void **)&ctx->wh_zero, D * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&ctx->wh_mu, D * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&ctx->wh_one, sizeof(double)) != hipSuccess || hipMalloc((void **)&Lw, mb) != hipSuccess ||
      hipMalloc((void **)&Lt, mb) != hipSuccess || hipMalloc((void **)&M, mb) != hipSuccess ||
      hipMalloc((void **)&small, (size_t)2 * NB * NB * sizeof(double)) != hipSuccess ||
      hipMalloc((void **)&info, 3 * sizeof(int)) != hipSuccess) {  // [0] failed pivot, [1] sqrt_mass is not triangular, [2] the operator differs from the pending record's
    ctx->err = "whitened dense MVN: device allocation failed";
    return done(-1);
  }
  static const double one = 1.0;
  if (hipMemcpyAsync(Lw, ctx->met.imm, mb, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemsetAsync(info, 0, 3 * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(ctx->wh_zero, 0, D * sizeof(double), st) != hipSuccess ||
      hipMemcpyAsync(ctx->wh_mu, ctx->tgt.mu, D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(ctx->wh_one, &one, sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) {
    ctx->err = "whitened dense MVN: device copy failed";
    return done(-1);
  }
  ctx->prof = false;
  int rc = dense_cholesky(ctx, Lw, D, small, small + NB * NB, info, st);
  const dim3 grid((unsigned)((D + 31) / 32), (unsigned)((D + 31) / 32));
  if (!rc) {
    hipLaunchKernelGGL(k_tril_pair, grid, dim3(32, 32), 0, st, (const double *)Lw, ctx->wh_L, Lt, (long long)D);
    hipLaunchKernelGGL(k_transpose, grid, dim3(32, 8), 0, st, ctx->met.sqrt_mass, ctx->wh_Linv, (long long)D);
    // sqrt_mass may be the caller's: its products, and those of its transpose L^-1, take the triangular hint only
    // when its lower triangle is all-zero bits (L's upper one is: k_tril_pair writes it)
    hipLaunchKernelGGL(k_check_upper, grid, dim3(32, 32), 0, st, ctx->met.sqrt_mass, (long long)D, info + 1);
    rc = gemm(ctx, D, D, D, Lt, D, ctx->tgt.prec, D, M, D, st);   // M = L^T P   (P symmetric: its rows are its columns)
  }
  if (!rc) rc = gemm(ctx, D, D, D, M, D, Lt, D, Lw, D, st);      // M L (the rows of L^T are the columns of L)
  if (!rc) {
    hipLaunchKernelGGL(k_symmetrize, grid, dim3(32, 32), 0, st, (const double *)Lw, ctx->wh_H, (long long)D);
    if (ctx->carry.pending) {
      const unsigned nb = (unsigned)(((size_t)D * D + 255) / 256);
      hipLaunchKernelGGL(k_bits_differ, dim3(nb), dim3(256), 0, st, (const double *)ctx->wh_L, (const double *)ctx->carry.old_L, (long long)(D * D), info + 2);
      hipLaunchKernelGGL(k_bits_differ, dim3(nb), dim3(256), 0, st, (const double *)ctx->wh_Linv, (const double *)ctx->carry.old_Linv, (long long)(D * D), info + 2);
      hipLaunchKernelGGL(k_bits_differ, dim3(nb), dim3(256), 0, st, (const double *)ctx->wh_H, (const double *)ctx->carry.old_H, (long long)(D * D), info + 2);
      hipLaunchKernelGGL(k_bits_differ, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, (const double *)ctx->wh_mu, (const double *)ctx->carry.old_mu, (long long)D, info + 2);
    }
    int h_info[3] = {0, 0, 0};
    if (hipMemcpyAsync(h_info, info, 3 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
      ctx->err = "whitened dense MVN: kernels failed";
      rc = -1;
    } else if (h_info[0]) {
      ctx->err = "dense inverse mass matrix is not positive definite (pivot " + std::to_string(h_info[0]) + ")";
      rc = -2;
    }
    ctx->wh_tri = !rc && h_info[1] == 0;
    if (ctx->carry.pending) {  // the record counts again only under the operator it was made with
      const bool same = !rc && h_info[2] == 0;
      carry_drop(ctx);
      ctx->carry.valid = same;
    }
  }
  if (!rc) ctx->wh_ready = true;
  return done(rc);
}

// ---- eigen route of the whitened mode ("dense_eigen").  H is one matrix for the life of a binding: with
// H = V diag(lam) V^T and y = V^T z, s = V^T r the whitened problem is a coordinate-wise Gaussian of precisions lam_i
// under the identity metric, and NUTS is equivariant under the rotation (kinetic energy, U and every U-turn dot product
// are unchanged; s is the raw normals, rotated).  The leapfrogs then need no product at all.
constexpr int64_t EIGEN_MIN_D = 2048;  // "dense_eigen" 1: below, the recorded byte-exact cases keep the route they were recorded with
// Acceptance bounds of a basis (white_basis): ten times the larger of what LAPACK's dsyevd leaves for the operators of
// tests/test_gpu_dense_eigen.py (D = 513, 700, both spectra: max |V^T V - I| 3.4e-15, residual 2.4e-15) and what
// rocsolver_dsyevd leaves for the benchmark's operator at D = 10^4 (4.6e-15, 1.9e-15) -- DESIGN §3 has the table
constexpr double EIGEN_ORTH_MAX = 4.6e-14, EIGEN_RESID_MAX = 2.4e-14;
static bool eigen_wanted(const aehmc_ctx *ctx, int64_t D) {
  return ctx->opt_dense_eigen == 2 || (ctx->opt_dense_eigen == 1 && D >= EIGEN_MIN_D);
}
// rocsolver_dsyevd and the three rocblas handle calls it needs, looked up once per process.  A process that already holds
// the libraries (PyTorch loads its own) gets those; otherwise the loader's search path decides.
struct EigenSolver {
  int (*create)(void **) = nullptr;
  int (*destroy)(void *) = nullptr;
  int (*set_stream)(void *, hipStream_t) = nullptr;
  int (*dsyevd)(void *, int, int, int, double *, int, double *, double *, int *) = nullptr;
  bool ok = false;
};
static const EigenSolver &eigen_solver() {
  static const EigenSolver api = [] {
    EigenSolver s;
    void *h = nullptr;
    for (const char *name : {"librocsolver.so.0", "librocsolver.so"}) {
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    }
    for (const char *name : {"librocsolver.so.0", "librocsolver.so"}) {
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    }
    if (!h) return s;
    s.create = (decltype(s.create))dlsym(h, "rocblas_create_handle");
    s.destroy = (decltype(s.destroy))dlsym(h, "rocblas_destroy_handle");
    s.set_stream = (decltype(s.set_stream))dlsym(h, "rocblas_set_stream");
    s.dsyevd = (decltype(s.dsyevd))dlsym(h, "rocsolver_dsyevd");
    s.ok = s.create && s.destroy && s.set_stream && s.dsyevd;
    return s;
  }();
  return api;
}
// V^T (the columns of the solver's column-major output are the eigenvectors: read row-major it IS V^T) and lam of the
// symmetric H, in place in `Vt`.  Returns the state: 1, or -1 / -2 (aehmc_white_basis_info)
static int eigen_solve(aehmc_ctx *ctx, double *Vt, double *lam, int64_t D, hipStream_t st) {
  const EigenSolver &api = eigen_solver();
  if (!ctx->opt_eigen_solver || !api.ok || D > INT32_MAX) return -1;
  double *E = nullptr;
  int *info = nullptr;
  void *handle = nullptr;
  int state = -2, h_info = -1;
  const auto t0 = std::chrono::steady_clock::now();
  if (hipMalloc((void **)&E, D * sizeof(double)) == hipSuccess && hipMalloc((void **)&info, sizeof(int)) == hipSuccess &&
      api.create(&handle) == 0 && api.set_stream(handle, st) == 0 &&
      api.dsyevd(handle, /*rocblas_evect_original*/ 211, /*rocblas_fill_lower*/ 122, (int)D, Vt, (int)D, lam, E, info) == 0 &&
      hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
      hipStreamSynchronize(st) == hipSuccess && h_info == 0)
    state = 1;
  (void)hipGetLastError();
  ctx->eig.solver_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (handle) (void)api.destroy(handle);
  (void)hipFree(E); (void)hipFree(info);
  return state;
}
// The basis of the bound operator (white_prepare has run), once per operator: the caller's (aehmc_set_white_basis), the
// one kept across a re-binding if H has its bits, or the solver's; checked on the device; then the three transforms by
// the project's GEMM.  Whatever goes wrong leaves the whitened route: eig.ready says whether the eigen route may run.
static int white_basis(aehmc_ctx *ctx, hipStream_t st) {
  auto &e = ctx->eig;
  if (e.tried) return 0;
  e.tried = true;
  e.ready = false;
  const double kept_orth = e.orth, kept_resid = e.resid, kept_ms = e.solver_ms;  // (of the basis kept aside, if one is)
  e.orth = e.resid = -1.0;
  e.solver_ms = 0.0;
  const int64_t D = ctx->tgt.D;
  const size_t mb = (size_t)D * D * sizeof(double);
  double *G = nullptr, *R = nullptr;
  unsigned long long *chk = nullptr;  // [0..2] k_basis_check, [3] (as int) k_bits_differ
  const bool prof = ctx->prof;  // (the formation's GEMMs are not the profiled workload's)
  auto done = [&](int state) {
    (void)hipFree(G); (void)hipFree(R); (void)hipFree(chk);
    (void)hipGetLastError();
    ctx->prof = prof;
    eigen_free_keep(ctx);
    e.state = state;
    if (state > 0) {
      e.ready = true;
      e.D = D;
    } else {
      for (double **p : {&e.Vt, &e.lam, &e.Tin, &e.Tout, &e.Tp}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
      }
    }
    return 0;
  };
  if (hipMalloc((void **)&chk, 4 * sizeof(unsigned long long)) != hipSuccess ||
      hipMemsetAsync(chk, 0, 4 * sizeof(unsigned long long), st) != hipSuccess)
    return done(-4);
  int state = 0;
  const dim3 tgrid((unsigned)((D + 31) / 32), (unsigned)((D + 31) / 32));
  if (e.sup_V) {
    if (e.sup_D != D) return done(-3);
    if (hipMalloc((void **)&e.Vt, mb) != hipSuccess || hipMalloc((void **)&e.lam, D * sizeof(double)) != hipSuccess) return done(-4);
    hipLaunchKernelGGL(k_transpose, tgrid, dim3(32, 8), 0, st, (const double *)e.sup_V, e.Vt, (long long)D);
    if (hipMemcpyAsync(e.lam, e.sup_lam, D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return done(-4);
    state = 2;
  } else {
    if (e.keep_H && e.keep_D == D) {
      unsigned long long h_chk[4] = {0, 0, 0, 1};
      hipLaunchKernelGGL(k_bits_differ, dim3((unsigned)(((size_t)D * D + 255) / 256)), dim3(256), 0, st, (const double *)ctx->wh_H,
                         (const double *)e.keep_H, (long long)(D * D), (int *)(chk + 3));
      if (hipMemcpyAsync(h_chk, chk, sizeof(h_chk), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return done(-4);
      if ((int)h_chk[3] == 0) {  // the same operator: its basis was checked against these very bits
        e.Vt = e.keep_Vt; e.lam = e.keep_lam;
        e.keep_Vt = e.keep_lam = nullptr;
        e.orth = kept_orth; e.resid = kept_resid; e.solver_ms = kept_ms;
        state = 3;
      }
    }
    if (!state) {
      if (hipMalloc((void **)&e.Vt, mb) != hipSuccess || hipMalloc((void **)&e.lam, D * sizeof(double)) != hipSuccess ||
          hipMemcpyAsync(e.Vt, ctx->wh_H, mb, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return done(-4);
      state = eigen_solve(ctx, e.Vt, e.lam, D, st);
      if (state < 0) return done(state);
    }
  }
  eigen_free_keep(ctx);  // (hipFree waits: the comparison above has run)
  ctx->prof = false;
  if (state != 3) {  // acceptance check: G = V^T V, R = (H V)^T (H is symmetric to the bit: its rows are its columns)
    if (hipMalloc((void **)&G, mb) != hipSuccess || hipMalloc((void **)&R, mb) != hipSuccess) return done(-4);
    if (gemm(ctx, D, D, D, e.Vt, D, e.Vt, D, G, D, st) || gemm(ctx, D, D, D, e.Vt, D, ctx->wh_H, D, R, D, st)) return done(-4);
    hipLaunchKernelGGL(k_basis_check, dim3((unsigned)(((size_t)D * D + 255) / 256)), dim3(256), 0, st, (const double *)G, (const double *)R,
                       (const double *)e.Vt, (const double *)e.lam, (long long)D, chk);
    double h[4] = {0, 0, 0, 0};
    if (hipMemcpyAsync(h, chk, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
        hipGetLastError() != hipSuccess)
      return done(-4);
    e.orth = h[0];
    e.resid = h[2] > 0.0 ? h[1] / h[2] : INFINITY;
    if (!(e.orth <= EIGEN_ORTH_MAX) || !(e.resid <= EIGEN_RESID_MAX)) return done(-3);
  }
  if (hipMalloc((void **)&e.Tin, mb) != hipSuccess || hipMalloc((void **)&e.Tout, mb) != hipSuccess ||
      hipMalloc((void **)&e.Tp, mb) != hipSuccess)
    return done(-4);
  // Tin = V^T L^-1 (L^-1 = sqrt_mass^T: its transpose is the bound array), Tout = L V, Tp = L^-T V = sqrt_mass V
  if (gemm(ctx, D, D, D, e.Vt, D, ctx->met.sqrt_mass, D, e.Tin, D, st) ||
      gemm(ctx, D, D, D, ctx->wh_L, D, e.Vt, D, e.Tout, D, st) ||
      gemm(ctx, D, D, D, ctx->met.sqrt_mass, D, e.Vt, D, e.Tp, D, st))
    return done(-4);
  return done(state);
}
// state and momentum of the whitened problem in workspace vectors that the dense-metric layout holds and the identity
// metric leaves unused
struct WhiteBufs {
  double *z, *hz, *z0, *r, *qn, *gn, *Un, *Uw;
  bool eig;  // the eigen route: z holds y = V^T z, r holds s = V^T r
};
// z0 = L^-1 (q0 - mu), H z0 (the product the leapfrogs form), U0 the caller's (U is invariant); `b` = the whitened
// problem's arguments: identity metric, mu = 0, precision H
// With "dense_whiten_carry" the two products run on the chains whose incoming state is not the carry record's
// (k_white_match, k_compact: all of them when there is no record, none in a chained run); the others keep the z and
// H z the previous transition ended on.  Decided on the device, per chain, by content.
// `ahead` (NUTS, "dense_whiten_ahead"): the half-step momentum gets a vector of its own -- vhalf, which only the literal
// dense mode uses.
// `want_eig` (NUTS, "dense_eigen"): with a basis of H (white_basis) the whitened state is y = V^T z, formed by ONE product
// with Tin = V^T L^-1, its gradient lam o y elementwise, and `b` a coordinate-wise problem (AEHMC_T_WHITE_EIGEN) for the
// diagonal lock-step stage; w.eig says that the route was taken.
static int white_begin(aehmc_ctx *ctx, const EngineArgs &a, EngineArgs &b, WhiteBufs &w, hipStream_t st, bool ahead = false,
                       bool want_eig = false) {
  if (int rc = white_prepare(ctx, st)) {  // (settles a pending record: valid again, or dropped)
    carry_drop(ctx);
    return rc;
  }
  if (want_eig) (void)white_basis(ctx, st);
  const bool eig = want_eig && ctx->eig.ready;
  w.eig = eig;
  const bool had = ctx->carry.valid && ctx->carry.eig == eig;  // (a record of the other route holds another vector)
  carry_drop(ctx);  // consumed: white_end records the next one, a call that fails midway none
  const int64_t C = a.C, D = a.D;
  w.z = a.cur_w; w.hz = a.end_w[0]; w.z0 = a.end_w[1]; w.r = a.cur_v; w.qn = a.end_v[0]; w.gn = a.end_v[1];
  w.Un = a.ckv; w.Uw = a.ckv + C;
  const int tri_in = ctx->wh_tri ? 1 : 0;
  if (ctx->opt_dense_whiten_carry) {
    const bool have = had && ctx->carry.C == C && ctx->carry.D == D && ctx->carry.z == w.z &&
                      ctx->carry.hz == w.hz && ctx->carry.qn == w.qn && ctx->carry.gn == w.gn;
    LAUNCH(k_white_match, C, st, a, have ? 1 : 0, (const double *)w.qn, (const double *)w.gn, (const double *)w.Un, a.rbuf);
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, (const ChainCtl *)a.ctl, (long long)C, a.row_idx, a.n_rows,
                       (int *)nullptr);
    HIPCHK(hipGetLastError());
    if (eig) {
      if (gemm(ctx, C, D, D, a.rbuf, D, ctx->eig.Tin, D, w.z, D, st, a.row_idx, a.n_rows, 0, 0, true)) return -1;
    } else {
      if (gemm(ctx, C, D, D, a.rbuf, D, ctx->wh_Linv, D, w.z, D, st, a.row_idx, a.n_rows, 0, tri_in, true)) return -1;
      if (gemm(ctx, C, D, D, w.z, D, ctx->wh_H, D, w.hz, D, st, a.row_idx, a.n_rows, 0, 0, true)) return -1;
    }
  } else {
    LAUNCH(k_residual, C, st, a, (const double *)a.q, a.rbuf);
    if (eig) {
      if (gemm(ctx, C, D, D, a.rbuf, D, ctx->eig.Tin, D, w.z, D, st)) return -1;
    } else {
      if (gemm(ctx, C, D, D, a.rbuf, D, ctx->wh_Linv, D, w.z, D, st, nullptr, nullptr, 0, tri_in)) return -1;
      if (gemm(ctx, C, D, D, w.z, D, ctx->wh_H, D, w.hz, D, st)) return -1;
    }
  }
  if (eig) LAUNCH(k_eigen_grad, C, st, a, (const double *)ctx->eig.lam, (const double *)w.z, w.hz);  // (every row: the same bits as the record's)
  HIPCHK(hipMemcpyAsync(w.z0, w.z, (size_t)C * D * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(w.Uw, a.U, (size_t)C * sizeof(double), hipMemcpyDeviceToDevice, st));
  b = a;
  b.met_ndim = 0;
  b.imm = b.sqrt_mass = ctx->wh_one;
  b.imm_cs = 0;
  b.linear = 0;
  b.mu = ctx->wh_zero;
  b.white_prec = ctx->wh_H;
  b.cur_v = b.cur_w = b.ckv = nullptr;
  for (int e = 0; e < 2; e++) b.end_v[e] = b.end_w[e] = nullptr;
  b.q = w.z; b.g = w.hz; b.U = w.Uw;
  b.out.momentum = w.r;
  b.phalf = ahead ? a.vhalf : nullptr;
  if (eig) {
    b.tkind = AEHMC_T_WHITE_EIGEN;
    b.sigma = ctx->eig.lam;
    b.white_prec = nullptr;
    b.phalf = nullptr;
  }
  return 0;
}
// p = L^-T r (today's momentum product), q = mu + L z, then (U, g) evaluated afresh at q as aehmc_new_state does; a
// chain whose returned point is its initial one keeps the caller's (q0, U0, g0)
static int white_end(aehmc_ctx *ctx, const EngineArgs &a, const WhiteBufs &w, hipStream_t st) {
  const int64_t C = a.C, D = a.D;
  if (w.eig) {  // p = (L^-T V) s, q - mu = (L V) y
    if (a.out.momentum)
      if (gemm(ctx, C, D, D, w.r, D, ctx->eig.Tp, D, a.out.momentum, D, st)) return -1;
    if (gemm(ctx, C, D, D, w.z, D, ctx->eig.Tout, D, w.qn, D, st)) return -1;
  } else {
    if (a.out.momentum)
      if (metric_mul(ctx, C, w.r, ctx->met.sqrt_mass, a.out.momentum, st, nullptr, nullptr, ctx->wh_tri ? 2 : 0)) return -1;
    if (gemm(ctx, C, D, D, w.z, D, ctx->wh_L, D, w.qn, D, st, nullptr, nullptr, 0, 1)) return -1;
  }
  LAUNCH(k_white_q, C, st, a, (const double *)w.qn, w.qn, a.rbuf);
  if (gemm(ctx, C, D, D, a.rbuf, D, ctx->tgt.prec, D, w.gn, D, st)) return -1;
  LAUNCH(k_half_dot, C, st, a, (const double *)a.rbuf, (const double *)w.gn, w.Un);
  LAUNCH(k_white_out, C, st, a, (const double *)w.z, (const double *)w.z0, w.qn, w.gn, w.Un);
  if (ctx->opt_dense_whiten_carry) {
    ctx->carry.valid = true;
    ctx->carry.C = C; ctx->carry.D = D;
    ctx->carry.z = w.z; ctx->carry.hz = w.hz; ctx->carry.qn = w.qn; ctx->carry.gn = w.gn;
    ctx->carry.eig = w.eig;
  }
  return 0;
}

// one lock-step leapfrog of every live chain (integrators.py:54-73); `book` appends the
// NUTS bookkeeping; `need_v` says whether v' = imm p' must be formed (dense metric);
// `ri`/`nr`: compacted live-chain list for the GEMMs (may be null)
static int launch_leapfrog(aehmc_ctx *ctx, const EngineArgs &a, bool book, bool need_v, hipStream_t st,
                           const int *ri = nullptr, const int *nr = nullptr) {
  const bool md = a.met_ndim == 2;
  const bool tdense = a.tkind == AEHMC_T_DENSE_MVN;
  const int64_t C = a.C, D = a.D;
  const bool tlin = a.tkind == AEHMC_T_LINREG, tglm = a.tkind == AEHMC_T_GLM, tjoint = a.tkind == AEHMC_T_JOINT;
  // targets evaluated between the stages: dense MVN (GEMM), linear regression (row sums), user-defined row reduction,
  // user-defined joint density
  auto target_ext = [&]() -> int {
    if (tdense) return gemm(ctx, C, D, D, a.rbuf, D, a.white_prec ? a.white_prec : ctx->tgt.prec, D, a.cur_g, D, st, ri, nr);
    if (tglm) return launch_glm(ctx, a, a.cur_q, a.cur_g, nullptr, 1, st, ri, nr);
    if (tjoint) return launch_joint_rows(ctx, a, a.cur_q, a.cur_g, nullptr, 1, st, ri, nr);
    return launch_linreg(ctx, a, a.cur_q, a.cur_g, nullptr, 1, st);
  };
  const bool text = tdense || tlin || tglm || tjoint;
  if (!md && !text) {
    if (book) LAUNCH_T(C, st, a, k_step<true, true, true, false, true>);
    else LAUNCH_T(C, st, a, k_step<true, true, true, false, false>);
    return 0;
  }
  if (!md && text) {
    // (whitened dense MVN, NUTS lock-step loop: the first stages of every leapfrog but the first ride in the previous
    //  step's bookkeeping launch -- k_step_white)
    if (!(book && ctx->pre_done)) LAUNCH((k_step<true, true, false, false, false>), C, st, a);
    if (target_ext()) return -1;
    if (book && ctx->fuse_pre) {
      LAUNCH(k_step_white, C, st, a);
      ctx->pre_done = true;
    } else if (book) LAUNCH((k_step<false, false, true, false, true>), C, st, a);
    else LAUNCH((k_step<false, false, true, false, false>), C, st, a);
    return 0;
  }
  if (a.linear) {  // dense metric, v carried by linearity: one metric GEMM (w' = imm g')
    // (NUTS lock-step loop: the first stages of every leapfrog but the first ride in the previous
    //  step's bookkeeping launch -- k_step_linear<15, true>)
    if (!(book && ctx->pre_done)) LAUNCH_T(C, st, a, k_step_linear<12, false>);
    if (text)
      if (target_ext()) return -1;
    if (metric_mul(ctx, C, a.cur_g, ctx->met.imm, a.cur_w, st, ri, nr)) return -1;
    if (book && ctx->fuse_pre) {
      LAUNCH_T(C, st, a, k_step_linear<15, true>);
      ctx->pre_done = true;
    } else if (book) LAUNCH((k_step_linear<3, true>), C, st, a);
    else LAUNCH((k_step_linear<3, false>), C, st, a);
    return 0;
  }
  // dense metric, literal: v_half = imm p_half and v' = imm p' formed directly
  LAUNCH((k_step<true, false, false, true, false>), C, st, a);
  if (metric_mul(ctx, C, a.cur_p, ctx->met.imm, a.vhalf, st, ri, nr)) return -1;
  if (!text) {
    LAUNCH_T(C, st, a, k_step<false, true, true, true, false>);
  } else {
    LAUNCH((k_step<false, true, false, true, false>), C, st, a);
    if (target_ext()) return -1;
    LAUNCH((k_step<false, false, true, true, false>), C, st, a);
  }
  if (need_v || book)
    if (metric_mul(ctx, C, a.cur_p, ctx->met.imm, a.cur_v, st, ri, nr)) return -1;
  if (book) LAUNCH((k_step<false, false, false, true, true>), C, st, a);
  return 0;
}

// One lock-step of the whitened NUTS loop under "dense_whiten_ahead": `GEMM | stage`, the stage being
// k_step_white_ahead.  a.cur_q holds every live chain's current point and a.rbuf receives the position the next product
// multiplies, so the two pointers change places after every kernel that writes the latter: the first lock-step's
// k_white_half_step, then each stage launch.  (The caller's copy of the arguments is the one that is swapped.)
static int launch_white_ahead(aehmc_ctx *ctx, EngineArgs &a, hipStream_t st, const int *ri, const int *nr) {
  const int64_t C = a.C, D = a.D;
  if (!ctx->pre_done) {
    LAUNCH(k_white_half_step, C, st, a);
    std::swap(a.cur_q, a.rbuf);
    ctx->pre_done = true;
  }
  if (gemm(ctx, C, D, D, a.cur_q, D, a.white_prec, D, a.cur_g, D, st, ri, nr)) return -1;
  LAUNCH(k_step_white_ahead, C, st, a);
  std::swap(a.cur_q, a.rbuf);
  return 0;
}

// momentum draw (metrics.py:65-68) + per-chain init, for both samplers
static int launch_begin(aehmc_ctx *ctx, const EngineArgs &a, bool nuts, hipStream_t st) {
  const bool md = a.met_ndim == 2;
  const int64_t C = a.C;
  if (!md) {
    if (nuts) LAUNCH(k_nuts_begin_diag, C, st, a);
    else LAUNCH(k_hmc_begin_diag, C, st, a);
    return 0;
  }
  LAUNCH(k_nuts_draw<true>, C, st, a);
  if (metric_mul(ctx, C, a.zbuf, ctx->met.sqrt_mass, a.cur_p, st)) return -1;  // p = L^-T z
  if (metric_mul(ctx, C, a.cur_p, ctx->met.imm, a.cur_v, st)) return -1;
  if (a.linear)  // w0 = imm g0
    if (metric_mul(ctx, C, a.g, ctx->met.imm, a.cur_w, st)) return -1;
  if (nuts) LAUNCH(k_nuts_init<true>, C, st, a);
  else LAUNCH(k_hmc_init<true>, C, st, a);
  return 0;
}

// ------------------------------------------------------------------ API ------------
extern "C" int aehmc_new_state(aehmc_ctx *ctx, int64_t C, const double *q, double *U, double *g,
                               void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EngineArgs a;
  if (ctx->has_tgt && (target_is_elem_host(ctx->tgt.kind) || ctx->tgt.kind == AEHMC_T_CUSTOM)) {
    memset(&a, 0, sizeof(a));
    a.C = C; a.D = ctx->tgt.D; a.tkind = ctx->tgt.kind;
    a.mu = ctx->tgt.mu; a.sigma = ctx->tgt.sigma; a.log_sigma = ctx->log_sigma;
    a.cparams = ctx->bound.d_cparams;
    a.q = const_cast<double *>(q); a.U = U; a.g = g;
    LAUNCH_T(C, st, a, k_new_state_elem);
    return 0;
  }
  if (ctx->has_tgt && ctx->tgt.kind == AEHMC_T_JOINT) {
    memset(&a, 0, sizeof(a));
    a.C = C; a.D = ctx->tgt.D; a.tkind = ctx->tgt.kind;
    a.cparams = ctx->bound.d_cparams;
    a.q = const_cast<double *>(q); a.U = U; a.g = g;
    if (a.D > FUSED_DENSE_MAX_D) return launch_joint_rows(ctx, a, q, g, U, 0, st, nullptr, nullptr);
    return rtc_launch(ctx, RTC_JBASE, "aehmc::k_new_state_joint", chain_grid(C), dim3(256), 0, st, a);
  }
  if (int rc = fill_args(ctx, C, 1, a, false)) return rc;
  if (a.tkind == AEHMC_T_DENSE_MVN) {
    LAUNCH(k_residual, C, st, a, q, a.rbuf);
    if (gemm(ctx, C, a.D, a.D, a.rbuf, a.D, ctx->tgt.prec, a.D, g, a.D, st)) return -1;
    LAUNCH(k_half_dot, C, st, a, (const double *)a.rbuf, (const double *)g, U);
    return 0;
  }
  if (a.tkind == AEHMC_T_LINREG) {
    return launch_linreg(ctx, a, q, g, U, 0, st);
  }
  if (a.tkind == AEHMC_T_GLM) return launch_glm(ctx, a, q, g, U, 0, st, nullptr, nullptr);
  FAIL("new_state: target kind not implemented");
}

// which kernel family a NUTS call takes (one place: aehmc_nuts_warmup asks before it commits to a
// single-launch warm-up)
enum { NUTS_PATH_LOCKSTEP = 0, NUTS_PATH_LINREG, NUTS_PATH_TEAMS, NUTS_PATH_WIDE, NUTS_PATH_FUSED_DENSE,
       NUTS_PATH_BLOCK_DENSE, NUTS_PATH_PC_DENSE, NUTS_PATH_JOINT_ROWS, NUTS_PATH_GLM_ROWS, NUTS_PATH_JOINT_WG };
// user-defined row-reduction target with few coordinates: the one-launch kernels of glm_rows.cuh keep D partial sums per lane
constexpr int GLM_ROWS_MAX_D = 32;
// Where they pay (tools/debug/glm_time.py, logistic regression; profiles/r5/INDEX.md): the sweep is bound by the user's row
// function on the vector ALUs at 2 - 3 wavefronts per SIMD, the lock-step path runs it at full occupancy, only for live
// chains, and puts the products with X on the matrix cores -- but pays five launches per leapfrog.  One launch wins with
// few coordinates (<= 16: 144 - 152 registers) or few chains (<= 1024: the lock-step path's launches dominate).
static bool glm_rows_wanted(int64_t D, int64_t C) { return D <= GLM_ROWS_MAX_D && (D <= 16 || C <= 1024); }
// long data, few chains: a workgroup of eight wavefronts per chain (glm_rows.cuh: k_nuts_glm_wg / k_hmc_glm_wg)
static bool glm_wg_wanted(const aehmc_ctx *ctx, int64_t D, int64_t C) {
  if (!ctx->opt_joint_wg || D > GLM_ROWS_MAX_D) return false;
  return ctx->opt_joint_wg > 1 || (ctx->glm_N >= 8192 && C <= 2048);
}
static std::string glm_name(const char *kernel, int64_t D, bool wg) {
  return std::string("aehmc::") + kernel + "<" + std::to_string(D) + (wg ? ", 8>" : ">");  // (the kernel for the target's own D)
}
static int nuts_path(const aehmc_ctx *ctx, int64_t C, int64_t max_num_expansions) {
  const int tkind = ctx->tgt.kind, nd = ctx->met.ndim;
  const int64_t D = ctx->tgt.D;
  if (ctx->opt_resident_nuts && nuts_linreg_supported(tkind, nd, D, max_num_expansions)) return NUTS_PATH_LINREG;
  // auto (2) == always where a single-launch kernel exists (round 3): measured again with round 2's resident
  // kernels, they beat the lock-step path at EVERY chain count -- 1.6x to 3x between 2048 and 16384 chains, where
  // the old rule still picked lock-step (tools/debug/resident_vs_lockstep.py, profiles/r3/INDEX.md)
  const bool want_resident = ctx->opt_resident_nuts != 0;
  if (want_resident && nuts_resident_supported(tkind, nd, D)) return NUTS_PATH_TEAMS;  // D <= 512
  if (want_resident && tkind == AEHMC_T_CUSTOM && nd < 2 && D <= 512) return NUTS_PATH_TEAMS;  // (run-time compiled)
  if (want_resident && tkind == AEHMC_T_CUSTOM && nd < 2 && D <= 10176) return NUTS_PATH_WIDE;  // (run-time compiled)
  if (want_resident && nuts_wide_supported(tkind, nd, D)) return NUTS_PATH_WIDE;
  // small dense problems (shared dense metric and / or dense-precision target, D <= 64): one launch, the products
  // inside the wavefront (k_nuts_resident's DENSE instantiations)
  // a traced joint density above 2048 coordinates, scalar / diagonal metric: the workgroup-per-chain kernel with the
  // program's rows in LDS (k_nuts_wide<512, R, true, AEHMC_T_JOINT>, run-time compiled; "joint_wide" option)
  if (want_resident && joint_wide_wanted(ctx)) return NUTS_PATH_WIDE;
  // (none of the joint routes below is taken above JOINT_ROWS_MAX_D: there the lock-step path evaluates the density a
  //  workgroup per chain, k_target_joint_wg)
  // a traced joint density with long data sweeps and few chains: a workgroup per chain (k_nuts_joint_wg, run-time compiled)
  if (want_resident && tkind == AEHMC_T_JOINT && nd < 2 && D <= JOINT_ROWS_MAX_D && joint_wg_wanted(ctx, C)) return NUTS_PATH_JOINT_WG;
  // a joint density with a reverse-mode program (a traced Python logprob_fn), scalar / diagonal metric: the register-resident
  // kernel with the program's rows in LDS -- from 17 coordinates on, or when its reductions are long, it beats the 64
  // forward passes side by side of the dense-path kernel below (funnel, 4096 chains: D = 32 2.5 -> 3.5e8 leapfrog/s, D = 64
  // 1.6 -> 3.4e8; D = 4 / 10: 4.7 / 4.0e8 forward against 4.3 / 3.9e8)
  if (want_resident && tkind == AEHMC_T_JOINT && nd < 2 && D <= FUSED_DENSE_MAX_D && ctx->bound.has_grad &&
      (ctx->opt_joint_resident == 2 ||
       (ctx->opt_joint_resident == 1 && (D > 16 || ctx->bound.grad_small))))
    return NUTS_PATH_TEAMS;
  if (want_resident && tkind == AEHMC_T_JOINT && D <= FUSED_DENSE_MAX_D) return NUTS_PATH_FUSED_DENSE;  // (run-time compiled)
  if (want_resident && tkind == AEHMC_T_GLM && nd < 2 && (glm_rows_wanted(D, C) || glm_wg_wanted(ctx, D, C))) return NUTS_PATH_GLM_ROWS;  // (run-time compiled)
  // joint target of more than 64 coordinates, scalar / diagonal metric: the lock-step loop of a chain in one wavefront,
  // one launch per call (k_nuts_joint_rows); with a dense metric the lock-step path itself (GEMMs over all chains)
  // -- up to D = 192: beyond, the density's O(D^2 / 64) terms are the whole cost and a wavefront that carries its chain
  // through a deep tree holds its SIMD slot while finished chains idle, where the lock-step path compacts the live
  // chains (funnel, 4096 chains: D = 100 3.1 -> 4.9e7 leapfrog/s in one launch, D = 256 1.41 -> 1.35e7: profiles/r5/INDEX.md)
  // a density with a reverse-mode program (AEHMC_JOINT_GRAD, a traced Python logprob_fn) up to D = 512: the register-resident
  // kernel, the position handed to the program through LDS rows (nuts_resident.cuh)
  if (want_resident && tkind == AEHMC_T_JOINT && nd < 2 && D <= 512 && ctx->opt_joint_resident && ctx->bound.has_grad)
    return NUTS_PATH_TEAMS;
  // (... costs O(D / 64) per gradient: one launch whatever D)
  if (want_resident && tkind == AEHMC_T_JOINT && nd < 2 && D <= JOINT_ROWS_MAX_D &&
      (D <= 192 || ctx->bound.has_grad))
    return NUTS_PATH_JOINT_ROWS;
  if (want_resident && nuts_resident_dense_supported(tkind, nd, D))
    return NUTS_PATH_FUSED_DENSE;  // (per-chain dense metrics included: each wavefront reads its own matrices)
  // mid-size dense problems (shared dense metric, 64 < D <= 512, linear dense mode): a workgroup per 16 chains runs
  // the lock-step loop itself, products on MFMA inside the workgroup (nuts_block.cuh)
  if (want_resident && ctx->opt_block_dense && ctx->opt_dense_linear &&
      (block_dense_supported(tkind, nd, ctx->met.per_chain, D) ||
       (tkind == AEHMC_T_CUSTOM && nd == 2 && !ctx->met.per_chain && D >= BLK_MIN_D && D <= BLK_MAX_D)))  // (run-time compiled)
    return NUTS_PATH_BLOCK_DENSE;
  // one dense metric per chain (what full-matrix window adaptation returns), 64 < D <= 512, coordinate-wise target: a
  // wavefront per chain runs the whole call and streams its own matrix (nuts_pc_dense.cuh)
  if (want_resident && ctx->opt_pc_dense && ctx->opt_dense_linear &&
      nuts_pc_dense_supported(tkind, nd, ctx->met.per_chain, D))
    return NUTS_PATH_PC_DENSE;
  return NUTS_PATH_LOCKSTEP;
}

// The NutsSampleArgs of a route.  The caller's multi-transition request is taken -- and *multi_done set -- where the
// route's kernel runs all of it in its one launch (`allowed`, a callable asked only when there is a request); otherwise
// ONE transition.
template <class Allowed>
static NutsSampleArgs take_multi(const NutsSampleArgs *multi, bool *multi_done, Allowed allowed) {
  NutsSampleArgs m{};
  m.T = 1;
  if (multi && multi_done && allowed()) {
    m = *multi;
    *multi_done = true;
  }
  return m;
}

// One NUTS transition of every chain.  `multi` (optional): the caller wants multi->T transitions with
// per-transition outputs; a kernel that runs them all in one launch does so and sets *multi_done,
// otherwise ONE transition is run and the caller loops.
static int nuts_run(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                    int64_t max_num_expansions, double divergence_threshold, double *q, double *U,
                    double *g, const aehmc_diagnostics *out, hipStream_t st,
                    const NutsSampleArgs *multi = nullptr, bool *multi_done = nullptr) {
  if (max_num_expansions < 1 || max_num_expansions > 20) FAIL("max_num_expansions must be in [1, 20]");
  if (!out->acceptance_probability || !out->is_diverging) FAIL("diagnostics arrays missing");
  EngineArgs a;
  if (int rc = fill_args(ctx, C, max_num_expansions, a, true, true)) return rc;
  a.eps = step_size; a.thr = divergence_threshold;
  a.rng = rng; a.nsites = 4;
  a.q = q; a.U = U; a.g = g; a.out = *out;
  // The single-launch kernels (teams of <= 64 lanes up to D = 512, a workgroup per chain above, the
  // workgroup-cooperative regression kernel) are taken wherever they exist; the lock-step engine below serves
  // dense metrics, dense targets, and `resident_nuts` = 0.
  const int path = nuts_path(ctx, C, max_num_expansions);
  const bool white = path == NUTS_PATH_LOCKSTEP && white_wanted(ctx, a);
  if (!white) carry_drop(ctx);  // (every other route may write the workspace vectors the record lives in)
  if (path == NUTS_PATH_LINREG) {
    const NutsSampleArgs m = take_multi(multi, multi_done, [&] {
      return !(multi->adapt && a.met_ndim == 2 && !(multi->ad.full && ctx->met.per_chain));
    });
    return profiled(ctx, st, [&](bool) -> int { HIPCHK(tu::nuts_linreg(a, m, st)); return 0; });
  }
  if (path == NUTS_PATH_WIDE) {  // one workgroup per chain (nuts_wide.cuh): momentum drawn at one wavefront per chain first
    return profiled(ctx, st, [&](bool) -> int {
      if (!wide_rows_padded(a.D))  // (rows of nuts_wide_ld(D) would run past the workspace's vectors)
        FAIL("internal: the workgroup-per-chain NUTS kernel needs D > 512, got D = " + std::to_string(a.D));
      a.ldw = nuts_wide_ld(a.D);
      hipLaunchKernelGGL(k_draw_momentum, chain_grid(C), dim3(256), 0, st, a.rng, a.nsites, (long long)C,
                         (long long)a.D, a.sqrt_mass, (long long)a.imm_cs, a.met_ndim, a.zbuf, a.ldw, 1);
      HIPCHK(hipGetLastError());
      if (a.tkind == AEHMC_T_CUSTOM) {  // the same instantiation (plan_nuts_wide), compiled against the user's function
        return rtc_launch(ctx, RTC_WIDE, nuts_wide_launch(plan_nuts_wide(a.D), AEHMC_T_CUSTOM, C), st, a);
      }
      if (a.tkind == AEHMC_T_JOINT) {  // traced joint density: the rows of its program (q, dU/dq) in LDS at every D
        const KernelLaunch k = nuts_wide_launch(plan_nuts_wide_joint(a.D), AEHMC_T_JOINT, C);
        return joint_rows_launch(ctx, RTC_JWIDE, k.name, a.D + 1, k.grid, k.block, st, a);
      }
      HIPCHK(tu::nuts_wide(a, st));
      return 0;
    });
  }
  if (path == NUTS_PATH_TEAMS) {  // teams of <= 64 lanes: any number of transitions in one launch
    const NutsSampleArgs m = take_multi(multi, multi_done, [] { return true; });
    return profiled(ctx, st, [&](bool) -> int {
      if (a.tkind == AEHMC_T_CUSTOM) {  // the same instantiation, compiled against the user's function
        return rtc_launch(ctx, RTC_NUTS, nuts_resident_launch(plan_nuts_resident(a, m, ctx->opt_resident_min_team)), st, a, m);
      }
      if (a.tkind == AEHMC_T_JOINT) {  // joint density with a reverse-mode program: one wavefront per chain, rows in LDS
        return rtc_launch(ctx, RTC_JNUTS, nuts_resident_launch(plan_nuts_resident_joint(a, m)), st, a, m);
      }
      HIPCHK(tu::nuts_resident(a, m, st, ctx->opt_resident_min_team));
      return 0;
    });
  }
  if (path == NUTS_PATH_FUSED_DENSE) {  // small dense problems: k_nuts_resident's DENSE instantiations
    const bool md = a.met_ndim == 2, td = a.tkind == AEHMC_T_DENSE_MVN, pc = md && ctx->met.per_chain;
    a.linear = 0;  // literal products (metrics.py:71)
    // (adaptation in the launch: per-chain dense)
    NutsSampleArgs m = take_multi(multi, multi_done, [&] { return (!multi->adapt || (pc && multi->ad.full)); });
    m.prec = ctx->tgt.prec;
    if (pc) {  // the chains' transposed matrices
      if (int rc = grow(ctx, &ctx->fd_ws, &ctx->fd_ws_bytes, (size_t)C * a.D * a.D * sizeof(double))) return rc;
      m.imm_ws = ctx->fd_ws;
    }
    return profiled(ctx, st, [&](bool) -> int {
      if (a.tkind == AEHMC_T_JOINT) {  // the same kernel, compiled against the user's density (DENSE bit 8: joint target)
        const int dense = (md ? RES_DENSE_METRIC : 0) | (pc ? RES_DENSE_PER_CHAIN : 0) | RES_DENSE_JOINT;
        return rtc_launch(ctx, RTC_JNUTS, nuts_resident_dense_launch(a, m, dense), st, a, m);
      }
      HIPCHK(tu::nuts_resident_dense(a, m, st, md, td, pc));
      return 0;
    });
  }
  if (path == NUTS_PATH_BLOCK_DENSE) {  // mid-size dense problems: every transition of the call in one launch
    NutsSampleArgs m = take_multi(multi, multi_done, [&] { return !multi->adapt; });
    m.prec = ctx->tgt.prec;
    m.roll = ctx->opt_block_roll;
    if (int rc = grow(ctx, &ctx->blk_pack, &ctx->blk_pack_bytes, blk_pack_bytes(a.D))) return rc;
    double *bp = ctx->blk_pack;
    return profiled(ctx, st, [&](bool) -> int {
      if (a.tkind == AEHMC_T_CUSTOM) {  // the transition-by-transition kernels, compiled against the user's function
        BlkMats mats;
        HIPCHK(blk_pack_matrices(a, nullptr, bp, mats, st));
        EngineArgs b = a;
        b.imm = mats.imm; b.sqrt_mass = mats.sqrt_mass;
        return rtc_launch(ctx, RTC_BLOCK, block_launch(/*nuts*/ true, ctx->opt_block_dense != 2, a.D, C), st, b, m);
      }
      if (ctx->opt_block_dense != 2 && block_roll_wanted(a.D, m.T, ctx->opt_block_roll)) HIPCHK(tu::nuts_block_roll(a, m, bp, st));
      else if (ctx->opt_block_dense != 2 && block_reg_supported(a.D)) HIPCHK(tu::nuts_block_reg(a, m, bp, st));
      else HIPCHK(tu::nuts_block_dense(a, m, bp, st));
      return 0;
    });
  }
  if (path == NUTS_PATH_GLM_ROWS) {  // row-reduction target, D <= 32, scalar / diagonal metric: every transition of the call in one launch
    const NutsSampleArgs m = take_multi(multi, multi_done, [&] { return !multi->adapt; });
    const bool wg = glm_wg_wanted(ctx, a.D, C);
    const std::string name = glm_name(wg ? "k_nuts_glm_wg" : "k_nuts_glm_rows", a.D, wg);
    return profiled(ctx, st, [&](bool) -> int {
      int waves = 0;
      if (wg)
        if (int rc = wg_program(ctx, RTC_GLMK, name, &waves)) return rc;
      return rtc_launch(ctx, {RTC_GLMK, waves}, name, wg ? dim3((unsigned)C) : chain_grid(C), dim3(wg ? 512 : 256), 0, st, a, m,
                        (const double *)ctx->glm_XT, ctx->glm_y, (long long)ctx->glm_N);
    });
  }
  if (path == NUTS_PATH_JOINT_WG) {  // traced joint density, long sweeps, few chains: a workgroup per chain, one launch per call
    const NutsSampleArgs m = take_multi(multi, multi_done, [&] { return !multi->adapt; });
    return profiled(ctx, st, [&](bool) -> int {
      int waves = 0;
      if (int rc = wg_program(ctx, RTC_JWG, RTC_JWG_NUTS, &waves)) return rc;
      return rtc_launch(ctx, {RTC_JWG, waves}, RTC_JWG_NUTS, dim3((unsigned)C), dim3(512), (size_t)2 * a.D * sizeof(double), st, a, m);
    });
  }
  if (path == NUTS_PATH_JOINT_ROWS) {  // joint target, D > 64, scalar / diagonal metric: every transition of the call in one launch
    const NutsSampleArgs m = take_multi(multi, multi_done, [&] { return !multi->adapt; });
    return profiled(ctx, st, [&](bool) -> int { return rtc_launch(ctx, RTC_JBASE, "aehmc::k_nuts_joint_rows", chain_grid(C), dim3(256), (size_t)8 * a.D * sizeof(double), st, a, m); });
  }
  if (path == NUTS_PATH_PC_DENSE) {  // per-chain dense metrics, 64 < D <= 512: every transition of the call in one launch
    const NutsSampleArgs m = take_multi(multi, multi_done, [&] { return !multi->adapt; });
    return profiled(ctx, st, [&](bool) -> int { HIPCHK(tu::nuts_pc_dense(a, m, st)); return 0; });
  }
  if (ctx->opt_fused_nuts && a.met_ndim < 2 && target_is_elem_host(a.tkind)) {
    return profiled(ctx, st, [&](bool) -> int { LAUNCH(k_nuts_fused, C, st, a); return 0; });
  }
  ctx->rows_hint = 0;
  EngineArgs wa;  // whitened mode: the transition runs on the whitened problem (white_begin), mapped back at the end
  WhiteBufs wb{};
  if (white)
    if (int rc = white_begin(ctx, a, wa, wb, st, ctx->opt_dense_whiten_ahead, eigen_wanted(ctx, a.D))) return rc;
  EngineArgs &e = white ? wa : a;
  const bool eig = white && wb.eig;  // a coordinate-wise problem from here on: the diagonal stage, nothing to compact
  const bool ahead = white && e.phalf;
  ctx->fuse_pre = !eig && (a.linear != 0 || white);
  ctx->pre_done = false;
  if (eig && ctx->opt_dense_eigen_wide && nuts_wide_eigen_supported(a.D)) {
    // "dense_eigen_wide": the coordinate-wise problem is k_nuts_wide's -- one workgroup carries a chain through its whole
    // tree, lambda where the isotropic instantiation keeps imm.  The raw normals as every route draws them (rows of D in
    // cur_p, which the kernel leaves alone), s = V^T r into zbuf with the kernel's row stride (its idle slots read the
    // padding columns as their momentum: zeroed), one launch.  The kernel's work vectors (ckp, cks, slot_*, end_q/p/g,
    // psum, zbuf) and WhiteBufs' (cur_w, end_w, cur_v, end_v, ckv: the dense-metric block of ws_layout) are disjoint.
    const int64_t D = a.D, ldw = nuts_wide_ld(D);
    hipLaunchKernelGGL(k_draw_momentum, chain_grid(C), dim3(256), 0, st, e.rng, e.nsites, (long long)C, (long long)D,
                       e.sqrt_mass, (long long)e.imm_cs, e.met_ndim, e.cur_p, (long long)D, 1);
    HIPCHK(hipGetLastError());
    if (ldw > D)
      HIPCHK(hipMemset2DAsync(e.zbuf + D, (size_t)ldw * sizeof(double), 0, (size_t)(ldw - D) * sizeof(double), (size_t)C, st));
    if (gemm(ctx, C, D, D, e.cur_p, D, ctx->eig.Vt, D, e.zbuf, ldw, st)) return -1;
    e.ldw = ldw;
    HIPCHK(tu::nuts_wide(e, st));
    return white_end(ctx, a, wb, st);
  }
  if (eig) {  // the raw normals as every route draws them, s = V^T r, then the chain's init on the rotated momentum
    LAUNCH(k_nuts_draw<true>, C, st, e);
    if (gemm(ctx, C, a.D, a.D, e.zbuf, a.D, ctx->eig.Vt, a.D, e.cur_p, a.D, st)) return -1;
    LAUNCH(k_nuts_init<false>, C, st, e);
  } else if (int rc = launch_begin(ctx, e, true, st)) return rc;
  long long maxsteps = 0;
  for (int j = 0; j < max_num_expansions; j++) maxsteps += (1LL << j) + 1;  // 2**j + 1 per expansion
  const bool compact = !eig && ctx->opt_compact && (a.met_ndim == 2 || a.tkind == AEHMC_T_DENSE_MVN || a.tkind == AEHMC_T_GLM || a.tkind == AEHMC_T_JOINT);
  const int *ri = compact ? a.row_idx : nullptr, *nr = compact ? a.n_rows : nullptr;
  if (compact) {
    hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, (const ChainCtl *)a.ctl, (long long)C,
                       a.row_idx, a.n_rows, (int *)nullptr);
    HIPCHK(hipGetLastError());
  }
  long long s = 0;
  int batch = 0;
  while (s < maxsteps) {
    if (batch >= 2) {  // lagging poll: never drains the queue
      int slot = (batch - 2) % NRING;
      HIPCHK(hipEventSynchronize(ctx->ev[slot]));
      if (int rc = check_device_errors(ctx)) return rc;
      if (ctx->h_active[slot] == 0) break;
      if (compact) ctx->rows_hint = ctx->h_active[slot];
    }
    const int slot = batch % NRING;
    for (int k = 0; k < STEP_BATCH && s < maxsteps; k++, s++) {
      if (int rc = ahead ? launch_white_ahead(ctx, e, st, ri, nr) : launch_leapfrog(ctx, e, true, true, st, ri, nr)) return rc;
      if (compact) {
        const bool last = (k == STEP_BATCH - 1) || (s == maxsteps - 1);
        hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, st, (const ChainCtl *)a.ctl,
                           (long long)C, a.row_idx, a.n_rows, last ? ctx->d_active + slot : (int *)nullptr);
        HIPCHK(hipGetLastError());
      }
    }
    if (!compact) {
      hipLaunchKernelGGL(k_count_active, dim3(1), dim3(1024), 0, st, (const ChainCtl *)a.ctl,
                         (long long)C, ctx->d_active + slot);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ev[slot], st));
    batch++;
  }
  ctx->rows_hint = 0;
  ctx->fuse_pre = ctx->pre_done = false;
  if (white) return white_end(ctx, a, wb, st);
  return 0;
}

extern "C" int aehmc_nuts_step(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                               int64_t max_num_expansions, double divergence_threshold, double *q,
                               double *U, double *g, const aehmc_diagnostics *out, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  return nuts_run(ctx, C, rng, step_size, max_num_expansions, divergence_threshold, q, U, g, out,
                  (hipStream_t)stream);
}

// What the four warm-up entry points check before they enqueue anything (`State`: aehmc_adapt_state, one adaptation per
// chain, or aehmc_pooled_adapt_state, ONE for all chains): the arguments, then that the bound step sizes and metric are
// the adaptation state's own arrays -- every path samples with the bound arrays while the update kernel rewrites the
// state's, so they must be the same.
template <class State>
static int warmup_bound(aehmc_ctx *ctx, int64_t C, const aehmc_diagnostics *out, const State *state,
                        const int32_t *stage, const int32_t *is_window_end) {
  constexpr bool pooled = std::is_same<State, aehmc_pooled_adapt_state>::value;
  if (!ctx || !out || !state || !stage || !is_window_end) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->has_tgt || (pooled && !ctx->has_met)) FAIL("set_target and set_metric must be called first");
  if (!ctx->eps_c || (pooled ? ctx->eps_n != C || ctx->met.per_chain : !ctx->met.per_chain))
    FAIL(pooled ? "pooled warm-up needs the step sizes [C] of the adaptation state and a SHARED metric bound"
                : "warm-up needs per-chain step sizes and a per-chain metric bound to the adaptation state");
  if (ctx->met.imm != state->imm || ctx->met.sqrt_mass != state->sqrt_mass || ctx->eps_c != state->step_size)
    FAIL(pooled ? "pooled warm-up: the bound metric / step sizes are not the adaptation state's own arrays "
                  "(bind state->imm, state->sqrt_mass with aehmc_set_metric and state->step_size with aehmc_set_step_sizes)"
                : "warm-up: the bound per-chain metric / step sizes are not the adaptation state's own arrays "
                  "(bind state->imm, state->sqrt_mass with aehmc_set_metric and state->step_size with aehmc_set_step_sizes)");
  if (pooled && (ctx->met.ndim == 2) != (state->full != 0)) FAIL("pooled warm-up: the bound metric and state->full disagree");
  return 0;
}

// The warm-up loop (window_adaptation.py:66-77): num_steps x (`transition()`, then `update` -- aehmc_adapt_update or
// aehmc_pooled_adapt_update -- on its acceptance probabilities and positions), enqueued in one call: the same kernels in
// the same order as the caller's own loop.  `rebind` (pooled): after a window end the shared metric is bound again --
// the same arrays, new content: the engine drops what it derived from the old one.
template <class Transition, class Update, class State>
static int warmup_loop(aehmc_ctx *ctx, int64_t C, int64_t num_steps, const int32_t *stage, const int32_t *is_window_end,
                       double target_acceptance_rate, const double *q, const aehmc_diagnostics *out, const State *state,
                       void *stream, bool rebind, Update update, Transition transition) {
  const int64_t D = ctx->tgt.D;
  for (int64_t i = 0; i < num_steps; i++) {
    if (int rc = transition()) return rc;
    if (int rc = update(ctx, C, D, stage[i], is_window_end[i], i == num_steps - 1, target_acceptance_rate,
                        out->acceptance_probability, q, state, stream))
      return rc;
    if (rebind && is_window_end[i]) {
      const aehmc_metric m = ctx->met;
      if (int rc = aehmc_set_metric(ctx, &m)) return rc;
    }
  }
  return 0;
}

// window_adaptation.run (window_adaptation.py:17-116): the whole warm-up loop -- one NUTS transition
// with the current per-chain parameters, then the adaptation update -- enqueued without returning
// to the host language between steps.  The caller has bound the per-chain metric (state->imm /
// state->sqrt_mass) and step sizes (state->step_size), which the update kernel rewrites in place.
extern "C" int aehmc_nuts_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps,
                                 const int32_t *stage, const int32_t *is_window_end,
                                 double target_acceptance_rate, int64_t max_num_expansions,
                                 double divergence_threshold, double *q, double *U, double *g,
                                 const aehmc_diagnostics *out, const aehmc_adapt_state *state, void *stream) {
  if (int rc = warmup_bound(ctx, C, out, state, stage, is_window_end)) return rc;
  const int64_t D = ctx->tgt.D;
  // diagonal mass matrix, regression target or a coordinate-wise target with D <= 512: the whole warm-up
  // in ONE launch, the chains adapting and moving on at their own pace (nuts_linreg.cuh: every chain;
  // nuts_resident.cuh: every wavefront) -- the same arithmetic as the loop below
  const int path = ctx->has_met ? nuts_path(ctx, C, max_num_expansions) : NUTS_PATH_LOCKSTEP;
  const bool one_launch_diag = (path == NUTS_PATH_LINREG || path == NUTS_PATH_TEAMS) && !state->full &&
                               (ctx->met.ndim == 1 || (ctx->met.ndim == 0 && D == 1 && path == NUTS_PATH_TEAMS));
  // is_mass_matrix_full with D <= 64: the small-dense kernel adapts its chain's matrix itself
  // (and the regression kernel its chain's 2 x 2 matrix)
  const bool one_launch_full = (path == NUTS_PATH_FUSED_DENSE || path == NUTS_PATH_LINREG) && state->full &&
                               ctx->met.ndim == 2;
  if (num_steps > 0 && (one_launch_diag || one_launch_full) && ctx->met.per_chain) {
    hipStream_t st = (hipStream_t)stream;
    AdaptArgs aa;
    if (int rc = adapt_args(ctx, C, D, state, aa)) return rc;
    if (ctx->d_sched_n < num_steps) {
      if (ctx->d_sched) HIPCHK(hipFree(ctx->d_sched));
      ctx->d_sched = nullptr;
      HIPCHK(hipMalloc(&ctx->d_sched, (size_t)2 * num_steps * sizeof(int)));
      ctx->d_sched_n = num_steps;
    }
    HIPCHK(hipMemcpyAsync(ctx->d_sched, stage, (size_t)num_steps * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->d_sched + num_steps, is_window_end, (size_t)num_steps * sizeof(int),
                          hipMemcpyHostToDevice, st));
    NutsSampleArgs multi{};
    multi.T = num_steps;
    multi.adapt = 1;
    multi.stage = ctx->d_sched;
    multi.window_end = ctx->d_sched + num_steps;
    multi.target = target_acceptance_rate;
    multi.gamma = aa.gamma; multi.t0 = aa.t0; multi.kappa = aa.kappa;
    multi.ad = *state;
    bool all_done = false;
    if (int rc = nuts_run(ctx, C, rng, 0.0, max_num_expansions, divergence_threshold, q, U, g, out, st, &multi,
                          &all_done))
      return rc;
    if (!all_done) FAIL("internal: the fused warm-up kernel was not taken");
    return 0;
  }
  return warmup_loop(ctx, C, num_steps, stage, is_window_end, target_acceptance_rate, q, out, state, stream, false,
                     aehmc_adapt_update, [&] {
                       return nuts_run(ctx, C, rng, 0.0, max_num_expansions, divergence_threshold, q, U, g, out,
                                       (hipStream_t)stream);
                     });
}

// one transition of a sample() call into the caller's histories (each optional): the positions after transition t, its
// acceptance probabilities and divergence flags
static int record_transition(aehmc_ctx *ctx, int64_t C, int64_t D, int64_t t, const double *q,
                             const aehmc_diagnostics *out, double *samples, double *acceptance_history,
                             int32_t *divergence_history, hipStream_t st) {
  if (samples)
    HIPCHK(hipMemcpyAsync(samples + (size_t)t * C * D, q, (size_t)C * D * sizeof(double),
                          hipMemcpyDeviceToDevice, st));
  if (acceptance_history)
    HIPCHK(hipMemcpyAsync(acceptance_history + (size_t)t * C, out->acceptance_probability,
                          C * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (divergence_history)
    HIPCHK(hipMemcpyAsync(divergence_history + (size_t)t * C, out->is_diverging, C * sizeof(int32_t),
                          hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int aehmc_nuts_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                                 int64_t max_num_expansions, double divergence_threshold,
                                 int64_t num_samples, double *q, double *U, double *g,
                                 const aehmc_diagnostics *out, double *samples,
                                 double *acceptance_history, int32_t *divergence_history,
                                 int64_t *n_leapfrog_total, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (num_samples < 1) FAIL("number of transitions must be >= 1");
  if (!ctx->has_tgt) FAIL("set_target and set_metric must be called first");
  const int64_t D = ctx->tgt.D;
  if (n_leapfrog_total) {
    if (!out->n_leapfrog) FAIL("n_leapfrog_total needs out->n_leapfrog");
    HIPCHK(hipMemsetAsync(n_leapfrog_total, 0, C * sizeof(int64_t), st));
  }
  NutsSampleArgs multi{};
  multi.T = num_samples;
  multi.samples = samples;
  multi.acc_hist = acceptance_history;
  multi.div_hist = divergence_history;
  multi.nleap_total = (long long *)n_leapfrog_total;
  for (int64_t t = 0; t < num_samples; t++) {
    bool all_done = false;
    if (int rc = nuts_run(ctx, C, rng, step_size, max_num_expansions, divergence_threshold, q, U, g,
                          out, st, t == 0 ? &multi : nullptr, &all_done))
      return rc;
    if (all_done) return 0;  // every transition ran inside that one launch
    if (int rc = record_transition(ctx, C, D, t, q, out, samples, acceptance_history, divergence_history, st)) return rc;
    if (n_leapfrog_total)
      LAUNCH(k_add_i64, C, st, (long long *)n_leapfrog_total, (const long long *)out->n_leapfrog, (long long)C);
  }
  return 0;
}

// which kernel family an HMC call takes, as nuts_path for NUTS: the first condition that holds, read from the bound
// target / metric and the options alone (of what fill_args puts into EngineArgs: a.tkind = ctx->tgt.kind, a.met_ndim =
// ctx->met.ndim, a.linear = dense metric && "dense_linear").  hmc_run holds one block per route and no condition.
enum { HMC_PATH_LOCKSTEP = 0, HMC_PATH_FUSED, HMC_PATH_CUSTOM_FUSED, HMC_PATH_JOINT_FUSED, HMC_PATH_LINREG, HMC_PATH_WIDE,
       HMC_PATH_FUSED_DENSE, HMC_PATH_GLM_ROWS, HMC_PATH_JOINT_WG, HMC_PATH_JOINT_ROWS, HMC_PATH_PC_DENSE, HMC_PATH_BLOCK_DENSE };
static int hmc_path(const aehmc_ctx *ctx, int64_t C) {
  const int tkind = ctx->tgt.kind, nd = ctx->met.ndim;
  const int64_t D = ctx->tgt.D;
  // fused register-resident path (hmc_fused.cuh): diagonal/scalar metric, coordinate-wise target
  if (ctx->opt_fused_hmc && hmc_fused_supported(ctx->tgt.kind, ctx->met.ndim, D)) return HMC_PATH_FUSED;
  // user-defined coordinate-wise target: the same fused kernel, compiled against the user's function at run time
  if (ctx->opt_fused_hmc && ctx->tgt.kind == AEHMC_T_CUSTOM && ctx->met.ndim < 2 && D <= 1024) return HMC_PATH_CUSTOM_FUSED;
  // traced joint density with its reverse-mode program, 64 < D <= 1024: the same fused kernel ("joint_resident" option;
  // D <= 64 stays on k_hmc_fused_dense)
  if (ctx->opt_fused_hmc && ctx->opt_joint_resident && ctx->tgt.kind == AEHMC_T_JOINT && ctx->bound.has_grad && ctx->met.ndim < 2 &&
      D > FUSED_DENSE_MAX_D && D <= 1024 && !joint_wg_wanted(ctx, C) && !joint_wide_wanted(ctx))
    return HMC_PATH_JOINT_FUSED;
  // regression target (hmc_linreg.cuh)
  if (ctx->opt_fused_hmc && hmc_linreg_supported(ctx->tgt.kind, ctx->met.ndim, D)) return HMC_PATH_LINREG;
  // a workgroup per chain (k_hmc_wide); a user-defined coordinate-wise target: the same kernel compiled against the user's function
  const bool custom_wide = ctx->tgt.kind == AEHMC_T_CUSTOM && ctx->met.ndim < 2 && D > 1024 && D <= 10240;
  // (a traced joint density above 2048 coordinates: the AEHMC_T_JOINT instantiation, the program's rows in LDS)
  const bool joint_wide = joint_wide_wanted(ctx);
  if (ctx->opt_fused_hmc && (custom_wide || joint_wide || hmc_resident_supported(ctx->tgt.kind, ctx->met.ndim, D))) return HMC_PATH_WIDE;
  // small dense problems (shared dense metric and / or dense-precision target, D <= 64): the transition in one
  // launch with the products inside the wavefront (k_hmc_fused_dense), as for NUTS
  const bool tjoint = tkind == AEHMC_T_JOINT;
  const bool fused_dense = ctx->opt_fused_hmc && D <= FUSED_DENSE_MAX_D && !(tjoint && nd < 2 && joint_wg_wanted(ctx, C)) &&
                           (tjoint || ((nd == 2 || tkind == AEHMC_T_DENSE_MVN) &&
                                       (target_is_elem_host(tkind) || tkind == AEHMC_T_DENSE_MVN)));
  if (fused_dense) return HMC_PATH_FUSED_DENSE;
  // row-reduction target with D <= 32, scalar / diagonal metric (glm_rows.cuh)
  if (ctx->opt_fused_hmc && tkind == AEHMC_T_GLM && nd < 2 && (glm_rows_wanted(D, C) || glm_wg_wanted(ctx, D, C))) return HMC_PATH_GLM_ROWS;
  // traced joint density with long data sweeps, few chains: a workgroup per chain (k_hmc_joint_wg)
  if (ctx->opt_fused_hmc && tjoint && nd < 2 && D <= JOINT_ROWS_MAX_D && joint_wg_wanted(ctx, C)) return HMC_PATH_JOINT_WG;
  // joint target of more than 64 coordinates, scalar / diagonal metric (k_hmc_joint_rows)
  if (ctx->opt_fused_hmc && tjoint && nd < 2 && D <= JOINT_ROWS_MAX_D) return HMC_PATH_JOINT_ROWS;
  const bool linear = nd == 2 && ctx->opt_dense_linear;  // (fill_args: a.linear)
  // one dense metric per chain, 64 < D <= 512, coordinate-wise target, linear dense mode (nuts_pc_dense.cuh)
  if (ctx->opt_fused_hmc && ctx->opt_pc_dense && linear && nuts_pc_dense_supported(tkind, nd, ctx->met.per_chain, D)) return HMC_PATH_PC_DENSE;
  // mid-size dense problems (shared dense metric, 64 < D <= 512, linear dense mode; nuts_block.cuh)
  const bool custom_block = tkind == AEHMC_T_CUSTOM && nd == 2 && !ctx->met.per_chain && D >= BLK_MIN_D && D <= BLK_MAX_D;
  if (ctx->opt_fused_hmc && ctx->opt_block_dense && linear && (custom_block || block_dense_supported(tkind, nd, ctx->met.per_chain, D)))
    return HMC_PATH_BLOCK_DENSE;
  return HMC_PATH_LOCKSTEP;
}
// what every whole-call kernel on HmcFusedArgs reads of the call; the route adds its target's parameters, its literal
// `tkind`, the per-transition outputs and, where its kernel has the mode, `fc`
static HmcFusedArgs hmc_fused_args(const aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size, int64_t L,
                                   double divergence_threshold, double *q, double *U, double *g, const aehmc_diagnostics *out) {
  HmcFusedArgs f{};
  f.C = C; f.D = ctx->tgt.D; f.L = L; f.eps = step_size; f.thr = divergence_threshold;
  f.met_ndim = ctx->met.ndim; f.imm = ctx->met.imm; f.sqrt_mass = ctx->met.sqrt_mass;
  f.imm_cs = ctx->met.per_chain ? (ctx->met.ndim == 0 ? 1 : f.D) : 0;
  f.eps_c = ctx->eps_c;
  f.rng = rng; f.q = q; f.U = U; f.g = g; f.out = *out;
  return f;
}
// one library instantiation of k_hmc_fused_dense (LS: the trajectory lengths come from h.len)
template <bool MD, bool TD, bool PC, bool LS>
static hipError_t launch_hmc_fused_dense(const KernelLaunch &k, const EngineArgs &a, const HmcSampleArgs &h, hipStream_t st) {
  if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hmc_fused_dense<MD, TD, PC, LS>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.dyn))
    return e;
  hipLaunchKernelGGL((k_hmc_fused_dense<MD, TD, PC, LS>), k.grid, k.block, k.dyn, st, a, h);
  return hipGetLastError();
}
// The trajectory lengths of a call that does not run one L throughout: `dev`[t * stride] on the device (stride 1: one per
// transition; 0: one cell for the whole call, the ChEES warm-up's num_steps), clamped to [0, max] by the kernels; `host`:
// the same [T] entries where the caller knows them (nullptr: the warm-up's cell), `sum` their total.
struct HmcLens {
  const long long *dev;
  long long stride;
  const int64_t *host;
  long long max, sum;
};
// The routes whose kernels read the lengths from device memory (DESIGN section 3 lists them); every other route runs a
// call with lengths as single transitions, L from `host`.
static bool hmc_path_reads_lengths(int path) {
  return path == HMC_PATH_FUSED || path == HMC_PATH_CUSTOM_FUSED || path == HMC_PATH_JOINT_FUSED || path == HMC_PATH_LINREG ||
         path == HMC_PATH_WIDE || path == HMC_PATH_FUSED_DENSE || path == HMC_PATH_BLOCK_DENSE;
}
// n_leapfrog = `total` (L T, or the sum of the call's lengths) of every chain behind a kernel that ran the whole call.
// `only_multi`: the route's kernel writes it itself when T == 1 (which routes do is kernel behaviour)
static int fill_n_leapfrog(aehmc_ctx *ctx, int64_t C, int64_t total, int64_t T, const aehmc_diagnostics *out, bool only_multi,
                           hipStream_t st) {
  if ((!only_multi || T > 1) && out->n_leapfrog)
    LAUNCH(k_fill_i64, C, st, (long long *)out->n_leapfrog, (long long)C, (long long)total);
  return 0;
}

// T HMC transitions of every chain; optional per-transition outputs (samples [T,C,D],
// acc_hist [T,C], div_hist [T,C])
static int hmc_run(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size, int64_t L,
                   double divergence_threshold, int64_t T, double *q, double *U, double *g,
                   const aehmc_diagnostics *out, double *samples, double *acc_hist,
                   int32_t *div_hist, hipStream_t st, const HmcLens *len = nullptr) {
  if (L < 0) FAIL("num_integration_steps must be >= 0");
  if (T < 1) FAIL("number of transitions must be >= 1");
  if (!out->acceptance_probability || !out->is_diverging) FAIL("diagnostics arrays missing");
  if (!ctx->has_tgt || !ctx->has_met) FAIL("set_target and set_metric must be called first");
  const int64_t D = ctx->tgt.D;
  const int path = hmc_path(ctx, C);
  if (len && !hmc_path_reads_lengths(path)) {  // one single-transition pass per entry, as the caller's own loop would run them
    if (!len->host) FAIL("internal: this route needs the trajectory lengths on the host");
    for (int64_t t = 0; t < T; t++) {
      if (int rc = hmc_run(ctx, C, rng, step_size, len->host[t], divergence_threshold, 1, q, U, g, out, nullptr, nullptr,
                           nullptr, st))
        return rc;
      if (int rc = record_transition(ctx, C, D, t, q, out, samples, acc_hist, div_hist, st)) return rc;
    }
    return fill_n_leapfrog(ctx, C, len->sum, T, out, true, st);
  }
  const int64_t total = len ? len->sum : L * T;  // n_leapfrog of the whole call
  const HmcLengths dl = len ? HmcLengths{len->dev, len->stride, len->max} : HmcLengths{nullptr, 0, 0};
  // The first four routes run the whole call in one launch on HmcFusedArgs alone: no workspace, so no fill_args (they
  // never report "workspace too small" or "dimensions differ").
  if (path == HMC_PATH_FUSED || path == HMC_PATH_CUSTOM_FUSED || path == HMC_PATH_JOINT_FUSED || path == HMC_PATH_LINREG) {
    if (int rc = check_per_chain(ctx, C)) return rc;
    HmcFusedArgs f = hmc_fused_args(ctx, C, rng, step_size, L, divergence_threshold, q, U, g, out);
    f.T = T; f.samples = samples; f.acc_hist = acc_hist; f.div_hist = div_hist;
    f.Ls = dl.Ls; f.ls = dl.ls; f.Lmax = dl.Lmax;
    if (path == HMC_PATH_FUSED) {  // fused register-resident path (hmc_fused.cuh): diagonal/scalar metric, coordinate-wise target
      f.tkind = ctx->tgt.kind; f.mu = ctx->tgt.mu; f.sigma = ctx->tgt.sigma; f.log_sigma = ctx->log_sigma;
      f.fc = ctx->opt_fp_contract;
      return profiled(ctx, st, [&](bool) -> int { HIPCHK(tu::hmc_fused(f, st)); return 0; });
    }
    if (path == HMC_PATH_LINREG) {  // regression target: the whole call in one launch, four chains per workgroup (hmc_linreg.cuh)
      f.tkind = ctx->tgt.kind; f.X = ctx->tgt.X; f.y = ctx->tgt.y; f.N = ctx->tgt.N;
      return profiled(ctx, st, [&](bool) -> int { HIPCHK(tu::hmc_linreg(f, st)); return 0; });
    }
    if (path == HMC_PATH_CUSTOM_FUSED) {  // user-defined coordinate-wise target: the same fused kernel, compiled against the user's function at run time
      f.tkind = AEHMC_T_CUSTOM; f.cparams = ctx->bound.d_cparams;
      f.fc = ctx->opt_fp_contract;
      return profiled(ctx, st, [&](bool) -> int {
        return rtc_launch(ctx, RTC_HMC, hmc_fused_launch(D, AEHMC_T_CUSTOM, f.fc, C, len != nullptr), st, f);
      });
    }
    // traced joint density (round 6): the same fused kernel with the position and gradient rows of the generated program in LDS
    f.tkind = AEHMC_T_JOINT; f.cparams = ctx->bound.d_cparams;
    return profiled(ctx, st, [&](bool) -> int {
      return rtc_launch(ctx, RTC_JHMCF, hmc_fused_launch(D, AEHMC_T_JOINT, false, C, len != nullptr), st, f);
    });
  }
  EngineArgs a;
  if (int rc = fill_args(ctx, C, 1, a, true, true)) return rc;
  const bool white = path == HMC_PATH_LOCKSTEP && white_wanted(ctx, a);
  if (!white) carry_drop(ctx);  // (every other route may write the workspace vectors the record lives in)
  if (path == HMC_PATH_WIDE) {  // a workgroup per chain (k_hmc_wide), coordinate-wise target or traced joint density
    HmcFusedArgs f = hmc_fused_args(ctx, C, rng, step_size, L, divergence_threshold, q, U, g, out);
    f.tkind = ctx->tgt.kind; f.mu = ctx->tgt.mu; f.sigma = ctx->tgt.sigma; f.log_sigma = ctx->log_sigma;
    f.cparams = ctx->bound.d_cparams;
    f.fc = ctx->opt_fp_contract;
    // A launch pair per CHUNK of transitions: the momenta of the chunk are drawn first, at one wavefront per
    // chain (k_draw_momentum), into [nt][C][D]; the workgroup-per-chain kernel then runs the nt transitions
    // with the position on chip.  The chunk's normals live in the first work vectors of the workspace (cur_q
    // ... zbuf are contiguous and unused on this path): as many transitions as fit, 22 with the HMC layout.
    // (Drawing chunk k+1 on a side stream BESIDE the integration of chunk k was measured in round 3: the two
    // kernels do share the CUs -- 4 x 96 + 96 of a SIMD's 512 registers -- but both are bound by VALU issue, and
    // together they take what they take one after the other: profiles/r3/INDEX.md.)
    const size_t vec = (size_t)((char *)a.cur_p - (char *)a.cur_q);
    const size_t cap_bytes = (size_t)((char *)a.zbuf - (char *)a.cur_q) + vec;
    const int64_t cap = (int64_t)(cap_bytes / ((size_t)C * D * sizeof(double)));
    // the chunk's normals overlay cur_q .. zbuf: that span must be what ws_layout makes it -- contiguous vectors of
    // one size, inside the caller's workspace, none of them touched by k_draw_momentum / k_hmc_wide themselves
    if (cap < 1 || (char *)a.cur_g - (char *)a.cur_p != (ptrdiff_t)vec || a.zbuf < a.cur_q ||
        (char *)a.zbuf + vec > (char *)ctx->ws + ctx->ws_bytes || (char *)a.cur_q < (char *)ctx->ws)
      FAIL("internal: the workspace span for the momentum rows is not the layout hmc_run expects");
    double *zall = a.cur_q;
    return profiled(ctx, st, [&](bool) -> int {
      for (int64_t t0 = 0; t0 < T; t0 += cap) {
        const int nt = (int)(T - t0 < cap ? T - t0 : cap);
        hipLaunchKernelGGL(k_draw_momentum, chain_grid(C), dim3(256), 0, st, rng, 2, (long long)C, (long long)D,
                           f.sqrt_mass, f.imm_cs, f.met_ndim, zall, (long long)D, nt);
        HIPCHK(hipGetLastError());
        f.samples = samples ? samples + (size_t)t0 * C * D : nullptr;
        f.acc_hist = acc_hist ? acc_hist + (size_t)t0 * C : nullptr;
        f.div_hist = div_hist ? div_hist + (size_t)t0 * C : nullptr;
        f.out.momentum = t0 + nt == T ? out->momentum : nullptr;  // only the last transition's is observable
        if (dl.Ls) {  // the chunk's own slice of the lengths
          f.Ls = dl.Ls + t0 * dl.ls; f.ls = dl.ls; f.Lmax = dl.Lmax;
        }
        if (f.tkind == AEHMC_T_CUSTOM) {  // the same instantiation (plan_hmc_wide), compiled against the user's function (round 5)
          const KernelLaunch k = hmc_wide_launch(plan_hmc_wide(D, AEHMC_T_CUSTOM), AEHMC_T_CUSTOM, f.fc, C);
          if (int rc = rtc_launch(ctx, RTC_HMC, k, st, f, (const double *)zall, nt)) return rc;
        } else if (f.tkind == AEHMC_T_JOINT) {  // k_nuts_wide's rule: 512 threads (the program's workgroup), q and dU/dq in LDS only
          const KernelLaunch k = hmc_wide_launch(plan_hmc_wide_joint(D), AEHMC_T_JOINT, false, C);
          if (int rc = joint_rows_launch(ctx, RTC_JWIDE, k.name, D + 1, k.grid, k.block, st, f, (const double *)zall, nt))
            return rc;
        } else {
          HIPCHK(tu::hmc_resident(f, zall, nt, st));
        }
      }
      return fill_n_leapfrog(ctx, C, total, T, out, true, st);
    });
  }
  a.eps = step_size; a.thr = divergence_threshold;
  a.rng = rng; a.nsites = 2;
  a.q = q; a.U = U; a.g = g; a.out = *out;
  // The routes below run the whole call in one launch on (EngineArgs, HmcSampleArgs): the kernel, then n_leapfrog of the
  // whole call where the kernel does not write it itself (fill_n_leapfrog)
  HmcSampleArgs h{(long long)L, (long long)T, samples, acc_hist, (int *)div_hist, ctx->tgt.prec, nullptr, dl};
  const auto run = [&](auto launch, int64_t n_leapfrog, bool only_multi) -> int {
    if (int rc = profiled(ctx, st, launch)) return rc;
    return fill_n_leapfrog(ctx, C, n_leapfrog, T, out, only_multi, st);
  };
  if (path == HMC_PATH_FUSED_DENSE) {  // small dense problems: all T transitions in one launch (k_hmc_fused_dense), as for NUTS
    const bool tjoint = a.tkind == AEHMC_T_JOINT;
    const bool md = a.met_ndim == 2, td = a.tkind == AEHMC_T_DENSE_MVN, pc = md && ctx->met.per_chain;
    EngineArgs b = a;
    b.linear = 0;  // literal products (metrics.py:71)
    const KernelLaunch k = hmc_fused_dense_launch(md, td, pc, D, C, len != nullptr);
    if (pc) {  // the chains' transposed matrices
      if (int rc = grow(ctx, &ctx->fd_ws, &ctx->fd_ws_bytes, (size_t)C * D * D * sizeof(double))) return rc;
      h.imm_ws = ctx->fd_ws;
    }
#define AEHMC_FD_LAUNCH(MDV, TDV, PCV) \
  HIPCHK((len ? launch_hmc_fused_dense<MDV, TDV, PCV, true> : launch_hmc_fused_dense<MDV, TDV, PCV, false>)(k, b, h, st))
    return run([&](bool) -> int {
      if (tjoint) return rtc_launch(ctx, RTC_JHMC, k, st, b, h);  // the same kernel, compiled against the user's density
      if (md && td && pc) AEHMC_FD_LAUNCH(true, true, true);
      else if (md && td) AEHMC_FD_LAUNCH(true, true, false);
      else if (md && pc) AEHMC_FD_LAUNCH(true, false, true);
      else if (md) AEHMC_FD_LAUNCH(true, false, false);
      else AEHMC_FD_LAUNCH(false, true, false);
      return 0;
    }, total, true);
#undef AEHMC_FD_LAUNCH
  }
  if (path == HMC_PATH_GLM_ROWS) {  // row-reduction target with D <= 32, scalar / diagonal metric: all T transitions in one launch (glm_rows.cuh)
    const bool wg = glm_wg_wanted(ctx, D, C);
    const std::string name = glm_name(wg ? "k_hmc_glm_wg" : "k_hmc_glm_rows", D, wg);
    return run([&](bool) -> int {
      int waves = 0;
      if (wg)
        if (int rc = wg_program(ctx, RTC_GLMK, name, &waves)) return rc;
      return rtc_launch(ctx, {RTC_GLMK, waves}, name, wg ? dim3((unsigned)C) : chain_grid(C), dim3(wg ? 512 : 256), 0, st, a, h,
                        (const double *)ctx->glm_XT, ctx->glm_y, (long long)ctx->glm_N);
    }, L * T, false);
  }
  if (path == HMC_PATH_JOINT_WG) {  // traced joint density with long data sweeps, few chains: a workgroup per chain (k_hmc_joint_wg)
    return run([&](bool) -> int {
      int waves = 0;
      if (int rc = wg_program(ctx, RTC_JWG, RTC_JWG_HMC, &waves)) return rc;
      return rtc_launch(ctx, {RTC_JWG, waves}, RTC_JWG_HMC, dim3((unsigned)C), dim3(512), (size_t)2 * D * sizeof(double), st, a, h);
    }, L * T, false);
  }
  if (path == HMC_PATH_JOINT_ROWS) {  // all T transitions in one launch, the lock-step loop of a chain in one wavefront (k_hmc_joint_rows)
    return run([&](bool) -> int {
      return rtc_launch(ctx, RTC_JBASE, "aehmc::k_hmc_joint_rows", chain_grid(C), dim3(256), (size_t)8 * D * sizeof(double), st, a, h);
    }, L * T, false);
  }
  if (path == HMC_PATH_PC_DENSE) {  // all T transitions in one launch, the wavefront that owns a chain streaming its matrix (nuts_pc_dense.cuh)
    return run([&](bool) -> int { HIPCHK(tu::hmc_pc_dense(a, h, st)); return 0; }, L * T, false);
  }
  if (path == HMC_PATH_BLOCK_DENSE) {  // all T transitions in one launch, a workgroup per 16 chains, products on MFMA (nuts_block.cuh)
    if (int rc = grow(ctx, &ctx->blk_pack, &ctx->blk_pack_bytes, blk_pack_bytes(D))) return rc;
    double *bp = ctx->blk_pack;
    return run([&](bool) -> int {
      if (a.tkind == AEHMC_T_CUSTOM) {  // user-defined coordinate-wise target: the same kernels, compiled against the user's function (round 5)
        BlkMats mats;
        HIPCHK(blk_pack_matrices(a, nullptr, bp, mats, st));
        EngineArgs b = a;
        b.imm = mats.imm; b.sqrt_mass = mats.sqrt_mass;
        return rtc_launch(ctx, RTC_BLOCK, block_launch(/*nuts*/ false, ctx->opt_block_dense != 2, D, C, len != nullptr), st, b, h);
      }
      if (ctx->opt_block_dense != 2 && block_reg_supported(D)) HIPCHK(tu::hmc_block_reg(a, h, bp, st));
      else HIPCHK(tu::hmc_block_dense(a, h, bp, st));
      return 0;
    }, total, true);
  }
  for (int64_t t = 0; t < T; t++) {
    EngineArgs wa;  // whitened mode: each transition mapped in and out on its own (white_begin / white_end)
    WhiteBufs wb{};
    if (white)
      if (int rc = white_begin(ctx, a, wa, wb, st)) return rc;
    const EngineArgs &e = white ? wa : a;
    if (int rc = launch_begin(ctx, e, false, st)) return rc;
    for (int64_t l = 0; l < L; l++)
      if (int rc = launch_leapfrog(ctx, e, false, l == L - 1, st)) return rc;
    if (e.met_ndim == 2) LAUNCH(k_hmc_end<true>, C, st, e, (long long)L);
    else LAUNCH(k_hmc_end<false>, C, st, e, (long long)L);
    if (white)
      if (int rc = white_end(ctx, a, wb, st)) return rc;
    if (int rc = record_transition(ctx, C, D, t, q, out, samples, acc_hist, div_hist, st)) return rc;
  }
  return fill_n_leapfrog(ctx, C, L * T, T, out, true, st);
}

extern "C" int aehmc_hmc_step(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                              int64_t L, double divergence_threshold, double *q, double *U,
                              double *g, const aehmc_diagnostics *out, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  return hmc_run(ctx, C, rng, step_size, L, divergence_threshold, 1, q, U, g, out, nullptr, nullptr,
                 nullptr, (hipStream_t)stream);
}

extern "C" int aehmc_hmc_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                                int64_t L, double divergence_threshold, int64_t num_samples,
                                double *q, double *U, double *g, const aehmc_diagnostics *out,
                                double *samples, double *acceptance_history,
                                int32_t *divergence_history, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  return hmc_run(ctx, C, rng, step_size, L, divergence_threshold, num_samples, q, U, g, out, samples,
                 acceptance_history, divergence_history, (hipStream_t)stream);
}

// aehmc_hmc_sample with one trajectory length per transition: the lengths go into a ctx-owned device array on the
// caller's stream, and the kernels of the one-launch routes read transition t's from there
extern "C" int aehmc_hmc_sample_lengths(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size, const int64_t *lengths,
                                        double divergence_threshold, int64_t num_samples, double *q, double *U, double *g,
                                        const aehmc_diagnostics *out, double *samples, double *acceptance_history,
                                        int32_t *divergence_history, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (num_samples < 1) FAIL("number of transitions must be >= 1");
  if (!lengths) FAIL("lengths missing");
  HmcLens len{nullptr, 1, lengths, 0, 0};
  for (int64_t t = 0; t < num_samples; t++) {
    if (lengths[t] < 0) FAIL("num_integration_steps must be >= 0");
    if (lengths[t] > len.max) len.max = lengths[t];
    len.sum += lengths[t];
  }
  hipStream_t st = (hipStream_t)stream;
  if (int rc = grow(ctx, &ctx->hmc_lens, &ctx->hmc_lens_bytes, (size_t)num_samples * sizeof(int64_t))) return rc;
  HIPCHK(hipMemcpyAsync(ctx->hmc_lens, lengths, (size_t)num_samples * sizeof(int64_t), hipMemcpyHostToDevice, st));
  len.dev = (const long long *)ctx->hmc_lens;
  return hmc_run(ctx, C, rng, step_size, 0, divergence_threshold, num_samples, q, U, g, out, samples, acceptance_history,
                 divergence_history, st, &len);
}

// chees.run: num_steps x (q -> before; one HMC transition of state->num_steps leapfrogs; momentum . imm for a dense
// metric; aehmc_chees_update), enqueued in one call -- the same kernels in the same order as the caller's own loop
extern "C" int aehmc_chees_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps,
                                  double target_acceptance_rate, double learning_rate, int64_t max_num_steps,
                                  double inverse_mass_scalar, double divergence_threshold, double *q, double *U, double *g,
                                  const aehmc_diagnostics *out, const aehmc_chees_state *state, void *stream) {
  if (!ctx || !out || !state) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->has_tgt || !ctx->has_met) FAIL("set_target and set_metric must be called first");
  if (num_steps < 0) FAIL("chees: num_steps must be >= 0");
  if (max_num_steps < 1) FAIL("chees: max_num_steps must be at least 1");
  if (ctx->met.per_chain) FAIL("chees warm-up needs ONE shared metric bound");
  if (!state->step_size || !state->num_steps || ctx->eps_c != state->step_size || ctx->eps_n != C)
    FAIL("chees warm-up: the bound step sizes are not the adaptation state's own array (bind state->step_size with "
         "aehmc_set_step_sizes)");
  if (!out->momentum || !out->is_turning || !out->acceptance_probability)
    FAIL("chees warm-up needs out->momentum, out->is_turning (the accept flag) and out->acceptance_probability");
  const int64_t D = ctx->tgt.D;
  const int nd = ctx->met.ndim;
  const size_t vec = (size_t)C * D * sizeof(double);
  if (int rc = grow(ctx, &ctx->chees_loop, &ctx->chees_loop_bytes, (nd == 2 ? 2 : 1) * vec)) return rc;
  double *before = ctx->chees_loop, *prod = ctx->chees_loop + (size_t)C * D;
  const bool on_device = hmc_path_reads_lengths(hmc_path(ctx, C));
  const HmcLens len{(const long long *)state->num_steps, 0, nullptr, max_num_steps, 0};
  for (int64_t i = 0; i < num_steps; i++) {
    HIPCHK(hipMemcpyAsync(before, q, vec, hipMemcpyDeviceToDevice, st));
    if (on_device) {  // the transition reads the cell itself (clamped to max_num_steps, which init does not apply)
      if (int rc = hmc_run(ctx, C, rng, 0.0, 0, divergence_threshold, 1, q, U, g, out, nullptr, nullptr, nullptr, st, &len))
        return rc;
    } else {  // the route takes L from the host: the one int64 is read back, as chees.adaptation's caller does
      int64_t L = 0;
      HIPCHK(hipMemcpyAsync(&L, state->num_steps, sizeof(L), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      L = L < 0 ? 0 : (L > max_num_steps ? max_num_steps : L);
      if (int rc = hmc_run(ctx, C, rng, 0.0, L, divergence_threshold, 1, q, U, g, out, nullptr, nullptr, nullptr, st))
        return rc;
    }
    const double *mom = out->momentum;
    if (nd == 2) {  // (imm is symmetric: momentum . imm^T)
      if (int rc = gemm(ctx, C, D, D, out->momentum, D, ctx->met.imm, D, prod, D, st)) return rc;
      mom = prod;
    }
    if (int rc = aehmc_chees_update(ctx, C, D, i == num_steps - 1, target_acceptance_rate, learning_rate, max_num_steps,
                                    before, q, mom, nd == 1 ? ctx->met.imm : nullptr,
                                    nd == 2 ? 1.0 : (nd == 1 ? 0.0 : inverse_mass_scalar), out->is_turning,
                                    out->acceptance_probability, state, stream))
      return rc;
  }
  return 0;
}

// ---- generalised HMC (ghmc_fused.cuh) and its MEADS warm-up (meads.cuh) ----
// T transitions in one launch; `params`: eps, alpha, delta on the device
static int ghmc_run(aehmc_ctx *ctx, int64_t C, uint64_t *rng, const double *params, const double *scale, int64_t scale_n,
                    double divergence_threshold, int64_t T, double *q, double *U, double *g, double *momentum,
                    int32_t has_momentum, double *slice, int32_t has_slice, const aehmc_diagnostics *out, double *samples,
                    double *acc_hist, int32_t *div_hist, hipStream_t st) {
  if (T < 1) FAIL("ghmc: number of transitions must be >= 1");
  if (C < 1 || !rng || !params || !scale || !q || !U || !g || !momentum || !slice) FAIL("ghmc: bad arguments");
  if (!out->acceptance_probability || !out->is_diverging) FAIL("diagnostics arrays missing");
  if (!ctx->has_tgt) FAIL("set_target must be called first");
  const int64_t D = ctx->tgt.D;
  const int tkind = ctx->tgt.kind;
  if (D > GHMC_MAX_D)
    FAIL("ghmc: D = " + std::to_string(D) + " is above the " + std::to_string(GHMC_MAX_D) +
         " coordinates a wavefront holds in registers (k_ghmc_fused); there is no other route");
  if (scale_n != 1 && scale_n != D)
    FAIL("ghmc: the scale is ONE scalar or [D] vector shared by all chains (scale_n = 1 or D), got " + std::to_string(scale_n) +
         " entries; dense and per-chain preconditioners are not supported");
  GhmcArgs f{};
  f.C = C; f.D = D; f.T = T; f.thr = divergence_threshold; f.params = params; f.scale = scale; f.scale_n = (int)scale_n;
  f.rng = rng; f.q = q; f.U = U; f.g = g; f.v = momentum; f.slice = slice; f.has_v = has_momentum; f.has_slice = has_slice;
  f.out = *out; f.samples = samples; f.acc_hist = acc_hist; f.div_hist = div_hist;
  if (ghmc_target_is_elem(tkind)) {
    f.tkind = tkind; f.mu = ctx->tgt.mu; f.sigma = ctx->tgt.sigma; f.log_sigma = ctx->log_sigma;
    return profiled(ctx, st, [&](bool) -> int { HIPCHK(tu::ghmc_fused(f, st)); return 0; });
  }
  if (tkind == AEHMC_T_CUSTOM) {  // user-defined coordinate-wise target: the kernel compiled against the user's function
    f.tkind = AEHMC_T_CUSTOM; f.cparams = ctx->bound.d_cparams;
    return profiled(ctx, st, [&](bool) -> int { return rtc_launch(ctx, RTC_GHMC, ghmc_fused_launch(D, AEHMC_T_CUSTOM, C), st, f); });
  }
  if (tkind == AEHMC_T_JOINT) {
    if (!ctx->bound.has_grad)
      FAIL("ghmc: a joint density needs its reverse-mode program (AEHMC_JOINT_GRAD: a traced Python function, "
           "targets.from_callable(..., reverse=True) below 65 coordinates); forward mode is not supported");
    f.tkind = AEHMC_T_JOINT; f.cparams = ctx->bound.d_cparams;
    return profiled(ctx, st, [&](bool) -> int { return rtc_launch(ctx, RTC_JGHMC, ghmc_fused_launch(D, AEHMC_T_JOINT, C), st, f); });
  }
  FAIL("ghmc: the bound target (kind " + std::to_string(tkind) + ") is not supported: generalised HMC runs the "
       "coordinate-wise targets, targets.Custom and joint densities with a reverse-mode program (no dense MVN, regression "
       "or GLM target)");
}

extern "C" int aehmc_ghmc_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, const double *params, double step_size,
                                 double alpha, double delta, const double *scale, int64_t scale_n,
                                 double divergence_threshold, int64_t num_samples, double *q, double *U, double *g,
                                 double *momentum, int32_t has_momentum, double *slice, int32_t has_slice,
                                 const aehmc_diagnostics *out, double *samples, double *acceptance_history,
                                 int32_t *divergence_history, void *stream) {
  if (!ctx || !out) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (!params) {  // host numbers: into the ctx's own cell on the caller's stream, then the one code path
    if (!(step_size > 0)) FAIL("ghmc: step_size must be positive");
    if (!(alpha > 0 && alpha <= 1)) FAIL("ghmc: alpha must lie in (0, 1]");
    if (!(delta >= 0)) FAIL("ghmc: delta must be >= 0");
    if (int rc = grow(ctx, &ctx->ghmc_cell, &ctx->ghmc_cell_bytes, 3 * sizeof(double))) return rc;
    HIPCHK(tu::meads_set3(ctx->ghmc_cell, step_size, alpha, delta, st));
    params = ctx->ghmc_cell;
  }
  return ghmc_run(ctx, C, rng, params, scale, scale_n, divergence_threshold, num_samples, q, U, g, momentum, has_momentum,
                  slice, has_slice, out, samples, acceptance_history, divergence_history, st);
}

extern "C" int aehmc_meads_update(aehmc_ctx *ctx, int64_t C, int64_t D, const double *position,
                                  const double *potential_energy_grad, double step_size_multiplier, double damping_slowdown,
                                  const aehmc_meads_state *state, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (!state || D <= 0 || !position || !potential_energy_grad) FAIL("meads: bad arguments");
  if (C < 2) FAIL("meads: the cross-chain statistics need at least 2 chains");
  if (!state->params || !state->scale || !state->count || !state->skipped) FAIL("meads: state arrays missing");
  if (!(step_size_multiplier > 0)) FAIL("meads: step_size_multiplier must be positive");
  MeadsArgs a;
  memset(&a, 0, sizeof(a));
  a.C = C; a.D = D; a.multiplier = step_size_multiplier; a.slowdown = damping_slowdown;
  a.Q = position; a.G = potential_energy_grad; a.s = *state;
  pool_parts(C, D, a.P, a.rows_per);
  if (int rc = grow(ctx, &ctx->meads_work, &ctx->meads_work_bytes, meads_work_doubles(C, D) * sizeof(double))) return rc;
  a.part = ctx->meads_work;
  a.m = a.part + (size_t)a.P * D;
  a.sd = a.m + D;  // (adjacent: k_meads_scalars copies both at once)
  a.fro = a.sd + D;
  a.nz = a.fro + 2 * D;
  a.ng = a.nz + C;
  a.Sz = a.ng + C;
  a.Sg = a.Sz + (size_t)D * D;
  HIPCHK(hipMemsetAsync(a.Sz, 0, (size_t)2 * D * D * sizeof(double), st));
  HIPCHK(tu::meads_means(a, st));
  if (int rc = syrk(ctx, C, D, position, D, a.m, 0.0, nullptr, nullptr, a.Sz, D, st)) return rc;
  if (int rc = syrk(ctx, C, D, potential_energy_grad, D, nullptr, 0.0, nullptr, nullptr, a.Sg, D, st)) return rc;
  HIPCHK(tu::meads_finish(a, st));
  return 0;
}

extern "C" int aehmc_meads_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, double step_size_multiplier,
                                  double damping_slowdown, double divergence_threshold, double *q, double *U, double *g,
                                  double *momentum, int32_t has_momentum, double *slice, int32_t has_slice,
                                  const aehmc_diagnostics *out, const aehmc_meads_state *state, void *stream) {
  if (!ctx || !out || !state) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->has_tgt) FAIL("set_target must be called first");
  if (num_steps < 0) FAIL("meads: num_steps must be >= 0");
  const int64_t D = ctx->tgt.D;
  if (int rc = aehmc_meads_update(ctx, C, D, q, g, step_size_multiplier, damping_slowdown, state, stream)) return rc;
  for (int64_t i = 0; i < num_steps; i++) {
    if (int rc = ghmc_run(ctx, C, rng, state->params, state->scale, D, divergence_threshold, 1, q, U, g, momentum,
                          has_momentum || i > 0, slice, has_slice || i > 0, out, nullptr, nullptr, nullptr, (hipStream_t)stream))
      return rc;
    if (int rc = aehmc_meads_update(ctx, C, D, q, g, step_size_multiplier, damping_slowdown, state, stream)) return rc;
  }
  return 0;
}

// window_adaptation.run around an HMC kernel (window_adaptation.py:66: `kernel(chain_state, *parameters)` with the
// trajectory length closed over): num_steps x (one HMC transition with the current per-chain parameters, then
// aehmc_adapt_update), enqueued in one call -- the same kernels in the same order as the caller's own loop
extern "C" int aehmc_hmc_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, const int32_t *stage,
                                const int32_t *is_window_end, double target_acceptance_rate,
                                int64_t num_integration_steps, double divergence_threshold, double *q, double *U,
                                double *g, const aehmc_diagnostics *out, const aehmc_adapt_state *state,
                                void *stream) {
  if (int rc = warmup_bound(ctx, C, out, state, stage, is_window_end)) return rc;
  return warmup_loop(ctx, C, num_steps, stage, is_window_end, target_acceptance_rate, q, out, state, stream, false,
                     aehmc_adapt_update, [&] {
                       return hmc_run(ctx, C, rng, 0.0, num_integration_steps, divergence_threshold, 1, q, U, g, out,
                                      nullptr, nullptr, nullptr, (hipStream_t)stream);
                     });
}

// window_adaptation.run(..., pooled=True): the transitions run with ONE shared metric and one step size (every entry of
// state->step_size), on whatever route nuts_run / hmc_run give such a binding; the pooled update follows each
extern "C" int aehmc_nuts_warmup_pooled(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps,
                                        const int32_t *stage, const int32_t *is_window_end,
                                        double target_acceptance_rate, int64_t max_num_expansions,
                                        double divergence_threshold, double *q, double *U, double *g,
                                        const aehmc_diagnostics *out, const aehmc_pooled_adapt_state *state,
                                        void *stream) {
  if (int rc = warmup_bound(ctx, C, out, state, stage, is_window_end)) return rc;
  return warmup_loop(ctx, C, num_steps, stage, is_window_end, target_acceptance_rate, q, out, state, stream, true,
                     aehmc_pooled_adapt_update, [&] {
                       return nuts_run(ctx, C, rng, 0.0, max_num_expansions, divergence_threshold, q, U, g, out,
                                       (hipStream_t)stream);
                     });
}
extern "C" int aehmc_hmc_warmup_pooled(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps,
                                       const int32_t *stage, const int32_t *is_window_end,
                                       double target_acceptance_rate, int64_t num_integration_steps,
                                       double divergence_threshold, double *q, double *U, double *g,
                                       const aehmc_diagnostics *out, const aehmc_pooled_adapt_state *state,
                                       void *stream) {
  if (int rc = warmup_bound(ctx, C, out, state, stage, is_window_end)) return rc;
  return warmup_loop(ctx, C, num_steps, stage, is_window_end, target_acceptance_rate, q, out, state, stream, true,
                     aehmc_pooled_adapt_update, [&] {
                       return hmc_run(ctx, C, rng, 0.0, num_integration_steps, divergence_threshold, 1, q, U, g, out,
                                      nullptr, nullptr, nullptr, (hipStream_t)stream);
                     });
}

extern "C" int aehmc_leapfrog(aehmc_ctx *ctx, int64_t C, double step_size, int64_t nsteps, double *q,
                              double *p, double *U, double *g, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EngineArgs a;
  if (int rc = fill_args(ctx, C, 1, a)) return rc;
  a.eps = step_size;
  a.linear = 0;                           // building block: literal metric products
  a.cur_q = q; a.cur_p = p; a.cur_g = g;  // integrate the caller's arrays in place
  LAUNCH(k_ctl_set, C, st, a, (const double *)U);
  for (int64_t l = 0; l < nsteps; l++)
    if (int rc = launch_leapfrog(ctx, a, false, false, st)) return rc;
  LAUNCH(k_ctl_get_U, C, st, a, U);
  return 0;
}

extern "C" int aehmc_kinetic_energy(aehmc_ctx *ctx, int64_t C, const double *p, double *K, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EngineArgs a;
  if (int rc = fill_args(ctx, C, 1, a)) return rc;
  if (a.met_ndim == 2) {
    if (metric_mul(ctx, C, p, ctx->met.imm, a.vhalf, st)) return -1;
  } else {
    LAUNCH(k_vel_diag, C, st, a, p, a.vhalf);
  }
  LAUNCH(k_half_dot, C, st, a, (const double *)a.vhalf, p, K);
  return 0;
}

extern "C" int aehmc_is_turning(aehmc_ctx *ctx, int64_t C, const double *pl, const double *pr,
                                const double *ps, int32_t *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  EngineArgs a;
  if (int rc = fill_args(ctx, C, 1, a)) return rc;
  if (a.met_ndim == 2) {
    if (metric_mul(ctx, C, pl, ctx->met.imm, a.vhalf, st)) return -1;
    if (metric_mul(ctx, C, pr, ctx->met.imm, a.zbuf, st)) return -1;
  } else {
    LAUNCH(k_vel_diag, C, st, a, pl, a.vhalf);
    LAUNCH(k_vel_diag, C, st, a, pr, a.zbuf);
  }
  LAUNCH(k_is_turning, C, st, a, pl, pr, ps, (const double *)a.vhalf, (const double *)a.zbuf, out);
  return 0;
}

extern "C" int aehmc_rng_normals(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t n, double *out,
                                 void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_rng_normals, chain_grid(C), dim3(256), 0, (hipStream_t)stream, rng,
                     (long long)C, (long long)n, out);
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aehmc_rng_bernoulli(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t n,
                                   const double *p, int32_t *out, void *stream) {
  if (!ctx) return -2;
  HIPCHK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_rng_bernoulli, chain_grid(C), dim3(256), 0, (hipStream_t)stream, rng,
                     (long long)C, (long long)n, p, out);
  HIPCHK(hipGetLastError());
  return 0;
}
