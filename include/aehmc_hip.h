/* aehmc_hip.h -- C-ABI of the MI355X (gfx950) many-chain HMC/NUTS trajectory engine.
 *
 * Drop-in boundary for the leapfrog hot path of aesara-devs/aehmc.  The
 * reference has no FFI of its own: its boundary is the Python API
 *     aehmc/hmc.py:16   new_state(q, logprob_fn)
 *     aehmc/hmc.py:43   hmc.new_kernel(srng, logprob_fn, divergence_threshold)
 *     aehmc/hmc.py:77   step(state, step_size, inverse_mass_matrix, num_integration_steps)
 *     aehmc/nuts.py:17  nuts.new_kernel(srng, logprob_fn, max_num_expansions, divergence_threshold)
 *     aehmc/nuts.py:56  step(state, step_size, inverse_mass_matrix)
 * and everything those build symbolically (integrators.py, metrics.py, trajectory.py,
 * termination.py, proposals.py).  The entry points below are what a ctypes binding of
 * that path binds; aehmc_amd/{hmc,nuts}.py are thin wrappers.
 *
 * Conventions
 *  - every call returns 0 on success, <0 on error (aehmc_last_error gives the text);
 *    nothing throws across the ABI.  Numerical failure is data (is_diverging), not an
 *    error (reference: proposals.py:43-45, hmc.py:189-191).
 *  - all array arguments are DEVICE pointers owned by the caller (hipMalloc or a
 *    torch-ROCm tensor's data_ptr); chain-major row layout [C, D], float64.  The
 *    library owns only the ctx and the workspace the caller hands it.
 *  - `stream` is a hipStream_t passed as void*; work is enqueued on it in order.  NUTS
 *    polls a pinned "chains still active" word to stop launching early, so a NUTS call
 *    may block the host for part of its duration; results are complete on `stream`.
 *  - a ctx is not thread-safe; distinct ctxs are independent; no global state.  ONE STREAM PER CTX at a time: the
 *    ctx owns scratch that every call rewrites on the call's stream (the packed matrices of the block-resident dense
 *    kernels, per-chain factorisation scratch, the GLM work arrays), so calls on two streams may only share a ctx if
 *    the caller orders them (events); use one ctx per stream otherwise.
 *  - RNG ("scheme A"): per chain, one PCG64 per RNG call site of the
 *    reference graph, in graph-construction order; rng is uint64 [C, n_sites, 4] =
 *    (state_hi, state_lo, inc_hi, inc_lo), advanced in place exactly as numpy's
 *    Generator.normal / Generator.binomial(1, p) would advance it.
 */
#ifndef AEHMC_HIP_H
#define AEHMC_HIP_H

#ifndef __HIPCC_RTC__  /* (hipRTC supplies the runtime, the math functions and the fixed-width integers itself) */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aehmc_ctx aehmc_ctx;

/* logprob_fn stand-ins (arbitrary Python callables cannot be compiled to HIP) */
enum aehmc_target_kind {
  AEHMC_T_STD_NORMAL = 0,   /* aeppl N(0,1) per coordinate: U = sum 0.5 q^2 + log sqrt(2 pi)  (README.md:27-36) */
  AEHMC_T_ISO_GAUSSIAN = 1, /* U = 0.5 |q|^2 (tests/test_trajectory.py:150-151) */
  AEHMC_T_DIAG_GAUSSIAN = 2,/* N(mu, diag sigma^2) */
  AEHMC_T_DENSE_MVN = 3,    /* U = 0.5 (q-mu)^T P (q-mu), P dense symmetric [D,D] */
  AEHMC_T_LINREG = 4,       /* examples/LinearRegression.ipynb:126-166, q = [w, log n] */
  AEHMC_T_CUSTOM = 5,       /* user-defined coordinate-wise target, compiled at run time: aehmc_set_custom_target */
  AEHMC_T_GLM = 6,          /* user-defined row-reduction target over a data matrix: aehmc_set_custom_glm_target */
  AEHMC_T_JOINT = 7,        /* user-defined JOINT (non-separable) log-density, D <= 2048 (10176 with a reverse-mode
                               program), differentiated by the engine: aehmc_set_custom_joint_target */
  AEHMC_T_WHITE_EIGEN = 8   /* the engine's own: dU/dy_i = lambda_i y_i, U = 0.5 sum y_i dU/dy_i -- a whitened dense MVN in
                               the eigenbasis of its operator ("dense_eigen").  Not accepted by aehmc_set_target */
};

typedef struct {
  int32_t kind;          /* aehmc_target_kind */
  int32_t reserved;
  int64_t D;             /* position dimension */
  const double *mu;      /* [D]   diag / dense */
  const double *sigma;   /* [D]   diag */
  const double *prec;    /* [D,D] dense, row-major */
  const double *X;       /* [N]   linreg (16-byte aligned) */
  const double *y;       /* [N]   linreg (16-byte aligned) */
  int64_t N;
} aehmc_target;

/* gaussian_metric(inverse_mass_matrix) -- metrics.py:10-106.  ndim 0/1/2 = scalar /
 * diagonal / dense exactly as metrics.py:44-63; sqrt_mass is sqrt(1/imm) (ndim<2) or
 * L^-T with imm = L L^T (metrics.py:56-58).  Dense imm must be symmetric. */
typedef struct {
  int32_t ndim;
  int32_t per_chain;       /* 1: imm / sqrt_mass are [C,1] (ndim 0), [C,D] (ndim 1) or [C,D,D]
                              (ndim 2, D <= 2048), one per chain -- what per-chain window
                              adaptation produces; sqrt_mass must be given
                              (aehmc_metric_sqrt_per_chain computes the dense one); 0: shared */
  int64_t D;
  const double *imm;       /* [1] | [D] | [D,D] */
  const double *sqrt_mass; /* [1] | [D] | [D,D], or NULL: aehmc_set_metric computes it on the
                              device (dense: blocked Cholesky + triangular inverse on the fp64
                              MFMA GEMM) into ctx-owned memory */
  int64_t n_chains;        /* per_chain: number of rows C of imm / sqrt_mass (the step calls
                              refuse a different chain count); 0 when shared */
} aehmc_metric;

/* warm-up state of window_adaptation.run (window_adaptation.py:17-116), one row per chain:
 * DualAveragingState (algorithms.py:9-14), Welford state (algorithms.py:141-165) and the
 * current parameters (step_size, inverse_mass_matrix [+ its sqrt-mass]) */
typedef struct {
  int64_t *da_step;                      /* [C] */
  double *da_x, *da_x_avg, *da_g_avg, *da_mu; /* [C] */
  double *wc_mean, *wc_m2;               /* [C,D] (diagonal adaptation) */
  int64_t *wc_n;                         /* [C] */
  double *step_size;                     /* [C] */
  double *imm, *sqrt_mass;               /* [C,D] */
  int32_t full;                          /* 1: is_mass_matrix_full -- wc_m2, imm and sqrt_mass are
                                            [C,D,D] (full covariance per chain, D <= 2048) */
  int32_t reserved;
  double *work;                          /* full && D > 64: [C,D,D] scratch of the window-end
                                            factorisation (smaller D: LDS; may be NULL) */
} aehmc_adapt_state;

/* warm-up state of window_adaptation.run(..., pooled=True): ONE adaptation from all chains together -- one
 * DualAveragingState, one Welford state, one inverse mass matrix (shared shapes); only step_size has a chain axis: the
 * update writes the ONE step size into all C entries, the array aehmc_set_step_sizes binds */
typedef struct {
  int64_t *da_step;                      /* [1] */
  double *da_x, *da_x_avg, *da_g_avg, *da_mu; /* [1] */
  double *wc_mean, *wc_m2;               /* [D], [D] (diagonal adaptation) */
  int64_t *wc_n;                         /* [1]: draws in the Welford state (a multiple of C) */
  double *step_size;                     /* [C], all entries equal */
  double *imm, *sqrt_mass;               /* [D] */
  int32_t full;                          /* 1: is_mass_matrix_full -- wc_m2, imm and sqrt_mass are [D,D]; of wc_m2 only
                                            the lower triangle is kept up (its upper one is unspecified) */
  int32_t reserved;
} aehmc_pooled_adapt_state;

/* warm-up state of chees.run: ONE trajectory length and ONE step size adapted from all chains (ChEES-HMC); every array
 * is [1] but step_size */
typedef struct {
  int64_t *step;                         /* n >= 1: the update about to run */
  double *log_T, *log_T_avg;             /* log trajectory length, its weighted average */
  double *adam_m, *adam_v;               /* Adam moments of the ascent on log_T */
  double *h;                             /* Halton weight of the transition the next update will see */
  int64_t *num_steps;                    /* L of that transition: max(1, ceil(h T / step size)), capped */
  int64_t *da_step;                      /* dual averaging, as in aehmc_pooled_adapt_state */
  double *da_x, *da_x_avg, *da_g_avg, *da_mu;
  double *step_size;                     /* [C], all entries equal */
  double *sums;                          /* NULL, or [3 + 2 D]: a copy of what the last update summed -- S, A, abar,
                                            then the column means m0 [D] and m1 [D] (diagnostics; the update itself
                                            runs the same either way) */
} aehmc_chees_state;

/* state of the MEADS warm-up (meads.run): the four parameters of generalised HMC, adapted from all chains.  Before the
 * first update the caller fills params = (initial step size, 1, 0.5), scale = 1, count = skipped = 0. */
typedef struct {
  double *params;                        /* [3]: step size eps, momentum refreshment alpha, slice drift delta */
  double *scale;                         /* [D]: the preconditioner s, in the role of sqrt(inverse_mass_matrix) */
  int64_t *count;                        /* [1]: updates done so far */
  int64_t *skipped;                      /* [1]: of them, those the guard refused (parameters left as they were) */
  double *sums;                          /* NULL, or [8 + 2 D]: a copy of what the last update summed -- sum |z_c|^4,
                                            sum |z_c|^2, sum |gs_c|^4, sum |gs_c|^2, the two scaled Frobenius sums (Z, Gs),
                                            lam(Z), lam(Gs), then the column means m [D] and sd [D] (diagnostics) */
} aehmc_meads_state;

/* per-transition outputs == trajectory.py:379-384 Diagnostics (+ n_leapfrog) */
typedef struct {
  double *momentum;               /* [C,D] Diagnostics.state.momentum */
  double *acceptance_probability; /* [C] */
  int64_t *num_doublings;         /* [C] NUTS only (may be NULL for HMC) */
  int32_t *is_turning;            /* [C] NUTS only (may be NULL for HMC) */
  int32_t *is_diverging;          /* [C] */
  int64_t *n_leapfrog;            /* [C] integrator calls that belong to the trajectory */
} aehmc_diagnostics;

int aehmc_create(aehmc_ctx **out, int device);
int aehmc_destroy(aehmc_ctx *ctx);
const char *aehmc_last_error(const aehmc_ctx *ctx);

/* bind logprob_fn / inverse_mass_matrix (device buffers must outlive their use) */
int aehmc_set_target(aehmc_ctx *ctx, const aehmc_target *target);

/* A USER-DEFINED coordinate-wise logprob_fn (hmc.py:16-40 takes any callable; its gradient comes from autodiff,
 * integrators.py:61-65): `source` is HIP source that defines the device function `aehmc_custom_elem`,
 *     __device__ void aehmc_custom_elem
 *         (double q, long long i, const double *const *prm, double &u, double &g)
 * -- the contribution u of coordinate i to the potential energy U = -logprob(q) = sum_i u_i and du_i/dq_i = g --
 * with prm[k] the k-th of `n_params` device arrays (`params`: HOST array of device pointers; [D] each, or whatever the
 * function indexes).  The library compiles its kernel templates against it with hipRTC (libhiprtc, gfx950;
 * `include_dir` = the directory that holds the library's csrc/ headers) on first use and caches the code objects by
 * source: the lock-step engine (any metric, any D), the register-resident NUTS kernel (D <= 512, diagonal / scalar
 * metric) and the fused HMC kernel (D <= 1024, diagonal / scalar metric) and, since round 5, the workgroup-per-chain
 * NUTS / HMC kernels (diagonal / scalar metric, D <= 10176 / 10240) and the block-resident NUTS / HMC kernels (shared
 * dense metric, 64 < D <= 512).  The density alone is enough: with `#include "dual.cuh"` the source may define
 *     template <class T> __device__ T aehmc_logp
 *         (T q, long long i, const double *const *prm)
 * and a three-line aehmc_custom_elem that instantiates it with aehmc::Dual (what aehmc_amd/targets.py appends).
 * Compilation errors come back through aehmc_last_error with the compiler's log, and the previous binding stays. */
int aehmc_set_custom_target(aehmc_ctx *ctx, const char *source, int64_t D, const double *const *params,
                            int32_t n_params, const char *include_dir);

/* A user-defined ROW-REDUCTION ("GLM-type") logprob_fn over a data matrix X [N,D] (row-major, device) and responses
 * y [N] (device):  U(q) = sum_n loss(x_n . q, y_n) + sum_i prior(q_i),  dU/dq = X^T dloss/dz + prior'(q).  `source`
 * defines the device functions `aehmc_glm_row` and `aehmc_glm_prior`,
 *     __device__ void aehmc_glm_row
 *         (double z, double y, long long n, const double *const *prm, double &loss, double &dloss_dz)
 *     __device__ void aehmc_glm_prior
 *         (double q, long long i, const double *const *prm, double &u, double &g)
 * (logistic regression: loss = log1p(exp(z)) - y z, dloss = 1 / (1 + exp(-z)) - y).  Per leapfrog the two products
 * with X run as chain-batched fp64 MFMA GEMMs (Z = Q X^T, then G = dLoss X), the user's functions in run-time
 * compiled kernels between and behind them; lock-step engine (any metric).  The library keeps a transposed copy of X
 * and a [C, N] work array. */
/* (round 5: with D <= 32 and a scalar / diagonal metric NUTS and HMC run whole calls in ONE launch -- the wavefront that owns
 * a chain sweeps the rows itself, k_nuts_glm_rows / k_hmc_glm_rows -- when D <= 16 or the call has <= 1024 chains) */
int aehmc_set_custom_glm_target(aehmc_ctx *ctx, const char *source, int64_t D, int64_t N, const double *X,
                                const double *y, const double *const *params, int32_t n_params,
                                const char *include_dir);

/* A user-defined JOINT logprob_fn (reference: aehmc/hmc.py:16-40 takes any callable and differentiates it,
 * hmc.py:33-34, integrators.py:61-65): the user writes the log-DENSITY only, the engine differentiates it.  `source`
 * is HIP source that includes "dual.cuh" and defines
 *     template <class V> __device__ auto aehmc_logp
 *         (const V &q, const double *const *prm)
 * with q[i] the coordinates (i wave-uniform) and q.size() = D <= 2048 -- hierarchical models, funnels, anything that is
 * not a sum over coordinates or data rows.  Forward mode: lane i of the chain's wavefront evaluates the density with
 * the derivative seeded at coordinate i (csrc/dual.cuh), so for D <= 64 ONE evaluation per leapfrog yields U = -logp and
 * the whole gradient: the single-launch kernels of small problems (k_nuts_resident / k_hmc_fused_dense compiled against
 * it: scalar, diagonal or dense metric, shared or per chain, any number of transitions per launch) and new_state.
 * Above 64 coordinates, and with options resident_nuts / fused_hmc = 0, the density is evaluated on the lock-step path
 * between the stage kernels (k_target_joint_rows: the chain's row in LDS, ceil(D / 64) evaluations per gradient, lane l
 * seeding coordinate l + 64 k in pass k): any metric, O(D^2 / 64) density terms per leapfrog and chain; with a scalar or
 * diagonal metric the same loop runs for one chain per wavefront in one launch per call (k_nuts_joint_rows up to
 * D = 192, k_hmc_joint_rows at any D; bitwise the lock-step path).
 * A source with a reverse-mode program (#define AEHMC_JOINT_GRAD: aehmc_logp_grad_t, emitted by aehmc_amd/tracing.py)
 * may have up to 10176 coordinates.  Above 2048 one chain's position and gradient rows fill a workgroup's LDS: NUTS and
 * HMC with a scalar / diagonal metric run k_nuts_wide / k_hmc_wide compiled against the program (option "joint_wide"),
 * new_state and the lock-step path (a shared dense metric) evaluate it a workgroup per chain (k_target_joint_wg). */
int aehmc_set_custom_joint_target(aehmc_ctx *ctx, const char *source, int64_t D, const double *const *params,
                                  int32_t n_params, const char *include_dir);

/* Code objects of run-time compiled programs (the three entry points above) are kept in `dir` across processes: a file
 * per program, named by a hash of everything the compiler saw (source, options, kernel names).  The caller chooses a
 * directory that is specific to the library's own sources -- the headers a program includes (aehmc_amd/engine.py uses
 * ~/.cache/aehmc_amd/rtc-<source hash>).  NULL or "" switches the cache off (default). */
int aehmc_set_rtc_cache(aehmc_ctx *ctx, const char *dir);
/* How many run-time programs this ctx compiled with hipRTC and how many it took from the directory above (either
 * pointer may be NULL): what a caller checks to know that a second process did not recompile -- a count, not a time. */
int aehmc_rtc_stats(const aehmc_ctx *ctx, int64_t *compiled, int64_t *loaded_from_cache);
int aehmc_set_metric(aehmc_ctx *ctx, const aehmc_metric *metric);

/* engine options (name, default):
 *  "fused_hmc" 1    register-resident single-launch HMC when the metric is diagonal and the
 *                   target coordinate-wise, or the problem small and dense (D <= 64, see
 *                   "resident_nuts"); 0 forces the lock-step path
 *  "resident_nuts" 2 register-resident single-launch NUTS (a team of 1..64 lanes, or a
 *                   256/512-thread workgroup for large D, keeps the chain's moving state on chip
 *                   for the whole tree) for diagonal/scalar metrics, coordinate-wise
 *                   targets, D <= 10176, and the regression target (four chains per workgroup
 *                   share each pass over the data rows), and for small dense problems (D <= 64: a
 *                   dense inverse mass matrix -- shared or one per chain -- and / or the dense-precision
 *                   target, products inside the wavefront).  2 (auto) = 1 = wherever such a kernel exists
 *                   (round 3: it beats the lock-step path at every chain count), 0 = never
 *  "resident_min_team" 0  1: always give a chain the smallest team of lanes that holds it
 *                   (64/T chains per wavefront) instead of widening teams while the GPU would
 *                   otherwise run fewer than ~4096 wavefronts
 *  "fused_nuts" 0   1: whole NUTS transition in one launch (one wavefront per chain loops
 *                   leapfrog + tree bookkeeping over its HBM-resident state) when the metric is
 *                   diagonal and the target coordinate-wise -- lowest latency for a few
 *                   chains; the lock-step path (one launch per leapfrog) has the higher
 *                   throughput for thousands of chains and is the default
 *  "dense_linear" 1 dense metric: carry w = imm g with the state so that
 *                   v_half = v - (eps/2) w, v' = v_half - (eps/2) w' (one metric GEMM per
 *                   leapfrog); 0 forms imm p_half and imm p' directly as metrics.py:71 does
 *  "dense_whiten" 1 dense-precision Gaussian target (AEHMC_T_DENSE_MVN) under a shared dense inverse mass matrix,
 *                   "dense_linear" = 1, D > 512, lock-step path (NUTS and HMC): every transition maps the state to
 *                   z = L^-1 (q - mu), r = L^T p with imm = L L^T, runs its leapfrogs there -- a Gaussian of
 *                   precision H = L^T P L under the identity metric, ONE chain-batched product per leapfrog -- and
 *                   maps back: q = mu + L z, p = L^-T r, U and dU/dq evaluated afresh at q (as aehmc_new_state does);
 *                   a chain whose returned point is its initial one returns the caller's q, U, dU/dq unchanged.
 *                   Same discrete outputs and RNG consumption, reals equal up to rounding.  L, L^-1 and H are formed
 *                   from the BOUND arrays (prec, imm, sqrt_mass) once per binding and dropped by aehmc_set_target /
 *                   aehmc_set_metric: a caller who edits them in place must bind them again.  0 = two products per
 *                   leapfrog in the original coordinates
 *  "dense_whiten_carry" 1  whitened mode: the engine keeps, in the workspace, the state a transition returned next to
 *                   the whitened pair (z, H z) it came from.  A chain that enters the next whitened call with exactly
 *                   that q, U and dU/dq (compared bit for bit on the device, per chain) continues from the pair
 *                   instead of forming z = L^-1 (q - mu) and H z again; every other chain is mapped in as before.
 *                   After aehmc_set_target / aehmc_set_metric the record survives only if the operator formed
 *                   from the new arrays (L, L^-1, H, mu) is the old one bit for bit: results follow the content of the
 *                   bound arrays, not which arrays hold it (the old operator is held until the next whitened call
 *                   has compared it).  The record is dropped by anything that replaces the workspace or may write it (any other call that uses the workspace, another chain count or tree
 *                   depth).  Same discrete outputs, reals equal up to rounding (z is not rounded through q).
 *                   0 = every transition maps in from q
 *  "dense_whiten_ahead" 1  whitened mode, NUTS: the lock-step's bookkeeping pass also forms the chain's next half step
 *                   (p_half, z') from the values it holds, in a momentum vector of its own and a second position
 *                   buffer (two workspace vectors the mode left unused: the workspace does not grow), instead of a
 *                   second pass that reads them back; a chain that turns round forms it from its new rows.  The same
 *                   operations on the same bits: every output and the generator states equal 0's bit for bit.
 *                   0 = the two-pass stage
 *  "dense_eigen" 1  whitened mode, NUTS: H = L^T P L is the same matrix in every leapfrog of every call while target
 *                   and metric stay bound, so it is factored ONCE, H = V diag(lambda) V^T, and the transition runs in
 *                   y = V^T z, s = V^T r -- a coordinate-wise Gaussian of precisions lambda_i under the identity
 *                   metric, on the diagonal lock-step stage: no product inside the loop.  A transition keeps its
 *                   boundary products: s = V^T r (r: the raw normals, drawn as before), y0 = V^T L^-1 (q0 - mu) on the
 *                   chains the carry record does not cover, and at the end q = mu + (L V) y, p = (L^-T V) s, and
 *                   (U, dU/dq) afresh at q.  Same discrete outputs and generator states, reals equal up to rounding.
 *                   1 = wherever the whitened mode applies and D >= 2048; 2 = wherever it applies (D > 512); 0 = off.
 *                   The basis comes from rocsolver_dsyevd, looked up at run time (no link-time dependency), or from
 *                   the caller (aehmc_set_white_basis); either is checked on the device before use (max |V^T V - I|,
 *                   max |H V - V diag(lambda)| / max |lambda|).  Without a solver, or with a basis that fails the
 *                   check, the whitened route runs: aehmc_white_basis_info says which.  The basis is kept across a
 *                   re-binding whose H has the old bits.  HMC stays on the whitened route.
 *  "dense_eigen_wide" 1  eigen route, 512 < D <= 10176: the loop between the boundary products is ONE launch of the
 *                   workgroup-per-chain NUTS kernel (its isotropic instantiation with lambda in the place of the metric,
 *                   the rotated momentum s preset) instead of the diagonal lock-step stage with its launch per lock-step
 *                   and its host polls.  Same discrete outputs and generator states, reals equal up to rounding.
 *                   0 = the lock-step stage (what D > 10176 takes); a change drops the carry record
 *  "dense_eigen_solver" 1  0 = the look-up of the solver fails (for tests of the fall-back); a change drops the basis
 *  "gemm_small_tiles" 1  fp64 GEMM of a mid-size problem (fewer than 256 tiles of 128 x 128, N <= 2048):
 *                   1 = 64 x 128, 64 x 64 or 32 x 64 tiles, the largest that gives every CU two
 *                   workgroups (bitwise the results of the 128 x 128 kernel); 2 / 3 / 4 force
 *                   64 x 64 / 64 x 128 / 32 x 64; 0 = off
 *  "streamk" 2      fp64 GEMM: persistent grid; whole tiles for all but the last 1..2 rounds, the
 *                   rest of the (tile, k) space split evenly; a tile cut between two workgroups is
 *                   accumulated in k order (bitwise equal to 0).  2: 128 x 256 tiles, one
 *                   workgroup per CU, software-pipelined K loop (default); 1: 128 x 128 tiles,
 *                   two workgroups per CU; 0: one tile per workgroup
 *  "compact" 1      NUTS: chains whose transition has finished drop out of the GEMMs
 *  "block_dense" 1  mid-size dense problems (shared dense inverse mass matrix, 64 < D <= 512, "dense_linear" = 1,
 *                   coordinate-wise or dense-precision target): NUTS ("resident_nuts" != 0) and HMC ("fused_hmc" = 1)
 *                   run the whole call in ONE launch, a workgroup per 16 chains -- stages at a wavefront per chain,
 *                   products on fp64 MFMA inside the workgroup, same k-order as the chain-batched GEMM (bitwise
 *                   the lock-step path's results).  1: the chains' moving state in registers up to D = 256, in
 *                   L2-resident work rows above; 2: work rows at every D; 0 = the lock-step path
 *  "pc_dense" 1     one dense inverse mass matrix PER CHAIN (full-matrix window adaptation), 64 < D <= 512, coordinate-wise
 *                   target, "dense_linear" = 1: NUTS runs the whole call in one launch, the wavefront that owns a chain
 *                   streaming its matrix once per leapfrog (csrc/nuts_pc_dense.cuh; bitwise the lock-step path); 0 =
 *                   the lock-step path (per-chain mat-vec launches between the stage kernels)
 *  "block_roll" 0   block-resident NUTS with the state in registers, launches of several transitions: a chain whose
 *                   tree has ended begins its next transition as soon as this many chains of its workgroup wait
 *                   (one more in-workgroup product in that round: csrc/nuts_block_roll.cuh) instead of waiting for
 *                   the deepest of the 16 trees.  0 = rolling with the kernel's threshold (3 with a dense-precision
 *                   target, 4 otherwise) for D >= 192, all chains of a workgroup transition by transition below;
 *                   1 ... 15 = rolling at every D with this threshold; 16 = never.  Results do not depend on it
 *                   (bitwise)
 *  "fp_contract" 0  1: fast arithmetic in the leapfrog bodies of the register-resident HMC kernels
 *                   (diagonal / scalar metric, coordinate-wise target): every a*b+c one fused multiply-add,
 *                   eps*imm and 1/sigma^2 formed once, the half kicks between consecutive leapfrogs of a
 *                   static trajectory merged -- 2 fp64 operations per element and leapfrog instead of 6.
 *                   The integrator of integrators.py:54-73 within 1e-6 relative (the north star's bar);
 *                   0 (default) rounds every product and sum as the reference does and is bit-identical
 *                   to the oracle.  Momentum draw, energies and accept step are the same code in both modes
 *  "joint_resident" 1  joint user-defined density with a reverse-mode program, D <= 512, scalar / diagonal metric: NUTS on
 *                   the register-resident kernel (the position handed to the program through LDS rows) from 17
 *                   coordinates on or when the density's reductions are long; 2 = at every D <= 512; 0 = never (up to
 *                   64 coordinates the forward-mode dense-path kernel, above the one-launch kernel over the chains' L2
 *                   rows, k_nuts_joint_rows: same arithmetic and bits as that one).  HMC: 64 < D <= 1024 on k_hmc_fused
 *                   compiled against the program in the same way (non-zero), or k_hmc_joint_rows (0): same bits
 *  "joint_wg"    1  joint user-defined density that comes with its reverse-mode program (AEHMC_JOINT_GRAD) and sweeps
 *                   long data (AEHMC_JOINT_SWEEP_TERMS >= 8192) in a call of <= 2048 chains: a WORKGROUP of eight
 *                   wavefronts per chain runs the program (k_nuts_joint_wg / k_hmc_joint_wg); 0 = never (a wavefront
 *                   per chain), 2 = always.  Discrete outputs identical, values to rounding (the sums are associated
 *                   differently).  Also the workgroup-per-chain kernels of a row-reduction target (GLM, N >= 8192)
 *  "joint_wide"  1  joint user-defined density with its reverse-mode program (AEHMC_JOINT_GRAD), scalar / diagonal metric:
 *                   NUTS and HMC on the workgroup-per-chain kernels (k_nuts_wide / k_hmc_wide compiled against the
 *                   program, 512 threads, the chain's position and gradient rows in LDS) -- 1: above D = 2048 (there
 *                   the only route besides the lock-step path); 2: also for 512 < D <= 2048 (cross-checks); 0 = never
 *                   (above 2048 the lock-step path, the density evaluated a workgroup per chain: k_target_joint_wg).
 *                   Discrete outputs identical, values to rounding (sums associated differently)
 *  "wg_waves"    0  wavefronts per SIMD those workgroup-per-chain kernels are compiled for: 4 (two workgroups per CU,
 *                   128 registers per lane), 3 (one, 168 registers); 0 = four unless the program then keeps more than
 *                   320 bytes per lane in scratch.  Same results either way */
int aehmc_set_option(aehmc_ctx *ctx, const char *name, int64_t value);

/* "dense_eigen": the caller's own eigenbasis of the whitened operator H = L^T P L of the bound target and metric, in
 * place of the solver's.  V [D, D] row-major, its COLUMNS the eigenvectors; lam [D] the eigenvalues (device arrays,
 * copied).  It is checked like the solver's when the next NUTS call forms the route, and stays the ctx's choice until
 * it is cleared with V = lam = NULL: a basis that does not fit the operator then bound is rejected, and the whitened
 * route runs.  Drops the current basis and the carry record. */
int aehmc_set_white_basis(aehmc_ctx *ctx, int64_t D, const double *V, const double *lam, void *stream);
/* What the last whitened NUTS call decided.  state: 1 the solver's basis is in use, 2 the caller's, 3 one kept across a
 * re-binding; 0 none was asked for yet; -1 the solver (library or symbol) is missing, -2 it reported info != 0 or
 * failed, -3 the basis failed the acceptance check, -4 no memory for it.  orth = max |V^T V - I| and resid =
 * max |H V - V diag(lam)| / max |lam| as measured (-1: not measured), solver_ms the wall time of the factorisation.
 * Any pointer may be NULL. */
int aehmc_white_basis_info(aehmc_ctx *ctx, int32_t *state, double *orth, double *resid, double *solver_ms);

/* workspace the caller must provide to the step calls for C chains */
int64_t aehmc_workspace_bytes(const aehmc_ctx *ctx, int64_t C, int64_t max_num_expansions);
int aehmc_set_workspace(aehmc_ctx *ctx, void *workspace, int64_t bytes);

/* hmc.new_state -- hmc.py:16-40: U = -logprob(q), g = dU/dq */
int aehmc_new_state(aehmc_ctx *ctx, int64_t C, const double *q, double *U, double *g, void *stream);

/* hmc.new_kernel(...)(state, step_size, imm, L) -- hmc.py:77-124,157-204, trajectory.py:31-107.
 * rng [C,2,4]: site #1 momentum, #2 accept.  q,U,g updated in place. */
int aehmc_hmc_step(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                   int64_t num_integration_steps, double divergence_threshold, double *q,
                   double *U, double *g, const aehmc_diagnostics *out, void *stream);

/* num_samples consecutive HMC transitions per chain in one call -- the user-level loop
 * `aesara.scan(kernel, n_steps=N)` of tests/test_hmc.py:138-148 / README.md.  One launch
 * when the fused path applies.  Optional outputs: samples [N,C,D] (position after every
 * transition), acceptance_history [N,C], divergence_history [N,C]; `out` describes the
 * last transition, out->n_leapfrog the total. */
int aehmc_hmc_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                     int64_t num_integration_steps, double divergence_threshold,
                     int64_t num_samples, double *q, double *U, double *g,
                     const aehmc_diagnostics *out, double *samples, double *acceptance_history,
                     int32_t *divergence_history, void *stream);

/* aehmc_hmc_sample with one trajectory length per transition (randomised-length HMC; chees.sample's jittered lengths):
 * transition t runs lengths[t] leapfrogs.  `lengths` is a HOST array of num_samples entries, each >= 0 (a negative one is
 * an error); the engine copies it into a device array of its own on `stream`.  On the routes whose kernels run a whole
 * call in one launch with a coordinate-wise target or a shared dense metric (fused, workgroup per chain, small dense,
 * block dense, regression; DESIGN.md section 3 lists every route) the call is still ONE launch: the kernels read
 * transition t's length from that array, clamped to [0, max(lengths)].  On the other routes the call runs num_samples
 * single transitions with L = lengths[t], as the caller's own loop of aehmc_hmc_step calls would, and records each.
 * Either way the results are bit-equal to that loop.  out->n_leapfrog: the sum of the lengths. */
int aehmc_hmc_sample_lengths(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size, const int64_t *lengths,
                             double divergence_threshold, int64_t num_samples, double *q, double *U, double *g,
                             const aehmc_diagnostics *out, double *samples, double *acceptance_history,
                             int32_t *divergence_history, void *stream);

/* nuts.new_kernel(...)(state, step_size, imm) -- nuts.py:56-153, trajectory.py:154-374,428-714,
 * termination.py:19-235, proposals.py.  rng [C,4,4]: #1 momentum, #2 direction,
 * #3 uniform progressive, #4 biased progressive.  q,U,g updated in place. */
int aehmc_nuts_step(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                    int64_t max_num_expansions, double divergence_threshold, double *q,
                    double *U, double *g, const aehmc_diagnostics *out, void *stream);

/* per-chain step sizes [n] overriding the scalar step_size argument of the step calls
 * (NULL restores the scalar) -- window adaptation adapts one step size per chain.  A step
 * call with a chain count other than n fails. */
int aehmc_set_step_sizes(aehmc_ctx *ctx, const double *step_sizes, int64_t n);

/* window_adaptation.window_adaptation(...).init / .update (window_adaptation.py:119-227,
 * step_size.py:9-100, mass_matrix.py:12-120, algorithms.py:17-204), diagonal mass matrix,
 * one adaptation per chain.  `stage` / `is_window_end` come from build_schedule
 * (window_adaptation.py:230-327, host side); `is_last` = last warm-up step. */
int aehmc_adapt_init(aehmc_ctx *ctx, int64_t C, int64_t D, double initial_step_size,
                     const aehmc_adapt_state *state, void *stream);
int aehmc_adapt_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t stage, int32_t is_window_end,
                       int32_t is_last, double target_acceptance_rate,
                       const double *acceptance_probability, const double *position,
                       const aehmc_adapt_state *state, void *stream);

/* Pooled window adaptation: the same schedule, ONE adaptation from all chains.  One update, with
 * the positions [C,D] and acceptance probabilities [C] after the transition:
 *   abar = (sum_c a_c) / C goes through the dual-averaging update of aehmc_adapt_update (C = 1: its bits);
 *   slow stage, batch Welford with b = (sum_c X_c) / C: n' = n + C, d = b - mean, mean' = mean + d (C / n'),
 *     m2' = m2 + sum_c (X_c - b)(X_c - b)^T + (n C / n') d d^T (aehmc_syrk_tn; a diagonal metric keeps the diagonal);
 *   window end: imm = (n / (n + 5)) m2 / (n - 1) + 1e-3 (5 / (n + 5)) [on the diagonal when full] with the pooled
 *     count, written to BOTH triangles from the same value; sqrt_mass = sqrt(1 / imm) or chol(imm)^-T by the
 *     machinery of aehmc_metric_sqrt on `stream` (a dense window end therefore waits for the stream; an estimate that
 *     is not positive definite leaves NaNs in sqrt_mass and is not an error); Welford state zeroed, dual averaging
 *     restarted; after the last step the step size is exp(x_avg).
 * Sums over the chains run in an order fixed by (C, D) -- no floating-point atomics, two calls are bit-equal.  No D
 * limit of its own; the ctx keeps the scratch.  A caller who samples with state->imm / state->sqrt_mass bound binds
 * them again (aehmc_set_metric) after a window end: the engine derives operators from a bound matrix's content. */
int aehmc_pooled_adapt_init(aehmc_ctx *ctx, int64_t C, int64_t D, double initial_step_size,
                            const aehmc_pooled_adapt_state *state, void *stream);
int aehmc_pooled_adapt_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t stage, int32_t is_window_end,
                              int32_t is_last, double target_acceptance_rate,
                              const double *acceptance_probability, const double *position,
                              const aehmc_pooled_adapt_state *state, void *stream);

/* ChEES warm-up for static HMC (Hoffman, Radul, Sountsov 2021): the trajectory length T and the step
 * size adapted from all chains, around aehmc_hmc_step with a FIXED shared metric.  The transitions export the returned
 * state and the accept flag (aehmc_diagnostics.is_turning), not the proposal: the accept flag stands in for the
 * acceptance probability as the weight, and on accept the returned momentum is the flipped end momentum, so the end
 * velocity is v = -imm o momentum.  One update with n = step, T = exp(log_T), h as stored, positions [C,D] before and
 * after the transition:
 *   m0, m1 = column means of position_before / position_after over ALL chains;
 *   s_c = (|q1_c - m1|^2 - |q0_c - m0|^2) <q1_c - m1, v_c>;  A = sum_c accepted_c,  S = sum_c (accepted_c ? s_c : 0)
 *     (a select: the rows of a rejected chain are not read into S, whatever they hold);
 *   G = h T S / max(A, 1), 0 when A = 0 or G is not finite;  Adam ascent on log_T: m = 0.9 m + 0.1 G,
 *     v = 0.999 v + 0.001 G^2, log_T += learning_rate (m / (1 - 0.9^n)) / (sqrt(v / (1 - 0.999^n)) + 1e-8);
 *   abar = (sum_c a_c) / C through the dual-averaging update of aehmc_pooled_adapt_update (gamma 0.05, t0 10,
 *     kappa 0.75); the new step size eps goes into all C entries of step_size;
 *   log_T clamped to [log eps, log(max_num_steps eps)];  log_T_avg = w log_T + (1 - w) log_T_avg, w = n^-kappa;
 *   is_last: step size = exp(x_avg), log_T = log_T_avg;
 *   step = n + 1, h = base-2 radical inverse of n + 1 (1/2, 1/4, 3/4, 1/8, ...),
 *     num_steps = max(1, ceil(h T / eps)) capped at max_num_steps.
 * `velocity_or_momentum` [C,D] is read as the momentum: v = -inverse_mass_diag o momentum with inverse_mass_diag [D], or
 * v = -inverse_mass_scalar momentum when it is NULL.  For a shared DENSE metric the caller forms momentum . imm
 * (aehmc_gemm_nt) and passes it with inverse_mass_scalar = 1; an array that already holds the velocity goes with -1.
 * init: step 1, log_T = log_T_avg = log(initial_trajectory_length), Adam moments 0, dual averaging as
 * aehmc_pooled_adapt_init leaves it (first step size exp(0) = 1), h = 1/2, num_steps from these (no cap yet).
 * Sums over the chains run in an order fixed by (C, D) -- no floating-point atomics, two calls are bit-equal.  Five
 * reads of [C,D] per update; the ctx keeps the scratch. */
int aehmc_chees_init(aehmc_ctx *ctx, int64_t C, double initial_step_size, double initial_trajectory_length,
                     const aehmc_chees_state *state, void *stream);
int aehmc_chees_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t is_last, double target_acceptance_rate,
                       double learning_rate, int64_t max_num_steps, const double *position_before,
                       const double *position_after, const double *velocity_or_momentum,
                       const double *inverse_mass_diag, double inverse_mass_scalar, const int32_t *accepted,
                       const double *acceptance_probability, const aehmc_chees_state *state, void *stream);

/* The whole ChEES warm-up in one call: num_steps x (copy q; one HMC transition of state->num_steps leapfrogs, at most
 * max_num_steps; for a dense metric momentum . imm; aehmc_chees_update on the copy, q, the momentum, the accept flags
 * out->is_turning and out->acceptance_probability, is_last at the last step) -- the kernels of the caller's own loop in
 * its order, bit-equal to it.  Before the call: aehmc_chees_init on `state`, ONE shared metric bound (scalar: its value
 * also in inverse_mass_scalar; diagonal and dense: taken from the binding), the step sizes bound to state->step_size
 * (aehmc_set_step_sizes, n = C), and out->momentum, out->is_turning, out->acceptance_probability present.  On the routes
 * that read trajectory lengths from device memory (see aehmc_hmc_sample_lengths) the transition takes its length from
 * the state's own cell and nothing is read back: the call returns with all num_steps steps enqueued.  On the other
 * routes the kernels take L from the host, and the call reads the one int64 back before every transition (a stream
 * synchronisation per step, as the caller's loop has).  out->n_leapfrog afterwards: the length of the LAST transition
 * (the kernels write what they ran).  The ctx keeps the two [C,D] work arrays. */
int aehmc_chees_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, double target_acceptance_rate,
                       double learning_rate, int64_t max_num_steps, double inverse_mass_scalar,
                       double divergence_threshold, double *q, double *U, double *g, const aehmc_diagnostics *out,
                       const aehmc_chees_state *state, void *stream);

/* Generalised HMC with a persistent WHITENED momentum v ~ N(0, I) and a non-reversible slice variable u in (-1, 1)
 * (Hoffman & Sountsov 2022): num_samples >= 1 transitions of every chain in one launch, each exactly
 * one leapfrog.  `scale` (device, scale_n = 1 or D, shared by all chains) plays the role of sqrt(inverse_mass_matrix); the
 * bound metric is not read.  One transition:
 *   z = D standard normals of generator site #1;  v = sqrt(1 - alpha) v + sqrt(alpha) z  (has_momentum = 0: the first
 *   transition of the call sets v = z);  u = fmod((u + 1) + delta, 2) - 1  (has_slice = 0: first u = 2 r - 1 with r one
 *   double of site #2, the only draw that site makes);  H0 = U + v.v / 2;
 *   vh = v - (eps / 2)(s g), q' = q + eps (s vh), g' = dU/dq(q'), v' = vh - (eps / 2)(s g');
 *   d = H0 - (U' + v'.v' / 2), NaN -> -inf;  is_diverging = |d| > divergence_threshold;  acceptance_probability =
 *   min(1, exp d);  accept iff d > -inf and log|u| <= d -- no random number;
 *   accept: (q, U, g, v) = (q', U', g', v'), u = u exp(-d);  reject: v = -v (the refreshed one), u unchanged.
 * Parameters: `params` (device, [3]: eps, alpha, delta -- the cell of an aehmc_meads_state, say), or NULL and the three
 * host numbers, which the engine places in a cell of its own on the caller's stream: one code path either way.
 * In place: q, U, g, `momentum` [C,D] and `slice` [C] (read only with their has_ flag, always written).  `out` as HMC
 * fills it: acceptance_probability, is_diverging, n_leapfrog = num_samples, is_turning reused as the accept flag;
 * out->momentum is not written.  Optional per-transition outputs as for HMC sampling.
 * Bound target: the coordinate-wise ones of the library, a user-defined coordinate-wise one, or a joint density that
 * brings its reverse-mode program, D <= 1024.  Anything else -- a regression or GLM target, a joint density without that
 * program, D > 1024, scale_n not 1 or D -- is an error that names the limit; there is no other route. */
int aehmc_ghmc_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, const double *params, double step_size, double alpha,
                      double delta, const double *scale, int64_t scale_n, double divergence_threshold,
                      int64_t num_samples, double *q, double *U, double *g, double *momentum, int32_t has_momentum,
                      double *slice, int32_t has_slice, const aehmc_diagnostics *out, double *samples,
                      double *acceptance_history, int32_t *divergence_history, void *stream);

/* One MEADS update (Hoffman & Sountsov 2022, the all-chains variant) from positions and potential gradients [C,D], C >= 2:
 *   m = column means, var_i = (1 / C) sum_c (Q_ci - m_i)^2, sd = sqrt(var), Z = (Q - m) / sd, Gs = G sd;
 *   lam(X) for X [n,d], S = X X^T:  [(sum_ab S_ab^2 - sum_a S_aa^2) / (n (n - 1))] / [sum_a S_aa / n];
 *   eps = min(1, step_size_multiplier / sqrt(lam(Gs)));
 *   gamma = max(1 / sqrt(lam(Z)), 1 / ((count + 1)^damping_slowdown eps));
 *   alpha = 1 - exp(-2 eps gamma);  delta = alpha / 2;  scale = sd;  count += 1.
 * If eps, alpha, delta or some sd_i is not finite, eps <= 0, or some sd_i = 0, the parameters and the scale stay as they
 * were and skipped += 1 (count still advances).  The C x C matrix is never formed: sum_ab S_ab^2 is the squared
 * Frobenius norm of X^T X, taken from the two symmetric rank-C products (the centred one of Q scaled by 1 / (sd_i sd_j),
 * the uncentred one of G by sd_i sd_j).  Sums run in an order fixed by (C, D), no atomics: two calls are bit-equal.  The
 * ctx keeps the scratch (two [D,D] matrices among it). */
int aehmc_meads_update(aehmc_ctx *ctx, int64_t C, int64_t D, const double *position, const double *potential_energy_grad,
                       double step_size_multiplier, double damping_slowdown, const aehmc_meads_state *state,
                       void *stream);

/* The whole MEADS warm-up in one call: an update on the starting state, then num_steps x (one generalised-HMC transition
 * that reads state->params and state->scale where they lie; an update on the new q, g).  Nothing is read back: the call
 * returns with every step enqueued.  `momentum`, `slice`, their flags and `out` as for the sampling call above; after the
 * first transition both are carried.  The same kernels in the same order as a caller's own loop over the two calls above
 * (which hands the parameters back as host numbers: the same bits). */
int aehmc_meads_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, double step_size_multiplier,
                       double damping_slowdown, double divergence_threshold, double *q, double *U, double *g,
                       double *momentum, int32_t has_momentum, double *slice, int32_t has_slice,
                       const aehmc_diagnostics *out, const aehmc_meads_state *state, void *stream);

/* step_size.dual_averaging_adaptation(target, gamma, t0, kappa) -> update (step_size.py:9-100 over
 * algorithms.dual_averaging, algorithms.py:17-115) as a stand-alone building block around any kernel
 * (tests/test_step_size.py:13-88 wraps hmc.new_kernel with it): one update of the C per-chain states
 * (step [C] int64, iterates x = log step size, iterates_avg, gradient_avg, shrinkage_pts mu, all [C],
 * in place) with gradient = target_acceptance_rate - acceptance_probability.  The states start as
 * algorithms.py:56-76 says: step 1, x = x_avg = gradient_avg = 0, mu as given.  `step_size_out` [C]
 * (may be NULL) receives exp(x) of the updated iterate -- what the test feeds to the next transition. */
int aehmc_dual_averaging_update(aehmc_ctx *ctx, int64_t C, double target_acceptance_rate, double gamma,
                                double t0, double kappa, const double *acceptance_probability,
                                int64_t *step, double *iterates, double *iterates_avg, double *gradient_avg,
                                const double *shrinkage_pts, double *step_size_out, void *stream);

/* algorithms.welford_covariance(compute_covariance) -> update / final (algorithms.py:120-204) and
 * mass_matrix.covariance_adaptation -> final (mass_matrix.py:83-118) as stand-alone building blocks, C independent
 * estimators (tests/test_algorithms.py:60-133, tests/test_mass_matrix.py:11-60 drive them directly): `update` takes
 * one new value [C,D] per estimator (mean [C,D], m2 [C,D] -- or [C,D,D] with `full`, grown by
 * outer(updated_delta, delta) --, sample_size [C], all in place); `final` writes m2 / (sample_size - 1) and, with
 * `shrink`, Stan's regularisation (n / (n + 5)) cov + 1e-3 (5 / (n + 5)) (on the diagonal only when `full`) -- the
 * arithmetic of the warm-up kernels, bit for bit. */
int aehmc_welford_update(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t full, const double *value, double *mean,
                         double *m2, int64_t *sample_size, void *stream);
int aehmc_covariance_final(aehmc_ctx *ctx, int64_t C, int64_t D, int32_t full, int32_t shrink, const double *m2,
                           const int64_t *sample_size, double *out, void *stream);

/* ---- posterior summaries of the draws (aehmc_amd/summary.py) ----
 * What the reference's end-to-end checks compute on the host from every draw (tests/test_hmc.py:158-167: arviz.ess,
 * then std / sqrt(ess)), on the device: per-chain moments, split R-hat, effective sample size and Monte-Carlo standard
 * error per coordinate.  fp64, deterministic (no floating-point atomics, fixed summation orders: two calls on the same
 * input are bit-equal).  All buffers are the caller's; none of these calls touches the workspace, the target or the
 * metric.  `n_segments` is 1 (whole chains) or 2 (split chains): with h = num_draws / 2, draws [0, h) are segment 0 and
 * draws [num_draws - h, num_draws) segment 1 (an odd run's middle draw belongs to neither); the segment length n is
 * num_draws or h, the number of split chains m = n_segments * C.
 *
 * update: folds the chunk samples [T, C, D] -- draws t0 ... t0 + T - 1 of a run of num_draws -- into the running
 * moments mean, m2 [n_segments, C, D] (Welford, ascending t; both start as ZEROS).  Chunks must arrive in order;
 * where they are cut does not change a bit of the result.
 *
 * autocov: acov [K, D], for lags 0 ... K - 1 the biased autocovariance (divided by n) of every split chain about its
 * own mean (`mean` as left by update after the whole run), averaged over the m split chains.  Needs all draws,
 * samples [num_draws, C, D].  work [G, K, D] holds the partial sums of G groups of split chains (1 <= G <= m; group g
 * takes the chains g, g + G, ... in order): more groups, more workgroups.  One coordinate's centred series and K zeros
 * sit in a workgroup's LDS: n + K <= AEHMC_SUMMARY_MAX_ROWS, 2 <= K <= n.
 *
 * final: out [7, D] = mean, sd, rhat, ess, mcse, ess_chains, mcse_chains.  W = mean of the chains' variances (ddof 1),
 * B/n = variance of the chains' means (ddof 1; 0 when m = 1), var+ = W (n - 1) / n + B/n; mean = pooled mean,
 * sd = sqrt(var+), rhat = sqrt(var+ / W), mcse_chains = sqrt((B/n) / m) (NaN when m = 1), ess_chains = var+ / mcse_chains^2.
 * With acov: rho_k = 1 - (W - acov_k) / var+, rho_0 = 1; pair sums P_j = rho_2j + rho_2j+1 are taken while positive
 * (P_0 always) and clipped to the one before (Geyer's initial positive, initial monotone sequence);
 * tau = -1 + 2 sum P_j + (the even term of the first non-positive pair, if positive), at least 1 / log10(m n);
 * ess = m n / tau, mcse = sd / sqrt(ess); lag_truncated [D] = 1 where the pairs were still positive when the K lags ran
 * out.  Without acov (NULL; lag_truncated may be NULL too) rows 3 and 4 of out are left alone.  A coordinate that never
 * moved (var+ = 0) gives rhat = ess = ess_chains = NaN and mcse = 0. */
#define AEHMC_SUMMARY_MAX_ROWS 8192
int aehmc_summary_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws,
                         int32_t n_segments, const double *samples, double *mean, double *m2, void *stream);
int aehmc_summary_autocov(aehmc_ctx *ctx, int64_t num_draws, int64_t C, int64_t D, int32_t n_segments, int64_t K,
                          int64_t G, const double *samples, const double *mean, double *work, double *acov,
                          void *stream);
int aehmc_summary_final(aehmc_ctx *ctx, int64_t num_draws, int64_t C, int64_t D, int32_t n_segments, int64_t K,
                        const double *mean, const double *m2, const double *acov, double *out,
                        int32_t *lag_truncated, void *stream);

/* The same acov [K, D] without the stored draws, for a run of any length: lag_update folds the chunk samples [T, C, D]
 * (draws t0 ... t0 + T - 1, in order, as update) into lagged products over a ring of the last K - 1 draws, and leaves
 * acov complete once the run's last draw has been folded; it then goes into final as it stands.  2 <= K <= n, and no
 * AEHMC_SUMMARY_MAX_ROWS limit.  Every split chain is shifted by its first draw a (y_t = x_t - a); per chain
 * R(k) = sum_{t >= k} y_t y_{t-k} and Y = sum y_t are accumulated in ascending t, and at the segment's last draw, with
 * ybar = Y / n and first_k / last_k the sums of its first / last k shifted draws,
 *   n acov(k) = R(k) - ybar (2 Y - first_k - last_k) + (n - k) ybar^2,
 * which is the autocovariance about the chain's own mean.  State between the calls, all ZEROS at the start and not to
 * be touched in between: shift, sums [C, D] (a, Y), ring, head [K - 1, C, D] (the last and the segment's first K - 1
 * shifted draws) and work [G, K, D], G = ceil(C / aehmc_summary_lag_group(K)): the products, summed over the chains of
 * a group for every draw before they are added, groups reduced in ascending order.  lag_group(K) is the number of
 * consecutive chains per group the engine uses at K lags (the group's rows sit in LDS: 4 up to 48 lags, 2 above; 0 for
 * K < 2).  Segment 1 reuses the state of segment 0.  No floating-point atomics: the
 * additions into every accumulator depend on the shapes alone, so where the chunks are cut does not change a bit. */
int aehmc_summary_lag_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws,
                             int32_t n_segments, int64_t K, const double *samples, double *shift, double *sums,
                             double *ring, double *head, double *work, double *acov, void *stream);
int64_t aehmc_summary_lag_group(int64_t K);

/* ---- nested R-hat for many short chains (aehmc_amd/summary.py) ----
 * The convergence check of the many-chain regime (Margossian, Hoffman, Sountsov, Riou-Durand, Vehtari & Gelman, "Nested
 * R-hat"): the C chains are K = C / chains_per_superchain superchains of M = chains_per_superchain CONSECUTIVE chains
 * (chain c belongs to superchain c / M) that share a starting point, and the run of num_draws draws is cut into
 * num_draws / window windows of `window` draws.  Per window and coordinate, with a_c the mean and s2_c the variance
 * (divisor window - 1; 0 for a window of one draw) of chain c over the window:
 *   abar_k  = mean of a_c over the chains of superchain k,        abar = mean of the abar_k,
 *   between = sum_k (abar_k - abar)^2 / (K - 1),
 *   within  = mean over k of [ sum_{c in k} (a_c - abar_k)^2 / (M - 1)  (0 when M = 1)  +  mean of s2_c over c in k ],
 *   nested_rhat = sqrt(1 + between / within),   mcse_superchains = sqrt(between / K).
 * within = between = 0 gives NaN, within = 0 < between +inf, between = 0 < within exactly 1; a non-finite draw makes its
 * own coordinate and window non-finite and changes nothing else.  K >= 2, M >= 1, window >= 1 -- but not M = 1 with
 * window = 1, which leaves nothing inside a superchain --, C * D <= 2^38.
 *
 * nested_update: folds the chunk samples [T, C, D] -- draws t0 ... t0 + T - 1 of the run, chunks in order -- and writes
 * the rows of every window whose last draw the chunk holds: out [num_draws / window, 5, D] = nested_rhat, between,
 * within, mean (abar), mcse_superchains.  State between the calls, the caller's and not to be touched in between:
 * mean, m2 [C, D], the chains' running moments of the window that is still open (they need no initial value), and out.
 * Nothing else is allocated, whatever T and the number of windows.  At most two kernel launches a call, whatever T and
 * however many windows end in the chunk.  fp64, no floating-point atomics; every sum runs in an order fixed by
 * (C, D, K, M, window): a chain's draws in ascending t, a superchain's chains in ascending c, the superchains k, k + L,
 * ... of each of the L = 256 / min(16, D rounded up to a power of two) lanes of a coordinate in ascending k, the lanes
 * in a fixed tree (pairwise combination of count, mean and sum of squares).  Where the chunks are cut -- inside a window,
 * chunks of one draw -- does not change a bit. */
int aehmc_nested_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t t0, int64_t num_draws, int64_t window,
                        int64_t chains_per_superchain, const double *samples, double *mean, double *m2, double *out,
                        void *stream);

/* ---- order statistics and quantiles of the stored draws (aehmc_amd/summary.py) ----
 * What the reference's users take from arviz on the host (the 5 % / 50 % / 95 % columns of a posterior table), on the
 * device and without a sort: samples [R, D] is the [num_draws, C, D] array of the sampling calls viewed flat, R = N C
 * rows (chains pooled, as the mean and sd of `final` are), 1 <= R < 2^31.  Every double maps to a 64-bit key monotone
 * in its value (negatives: all bits flipped; non-negatives: sign bit set; -0.0 sorts just below +0.0), and the key of
 * the k-th smallest value of a coordinate is found digit by digit, most significant first: 8 passes of 8 bits, each a
 * histogram of the keys that still match the digits found so far, a scan, and the choice of the next digit.  Up to 8
 * ranks share a sweep of 8 passes (a key is counted once however many ranks it still matches), more ranks take
 * ceil(distinct ranks / 8) sweeps: bytes read = sweeps * 8 * R * D * 8.  Counts are integers (LDS and global integer
 * atomics: the result does not depend on the order of arrival), fp64 selection is exact: the result is the bits of
 * np.sort(samples, axis=0)[rank], and two calls on the same input are bit-equal.  A coordinate that holds a NaN gives
 * NaN for every rank and probability (numpy.quantile does); -inf and +inf are ordinary values.  All buffers are the
 * caller's; none of these calls touches the workspace, the target or the metric.
 *
 * quantile_work: the bytes of scratch `work` (device, 256-byte aligned) that a call with M ranks, or M probabilities,
 * needs at these shapes; 0 for shapes the calls refuse.  A misaligned `work` is refused with an error code.
 *
 * order_stats: out [M, D], out[i] = the ranks[i]-th smallest (0-based) value of every coordinate.  `ranks` is a HOST
 * array of M values in [0, R), in any order, repeats allowed; M <= AEHMC_SUMMARY_QUANTILE_MAX.
 *
 * quantiles: out [Q, D], the quantile at probs[i] by numpy's default "linear" rule (R type 7), evaluated in fp64 on the
 * device: h = p (R - 1), lo = floor(h), g = h - lo, a = x_(lo), b = x_(min(lo + 1, R - 1)), d = b - a,
 * q = a + d g if g < 0.5, else b - d (1 - g) (unfused: the bits of numpy.quantile's own formula).  `probs` is a HOST
 * array of Q values in [0, 1]; Q <= AEHMC_SUMMARY_QUANTILE_MAX.  The two ranks of a probability are neighbours and
 * share their counters until their keys part, so Q probabilities cost ceil(distinct ranks / 8) sweeps, at most
 * ceil(Q / 4). */
#define AEHMC_SUMMARY_QUANTILE_MAX 64
int64_t aehmc_summary_quantile_work(int64_t R, int64_t D, int64_t M);
int aehmc_summary_order_stats(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t M, const double *samples,
                              const int64_t *ranks, double *out, void *work, int64_t work_bytes, void *stream);
int aehmc_summary_quantiles(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t Q, const double *samples,
                            const double *probs, double *out, void *work, int64_t work_bytes, void *stream);

/* ---- streaming quantiles: a histogram sketch of draws that are not stored (aehmc_amd/summary.py) ----
 * What `update` above is to the moments, for quantiles: every chunk samples [T, C, D] of a run is folded into a
 * fixed-grid histogram per coordinate and may then be discarded; the chains are pooled.  Coordinate d has the grid
 * lo[d] ... hi[d] in B bins of width[d] = (hi[d] - lo[d]) / B, with inv_width[d] = 1 / width[d]; the CALLER computes
 * width and inv_width once, in fp64, and hands the same [D] device arrays to every call -- the kernels never recompute
 * them.  B is a power of two in [AEHMC_SUMMARY_SKETCH_MIN_BINS, AEHMC_SUMMARY_SKETCH_MAX_BINS].  counts [D, B + 3]
 * (device, 64-bit, ZEROS at the start): slot 0 below the grid, slots 1 ... B interior, slot B + 1 above, slot B + 2 NaN.
 * A value x goes to the slot of t = (x - lo) * inv_width (two rounded fp64 operations): NaN -> B + 2, t < 0 -> 0,
 * t >= B -> B + 1, else 1 + (long long)t; -inf / +inf land below / above without a special case.  The map is monotone
 * in x, so the k-th order statistic lies in the slot in which the cumulative count passes k.  Integer additions only
 * (LDS atomics per workgroup, one 64-bit global atomic per non-empty counter): counts do not depend on where the chunks
 * are cut, on the order of arrival or on the launch geometry, and counts of runs that share a grid may be added.  All
 * buffers are the caller's; none of these calls touches the workspace, the target or the metric.
 *
 * sketch_update: folds samples [T, C, D] into counts.  A workgroup counts in 32 bits: 1 <= T C < 2^31 rows a call (the
 * 64-bit totals have no such limit).
 *
 * sketch_quantiles: estimate [Q, D] and resolved [Q, D] at probs (a HOST array of Q values in [0, 1];
 * Q <= AEHMC_SUMMARY_QUANTILE_MAX).  With R the total of a coordinate's B + 3 counters (read back from the first
 * coordinate: the call waits for the stream; R >= 1), the ranks are those of `quantiles` above: h = p (R - 1),
 * k = floor(h), g = h - k, k1 = min(k + 1, R - 1).  Rank r lies in the slot j with cum[j-1] <= r < cum[j] (cum over
 * slots 0 ... B + 1) at pos(r) = lo + width ((j - 1) + (r - cum[j-1] + 0.5) / count[j]), and
 * estimate = pos(k) + g (pos(k1) - pos(k)).  resolved = 1 where both slots are interior and the coordinate counted no
 * NaN: there |estimate - exact quantile| <= width up to rounding.  A coordinate that counted a NaN gives NaN (as
 * `quantiles` does); otherwise an unresolved estimate is the formula's value, outside the grid and without a bound. */
#define AEHMC_SUMMARY_SKETCH_MIN_BINS 64
#define AEHMC_SUMMARY_SKETCH_MAX_BINS 4096
int aehmc_summary_sketch_update(aehmc_ctx *ctx, int64_t T, int64_t C, int64_t D, int64_t B, const double *samples,
                                const double *lo, const double *inv_width, int64_t *counts, void *stream);
int aehmc_summary_sketch_quantiles(aehmc_ctx *ctx, int64_t D, int64_t B, int64_t Q, const double *probs,
                                   const int64_t *counts, const double *lo, const double *width, double *estimate,
                                   int32_t *resolved, void *stream);

/* ---- constrained draws from unconstrained positions (aehmc_amd/transforms.py) ----
 * The samplers move in R^D_in; a model's parameters are scales, probabilities, ordered cut-points, mixture weights.
 * `constrain` maps x [R, D_in] to y [R, D_out] (fp64, device) in one pass, OUT OF PLACE: the byte ranges of x and y must
 * not overlap (refused otherwise).  D_out = D_in + the number of simplex segments.  1 <= R, 1 <= D_in, D_out < 2^31.
 *
 * table: D_out entries of 40 bytes each (the struct below) on the DEVICE, one per OUTPUT coordinate, built once per
 * model: kind; pos and len, the entry's position in its segment and the segment's length in output coordinates (0 and 1
 * for a coordinate-wise kind; ORDERED of n: j and n; SIMPLEX of K: j and K, fed by K - 1 inputs; len <=
 * AEHMC_CONSTRAIN_MAX_LEN); first, the index of the segment's first INPUT coordinate (a coordinate-wise kind: the
 * entry's own input); lo and hi, the bounds (0 where unused); reserved = 0.  An entry whose segment does not lie
 * inside the row, or of an unknown kind, writes NaN and reads nothing.
 *
 * Formulas, every operation rounded on its own, in this order:
 *   REAL      y = x
 *   LOWER     y = lo + exp(x)
 *   UPPER     y = hi - exp(x)
 *   INTERVAL  s = 1 / (1 + exp(-x)) where x >= 0, else e / (1 + e) with e = exp(x);  y = lo + (hi - lo) s;
 *             y = hi where s == 1 or y > hi
 *   ORDERED   t = x_0;  t = t + exp(x_j) for j = 1 ... pos, ascending;  y = t
 *   SIMPLEX   xt = (x_0 ... x_{K-2}, 0);  m = the largest xt_j (m = xt_0, replaced where xt_j > m, j ascending);
 *             L = m + log(sum_j exp(xt_j - m)), the sum ascending in j;  y = exp(xt_pos - L)
 * NaN in gives NaN out.  INTERVAL gives exactly lo and exactly hi for large |x|, never a NaN from a finite x.  exp
 * overflow gives +inf in LOWER and ORDERED, -inf in UPPER.  A SIMPLEX with +inf among its inputs gives NaN (inf - inf),
 * with -inf a weight of 0.  One thread computes one output from its inputs alone: the result depends neither on the
 * launch geometry nor on how the rows are cut into calls.  All buffers are the caller's; the call touches neither the
 * workspace, nor the target, nor the metric. */
#define AEHMC_CONSTRAIN_MAX_LEN 64
enum { AEHMC_CONSTRAIN_REAL = 0, AEHMC_CONSTRAIN_LOWER = 1, AEHMC_CONSTRAIN_UPPER = 2, AEHMC_CONSTRAIN_INTERVAL = 3,
       AEHMC_CONSTRAIN_ORDERED = 4, AEHMC_CONSTRAIN_SIMPLEX = 5 };
typedef struct aehmc_constrain_entry {
  int32_t kind, pos, len, reserved;
  int64_t first;
  double lo, hi;
} aehmc_constrain_entry;
int aehmc_constrain(aehmc_ctx *ctx, int64_t R, int64_t D_in, int64_t D_out, const double *x,
                    const aehmc_constrain_entry *table, double *y, void *stream);

/* ---- pointwise log-likelihoods of traced models and streaming WAIC (aehmc_amd/summary.py) ----
 * A POINTWISE PROGRAM is a vector function of one chain's position, one entry per observation, given as HIP source that
 * defines (aehmc_amd/tracing.py: trace_pointwise writes it; `#include "dual.cuh"` first for softplus / logistic / square)
 *   template <class V> __device__ void aehmc_pointwise_head
 *       (const V &q, const double *const *prm, double *h);
 *   template <class V> __device__ double aehmc_pointwise
 *       (const V &q, const double *h, long long j, const double *const *prm);
 * q[i] are the row's coordinates, prm the parameter arrays; the head writes the n_head values of a row that do not depend
 * on j (n_head may be 0), and aehmc_pointwise returns entry j from the row and those values.
 *
 * set_pointwise compiles the source with hipRTC (the on-disk cache of aehmc_set_rtc_cache serves it too) and binds it
 * BESIDE the target: the sampler's target, metric and workspace are not touched, so a run can sample with the target
 * while it folds.  1 <= D <= 10176, 1 <= n_out <= 65535 * 256, 0 <= n_head <= 8192.  params: n_params device arrays (a
 * host array of device pointers), owned by the caller and alive while the program is bound.  The call is a transaction: a
 * source that does not compile returns an error, with the compiler's log in aehmc_last_error, and leaves the previously
 * bound pointwise program in place.
 *
 * pointwise_eval: x [R, D] (fp64, device, contiguous) -> out [R, n_out], one kernel; out[r][j] depends on row r alone.
 *
 * WAIC state: [4][n_obs] doubles (device) -- per observation the running maximum m, s = sum exp(l - m), the mean and
 * the sum of squared deviations M2 of the values folded so far -- and the number of draws behind it, n_state, which the
 * CALLER keeps: 0 and (m, s, mean, M2) = (-inf, 0, 0, 0) to start, then n_state += R after every fold.
 *   pointwise_waic_fold  folds the program's values of rows x [R, D] into `state` without storing them;
 *   waic_fold            folds a stored block x [R, n_obs] (precompiled: needs no bound program);
 *   waic_merge           adds `other` (n_other >= 1 draws, another state, not `state` itself) behind `state`;
 *   waic_final           lppd[i] = m + log(s) - log(n_state), p[i] = M2 / (n_state - 1)  (n_state >= 1; [n_obs] each).
 * A fold cuts its R rows into parts of 256 consecutive rows (the last one shorter), folds each part draw by draw in
 * ascending order -- l > m: s = s exp(m - l) + 1, m = l, else s = s + exp(l - m); Welford's update for mean and M2 --
 * and adds the parts in ascending order behind the state: max-rescaling for (m, s), the pairwise update of Chan, Golub &
 * LeVeque (1983) for (mean, M2); csrc/pointwise.cuh states every operation.  The partition depends on R alone, never on
 * the device; there are no atomics: equal calls give equal bits, and pointwise_waic_fold(x) gives the bits of
 * waic_fold(pointwise_eval(x)).  How the draws are cut into calls changes the partition, so the result to rounding.
 * A -inf value adds nothing to s and makes M2 (so p) NaN; a NaN makes the observation NaN; other observations are not
 * affected.  The parts [ceil(R / 256)][4][n_obs] live in a buffer of the ctx that grows on demand (hipFree / hipMalloc
 * inside the call when it grows: not during stream capture).  1 <= R <= 2^31 * 256 - 256, n_state < 2^53. */
int aehmc_set_pointwise(aehmc_ctx *ctx, const char *source, int64_t D, int64_t n_out, int32_t n_head,
                        const double *const *params, int32_t n_params, const char *include_dir);
int aehmc_pointwise_eval(aehmc_ctx *ctx, int64_t R, const double *x, double *out, void *stream);
int aehmc_pointwise_waic_fold(aehmc_ctx *ctx, int64_t R, const double *x, double *state, int64_t n_state, void *stream);
int aehmc_waic_fold(aehmc_ctx *ctx, int64_t R, int64_t n_obs, const double *x, double *state, int64_t n_state,
                    void *stream);
int aehmc_waic_merge(aehmc_ctx *ctx, int64_t n_obs, double *state, int64_t n_state, const double *other,
                     int64_t n_other, void *stream);
int aehmc_waic_final(aehmc_ctx *ctx, int64_t n_obs, const double *state, int64_t n_state, double *lppd, double *p,
                     void *stream);

/* ---- average ranks and normal scores of the stored draws (aehmc_amd/summary.py) ----
 * What the rank-normalised split R-hat and the bulk ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) are
 * computed from: samples [R, D] as above, out [R, D].  mode 0: out = the average rank of every draw among the R draws
 * of its coordinate, r = #{y < x} + (#{y == x} + 1) / 2 (1-based; scipy.stats.rankdata(method="average")), a
 * half-integer below 2^31 and so exact.  mode 1: out = the normal score Phi^-1((r - 3/8) / (R + 1/4)), Phi^-1 by
 * Wichura's AS 241 (PPND16) in fp64.  center [D] (device) or NULL: with it the ranks are those of |x - center[d]| (the
 * folded draws; no copy of them is made).  Values compare as IEEE values: -0.0 and +0.0 tie, -inf and +inf and
 * denormals are ordinary; a coordinate that holds a NaN (or whose fold makes one) gives NaN for every draw.
 *
 * Method (csrc/rank.cuh): per tile of T coordinates the keys are written as columns, sorted by a least-significant-
 * digit radix sort (8 passes of 8 bits, keys only, every position from counts and scans: the same bits on every run),
 * and every draw's two bounds are searched in its sorted column.  `work` (device, 256-byte aligned) decides T: the call
 * takes the widest tile that work_bytes hold, anything from one coordinate's need (2 R keys of 8 bytes, 1 KiB of
 * counters per started 4096 keys, each rounded up to 256 bytes) upward, and the result does not depend on it.
 * rank_work: the default scratch -- the widest tile under 256 MiB, at least one coordinate; 0 for shapes the call
 * refuses (1 <= R < 2^31, 1 <= D < 2^31). */
int64_t aehmc_summary_rank_work(int64_t R, int64_t D);
int aehmc_summary_rank(aehmc_ctx *ctx, int64_t R, int64_t D, const double *samples, const double *center, int mode,
                       double *out, void *work, int64_t work_bytes, void *stream);

/* ---- highest-density intervals and the MCSE of quantiles (aehmc_amd/summary.py) ----
 * The remaining columns of a posterior table that need values at positions of the sorted pooled draws which differ from
 * coordinate to coordinate: consumers of the sorted key columns of `rank` above (csrc/posterior.cuh).  samples [R, D]
 * as above, the chains pooled; -0.0 and +0.0 tie and come back as +0.0, -inf and +inf and denormals are ordinary
 * values, a coordinate that holds a NaN answers NaN.  `work` is that of aehmc_summary_rank_work(R, D): 256-byte
 * aligned, anything from one coordinate's need upward, and the result does not depend on it; 1 <= R < 2^31.  No
 * floating-point atomics: two calls on the same input are bit-equal.
 *
 * hdi: with s_0 <= ... <= s_{R-1} a coordinate's sorted draws and m = min(floor(prob R), R - 1) (the product in fp64),
 * the windows w_i = s_{i+m} - s_i, i = 0 ... R - m - 1 (a NaN width, inf - inf, counts as +inf), i* the smallest i of
 * minimal width: lower [D] = s_{i*}, upper [D] = s_{i*+m}, index [D] (or NULL) = i*; NaN, NaN and -1 for a coordinate
 * with a NaN.  ArviZ's unimodal hdi with m held to R - 1, so that prob = 1 gives (min, max).  prob in (0, 1].
 *
 * quantile_mcse: out [Q, D], the Monte-Carlo standard error of the quantile at probs[q] (posterior::mcse_quantile,
 * ArviZ's _mcse_quantile).  `probs` is a HOST array of Q values in [0, 1], Q <= AEHMC_SUMMARY_QUANTILE_MAX; ess [Q, D]
 * (device) the effective sample size of the indicator x <= quantile per probability and coordinate.  With e = ess[q][d],
 * p = probs[q]: a1 = beta_quantile(0.1586553, e p + 1, e (1 - p) + 1), a2 = beta_quantile(0.8413447, the same),
 * lo = max(floor(a1 R), 1) - 1, hi = min(ceil(a2 R), R) - 1, out = (s_hi - s_lo) / 2; ranks [2, Q, D] (or NULL) = lo,
 * hi.  An e that is NaN, infinite or <= 0 gives NaN (ranks -1), as does a coordinate with a NaN.
 *
 * beta_quantile: out[i] = the x with I_x(a[i], b[i]) = p[i] (the regularised incomplete beta function), for n
 * elements of DEVICE arrays; fp64, a, b >= 1 and finite, 0 < p < 1, NaN otherwise.  The continued fraction of I_x with
 * a bounded number of terms, Halley steps inside a bisection bracket; accuracy in DESIGN.md section 4. */
int aehmc_summary_hdi(aehmc_ctx *ctx, int64_t R, int64_t D, const double *samples, double prob, double *lower,
                      double *upper, int64_t *index, void *work, int64_t work_bytes, void *stream);
int aehmc_summary_quantile_mcse(aehmc_ctx *ctx, int64_t R, int64_t D, int64_t Q, const double *samples,
                                const double *probs, const double *ess, double *out, int64_t *ranks, void *work,
                                int64_t work_bytes, void *stream);
int aehmc_beta_quantile(aehmc_ctx *ctx, int64_t n, const double *p, const double *a, const double *b, double *out,
                        void *stream);

/* ---- Pareto-smoothed importance sampling: PSIS weights, Pareto k, PSIS-LOO (aehmc_amd/summary.py) ----
 * Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling", with Zhang & Stephens' (2009) fit of
 * the generalised Pareto distribution and the prior constants of ArviZ's _gpdfit: what az.loo / R's loo compute, per
 * column of log_ratios [R, D] (R pooled draws, D columns: one observation is one coordinate), in fp64.  One more
 * consumer of the sorted key columns of `rank` above (csrc/psis.cuh): `work` is that of aehmc_summary_rank_work(R, D),
 * 256-byte aligned, anything from one coordinate's need upward; 1 <= R < 2^31.  No floating-point atomics: every output
 * is the same bits on every run and for every size of `work`.  Under a permutation of the rows pareto_k and tail_len
 * keep their bits and every row keeps the bits of its log-weight (they come from the sorted column); log_mean is summed
 * along the rows and is equal to rounding only.
 *
 * Per column x, with reff = reff[d] (device, [D]) or 1 if reff is NULL:
 *  - mx = max(x).  A NaN in the column, an mx that is not finite (a +inf, or all -inf) or a reff that is not finite
 *    and > 0: every output of the column is NaN and tail_len = -1.  -inf entries are ordinary: weight 0.  y = x - mx.
 *  - M = ceil(min(R / 5, 3 sqrt(R / reff))) held to [0, R - 1]; with s the sorted y, cut = max(s[R - M - 1],
 *    log(DBL_MIN)); the tail is the draws with y > cut, strictly, n = tail_len <= M of them.
 *  - n <= 4: pareto_k = +inf and nothing is smoothed.  Otherwise t_j = exp(s_j) - exp(cut) over the tail, ascending,
 *    m = 30 + floor(sqrt n), b_i = (1 - sqrt(m / (i - 0.5))) / (3 t_q) + 1 / t_n for i = 1 ... m with
 *    t_q = t[floor(n / 4 + 0.5) - 1], k_i = mean_j log1p(-b_i t_j), L_i = n (log(-b_i / k_i) - k_i - 1),
 *    w_i = 1 / sum_l exp(L_l - L_i), weights below 10 DBL_EPSILON dropped and the rest renormalised, b = sum w_i b_i,
 *    k' = mean_j log1p(-b t_j), sigma = -k' / b, pareto_k = (n k' + 5) / (n + 10).  If that is not finite or sigma is
 *    not > 0 the fit has failed: pareto_k = NaN and nothing is smoothed.
 *  - smoothing: place j = 0 ... n - 1 of the tail gets min(log(sigma gpinv((j + 0.5) / n) + exp(cut)), 0),
 *    gpinv(p) = expm1(-k log1p(-p)) / k, or -log1p(-p) when |k| < DBL_EPSILON.  Tied tail draws that occupy the places
 *    lo ... hi - 1 all receive the log of the mean of the exp of those places' values, summed in ascending place: the
 *    weights are a function of the multiset of draws, and without ties they are ArviZ's psislw.
 *  - log_weights [R, D] (or NULL: not stored) = the result minus the log of the sum of its exp: sum exp = 1.
 *  - with log_values [R, D]: log_mean [D] = log sum_s exp(log_weights + log_values), whether or not log_weights is
 *    stored; log_mean is required if and only if log_values is given.
 * pareto_k [D] is required, tail_len [D] (int64) may be NULL.
 *
 * PSIS-LOO is log_ratios = -log_lik, log_values = log_lik, and log_mean is then elpd_loo_i.  For that case log_ratios
 * may be NULL: the ratios are then -log_values, no negated copy is read, and with log_weights NULL the call touches no
 * memory of size R D besides its input. */
int aehmc_summary_psis(aehmc_ctx *ctx, int64_t R, int64_t D, const double *log_ratios, const double *reff,
                       const double *log_values, double *log_weights, double *pareto_k, int64_t *tail_len,
                       double *log_mean, void *work, int64_t work_bytes, void *stream);

/* window_adaptation.run (window_adaptation.py:17-116) for a NUTS kernel: num_steps x (one transition
 * with the current per-chain parameters, then aehmc_adapt_update), enqueued in one call.  `stage` /
 * `is_window_end` [num_steps] are HOST arrays from build_schedule.  Before the call the caller binds
 * the per-chain metric to state->imm / state->sqrt_mass (aehmc_set_metric, per_chain = 1) and the step
 * sizes to state->step_size (aehmc_set_step_sizes); the update kernel rewrites them in place.
 * `out` receives the diagnostics of the last warm-up transition.  Diagonal mass matrix with the
 * regression target, or with a coordinate-wise target of D <= 512 on the register-resident kernel,
 * and a full mass matrix per chain (state->full) with D <= 64 and a coordinate-wise or dense-precision
 * target, or with the regression target: the whole warm-up is ONE launch in which the chains adapt and move on at their own pace
 * (same arithmetic, same results as the loop). */
int aehmc_nuts_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, const int32_t *stage,
                      const int32_t *is_window_end, double target_acceptance_rate,
                      int64_t max_num_expansions, double divergence_threshold, double *q, double *U,
                      double *g, const aehmc_diagnostics *out, const aehmc_adapt_state *state, void *stream);

/* The same loop around an HMC kernel (the reference's run() calls `kernel(chain_state, *parameters)`,
 * window_adaptation.py:66, so there an HMC kernel is wrapped in a function that closes over the trajectory length
 * num_integration_steps): num_steps x (one HMC transition with the current per-chain parameters, then
 * aehmc_adapt_update).  Same binding rules, same `stage` / `is_window_end` host arrays as aehmc_nuts_warmup. */
int aehmc_hmc_warmup(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, const int32_t *stage,
                     const int32_t *is_window_end, double target_acceptance_rate, int64_t num_integration_steps,
                     double divergence_threshold, double *q, double *U, double *g, const aehmc_diagnostics *out,
                     const aehmc_adapt_state *state, void *stream);

/* The same loops with POOLED adaptation: num_steps x (one transition, then aehmc_pooled_adapt_update), enqueued in
 * one call.  Before the call the caller binds the SHARED metric to state->imm / state->sqrt_mass (aehmc_set_metric,
 * per_chain = 0) and the step sizes to state->step_size (aehmc_set_step_sizes, n = C).  After a window end the loop
 * binds the metric again, so that the engine drops what it derived from the old content (the whitened operator and
 * its carry record).  The transitions take the shared-metric routes of aehmc_nuts_step / aehmc_hmc_step. */
int aehmc_nuts_warmup_pooled(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, const int32_t *stage,
                             const int32_t *is_window_end, double target_acceptance_rate,
                             int64_t max_num_expansions, double divergence_threshold, double *q, double *U,
                             double *g, const aehmc_diagnostics *out, const aehmc_pooled_adapt_state *state,
                             void *stream);
int aehmc_hmc_warmup_pooled(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t num_steps, const int32_t *stage,
                            const int32_t *is_window_end, double target_acceptance_rate,
                            int64_t num_integration_steps, double divergence_threshold, double *q, double *U,
                            double *g, const aehmc_diagnostics *out, const aehmc_pooled_adapt_state *state,
                            void *stream);

/* num_samples consecutive NUTS transitions per chain (the user-level scan of
 * tests/test_hmc.py:296-324); same optional outputs as aehmc_hmc_sample plus the per-chain
 * leapfrog total [C].  `out` describes the last transition.  (Regression target and register-resident
 * kernel, D <= 512: one launch for all num_samples transitions.) */
int aehmc_nuts_sample(aehmc_ctx *ctx, int64_t C, uint64_t *rng, double step_size,
                      int64_t max_num_expansions, double divergence_threshold, int64_t num_samples,
                      double *q, double *U, double *g, const aehmc_diagnostics *out, double *samples,
                      double *acceptance_history, int32_t *divergence_history,
                      int64_t *n_leapfrog_total, void *stream);

/* sqrt_mass = sqrt(1 / imm) (ndim 0 / 1) or chol(imm)^-T (ndim 2; metrics.py:45,49,56-58: blocked Cholesky +
 * triangular inverse on the fp64 MFMA GEMM) of ONE shared metric into a caller-owned array ([1] | [D] | [D,D]) --
 * what aehmc_set_metric computes into ctx memory when aehmc_metric.sqrt_mass is NULL.  A caller that alternates
 * between several metrics factors each once, keeps the results and passes them in aehmc_metric.sqrt_mass. */
int aehmc_metric_sqrt(aehmc_ctx *ctx, int32_t ndim, int64_t D, const double *imm, double *sqrt_mass, void *stream);

/* sqrt_mass[c] = chol(imm[c])^-T (metrics.py:56-58) for C dense D x D matrices, D <= 2048 (one
 * wavefront per matrix: in LDS up to D = 64, in a temporary device buffer above) */
int aehmc_metric_sqrt_per_chain(aehmc_ctx *ctx, int64_t C, int64_t D, const double *imm, double *sqrt_mass,
                                void *stream);

/* ---- building blocks exported for known-answer tests / callers that want them ---- */

/* integrators.py:54-73 applied nsteps times to C chains (state in place) */
int aehmc_leapfrog(aehmc_ctx *ctx, int64_t C, double step_size, int64_t nsteps, double *q,
                   double *p, double *U, double *g, void *stream);
/* metrics.py:70-73 */
int aehmc_kinetic_energy(aehmc_ctx *ctx, int64_t C, const double *p, double *K, void *stream);
/* metrics.py:75-104 */
int aehmc_is_turning(aehmc_ctx *ctx, int64_t C, const double *p_left, const double *p_right,
                     const double *p_sum, int32_t *out, void *stream);
/* RNG streams as numpy would produce them: n normals / bernoulli(p[i]) from rng [C,4] */
int aehmc_rng_normals(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t n, double *out, void *stream);
int aehmc_rng_bernoulli(aehmc_ctx *ctx, int64_t C, uint64_t *rng, int64_t n, const double *p,
                        int32_t *out, void *stream);
/* fp64 MFMA GEMM used by the dense-metric path: Cmat[M,N] = A[M,K] * B[N,K]^T (row-major) */
int aehmc_gemm_nt(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                  const double *B, int64_t ldb, double *Cmat, int64_t ldc, void *stream);
/* The same product with a hint on B: tri = 0 none, 1 = B[n,k] == 0 for k > n (lower triangular), 2 = B[n,k] == 0 for
 * k < n (upper triangular).  A hint, not a mode: the 128 x 256 stream-K kernel (>= 256 tiles, K % 16 == 0) skips the
 * K-tiles that lie wholly in the zero triangle, every other kernel computes the full product.  For FINITE A the result
 * is bitwise that of aehmc_gemm_nt (skipped terms are a * 0 added to accumulators that start at +0); a NaN or infinity
 * in A reaches only the elements whose K range holds it.  B's other triangle must be exact zeros.  row_idx / n_rows
 * (both or neither; device pointers): compacted rows -- tile row r reads A row row_idx[r] and writes C row row_idx[r],
 * *n_rows <= M rows exist.  The profiled flop count adds the K-tiles a launch executes. */
int aehmc_gemm_nt_tri(aehmc_ctx *ctx, int64_t M, int64_t N, int64_t K, const double *A, int64_t lda,
                      const double *B, int64_t ldb, double *Cmat, int64_t ldc, int32_t tri, const int32_t *row_idx,
                      const int32_t *n_rows, void *stream);

/* Symmetric rank-C update on the fp64 MFMA, X [C, ldx >= D] chain-major (the product X^T X, summed over the rows):
 *   S[i,j] += sum_c (X[c,i] - centre[i]) (X[c,j] - centre[j]) + w delta[i] delta[j]     for j <= i
 * (S [D, lds >= D] row-major; `centre` and `delta` [D] may be NULL: no centring / no rank-one term).  Only tiles on or
 * below the diagonal are computed; elements strictly above the diagonal are unspecified after the call.  Chains are
 * summed in ascending tiles of 16, a mid-size D in a fixed number of parts added in order: bit-equal between calls. */
int aehmc_syrk_tn(aehmc_ctx *ctx, int64_t C, int64_t D, const double *X, int64_t ldx, const double *centre, double w,
                  const double *delta, double *S, int64_t lds, void *stream);

/* timing hooks for bench.py: HIP events (on the launch stream) around every launch of the
 * dominant kernel (fp64 GEMM, or the fused HMC kernel) since profile_enable(1), and the
 * algorithmic flops of those GEMM launches (2*rows*N*K with the live row count). */
int aehmc_profile_enable(aehmc_ctx *ctx, int enable);
int aehmc_profile_read(aehmc_ctx *ctx, double *kernel_ms_total, int64_t *kernel_launches,
                       double *gemm_flops_total);

/* wait for `stream` and report device-side failures that are not data (a stream-K GEMM
 * hand-off that timed out because the persistent grid was not co-resident): the step calls
 * are asynchronous, so such a failure in the last launches of a call surfaces here, at the
 * next GEMM launch or in aehmc_profile_read. */
int aehmc_synchronize(aehmc_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AEHMC_HIP_H */
