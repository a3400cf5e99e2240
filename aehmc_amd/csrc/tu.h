// The library is compiled as several translation units (engine.hip + tu_*.hip, `make -j`): each kernel family's
// launch function is instantiated in its own file and reached through the plain functions declared here.
// engine.hip still includes the family headers -- for their argument structs and host-side predicates -- but never
// names a launch_* function of theirs, so none of their kernels is instantiated there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aehmc {
struct EngineArgs;
struct NutsSampleArgs;
struct HmcFusedArgs;
struct HmcSampleArgs;
struct GemmStreamK;
struct PoolArgs;
struct CheesArgs;
struct GhmcArgs;
struct MeadsArgs;
namespace tu {
// gemm_f64.cuh
hipError_t gemm_nt_f64(int64_t M, int64_t N, int64_t K, const double *A, int64_t lda, const double *B, int64_t ldb,
                       double *Cm, int64_t ldc, hipStream_t stream, const int *row_idx, const int *n_rows,
                       unsigned long long *flop_counter, const GemmStreamK *sk, int sk_grid, int mode, int sk_grid_wide,
                       int small_tiles, int tri, bool in_place);
hipError_t gemm_streamk_occupancy(int *per_cu);
// nuts_linreg.cuh, hmc_linreg.cuh
hipError_t nuts_linreg(const EngineArgs &a, const NutsSampleArgs &m, hipStream_t st);
hipError_t hmc_linreg(const HmcFusedArgs &a, hipStream_t st);
// nuts_wide.cuh
hipError_t nuts_wide(const EngineArgs &a, hipStream_t st);
// nuts_resident.cuh
hipError_t nuts_resident(const EngineArgs &a, const NutsSampleArgs &m, hipStream_t st, int force_min_team);
hipError_t nuts_resident_dense(const EngineArgs &a, const NutsSampleArgs &m, hipStream_t st, bool md, bool td, bool pc);
// nuts_block*.cuh
hipError_t nuts_block_roll(const EngineArgs &a, const NutsSampleArgs &m, double *bp, hipStream_t st);
hipError_t nuts_block_reg(const EngineArgs &a, const NutsSampleArgs &m, double *bp, hipStream_t st);
hipError_t nuts_block_dense(const EngineArgs &a, const NutsSampleArgs &m, double *bp, hipStream_t st);
// (h.len.Ls: trajectory lengths from device memory, or nullptr -- the launch constant h.L)
hipError_t hmc_block_reg(const EngineArgs &a, const HmcSampleArgs &h, double *bp, hipStream_t st);
hipError_t hmc_block_dense(const EngineArgs &a, const HmcSampleArgs &h, double *bp, hipStream_t st);
// nuts_pc_dense.cuh
hipError_t nuts_pc_dense(const EngineArgs &a, const NutsSampleArgs &m, hipStream_t st);
hipError_t hmc_pc_dense(const EngineArgs &a, const HmcSampleArgs &h, hipStream_t st);
// hmc_fused.cuh
hipError_t hmc_fused(const HmcFusedArgs &a, hipStream_t st);
hipError_t hmc_resident(const HmcFusedArgs &a, const double *zbuf, int nt, hipStream_t st);
// summary.cuh
hipError_t summary_update(const double *x, long long T, long long E, long long t0, long long N, int S, double *mean,
                          double *m2, hipStream_t st);
hipError_t summary_acov(const double *x, const double *mean, double *partial, double *acov, long long N, long long C,
                        long long D, int S, long long K, int G, hipStream_t st);
hipError_t summary_final(const double *mean, const double *m2, const double *acov, double *out, int *lag_truncated,
                         long long n, long long m, long long D, long long K, hipStream_t st);
hipError_t summary_lag_update(const double *x, long long T, long long C, long long D, long long t0, long long N, int S,
                              long long K, int CG, double *shift, double *sums, double *ring, double *head,
                              double *prod, double *acov, hipStream_t st);
int summary_lag_group(long long K);
// nested.cuh (windows of w draws, superchains of M chains; nested_blocks: workgroups per window that ends in a chunk)
hipError_t nested_update(const double *x, long long T, long long C, long long D, long long t0, long long w, long long M,
                         double *mean, double *m2, double *out, hipStream_t st);
long long nested_blocks(long long D);
// quantile.cuh (work: the caller's scratch of quantile_work_bytes(D, M); the statistics land in its stats rows)
size_t quantile_work_bytes(long long D, long long M);
hipError_t quantile_stats(const double *x, long long R, long long D, int U, const long long *ranks, void *work,
                          long long M, hipStream_t st);
hipError_t quantile_out(void *work, long long D, long long M, int n, const int *lo, const int *hi, const double *g,
                        double *out, hipStream_t st);  // rows lo of the statistics; with g, interpolated towards rows hi
// sketch.cuh (x [R][D] into counts [D][B + 3]; U distinct ascending ranks, rows lo_row / hi_row of them and the gap g
// behind each of Q probabilities: all host arrays)
hipError_t sketch_update(const double *x, long long R, long long D, int B, const double *lo, const double *inv,
                         unsigned long long *counts, hipStream_t st);
hipError_t sketch_quantiles(const unsigned long long *counts, const double *lo, const double *width, long long D, int B,
                            int Q, int U, const long long *ranks, const int *lo_row, const int *hi_row, const double *g,
                            double *estimate, int *resolved, hipStream_t st);
// constrain.cuh (x [R][D_in] into y [R][D_out], disjoint; table: D_out entries of 40 bytes on the device)
hipError_t constrain(const double *x, long long R, long long D_in, long long D_out, const void *table, double *y,
                     hipStream_t st);
// pointwise.cuh (ws: the parts of a fold [parts][4][n_obs]; state [4][n_obs] behind n_state draws)
hipError_t waic_fold_stored(const double *x, long long R, long long n_obs, double *ws, hipStream_t st);
hipError_t waic_merge(const double *ws, long long parts, long long part_rows, long long R, double *state, double n_state,
                      long long n_obs, hipStream_t st);
hipError_t waic_final(const double *state, double n_state, long long n_obs, double *lppd, double *p, hipStream_t st);
// rank.cuh (a tile of T coordinates needs rank_work_bytes(R, T) of scratch; rank_tile_width: the widest tile that
// `bytes` hold, 0 if none; rank_default_tile: what fits under 256 MiB, at least 1)
size_t rank_work_bytes(long long R, long long T);
long long rank_tile_width(long long R, long long D, size_t bytes);
long long rank_default_tile(long long R, long long D);
hipError_t rank(const double *x, const double *centre, long long R, long long D, int mode, double *out, void *work,
                long long T, hipStream_t st);
// posterior.cuh (on rank.cuh's sorted columns, the same scratch and tiles; m: the HDI's window in order statistics;
// probs [Q] host, ess [Q][D] device; beta_quantile: device arrays of n)
hipError_t hdi(const double *x, long long R, long long D, long long m, double *lower, double *upper, long long *index,
               void *work, long long T, hipStream_t st);
hipError_t quantile_mcse(const double *x, long long R, long long D, int Q, const double *probs, const double *ess,
                         double *out, long long *ranks, void *work, long long T, hipStream_t st);
hipError_t beta_quantile(long long n, const double *p, const double *a, const double *b, double *out, hipStream_t st);
// psis.cuh (the same scratch and tiles again; neg: the ratios are -x; reff [D], v [R][D], log_weights [R][D], tail_len
// [D] may be null, log_mean [D] goes with v)
hipError_t psis(const double *x, bool neg, const double *reff, const double *v, double *log_weights, double *pareto_k,
                long long *tail_len, double *log_mean, long long R, long long D, void *work, long long T, hipStream_t st);
// syrk_f64.cuh, pooled_adapt.cuh
hipError_t syrk_tn(long long C, long long D, const double *X, long long ldx, const double *centre, double w,
                   const double *w_dev, const double *delta, double *S, long long lds, double *partial, hipStream_t st);
size_t syrk_partial_doubles(long long C, long long D);
hipError_t pool_init(const PoolArgs &a, double initial_step_size, hipStream_t st);
hipError_t pool_sums(const PoolArgs &a, hipStream_t st);
hipError_t pool_imm(const PoolArgs &a, hipStream_t st);
hipError_t pool_scalars(const PoolArgs &a, hipStream_t st);
// chees.cuh
hipError_t chees_init(const CheesArgs &a, double initial_step_size, double initial_trajectory_length, hipStream_t st);
hipError_t chees_update(const CheesArgs &a, hipStream_t st);
// ghmc_fused.cuh
hipError_t ghmc_fused(const GhmcArgs &a, hipStream_t st);
// meads.cuh (the two rank-C products of an update run between meads_means and meads_finish)
hipError_t meads_set3(double *cell, double x, double y, double z, hipStream_t st);
hipError_t meads_means(const MeadsArgs &a, hipStream_t st);
hipError_t meads_finish(const MeadsArgs &a, hipStream_t st);
}  // namespace tu
}  // namespace aehmc
