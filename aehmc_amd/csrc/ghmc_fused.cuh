// Generalised HMC (Horowitz 1991; the persistent, non-reversible form of Hoffman & Sountsov, "Tuning-Free Generalized
// Hamiltonian Monte Carlo", AISTATS 2022), register-resident: one chain per wavefront, four per workgroup, lane l holds
// elements l, l + 64, ... in VGPRs, all T transitions of a call in ONE launch (k_ghmc_fused, D <= 1024).
//
// The momentum is kept WHITENED, v ~ N(0, I), kinetic energy v.v / 2; the preconditioner is a `scale` s (scalar or [D],
// shared by all chains) in the role of sqrt(inverse_mass_matrix), so a momentum stays valid when the warm-up rewrites s
// between two transitions.  A chain carries q, U, g = dU/dq, v and a slice variable u in (-1, 1).  One transition, with
// eps, alpha, delta read from device memory (params [3]):
//   1  z = D standard normals of site #1 (wave_normals: numpy's standard_normal(D))
//   2  v = sqrt(1 - alpha) v + sqrt(alpha) z          (no momentum handed in: the call's first transition sets v = z)
//   3  u = fmod((u + 1) + delta, 2) - 1               (no slice handed in: first u = 2 r - 1, r one double of site #2)
//   4  H0 = U + v.v / 2
//   5  vh = v - (eps / 2)(s g);  q' = q + eps (s vh);  g' = dU/dq(q');  v' = vh - (eps / 2)(s g')
//   6  d = H0 - (U' + v'.v' / 2), NaN -> -inf;  diverging: |d| > threshold;  acceptance probability min(1, exp d);
//      accept iff d > -inf and log|u| <= d: no random number
//   7  accept: (q, U, g, v) = (q', U', g', v'), u = u exp(-d);  reject: v = -v (the refreshed one), u as it is
// Steps 2, 3, 5 are elementwise fp64 in the written association (the library is compiled without contraction); the two
// energy sums are wavefront reductions.  Default arithmetic only: there is no fp_contract variant.
//
// Targets: the coordinate-wise ones of the library; in the run-time compiled copies AEHMC_T_CUSTOM (the user's
// aehmc_custom_elem) and AEHMC_T_JOINT with its reverse-mode program (AEHMC_JOINT_GRAD: position and gradient rows in
// LDS, the first doubling as the row of normals, as in k_hmc_fused).
#pragma once
#include <hip/hip_runtime.h>

#include "engine.cuh"

namespace aehmc {

struct GhmcArgs {
  long long C, D, T;
  double thr;
  const double *params;  // [3]: eps, alpha, delta
  const double *scale;   // [1] or [D]
  int scale_n;           // 1 or D
  int tkind;
  const double *mu, *sigma, *log_sigma;
  const double *const *cparams;  // user-defined target (run-time compiled instantiations only)
  uint64_t *rng;                 // [C,2,4]
  double *q, *U, *g;
  double *v;      // [C,D] whitened momentum: read if has_v, always written
  double *slice;  // [C]: read if has_slice, always written
  int has_v, has_slice;
  aehmc_diagnostics out;
  double *samples;    // [T,C,D] or null
  double *acc_hist;   // [T,C] or null
  int32_t *div_hist;  // [T,C] or null
};

inline bool ghmc_target_is_elem(int k) {
  return k == AEHMC_T_STD_NORMAL || k == AEHMC_T_ISO_GAUSSIAN || k == AEHMC_T_DIAG_GAUSSIAN;
}
constexpr long long GHMC_MAX_D = 1024;

#ifdef AEHMC_CUSTOM_TARGET
#define AEHMC_GHMC_CUSTOM_ELEM(q, i, u, g) aehmc_custom_elem((q), (i), a.cparams, (u), (g))
#else
#define AEHMC_GHMC_CUSTOM_ELEM(q, i, u, g) do { (u) = 0.0; (g) = 0.0; } while (0)
#endif

// a value every lane holds alike, moved to scalar registers
__device__ __forceinline__ double ghmc_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)),
                          __builtin_amdgcn_readfirstlane(__double2loint(x)));
}
// 4096 chains are 4 wavefronts per SIMD: the small instantiations are held to registers that leave room for them (the
// diagonal Gaussian at R = 4 keeps mu and sigma beside the chain and would spill 12 bytes per lane at that floor: 3)
constexpr int ghmc_min_waves(int R, int TK) {
  return TK == AEHMC_T_JOINT ? 1 : R <= 2 ? 4 : R == 4 ? (TK == AEHMC_T_DIAG_GAUSSIAN ? 3 : 4) : 1;
}

template <int R, int TK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ghmc_min_waves(R, TK)))) void k_ghmc_fused(GhmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double zlds[];  // [4 waves][R*64] (joint target: twice that)
  __shared__ double ztab[ZIG_LDS_DOUBLES];
  const ZigTabLds tab = zig_tab_to_lds(ztab);
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long c = (long long)blockIdx.x * 4 + w;
  if (c >= a.C) return;
  const size_t row = (size_t)c * a.D;
  double *zrow = zlds + (size_t)w * ((TK == AEHMC_T_JOINT ? 2 : 1) * R * 64);

  double q[R], g[R], v[R], qn[R], gn[R], vn[R], s[R], mu[R], sg[R];
  bool ok[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const long long i = lane + 64 * r;
    ok[r] = i < a.D;
    const long long ii = ok[r] ? i : 0;
    s[r] = a.scale[a.scale_n == 1 ? 0 : ii];
    mu[r] = TK == AEHMC_T_DIAG_GAUSSIAN ? a.mu[ii] : 0.0;
    sg[r] = TK == AEHMC_T_DIAG_GAUSSIAN ? a.sigma[ii] : 1.0;
    q[r] = ok[r] ? a.q[row + ii] : 0.0;
    g[r] = ok[r] ? a.g[row + ii] : 0.0;
    v[r] = (ok[r] && a.has_v) ? a.v[row + ii] : 0.0;
  }
  double U = a.U[c];
  Pcg64 g1 = pcg_load(a.rng + (size_t)c * 8);  // site #1: the momentum refreshment
  const double eps = ghmc_uniform(a.params[0]), alpha = ghmc_uniform(a.params[1]), delta = ghmc_uniform(a.params[2]);
  const double b = 0.5 * eps;
  const double keep = sqrt(1.0 - alpha), mix = sqrt(alpha);
  double u;
  if (a.has_slice) {
    u = ghmc_uniform(a.slice[c]);
  } else {  // site #2: the one draw it ever makes
    Pcg64 g2 = pcg_load(a.rng + (size_t)c * 8 + 4);
    const double r01 = pcg_next_double(g2);
    u = 2.0 * r01 - 1.0;
    if (lane == 0) pcg_store(a.rng + (size_t)c * 8 + 4, g2);
  }
  double pa = 0.0;
  int is_div = 0, acc = 0;

  const PcgLaneJump jump1 = pcg_lane_jump(g1);
  for (long long t = 0; t < a.T; t++) {
    wave_normals(g1, a.D, [=](long long i, double z) { zrow[i] = z; }, tab, jump1);
    __threadfence_block();
    const bool fresh = t == 0 && !a.has_v;  // (wave-uniform)
    double kd = 0.0;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const double z = ok[r] ? zrow[lane + 64 * r] : 0.0;
      v[r] = fresh ? z : keep * v[r] + mix * z;
      if (ok[r]) kd += v[r] * v[r];
    }
    __threadfence_block();
    kd = wave_sum(kd);
    u = fmod((u + 1.0) + delta, 2.0) - 1.0;
    const double H0 = U + 0.5 * kd;

    double usum = 0.0, U_joint = U;
    (void)U_joint;
    kd = 0.0;
#ifdef AEHMC_JOINT_GRAD
    if (TK == AEHMC_T_JOINT) {
      double *const grow = zrow + R * 64;
#pragma unroll
      for (int r = 0; r < R; r++) {
        vn[r] = v[r] - b * (s[r] * g[r]);
        qn[r] = q[r] + eps * (s[r] * vn[r]);
        if (ok[r]) {
          zrow[lane + 64 * r] = qn[r];
          grow[lane + 64 * r] = 0.0;
        }
      }
      __threadfence_block();
      const double lp = aehmc_logp_grad(zrow, grow, lane, a.cparams);
      __threadfence_block();
#pragma unroll
      for (int r = 0; r < R; r++) {
        gn[r] = ok[r] ? -grow[lane + 64 * r] : 0.0;
        vn[r] = vn[r] - b * (s[r] * gn[r]);
        if (ok[r]) kd += vn[r] * vn[r];
      }
      U_joint = -lp;
      __threadfence_block();
    } else
#endif
    {
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long i = ok[r] ? lane + 64 * r : 0;
        vn[r] = v[r] - b * (s[r] * g[r]);
        qn[r] = q[r] + eps * (s[r] * vn[r]);
        double ue = 0.0;
        if (TK == AEHMC_T_STD_NORMAL) {
          gn[r] = qn[r];
          ue = 0.5 * (qn[r] * qn[r]) + AEHMC_LOG_SQRT_2PI;
        } else if (TK == AEHMC_T_ISO_GAUSSIAN) {
          gn[r] = qn[r];
          ue = qn[r] * qn[r];
        } else if (TK == AEHMC_T_CUSTOM) {
          AEHMC_GHMC_CUSTOM_ELEM(qn[r], i, ue, gn[r]);
        } else if (TK == AEHMC_T_DIAG_GAUSSIAN) {
          const double zz = (qn[r] - mu[r]) / sg[r];
          gn[r] = zz / sg[r];
          ue = 0.5 * (zz * zz) + a.log_sigma[i] + AEHMC_LOG_SQRT_2PI;
        } else {
          gn[r] = 0.0;
        }
        vn[r] = vn[r] - b * (s[r] * gn[r]);
        if (ok[r]) {
          usum += ue;
          kd += vn[r] * vn[r];
        }
      }
      usum = wave_sum(usum);
    }
    kd = wave_sum(kd);
    const double Unew = TK == AEHMC_T_JOINT ? U_joint : (TK == AEHMC_T_ISO_GAUSSIAN ? 0.5 * usum : usum);
    double d = H0 - (Unew + 0.5 * kd);
    if (isnan(d)) d = -INFINITY;
    is_div = fabs(d) > a.thr;
    pa = exp(d);
    if (pa > 1.0) pa = 1.0;
    acc = d > -INFINITY && log(fabs(u)) <= d;
    if (acc) {  // (wave-uniform)
      U = Unew;
      u = u * exp(-d);
#pragma unroll
      for (int r = 0; r < R; r++) {
        q[r] = qn[r];
        g[r] = gn[r];
        v[r] = vn[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; r++) v[r] = -v[r];
    }
    if (a.samples) {
      double *dst = a.samples + ((size_t)t * a.C + c) * a.D;
#pragma unroll
      for (int r = 0; r < R; r++)
        if (ok[r]) dst[lane + 64 * r] = q[r];
    }
    if (lane == 0) {
      if (a.acc_hist) a.acc_hist[(size_t)t * a.C + c] = pa;
      if (a.div_hist) a.div_hist[(size_t)t * a.C + c] = is_div;
    }
  }

#pragma unroll
  for (int r = 0; r < R; r++) {
    if (ok[r]) {
      const long long i = lane + 64 * r;
      a.q[row + i] = q[r];
      a.g[row + i] = g[r];
      a.v[row + i] = v[r];
    }
  }
  if (lane == 0) {
    pcg_store(a.rng + (size_t)c * 8, g1);
    a.U[c] = U;
    a.slice[c] = u;
    a.out.acceptance_probability[c] = pa;
    a.out.is_diverging[c] = is_div;
    if (a.out.n_leapfrog) a.out.n_leapfrog[c] = a.T;
    if (a.out.is_turning) a.out.is_turning[c] = acc;  // reused as the accept flag, as HMC does
  }
}

// elements per lane of the instantiation that holds a D-dimensional chain
inline int ghmc_fused_r(long long D) {
  const long long r = (D + 63) / 64;
  return r <= 1 ? 1 : r <= 2 ? 2 : r <= 4 ? 4 : r <= 8 ? 8 : 16;
}
#ifndef __HIPCC_RTC__
inline size_t ghmc_fused_lds(int R, int tkind) { return (size_t)4 * (tkind == AEHMC_T_JOINT ? 2 : 1) * R * 64 * sizeof(double); }
template <int R>
inline hipError_t launch_ghmc_fused_r(const GhmcArgs &a, hipStream_t st) {
  const dim3 grid((unsigned)((a.C + 3) / 4)), block(256);
  const size_t lds = ghmc_fused_lds(R, a.tkind);
  switch (a.tkind) {
    case AEHMC_T_STD_NORMAL:
      hipLaunchKernelGGL((k_ghmc_fused<R, AEHMC_T_STD_NORMAL>), grid, block, lds, st, a);
      break;
    case AEHMC_T_ISO_GAUSSIAN:
      hipLaunchKernelGGL((k_ghmc_fused<R, AEHMC_T_ISO_GAUSSIAN>), grid, block, lds, st, a);
      break;
    case AEHMC_T_DIAG_GAUSSIAN:
      hipLaunchKernelGGL((k_ghmc_fused<R, AEHMC_T_DIAG_GAUSSIAN>), grid, block, lds, st, a);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
inline hipError_t launch_ghmc_fused(const GhmcArgs &a, hipStream_t st) {
  if (a.D < 1 || a.D > GHMC_MAX_D) return hipErrorInvalidValue;
  switch (ghmc_fused_r(a.D)) {
    case 1: return launch_ghmc_fused_r<1>(a, st);
    case 2: return launch_ghmc_fused_r<2>(a, st);
    case 4: return launch_ghmc_fused_r<4>(a, st);
    case 8: return launch_ghmc_fused_r<8>(a, st);
    default: return launch_ghmc_fused_r<16>(a, st);
  }
}
// the run-time compiled copy of that instantiation (AEHMC_T_CUSTOM; AEHMC_T_JOINT: the gradient rows of the program in
// LDS beside the position rows)
inline KernelLaunch ghmc_fused_launch(long long D, aehmc_target_kind tkind, long long C) {
  const int R = ghmc_fused_r(D);
  return {"aehmc::k_ghmc_fused<" + std::to_string(R) + ", " + std::to_string((int)tkind) + ">", dim3((unsigned)((C + 3) / 4)),
          dim3(256), ghmc_fused_lds(R, tkind)};
}
#endif  // __HIPCC_RTC__

}  // namespace aehmc
