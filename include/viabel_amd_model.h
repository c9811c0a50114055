/*
 * viabel_amd_model.h — device-side helpers for writing a model plugin
 * (VB_TARGET_PLUGIN, include/viabel_amd.h "Device model plugins").
 *
 * A plugin is a gfx950 code object with a kernel
 *   extern "C" __global__ void NAME(const double* x, long long n, int D, const double* data,
 *                                   long long n_data, double* logp, double* grad)
 * and its launch record, extern "C" __device__ const int NAME_launch[3] =
 * {block, rows_per_block, dmax}.  With this header the user writes one device function
 * and a macro makes both:
 *
 *   VB_MODEL_ROWS(NAME, fn)                one lane per sample row; record {256, 256, 0}
 *     double fn(const double* x, int D, const double* data, long long n_data,
 *               double* grad_or_null)      returns log p(x), writes grad[0 .. D) when non-null
 *
 *   VB_MODEL_SUM(NAME, DMAX, prior, term)  log p(x) = prior(x) + sum_{m < M} term(x, m),
 *                                          M = data[0]; one wave per sample row, four rows
 *                                          per 256-thread block; record {256, 4, DMAX}
 *     double prior(const double* x, int D, const double* data, double* g)
 *     double term(const double* x, int D, const double* data, long long m, double* g)
 *       both return their part of log p and ADD their part of the gradient to g[0 .. D).
 *       g is never null and is a register array of DMAX doubles: index it with
 *       compile-time constants only (a `#pragma unroll` loop over d < DMAX with an
 *       `if (d < D)` guard) and do not compare it with null; a run-time index or a null
 *       test sends it to scratch memory.  Log-weight calls (grad == null) run an instance
 *       that never reads g, so the compiler drops the gradient work there and the value
 *       is the same bits.  x points to the sample's row, staged once into LDS.
 *
 * Compile:  hipcc --genco --offload-arch=gfx950 -O3 -std=c++17 -I include model.hip -o model.hsaco
 * (viabel_amd.plugin.compile does this).  No fast-math: the library's own kernels keep IEEE
 * semantics and so should a model.
 *
 * The sum form's reduction has a fixed order: lane l adds the observations m = l, l + 64,
 * ... in ascending order, then the 64 lane sums are added by a fixed butterfly (DPP row
 * operations and the gfx950 permlane swaps, the library's own wave sum).  No atomics: the
 * same call gives the same bits every time.
 */
#ifndef VIABEL_AMD_MODEL_H
#define VIABEL_AMD_MODEL_H

#include <hip/hip_runtime.h>

namespace vbm {

// ---- wave-wide sum of a double (wave64): every lane ends with the same total ----
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double swap_sum16(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

__device__ __forceinline__ double swap_sum32(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}

__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  v = swap_sum16(v);       // rows 0+1, 2+3
  return swap_sum32(v);    // halves
}

constexpr int kSumBlock = 256;  // threads per block of the sum form
constexpr int kSumRows = 4;     // sample rows per block: one wave each

// The wave of one sample row: lanes stride over the observations with log p and the
// gradient sums in registers, the wave sums them, lane 0 adds the prior and stores.
// GRAD false: g is never read, so its sums are dead code (the value is the same bits).
template <int DMAX, bool GRAD, class Prior, class Term>
__device__ __forceinline__ void sum_row(Prior prior, Term term, const double* xs, int D,
                                        const double* data, int lane, double* logp_r,
                                        double* grad_r) {
  const long long M = data ? (long long)data[0] : 0;   // no data block: the prior alone
  double g[DMAX];
#pragma unroll
  for (int d = 0; d < DMAX; ++d) g[d] = 0.0;
  double lp = 0.0;
  for (long long m = lane; m < M; m += 64) lp += term(xs, D, data, m, g);
  lp = wave_sum(lp);
  if (GRAD) {
#pragma unroll
    for (int d = 0; d < DMAX; ++d)
      if (d < D) g[d] = wave_sum(g[d]);   // D is uniform over the wave
  }
  if (lane == 0) {
    lp += prior(xs, D, data, g);
    *logp_r = lp;
    if (GRAD) {
#pragma unroll
      for (int d = 0; d < DMAX; ++d)
        if (d < D) grad_r[d] = g[d];
    }
  }
}

template <int DMAX, class Prior, class Term>
__device__ __forceinline__ void sum_kernel(Prior prior, Term term, const double* x, long long n,
                                           int D, const double* data, double* logp, double* grad) {
  __shared__ double xs[kSumRows][DMAX];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const long long r = (long long)blockIdx.x * kSumRows + wave;
  // the loader refuses dim > DMAX; a launch outside it writes nothing rather than past xs.
  // Whole waves leave here: no block-wide barrier follows
  if (r >= n || D > DMAX) return;
  for (int d = lane; d < D; d += 64) xs[wave][d] = x[r * D + d];
  // the row is read back by every lane of this wave only: a wave's LDS operations
  // complete in order, and the fence keeps the compiler from moving reads above the store
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (grad)
    sum_row<DMAX, true>(prior, term, xs[wave], D, data, lane, logp + r, grad + r * D);
  else
    sum_row<DMAX, false>(prior, term, xs[wave], D, data, lane, logp + r, nullptr);
}

}  // namespace vbm

#define VB_MODEL_ARGS                                                                   \
  const double *x, long long n, int D, const double *data, long long n_data, double *logp, \
      double *grad

// One lane per sample row.
#define VB_MODEL_ROWS(NAME, FN)                                                            \
  extern "C" __device__ __attribute__((used, visibility("default"))) const int NAME##_launch[3] = { \
      256, 256, 0};                                                                        \
  extern "C" __global__ __launch_bounds__(256) void NAME(VB_MODEL_ARGS) {                  \
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;                         \
    if (r >= n) return;                                                                    \
    logp[r] = FN(x + r * D, D, data, n_data, grad ? grad + r * D : nullptr);               \
  }

// One wave per sample row over the M = data[0] observations; D <= DMAX.
#define VB_MODEL_SUM(NAME, DMAX, PRIOR, TERM)                                              \
  extern "C" __device__ __attribute__((used, visibility("default"))) const int NAME##_launch[3] = { \
      vbm::kSumBlock, vbm::kSumRows, DMAX};                                                \
  extern "C" __global__ __launch_bounds__(256) void NAME(VB_MODEL_ARGS) {                  \
    (void)n_data;                                                                          \
    vbm::sum_kernel<DMAX>(                                                                 \
        [](const double* xx, int dd, const double* dt, double* g) {                        \
          return PRIOR(xx, dd, dt, g);                                                     \
        },                                                                                 \
        [](const double* xx, int dd, const double* dt, long long m, double* g) {           \
          return TERM(xx, dd, dt, m, g);                                                   \
        },                                                                                 \
        x, n, D, data, logp, grad);                                                        \
  }

#endif /* VIABEL_AMD_MODEL_H */
