// vb_glm.hip — device-resident regression targets (VB_TARGET_REGRESSION).
//
// log p(beta) = sum_d log N(beta_d; 0, s^2) + sum_m l(y_m, x_m . beta) and its
// gradient -beta / s^2 + sum_m l'(y_m, eta_m) x_m for the n sample rows beta of
// x [n][D], over the data matrix X [M][D] and responses y [M] of the target's
// parameter block (layout in include/viabel_amd.h), with the gaussian, student_t,
// bernoulli_logit, poisson_log and neg_binomial_2_log links; the two count links add
// the block's per-observation offset eta0 [M] to eta.  All arithmetic is fp64.
//
// The grid is sample-row tiles x observation chunks (x column slabs on the matrix
// path): a fit step has ~100 rows, so the observations must fill the chip.  Each
// block writes its chunk's partial log p and gradient; glm_combine_kernel adds the
// chunks in chunk order and the prior.  No atomics: the same call gives the same
// bits.  With one chunk the main kernel writes the final values itself.
//
//   D <= 16 (glm_rows_small_kernel): one lane per sample row, beta and the
//     gradient accumulator in registers, X / y staged 64 observations at a time
//     through LDS and read as broadcasts.
//   D > 16 (glm_rows_mfma_kernel): a 16-row sample tile per block, each of the
//     4 waves taking every 4th 16-observation tile of the chunk: eta = B X^T on
//     v_mfma_f64_16x16x4_f64 over D in LDS slices of 32 columns (zero padded in
//     LDS), the link applied to the accumulators, the residual tile handed
//     through LDS to the second product G += R X for the block's column slab
//     (<= 128 columns held in accumulators).  eta never leaves the registers.
//     MFMA operand maps as vb_gemm.hpp: A[l&15][k=l>>4], B[k=l>>4][l&15],
//     C row = (l>>4) + 4 r, col = l&15.
//     D > 128: one block per 128-column slab, each recomputing eta.
#include <algorithm>
#include <cmath>

#include "../../include/viabel_amd.h"
#include "vb_internal.hpp"

namespace vbk {
namespace {

using d4 = gemm_detail::d4;

constexpr int kGlmTile = 64;      // observations per LDS tile (small path) / per 4-wave round
constexpr int kGlmKD = 32;        // columns per LDS slice (matrix path)
constexpr int kGlmSX = 34;        // LDS row stride of a 32-column slice (vb_gemm.hpp's [row][k])
constexpr int kGlmSR = 17;        // LDS row stride of the residual tile
constexpr int kGlmWave = 2 * 16 * kGlmSX + 16 * kGlmSR;   // doubles of LDS per wave
constexpr long long kGlmScratchMax = 32LL << 20;          // doubles of chunk partials at most

struct GlmK {
  int D, nchunk;
  long long n, M, chunk_obs;
  double k0, k1, k2, k3;   // link constants (glm_link)
  double inv_s2, c_all;    // prior precision; every constant of log p (prior + M observations)
  const double* X;         // [M][D]
  const double* y;         // [M]
  const double* x;         // [n][D]
  double* logp;            // [n]
  double* grad;            // [n][D] or null
  double* plp;             // [nchunk][n]      (nchunk > 1)
  double* pg;              // [nchunk][n][D]   (nchunk > 1, grad)
  const double* eta0;      // [M]: offset of eta (LIK >= 3; not read otherwise)
};

// l(y, eta) without its constant, and dl / d eta
template <int LIK>
__device__ __forceinline__ void glm_link(const GlmK& k, double eta, double y, double& l,
                                         double& dl) {
  if constexpr (LIK == 0) {          // gaussian: k0 = 1 / sigma^2
    const double r = y - eta;
    l = -0.5 * k.k0 * (r * r);
    dl = k.k0 * r;
  } else if constexpr (LIK == 1) {   // student_t: k0 = 1 / (nu sigma^2), k1 = (nu + 1) / 2,
    const double r = y - eta;        //            k2 = nu + 1, k3 = nu sigma^2
    const double r2 = r * r;
    l = -k.k1 * log1p(r2 * k.k0);
    dl = k.k2 * r / (k.k3 + r2);
  } else if constexpr (LIK == 2) {   // bernoulli_logit: softplus and the logistic from one exp
    const double e = exp(-fabs(eta));
    l = y * eta - (fmax(eta, 0.0) + log1p(e));
    const double inv = 1.0 / (1.0 + e);
    dl = y - (eta >= 0.0 ? inv : e * inv);
  } else if constexpr (LIK == 3) {   // poisson_log: -inf past exp's range, no clamp
    const double e = exp(eta);
    l = y * eta - e;
    dl = y - e;
  } else {                           // neg_binomial_2_log: k0 = phi, k1 = log phi;
    const double z = eta - k.k1;     // (y + phi) softplus(zeta), zeta = eta - log phi
    const double e = exp(-fabs(z));
    const double yp = y + k.k0;
    l = y * eta - yp * (fmax(z, 0.0) + log1p(e));
    const double inv = 1.0 / (1.0 + e);
    dl = y - yp * (z >= 0.0 ? inv : e * inv);
  }
}

__device__ __forceinline__ double glm_final_logp(const GlmK& k, double sum_l, double ss) {
  return k.c_all + (sum_l - 0.5 * k.inv_s2 * ss);
}

// ---- D <= 16: one lane per sample row ------------------------------------------
template <int LIK, bool GRAD, int DP>
__global__ __launch_bounds__(256) void glm_rows_small_kernel(GlmK k) {
  __shared__ double Xs[kGlmTile * DP];
  constexpr bool OFFS = LIK >= 3;               // eta0 rides behind y in the tile
  __shared__ double ys[OFFS ? 2 * kGlmTile : kGlmTile];
  const int t = threadIdx.x, nt = blockDim.x, D = k.D;
  const long long row = (long long)blockIdx.x * nt + t;
  const bool live = row < k.n;
  double beta[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    beta[d] = (live && d < D) ? k.x[row * D + d] : 0.0;
    g[d] = 0.0;
  }
  double lp = 0.0;
  const long long m0 = (long long)blockIdx.y * k.chunk_obs;
  const long long m1 = m0 + k.chunk_obs < k.M ? m0 + k.chunk_obs : k.M;
  for (long long mt = m0; mt < m1; mt += kGlmTile) {
    const int cnt = m1 - mt < kGlmTile ? (int)(m1 - mt) : kGlmTile;
    __syncthreads();
    for (int i = t; i < kGlmTile * DP; i += nt) {
      const int mm = i / DP, d = i % DP;
      Xs[i] = (mm < cnt && d < D) ? k.X[(mt + mm) * D + d] : 0.0;
    }
    for (int i = t; i < kGlmTile; i += nt) ys[i] = i < cnt ? k.y[mt + i] : 0.0;
    if constexpr (OFFS) {
      for (int i = t; i < kGlmTile; i += nt) ys[kGlmTile + i] = i < cnt ? k.eta0[mt + i] : 0.0;
    }
    __syncthreads();
    for (int mm = 0; mm < cnt; ++mm) {
      const double* xr = Xs + mm * DP;
      double eta = 0.0;
#pragma unroll
      for (int d = 0; d < DP; ++d) eta = fma(beta[d], xr[d], eta);
      if constexpr (OFFS) eta += ys[kGlmTile + mm];
      double l, dl;
      glm_link<LIK>(k, eta, ys[mm], l, dl);
      lp += l;
      if constexpr (GRAD) {
#pragma unroll
        for (int d = 0; d < DP; ++d) g[d] = fma(dl, xr[d], g[d]);
      }
    }
  }
  if (!live) return;
  if (k.nchunk == 1) {
    double ss = 0.0;
#pragma unroll
    for (int d = 0; d < DP; ++d) ss = fma(beta[d], beta[d], ss);
    k.logp[row] = glm_final_logp(k, lp, ss);
    if constexpr (GRAD) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) k.grad[row * D + d] = g[d] - beta[d] * k.inv_s2;
    }
  } else {
    const long long pr = (long long)blockIdx.y * k.n + row;
    k.plp[pr] = lp;
    if constexpr (GRAD) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) k.pg[pr * D + d] = g[d];
    }
  }
}

// ---- D > 16: 16 sample rows x 16 observations per MFMA tile -----------------------
// dst [16][kGlmSX] <- src[r0 + i][c0 + j] (row stride D), i < 16, j < 32; zero for
// rows >= rmax and columns >= D.  One wave.
__device__ __forceinline__ void glm_stage(double* dst, const double* src, long long r0,
                                          long long rmax, int c0, int D, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = i * 64 + lane, rr = idx >> 5, cc = idx & 31;
    double v = 0.0;
    if (r0 + rr < rmax && c0 + cc < D) v = src[(r0 + rr) * D + c0 + cc];
    dst[rr * kGlmSX + cc] = v;
  }
}

template <int LIK, bool GRAD, int NCT>
__global__ __launch_bounds__(256) void glm_rows_mfma_kernel(GlmK k) {
  __shared__ double smem[4 * kGlmWave];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, lr = lane & 15, lq = lane >> 4;
  double* Xs = smem + w * kGlmWave;
  double* Bs = Xs + 16 * kGlmSX;
  double* Rs = Bs + 16 * kGlmSX;
  const int D = k.D;
  const int nK = (D + kGlmKD - 1) / kGlmKD;
  const long long row0 = (long long)blockIdx.x * 16;
  const int col0 = (int)blockIdx.z * (NCT * 16);
  const long long m0 = (long long)blockIdx.y * k.chunk_obs;
  const long long m1 = m0 + k.chunk_obs < k.M ? m0 + k.chunk_obs : k.M;
  const int ntiles = (int)((m1 - m0 + 15) / 16);
  const int rounds = (ntiles + 3) / 4;
  d4 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  double lpa[4] = {0.0, 0.0, 0.0, 0.0};

  // every wave runs the same number of rounds (the barriers are block-wide); a wave
  // without a tile in the last round only takes part in the barriers
  for (int it = 0; it < rounds; ++it) {
    const int tile = it * 4 + w;
    const bool valid = tile < ntiles;
    const long long mt = m0 + (long long)tile * 16;
    d4 e0 = d4{0.0, 0.0, 0.0, 0.0}, e1 = e0;
    for (int kt = 0; kt < nK; ++kt) {
      __syncthreads();
      if (valid) {
        glm_stage(Xs, k.X, mt, m1, kt * kGlmKD, D, lane);
        // one slice holds every column: the sample tile is staged once
        if (nK > 1 || it == 0) glm_stage(Bs, k.x, row0, k.n, kt * kGlmKD, D, lane);
      }
      __syncthreads();
      if (valid) {
#pragma unroll
        for (int s = 0; s < kGlmKD / 4; s += 2) {
          e0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[lr * kGlmSX + 4 * s + lq],
                                                    Xs[lr * kGlmSX + 4 * s + lq], e0, 0, 0, 0);
          e1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Bs[lr * kGlmSX + 4 * s + 4 + lq],
                                                    Xs[lr * kGlmSX + 4 * s + 4 + lq], e1, 0, 0, 0);
        }
      }
    }
    if (valid) {
      // lane: sample rows lq + 4 r, observation mt + lr
      const d4 eta = e0 + e1;
      const bool ok = mt + lr < m1;
      const double yv = ok ? k.y[mt + lr] : 0.0;
      double ev = 0.0;
      if constexpr (LIK >= 3) ev = ok ? k.eta0[mt + lr] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double l, dl;
        if constexpr (LIK >= 3)
          glm_link<LIK>(k, eta[r] + ev, yv, l, dl);
        else
          glm_link<LIK>(k, eta[r], yv, l, dl);
        lpa[r] += ok ? l : 0.0;
        if constexpr (GRAD) Rs[(lq + 4 * r) * kGlmSR + lr] = ok ? dl : 0.0;
      }
    }
    if constexpr (GRAD) {
      // G[rows][slab columns] += R [16 x 16 observations] X [16 observations][columns]
#pragma unroll
      for (int cs = 0; cs < NCT / 2; ++cs) {
        if (nK > 1) {   // (one slice: Xs already holds the tile's columns 0..31)
          __syncthreads();
          if (valid) glm_stage(Xs, k.X, mt, m1, col0 + cs * 32, D, lane);
        }
        __syncthreads();
        if (valid) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc[cs * 2 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                  Rs[lr * kGlmSR + 4 * s + lq], Xs[(4 * s + lq) * kGlmSX + j * 16 + lr],
                  acc[cs * 2 + j], 0, 0, 0);
          }
        }
      }
    }
  }

  // the waves' partial sums meet in LDS, added in wave order
  double* red = smem;
  const bool fin = k.nchunk == 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) lpa[r] += __shfl_xor(lpa[r], off, 64);
  }
  __syncthreads();
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w * 16 + lq + 4 * r] = lpa[r];
  }
  __syncthreads();
  if (blockIdx.z == 0 && t < 16 && row0 + t < k.n) {
    const long long row = row0 + t;
    const double s = ((red[t] + red[16 + t]) + red[32 + t]) + red[48 + t];
    if (fin) {
      double ss = 0.0;
      for (int d = 0; d < D; ++d) {
        const double b = k.x[row * D + d];
        ss = fma(b, b, ss);
      }
      k.logp[row] = glm_final_logp(k, s, ss);
    } else {
      k.plp[(long long)blockIdx.y * k.n + row] = s;
    }
  }
  if constexpr (GRAD) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w * 256 + r * 64 + lane] = acc[c][r];
      __syncthreads();
      const int ln = t & 63, rr = (ln >> 4) + 4 * (t >> 6), col = col0 + c * 16 + (ln & 15);
      const long long row = row0 + rr;
      if (row < k.n && col < D) {
        const double s = ((red[t] + red[256 + t]) + red[512 + t]) + red[768 + t];
        if (fin)
          k.grad[row * D + col] = s - k.x[row * D + col] * k.inv_s2;
        else
          k.pg[((long long)blockIdx.y * k.n + row) * D + col] = s;
      }
    }
  }
}

// chunk partials, added in chunk order, and the prior: job i < n is log p of row i,
// job n + j is gradient entry j of [n][D]
__global__ __launch_bounds__(256) void glm_combine_kernel(GlmK k, int with_grad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nd = k.n * k.D;
  if (i < k.n) {
    double s = 0.0;
    for (int c = 0; c < k.nchunk; ++c) s += k.plp[(long long)c * k.n + i];
    double ss = 0.0;
    for (int d = 0; d < k.D; ++d) {
      const double b = k.x[i * k.D + d];
      ss = fma(b, b, ss);
    }
    k.logp[i] = glm_final_logp(k, s, ss);
  } else if (with_grad && i - k.n < nd) {
    const long long j = i - k.n;
    double s = 0.0;
    for (int c = 0; c < k.nchunk; ++c) s += k.pg[(long long)c * nd + j];
    k.grad[j] = s - k.x[j] * k.inv_s2;
  }
}

int glm_cu_count() {
  static int cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] > 0) return cached[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    n = 256;
  }
  cached[dev] = n;
  return n;
}

struct GlmPlan {
  bool small;
  int tb;              // threads per block
  int nchunk, nct, nslab;
  long long chunk_obs, row_blocks;
};

// Chunking rule: enough observation chunks that row tiles x chunks reach 4 blocks
// per CU (a 100-row step fills the chip), none when the row tiles alone do (10^6
// bound draws); a chunk is a whole number of 64-observation tiles; the partials
// stay under kGlmScratchMax doubles.
GlmPlan glm_plan(int D, long long n, long long M, bool grad) {
  GlmPlan p{};
  p.small = D <= kBlockDMax;
  p.tb = p.small ? (n <= 4096 ? 64 : 256) : 256;
  const long long rpb = p.small ? p.tb : 16;
  p.row_blocks = (n + rpb - 1) / rpb;
  const long long target = 4LL * glm_cu_count();
  const long long max_chunks = std::min<long long>((M + kGlmTile - 1) / kGlmTile, 1024);
  long long nc = std::max<long long>(1, std::min(max_chunks, (target + p.row_blocks - 1) / p.row_blocks));
  const long long per = std::max<long long>(1, n) * (1 + (grad ? D : 0));
  if (nc > 1 && nc * per > kGlmScratchMax) nc = std::max<long long>(1, kGlmScratchMax / per);
  long long co = (M + nc - 1) / nc;
  co = (co + kGlmTile - 1) / kGlmTile * kGlmTile;
  p.chunk_obs = co;
  p.nchunk = (int)((M + co - 1) / co);
  p.nct = D <= 32 ? 2 : D <= 64 ? 4 : 8;
  p.nslab = grad ? (D + p.nct * 16 - 1) / (p.nct * 16) : 1;
  return p;
}

template <int LIK, bool GRAD>
void glm_launch_small(const GlmPlan& p, const GlmK& k, hipStream_t s) {
  const dim3 g((unsigned)p.row_blocks, (unsigned)p.nchunk), b(p.tb);
  if (k.D <= 2)
    hipLaunchKernelGGL((glm_rows_small_kernel<LIK, GRAD, 2>), g, b, 0, s, k);
  else if (k.D <= 4)
    hipLaunchKernelGGL((glm_rows_small_kernel<LIK, GRAD, 4>), g, b, 0, s, k);
  else if (k.D <= 8)
    hipLaunchKernelGGL((glm_rows_small_kernel<LIK, GRAD, 8>), g, b, 0, s, k);
  else
    hipLaunchKernelGGL((glm_rows_small_kernel<LIK, GRAD, 16>), g, b, 0, s, k);
}

template <int LIK>
void glm_launch(const GlmPlan& p, const GlmK& k, hipStream_t s) {
  const bool grad = k.grad != nullptr;
  if (p.small) {
    if (grad)
      glm_launch_small<LIK, true>(p, k, s);
    else
      glm_launch_small<LIK, false>(p, k, s);
    return;
  }
  const dim3 g((unsigned)p.row_blocks, (unsigned)p.nchunk, (unsigned)p.nslab), b(256);
  if (!grad)
    hipLaunchKernelGGL((glm_rows_mfma_kernel<LIK, false, 2>), g, b, 0, s, k);
  else if (p.nct == 2)
    hipLaunchKernelGGL((glm_rows_mfma_kernel<LIK, true, 2>), g, b, 0, s, k);
  else if (p.nct == 4)
    hipLaunchKernelGGL((glm_rows_mfma_kernel<LIK, true, 4>), g, b, 0, s, k);
  else
    hipLaunchKernelGGL((glm_rows_mfma_kernel<LIK, true, 8>), g, b, 0, s, k);
}

// lgamma(x + 1/2) - lgamma(x) - log(x) / 2 for x > 0, to a few 2^-53 absolute.  The
// difference of the two lgamma loses the digits of M c_obs as nu grows (~1e-9 per
// observation at nu = 1e6).  From x >= 32 the asymptotic series (next term < 4e-22); a
// smaller x climbs there by Gamma(x + 1) = x Gamma(x); below 1 the two lgamma are small
// and their difference is taken as it stands.
double lgamma_half_step(double x) {
  if (x < 1.0) return std::lgamma(x + 0.5) - std::lgamma(x) - 0.5 * std::log(x);
  const double x0 = x;
  double steps = 0.0;
  while (x < 32.0) {
    steps += std::log1p(0.5 / x);
    x += 1.0;
  }
  const double t = 1.0 / x, t2 = t * t;
  const double tail =
      t * (-1.0 / 8 + t2 * (1.0 / 192 + t2 * (-1.0 / 640 + t2 * (17.0 / 14336 + t2 * (-31.0 / 18432 + t2 * (691.0 / 180224))))));
  return x == x0 ? tail : tail + (0.5 * std::log(x / x0) - steps);
}

}  // namespace

size_t glm_scratch_doubles(int D, long long n, long long M, bool grad) {
  if (n < 1) return 0;
  const GlmPlan p = glm_plan(D, n, M, grad);
  return p.nchunk > 1 ? (size_t)p.nchunk * (size_t)n * (size_t)(1 + (grad ? D : 0)) : 0;
}

hipError_t launch_glm_rows(int D, long long n, const GlmHead& h, const double* params,
                           const double* x, double* logp, double* grad, double* scratch,
                           hipStream_t s) {
  if (n < 1) return hipSuccess;
  const GlmPlan p = glm_plan(D, n, h.M, grad != nullptr);
  if (p.row_blocks > 0x7fffffffLL || p.nslab > 65535) return hipErrorInvalidValue;
  if (p.nchunk > 1 && !scratch) return hipErrorInvalidValue;
  GlmK k{};
  k.D = D;
  k.nchunk = p.nchunk;
  k.n = n;
  k.M = h.M;
  k.chunk_obs = p.chunk_obs;
  double c_obs = 0.0;
  const double log2pi = 1.8378770664093454835606594728112;
  if (h.lik == 0) {
    k.k0 = 1.0 / (h.sigma * h.sigma);
    c_obs = -0.5 * log2pi - std::log(h.sigma);
  } else if (h.lik == 1) {
    k.k3 = h.nu * (h.sigma * h.sigma);
    k.k0 = 1.0 / k.k3;
    k.k1 = 0.5 * (h.nu + 1.0);
    k.k2 = h.nu + 1.0;
    // lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2, the log(nu / 2) / 2 cancelled
    c_obs = lgamma_half_step(0.5 * h.nu) - 0.5 * log2pi - std::log(h.sigma);
  } else if (h.lik == 4) {
    k.k0 = h.phi;
    k.k1 = std::log(h.phi);
  }
  k.inv_s2 = 1.0 / (h.prior * h.prior);
  k.c_all = -(double)D * (0.5 * log2pi + std::log(h.prior)) + (double)h.M * c_obs;
  if (h.lik >= 3) k.c_all += h.c_data;   // the data-only constants, summed by the packer
  k.X = params + kGlmHeader;
  k.y = k.X + (size_t)h.M * D;
  k.eta0 = h.lik >= 3 ? k.y + h.M : nullptr;
  k.x = x;
  k.logp = logp;
  k.grad = grad;
  k.plp = scratch;
  k.pg = scratch ? scratch + (size_t)p.nchunk * n : nullptr;
  if (h.lik == 0)
    glm_launch<0>(p, k, s);
  else if (h.lik == 1)
    glm_launch<1>(p, k, s);
  else if (h.lik == 2)
    glm_launch<2>(p, k, s);
  else if (h.lik == 3)
    glm_launch<3>(p, k, s);
  else
    glm_launch<4>(p, k, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.nchunk == 1) return e;
  const long long jobs = n + (grad ? n * D : 0);
  hipLaunchKernelGGL(glm_combine_kernel, dim3((unsigned)((jobs + 255) / 256)), dim3(256), 0, s, k,
                     grad ? 1 : 0);
  return hipGetLastError();
}

}  // namespace vbk
