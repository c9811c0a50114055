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
//
// Learned scale / dispersion (the block's `learn` field): the sample rows are [beta (p),
// lambda], lambda = log sigma (gaussian, student_t) or log phi (neg_binomial_2_log), X is
// [M][p].  The same two kernels serve it as the instances LIK = 5, 6, 7 (the learned forms
// of 0, 1, 4), chosen BY p EXACTLY AS A FIXED BLOCK WITH D = p IS: p <= 16 the lane-per-row
// kernel (DP from p), p > 16 the matrix kernel with NCT and the column slabs from p.
// Column p (lambda) never enters the R X product: the sample rows have their own stride
// (p + 1) and their own bound (p).  The link constants depend on the row: a lane of the
// lane-per-row kernel forms its own in its prologue (one exp); the matrix kernel keeps
// 16 rows x 2 doubles in LDS behind the waves' tiles (a lane serves the rows lq + 4 r; in
// registers they would cost 16 VGPRs beside the 8 of the second accumulator) and reads
// them as broadcasts (16 lanes per address).  sum_m dl/dlambda is a second per-row scalar
// beside lp: same wave reduction, same wave-order LDS sum, same writer, a partial array
// pla [nchunk][n] beside plp.  The gaussian needs none: sum_m (-1 + r^2 / sigma^2) =
// -M - 2 sum_m l_m.  The negative binomial's table sums A(phi) = sum_j T_j log1p(j / phi)
// and dA/dlambda = -sum_j T_j j / (phi + j) are formed once per call by glm_disp_kernel.
// The learned links, the prior of lambda and the table sums are defined in vb_links.hpp,
// which vb_mlm.hip's learned instances share.
#include <algorithm>
#include <cmath>

#include "../../include/viabel_amd.h"
#include "vb_internal.hpp"
#include "vb_links.hpp"

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
  LinkK lk;                // link constants (vb_links.hpp)
  double inv_s2, c_all;    // prior precision; every constant of log p (prior + M observations)
  const double* X;         // [M][D]
  const double* y;         // [M]
  const double* x;         // [n][D]
  double* logp;            // [n]
  double* grad;            // [n][D] or null
  double* plp;             // [nchunk][n]      (nchunk > 1)
  double* pg;              // [nchunk][n][D]   (nchunk > 1, grad)
  const double* eta0;      // [M]: offset of eta (LIK 3, 4, 7; not read otherwise)
  // learned mode (LIK >= 5): D above is p, the columns of X; x and grad have Dx = p + 1
  // columns, column p is lambda
  int Dx;
  long long J;             // length of T (LIK 7)
  double nu, inv_nu;       // student_t (lk.k1, lk.k2 as in obs_link)
  double ls_aux, Mf;       // log s_aux; M as a double
  const double* T;         // [J]: T[j] = #{m : y_m > j}
  double* tab;             // [2][n]: A(phi), dA/dlambda of the rows (LIK 7)
  double* pla;             // [nchunk][n]  (nchunk > 1, grad; LIK 6, 7)
};

__device__ __forceinline__ double glm_final_logp(const GlmK& k, double sum_l, double ss) {
  return k.c_all + (sum_l - 0.5 * k.inv_s2 * ss);
}

// learned mode: log p and d log p / d lambda of one row from its reduced sums: the prior
// of beta, -M lambda (gaussian, student_t), the half-Cauchy prior of e^lambda with its
// Jacobian, softplus and the logistic of w = 2 (lambda - log s_aux) from one exp, and the
// table sums of the negative binomial
template <int LIK>
__device__ __forceinline__ void glm_aux_final(const GlmK& k, long long row, double lam,
                                              double sum_l, double sum_la, double ss, double& lp,
                                              double& gl) {
  double sp, lg;
  aux_lambda_prior(lam, k.ls_aux, sp, lg);
  const double v = k.c_all + (sum_l - 0.5 * k.inv_s2 * ss);
  const double gp = 1.0 - 2.0 * lg;
  if constexpr (LIK == 7) {
    lp = v + ((lam - sp) + k.tab[row]);
    gl = (sum_la + k.tab[k.n + row]) + gp;
  } else {
    lp = v + (fma(-k.Mf, lam, lam) - sp);
    if constexpr (LIK == 5)
      gl = (-2.0 * sum_l - k.Mf) + gp;
    else
      gl = (sum_la - k.Mf) + gp;
  }
}

// ---- D <= 16: one lane per sample row ------------------------------------------
template <int LIK, bool GRAD, int DP>
__global__ __launch_bounds__(256) void glm_rows_small_kernel(GlmK k) {
  __shared__ double Xs[kGlmTile * DP];
  constexpr bool OFFS = link_offset(LIK);       // eta0 rides behind y in the tile
  constexpr bool LRN = link_learned(LIK);
  __shared__ double ys[OFFS ? 2 * kGlmTile : kGlmTile];
  const int t = threadIdx.x, nt = blockDim.x, D = k.D;
  const int Dx = LRN ? k.Dx : D;                // row stride of x and grad
  const long long row = (long long)blockIdx.x * nt + t;
  const bool live = row < k.n;
  double beta[DP], g[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    beta[d] = (live && d < D) ? k.x[row * Dx + d] : 0.0;
    g[d] = 0.0;
  }
  double lp = 0.0;
  double lam = 0.0, ca = 0.0, cb = 0.0, la = 0.0;   // learned mode only
  if constexpr (LRN) {
    lam = live ? k.x[row * Dx + D] : 0.0;
    glm_row_consts<LIK>(lam, ca, cb);
  }
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
      if constexpr (LRN) {
        double dlam;
        glm_link_aux<LIK>(k, ca, cb, eta, ys[mm], l, dl, dlam);
        if constexpr (GRAD && LIK != 5) la += dlam;
      } else {
        obs_link<LIK>(k.lk, eta, ys[mm], l, dl);
      }
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
    if constexpr (LRN) {
      double lpv, gl;
      glm_aux_final<LIK>(k, row, lam, lp, la, ss, lpv, gl);
      k.logp[row] = lpv;
      if constexpr (GRAD) k.grad[row * Dx + D] = gl;
    } else {
      k.logp[row] = glm_final_logp(k, lp, ss);
    }
    if constexpr (GRAD) {
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) k.grad[row * Dx + d] = g[d] - beta[d] * k.inv_s2;
    }
  } else {
    const long long pr = (long long)blockIdx.y * k.n + row;
    k.plp[pr] = lp;
    if constexpr (GRAD) {
      if constexpr (LRN && LIK != 5) k.pla[pr] = la;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) k.pg[pr * D + d] = g[d];
    }
  }
}

// ---- D > 16: 16 sample rows x 16 observations per MFMA tile -----------------------
// dst [16][kGlmSX] <- src[r0 + i][c0 + j] (row stride ld), i < 16, j < 32; zero for
// rows >= rmax and columns >= D.  One wave.
__device__ __forceinline__ void glm_stage(double* dst, const double* src, long long r0,
                                          long long rmax, int c0, int D, int ld, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = i * 64 + lane, rr = idx >> 5, cc = idx & 31;
    double v = 0.0;
    if (r0 + rr < rmax && c0 + cc < D) v = src[(r0 + rr) * ld + c0 + cc];
    dst[rr * kGlmSX + cc] = v;
  }
}

template <int LIK, bool GRAD, int NCT>
__global__ __launch_bounds__(256) void glm_rows_mfma_kernel(GlmK k) {
  constexpr bool OFFS = link_offset(LIK);
  constexpr bool LRN = link_learned(LIK);
  constexpr bool LACC = LRN && GRAD && LIK != 5;   // a second per-row accumulator
  // learned mode: the 16 rows' link constants (ca, cb) behind the waves' tiles
  __shared__ double smem[4 * kGlmWave + (LRN ? 32 : 0)];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, lr = lane & 15, lq = lane >> 4;
  double* Xs = smem + w * kGlmWave;
  double* Bs = Xs + 16 * kGlmSX;
  double* Rs = Bs + 16 * kGlmSX;
  const int D = k.D;
  const int Dx = LRN ? k.Dx : D;                // row stride of x and grad
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
  double laa[4] = {0.0, 0.0, 0.0, 0.0};          // LACC only
  if constexpr (LRN) {
    // read after the first barrier of the loop below (every chunk has a tile)
    if (t < 16) {
      double ca, cb;
      glm_row_consts<LIK>(row0 + t < k.n ? k.x[(row0 + t) * Dx + D] : 0.0, ca, cb);
      smem[4 * kGlmWave + 2 * t] = ca;
      smem[4 * kGlmWave + 2 * t + 1] = cb;
    }
  }

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
        glm_stage(Xs, k.X, mt, m1, kt * kGlmKD, D, D, lane);
        // one slice holds every column: the sample tile is staged once
        if (nK > 1 || it == 0) glm_stage(Bs, k.x, row0, k.n, kt * kGlmKD, D, Dx, lane);
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
      if constexpr (OFFS) ev = ok ? k.eta0[mt + lr] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double l, dl;
        if constexpr (LRN) {
          const double* rk = smem + 4 * kGlmWave + 2 * (lq + 4 * r);
          double dlam;
          glm_link_aux<LIK>(k, rk[0], rk[1], OFFS ? eta[r] + ev : eta[r], yv, l, dl, dlam);
          if constexpr (LACC) laa[r] += ok ? dlam : 0.0;
        } else if constexpr (OFFS) {
          obs_link<LIK>(k.lk, eta[r] + ev, yv, l, dl);
        } else {
          obs_link<LIK>(k.lk, eta[r], yv, l, dl);
        }
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
          if (valid) glm_stage(Xs, k.X, mt, m1, col0 + cs * 32, D, D, lane);
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
    if constexpr (LACC) {
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) laa[r] += __shfl_xor(laa[r], off, 64);
    }
  }
  __syncthreads();
  if (lr == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w * 16 + lq + 4 * r] = lpa[r];
    if constexpr (LACC) {
#pragma unroll
      for (int r = 0; r < 4; ++r) red[64 + w * 16 + lq + 4 * r] = laa[r];
    }
  }
  __syncthreads();
  if (blockIdx.z == 0 && t < 16 && row0 + t < k.n) {
    const long long row = row0 + t;
    const double s = ((red[t] + red[16 + t]) + red[32 + t]) + red[48 + t];
    double sl = 0.0;
    if constexpr (LACC) sl = ((red[64 + t] + red[80 + t]) + red[96 + t]) + red[112 + t];
    if (fin) {
      double ss = 0.0;
      for (int d = 0; d < D; ++d) {
        const double b = k.x[row * Dx + d];
        ss = fma(b, b, ss);
      }
      if constexpr (LRN) {
        double lpv, gl;
        glm_aux_final<LIK>(k, row, k.x[row * Dx + D], s, sl, ss, lpv, gl);
        k.logp[row] = lpv;
        if constexpr (GRAD) k.grad[row * Dx + D] = gl;
      } else {
        k.logp[row] = glm_final_logp(k, s, ss);
      }
    } else {
      k.plp[(long long)blockIdx.y * k.n + row] = s;
      if constexpr (LACC) k.pla[(long long)blockIdx.y * k.n + row] = sl;
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
          k.grad[row * Dx + col] = s - k.x[row * Dx + col] * k.inv_s2;
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

// the same for the learned instances: job i < n also writes d log p / d lambda of row i;
// job n + j is gradient entry j of the [n][p] coefficient columns
template <int LIK>
__global__ __launch_bounds__(256) void glm_combine_aux_kernel(GlmK k, int with_grad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nd = k.n * k.D;
  if (i < k.n) {
    double s = 0.0, sl = 0.0;
    for (int c = 0; c < k.nchunk; ++c) s += k.plp[(long long)c * k.n + i];
    if constexpr (LIK != 5) {
      if (with_grad)
        for (int c = 0; c < k.nchunk; ++c) sl += k.pla[(long long)c * k.n + i];
    }
    double ss = 0.0;
    for (int d = 0; d < k.D; ++d) {
      const double b = k.x[i * k.Dx + d];
      ss = fma(b, b, ss);
    }
    double lpv, gl;
    glm_aux_final<LIK>(k, i, k.x[i * k.Dx + k.D], s, sl, ss, lpv, gl);
    k.logp[i] = lpv;
    if (with_grad) k.grad[i * k.Dx + k.D] = gl;
  } else if (with_grad && i - k.n < nd) {
    const long long j = i - k.n, row = j / k.D, col = j % k.D;
    double s = 0.0;
    for (int c = 0; c < k.nchunk; ++c) s += k.pg[(long long)c * nd + j];
    k.grad[row * k.Dx + col] = s - k.x[row * k.Dx + col] * k.inv_s2;
  }
}

// learned dispersion: the table sums of the n rows (disp_row_sums of vb_links.hpp), one
// sample row per block
__global__ __launch_bounds__(256) void glm_disp_kernel(GlmK k) {
  disp_row_sums(k.x, k.Dx, k.D, k.T, k.J, k.tab, k.n);
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
// stay under kGlmScratchMax doubles.  A learned block plans with D = p and one more
// partial per row (pla) beside the gradient's.
GlmPlan glm_plan(int D, long long n, long long M, bool grad, int extra = 0) {
  GlmPlan p{};
  p.small = D <= kBlockDMax;
  p.tb = p.small ? (n <= 4096 ? 64 : 256) : 256;
  const long long rpb = p.small ? p.tb : 16;
  p.row_blocks = (n + rpb - 1) / rpb;
  const long long target = 4LL * glm_cu_count();
  const long long max_chunks = std::min<long long>((M + kGlmTile - 1) / kGlmTile, 1024);
  long long nc = std::max<long long>(1, std::min(max_chunks, (target + p.row_blocks - 1) / p.row_blocks));
  const long long per = std::max<long long>(1, n) * (1 + (grad ? D + extra : 0));
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

}  // namespace

size_t glm_scratch_doubles(int D, long long n, const GlmHead& h, bool grad) {
  if (n < 1) return 0;
  if (h.learn) {   // [tab 2 n (likelihood 4)] [plp] [pla (grad)] [pg (grad)]
    const int pc = D - 1;
    const GlmPlan p = glm_plan(pc, n, h.M, grad, 1);
    const size_t tab = h.lik == 4 ? 2 * (size_t)n : 0;
    return tab + (p.nchunk > 1 ? (size_t)p.nchunk * (size_t)n * (size_t)(1 + (grad ? 1 + pc : 0)) : 0);
  }
  const GlmPlan p = glm_plan(D, n, h.M, grad);
  return p.nchunk > 1 ? (size_t)p.nchunk * (size_t)n * (size_t)(1 + (grad ? D : 0)) : 0;
}

// the learned block: the instances 5, 6, 7 over p = D - 1 columns
static hipError_t launch_glm_rows_aux(int D, long long n, const GlmHead& h, const double* params,
                                      const double* x, double* logp, double* grad,
                                      double* scratch, hipStream_t s) {
  const int pc = D - 1;
  if (pc < 1) return hipErrorInvalidValue;
  const GlmPlan p = glm_plan(pc, n, h.M, grad != nullptr, 1);
  if (p.row_blocks > 0x7fffffffLL || p.nslab > 65535 || n > 0x7fffffffLL) return hipErrorInvalidValue;
  if ((p.nchunk > 1 || h.lik == 4) && !scratch) return hipErrorInvalidValue;
  GlmK k{};
  k.D = pc;
  k.Dx = D;
  k.nchunk = p.nchunk;
  k.n = n;
  k.M = h.M;
  k.Mf = (double)h.M;
  k.chunk_obs = p.chunk_obs;
  const AuxConsts a = aux_consts(h.lik, h.nu, h.s_aux);   // vb_links.hpp
  k.lk.k1 = a.k1;
  k.lk.k2 = a.k2;
  k.nu = a.nu;
  k.inv_nu = a.inv_nu;
  k.inv_s2 = 1.0 / (h.prior * h.prior);
  k.ls_aux = a.ls_aux;
  k.c_all = -(double)pc * (0.5 * kLog2Pi + std::log(h.prior)) + (double)h.M * a.c_obs + a.c_aux;
  if (h.lik == 4) k.c_all += h.c_data;
  k.X = params + kGlmHeader;
  k.y = k.X + (size_t)h.M * pc;
  k.eta0 = h.lik == 4 ? k.y + h.M : nullptr;
  k.J = h.lik == 4 ? h.J : 0;
  k.T = h.lik == 4 ? k.eta0 + h.M + 2 : nullptr;   // behind c_data and J
  k.x = x;
  k.logp = logp;
  k.grad = grad;
  double* sc = scratch;
  if (h.lik == 4) {
    k.tab = sc;
    sc += 2 * (size_t)n;
  }
  if (p.nchunk > 1) {
    k.plp = sc;
    sc += (size_t)p.nchunk * n;
    if (grad) {
      k.pla = sc;
      k.pg = sc + (size_t)p.nchunk * n;
    }
  }
  if (h.lik == 4) {
    hipLaunchKernelGGL(glm_disp_kernel, dim3((unsigned)n), dim3(256), 0, s, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (h.lik == 0)
    glm_launch<5>(p, k, s);
  else if (h.lik == 1)
    glm_launch<6>(p, k, s);
  else
    glm_launch<7>(p, k, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.nchunk == 1) return e;
  const long long jobs = n + (grad ? n * pc : 0);
  const dim3 g((unsigned)((jobs + 255) / 256)), b(256);
  if (h.lik == 0)
    hipLaunchKernelGGL(glm_combine_aux_kernel<5>, g, b, 0, s, k, grad ? 1 : 0);
  else if (h.lik == 1)
    hipLaunchKernelGGL(glm_combine_aux_kernel<6>, g, b, 0, s, k, grad ? 1 : 0);
  else
    hipLaunchKernelGGL(glm_combine_aux_kernel<7>, g, b, 0, s, k, grad ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_glm_rows(int D, long long n, const GlmHead& h, const double* params,
                           const double* x, double* logp, double* grad, double* scratch,
                           hipStream_t s) {
  if (n < 1) return hipSuccess;
  if (h.learn) return launch_glm_rows_aux(D, n, h, params, x, logp, grad, scratch, s);
  const GlmPlan p = glm_plan(D, n, h.M, grad != nullptr);
  if (p.row_blocks > 0x7fffffffLL || p.nslab > 65535) return hipErrorInvalidValue;
  if (p.nchunk > 1 && !scratch) return hipErrorInvalidValue;
  GlmK k{};
  k.D = D;
  k.nchunk = p.nchunk;
  k.n = n;
  k.M = h.M;
  k.chunk_obs = p.chunk_obs;
  const double c_obs = link_consts(h.lik, h.nu, h.sigma, h.phi, &k.lk);
  k.inv_s2 = 1.0 / (h.prior * h.prior);
  k.c_all = -(double)D * (0.5 * kLog2Pi + std::log(h.prior)) + (double)h.M * c_obs;
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
