// vb_lrg.hip — low-rank-plus-diagonal Gaussian family
// (low_rank_gaussian_variational_family) and its KLVI / KLVI_PD / CHIVI value +
// gradient.
//
// lambda = [mu (D), log_d (D), B row-major (D x R)], d = exp(log_d), 1 <= R <= 64,
// Sigma = B B^T + diag(d^2).  With W = diag(1/d) B and the capacitance matrix
// C = I_R + W^T W (R x R, C >= I):
//   x = mu + d z + B u,               eps row = [z (D), u (R)]
//   entropy = D/2 (1 + log 2 pi) + sum log_d + 1/2 log det C
//   y = (x - mu) / d (= z + W u on the family's own draws),
//   t = C^-1 W^T y,  rho = y - W t,   Sigma^-1 (x - mu) = rho / d,
//   log q(x) = -D/2 log 2 pi - sum log_d - 1/2 log det C - 1/2 (|rho|^2 + |t|^2)
// (the sum of squares, not |y|^2 - v^T C^-1 v, which cancels when B dominates d).
// No D x D matrix is formed anywhere.
//
// One step, besides the target's launches:
//   1 lrg_cap_part_kernel  partial W^T W and sum log_d of a block of rows
//   2 lrg_cap_kernel       C (fixed-order combine), its Cholesky factor in LDS,
//                          C^-1, 1/2 log det C, sum log_d         (one block)
//   3 lrg_h_kernel         entropy gradient: H_B = diag(1/d) W C^-1, H_d = 1 - diag(W C^-1 W^T)
//   4 lrg_noise_kernel     eps rows from Philox at width D + R (host draws are read in place)
//   5 lrg_x_kernel         X = mu + d z + U B^T on v_mfma_f64_16x16x4_f64 (depth R,
//                          zero-padded in registers)
//     target               log p, G = d log p / dx (target_eval)
//   6 lrg_quad_kernel      per sample: t_n, a_n = rho_n / d, q_n = |rho_n|^2 + |t_n|^2
//                          (KLVI_PD, CHIVI and log weights; KLVI needs no log q)
//   7 lrg_grad_kernel      (KLVI: the entropy form; KLVI_PD and CHIVI: sum_n r_n grad lw_n,
//                          which keeps the per-sample zero-mean terms of log q)
//                          weights r_n in every block's prologue (fixed order, the
//                          same bits in every block), one depth-N chain per entry
//                          of the gradient, the entropy term, and in fused runs the
//                          windowed adagrad step and the history row.
// Launches 1-3 read lambda before launch 7 updates it in place; launch 7's blocks
// read of lambda only the log_d entries they update themselves.
// fp64 throughout, no atomics, every sum in a fixed order; a row's bits do not
// depend on the rows beside it.  No host synchronisation inside a step.
#include "vb_device.hpp"
#include "vb_internal.hpp"

#include <algorithm>
#include <cmath>

namespace vbk {
using namespace vbd;

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(2 pi) / 2
constexpr int kChunk = 512;                             // samples per staged block of weights
constexpr int kRMax = kLrgRankMax;
constexpr int kLd = kRMax + 1;                          // LDS row stride of an R x R matrix
constexpr int kCapBlocksMax = 1024;                     // partial blocks of W^T W at most

#define LRG_HIP(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return vb_set_error(e_ == hipErrorOutOfMemory ? -3 : -2, "%s failed: %s (%s:%d)", #expr, \
                          hipGetErrorString(e_), __FILE__, __LINE__);                      \
  } while (0)

// Fixed-order sum / max over the 256 threads of a block (4 waves); every thread
// receives the result.
__device__ __forceinline__ double block_reduce(double v, bool mx, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = mx ? fmax(v, o) : v + o;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < 4; ++w) r = mx ? fmax(r, red[w]) : r + red[w];
  return r;
}

// Launch 1.  Block b takes the rows [b rows, (b + 1) rows) of W = diag(1/d) B:
// part[b][a R + c] = sum_i w_ia w_ic over them (i ascending), part[b][R R] = their
// sum of log_d.  Thread t owns the entries t, t + 256, ... (16 at R = 64).
__global__ __launch_bounds__(256) void lrg_cap_part_kernel(int D, int R, int rows, const double* lam,
                                                           double* part) {
  __shared__ double ws[16][kRMax];
  __shared__ double red[4];
  const int t = threadIdx.x, rr = R * R;
  const int i0 = blockIdx.x * rows, i1 = min(D, i0 + rows);
  int ea[16], ec[16];
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int e = t + 256 * k;
    ea[k] = e < rr ? e / R : 0;
    ec[k] = e < rr ? e % R : 0;
    acc[k] = 0.0;
  }
  for (int s0 = i0; s0 < i1; s0 += 16) {
    const int sn = min(16, i1 - s0);
    __syncthreads();
    for (int e = t; e < sn * R; e += 256) {
      const int i = s0 + e / R, a = e % R;
      ws[e / R][a] = lam[2LL * D + (long long)i * R + a] / exp(lam[D + i]);
    }
    __syncthreads();
    for (int s = 0; s < sn; ++s) {
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = fma(ws[s][ea[k]], ws[s][ec[k]], acc[k]);
    }
  }
  double* out = part + (long long)blockIdx.x * (rr + 1);
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (t + 256 * k < rr) out[t + 256 * k] = acc[k];
  double sl = 0.0;
  for (int i = i0 + t; i < i1; i += 256) sl += lam[D + i];
  sl = block_reduce(sl, false, red);
  if (t == 0) out[rr] = sl;
}

// Launch 2 (one block).  C = I + sum_b part[b] in block order, Cholesky C = L L^T in
// LDS (lower triangle, in place), L^-1 by columns into the unused upper triangle
// (its diagonal in dinv), cinv = L^-T L^-1, scal[0] = sum log_d, scal[1] = 1/2 log det C
// = sum log L_kk.
__global__ __launch_bounds__(256) void lrg_cap_kernel(int R, int nblk, const double* part,
                                                      double* cinv, double* scal) {
  __shared__ double M[kRMax * kLd];
  __shared__ double dinv[kRMax];
  const int t = threadIdx.x, rr = R * R;
  for (int e = t; e < rr; e += 256) {
    const int a = e / R, c = e % R;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(long long)b * (rr + 1) + e];
    M[a * kLd + c] = (a == c ? 1.0 : 0.0) + s;
  }
  if (t == 0) {
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(long long)b * (rr + 1) + rr];
    scal[0] = s;
  }
  __syncthreads();
  for (int k = 0; k < R; ++k) {
    if (t == 0) M[k * kLd + k] = sqrt(M[k * kLd + k]);
    __syncthreads();
    const double dk = M[k * kLd + k];
    for (int i = k + 1 + t; i < R; i += 256) M[i * kLd + k] /= dk;
    __syncthreads();
    const int m = R - k - 1;
    for (int e = t; e < m * m; e += 256) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) M[i * kLd + j] = fma(-M[i * kLd + k], M[j * kLd + k], M[i * kLd + j]);
    }
    __syncthreads();
  }
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < R; ++k) s += log(M[k * kLd + k]);
    scal[1] = s;
  }
  // column j of L^-1: Linv[i][j], i > j, is kept at M[j][i]
  if (t < R) {
    const int j = t;
    const double dj = 1.0 / M[j * kLd + j];
    dinv[j] = dj;
    for (int i = j + 1; i < R; ++i) {
      double s = M[i * kLd + j] * dj;
      for (int k = j + 1; k < i; ++k) s = fma(M[i * kLd + k], M[j * kLd + k], s);
      M[j * kLd + i] = -s / M[i * kLd + i];
    }
  }
  __syncthreads();
  for (int e = t; e < rr; e += 256) {
    const int a = e / R, c = e % R;
    double s = 0.0;
    for (int k = max(a, c); k < R; ++k) {
      const double la = k == a ? dinv[a] : M[a * kLd + k];
      const double lc = k == c ? dinv[c] : M[c * kLd + k];
      s = fma(la, lc, s);
    }
    cinv[e] = s;
  }
}

// Launch 3.  One wave per row i, 16 rows per wave: lane a holds w_ia, v_a = sum_b w_ib
// C^-1[b][a] (b ascending), H_B[i][a] = v_a / d_i, H_d[i] = 1 - sum_a w_ia v_a.
__global__ __launch_bounds__(256) void lrg_h_kernel(int D, int R, const double* lam,
                                                    const double* cinv, double* hb, double* hd) {
  __shared__ double Ci[kRMax * kLd];
  const int t = threadIdx.x, lane = t & 63;
  for (int e = t; e < R * R; e += 256) Ci[(e / R) * kLd + e % R] = cinv[e];
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * 64 + (t >> 6) * 16;
  for (int s = 0; s < 16; ++s) {
    const long long i = r0 + s;
    if (i >= D) break;   // uniform over the wave; no block barrier below
    const double inv_d = 1.0 / exp(lam[D + i]);
    const double w = lane < R ? lam[2LL * D + i * R + lane] * inv_d : 0.0;
    double v = 0.0;
    for (int b = 0; b < R; ++b) v = fma(__shfl(w, b, 64), lane < R ? Ci[b * kLd + lane] : 0.0, v);
    if (lane < R) hb[i * R + lane] = v * inv_d;
    const double q = wave_sum(w * v);
    if (lane == 0) hd[i] = 1.0 - q;
  }
}

// Launch 4.  One wave per eps row of width Wd = D + R, from Philox (column pair j,
// sample, step, purpose 0: the Gaussian z row of a family of dimension D + R).
__global__ __launch_bounds__(256) void lrg_noise_kernel(int Wd, long long n, Rng rng, uint32_t step,
                                                        double* eps) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const int np = (Wd + 1) / 2;
  for (int j = lane; j < np; j += 64) {
    double z0, z1;
    normal_pair(rng.draw((uint32_t)j, (uint32_t)row, step, 0u), z0, z1);
    eps[row * Wd + 2 * j] = z0;
    if (2 * j + 1 < Wd) eps[row * Wd + 2 * j + 1] = z1;
  }
}

// Launch 5.  X = mu + d z + U B^T, one wave per 16 x 16 tile (16 samples x 16
// coordinates): A = U (row lane & 15, k = lane >> 4), B operand [k][col] = B[col][k].
// Ranks that are no multiple of 4 are padded with zeros in registers.
__global__ __launch_bounds__(256) void lrg_x_kernel(int D, int R, long long n, const double* lam,
                                                    const double* eps, double* x) {
  const int tiles_c = (D + 15) / 16;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long rt = tile / tiles_c;
  const int ct = (int)(tile % tiles_c);
  if (rt * 16 >= n) return;
  const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const long long row = rt * 16 + r, ld = (long long)D + R;
  const int col = ct * 16 + r;
  const bool row_ok = row < n, col_ok = col < D;
  const double* urow = eps + (row_ok ? row : 0) * ld + D;
  const double* brow = lam + 2LL * D + (col_ok ? (long long)col * R : 0);
  d4 acc[4] = {};
  for (int k0 = 0; k0 < R; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * s + kq;
      double a = 0.0, b = 0.0;
      if (row_ok && k < R) a = urow[k];
      if (col_ok && k < R) b = brow[k];
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
    }
  }
  const d4 r4 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (!col_ok) return;
  const double m = lam[col], d = exp(lam[D + col]);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const long long orow = rt * 16 + kq + 4 * rr;
    if (orow < n) x[orow * D + col] = fma(d, eps[orow * ld + col], m) + r4[rr];
  }
}

// Launch 6.  One block per sample / point n.  pts == null: y = z + W u from the eps row;
// otherwise y = (pts[n] - mu) / d.  v = W^T y (per-thread partial sums over i = t, t +
// 256, ..., then lanes, then waves: a fixed order), t = C^-1 v, rho = y - W t.  Writes
// tt [n][R] = t, aa [n][D] = rho / d (first y, by the same thread), qq[n] = |rho|^2 + |t|^2
// and, with out non-null, out[n] = log q.  RP: R rounded up to 4 .. 64, the unrolled
// register width.
template <int RP>
__global__ __launch_bounds__(256) void lrg_quad_kernel(int D, int R, const double* lam,
                                                       const double* eps, const double* pts,
                                                       const double* cinv, const double* scal,
                                                       double* tt, double* aa, double* qq,
                                                       double* out) {
  __shared__ double us[kRMax], vv[kRMax], ts[kRMax];
  __shared__ double part[4][kRMax];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long n = blockIdx.x, ld = (long long)D + R;
  const double* B = lam + 2LL * D;
  double* arow = aa + n * D;
  if (!pts && t < R) us[t] = eps[n * ld + D + t];
  __syncthreads();
  double acc[RP];
#pragma unroll
  for (int a = 0; a < RP; ++a) acc[a] = 0.0;
  for (int i = t; i < D; i += 256) {
    const double inv_d = 1.0 / exp(lam[D + i]);
    const double* bi = B + (long long)i * R;
    double w[RP];
#pragma unroll
    for (int a = 0; a < RP; ++a) w[a] = a < R ? bi[a] * inv_d : 0.0;
    double y;
    if (pts) {
      y = (pts[n * D + i] - lam[i]) * inv_d;
    } else {
      y = eps[n * ld + i];
#pragma unroll
      for (int a = 0; a < RP; ++a)
        if (a < R) y = fma(w[a], us[a], y);
    }
    arow[i] = y;
#pragma unroll
    for (int a = 0; a < RP; ++a) acc[a] = fma(w[a], y, acc[a]);
  }
#pragma unroll
  for (int a = 0; a < RP; ++a) {
    const double s = wave_sum(acc[a]);
    if (lane == 0) part[wv][a] = s;
  }
  __syncthreads();
  if (t < R) vv[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
  __syncthreads();
  if (t < R) {
    double s = 0.0;
    for (int b = 0; b < R; ++b) s = fma(cinv[t * R + b], vv[b], s);
    ts[t] = s;
    tt[n * R + t] = s;
  }
  __syncthreads();
  double ss = 0.0;
  for (int i = t; i < D; i += 256) {
    const double inv_d = 1.0 / exp(lam[D + i]);
    const double* bi = B + (long long)i * R;
    double rho = arow[i];
#pragma unroll
    for (int a = 0; a < RP; ++a)
      if (a < R) rho = fma(-(bi[a] * inv_d), ts[a], rho);
    arow[i] = rho * inv_d;
    ss = fma(rho, rho, ss);
  }
  ss = block_reduce(ss, false, red);
  if (t == 0) {
    double s2 = 0.0;
    for (int a = 0; a < R; ++a) s2 = fma(ts[a], ts[a], s2);
    const double q = ss + s2;
    qq[n] = q;
    if (out) out[n] = (-(double)D * kHalfLog2Pi - scal[0] - scal[1]) - 0.5 * q;
  }
}

// Launch 7 (see the file comment).  mode: 0 KLVI, 1 CHIVI, 2 KLVI_PD.
struct LrgGradArgs {
  int D, R, N, mode, upd;
  double alpha;
  const double *G, *eps, *logp, *qq, *scal, *aa, *tt, *hb, *hd;
  double* value;
  double* grad;   // [P], when !upd
  double* lam;    // read (own log_d entries); updated in place when upd
  double* ring;
  int W;
  long long step;
  double lr, eps_ada;
  double* hrow;
};

// Entry e = i (R + 2) + c of the gradient: c = 0 mu_i, c = 1 log_d_i, c >= 2 B[i][c - 2];
// one thread per entry, one chain over the samples in order.
__global__ __launch_bounds__(256) void lrg_grad_kernel(LrgGradArgs a) {
  __shared__ double red[4];
  __shared__ double rs[kChunk];
  const int D = a.D, R = a.R, N = a.N, t = threadIdx.x;
  const double inv_n = 1.0 / N;
  // ---- weights: the same arithmetic in the same order in every block
  const double sum_ld = a.scal[0], hld = a.scal[1];
  const double lq0 = ((double)D * kHalfLog2Pi + sum_ld) + hld;   // -log q(x_n) = lq0 + q_n / 2
  double mx = 0.0, rsum = -1.0;
  if (a.mode == 1) {
    double m = -INFINITY;
    for (int k = t; k < N; k += 256) m = fmax(m, a.logp[k] + lq0 + 0.5 * a.qq[k]);
    mx = block_reduce(m, true, red);
    double sw = 0.0;
    for (int k = t; k < N; k += 256) sw += exp(a.alpha * ((a.logp[k] + lq0 + 0.5 * a.qq[k]) - mx));
    sw = block_reduce(sw, false, red);
    rsum = a.alpha * sw * inv_n;
    if (blockIdx.x == 0 && t == 0) *a.value = log(sw * inv_n) / a.alpha + mx;
  } else if (blockIdx.x == 0) {
    double s = 0.0;
    if (a.mode == 2)
      for (int k = t; k < N; k += 256) s += a.logp[k] + lq0 + 0.5 * a.qq[k];
    else
      for (int k = t; k < N; k += 256) s += a.logp[k];
    s = block_reduce(s, false, red);
    if (t == 0)
      *a.value = a.mode == 2 ? -(s * inv_n)
                             : -((((double)D * (0.5 + kHalfLog2Pi) + sum_ld) + hld) + s * inv_n);
  }
  const long long C = R + 2, P = (long long)D * C, ld = (long long)D + R;
  const long long e = (long long)blockIdx.x * 256 + t;
  const bool live = e < P;
  const long long i = live ? e / C : 0;
  const int c = live ? (int)(e % C) : 0;
  const bool chivi = a.mode == 1;
  // KLVI_PD and CHIVI differentiate log q(x(lambda); lambda) sample by sample: the
  // zero-mean terms stay (only KLVI's entropy form drops them)
  const bool full = a.mode != 0;
  const long long p = c == 0 ? i : c == 1 ? D + i : 2LL * D + i * R + (c - 2);
  const double d = (live && c == 1) ? exp(a.lam[p]) : 0.0;
  // the factor of g (and a) of this entry in row n: 1, d z_ni or u_n,c-2
  const long long fcol = c == 1 ? i : D + (c - 2);
  double acc = 0.0;
  for (int c0 = 0; c0 < N; c0 += kChunk) {
    const int cn = min(kChunk, N - c0);
    __syncthreads();
    for (int k = t; k < cn; k += 256) {
      double w = -inv_n;
      if (chivi)
        w = a.alpha * exp(a.alpha * ((a.logp[c0 + k] + lq0 + 0.5 * a.qq[c0 + k]) - mx)) * inv_n;
      rs[k] = w;
    }
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < cn; ++k) {
      const long long n = c0 + k;
      const double g = a.G[n * D + i];
      if (c == 0) {
        acc = fma(rs[k], g, acc);
        continue;
      }
      double f = a.eps[n * ld + fcol];
      if (c == 1) f *= d;
      if (!full) {
        acc = fma(rs[k] * g, f, acc);
      } else {
        const double an = a.aa[n * D + i];
        const double back = c == 1 ? (an * d) * (an * d) : an * a.tt[n * R + (c - 2)];
        acc = fma(rs[k], fma(g + an, f, -back), acc);
      }
    }
  }
  if (!live) return;
  double g = acc;
  if (c == 1) g = fma(rsum, a.hd[i], acc);
  if (c >= 2) g = fma(rsum, a.hb[i * R + (c - 2)], acc);
  if (a.upd) {
    const double v = adagrad_step(p, P, a.lam[p], g, a.ring, a.W, a.step, a.lr, a.eps_ada, nullptr);
    a.lam[p] = v;
    if (a.hrow) a.hrow[p] = v;
  } else {
    a.grad[p] = g;
  }
}

// lw_n = log p(x_n) - log q(x_n) on the family's own draws
__global__ __launch_bounds__(256) void lrg_lw_kernel(int D, long long m, const double* logp,
                                                     const double* qq, const double* scal,
                                                     double* lw) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  lw[k] = logp[k] + (((double)D * kHalfLog2Pi + scal[0]) + scal[1]) + 0.5 * qq[k];
}

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

int grid_ok(long long blocks) {
  if (blocks > 2147483647LL) return vb_set_error(-4, "low-rank Gaussian: too many rows for one launch");
  return 0;
}

// The family's workspace for n rows: the row buffers of the shared workspace (eps rows
// of width D + R in Z) and its own block.
struct LrgBufs {
  FrRows b;
  double *part, *cinv, *hb, *hd, *tt, *aa, *qq;
  int cap_rows, cap_blocks;
};

int lrg_bufs(FrWork* W, int D, int R, long long n, LrgBufs* o) {
  if (int rc = fr_rows(W, D + R, n, &o->b)) return rc;
  o->cap_rows = (int)std::max<long long>(64, cdiv(D, kCapBlocksMax));
  o->cap_blocks = (int)cdiv(D, o->cap_rows);
  const size_t rr = (size_t)R * R, np = (size_t)o->cap_blocks * (rr + 1);
  const size_t dr = (size_t)D * R, nr = (size_t)n * R, nd = (size_t)n * D;
  double* p;
  if (int rc = fr_extra(W, np + rr + dr + D + nr + nd + (size_t)n, &p)) return rc;
  o->part = p;
  o->cinv = o->part + np;
  o->hb = o->cinv + rr;
  o->hd = o->hb + dr;
  o->tt = o->hd + D;
  o->aa = o->tt + nr;
  o->qq = o->aa + nd;
  return 0;
}

// launches 1-2 (and 3 with the entropy gradient)
int capacitance(const LrgBufs& w, int D, int R, const double* lam, bool grad, hipStream_t st) {
  hipLaunchKernelGGL(lrg_cap_part_kernel, dim3((unsigned)w.cap_blocks), dim3(256), 0, st, D, R,
                     w.cap_rows, lam, w.part);
  hipLaunchKernelGGL(lrg_cap_kernel, dim3(1), dim3(256), 0, st, R, w.cap_blocks, w.part, w.cinv,
                     w.b.scal);
  if (grad)
    hipLaunchKernelGGL(lrg_h_kernel, dim3((unsigned)cdiv(D, 64)), dim3(256), 0, st, D, R, lam, w.cinv,
                       w.hb, w.hd);
  LRG_HIP(hipGetLastError());
  return 0;
}

// launches 4-5: eps (the workspace's or the caller's) and x
int draw_transform(const LrgBufs& w, int D, int R, long long n, const double* lam, const Noise& nz,
                   double* x, const double** eps_out, hipStream_t st) {
  const double* eps = nz.eps ? nz.eps : w.b.Z;
  if (!nz.eps) {
    if (int rc = grid_ok(cdiv(n, 4))) return rc;
    hipLaunchKernelGGL(lrg_noise_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, D + R, n,
                       Rng{nz.k0, nz.k1, nz.stream}, (uint32_t)nz.step, w.b.Z);
  }
  const long long tiles = cdiv(n, 16) * cdiv(D, 16);
  if (int rc = grid_ok(cdiv(tiles, 4))) return rc;
  hipLaunchKernelGGL(lrg_x_kernel, dim3((unsigned)cdiv(tiles, 4)), dim3(256), 0, st, D, R, n, lam, eps, x);
  LRG_HIP(hipGetLastError());
  *eps_out = eps;
  return 0;
}

// launch 6 at the register width of R
int quad(const LrgBufs& w, int D, int R, long long n, const double* lam, const double* eps,
         const double* pts, double* out, hipStream_t st) {
  if (int rc = grid_ok(n)) return rc;
  const dim3 g((unsigned)n), b(256);
#define LRG_QUAD(RP)                                                                          \
  hipLaunchKernelGGL(lrg_quad_kernel<RP>, g, b, 0, st, D, R, lam, eps, pts, w.cinv, w.b.scal, \
                     w.tt, w.aa, w.qq, out)
  if (R <= 4) LRG_QUAD(4);
  else if (R <= 8) LRG_QUAD(8);
  else if (R <= 16) LRG_QUAD(16);
  else if (R <= 32) LRG_QUAD(32);
  else LRG_QUAD(64);
#undef LRG_QUAD
  LRG_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// x [n][D] = mu + d z + u B^T; nz.eps (host draws, on the device) = [n][D + R]
int lrg_sample(FrWork* W, const Family& f, const double* lam, long long n, const Noise& nz,
               double* x, hipStream_t st) {
  LrgBufs w;
  if (int rc = lrg_bufs(W, f.D, f.R, n, &w)) return rc;
  const double* eps;
  return draw_transform(w, f.D, f.R, n, lam, nz, x, &eps, st);
}

// One KLVI / KLVI_PD / CHIVI value + gradient at lam (device pointers).  up non-null:
// the windowed adagrad step rides in the gradient kernel's epilogue (lam updated in
// place, ring / history row written; grad is not written).
int lrg_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz, double* value,
                   double* grad, hipStream_t st, const MfUpdate* up) {
  const int D = f.fam.D, R = f.fam.R, N = f.N;
  LrgBufs w;
  if (int rc = lrg_bufs(W, D, R, N, &w)) return rc;
  if (int rc = capacitance(w, D, R, lam, true, st)) return rc;
  const double* eps;
  if (int rc = draw_transform(w, D, R, N, lam, nz, w.b.X, &eps, st)) return rc;
  if (int rc = target_eval(W, f.tgt, N, w.b.X, w.b.logp, w.b.G, st)) return rc;
  const int mode = f.chivi ? 1 : f.pd ? 2 : 0;
  if (mode != 0)
    if (int rc = quad(w, D, R, N, lam, eps, nullptr, nullptr, st)) return rc;
  LrgGradArgs a{};
  a.D = D;
  a.R = R;
  a.N = N;
  a.mode = mode;
  a.upd = up != nullptr;
  a.alpha = f.alpha;
  a.G = w.b.G;
  a.eps = eps;
  a.logp = w.b.logp;
  a.qq = w.qq;
  a.scal = w.b.scal;
  a.aa = w.aa;
  a.tt = w.tt;
  a.hb = w.hb;
  a.hd = w.hd;
  a.value = value;
  a.grad = grad;
  a.lam = const_cast<double*>(lam);
  if (up) {
    a.ring = up->ring;
    a.W = up->W;
    a.step = up->step;
    a.lr = up->lr;
    a.eps_ada = up->eps;
    a.hrow = up->hrow;
  }
  const long long P = (long long)D * (R + 2);
  if (int rc = grid_ok(cdiv(P, 256))) return rc;
  hipLaunchKernelGGL(lrg_grad_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, st, a);
  LRG_HIP(hipGetLastError());
  return 0;
}

// log q(x) for arbitrary x [n][D] at lam
int lrg_logdensity(FrWork* W, const Family& f, const double* lam, const double* x, long long n,
                   double* out, hipStream_t st) {
  LrgBufs w;
  if (int rc = lrg_bufs(W, f.D, f.R, n, &w)) return rc;
  if (int rc = capacitance(w, f.D, f.R, lam, false, st)) return rc;
  return quad(w, f.D, f.R, n, lam, nullptr, x, out, st);
}

// log weights lw = log p(x) - log q(x), x ~ q; xs (nullable) receives the samples
int lrg_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                    double* lw, double* xs, hipStream_t st) {
  const int D = f.fam.D, R = f.fam.R;
  LrgBufs w;
  if (int rc = lrg_bufs(W, D, R, m, &w)) return rc;
  if (int rc = capacitance(w, D, R, lam, false, st)) return rc;
  double* x = xs ? xs : w.b.X;
  const double* eps;
  if (int rc = draw_transform(w, D, R, m, lam, nz, x, &eps, st)) return rc;
  if (int rc = target_eval(W, f.tgt, m, x, w.b.logp, nullptr, st)) return rc;
  if (int rc = quad(w, D, R, m, lam, eps, nullptr, nullptr, st)) return rc;
  hipLaunchKernelGGL(lrg_lw_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, D, m, w.b.logp,
                     w.qq, w.b.scal, lw);
  LRG_HIP(hipGetLastError());
  return 0;
}

}  // namespace vbk
