// vb_frg.hip — full-rank Gaussian family on its Cholesky factor
// (cholesky_gaussian_variational_family; what viabel/vb.py:85-137 was meant to be)
// and its KLVI / KLVI_PD / CHIVI value + gradient (vb.py:236-295).
//
// lambda = [mu (D), tril(M) row-major (D(D+1)/2)], L = M with exp'd diagonal,
// Sigma = L L^T: VB_FAMILY_FR_T's layout.  With the Cholesky factor as the
// transform nothing of the t path's sqrtm machinery is needed:
//   x = mu + L z,   entropy = D/2 (1 + log 2 pi) + sum M_ii,
//   log q(x_n) = -D/2 log 2 pi - sum M_ii - 1/2 |z_n|^2   on the family's own draws.
//
// One step, three launches of the family's own besides the target's:
//   1 frg_noise_kernel  Z (Philox; host draws are read in place), zz_n = |z_n|^2,
//                       sum M_ii
//   2 frg_x_kernel      X = mu + Z L^T on v_mfma_f64_16x16x4_f64, L read from the
//                       packed parameters; k tiles above the diagonal tile are skipped
//     target            log p, G = d log p / dx (target_eval)
//   3 frg_grad_kernel   weights r_n in every block's prologue (fixed order, the
//                       same bits in every block), then the lower-triangle tiles of
//                       G_L = G^T diag(r) Z (depth N) and the mean gradient
//                       sum_n r_n g_n as one more tile column; the epilogue packs
//                         grad[i][j] = G_L[i][j] (i > j),
//                         grad[i][i] = G_L[i][i] L_ii + sum_n r_n
//                       and, in fused runs, applies the windowed adagrad step and
//                       writes the history row.  G_L never reaches memory.
//   KLVI / KLVI_PD: r_n = -1/N.  CHIVI: r_n = alpha w_n / N, w_n = exp(alpha (lw_n -
//   max lw)), lw_n = log p(x_n) + D/2 log 2 pi + sum M_ii + zz_n / 2.
// fp64 throughout, no atomics, every sum in a fixed order; a row's bits do not
// depend on the rows beside it.  No host synchronisation inside a step.
//
// log q of arbitrary points (off the step): forward substitution, one point per
// lane, by column blocks of 16 with the trailing update on a transposed residual
// (coalesced); no eigendecomposition and no inverse of L.
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

#define FRG_HIP(expr)                                                                      \
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

// sum_i M_ii of the packed parameters, by the whole block
__device__ __forceinline__ double sum_log_diag(int D, const double* lam, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < D; i += 256) a += lam[D + (long long)i * (i + 1) / 2 + i];
  return block_reduce(a, false, red);
}

// Launch 1.  One wave per sample row: z[row] from Philox (column pair d/2, sample,
// step, purpose 0: the full-rank t family's z) unless the draws are the caller's
// (src), and zz[row] = sum_d z^2 (zz nullable).  The block after the last row block
// writes scal[0] = sum M_ii (scal nullable).
__global__ __launch_bounds__(256) void frg_noise_kernel(int D, long long n, Rng rng, uint32_t step,
                                                        const double* src, double* z, double* zz,
                                                        const double* lam, double* scal) {
  __shared__ double red[4];
  const long long row_blocks = (n + 3) / 4;
  if ((long long)blockIdx.x >= row_blocks) {
    const double s = sum_log_diag(D, lam, red);
    if (threadIdx.x == 0) scal[0] = s;
    return;
  }
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const int np = (D + 1) / 2;
  double a = 0.0;
  for (int j = lane; j < np; j += 64) {
    double z0, z1 = 0.0;
    const bool two = 2 * j + 1 < D;
    if (src) {
      z0 = src[row * D + 2 * j];
      if (two) z1 = src[row * D + 2 * j + 1];
    } else {
      normal_pair(rng.draw((uint32_t)j, (uint32_t)row, step, 0u), z0, z1);
      z[row * D + 2 * j] = z0;
      if (two) z[row * D + 2 * j + 1] = z1;
    }
    a = fma(z0, z0, a);
    if (two) a = fma(z1, z1, a);
  }
  a = wave_sum(a);
  if (lane == 0 && zz) zz[row] = a;
}

// Launch 2.  X = mu + Z L^T, one wave per 16 x 16 tile (16 samples x 16 coordinates):
// A = Z (row lane & 15, k = lane >> 4), B[k][col] = L[col][k] from the packed
// parameters (exp on the diagonal, zero above it).  Tile column ct needs k < 16 (ct +
// 1) only: the k tiles above the diagonal tile are not visited.
__global__ __launch_bounds__(256) void frg_x_kernel(int D, long long n, const double* lam,
                                                    const double* z, double* x) {
  const int tiles_c = (D + 15) / 16;
  const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long rt = tile / tiles_c;
  const int ct = (int)(tile % tiles_c);
  if (rt * 16 >= n) return;
  const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const long long row = rt * 16 + r;
  const int col = ct * 16 + r;
  const int kend = min(D, (ct + 1) * 16);
  const bool row_ok = row < n, col_ok = col < D;
  const double* zrow = z + (row_ok ? row : 0) * D;
  const double* lrow = lam + D + (col_ok ? (long long)col * (col + 1) / 2 : 0);
  d4 acc[4] = {};
  for (int k0 = 0; k0 < kend; k0 += 16) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 4 * s + kq;
      double a = 0.0, b = 0.0;
      if (row_ok && k < kend) a = zrow[k];
      if (col_ok && k <= col) {
        b = lrow[k];
        if (k == col) b = exp(b);
      }
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
    }
  }
  const d4 r4 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (!col_ok) return;
  const double m = lam[col];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const long long orow = rt * 16 + kq + 4 * rr;
    if (orow < n) x[orow * D + col] = m + r4[rr];
  }
}

// Launch 3 (see the file comment).  mode: 0 KLVI, 1 CHIVI, 2 KLVI_PD.
struct FrgGradArgs {
  int D, N, mode, upd;
  double alpha;
  const double *G, *Z, *logp, *zz, *scal;
  double* value;
  double* grad;   // [P], when !upd
  double* lam;    // read (own diagonal entries); updated in place when upd
  double* ring;
  int W;
  long long step;
  double lr, eps;
  double* hrow;
};

__global__ __launch_bounds__(256) void frg_grad_kernel(FrgGradArgs a) {
  __shared__ double red[4];
  __shared__ double rs[kChunk];
  const int D = a.D, N = a.N, t = threadIdx.x;
  const double inv_n = 1.0 / N;
  // ---- weights: the same arithmetic in the same order in every block
  const double sum_m = a.scal[0];
  const double lq0 = (double)D * kHalfLog2Pi + sum_m;   // -log q(x_n) = lq0 + zz_n / 2
  double mx = 0.0, rsum = -1.0;
  if (a.mode == 1) {
    double m = -INFINITY;
    for (int k = t; k < N; k += 256) m = fmax(m, a.logp[k] + lq0 + 0.5 * a.zz[k]);
    mx = block_reduce(m, true, red);
    double sw = 0.0;
    for (int k = t; k < N; k += 256) sw += exp(a.alpha * ((a.logp[k] + lq0 + 0.5 * a.zz[k]) - mx));
    sw = block_reduce(sw, false, red);
    rsum = a.alpha * sw * inv_n;
    if (blockIdx.x == 0 && t == 0) *a.value = log(sw * inv_n) / a.alpha + mx;
  } else if (blockIdx.x == 0) {
    double s = 0.0;
    if (a.mode == 2)
      for (int k = t; k < N; k += 256) s += a.logp[k] + lq0 + 0.5 * a.zz[k];
    else
      for (int k = t; k < N; k += 256) s += a.logp[k];
    s = block_reduce(s, false, red);
    if (t == 0)
      *a.value = a.mode == 2 ? -(s * inv_n)
                             : -(((double)D * (0.5 + kHalfLog2Pi) + sum_m) + s * inv_n);
  }
  // ---- this wave's tile: row ti of the tile triangle holds the mean-gradient tile
  // (tj = -1) and the tiles tj = 0 .. ti
  const int nt = (D + 15) / 16;
  const long long n_tiles = (long long)nt * (nt + 3) / 2;
  const long long tile = (long long)blockIdx.x * 4 + (t >> 6);
  const bool live = tile < n_tiles;
  int ti = 0, tj = -1;
  if (live) {
    long long i = (long long)((sqrt(8.0 * (double)tile + 9.0) - 3.0) * 0.5);
    while ((i + 1) * (i + 4) / 2 <= tile) ++i;
    while (i * (i + 3) / 2 > tile) --i;
    ti = (int)i;
    tj = (int)(tile - i * (i + 3) / 2) - 1;
  }
  const int lane = t & 63, r = lane & 15, kq = lane >> 4;
  const int ia = ti * 16 + r;                 // A = G^T: row i = ia, k = sample
  const int jb = tj < 0 ? 0 : tj * 16 + r;    // B = diag(r) Z: column j = jb
  const bool a_ok = live && ia < D, b_ok = live && tj >= 0 && jb < D;
  const double ones = (live && tj < 0 && r == 0) ? 1.0 : 0.0;
  d4 acc[4] = {};
  for (int c0 = 0; c0 < N; c0 += kChunk) {
    const int cn = min(kChunk, N - c0);
    __syncthreads();
    for (int k = t; k < cn; k += 256) {
      double w = -inv_n;
      if (a.mode == 1)
        w = a.alpha * exp(a.alpha * ((a.logp[c0 + k] + lq0 + 0.5 * a.zz[c0 + k]) - mx)) * inv_n;
      rs[k] = w;
    }
    __syncthreads();
    if (!live) continue;
    for (int k0 = 0; k0 < cn; k0 += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = k0 + 4 * s + kq;
        double av = 0.0, bv = 0.0;
        if (k < cn) {
          const long long n = c0 + k;
          if (a_ok) av = a.G[n * D + ia];
          bv = (b_ok ? a.Z[n * D + jb] : ones) * rs[k];
        }
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[s], 0, 0, 0);
      }
    }
  }
  if (!live) return;
  const d4 r4 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  // ---- epilogue: C row = kq + 4 rr (coordinate i), column = lane & 15 (coordinate j)
  const long long P = D + (long long)D * (D + 1) / 2;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = ti * 16 + kq + 4 * rr;
    if (i >= D) continue;
    long long p;
    double g = r4[rr];
    if (tj < 0) {
      if (r != 0) continue;
      p = i;
    } else {
      const int j = tj * 16 + r;
      if (j > i) continue;
      p = D + (long long)i * (i + 1) / 2 + j;
      if (j == i) g = fma(g, exp(a.lam[p]), rsum);
    }
    if (a.upd) {
      const double v = adagrad_step(p, P, a.lam[p], g, a.ring, a.W, a.step, a.lr, a.eps, nullptr);
      a.lam[p] = v;
      if (a.hrow) a.hrow[p] = v;
    } else {
      a.grad[p] = g;
    }
  }
}

// lw_n = log p(x_n) - log q(x_n) on the family's own draws
__global__ __launch_bounds__(256) void frg_lw_kernel(int D, long long m, const double* logp,
                                                     const double* zz, const double* scal,
                                                     double* lw) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  lw[k] = logp[k] + ((double)D * kHalfLog2Pi + scal[0]) + 0.5 * zz[k];
}

// log q of arbitrary points, one point per lane: y = L^-1 (x - mu) by column blocks of
// 16.  Each block's 16 unknowns are solved in registers, then the rows below take the
// trailing update r_i -= sum_k L[i][b0 + k] y_k on the transposed residual yt [D][n]
// (first touched, from x - mu, by the first block's update).
__global__ __launch_bounds__(256) void frg_logq_kernel(int D, long long n, const double* lam,
                                                       const double* x, double* yt, double* out) {
  __shared__ double red[4];
  const double sum_m = sum_log_diag(D, lam, red);
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const double* xr = x + row * D;
  double ss = 0.0;
  for (int b0 = 0; b0 < D; b0 += 16) {
    const int bw = min(16, D - b0);
    double y[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      y[k] = 0.0;
      if (k < bw) {
        const int i = b0 + k;
        const double* li = lam + D + (long long)i * (i + 1) / 2;
        double c = b0 == 0 ? xr[i] - lam[i] : yt[(long long)i * n + row];
#pragma unroll
        for (int m = 0; m < k; ++m) c = fma(-li[b0 + m], y[m], c);
        y[k] = c / exp(li[i]);
        ss = fma(y[k], y[k], ss);
      }
    }
    for (int i = b0 + 16; i < D; ++i) {
      const double* li = lam + D + (long long)i * (i + 1) / 2 + b0;
      double c = b0 == 0 ? xr[i] - lam[i] : yt[(long long)i * n + row];
#pragma unroll
      for (int k = 0; k < 16; ++k) c = fma(-li[k], y[k], c);
      yt[(long long)i * n + row] = c;
    }
  }
  out[row] = (-(double)D * kHalfLog2Pi - sum_m) - 0.5 * ss;
}

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

int grid_ok(long long blocks) {
  if (blocks > 2147483647LL) return vb_set_error(-4, "full-rank Gaussian: too many rows for one launch");
  return 0;
}

// launches 1 and 2 of a step / sample / log-weight call: z (the workspace's or the
// caller's), zz (nullable), scal[0] = sum M_ii (with zz), x
int draw_transform(const FrRows& b, int D, long long n, const double* lam, const Noise& nz,
                   bool want_zz, double* x, const double** z_out, hipStream_t st) {
  const double* z = nz.eps ? nz.eps : b.Z;
  if (!nz.eps || want_zz) {
    const long long nb = cdiv(n, 4) + (want_zz ? 1 : 0);
    if (int rc = grid_ok(nb)) return rc;
    hipLaunchKernelGGL(frg_noise_kernel, dim3((unsigned)nb), dim3(256), 0, st, D, n,
                       Rng{nz.k0, nz.k1, nz.stream}, (uint32_t)nz.step, nz.eps, b.Z,
                       want_zz ? b.zz : nullptr, lam, want_zz ? b.scal : nullptr);
  }
  const long long tiles = cdiv(n, 16) * cdiv(D, 16);
  if (int rc = grid_ok(cdiv(tiles, 4))) return rc;
  hipLaunchKernelGGL(frg_x_kernel, dim3((unsigned)cdiv(tiles, 4)), dim3(256), 0, st, D, n, lam, z, x);
  FRG_HIP(hipGetLastError());
  *z_out = z;
  return 0;
}

}  // namespace

// x [n][D] = mu + z L^T; nz.eps (host draws, on the device) = z [n][D]
int frg_sample(FrWork* W, const Family& f, const double* lam, long long n, const Noise& nz,
               double* x, hipStream_t st) {
  FrRows b;
  if (int rc = fr_rows(W, f.D, n, &b)) return rc;
  const double* z;
  return draw_transform(b, f.D, n, lam, nz, false, x, &z, st);
}

// One KLVI / KLVI_PD / CHIVI value + gradient at lam (device pointers).  up non-null:
// the windowed adagrad step rides in the gradient kernel's epilogue (lam updated in
// place, ring / history row written; grad is not written).
int frg_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz, double* value,
                   double* grad, hipStream_t st, const MfUpdate* up) {
  const int D = f.fam.D, N = f.N;
  FrRows b;
  if (int rc = fr_rows(W, D, N, &b)) return rc;
  const double* z;
  if (int rc = draw_transform(b, D, N, lam, nz, true, b.X, &z, st)) return rc;
  if (int rc = target_eval(W, f.tgt, N, b.X, b.logp, b.G, st)) return rc;
  FrgGradArgs a{};
  a.D = D;
  a.N = N;
  a.mode = f.chivi ? 1 : f.pd ? 2 : 0;
  a.upd = up != nullptr;
  a.alpha = f.alpha;
  a.G = b.G;
  a.Z = z;
  a.logp = b.logp;
  a.zz = b.zz;
  a.scal = b.scal;
  a.value = value;
  a.grad = grad;
  a.lam = const_cast<double*>(lam);
  if (up) {
    a.ring = up->ring;
    a.W = up->W;
    a.step = up->step;
    a.lr = up->lr;
    a.eps = up->eps;
    a.hrow = up->hrow;
  }
  const long long nt = cdiv(D, 16), tiles = nt * (nt + 3) / 2;
  hipLaunchKernelGGL(frg_grad_kernel, dim3((unsigned)cdiv(tiles, 4)), dim3(256), 0, st, a);
  FRG_HIP(hipGetLastError());
  return 0;
}

// log q(x) for arbitrary x [n][D] at lam
int frg_logdensity(FrWork* W, const Family& f, const double* lam, const double* x, long long n,
                   double* out, hipStream_t st) {
  FrRows b;
  if (int rc = fr_rows(W, f.D, n, &b)) return rc;
  if (int rc = grid_ok(cdiv(n, 256))) return rc;
  hipLaunchKernelGGL(frg_logq_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, f.D, n, lam, x,
                     b.X, out);
  FRG_HIP(hipGetLastError());
  return 0;
}

// log weights lw = log p(x) - log q(x), x ~ q; xs (nullable) receives the samples
int frg_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                    double* lw, double* xs, hipStream_t st) {
  const int D = f.fam.D;
  FrRows b;
  if (int rc = fr_rows(W, D, m, &b)) return rc;
  double* x = xs ? xs : b.X;
  const double* z;
  if (int rc = draw_transform(b, D, m, lam, nz, true, x, &z, st)) return rc;
  if (int rc = target_eval(W, f.tgt, m, x, b.logp, nullptr, st)) return rc;
  hipLaunchKernelGGL(frg_lw_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, D, m, b.logp,
                     b.zz, b.scal, lw);
  FRG_HIP(hipGetLastError());
  return 0;
}

}  // namespace vbk
