// vb_mlm.hip — multilevel regression on the device (VB_TARGET_MULTILEVEL).
//
// A regression whose intercept varies by group: M observations sorted by group, p fixed
// effects, G groups; x = [beta (p), u = log tau, then G more], D = p + 1 + G; the
// normalised joint density in these coordinates (layout and formulas in
// include/viabel_amd.h), tau = exp(u), w = (tau / s_tau)^2:
//
//   common        - sum beta_d^2 / (2 s^2) - log1p(w) + u + sum_m l(y_m, eta_m) + constants
//   non-centred   - sum at_g^2 / 2,                  eta_m = x_m . beta + tau at_g(m)
//   centred       - G u - sum (a_g / tau)^2 / 2,     eta_m = x_m . beta + a_g(m)
//
// With dl_m = dl / d eta_m and S_g the sum of dl_m over group g:
//   d beta = -beta / s^2 + sum_m dl_m x_m
//   centred       d a_g = S_g - a_g / tau^2,   d u = 1 - 2 w / (1 + w) + sum (a_g / tau)^2 - G
//   non-centred   d at_g = tau S_g - at_g,     d u = 1 - 2 w / (1 + w) + tau sum S_g at_g
//
// for the n sample rows of x [n][D].  All arithmetic is fp64, no atomics, every sum in a
// fixed order.  The grid is sample-row tiles x observation chunks, as in vb_glm.hip: a
// fit step has ~100 rows, so the observations must fill the chip.  A chunk is a whole
// number of 64-observation tiles; there are min(ceil(M / 64), ceil(1024 / row tiles))
// of them (a constant, not the device's CU count: the bits do not depend on the chip),
// fewer when the chunk partials would pass kMlmScratchMax.
//
// Every lane of a block walks the same observations, so the group of an observation is
// block-uniform: a lane carries the running S_g of the current group and flushes it
// when the group changes, with no divergence.  A group that lies inside a chunk is
// finished there (its gradient entry stored, S_g at_g added to the chunk's sum); the
// chunk's first and last group may continue in its neighbours, so their S go to the
// chunk partials.  mlm_combine_kernel (one wave per sample row) adds the partials of
// log p, d beta and those groups in chunk order, and the prior terms.
//
//   p <= 16 (mlm_rows_lane_kernel): one lane per sample row, beta and its gradient in
//     registers; X, y and the group ids of 64 observations staged in LDS and read as
//     broadcasts.
//   p > 16 (mlm_rows_tile_kernel): 64 sample rows per block, 16 observations at a time
//     with their eta in registers, X staged in LDS slices of 16 columns; d beta is
//     accumulated in the chunk's partial in global memory (each lane its own row).  No
//     matrix instructions yet.
//
// The links are obs_link of vb_links.hpp, the definition vb_glm.hip uses; the two count
// links (poisson_log, neg_binomial_2_log) add the block's offset eta0 [M] to eta.
// grad == nullptr selects instances without gradient work; the value's operations are
// the same, so it is the same bit for bit.
//
// Learned scale / dispersion (the block's `learn`): the sample rows are [beta (p), u, G
// more, lambda], D = p + 2 + G, lambda = log sigma (gaussian, student_t) or log phi
// (neg_binomial_2_log) with e^lambda ~ half-Cauchy(0, s_aux); every other offset stays.
// The row kernels serve it as the instances LIK = 5, 6, 7 (the learned forms of 0, 1, 4,
// defined in vb_links.hpp beside the fixed ones): both kernels have one lane per sample
// row, so a lane forms its row's link constants from x[row][D - 1] in its prologue and
// keeps them in registers.  dl carries 1 / sigma, so S_g and every formula above hold as
// written.  sum_m dl/dlambda is one more per-row accumulator (LIK 6, 7 with a gradient;
// the gaussian's is -M - 2 sum l), stored to the chunk partial pla beside plp.
// mlm_combine_kernel's learned instances (its second template parameter) add it in the
// same chunk-order walk, and lane 0 adds -M lambda (gaussian, student_t), the prior of
// lambda and, for the negative binomial, the table sums A(phi) and dA/dlambda that
// mlm_disp_kernel formed before the row kernel, and writes grad[row][D - 1].
#include <algorithm>
#include <cmath>

#include "../../include/viabel_amd.h"
#include "vb_device.hpp"
#include "vb_internal.hpp"
#include "vb_links.hpp"

using namespace vbd;

namespace vbk {
namespace {

constexpr int kMlmLaneP = 16;      // lane-per-row kernel: p <= 16
constexpr int kMlmTile = 64;       // observations per LDS tile (lane kernel); chunk granule
constexpr int kMlmTM = 16;         // observations per round of the tile kernel
constexpr int kMlmKS = 16;         // columns per LDS slice of the tile kernel
constexpr long long kMlmBlocks = 1024;                    // row tiles x chunks aimed at
constexpr long long kMlmScratchMax = 32LL << 20;          // doubles of chunk partials at most

struct MlmK {
  int p, G, D, nchunk, centered;
  long long n, M, chunk_obs;
  LinkK lk;                       // link constants (vb_links.hpp)
  double inv_s2, inv_stau, c_all; // prior precision, 1 / s_tau, every constant of log p
  const double* X;                // [M][p]
  const double* y;                // [M]
  const double* off;              // [G + 1]
  const double* x;                // [n][D]
  double* logp;                   // [n]
  double* grad;                   // [n][D] or null
  double* bnd;                    // [nchunk][2]: first and last group of a chunk (grad)
  double* plp;                    // [n][nchunk]
  double* pf;                     // [n][nchunk]: S of the chunk's first group (grad)
  double* pl;                     // [n][nchunk]: S of its last group, 0 if the same (grad)
  double* psa;                    // [n][nchunk]: sum S_g at_g of the groups inside (grad)
  double* pg;                     // [nchunk][n][p] (grad)
  const double* eta0;             // [M]: offset of eta (LIK 3, 4, 7; not read otherwise)
  // learned mode (LIK >= 5): column D - 1 of x and grad is lambda
  long long J;                    // length of T (LIK 7)
  double nu, inv_nu;              // student_t (lk.k1, lk.k2 as in obs_link)
  double ls_aux, Mf;              // log s_aux; M as a double
  const double* T;                // [J]: T[j] = #{m : y_m > j}
  double* tab;                    // [2][n]: A(phi), dA/dlambda of the rows (LIK 7)
  double* pla;                    // [n][nchunk]: sum dl/dlambda of the chunk (grad; LIK 6, 7)
};

// The group g with off[g] <= m < off[g + 1], searched from lo (off[lo] <= m); the
// result lies in [lo, G - 1] whatever off holds.
__device__ __forceinline__ int mlm_group_of(const double* off, int G, long long m, int lo) {
  const double dm = (double)m;
  int hi = G;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= dm)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// A lane's walk over the groups of its chunk.
struct MlmWalk {
  int cg;                 // current group, -1 before the first observation
  double S;               // running sum of dl over the current group
  double araw, aeff;      // the row's coordinate of the group; its intercept
  double Sfirst, Slast;   // S of the chunk's first / last group
  double sa;              // sum S_g at_g over the groups inside the chunk (non-centred)
};

// The current group ends (in this chunk): gr = the row's gradient entries of the groups.
template <bool GRAD>
__device__ __forceinline__ void mlm_flush(const MlmK& k, MlmWalk& w, int gfirst, int glast,
                                          double tau, double it, double* gr, bool live) {
  if constexpr (GRAD) {
    if (w.cg < 0) return;
    if (w.cg == gfirst) {
      w.Sfirst = w.S;
    } else if (w.cg == glast) {
      w.Slast = w.S;
    } else if (k.centered) {
      if (live) gr[w.cg] = w.S - (w.araw * it) * it;
    } else {
      if (live) gr[w.cg] = tau * w.S - w.araw;
      w.sa = fma(w.S, w.araw, w.sa);
    }
  }
}

// Observation of group gi comes next: flush and load on a change of group.
template <bool GRAD>
__device__ __forceinline__ void mlm_enter(const MlmK& k, MlmWalk& w, int gi, int gfirst, int glast,
                                          double tau, double it, const double* ar, double* gr,
                                          bool live) {
  if (gi != w.cg) {
    mlm_flush<GRAD>(k, w, gfirst, glast, tau, it, gr, live);
    w.cg = gi;
    w.araw = ar[gi];
    w.aeff = k.centered ? w.araw : tau * w.araw;
    w.S = 0.0;
  }
}

// The chunk's partials of one row.
template <bool GRAD>
__device__ __forceinline__ void mlm_store_partials(const MlmK& k, const MlmWalk& w, long long row,
                                                   int c, double lp) {
  const long long pr = row * k.nchunk + c;
  k.plp[pr] = lp;
  if constexpr (GRAD) {
    k.pf[pr] = w.Sfirst;
    k.pl[pr] = w.Slast;
    k.psa[pr] = w.sa;
  }
}

// ---- p <= 16: one lane per sample row ---------------------------------------------
template <int LIK, bool GRAD, int PP>
__global__ __launch_bounds__(256) void mlm_rows_lane_kernel(MlmK k) {
  __shared__ double Xs[kMlmTile * PP];
  constexpr bool OFFS = link_offset(LIK);       // eta0 rides behind y in the tile
  constexpr bool LRN = link_learned(LIK);
  __shared__ double ys[OFFS ? 2 * kMlmTile : kMlmTile];
  __shared__ int gs[kMlmTile];
  const int t = threadIdx.x, nt = blockDim.x, p = k.p, G = k.G;
  const long long row = (long long)blockIdx.x * nt + t;
  const bool live = row < k.n;
  // a lane past the last row walks with the last row's values and stores nothing
  const long long rr = live ? row : k.n - 1;
  const double* xr = k.x + rr * k.D;
  const double* ar = xr + p + 1;
  double* gr = GRAD ? k.grad + rr * k.D + p + 1 : nullptr;
  double beta[PP], g[PP];
#pragma unroll
  for (int d = 0; d < PP; ++d) {
    beta[d] = d < p ? xr[d] : 0.0;
    g[d] = 0.0;
  }
  const double tau = exp_fast(xr[p]);
  const double it = rcp_refined(tau);
  double ca = 0.0, cb = 0.0, la = 0.0;   // learned mode only
  if constexpr (LRN) glm_row_consts<LIK>(xr[k.D - 1], ca, cb);
  const int c = blockIdx.y;
  const long long m0 = (long long)c * k.chunk_obs;
  const long long m1 = m0 + k.chunk_obs < k.M ? m0 + k.chunk_obs : k.M;
  const int gfirst = mlm_group_of(k.off, G, m0, 0);
  const int glast = mlm_group_of(k.off, G, m1 - 1, gfirst);
  if (GRAD && blockIdx.x == 0 && t == 0) {
    k.bnd[2 * c] = (double)gfirst;
    k.bnd[2 * c + 1] = (double)glast;
  }
  MlmWalk w{-1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double lp = 0.0;
  int gt = gfirst;   // group of the last observation staged so far
  for (long long mt = m0; mt < m1; mt += kMlmTile) {
    const int cnt = m1 - mt < kMlmTile ? (int)(m1 - mt) : kMlmTile;
    __syncthreads();
    for (int i = t; i < kMlmTile * PP; i += nt) {
      const int mm = i / PP, d = i % PP;
      Xs[i] = (mm < cnt && d < p) ? k.X[(mt + mm) * p + d] : 0.0;
    }
    for (int i = t; i < kMlmTile; i += nt) {
      ys[i] = i < cnt ? k.y[mt + i] : 0.0;
      if constexpr (OFFS) ys[kMlmTile + i] = i < cnt ? k.eta0[mt + i] : 0.0;
      gs[i] = i < cnt ? mlm_group_of(k.off, G, mt + i, gt) : gt;
    }
    __syncthreads();
    for (int mm = 0; mm < cnt; ++mm) {
      mlm_enter<GRAD>(k, w, gs[mm], gfirst, glast, tau, it, ar, gr, live);
      const double* xm = Xs + mm * PP;
      double eta = w.aeff;
#pragma unroll
      for (int d = 0; d < PP; ++d) eta = fma(beta[d], xm[d], eta);
      if constexpr (OFFS) eta += ys[kMlmTile + mm];
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
        w.S += dl;
#pragma unroll
        for (int d = 0; d < PP; ++d) g[d] = fma(dl, xm[d], g[d]);
      }
    }
    gt = gs[cnt - 1];
  }
  mlm_flush<GRAD>(k, w, gfirst, glast, tau, it, gr, live);
  if (!live) return;
  mlm_store_partials<GRAD>(k, w, row, c, lp);
  if constexpr (GRAD && LRN && LIK != 5) k.pla[row * k.nchunk + c] = la;
  if constexpr (GRAD) {
    double* pg = k.pg + ((long long)c * k.n + row) * p;
#pragma unroll
    for (int d = 0; d < PP; ++d)
      if (d < p) pg[d] = g[d];
  }
}

// ---- p > 16: 64 sample rows per block, 16 observations per round -------------------
template <int LIK, bool GRAD>
__global__ __launch_bounds__(64) void mlm_rows_tile_kernel(MlmK k) {
  __shared__ double Xs[kMlmTM * kMlmKS];
  constexpr bool OFFS = link_offset(LIK);       // eta0 rides behind y
  constexpr bool LRN = link_learned(LIK);
  __shared__ double ys[OFFS ? 2 * kMlmTM : kMlmTM];
  __shared__ int gs[kMlmTM];
  const int t = threadIdx.x, p = k.p, G = k.G;
  const long long row = (long long)blockIdx.x * 64 + t;
  const bool live = row < k.n;
  const long long rr = live ? row : k.n - 1;
  const double* xr = k.x + rr * k.D;
  const double* ar = xr + p + 1;
  double* gr = GRAD ? k.grad + rr * k.D + p + 1 : nullptr;
  const double tau = exp_fast(xr[p]);
  const double it = rcp_refined(tau);
  double ca = 0.0, cb = 0.0, la = 0.0;   // learned mode only
  if constexpr (LRN) glm_row_consts<LIK>(xr[k.D - 1], ca, cb);
  const int c = blockIdx.y;
  const long long m0 = (long long)c * k.chunk_obs;
  const long long m1 = m0 + k.chunk_obs < k.M ? m0 + k.chunk_obs : k.M;
  const int gfirst = mlm_group_of(k.off, G, m0, 0);
  const int glast = mlm_group_of(k.off, G, m1 - 1, gfirst);
  if (GRAD && blockIdx.x == 0 && t == 0) {
    k.bnd[2 * c] = (double)gfirst;
    k.bnd[2 * c + 1] = (double)glast;
  }
  double* pg =GRAD ? k.pg + ((long long)c * k.n + rr) * p : nullptr;
  MlmWalk w{-1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double lp = 0.0;
  int gt = gfirst;
  // X[mt + mm][c0 + j] -> Xs[mm][j], zero past the chunk's end and past column p
  auto stage = [&](long long mt, int cnt, int c0) {
    for (int i = t; i < kMlmTM * kMlmKS; i += 64) {
      const int mm = i / kMlmKS, j = i % kMlmKS;
      Xs[i] = (mm < cnt && c0 + j < p) ? k.X[(mt + mm) * p + c0 + j] : 0.0;
    }
  };
  for (long long mt = m0; mt < m1; mt += kMlmTM) {
    const int cnt = m1 - mt < kMlmTM ? (int)(m1 - mt) : kMlmTM;
    double eta[kMlmTM];
#pragma unroll
    for (int mm = 0; mm < kMlmTM; ++mm) eta[mm] = 0.0;
    for (int c0 = 0; c0 < p; c0 += kMlmKS) {
      __syncthreads();
      stage(mt, cnt, c0);
      if (c0 == 0 && t < kMlmTM) {
        ys[t] = t < cnt ? k.y[mt + t] : 0.0;
        if constexpr (OFFS) ys[kMlmTM + t] = t < cnt ? k.eta0[mt + t] : 0.0;
        gs[t] = t < cnt ? mlm_group_of(k.off, G, mt + t, gt) : gt;
      }
      __syncthreads();
      double b[kMlmKS];
#pragma unroll
      for (int j = 0; j < kMlmKS; ++j) b[j] = c0 + j < p ? xr[c0 + j] : 0.0;
#pragma unroll
      for (int mm = 0; mm < kMlmTM; ++mm) {
#pragma unroll
        for (int j = 0; j < kMlmKS; ++j) eta[mm] = fma(b[j], Xs[mm * kMlmKS + j], eta[mm]);
      }
    }
    double dlv[kMlmTM];
#pragma unroll
    for (int mm = 0; mm < kMlmTM; ++mm) {
      dlv[mm] = 0.0;
      if (mm < cnt) {
        mlm_enter<GRAD>(k, w, gs[mm], gfirst, glast, tau, it, ar, gr, live);
        double l, dl;
        if constexpr (LRN) {
          double dlam;
          glm_link_aux<LIK>(k, ca, cb,
                            OFFS ? (eta[mm] + w.aeff) + ys[kMlmTM + mm] : eta[mm] + w.aeff, ys[mm],
                            l, dl, dlam);
          if constexpr (GRAD && LIK != 5) la += dlam;
        } else if constexpr (OFFS) {
          obs_link<LIK>(k.lk, (eta[mm] + w.aeff) + ys[kMlmTM + mm], ys[mm], l, dl);
        } else {
          obs_link<LIK>(k.lk, eta[mm] + w.aeff, ys[mm], l, dl);
        }
        lp += l;
        if constexpr (GRAD) {
          w.S += dl;
          dlv[mm] = dl;
        }
      }
    }
    gt = gs[cnt - 1];
    if constexpr (GRAD) {
      const bool first = mt == m0;
      for (int c0 = 0; c0 < p; c0 += kMlmKS) {
        __syncthreads();
        stage(mt, cnt, c0);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kMlmKS; ++j) {
          double s = 0.0;
#pragma unroll
          for (int mm = 0; mm < kMlmTM; ++mm) s = fma(dlv[mm], Xs[mm * kMlmKS + j], s);
          if (live && c0 + j < p) pg[c0 + j] = first ? s : pg[c0 + j] + s;
        }
      }
    }
  }
  mlm_flush<GRAD>(k, w, gfirst, glast, tau, it, gr, live);
  if (live) {
    mlm_store_partials<GRAD>(k, w, row, c, lp);
    if constexpr (GRAD && LRN && LIK != 5) k.pla[row * k.nchunk + c] = la;
  }
}

// ---- chunk partials and prior terms: one wave per sample row ---------------------------
// LIK = 0: a fixed block; 5, 6, 7: the learned instances, which also add pla and finish
// lambda's entry
template <bool GRAD, int LIK = 0>
__global__ __launch_bounds__(64) void mlm_combine_kernel(MlmK k) {
  constexpr bool LRN = link_learned(LIK);
  constexpr bool LACC = LRN && GRAD && LIK != 5;   // pla is summed
  const int lane = threadIdx.x, p = k.p, G = k.G, nc = k.nchunk;
  const long long row = blockIdx.x;
  const double* xr = k.x + row * k.D;
  const double* ar = xr + p + 1;
  double* gr = GRAD ? k.grad + row * k.D + p + 1 : nullptr;
  const double u = xr[p];
  const double tau = exp_fast(u);
  const double it = rcp_refined(tau);
  // the groups' prior: z_g = a_g / tau (centred) or at_g; a group without observations
  // has no other gradient term
  double zz = 0.0;
  for (int g = lane; g < G; g += 64) {
    const double a = ar[g];
    const double z = k.centered ? a * it : a;
    zz = fma(z, z, zz);
    if constexpr (GRAD) {
      if (k.off[g + 1] == k.off[g]) gr[g] = k.centered ? -(z * it) : -a;
    }
  }
  zz = wave_sum_dpp(zz);
  // beta's prior, and d beta from the chunks in chunk order
  double ss = 0.0;
  for (int d = lane; d < p; d += 64) {
    const double b = xr[d];
    ss = fma(b, b, ss);
    if constexpr (GRAD) {
      double s = 0.0;
      for (int c = 0; c < nc; ++c) s += k.pg[((long long)c * k.n + row) * p + d];
      k.grad[row * k.D + d] = s - b * k.inv_s2;
    }
  }
  ss = wave_sum_dpp(ss);
  // the chunks, 64 at a time: a lane loads one chunk's partials, every lane then walks
  // them in chunk order (the same operations in every lane)
  double lps = 0.0, sa = 0.0, S = 0.0, las = 0.0;
  int cur = -1;
  auto finish = [&](int g, double Sg) {
    const double a = ar[g];
    if (k.centered) {
      if (lane == 0) gr[g] = Sg - (a * it) * it;
    } else {
      if (lane == 0) gr[g] = tau * Sg - a;
      sa = fma(Sg, a, sa);
    }
  };
  for (int cb = 0; cb < nc; cb += 64) {
    const int cc = cb + lane;
    const bool ok = cc < nc;
    const long long pr = row * nc + (ok ? cc : nc - 1);
    const double vlp = ok ? k.plp[pr] : 0.0;
    double vf = 0.0, vl = 0.0, vsa = 0.0, vla = 0.0;
    int bf = 0, bl = 0;
    if constexpr (LACC) vla = ok ? k.pla[pr] : 0.0;
    if constexpr (GRAD) {
      vf = k.pf[pr];
      vl = k.pl[pr];
      vsa = k.psa[pr];
      bf = (int)k.bnd[2 * (ok ? cc : nc - 1)];
      bl = (int)k.bnd[2 * (ok ? cc : nc - 1) + 1];
    }
    const int cnt = nc - cb < 64 ? nc - cb : 64;
    for (int i = 0; i < cnt; ++i) {
      lps += readlane_f64(vlp, i);
      if constexpr (LACC) las += readlane_f64(vla, i);
      if constexpr (GRAD) {
        sa += readlane_f64(vsa, i);
        const int f = __builtin_amdgcn_readlane(bf, i), l = __builtin_amdgcn_readlane(bl, i);
        const double sf = readlane_f64(vf, i), sl = readlane_f64(vl, i);
        if (f != cur) {
          if (cur >= 0) finish(cur, S);
          cur = f;
          S = 0.0;
        }
        S += sf;
        if (l != f) {
          finish(cur, S);
          cur = l;
          S = sl;
        }
      }
    }
  }
  if constexpr (GRAD) {
    if (cur >= 0) finish(cur, S);
  }
  if (lane != 0) return;
  // tau's half-Cauchy prior and the Jacobian (the guard at w = inf as vb_hier.hip)
  const double t5 = tau * k.inv_stau;
  const double w = t5 * t5;
  const double l1 = w < INFINITY ? log1p_pos_fast(w) : w;
  double cl = u - l1;
  if (k.centered) cl -= (double)G * u;
  const double v = k.c_all + (((lps - 0.5 * k.inv_s2 * ss) - 0.5 * zz) + cl);
  if constexpr (LRN) {
    // -M lambda (gaussian, student_t), the prior of lambda, the table sums (vb_glm.hip's
    // glm_aux_final, term by term)
    const double lam = xr[k.D - 1];
    double sp, lg;
    aux_lambda_prior(lam, k.ls_aux, sp, lg);
    const double gp = 1.0 - 2.0 * lg;
    if constexpr (LIK == 7)
      k.logp[row] = v + ((lam - sp) + k.tab[row]);
    else
      k.logp[row] = v + (fma(-k.Mf, lam, lam) - sp);
    if constexpr (GRAD) {
      double gl;
      if constexpr (LIK == 7)
        gl = (las + k.tab[k.n + row]) + gp;
      else if constexpr (LIK == 5)
        gl = (-2.0 * lps - k.Mf) + gp;
      else
        gl = (las - k.Mf) + gp;
      k.grad[row * k.D + k.D - 1] = gl;
    }
  } else {
    k.logp[row] = v;
  }
  if constexpr (GRAD) {
    const double gw = w < INFINITY ? fma(-2.0 * w, rcp_refined(1.0 + w), 1.0) : -1.0;
    k.grad[row * k.D + p] = gw + (k.centered ? zz - (double)G : tau * sa);
  }
}

// learned dispersion: the table sums of the n rows (disp_row_sums of vb_links.hpp), one
// sample row per block, lambda in the rows' last column
__global__ __launch_bounds__(256) void mlm_disp_kernel(MlmK k) {
  disp_row_sums(k.x, k.D, k.D - 1, k.T, k.J, k.tab, k.n);
}

struct MlmPlan {
  bool small;
  int tb;              // threads per block = sample rows per block
  int nchunk;
  long long chunk_obs, row_blocks;
};

// doubles of chunk partials per chunk; extra: 1 where a learned block carries pla
long long mlm_per_chunk(int p, long long n, bool grad, int extra = 0) {
  return 2 + std::max<long long>(1, n) * (1 + (grad ? 3 + p + extra : 0));
}

MlmPlan mlm_plan(int p, long long n, long long M, bool grad, int extra = 0) {
  MlmPlan pl{};
  pl.small = p <= kMlmLaneP;
  pl.tb = pl.small ? (n <= 4096 ? 64 : 256) : 64;
  pl.row_blocks = (n + pl.tb - 1) / pl.tb;
  const long long max_chunks = std::min<long long>((M + kMlmTile - 1) / kMlmTile, 1024);
  long long nc = std::max<long long>(
      1, std::min(max_chunks, (kMlmBlocks + pl.row_blocks - 1) / std::max<long long>(1, pl.row_blocks)));
  const long long per = mlm_per_chunk(p, n, grad, extra);
  if (nc > 1 && nc * per > kMlmScratchMax) nc = std::max<long long>(1, kMlmScratchMax / per);
  long long co = (M + nc - 1) / nc;
  co = (co + kMlmTile - 1) / kMlmTile * kMlmTile;
  pl.chunk_obs = co;
  pl.nchunk = (int)((M + co - 1) / co);
  return pl;
}

template <int LIK, bool GRAD>
void mlm_launch(const MlmPlan& pl, const MlmK& k, hipStream_t s) {
  const dim3 g((unsigned)pl.row_blocks, (unsigned)pl.nchunk), b(pl.tb);
  if (!pl.small)
    hipLaunchKernelGGL((mlm_rows_tile_kernel<LIK, GRAD>), g, b, 0, s, k);
  else if (k.p <= 2)
    hipLaunchKernelGGL((mlm_rows_lane_kernel<LIK, GRAD, 2>), g, b, 0, s, k);
  else if (k.p <= 4)
    hipLaunchKernelGGL((mlm_rows_lane_kernel<LIK, GRAD, 4>), g, b, 0, s, k);
  else if (k.p <= 8)
    hipLaunchKernelGGL((mlm_rows_lane_kernel<LIK, GRAD, 8>), g, b, 0, s, k);
  else
    hipLaunchKernelGGL((mlm_rows_lane_kernel<LIK, GRAD, 16>), g, b, 0, s, k);
}

// the row kernel and the combine kernel of a learned instance
template <int LIK>
hipError_t mlm_launch_aux(const MlmPlan& pl, const MlmK& k, hipStream_t s) {
  const bool g = k.grad != nullptr;
  g ? mlm_launch<LIK, true>(pl, k, s) : mlm_launch<LIK, false>(pl, k, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (g)
    hipLaunchKernelGGL((mlm_combine_kernel<true, LIK>), dim3((unsigned)k.n), dim3(64), 0, s, k);
  else
    hipLaunchKernelGGL((mlm_combine_kernel<false, LIK>), dim3((unsigned)k.n), dim3(64), 0, s, k);
  return hipGetLastError();
}

// a learned block carries pla (the gaussian needs none) and, for a dispersion, tab
int mlm_extra(const MlmHead& h) { return h.learn && h.lik != 0 ? 1 : 0; }
size_t mlm_tab_doubles(const MlmHead& h, long long n) {
  return h.learn && h.lik == 4 ? 2 * (size_t)n : 0;
}

}  // namespace

// [tab 2 n (learned dispersion)] [bnd] [plp] [pf] [pl] [psa] [pla (learned 1, 4)] [pg]
size_t mlm_scratch_doubles(int D, long long n, const MlmHead& h, bool grad) {
  if (n < 1) return 0;
  const long long pc = mlm_coefs(D, h);
  if (pc < 1) return 0;
  const int p = (int)pc, extra = mlm_extra(h);
  const MlmPlan pl = mlm_plan(p, n, h.M, grad, extra);
  return mlm_tab_doubles(h, n) + (size_t)pl.nchunk * (size_t)mlm_per_chunk(p, n, grad, extra);
}

hipError_t launch_mlm_rows(int D, long long n, const MlmHead& h, const double* params,
                           const double* x, double* logp, double* grad, double* scratch,
                           hipStream_t s) {
  if (n < 1) return hipSuccess;
  if (!params || !x || !logp || !scratch || h.M < 1 || h.G < 1 || h.G > 0x7fff0000LL ||
      mlm_coefs(D, h) < 1)
    return hipErrorInvalidValue;
  if (h.learn && (h.lik == 2 || h.lik == 3 || h.J < 0 || h.J > 65536)) return hipErrorInvalidValue;
  const int p = (int)mlm_coefs(D, h), extra = mlm_extra(h);
  const MlmPlan pl = mlm_plan(p, n, h.M, grad != nullptr, extra);
  if (pl.row_blocks > 0x7fffffffLL || n > 0x7fffffffLL) return hipErrorInvalidValue;
  MlmK k{};
  k.p = p;
  k.G = (int)h.G;
  k.D = D;
  k.nchunk = pl.nchunk;
  k.centered = h.centered;
  k.n = n;
  k.M = h.M;
  k.chunk_obs = pl.chunk_obs;
  k.inv_s2 = 1.0 / (h.prior * h.prior);
  k.inv_stau = 1.0 / h.tau_scale;
  // beta's prior, the observations, the half-Cauchy log(2 / (pi s_tau)), the groups' normal
  double c_obs;
  if (h.learn) {
    // as launch_glm_rows forms them for a learned block (vb_links.hpp): c_obs without
    // -log sigma, and the half-Cauchy log(2 / (pi s_aux)) of e^lambda
    const AuxConsts a = aux_consts(h.lik, h.nu, h.s_aux);
    k.lk.k1 = a.k1;
    k.lk.k2 = a.k2;
    k.nu = a.nu;
    k.inv_nu = a.inv_nu;
    k.ls_aux = a.ls_aux;
    k.Mf = (double)h.M;
    c_obs = a.c_obs;
  } else {
    c_obs = link_consts(h.lik, h.nu, h.sigma, h.phi, &k.lk);
  }
  k.c_all = -(double)p * (0.5 * kLog2Pi + std::log(h.prior)) + (double)h.M * c_obs +
            (std::log(2.0 / M_PI) - std::log(h.tau_scale)) - (double)h.G * (0.5 * kLog2Pi);
  if (h.lik >= 3) k.c_all += h.c_data;   // the data-only constants, summed by the packer
  if (h.learn) k.c_all += kLogTwoOverPi - k.ls_aux;
  k.X = params + kMlmHeader;
  k.y = k.X + (size_t)h.M * p;
  k.off = k.y + h.M;
  k.eta0 = h.lik >= 3 ? k.off + h.G + 1 : nullptr;
  if (h.learn && h.lik == 4) {   // behind eta0: c_data, s_aux, J
    k.J = h.J;
    k.T = k.eta0 + h.M + 3;
  }
  k.x = x;
  k.logp = logp;
  k.grad = grad;
  const size_t nn = (size_t)n * pl.nchunk;
  const size_t ntab = mlm_tab_doubles(h, n);
  if (ntab) k.tab = scratch;
  k.bnd = scratch + ntab;
  k.plp = k.bnd + 2 * (size_t)pl.nchunk;
  if (grad) {
    k.pf = k.plp + nn;
    k.pl = k.pf + nn;
    k.psa = k.pl + nn;
    k.pla = extra ? k.psa + nn : nullptr;
    k.pg = k.psa + nn + (extra ? nn : 0);
  }
  if (h.learn) {
    if (h.lik == 4) {
      hipLaunchKernelGGL(mlm_disp_kernel, dim3((unsigned)n), dim3(256), 0, s, k);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      return mlm_launch_aux<7>(pl, k, s);
    }
    return h.lik == 0 ? mlm_launch_aux<5>(pl, k, s) : mlm_launch_aux<6>(pl, k, s);
  }
  const bool g = grad != nullptr;
  if (h.lik == 0)
    g ? mlm_launch<0, true>(pl, k, s) : mlm_launch<0, false>(pl, k, s);
  else if (h.lik == 1)
    g ? mlm_launch<1, true>(pl, k, s) : mlm_launch<1, false>(pl, k, s);
  else if (h.lik == 2)
    g ? mlm_launch<2, true>(pl, k, s) : mlm_launch<2, false>(pl, k, s);
  else if (h.lik == 3)
    g ? mlm_launch<3, true>(pl, k, s) : mlm_launch<3, false>(pl, k, s);
  else
    g ? mlm_launch<4, true>(pl, k, s) : mlm_launch<4, false>(pl, k, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (g)
    hipLaunchKernelGGL(mlm_combine_kernel<true>, dim3((unsigned)n), dim3(64), 0, s, k);
  else
    hipLaunchKernelGGL(mlm_combine_kernel<false>, dim3((unsigned)n), dim3(64), 0, s, k);
  return hipGetLastError();
}

}  // namespace vbk
