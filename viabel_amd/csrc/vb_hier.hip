// vb_hier.hip — hierarchical normal means on the device (VB_TARGET_HIERARCHICAL).
//
// J groups with data y_j, sigma_j; unconstrained coordinates x = [mu, u = log tau,
// then J more], D = J + 2.  Stan's log_prob convention (constants of the ~ statements
// dropped, the Jacobian term +u kept), as EightSchools in vb_device.hpp:
//
//   common        -(mu / s_mu)^2 / 2 - log1p(w) + u,  tau = exp(u), w = (tau / s_tau)^2
//   non-centred   - sum th_j^2 / 2 - sum r_j^2 / 2,   r_j = (y_j - mu - tau th_j) / sigma_j
//   centred       - J u - sum z_j^2 / 2 - sum r_j^2 / 2,
//                 z_j = (th_j - mu) / tau,            r_j = (y_j - th_j) / sigma_j
//
// for the n sample rows of x [n][D], with the gradient [n][D] when asked for.  All
// arithmetic is fp64.  Divisions by sigma_j are multiplications by rcp_refined(sigma_j)
// (correctly rounded 1 / sigma_j), formed per lane; the division by tau is one refined
// reciprocal per row.  tau is computed once per row.
//
// Three shapes of kernel, chosen by D alone, so a row's bits depend neither on n nor
// on the rows that accompany it; no atomics, every sum in a fixed order:
//
//   D <= 16 (kBlockDMax; hier_rows_lane_kernel): one lane per sample row.  mu, u,
//     the row and its gradient stay in registers; y_j and sigma_j are read at
//     compile-time offsets from the kernel argument, as wave-uniform values.
//     The sums run over j in order; the common part is added to them last.
//   16 < D < 512 (hier_rows_wave_kernel<.., 1>): one wave per sample row, four rows
//     per block.  Lane l takes j = l, l + 64, ... with coalesced 8-byte loads of the
//     row, y and sigma; the three row sums (log p, d mu, d u) are accumulated per
//     lane in j order and combined by wave_sum_dpp.  Lane 0 stores logp, g[0], g[1].
//   D >= 512 (kHierBlockD, where the separable row kernels switch too;
//     hier_rows_wave_kernel<.., 4>): one block of four waves per sample row, thread
//     t taking j = t, t + 256, ...; each wave's wave_sum_dpp total goes through LDS
//     and thread 0 adds the four in wave order.
//
// A row is never split over blocks.  grad == nullptr selects instances without any
// gradient operation or store (log weights).
#include "../../include/viabel_amd.h"
#include "vb_device.hpp"
#include "vb_internal.hpp"

using namespace vbd;

namespace vbk {
namespace {

constexpr int kHierLaneJMax = kBlockDMax - 2;  // lane-per-row kernel: J <= 14
constexpr int kHierBlockD = 512;               // block-per-row kernel from this D

struct HierK {
  int J, D;
  long long n;
  double inv_smu, inv_stau;  // 1 / mu_scale, 1 / tau_scale
  const double* y;           // [J]
  const double* sigma;       // [J]
  const double* x;           // [n][D]
  double* logp;              // [n]
  double* grad;              // [n][D] or null
};

// The part of log p and of the mu and u gradients that does not run over j (the
// helpers and the guard at w = inf as EightSchools::row_half).
template <bool CENTERED, bool GRAD>
__device__ __forceinline__ void hier_common(const HierK& k, double mu, double u, double tau,
                                            double& lp, double& gmu, double& gu) {
  const double t5 = tau * k.inv_stau, m5 = mu * k.inv_smu;
  const double w = t5 * t5;
  const double l1 = w < INFINITY ? log1p_pos_fast(w) : w;
  lp = -0.5 * m5 * m5 - l1 + u;
  if constexpr (CENTERED) lp -= (double)k.J * u;
  if constexpr (GRAD) {
    const double rw = rcp_refined(1.0 + w);
    gmu = -m5 * k.inv_smu;
    gu = -2.0 * w * rw + 1.0;
    if constexpr (CENTERED) gu -= (double)k.J;
  }
}

// Group j's terms added to the three sums; returns d log p / d th_j.  is = 1 / sigma_j,
// it = 1 / tau (centred form only).
template <bool CENTERED, bool GRAD>
__device__ __forceinline__ double hier_term(double mu, double tau, double it, double th,
                                            double yj, double is, double& lp, double& gmu,
                                            double& gu) {
  if constexpr (CENTERED) {
    const double z = (th - mu) * it;
    const double r = (yj - th) * is;
    lp += -0.5 * z * z - 0.5 * r * r;
    if constexpr (GRAD) {
      const double zt = z * it;
      gmu += zt;
      gu += z * z;
      return -zt + r * is;
    }
  } else {
    const double tt = tau * th;
    const double r = (yj - mu - tt) * is;
    lp += -0.5 * th * th - 0.5 * r * r;
    if constexpr (GRAD) {
      const double rs = r * is;
      gmu += rs;
      gu += rs * tt;
      return -th + rs * tau;
    }
  }
  return 0.0;
}

// ---- D <= 16: one lane per sample row --------------------------------------------
// JP: compile-time bound of J (the loops unroll; j < J is wave-uniform).  Indices are
// clamped to J - 1, so every load is in bounds and none sits behind a branch.
template <bool CENTERED, bool GRAD, int JP>
__global__ __launch_bounds__(64) void hier_rows_lane_kernel(HierK k) {
  const long long row = (long long)blockIdx.x * 64 + threadIdx.x;
  if (row >= k.n) return;
  const int J = k.J;
  const double* xr = k.x + row * k.D;
  const double mu = xr[0], u = xr[1];
  double th[JP], yj[JP], is[JP];
#pragma unroll
  for (int j = 0; j < JP; ++j) {
    const int jj = j < J ? j : J - 1;
    th[j] = xr[2 + jj];
    yj[j] = k.y[jj];
    is[j] = rcp_refined(k.sigma[jj]);
  }
  const double tau = exp_fast(u);
  const double it = CENTERED ? rcp_refined(tau) : 0.0;
  // the sums over j first, the common part added to them at the end, as the wave kernel
  // does: added into -mu / s_mu^2 one by one, small z_j / tau of one sign each lose up
  // to half an ulp of that term (12 units of 2^-53 S at J = 14, log tau = 20)
  double lp = 0.0, gmu = 0.0, gu = 0.0;
  double g[JP] = {};
#pragma unroll
  for (int j = 0; j < JP; ++j)
    if (j < J) g[j] = hier_term<CENTERED, GRAD>(mu, tau, it, th[j], yj[j], is[j], lp, gmu, gu);
  double clp, cgmu = 0.0, cgu = 0.0;
  hier_common<CENTERED, GRAD>(k, mu, u, tau, clp, cgmu, cgu);
  k.logp[row] = clp + lp;
  if constexpr (GRAD) {
    double* gr = k.grad + row * k.D;
    gr[0] = cgmu + gmu;
    gr[1] = cgu + gu;
#pragma unroll
    for (int j = 0; j < JP; ++j)
      if (j < J) gr[2 + j] = g[j];
  }
}

// ---- D > 16: WPR waves per sample row ----------------------------------------------
// WPR == 1: four rows per 256-thread block, one per wave; WPR == 4: one row per block.
template <bool CENTERED, bool GRAD, int WPR>
__global__ __launch_bounds__(256) void hier_rows_wave_kernel(HierK k) {
  static_assert(WPR == 1 || WPR == 4, "one wave or the whole block per row");
  __shared__ double part[WPR == 1 ? 1 : 3 * WPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = WPR == 1 ? (long long)blockIdx.x * 4 + wave : (long long)blockIdx.x;
  // (a whole wave leaves; the one-wave-per-row form has no barrier)
  if (WPR == 1 && row >= k.n) return;
  const int J = k.J;
  constexpr int S = 64 * WPR;   // stride of a thread's j
  const int t = WPR == 1 ? lane : (int)threadIdx.x;
  const double* xr = k.x + row * k.D;
  const double* xt = xr + 2;
  double* gt = GRAD ? k.grad + row * k.D + 2 : nullptr;
  const double mu = xr[0], u = xr[1];
  const double tau = exp_fast(u);
  const double it = CENTERED ? rcp_refined(tau) : 0.0;
  double lp = 0.0, gmu = 0.0, gu = 0.0;
  int j = t;
  // four groups per round: twelve independent loads in flight, the sums still in j order
  for (; j + 3 * S < J; j += 4 * S) {
    double th[4], yj[4], sj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      th[q] = xt[j + q * S];
      yj[q] = k.y[j + q * S];
      sj[q] = k.sigma[j + q * S];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double g = hier_term<CENTERED, GRAD>(mu, tau, it, th[q], yj[q], rcp_refined(sj[q]),
                                                 lp, gmu, gu);
      if constexpr (GRAD) gt[j + q * S] = g;
    }
  }
  for (; j < J; j += S) {
    const double g = hier_term<CENTERED, GRAD>(mu, tau, it, xt[j], k.y[j], rcp_refined(k.sigma[j]),
                                               lp, gmu, gu);
    if constexpr (GRAD) gt[j] = g;
  }
  lp = wave_sum_dpp(lp);
  if constexpr (GRAD) {
    gmu = wave_sum_dpp(gmu);
    gu = wave_sum_dpp(gu);
  }
  if constexpr (WPR > 1) {
    if (lane == 0) {
      part[3 * wave] = lp;
      part[3 * wave + 1] = gmu;
      part[3 * wave + 2] = gu;
    }
    __syncthreads();
    if (t == 0) {
      lp = part[0];
      gmu = part[1];
      gu = part[2];
#pragma unroll
      for (int v = 1; v < WPR; ++v) {   // wave order
        lp += part[3 * v];
        gmu += part[3 * v + 1];
        gu += part[3 * v + 2];
      }
    }
  }
  if (t == 0) {
    double clp, cgmu = 0.0, cgu = 0.0;
    hier_common<CENTERED, GRAD>(k, mu, u, tau, clp, cgmu, cgu);
    k.logp[row] = clp + lp;
    if constexpr (GRAD) {
      double* gr = k.grad + row * k.D;
      gr[0] = cgmu + gmu;
      gr[1] = cgu + gu;
    }
  }
}

template <bool CENTERED, bool GRAD>
hipError_t hier_launch(const HierK& k, hipStream_t s) {
  const long long n = k.n;
  if (k.J <= kHierLaneJMax) {
    const long long nb = (n + 63) / 64;
    if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 g((unsigned)nb), b(64);
    if (k.J <= 4)
      hipLaunchKernelGGL((hier_rows_lane_kernel<CENTERED, GRAD, 4>), g, b, 0, s, k);
    else if (k.J <= 8)
      hipLaunchKernelGGL((hier_rows_lane_kernel<CENTERED, GRAD, 8>), g, b, 0, s, k);
    else
      hipLaunchKernelGGL((hier_rows_lane_kernel<CENTERED, GRAD, kHierLaneJMax>), g, b, 0, s, k);
  } else if (k.D < kHierBlockD) {
    const long long nb = (n + 3) / 4;
    if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((hier_rows_wave_kernel<CENTERED, GRAD, 1>), dim3((unsigned)nb), dim3(256), 0,
                       s, k);
  } else {
    if (n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((hier_rows_wave_kernel<CENTERED, GRAD, 4>), dim3((unsigned)n), dim3(256), 0,
                       s, k);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_hier_rows(int D, long long n, const HierHead& h, const double* params,
                            const double* x, double* logp, double* grad, hipStream_t s) {
  if (n < 1) return hipSuccess;
  if (!params || !x || !logp || h.J < 1 || h.J > 0x7fff0000LL || D != (int)h.J + 2)
    return hipErrorInvalidValue;
  HierK k{};
  k.J = (int)h.J;
  k.D = D;
  k.n = n;
  k.inv_smu = 1.0 / h.mu_scale;
  k.inv_stau = 1.0 / h.tau_scale;
  k.y = params + kHierHeader;
  k.sigma = k.y + h.J;
  k.x = x;
  k.logp = logp;
  k.grad = grad;
  if (h.centered)
    return grad ? hier_launch<true, true>(k, s) : hier_launch<true, false>(k, s);
  return grad ? hier_launch<false, true>(k, s) : hier_launch<false, false>(k, s);
}

}  // namespace vbk
