// robust_regression.hip — the robust-regression notebook's Stan model as a device model
// plugin (VB_MODEL_SUM of include/viabel_amd_model.h):
//   beta ~ normal(0, 10);  y_m ~ student_t(nu, x_m . beta, 1)
// up to the constants Stan's `~` drops:
//   log p(beta) = -1/2 sum_d (beta_d / 10)^2 - (nu + 1)/2 sum_m log1p(r_m^2 / nu),
//   r_m = y_m - x_m . beta
//   d log p / d beta = -beta / 100 + sum_m (nu + 1) r_m / (nu + r_m^2) x_m
// data = [M, nu, X [M][D] row-major, y [M]]  (targets.example_model packs it); D <= 32.
#include "viabel_amd_model.h"

#define RR_DMAX 32

static __device__ __forceinline__ double rr_prior(const double* b, int D, const double* data,
                                                  double* g) {
  double ss = 0.0;
#pragma unroll
  for (int d = 0; d < RR_DMAX; ++d)
    if (d < D) {
      const double bd = b[d];
      ss += (bd / 10.0) * (bd / 10.0);
      g[d] -= bd / 100.0;
    }
  return -0.5 * ss;
}

static __device__ __forceinline__ double rr_term(const double* b, int D, const double* data,
                                                 long long m, double* g) {
  const long long M = (long long)data[0];
  const double nu = data[1];
  const double* xm = data + 2 + m * D;
  double xr[RR_DMAX];
  double eta = 0.0;
#pragma unroll
  for (int d = 0; d < RR_DMAX; ++d) {
    xr[d] = d < D ? xm[d] : 0.0;
    if (d < D) eta += xr[d] * b[d];
  }
  const double r = data[2 + M * D + m] - eta;
  const double w = (nu + 1.0) * r / (nu + r * r);
#pragma unroll
  for (int d = 0; d < RR_DMAX; ++d)
    if (d < D) g[d] += w * xr[d];
  return -0.5 * (nu + 1.0) * log1p(r * r / nu);
}

VB_MODEL_SUM(vb_model, RR_DMAX, rr_prior, rr_term)
