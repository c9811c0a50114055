// banana.hip — a twisted Gaussian ("banana", Haario et al. 1999) as a device model plugin
// (VB_MODEL_ROWS of include/viabel_amd_model.h); no built-in target provides it.
//   x_1 ~ N(0, s^2),  x_2 + b x_1^2 - s^2 b ~ N(0, 1),  x_d ~ N(0, 1) for d >= 3
// (the map has unit Jacobian), constants dropped:
//   log p(x) = -x_1^2 / (2 s^2) - t^2 / 2 - 1/2 sum_{d >= 3} x_d^2,  t = x_2 + b x_1^2 - s^2 b
//   d/dx_1 = -x_1 / s^2 - 2 b x_1 t,  d/dx_2 = -t,  d/dx_d = -x_d
// D = 1 keeps the first factor only.  data = [s, b]; without a data block s = 10, b = 0.03.
#include "viabel_amd_model.h"

static __device__ double banana(const double* x, int D, const double* data, long long n_data,
                                double* grad) {
  const double s = n_data >= 2 ? data[0] : 10.0, b = n_data >= 2 ? data[1] : 0.03;
  const double x1 = x[0], s2 = s * s;
  double lp = -0.5 * x1 * x1 / s2;
  double g1 = -x1 / s2;
  if (D >= 2) {
    const double t = x[1] + b * x1 * x1 - s2 * b;
    lp -= 0.5 * t * t;
    g1 -= 2.0 * b * x1 * t;
    if (grad) grad[1] = -t;
  }
  if (grad) grad[0] = g1;
  for (int d = 2; d < D; ++d) {
    lp -= 0.5 * x[d] * x[d];
    if (grad) grad[d] = -x[d];
  }
  return lp;
}

VB_MODEL_ROWS(vb_model, banana)
