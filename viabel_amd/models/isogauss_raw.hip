// isogauss_raw.hip — the raw plugin contract without viabel_amd_model.h: a kernel with the
// seven arguments and its own launch record (include/viabel_amd.h, "Device model plugins").
//   log p(x) = sum_d -x_d^2 / 2 - D/2 log(2 pi),  d log p / dx = -x
// The library launches ceil(n / rows_per_block) blocks of `block` threads; here one lane
// per row in blocks of 128.
#include <hip/hip_runtime.h>

extern "C" __device__ __attribute__((used, visibility("default"))) const int vb_model_launch[3] = {
    128 /* block */, 128 /* rows_per_block */, 0 /* dmax: any dimension */};

extern "C" __global__ __launch_bounds__(128) void vb_model(const double* x, long long n, int D,
                                                           const double* data, long long n_data,
                                                           double* logp, double* grad) {
  const long long r = (long long)blockIdx.x * 128 + threadIdx.x;
  if (r >= n) return;   // rows past n: write nothing
  const double* xr = x + r * D;
  double ss = 0.0;
  for (int d = 0; d < D; ++d) {
    ss += xr[d] * xr[d];
    if (grad) grad[r * D + d] = -xr[d];   // grad is null for log-weight calls
  }
  logp[r] = -0.5 * ss - 0.5 * D * 1.8378770664093454836 /* log(2 pi) */;
}
