// vb_links.hpp — the observation likelihoods of the regression targets, defined once for
// vb_glm.hip (VB_TARGET_REGRESSION) and vb_mlm.hip (VB_TARGET_MULTILEVEL):
//
//   0 gaussian, 1 student_t, 2 bernoulli_logit, 3 poisson_log, 4 neg_binomial_2_log
//
// The host part (LinkK, link_has_offset, lgamma_half_step, link_consts) is plain C++ with
// no HIP runtime call, so a host-only program can include it; the device part (obs_link)
// is compiled by hipcc only.
//
// The forms with a learned scale or dispersion (the last coordinate of a sample row is
// lambda = log sigma for 0 and 1, log phi for 4) are the kernel instances LIK = 5, 6, 7 of
// both files: aux_consts on the host; glm_row_consts, glm_link_aux, aux_lambda_prior and
// disp_row_sums on the device.
#pragma once
#include <cmath>

namespace vbk {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;

// The constants of l(y, eta) that a kernel carries in its argument block:
//   gaussian            k0 = 1 / sigma^2
//   student_t           k0 = 1 / (nu sigma^2), k1 = (nu + 1) / 2, k2 = nu + 1, k3 = nu sigma^2
//   neg_binomial_2_log  k0 = phi, k1 = log phi
// (zero where a likelihood has none).
struct LinkK {
  double k0, k1, k2, k3;
};

// the two count likelihoods add the block's per-observation offset eta0 [M] to eta
constexpr bool link_has_offset(int lik) { return lik == 3 || lik == 4; }

// the learned instances of the kernels: LIK = 5, 6, 7 are the likelihoods 0, 1, 4 with
// lambda a coordinate; 7 takes the offset as 4 does
constexpr bool link_learned(int lik) { return lik >= 5; }
constexpr bool link_offset(int lik) { return link_has_offset(lik) || lik == 7; }

// lgamma(x + 1/2) - lgamma(x) - log(x) / 2 for x > 0, to a few 2^-53 absolute.  The
// difference of the two lgamma loses the digits of M c_obs as nu grows (~1e-9 per
// observation at nu = 1e6).  From x >= 32 the asymptotic series (next term < 4e-22); a
// smaller x climbs there by Gamma(x + 1) = x Gamma(x); below 1 the two lgamma are small
// and their difference is taken as it stands.
inline double lgamma_half_step(double x) {
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

// Fills *k for likelihood `lik` and returns c_obs, the constant of one observation's
// log density that does not depend on the data (the count likelihoods' data-only
// constants are summed by the packer).  nu is read by 1, sigma by 0 and 1, phi by 4.
inline double link_consts(int lik, double nu, double sigma, double phi, LinkK* k) {
  *k = LinkK{};
  if (lik == 0) {
    k->k0 = 1.0 / (sigma * sigma);
    return -0.5 * kLog2Pi - std::log(sigma);
  }
  if (lik == 1) {
    k->k3 = nu * (sigma * sigma);
    k->k0 = 1.0 / k->k3;
    k->k1 = 0.5 * (nu + 1.0);
    k->k2 = nu + 1.0;
    // lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2, the log(nu / 2) / 2 cancelled
    return lgamma_half_step(0.5 * nu) - 0.5 * kLog2Pi - std::log(sigma);
  }
  if (lik == 4) {
    k->k0 = phi;
    k->k1 = std::log(phi);
  }
  return 0.0;
}

// log(2 / pi): the half-Cauchy's constant without its scale
constexpr double kLogTwoOverPi = -0.45158270528945486472619522989488;

// The host constants of a learned block (likelihood 0, 1 or 4; e^lambda ~ half-Cauchy(0,
// s_aux)): the fixed link's constants at sigma = 1, that is c_obs without -log sigma
// (-M lambda is the row's) and the student_t's k1, k2; not its k0, k3, which hold sigma,
// and nothing of the negative binomial's, whose phi and log phi are the row's.  c_aux =
// log(2 / (pi s_aux)).
struct AuxConsts {
  double c_obs, k1, k2, nu, inv_nu, ls_aux, c_aux;
};
inline AuxConsts aux_consts(int lik, double nu, double s_aux) {
  AuxConsts a{};
  if (lik != 4) {
    LinkK fixed;
    a.c_obs = link_consts(lik, nu, 1.0, 0.0, &fixed);
    a.k1 = fixed.k1;
    a.k2 = fixed.k2;
  }
  if (lik == 1) {
    a.nu = nu;
    a.inv_nu = 1.0 / nu;
  }
  a.ls_aux = std::log(s_aux);
  a.c_aux = kLogTwoOverPi - a.ls_aux;
  return a;
}

#ifdef __HIPCC__
// l(y, eta) without its constant, and dl / d eta
template <int LIK>
__device__ __forceinline__ void obs_link(const LinkK& k, double eta, double y, double& l,
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

// learned mode: a row's link constants from its lambda.  gaussian, student_t: ca =
// 1 / sigma = exp(-lambda) (the residual is scaled before it is squared, so a residual of
// exactly 0 stays 0 where sigma^2 leaves the range); neg_binomial: ca = phi, cb = lambda
template <int LIK>
__device__ __forceinline__ void glm_row_consts(double lam, double& ca, double& cb) {
  if constexpr (LIK == 7) {
    ca = exp(lam);
    cb = lam;
  } else {
    ca = exp(-lam);
    cb = 0.0;
  }
}

// l(y, eta) without its constant and without -lambda, dl / d eta, and the observation's
// share of dl / d lambda without its -1 (LIK 5: not formed, -M - 2 sum l serves).  K is
// the kernel's argument block: lk.k1, lk.k2, nu and inv_nu are read (student_t)
template <int LIK, class K>
__device__ __forceinline__ void glm_link_aux(const K& k, double ca, double cb, double eta,
                                             double y, double& l, double& dl, double& dlam) {
  if constexpr (LIK == 5) {          // q = r / sigma
    const double q = (y - eta) * ca;
    l = -0.5 * (q * q);
    dl = q * ca;
    dlam = 0.0;
  } else if constexpr (LIK == 6) {   // t = (nu + 1) q / (nu + q^2): dl = t / sigma, dlam = t q
    const double q = (y - eta) * ca;
    const double q2 = q * q;
    l = -k.lk.k1 * log1p(q2 * k.inv_nu);
    const double t = k.lk.k2 * q / (k.nu + q2);
    dl = t * ca;
    dlam = t * q;
  } else {                           // phi = ca, zeta = eta - lambda
    const double z = eta - cb;
    const double e = exp(-fabs(z));
    const double yp = y + ca;
    const double sp = fmax(z, 0.0) + log1p(e);
    l = y * eta - yp * sp;
    const double inv = 1.0 / (1.0 + e);
    const double lg = yp * (z >= 0.0 ? inv : e * inv);
    dl = y - lg;
    dlam = lg - ca * sp;             // (y - dl) - phi softplus(zeta)
  }
}

// The half-Cauchy prior of e^lambda with its Jacobian, without its constant: sp =
// softplus(w) and lg = logistic(w) of w = 2 (lambda - log s_aux), from one exp;
// log p(lambda) = log(2 / (pi s_aux)) - sp + lambda, d / dlambda = 1 - 2 lg
__device__ __forceinline__ void aux_lambda_prior(double lam, double ls_aux, double& sp, double& lg) {
  const double w = 2.0 * (lam - ls_aux);
  const double e = exp(-fabs(w));
  sp = fmax(w, 0.0) + log1p(e);
  const double inv = 1.0 / (1.0 + e);
  lg = w >= 0.0 ? inv : e * inv;
}

// learned dispersion: A(phi) = sum_{j=1}^{J-1} T_j log1p(j / phi) -> out[row] and
// dA / dlambda = -sum_j T_j j / (phi + j) -> out[n + row] of the sample row blockIdx.x,
// whose lambda is x[row * stride + col], phi = exp(lambda) as the row kernels form it.  One
// 256-thread block per row.  Every term has one sign.  Threads stride over j; the partial
// sums meet by the wave reduction and then in wave order: the same bits every call.
__device__ __forceinline__ void disp_row_sums(const double* x, int stride, int col, const double* T,
                                              long long J, double* out, long long n) {
  __shared__ double red[8];
  const long long row = blockIdx.x;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const double phi = exp(x[row * stride + col]);
  double a = 0.0, da = 0.0;
  for (long long j = 1 + t; j < J; j += 256) {
    const double tj = T[j], fj = (double)j;
    a = fma(tj, log1p(fj / phi), a);
    da = fma(tj, fj / (phi + fj), da);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    da += __shfl_xor(da, off, 64);
  }
  if (lane == 0) {
    red[w] = a;
    red[4 + w] = da;
  }
  __syncthreads();
  if (t == 0) {
    out[row] = ((red[0] + red[1]) + red[2]) + red[3];
    out[n + row] = -(((red[4] + red[5]) + red[6]) + red[7]);
  }
}
#endif  // __HIPCC__

}  // namespace vbk
