// vb_links.hpp — the observation likelihoods of the regression targets, defined once for
// vb_glm.hip (VB_TARGET_REGRESSION) and vb_mlm.hip (VB_TARGET_MULTILEVEL):
//
//   0 gaussian, 1 student_t, 2 bernoulli_logit, 3 poisson_log, 4 neg_binomial_2_log
//
// The host part (LinkK, link_has_offset, lgamma_half_step, link_consts) is plain C++ with
// no HIP runtime call, so a host-only program can include it; the device part (obs_link)
// is compiled by hipcc only.  The forms with a learned scale or dispersion have one user
// and stay in vb_glm.hip.
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
#endif  // __HIPCC__

}  // namespace vbk
