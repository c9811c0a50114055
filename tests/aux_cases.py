"""Plain numpy restatement of the regression target with a learned scale or dispersion
(targets.regression(..., learn_scale=True) / (..., learn_phi=True)), every normalising
constant and the Jacobian kept, and seeded data makers; shared by the host and device
tests.  In the manner of tests/glm_cases.py and tests/count_cases.py, whose likelihoods
these are.

  z = [beta (p), lambda],  eta_m = x_m . beta (+ eta0_m for the negative binomial)
  beta_d ~ N(0, s^2);  theta = e^lambda ~ half-Cauchy(0, s_aux), in lambda with
  w = 2 (lambda - log s_aux):
      log p(lambda) = log(2 / (pi s_aux)) - softplus(w) + lambda,   d/dlambda = 1 - 2 logistic(w)
  gaussian    sigma = e^lambda, q = (y - eta) / sigma:
      l = -lambda - q^2 / 2 - log(2 pi) / 2;   dl/deta = q / sigma;   dl/dlambda = -1 + q^2
  student_t   l = -lambda - (nu + 1)/2 log1p(q^2 / nu) + c_nu,
      c_nu = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2
      t = (nu + 1) q / (nu + q^2):   dl/deta = t / sigma;   dl/dlambda = -1 + t q
  neg_binomial_2_log   phi = e^lambda, zeta = eta - lambda:
      l = y eta - (y + phi) softplus(zeta) + sum_{j<y} log1p(j / phi) - lgamma(y + 1)
      dl/deta = y - (y + phi) logistic(zeta)
      dl/dlambda = (y + phi) logistic(zeta) - phi softplus(zeta) - sum_{j<y} j / (phi + j)
  softplus(z) = max(z, 0) + log1p(exp(-|z|)), the logistic from the same exp.

The residual is scaled by 1 / sigma before it is squared, so a residual of exactly 0
gives exactly 0 at any lambda.  The negative binomial's sum over j is taken over the
table T[j] = #{m : y_m > j} (dispersion_table), as the device takes it.
"""
import math

import numpy as np

from tests import count_cases as cc
from tests import glm_cases as gc

LIKELIHOODS = ('gaussian', 'student_t', 'neg_binomial_2_log')
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def dispersion_table(y):
    """(T [J], sum_m -lgamma(y_m + 1)) by brute force: T[j] = #{m : y_m > j}, J = max y."""
    y = np.asarray(y, dtype=float)
    J = int(y.max()) if y.size else 0
    T = np.array([float(np.sum(y > j)) for j in range(J)])
    return T, math.fsum(-math.lgamma(v + 1.0) for v in y.tolist())


def _softplus_logistic(w):
    e = np.exp(-np.abs(w))
    return np.maximum(w, 0.0) + np.log1p(e), np.where(w >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def restatement(x, y, likelihood='gaussian', df=None, offset=None, prior_scale=10.0,
                hyper_scale=5.0):
    """f(z [n][p + 1]) -> (log p [n], d log p / dz [n][p + 1])."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    assert likelihood in LIKELIHOODS
    M, p = x.shape
    nb = likelihood == 'neg_binomial_2_log'
    eta0 = np.zeros(M) if offset is None else np.asarray(offset, dtype=float)
    if nb:
        T, c_data = dispersion_table(y)
        js = np.arange(T.size, dtype=float)
    c_nu = gc.lgamma_half_step(0.5 * df) - HALF_LOG_2PI if likelihood == 'student_t' else 0.0
    c_aux = math.log(2.0 / math.pi) - math.log(hyper_scale)

    def f(z):
        z = np.atleast_2d(np.asarray(z, dtype=float))
        assert z.shape[1] == p + 1
        b, lam = z[:, :p], z[:, p]
        eta = b @ x.T
        sp, lg = _softplus_logistic(2.0 * (lam - math.log(hyper_scale)))
        lp = (np.sum(-0.5 * (b / prior_scale) ** 2, axis=1)
              - p * (HALF_LOG_2PI + math.log(prior_scale)))
        prior = c_aux - sp + lam
        gl = 1.0 - 2.0 * lg
        if nb:
            eta = eta + eta0[None, :]
            phi = np.exp(lam)[:, None]
            s2, l2 = _softplus_logistic(eta - lam[:, None])
            yp = y[None, :] + phi
            l = y[None, :] * eta - yp * s2
            dl = y[None, :] - yp * l2
            with np.errstate(over='ignore'):
                A = np.sum(T[None, 1:] * np.log1p(js[None, 1:] / phi), axis=1)
                dA = -np.sum(T[None, 1:] * (js[None, 1:] / (phi + js[None, 1:])), axis=1)
            lp = lp + np.sum(l, axis=1) + c_data + A + prior
            gl = gl + np.sum(yp * l2 - phi * s2, axis=1) + dA
        else:
            ca = np.exp(-lam)[:, None]
            q = (y[None, :] - eta) * ca
            if likelihood == 'gaussian':
                l = -0.5 * q * q
                t = q
                c_obs = -HALF_LOG_2PI
            else:
                l = -0.5 * (df + 1) * np.log1p(q * q / df)
                t = (df + 1) * q / (df + q * q)
                c_obs = c_nu
            dl = t * ca
            lp = lp + np.sum(l, axis=1) + M * c_obs - M * lam + prior
            gl = gl + np.sum(t * q, axis=1) - M
        gb = -b / prior_scale ** 2 + dl @ x
        return lp, np.concatenate([gb, gl[:, None]], axis=1)
    return f


def make_data(p, M, likelihood, seed=0, df=5.0, scale=0.7, phi=3.0):
    """(x [M][p], y [M], offset [M] or None) drawn from the model at a seeded beta."""
    if likelihood == 'neg_binomial_2_log':
        return cc.make_data(p, M, likelihood, seed=seed, phi=phi)
    x, y = gc.make_data(p, M, likelihood, seed=seed, df=df, scale=scale)
    return x, y, None


def model_kwargs(likelihood, df=5.0, prior_scale=3.0, hyper_scale=2.0):
    """The keyword arguments shared by restatement and (with the learn flag of
    target_kwargs) targets.regression."""
    kw = dict(likelihood=likelihood, prior_scale=prior_scale, hyper_scale=hyper_scale)
    if likelihood == 'student_t':
        kw['df'] = df
    return kw


def target_kwargs(kw):
    """kw with the learn flag that targets.regression needs for its likelihood."""
    out = dict(kw)
    out['learn_phi' if kw['likelihood'] == 'neg_binomial_2_log' else 'learn_scale'] = True
    return out


def start_rows(rs, n, p, likelihood, spread=0.3):
    """n rows [beta, lambda] near a plausible fit: beta ~ spread randn, lambda near log of
    the data makers' scale / dispersion."""
    z = rs.randn(n, p + 1) * spread
    z[:, p] += math.log(3.0) if likelihood == 'neg_binomial_2_log' else math.log(0.7)
    return z
