"""Plain numpy restatement of the regression targets (targets.regression) with
every normalising constant, and a seeded data generator; shared by the host and
device tests.

  log p(beta) = sum_d log N(beta_d; 0, s^2) + sum_m l(y_m, x_m . beta)
  gaussian         l = log N(y; eta, sigma^2)
  student_t        l = log t_nu(y; eta, sigma)
  bernoulli_logit  l = y eta - softplus(eta)
"""
import math

import numpy as np

try:
    from scipy import stats as _stats
except Exception:                       # scipy is optional: the formulas are written out below
    _stats = None

LIKELIHOODS = ('gaussian', 'student_t', 'bernoulli_logit')


def _norm_logpdf(y, loc, scale):
    if _stats is not None:
        return _stats.norm.logpdf(y, loc=loc, scale=scale)
    r = (y - loc) / scale
    return -0.5 * r * r - math.log(scale) - 0.5 * math.log(2 * math.pi)


def lgamma_half_step(x):
    """lgamma(x + 1/2) - lgamma(x) - log(x) / 2 for x > 0, to a few 2^-53 absolute at
    any x (the difference of the two lgamma loses log p's digits as x grows: ~1e-9
    absolute at x = 5e5).  From x >= 32 the asymptotic series -1/(8x) + 1/(192 x^3) -
    1/(640 x^5) + 17/(14336 x^7) - 31/(18432 x^9) + 691/(180224 x^11) (next term
    below 4e-22); a smaller x climbs there by Gamma(x + 1) = x Gamma(x); below 1 the
    two lgamma are small and their difference is taken as it stands."""
    if x < 1.0:
        return math.lgamma(x + 0.5) - math.lgamma(x) - 0.5 * math.log(x)
    x0, steps = x, 0.0
    while x < 32.0:
        steps += math.log1p(0.5 / x)
        x += 1.0
    t = 1.0 / x
    t2 = t * t
    tail = t * (-1.0 / 8 + t2 * (1.0 / 192 + t2 * (-1.0 / 640 + t2 * (
        17.0 / 14336 + t2 * (-31.0 / 18432 + t2 * (691.0 / 180224))))))
    return tail if x == x0 else tail + (0.5 * math.log(x / x0) - steps)


def _t_logpdf(y, df, loc, scale):
    if _stats is not None:
        return _stats.t.logpdf(y, df, loc=loc, scale=scale)
    r = (y - loc) / scale
    # lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2, the log(df / 2) / 2 cancelled
    c = lgamma_half_step(0.5 * df) - 0.5 * math.log(2 * math.pi)
    return c - math.log(scale) - 0.5 * (df + 1) * np.log1p(r * r / df)


def restatement(x, y, likelihood='student_t', df=None, scale=1.0, prior_scale=10.0):
    """f(beta [n][D]) -> (log p [n], d log p / d beta [n][D])."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    assert likelihood in LIKELIHOODS

    def f(b):
        b = np.atleast_2d(np.asarray(b, dtype=float))
        eta = b @ x.T                                     # [n][M]
        lp = np.sum(_norm_logpdf(b, 0.0, prior_scale), axis=1)
        if likelihood == 'gaussian':
            r = y[None, :] - eta
            lp = lp + np.sum(_norm_logpdf(y[None, :], eta, scale), axis=1)
            dl = r / scale ** 2
        elif likelihood == 'student_t':
            r = y[None, :] - eta
            lp = lp + np.sum(_t_logpdf(y[None, :], df, eta, scale), axis=1)
            dl = (df + 1) * r / (df * scale ** 2 + r ** 2)
        else:
            e = np.exp(-np.abs(eta))
            lp = lp + np.sum(y[None, :] * eta - (np.maximum(eta, 0.0) + np.log1p(e)), axis=1)
            dl = y[None, :] - np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return lp, -b / prior_scale ** 2 + dl @ x
    return f


def make_data(D, M, likelihood, seed=0, df=5.0, scale=0.7):
    """x [M][D], y [M] drawn from the model at a seeded beta (a private RandomState)."""
    rs = np.random.RandomState(1000 * seed + 17 * D + M)
    x = rs.randn(M, D)
    beta = rs.randn(D) / math.sqrt(D)
    eta = x @ beta
    if likelihood == 'gaussian':
        y = eta + scale * rs.randn(M)
    elif likelihood == 'student_t':
        y = eta + scale * rs.standard_t(df, M)
    else:
        y = (rs.rand(M) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return x, y


def model_kwargs(likelihood, df=5.0, scale=0.7, prior_scale=3.0):
    """The keyword arguments shared by targets.regression and restatement."""
    kw = dict(likelihood=likelihood, prior_scale=prior_scale)
    if likelihood == 'student_t':
        kw['df'] = df
    if likelihood != 'bernoulli_logit':
        kw['scale'] = scale
    return kw
