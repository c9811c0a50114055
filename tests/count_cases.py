"""Plain numpy restatement of the two count likelihoods for both data targets
(targets.regression and targets.multilevel_regression with 'poisson_log' and
'neg_binomial_2_log'), every normalising constant kept, and seeded data makers; shared
by the host and device tests.  In the manner of tests/glm_cases.py and
tests/mlm_cases.py, whose priors and coordinates these are.

  eta_m = x_m . beta + eta0_m  (+ a_group[m], or tau at_group[m], in the multilevel target)
  poisson_log         l = y eta - exp(eta)                       - lgamma(y + 1)
  neg_binomial_2_log  l = y eta - (y + phi) softplus(eta - log phi)
                          + lgamma(y + phi) - lgamma(phi) - y log(phi) - lgamma(y + 1)
  softplus(z) = max(z, 0) + log1p(exp(-|z|))
  l' = y - exp(eta),  y - (y + phi) logistic(eta - log phi)

The data-only constants are summed once (count_constant): the negative binomial's first
three as sum_{j<y} log1p(j / phi), each distinct y once, the sum over m by math.fsum.
Past exp's range (eta > 709.78) the Poisson value is -inf and its gradient whatever IEEE
gives.
"""
import math

import numpy as np

from tests import mlm_cases as mc

LIKELIHOODS = ('poisson_log', 'neg_binomial_2_log')
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def count_constant(y, likelihood, phi=None):
    """sum_m c_m of the docstring (y small enough to walk the product)."""
    y = np.asarray(y, dtype=float)
    vals, counts = np.unique(y, return_counts=True)
    terms = []
    for v, c in zip(vals.tolist(), counts.tolist()):
        cm = -math.lgamma(v + 1.0)
        if likelihood == 'neg_binomial_2_log' and v > 0:
            cm = math.fsum([math.fsum(np.log1p(np.arange(int(v)) / phi).tolist()), cm])
        terms += [cm] * c
    return math.fsum(terms)


def link(likelihood, eta, y, phi=None):
    """(l without its constant, l') at eta [n][M], y [M]."""
    if likelihood == 'poisson_log':
        with np.errstate(over='ignore'):
            e = np.exp(eta)
        return y[None, :] * eta - e, y[None, :] - e
    z = eta - math.log(phi)
    e = np.exp(-np.abs(z))
    yp = (y + phi)[None, :]
    l = y[None, :] * eta - yp * (np.maximum(z, 0.0) + np.log1p(e))
    return l, y[None, :] - yp * np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _offset(offset, M):
    return np.zeros(M) if offset is None else np.asarray(offset, dtype=float)


def restatement(x, y, likelihood='poisson_log', phi=None, offset=None, prior_scale=10.0):
    """targets.regression: f(beta [n][D]) -> (log p [n], d log p / d beta [n][D])."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    assert likelihood in LIKELIHOODS
    M, D = x.shape
    eta0 = _offset(offset, M)
    c_data = count_constant(y, likelihood, phi)

    def f(b):
        b = np.atleast_2d(np.asarray(b, dtype=float))
        eta = b @ x.T + eta0[None, :]
        l, dl = link(likelihood, eta, y, phi)
        with np.errstate(invalid='ignore'):
            lp = (np.sum(-0.5 * (b / prior_scale) ** 2, axis=1)
                  - D * (HALF_LOG_2PI + math.log(prior_scale))) + np.sum(l, axis=1) + c_data
            g = -b / prior_scale ** 2 + dl @ x
        return lp, g
    return f


def mlm_restatement(x, y, group, likelihood='poisson_log', phi=None, offset=None,
                    prior_scale=10.0, tau_scale=5.0, centered=False, n_groups=None):
    """targets.multilevel_regression: f(z [n][D]) -> (log p [n], d log p / dz [n][D]),
    D = p + 1 + G, the coordinates and priors of tests/mlm_cases.py."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    group = np.asarray(group).astype(np.int64)
    assert likelihood in LIKELIHOODS
    M, p = x.shape
    G = int(group.max()) + 1 if n_groups is None else int(n_groups)
    eta0 = _offset(offset, M)
    c_data = count_constant(y, likelihood, phi)
    order = np.argsort(group, kind='stable')
    counts = np.bincount(group, minlength=G)
    filled = counts > 0
    starts = (np.cumsum(counts) - counts)[filled]

    def group_sums(v):                                     # [n][M] -> [n][G]
        S = np.zeros((v.shape[0], G))
        S[:, filled] = np.add.reduceat(v[:, order], starts, axis=1)
        return S

    def f(z):
        z = np.atleast_2d(np.asarray(z, dtype=float))
        assert z.shape[1] == p + 1 + G
        beta, u, a = z[:, :p], z[:, p], z[:, p + 1:]
        tau = np.exp(u)
        w = (tau / tau_scale) ** 2
        aeff = a if centered else tau[:, None] * a
        eta = (beta @ x.T + aeff[:, group]) + eta0[None, :]
        lp = np.sum(-0.5 * (beta / prior_scale) ** 2, axis=1) \
            - p * (HALF_LOG_2PI + math.log(prior_scale))
        lp = lp + (math.log(2.0 / math.pi) - math.log(tau_scale)) - np.log1p(w) + u
        l, dl = link(likelihood, eta, y, phi)
        lp = lp + np.sum(l, axis=1) + c_data - G * HALF_LOG_2PI
        S = group_sums(dl)
        gb = -beta / prior_scale ** 2 + dl @ x
        gu = 1.0 - 2.0 * w / (1.0 + w)
        if centered:
            zg = a / tau[:, None]
            lp = lp - G * u - 0.5 * np.sum(zg * zg, axis=1)
            ga = S - zg / tau[:, None]
            gu = gu + np.sum(zg * zg, axis=1) - G
        else:
            lp = lp - 0.5 * np.sum(a * a, axis=1)
            ga = tau[:, None] * S - a
            gu = gu + tau * np.sum(S * a, axis=1)
        return lp, np.concatenate([gb, gu[:, None], ga], axis=1)
    return f


def draw_counts(rs, likelihood, eta, phi=None):
    """Counts from the model at eta (clipped to a mean that numpy can draw)."""
    mu = np.exp(np.clip(eta, -30.0, 8.0))
    if likelihood == 'poisson_log':
        return rs.poisson(mu).astype(float)
    return rs.poisson(rs.gamma(phi, mu / phi)).astype(float)


def make_data(D, M, likelihood, seed=0, phi=3.0):
    """x [M][D], y [M], offset [M] drawn from the model at a seeded beta."""
    rs = np.random.RandomState(3000 * seed + 17 * D + M)
    x = rs.randn(M, D)
    beta = 0.5 * rs.randn(D) / math.sqrt(D)
    offset = np.log(rs.uniform(0.5, 4.0, M))
    y = draw_counts(rs, likelihood, x @ beta + offset, phi)
    return x, y, offset


def model_kwargs(likelihood, phi=3.0, prior_scale=3.0):
    """The keyword arguments shared by targets.regression and restatement."""
    kw = dict(likelihood=likelihood, prior_scale=prior_scale)
    if likelihood == 'neg_binomial_2_log':
        kw['phi'] = phi
    return kw


def mlm_make_data(p, G, M, likelihood, seed=0, phi=3.0):
    """x [M][p], y [M], group [M] (shuffled labels, the sizes of tests/mlm_cases.py),
    offset [M]."""
    rs = np.random.RandomState(3000 * seed + 17 * p + 5 * G + M)
    group = np.repeat(np.arange(G), mc.group_sizes(G, M, seed))
    group = group[rs.permutation(M)]
    x = rs.randn(M, p)
    beta = 0.5 * rs.randn(p) / math.sqrt(p)
    a = 0.5 * rs.randn(G)
    offset = np.log(rs.uniform(0.5, 4.0, M))
    y = draw_counts(rs, likelihood, x @ beta + a[group] + offset, phi)
    return x, y, group, offset


def mlm_model_kwargs(likelihood, centered, phi=3.0, prior_scale=3.0, tau_scale=2.0):
    kw = model_kwargs(likelihood, phi=phi, prior_scale=prior_scale)
    kw.update(tau_scale=tau_scale, centered=centered)
    return kw
