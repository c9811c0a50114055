"""Plain numpy restatement of the multilevel regression target
(targets.multilevel_regression, VB_TARGET_MULTILEVEL) with every normalising constant,
and a seeded data generator; shared by the host and device tests.

  z = [beta (p), u = log tau, then G more], tau = exp(u), w = (tau / s_tau)^2
  log p = sum_d log N(beta_d; 0, s^2) + log(2 / (pi s_tau)) - log1p(w) + u
          + sum_m l(y_m, eta_m)                    (the links of tests/glm_cases.py)
  centred       + sum_g log N(a_g; 0, tau^2),  eta_m = x_m . beta + a_group[m]
                (= -G u - sum (a_g / tau)^2 / 2 - G log(2 pi) / 2)
  non-centred   + sum_g log N(at_g; 0, 1),     eta_m = x_m . beta + tau at_group[m]

The observations are used in the order given (the device target sorts them by group).
"""
import math

import numpy as np

from tests import glm_cases as gc

LIKELIHOODS = gc.LIKELIHOODS
FORMS = (False, True)           # centred?
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def restatement(x, y, group, likelihood='gaussian', df=None, scale=1.0, prior_scale=10.0,
                tau_scale=5.0, centered=False, n_groups=None):
    """f(z [n][D]) -> (log p [n], d log p / dz [n][D]), D = p + 1 + G."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    group = np.asarray(group).astype(np.int64)
    assert likelihood in LIKELIHOODS
    M, p = x.shape
    G = int(group.max()) + 1 if n_groups is None else int(n_groups)
    # the sums over a group's observations: its members made contiguous once
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
        eta = beta @ x.T + aeff[:, group]                  # [n][M]
        lp = np.sum(-0.5 * (beta / prior_scale) ** 2, axis=1) \
            - p * (HALF_LOG_2PI + math.log(prior_scale))
        lp = lp + (math.log(2.0 / math.pi) - math.log(tau_scale)) - np.log1p(w) + u
        if likelihood == 'gaussian':
            r = y[None, :] - eta
            l = -0.5 * (r / scale) ** 2
            c_obs = -HALF_LOG_2PI - math.log(scale)
            dl = r / scale ** 2
        elif likelihood == 'student_t':
            r = y[None, :] - eta
            l = -0.5 * (df + 1) * np.log1p(r * r / (df * scale ** 2))
            c_obs = gc.lgamma_half_step(0.5 * df) - HALF_LOG_2PI - math.log(scale)
            dl = (df + 1) * r / (df * scale ** 2 + r * r)
        else:
            e = np.exp(-np.abs(eta))
            l = y[None, :] * eta - (np.maximum(eta, 0.0) + np.log1p(e))
            c_obs = 0.0
            dl = y[None, :] - np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        lp = lp + np.sum(l, axis=1) + M * c_obs - G * HALF_LOG_2PI
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


def group_sizes(G, M, seed):
    """Sizes of G groups over M observations: one group much larger than the rest, and
    as far as G and M have room one singleton and one empty group; the others share
    about 0.3 M at random (some of them may be empty as well)."""
    rs = np.random.RandomState(7000 + 131 * seed + 17 * G + M)
    sizes = np.zeros(G, dtype=np.int64)
    order = rs.permutation(G)
    big = order[0]
    sizes[big] = M
    if G >= 2 and M >= 2:
        sizes[order[1]] = 1
        sizes[big] -= 1
    if G >= 4:
        k = min(int(sizes[big]) - 1, int(0.3 * M))
        if k > 0:
            share = rs.multinomial(k, np.full(G - 3, 1.0 / (G - 3)))
            sizes[order[3:]] = share
            sizes[big] -= k
    assert sizes.sum() == M and sizes.min() >= 0
    return sizes


def make_data(p, G, M, likelihood, seed=0, df=5.0, scale=0.7):
    """x [M][p], y [M], group [M] (labels in 0 .. G - 1, in shuffled order) drawn from the
    model at seeded beta and intercepts (a private RandomState)."""
    rs = np.random.RandomState(1000 * seed + 17 * p + 5 * G + M)
    group = np.repeat(np.arange(G), group_sizes(G, M, seed))
    group = group[rs.permutation(M)]
    x = rs.randn(M, p)
    beta = rs.randn(p) / math.sqrt(p)
    a = 0.8 * rs.randn(G)
    eta = x @ beta + a[group]
    if likelihood == 'gaussian':
        y = eta + scale * rs.randn(M)
    elif likelihood == 'student_t':
        y = eta + scale * rs.standard_t(df, M)
    else:
        y = (rs.rand(M) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return x, y, group


def model_kwargs(likelihood, centered, df=5.0, scale=0.7, prior_scale=3.0, tau_scale=2.0):
    """The keyword arguments shared by targets.multilevel_regression and restatement."""
    kw = gc.model_kwargs(likelihood, df=df, scale=scale, prior_scale=prior_scale)
    kw.update(tau_scale=tau_scale, centered=centered)
    return kw


def rows(n, D, p, seed):
    """Sample rows in the region a fit visits (log tau about one unit wide)."""
    z = np.random.RandomState(seed).randn(n, D)
    z[:, p] *= 0.7
    return z
