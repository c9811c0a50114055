"""Plain numpy restatement of the multilevel regression target with a learned scale or
dispersion (targets.multilevel_regression(..., learn_scale=True) / (..., learn_phi=True)),
every normalising constant and both Jacobians kept, with seeded data makers and start rows;
shared by the host and device tests.  In the style of tests/mlm_cases.py (whose
coordinates, priors and group sums these are) and tests/aux_cases.py (whose learned
likelihoods and prior of lambda these are).

  z = [beta (p), u = log tau, then G more, lambda],  D = p + 2 + G
  tau = exp(u), w_tau = (tau / s_tau)^2, theta = e^lambda ~ half-Cauchy(0, s_aux), in lambda
  with w = 2 (lambda - log s_aux):
      log p(lambda) = log(2 / (pi s_aux)) - softplus(w) + lambda,  d/dlambda = 1 - 2 logistic(w)
  log p = sum_d log N(beta_d; 0, s^2) + log(2 / (pi s_tau)) - log1p(w_tau) + u + log p(lambda)
          + sum_m l(y_m, eta_m; lambda)             (the learned links of tests/aux_cases.py)
  centred       + sum_g log N(a_g; 0, tau^2),  eta_m = x_m . beta + a_group[m]
  non-centred   + sum_g log N(at_g; 0, 1),     eta_m = x_m . beta + tau at_group[m]
  (+ eta0_m for the negative binomial)

The observations are used in the order given (the device target sorts them by group).
"""
import math

import numpy as np

from tests import aux_cases as ac
from tests import count_cases as cc
from tests import glm_cases as gc
from tests import mlm_cases as mc

LIKELIHOODS = ac.LIKELIHOODS        # gaussian, student_t, neg_binomial_2_log
FORMS = mc.FORMS
HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def restatement(x, y, group, likelihood='gaussian', df=None, offset=None, prior_scale=10.0,
                tau_scale=5.0, centered=False, n_groups=None, hyper_scale=5.0):
    """f(z [n][D]) -> (log p [n], d log p / dz [n][D]), D = p + 2 + G."""
    x = np.asarray(x, dtype=float)
    y = np.asarray(y, dtype=float)
    group = np.asarray(group).astype(np.int64)
    assert likelihood in LIKELIHOODS
    M, p = x.shape
    G = int(group.max()) + 1 if n_groups is None else int(n_groups)
    nb = likelihood == 'neg_binomial_2_log'
    eta0 = np.zeros(M) if offset is None else np.asarray(offset, dtype=float)
    if nb:
        T, c_data = ac.dispersion_table(y)
        js = np.arange(T.size, dtype=float)
    c_nu = gc.lgamma_half_step(0.5 * df) - HALF_LOG_2PI if likelihood == 'student_t' else 0.0
    c_aux = math.log(2.0 / math.pi) - math.log(hyper_scale)
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
        assert z.shape[1] == p + 2 + G
        beta, u, a, lam = z[:, :p], z[:, p], z[:, p + 1:p + 1 + G], z[:, p + 1 + G]
        tau = np.exp(u)
        w = (tau / tau_scale) ** 2
        aeff = a if centered else tau[:, None] * a
        eta = beta @ x.T + aeff[:, group]                  # [n][M]
        lp = np.sum(-0.5 * (beta / prior_scale) ** 2, axis=1) \
            - p * (HALF_LOG_2PI + math.log(prior_scale))
        lp = lp + (math.log(2.0 / math.pi) - math.log(tau_scale)) - np.log1p(w) + u
        sp, lg = ac._softplus_logistic(2.0 * (lam - math.log(hyper_scale)))
        prior = c_aux - sp + lam
        gl = 1.0 - 2.0 * lg
        if nb:
            eta = eta + eta0[None, :]
            phi = np.exp(lam)[:, None]
            s2, l2 = ac._softplus_logistic(eta - lam[:, None])
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
        lp = lp - G * HALF_LOG_2PI
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
        return lp, np.concatenate([gb, gu[:, None], ga, gl[:, None]], axis=1)
    return f


def lambda_prior(lam, hyper_scale):
    """log p(lambda) of the module docstring."""
    sp, _ = ac._softplus_logistic(2.0 * (np.asarray(lam, dtype=float) - math.log(hyper_scale)))
    return math.log(2.0 / math.pi) - math.log(hyper_scale) - sp + lam


def make_data(p, G, M, likelihood, seed=0, df=5.0, scale=0.7, phi=3.0):
    """(x [M][p], y [M], group [M], offset [M] or None) drawn from the model."""
    if likelihood == 'neg_binomial_2_log':
        return cc.mlm_make_data(p, G, M, likelihood, seed=seed, phi=phi)
    return mc.make_data(p, G, M, likelihood, seed=seed, df=df, scale=scale) + (None,)


def model_kwargs(likelihood, centered, df=5.0, prior_scale=3.0, tau_scale=2.0, hyper_scale=2.0):
    """The keyword arguments shared by restatement and (with the learn flag of
    target_kwargs) targets.multilevel_regression."""
    kw = ac.model_kwargs(likelihood, df=df, prior_scale=prior_scale, hyper_scale=hyper_scale)
    kw.update(tau_scale=tau_scale, centered=centered)
    return kw


target_kwargs = ac.target_kwargs


def start_rows(rs, n, p, G, likelihood, spread=0.3):
    """n rows [beta, u, G more, lambda] near a plausible fit: spread randn, lambda near the
    log of the data makers' scale / dispersion."""
    z = rs.randn(n, p + 2 + G) * spread
    z[:, -1] += math.log(3.0) if likelihood == 'neg_binomial_2_log' else math.log(0.7)
    return z
