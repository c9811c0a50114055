"""Shared data and the numpy restatement of the hierarchical normal-means target
(targets.hierarchical_normal, VB_TARGET_HIERARCHICAL), written from the model's
definition:

  x = [mu, u = log tau, then J more], tau = exp(u), w = (tau / s_tau)^2
  common        -(mu / s_mu)^2 / 2 - log1p(w) + u
  non-centred   - sum th_j^2 / 2 - sum r_j^2 / 2,   r_j = (y_j - mu - tau th_j) / sigma_j
  centred       - J u - sum z_j^2 / 2 - sum r_j^2 / 2,
                z_j = (th_j - mu) / tau,            r_j = (y_j - th_j) / sigma_j

(Stan's log_prob convention: the constants of the ~ statements dropped, the
Jacobian term +u kept.)
"""
import numpy as np

ES_Y = (28., 8., -3., 7., -1., 1., 18., 12.)
ES_SIGMA = (15., 10., 16., 11., 9., 11., 10., 18.)


def make_data(J, seed):
    """y ~ 10 randn, sigma uniform in [5, 20]."""
    rs = np.random.RandomState(seed)
    return 10.0 * rs.randn(J), rs.uniform(5.0, 20.0, size=J)


def restatement(y, sigma, centered, mu_scale=5.0, tau_scale=5.0):
    """f(x) -> (log p (n,), d log p / dx (n, J + 2)) for x of shape (n, J + 2)."""
    y = np.asarray(y, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    J = y.size

    def f(x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        mu, u, th = x[:, 0], x[:, 1], x[:, 2:]
        tau = np.exp(u)
        w = (tau / tau_scale) ** 2
        lp = -(mu / mu_scale) ** 2 / 2 - np.log1p(w) + u
        gmu = -mu / mu_scale ** 2
        gu = -2 * w / (1 + w) + 1
        if centered:
            z = (th - mu[:, None]) / tau[:, None]
            r = (y - th) / sigma
            lp = lp - J * u - np.sum(z * z, axis=1) / 2 - np.sum(r * r, axis=1) / 2
            gmu = gmu + np.sum(z / tau[:, None], axis=1)
            gu = gu - J + np.sum(z * z, axis=1)
            gth = -z / tau[:, None] + r / sigma
        else:
            tt = tau[:, None] * th
            r = (y - mu[:, None] - tt) / sigma
            lp = lp - np.sum(th * th, axis=1) / 2 - np.sum(r * r, axis=1) / 2
            gmu = gmu + np.sum(r / sigma, axis=1)
            gu = gu + np.sum(r * tt / sigma, axis=1)
            gth = -th + r * tau[:, None] / sigma
        return lp, np.concatenate([gmu[:, None], gu[:, None], gth], axis=1)
    return f
