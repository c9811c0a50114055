"""Plain numpy restatement of the Cholesky full-rank Gaussian family
(vb.cholesky_gaussian_variational_family, VB_FAMILY_FR_GAUSSIAN) and of its three
estimators, for the parity tests of vb_frg.hip.

var_param = [mu (D), tril(M) row-major (D (D + 1) / 2)], L = M with its diagonal
exponentiated, Sigma = L L^T (oracle.fullrank_oracle.unpack).  A target is a
callable x [n, D] -> (log p [n], d log p / dx [n, D]).

The gradient of every estimator is

    grad mu = sum_n r_n g_n,   G_L = G^T diag(r) Z,
    grad tril = G_L[i][j] (i > j),  G_L[i][i] L_ii + sum_n r_n on the log diagonal,

with r_n = -1/N for KLVI and KLVI_PD and r_n = alpha w_n / N, w_n = exp(alpha (lw_n -
max lw)) for CHIVI.  No scipy in any formula here: the triangular solve of
logdensity is a forward substitution written out, as is every constant."""
import math

import numpy as np

from oracle.fullrank_oracle import unpack

LOG2PI = math.log(2.0 * math.pi)


def n_free(D):
    return D + D * (D + 1) // 2


def diag_index(D):
    """Positions of M_ii in var_param."""
    i = np.arange(D)
    return D + i * (i + 1) // 2 + i


class CholeskyGaussian:
    def __init__(self, dim):
        self.dim = int(dim)
        self.var_param_dim = n_free(self.dim)
        self.rs = np.random.RandomState(0)

    def draw(self, n, seed=None):
        rs = self.rs if seed is None else np.random.RandomState(seed)
        return rs.randn(n, self.dim)

    def transform(self, lam, z):
        mu, L, _ = unpack(np.asarray(lam, dtype=float), self.dim)
        return mu + z @ L.T

    def sample(self, lam, n, seed=None):
        return self.transform(lam, self.draw(n, seed))

    def sum_log_diag(self, lam):
        return float(np.sum(np.asarray(lam, dtype=float)[diag_index(self.dim)]))

    def entropy(self, lam):
        return 0.5 * self.dim * (1.0 + LOG2PI) + self.sum_log_diag(lam)

    def logdensity(self, x, lam):
        mu, L, _ = unpack(np.asarray(lam, dtype=float), self.dim)
        c = np.atleast_2d(np.asarray(x, dtype=float)) - mu
        y = np.zeros_like(c)
        for i in range(self.dim):          # forward substitution, row by row
            y[:, i] = (c[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
        out = -0.5 * self.dim * LOG2PI - self.sum_log_diag(lam) - 0.5 * np.sum(y * y, axis=1)
        return out[0] if np.ndim(x) == 1 else out

    def logdensity_of_draws(self, z, lam):
        """log q(mu + L z): the form the estimators use (no solve)."""
        return -0.5 * self.dim * LOG2PI - self.sum_log_diag(lam) - 0.5 * np.sum(z * z, axis=1)

    def mean_and_cov(self, lam):
        mu, _, Sig = unpack(np.asarray(lam, dtype=float), self.dim)
        return mu, Sig

    def pth_moment(self, p, lam):
        if p not in (2, 4):
            raise ValueError('only p = 2 or 4 supported')
        _, _, Sig = unpack(np.asarray(lam, dtype=float), self.dim)
        tr = np.trace(Sig)
        return tr if p == 2 else 2.0 * np.sum(Sig ** 2) + tr ** 2


def _pack(fam, lam, r, g, z):
    D = fam.dim
    _, L, _ = unpack(np.asarray(lam, dtype=float), D)
    GL = g.T @ (r[:, None] * z)
    out = np.empty(n_free(D))
    out[:D] = np.sum(r[:, None] * g, axis=0)
    T = np.tril(GL)
    T[np.diag_indices(D)] = np.diag(GL) * np.diag(L) + np.sum(r)
    out[D:] = T[np.tril_indices(D)]
    return out


def _draws(fam, n_samples, draws, seed=None):
    return fam.draw(n_samples, seed) if draws is None else np.asarray(draws, dtype=float)


def klvi_value_grad(fam, target, lam, n_samples, draws=None):
    z = _draws(fam, n_samples, draws)
    lp, g = target(fam.transform(lam, z))
    r = np.full(z.shape[0], -1.0 / z.shape[0])
    return -(fam.entropy(lam) + np.mean(lp)), _pack(fam, lam, r, g, z)


def klvi_pd_value_grad(fam, target, lam, n_samples, draws=None):
    z = _draws(fam, n_samples, draws)
    lp, g = target(fam.transform(lam, z))
    r = np.full(z.shape[0], -1.0 / z.shape[0])
    return -np.mean(lp - fam.logdensity_of_draws(z, lam)), _pack(fam, lam, r, g, z)


def chivi_value_grad(fam, target, lam, n_samples, alpha, draws=None):
    """draws None: the per-call seed from the global numpy RNG (vb.py:258)."""
    if draws is None:
        z = fam.draw(n_samples, np.random.randint(2 ** 32))
    else:
        z = np.asarray(draws, dtype=float)
    lp, g = target(fam.transform(lam, z))
    lw = lp - fam.logdensity_of_draws(z, lam)
    mx = np.max(lw)
    w = np.exp(alpha * (lw - mx))
    N = z.shape[0]
    return np.log(np.mean(w)) / alpha + mx, _pack(fam, lam, alpha * w / N, g, z)


def log_weights(fam, target, lam, n_samples, draws=None):
    z = _draws(fam, n_samples, draws)
    x = fam.transform(lam, z)
    lp, _ = target(x)
    return x, lp - fam.logdensity_of_draws(z, lam)
