"""Plain numpy restatement of the low-rank-plus-diagonal Gaussian family
(vb.low_rank_gaussian_variational_family, VB_FAMILY_LR_GAUSSIAN) and of its three
estimators, for the parity tests of vb_lrg.hip.

var_param = [mu (D), log_d (D), B (D x R, row-major)], d = exp(log_d),
Sigma = B B^T + diag(d^2).  A draw is one row [z (D), u (R)] of standard normals and
x = mu + d z + B u.  A target is a callable x [n, D] -> (log p [n], d log p / dx [n, D]).

With W = diag(1/d) B and C = I + W^T W (R x R):

    y = (x - mu) / d,  t = C^-1 W^T y,  rho = y - W t,  a = Sigma^-1 (x - mu) = rho / d,
    log q(x) = -D/2 log 2 pi - sum log_d - 1/2 log det C - 1/2 (|rho|^2 + |t|^2),
    entropy  = D/2 (1 + log 2 pi) + sum log_d + 1/2 log det C,
    H_B = diag(1/d) W C^-1,  H_d,i = 1 - w_i^T C^-1 w_i   (the entropy's gradient).

The gradient of every estimator, r_n = -1/N for KLVI and KLVI_PD and r_n = alpha w_n / N,
w_n = exp(alpha (lw_n - max lw)) for CHIVI:

    KLVI            grad mu = sum r_n g_n
                    grad log_d_i = sum_n r_n g_ni d_i z_ni + (sum r) H_d,i
                    grad B = G^T diag(r) U + (sum r) H_B
    KLVI_PD, CHIVI  grad mu = sum r_n g_n
                    grad log_d_i = sum_n r_n [(g_ni + a_ni) d_i z_ni - a_ni^2 d_i^2] + (sum r) H_d,i
                    grad B = (G + A)^T diag(r) U - A^T diag(r) T + (sum r) H_B   (A B = T)

KLVI_PD's value holds log q(x_n(lambda); lambda), which for this family depends on
lambda sample by sample (for the mean-field and Cholesky families it is a constant minus
|z_n|^2 / 2), so its gradient is the full form with r_n = -1/N, not KLVI's entropy form:
50-digit central differences of the value decide (tests/test_lrg_host.py).

No scipy: C^-1 is L^-T L^-1 from numpy's Cholesky factor and a forward substitution
written out.  The D x D matrix is formed in mean_and_cov only."""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)


def n_free(D, R):
    return D * (R + 2)


def pack(mu, log_d, B):
    return np.concatenate([np.asarray(mu, float), np.asarray(log_d, float),
                           np.asarray(B, float).ravel()])


class LowRankGaussian:
    def __init__(self, dim, rank):
        self.dim, self.rank = int(dim), int(rank)
        self.var_param_dim = n_free(self.dim, self.rank)
        self.rs = np.random.RandomState(0)

    def unpack(self, lam):
        lam = np.asarray(lam, dtype=float)
        D, R = self.dim, self.rank
        return lam[:D], lam[D:2 * D], lam[2 * D:].reshape(D, R)

    def draw(self, n, seed=None):
        rs = self.rs if seed is None else np.random.RandomState(seed)
        return rs.randn(n, self.dim + self.rank)

    def transform(self, lam, eps):
        mu, log_d, B = self.unpack(lam)
        D = self.dim
        return (mu + np.exp(log_d) * eps[:, :D]) + eps[:, D:] @ B.T

    def sample(self, lam, n, seed=None):
        return self.transform(lam, self.draw(n, seed))

    def capacitance(self, lam):
        """W, C^-1, 1/2 log det C."""
        _, log_d, B = self.unpack(lam)
        R = self.rank
        W = B / np.exp(log_d)[:, None]
        L = np.linalg.cholesky(np.eye(R) + W.T @ W)
        Li = np.zeros((R, R))
        for j in range(R):                      # forward substitution, column by column
            Li[j, j] = 1.0 / L[j, j]
            for i in range(j + 1, R):
                Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
        return W, Li.T @ Li, float(np.sum(np.log(np.diag(L))))

    def entropy(self, lam):
        _, log_d, _ = self.unpack(lam)
        _, _, hld = self.capacitance(lam)
        return (0.5 * self.dim * (1.0 + LOG2PI) + np.sum(log_d)) + hld

    def quad(self, y, lam):
        """t [n, R], a = rho / d [n, D], q = |rho|^2 + |t|^2 [n] of standardized rows y."""
        _, log_d, _ = self.unpack(lam)
        W, Ci, _ = self.capacitance(lam)
        t = (y @ W) @ Ci.T
        rho = y - t @ W.T
        return t, rho / np.exp(log_d), np.sum(rho * rho, axis=1) + np.sum(t * t, axis=1)

    def _logq(self, q, lam):
        _, log_d, _ = self.unpack(lam)
        _, _, hld = self.capacitance(lam)
        return (-0.5 * self.dim * LOG2PI - np.sum(log_d) - hld) - 0.5 * q

    def logdensity(self, x, lam):
        mu, log_d, _ = self.unpack(lam)
        y = (np.atleast_2d(np.asarray(x, dtype=float)) - mu) / np.exp(log_d)
        out = self._logq(self.quad(y, lam)[2], lam)
        return out[0] if np.ndim(x) == 1 else out

    def standardized(self, eps, lam):
        """y = z + W u of the family's own draws."""
        W, _, _ = self.capacitance(lam)
        D = self.dim
        return eps[:, :D] + eps[:, D:] @ W.T

    def logdensity_of_draws(self, eps, lam):
        return self._logq(self.quad(self.standardized(eps, lam), lam)[2], lam)

    def entropy_grad(self, lam):
        _, log_d, _ = self.unpack(lam)
        W, Ci, _ = self.capacitance(lam)
        V = W @ Ci
        return 1.0 - np.sum(W * V, axis=1), V / np.exp(log_d)[:, None]

    def mean_and_cov(self, lam):
        mu, log_d, B = self.unpack(lam)
        return mu, B @ B.T + np.diag(np.exp(2 * log_d))

    def pth_moment(self, p, lam):
        if p not in (2, 4):
            raise ValueError('only p = 2 or 4 supported')
        _, log_d, B = self.unpack(lam)
        d2 = np.exp(2 * log_d)
        b2 = np.sum(B * B, axis=1)
        tr = np.sum(d2) + np.sum(b2)
        if p == 2:
            return tr
        fro = np.sum(d2 ** 2) + 2 * np.sum(d2 * b2) + np.sum((B.T @ B) ** 2)
        return 2.0 * fro + tr ** 2


def _pack_grad(fam, lam, r, g, eps, chivi):
    D = fam.dim
    _, log_d, _ = fam.unpack(lam)
    d = np.exp(log_d)
    z, u = eps[:, :D], eps[:, D:]
    Hd, HB = fam.entropy_grad(lam)
    rsum = np.sum(r)
    rc = r[:, None]
    g_mu = np.sum(rc * g, axis=0)
    if not chivi:
        g_ld = np.sum(rc * g * (d * z), axis=0) + rsum * Hd
        g_B = g.T @ (rc * u) + rsum * HB
    else:
        t, a, _ = fam.quad(fam.standardized(eps, lam), lam)
        g_ld = np.sum(rc * ((g + a) * (d * z) - (a * d) ** 2), axis=0) + rsum * Hd
        g_B = ((g + a).T @ (rc * u) - a.T @ (rc * t)) + rsum * HB
    return pack(g_mu, g_ld, g_B)


def _draws(fam, n_samples, draws, seed=None):
    return fam.draw(n_samples, seed) if draws is None else np.asarray(draws, dtype=float)


def klvi_value_grad(fam, target, lam, n_samples, draws=None):
    eps = _draws(fam, n_samples, draws)
    lp, g = target(fam.transform(lam, eps))
    r = np.full(eps.shape[0], -1.0 / eps.shape[0])
    return -(fam.entropy(lam) + np.mean(lp)), _pack_grad(fam, lam, r, g, eps, False)


def klvi_pd_value_grad(fam, target, lam, n_samples, draws=None):
    eps = _draws(fam, n_samples, draws)
    lp, g = target(fam.transform(lam, eps))
    r = np.full(eps.shape[0], -1.0 / eps.shape[0])
    return (-np.mean(lp - fam.logdensity_of_draws(eps, lam)),
            _pack_grad(fam, lam, r, g, eps, True))


def chivi_value_grad(fam, target, lam, n_samples, alpha, draws=None):
    """draws None: the per-call seed from the global numpy RNG (vb.py:258)."""
    if draws is None:
        eps = fam.draw(n_samples, np.random.randint(2 ** 32))
    else:
        eps = np.asarray(draws, dtype=float)
    lp, g = target(fam.transform(lam, eps))
    lw = lp - fam.logdensity_of_draws(eps, lam)
    mx = np.max(lw)
    w = np.exp(alpha * (lw - mx))
    N = eps.shape[0]
    return np.log(np.mean(w)) / alpha + mx, _pack_grad(fam, lam, alpha * w / N, g, eps, True)


def log_weights(fam, target, lam, n_samples, draws=None):
    eps = _draws(fam, n_samples, draws)
    x = fam.transform(lam, eps)
    lp, _ = target(x)
    return x, lp - fam.logdensity_of_draws(eps, lam)
