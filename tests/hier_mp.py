"""Multiprecision restatement of the hierarchical normal-means target (mpmath, 50
digits), its condition sums and its edge point sets; shared by the CPU test that
pins the numpy restatement of tests/hier_cases.py (tests/test_oracle_hier_mp.py) and
the GPU test of the kernels (tests/test_gpu_hier_edges.py).  In the style of
tests/targets_mp.py, whose Ref, errors, jitter and centres it reuses.

The model (x = [mu, u = log tau, then J more], tau = exp(u), w = (tau / s_tau)^2):

  common        -(mu / s_mu)^2 / 2 - log1p(w) + u
  non-centred   - sum th_j^2 / 2 - sum r_j^2 / 2,   r_j = (y_j - mu - tau th_j) / sigma_j
  centred       - J u - sum z_j^2 / 2 - sum r_j^2 / 2,
                z_j = (th_j - mu) / tau,            r_j = (y_j - th_j) / sigma_j
                d mu = -mu / s_mu^2 + sum z_j / tau
                d u  = -2 w / (1 + w) + 1 - J + sum z_j^2
                d th_j = -z_j / tau + r_j / sigma_j

Error metric: err = |got - ref| / (2^-53 S), S the sum of the absolute values of the
terms added to form the result (tests/targets_mp.py).  The terms, per result:

  common        lp: (mu / s_mu)^2 / 2, log1p(w), |u|;  d mu: |mu| / s_mu^2;
                d u: 2 w / (1 + w), 1
  non-centred   lp: th_j^2 / 2, R_j^2 / 2 per j;  d mu: R_j / sigma_j;
                d u: R_j |tau th_j| / sigma_j;  d th_j: |th_j|, R_j tau / sigma_j
  centred       lp: J |u|; z_j^2 / 2, r_j^2 / 2 per j;  d mu: |z_j| / tau;
                d u: J, z_j^2;  d th_j: |z_j| / tau, |r_j| / sigma_j

In the non-centred form R_j = (|y_j| + |mu| + |tau th_j|) / sigma_j stands where
|r_j| would: the residual's inner sum y_j - mu - tau th_j cancels (mu = 30, log tau
= 4), and with |r_j| that cancellation is invisible to S: the plain metric gave the
numpy restatement up to 45 units for d th_j at J = 65, every other result <= 5.4.
"""
import functools

import numpy as np

from tests import hier_cases as hc
from tests import targets_mp as tm
from tests.targets_mp import Ref, errors, UNIT, ES_LOG_TAU, ES_MU, SEED   # noqa: F401

if tm.available():
    from mpmath import mp, mpf

SIZES = (1, 8, 14, 15, 65)      # the lane kernel's three instances; one and two wave passes
FORMS = (False, True)           # centred?
DATA_SEED = 97
BLOCK_ROWS = 12                 # rows per (log tau, mu) block; the centred form has two blocks


def available():
    return tm.available()


def data(J):
    """The groups of size J: the eight-schools constants at J = 8, seeded otherwise."""
    if J == 8:
        return np.array(hc.ES_Y), np.array(hc.ES_SIGMA)
    return hc.make_data(J, DATA_SEED + J)


def _reference(x, y, sigma, centered, mu_scale, tau_scale):
    n, D = x.shape
    J = D - 2
    out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
    ys = [mpf(float(v)) for v in y]
    sgs = [mpf(float(v)) for v in sigma]
    s_mu, s_tau = mpf(float(mu_scale)), mpf(float(tau_scale))
    for r in range(n):
        mu, u = mpf(float(x[r, 0])), mpf(float(x[r, 1]))
        tau = mp.exp(u)
        w = (tau / s_tau) ** 2
        l1 = mp.log1p(w)
        lp = -(mu / s_mu) ** 2 / 2 - l1 + u
        s_lp = (mu / s_mu) ** 2 / 2 + l1 + abs(u)
        gmu = -mu / s_mu ** 2
        s_gmu = abs(gmu)
        gu = -2 * w / (1 + w) + 1
        s_gu = 2 * w / (1 + w) + 1
        if centered:
            lp -= J * u
            s_lp += J * abs(u)
            gu -= J
            s_gu += J
        for j in range(J):
            th, yj, sg = mpf(float(x[r, 2 + j])), ys[j], sgs[j]
            if centered:
                z = (th - mu) / tau
                res = (yj - th) / sg
                lp += -z * z / 2 - res * res / 2
                s_lp += z * z / 2 + res * res / 2
                gmu += z / tau
                s_gmu += abs(z / tau)
                gu += z * z
                s_gu += z * z
                g = -z / tau + res / sg
                s_g = abs(z / tau) + abs(res / sg)
            else:
                tt = tau * th
                res = (yj - mu - tt) / sg
                big = (abs(yj) + abs(mu) + abs(tt)) / sg      # R_j
                lp += -th * th / 2 - res * res / 2
                s_lp += th * th / 2 + big * big / 2
                gmu += res / sg
                s_gmu += big / sg
                gu += res * tt / sg
                s_gu += big * abs(tt) / sg
                g = -th + res * tau / sg
                s_g = abs(th) + big * tau / sg
            out.g_hi[r, 2 + j], out.g_lo[r, 2 + j] = tm._split(g)
            out.g_S[r, 2 + j] = float(s_g)
        out.lp_hi[r], out.lp_lo[r] = tm._split(lp)
        out.lp_S[r] = float(s_lp)
        out.g_hi[r, 0], out.g_lo[r, 0] = tm._split(gmu)
        out.g_S[r, 0] = float(s_gmu)
        out.g_hi[r, 1], out.g_lo[r, 1] = tm._split(gu)
        out.g_S[r, 1] = float(s_gu)
    return out


def reference(x, y, sigma, centered, mu_scale=5.0, tau_scale=5.0):
    """Ref of the target at the rows of x (n, J + 2), evaluated with DIGITS digits."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    with mp.workdps(tm.DIGITS):
        return _reference(x, y, sigma, centered, mu_scale, tau_scale)


@functools.lru_cache(maxsize=None)
def edge_points(J, centered):
    """The edge rows of (J, form), at most 600: per log tau centre of ES_LOG_TAU and mu
    centre of ES_MU a block with the remaining coordinates standard normal, mu and log
    tau jittered as tests/targets_mp.py's edge_points jitters them (the log tau centre
    itself once); for the centred form a second block with th = mu + tau randn, the
    posterior's own region.  The last RANDOM_SHARE of the rows are standard normal."""
    D = J + 2
    rs = np.random.RandomState(SEED + 50000 + 1000 * int(centered) + J)
    k = BLOCK_ROWS
    rows = []
    for lt in ES_LOG_TAU:
        for m in ES_MU:
            for own in ((False, True) if centered else (False,)):
                blk = rs.randn(k, D)
                blk[:, 0] = tm._jit(rs, m, k) if m != 0.0 else 0.0
                blk[:, 1] = tm._jit(rs, lt, k)
                blk[0, 1] = lt
                if own:
                    blk[:, 2:] = blk[:, :1] + np.exp(blk[:, 1:2]) * blk[:, 2:]
                rows.append(blk)
    x = np.concatenate(rows)
    n_rand = max(1, int(round(tm.RANDOM_SHARE * x.shape[0] / (1.0 - tm.RANDOM_SHARE))))
    x = np.concatenate([x, rs.randn(n_rand, D)])
    assert x.shape[0] <= 600 and np.all(np.isfinite(x))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def edge_reference(J, centered):
    """(points, Ref) of (J, form), computed once per process and shared."""
    x = edge_points(J, centered)
    y, sigma = data(J)
    ref = reference(x, y, sigma, centered)
    for a in ref:
        a.setflags(write=False)
    return x, ref


CASES = [(J, c) for c in FORMS for J in SIZES]

# Worst error of the numpy restatement (tests/hier_cases.py) over the edge sets of
# every J of a form, value and gradient entries together, in units of 2^-53 S;
# measured by tests/test_oracle_hier_mp.py, which asserts twice these figures.  The
# GPU test allows the kernels 8 times them.  Keyed by `centered`.
HIER_ORACLE_ERR = {
    # non-centred: d th_13 at J = 15, row 227 (mu = 0, log tau = 19.98); value 3.62 (J = 15)
    False: 4.55,
    # centred: the value at J = 15, row 444 (mu = 0, log tau = 20, th = mu + tau randn);
    # gradient 4.79 (d mu at J = 15, row 177: mu = 30, log tau = -2)
    True: 5.06,
}
