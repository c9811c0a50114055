"""Multiprecision restatement (mpmath, 50 digits) of the mean-field Gaussian and
Student-t estimators and of one optimiser update, independent of
oracle/vb_oracle.py; shared by tests/test_oracle_mf_mp.py (which pins the numpy
oracle) and tests/test_gpu_mf_edges.py (the device kernels).

With lam = [mu (D), ls (D)], sigma = exp(ls) and standardised draws eps (N x D,
taken as exact doubles):

  x_nd     = mu_d + sigma_d eps_nd
  log q    gauss: sum_d [-z^2/2 - ls_d - log(2 pi)/2],  z = (x - mu) / sigma
           t:     sum_d [c - (df+1)/2 log1p(z^2/df) - ls_d],
                  c = lgamma((df+1)/2) - lgamma(df/2) - log(df pi)/2
  entropy  gauss: D/2 (1 + log 2 pi) + sum ls;  t: sum ls  (the reference drops the
           t family's constant, vb.py:156)
  KLVI     value -(H + mean_n log p(x_n));  d/dmu_d = -mean_n g_nd,
           d/dls_d = -(1 + sigma_d mean_n g_nd eps_nd)
  KLVI_PD  value -(mean log p - mean log q(x));  the same gradient
  CHIVI    lw_n = log p(x_n) - log q(x_n), M = max lw, w_n = exp(alpha (lw_n - M)),
           value log(mean w)/alpha + M;  d/dmu_d = alpha/N sum_n w_n g_nd,
           d/dls_d = alpha/N sum_n w_n (g_nd sigma_d eps_nd + 1)
  adagrad  lam - lr g / sqrt(eps + sum over the window of g_k^2)      (vb.py:365-374)

log p and its gradient are the row functions of tests/targets_mp.py (ROW), at the
multiprecision x.

Condition sums.  Every result carries S, the sum of the absolute values of the
terms added to form it; errors are reported in units of 2^-53 S (targets_mp).
A double evaluation rounds x = mu + sigma eps before the target sees it, by up to
dx_d = |mu_d| + |sigma_d eps_nd| units, so a row's S of log p gains sum_d |g_d| dx_d
and S of g_d gains sum_j |d g_d / d x_j| dx_j (the curvature: closed forms for
isogauss, the mixture (|g'| <= 3) and the funnel, multiprecision forward
differences for eight schools).  log q of an estimator may be read back from the
rounded x (the reference and the oracle call logdensity(x)): z = (x - mu) / sigma
then moves by dx / sigma, and S of log q gains sum_d |d log q / d z_d| dx_d / sigma_d
(large where sigma << |mu|: that form of log q is ill-conditioned there).  Then

  KLVI value   D/2 (1 + log 2 pi) + sum |ls| + mean S_lp     (PD: mean (S_lp + S_lq))
  d/dmu_d      mean_n S_g,nd          d/dls_d   1 + sigma_d mean_n S_g,nd |eps_nd|
  CHIVI        an error e_n of lw_n moves w_n by alpha (e_n + e_M) relatively:
    value      sum w_n S_lw,n / sum w + |log(mean w)| / alpha + |M|
    d/dmu_d    alpha/N sum_n w_n [S_g,nd + |g_nd| alpha (S_lw,n + S_lw,M)]
    d/dls_d    alpha/N sum_n w_n [S_g,nd sigma_d |eps_nd| + 1
                                  + (|g_nd sigma_d eps_nd| + 1) alpha (S_lw,n + S_lw,M)]
  update       |lam'| + |step|, step = lr g / sqrt(...)  (adagrad, RMSProp-IA, Adam-IA:
               ia_update's docstring)

The restatement's gradients are checked against multiprecision central
differences of its own values (fd_check; tests/test_oracle_mf_mp.py).
"""
from collections import namedtuple

import numpy as np

from tests import targets_mp as tm
from tests.targets_mp import DIGITS, UNIT, mpmath

if mpmath is not None:
    from mpmath import mp, mpf

# ref = hi + lo, S the condition sum (scalars or arrays of one shape)
Val = namedtuple('Val', 'hi lo S')
# a condition sum past the double range (the -inf cases: |g| dx ~ x^2) is held at it
DBL_MAX = float(np.finfo(np.float64).max)
# value: Val scalar; grad: Val (2D,); lw, lq, lp: Val (N,); x: (N, D) doubles
Est = namedtuple('Est', 'value grad lw lq lp x')


def available():
    return mpmath is not None


def _val(vals, Ss):
    """Val of mp numbers (scalar or nested list) and their condition sums."""
    if isinstance(vals, (list, tuple)):
        a = np.array(vals, dtype=object)
        hi = np.vectorize(float, otypes=[float])(a)
        lo = np.vectorize(lambda v, h: float(v - mpf(h)), otypes=[float])(a, hi)
        S = np.vectorize(float, otypes=[float])(np.array(Ss, dtype=object))
        return Val(hi, lo, np.minimum(S, DBL_MAX))
    hi = float(vals)
    return Val(hi, float(vals - mpf(hi)), min(float(Ss), DBL_MAX))


def units(got, ref):
    """|got - ref| in units of 2^-53 S; inf where got is not finite, or differs
    from a reference that is exactly 0 with S = 0."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        d = np.abs((got - ref.hi) - ref.lo)
        e = np.where(np.asarray(ref.S) > 0, d / (UNIT * np.asarray(ref.S)),
                     np.where(d == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), e, np.inf)


def finite(ref):
    return bool(np.all(np.isfinite(ref.hi)) and np.all(np.isfinite(ref.S)))


# ---- the family ---------------------------------------------------------------
def _t_const(df):
    """(c, S_c) of the t density's constant."""
    a, b, h = mp.loggamma((df + 1) / 2), mp.loggamma(df / 2), mp.log(df * mp.pi) / 2
    return a - b - h, abs(a) + abs(b) + abs(h)


def _logq1(kind, df, tc, ls, z):
    """One coordinate's log q at standardised z, and its condition sum."""
    if kind == 'gauss':
        h = mp.log(2 * mp.pi) / 2
        return -z * z / 2 - ls - h, z * z / 2 + abs(ls) + h
    t = (df + 1) / 2 * mp.log1p(z * z / df)
    return tc[0] - t - ls, tc[1] + t + abs(ls)


def _lam(lam):
    lam = [v if isinstance(v, mpf) else mpf(float(v)) for v in lam]
    D = len(lam) // 2
    return lam[:D], lam[D:]


def logdensity(kind, df, lam, x):
    """Val (n,) of log q(x_r; lam) at the rows of x (doubles)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    with mp.workdps(DIGITS):
        mu, ls = _lam(lam)
        dfm = None if df is None else mpf(float(df))
        tc = None if df is None else _t_const(dfm)
        sg = [mp.exp(v) for v in ls]
        out, S = [], []
        for r in range(x.shape[0]):
            t = [_logq1(kind, dfm, tc, ls[d], (mpf(float(x[r, d])) - mu[d]) / sg[d])
                 for d in range(len(mu))]
            out.append(mp.fsum(v[0] for v in t))
            S.append(mp.fsum(v[1] for v in t))
        return _val(out, S)


def transform(lam, eps):
    """Val (N, D) of x = mu + exp(ls) eps."""
    eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
    with mp.workdps(DIGITS):
        mu, ls = _lam(lam)
        sg = [mp.exp(v) for v in ls]
        x = [[mu[d] + sg[d] * mpf(float(e[d])) for d in range(len(mu))] for e in eps]
        S = [[abs(mu[d]) + abs(sg[d] * mpf(float(e[d]))) for d in range(len(mu))] for e in eps]
        return _val(x, S)


def entropy(kind, lam):
    with mp.workdps(DIGITS):
        _, ls = _lam(lam)
        c = len(ls) * (1 + mp.log(2 * mp.pi)) / 2 if kind == 'gauss' else mpf(0)
        return _val(c + mp.fsum(ls), c + mp.fsum(abs(v) for v in ls))


def mean_and_cov_diag(kind, df, lam):
    """Val (D,) of the covariance's diagonal (each entry one product: S = |entry|)."""
    with mp.workdps(DIGITS):
        _, ls = _lam(lam)
        c = 1 if kind == 'gauss' else mpf(float(df)) / (mpf(float(df)) - 2)
        v = [c * mp.exp(2 * l) for l in ls]
        return _val(v, v)


def pth_moment(kind, df, p, lam):
    with mp.workdps(DIGITS):
        _, ls = _lam(lam)
        v = [mp.exp(2 * l) for l in ls]
        s2, s4 = mp.fsum(v), mp.fsum(t * t for t in v)
        if kind == 'gauss':
            r = s2 if p == 2 else 2 * s4 + s2 ** 2
        else:
            dfm = mpf(float(df))
            c = dfm / (dfm - 2)
            r = c * s2 if p == 2 else c ** 2 * (2 * (dfm - 1) / (dfm - 4) * s4 + s2 ** 2)
        return _val(r, r)


# ---- the estimators -------------------------------------------------------------
def _curvature(target, xs, dx):
    """sum_j |d g_d / d x_j| dx_j per coordinate d."""
    D = len(xs)
    if target == 'isogauss':
        return list(dx)
    if target == 'mixture':
        return [3 * v for v in dx]          # g' = -1 + 16 w (1 - w) in [-1, 3]
    if target == 'funnel':
        v = xs[1]
        e2 = mp.exp(-2 * v)
        out = [None] * D
        cv = dx[1] / mpf('1.35') ** 2
        for d in range(D):
            if d == 1:
                continue
            cross = 2 * abs(xs[d]) * e2
            out[d] = e2 * dx[d] + cross * dx[1]
            cv += 2 * xs[d] ** 2 * e2 * dx[1] + cross * dx[d]
        out[1] = cv
        return out
    h = mpf(10) ** -25
    g0 = tm.ROW[target](xs)[2]
    out = [mpf(0)] * D
    for j in range(D):
        xj = list(xs)
        xj[j] = xs[j] + h
        gj = tm.ROW[target](xj)[2]
        for d in range(D):
            out[d] += abs((gj[d] - g0[d]) / h) * dx[j]
    return out


def _rows(kind, df, target, mu, ls, eps, curvature=True):
    """Per draw: (x, lp, S_lp, g, S_g, lq, S_lq), all multiprecision."""
    D = len(mu)
    sg = [mp.exp(v) for v in ls]
    dfm = None if df is None else mpf(float(df))
    tc = None if df is None else _t_const(dfm)
    rows = []
    for e in eps:
        em = [mpf(float(v)) for v in e]
        xs = [mu[d] + sg[d] * em[d] for d in range(D)]
        dx = [abs(mu[d]) + abs(sg[d] * em[d]) for d in range(D)]
        lp, s_lp, g, gS = tm.ROW[target](xs)
        if curvature:
            s_lp += mp.fsum(abs(g[d]) * dx[d] for d in range(D))
            cv = _curvature(target, xs, dx)
            gS = [gS[d] + cv[d] for d in range(D)]
        q = [_logq1(kind, dfm, tc, ls[d], em[d]) for d in range(D)]
        s_lq = mp.fsum(v[1] for v in q)
        if curvature:
            # log q read back from the rounded x (the oracle, the log-weight kernels):
            # z = (x - mu) / sigma moves by dx / sigma
            s_lq += mp.fsum((abs(em[d]) if kind == 'gauss' else
                             (dfm + 1) * abs(em[d]) / (dfm + em[d] ** 2)) * dx[d] / sg[d]
                            for d in range(D))
        rows.append((xs, lp, s_lp, g, gS, mp.fsum(v[0] for v in q), s_lq, em))
    return sg, rows


def _estimate(objective, kind, df, target, mu, ls, eps, alpha, M0=None, curvature=True):
    """The estimator at multiprecision (mu, ls): a dict of mp numbers.  M0: CHIVI's
    normaliser held fixed (the function the returned CHIVI gradient differentiates
    is mean_n exp(alpha (lw_n - M0)), reported as 'meanw')."""
    D, N = len(mu), len(eps)
    sg, rows = _rows(kind, df, target, mu, ls, eps, curvature)
    out = {'rows': rows}
    lw = [r[1] - r[5] for r in rows]
    lwS = [r[2] + r[6] for r in rows]
    out['lw'], out['lwS'] = lw, lwS
    if objective in ('klvi', 'klvi_pd'):
        mlp = mp.fsum(r[1] for r in rows) / N
        if objective == 'klvi':
            c = D * (1 + mp.log(2 * mp.pi)) / 2 if kind == 'gauss' else mpf(0)
            out['value'] = -(c + mp.fsum(ls) + mlp)
            out['valueS'] = c + mp.fsum(abs(v) for v in ls) + mp.fsum(r[2] for r in rows) / N
        else:
            out['value'] = -(mlp - mp.fsum(r[5] for r in rows) / N)
            out['valueS'] = mp.fsum(lwS) / N
        gm = [-mp.fsum(r[3][d] for r in rows) / N for d in range(D)]
        gmS = [mp.fsum(r[4][d] for r in rows) / N for d in range(D)]
        gl = [-(1 + sg[d] * mp.fsum(r[3][d] * r[7][d] for r in rows) / N) for d in range(D)]
        glS = [1 + sg[d] * mp.fsum(r[4][d] * abs(r[7][d]) for r in rows) / N for d in range(D)]
    else:
        a = mpf(float(alpha))
        k = max(range(N), key=lambda n: lw[n])
        M = lw[k] if M0 is None else M0
        w = [mp.exp(a * (v - M)) for v in lw]
        sw = mp.fsum(w)
        out['M'], out['meanw'] = M, sw / N
        out['value'] = mp.log(sw / N) / a + M
        out['valueS'] = (mp.fsum(w[n] * lwS[n] for n in range(N)) / sw
                         + abs(mp.log(sw / N)) / a + abs(M))
        rel = [a * (lwS[n] + lwS[k]) for n in range(N)]
        gm = [a * mp.fsum(w[n] * rows[n][3][d] for n in range(N)) / N for d in range(D)]
        gmS = [a * mp.fsum(w[n] * (rows[n][4][d] + abs(rows[n][3][d]) * rel[n])
                           for n in range(N)) / N for d in range(D)]
        gl = [a * mp.fsum(w[n] * (rows[n][3][d] * sg[d] * rows[n][7][d] + 1)
                          for n in range(N)) / N for d in range(D)]
        glS = [a * mp.fsum(w[n] * (rows[n][4][d] * sg[d] * abs(rows[n][7][d]) + 1
                                   + (abs(rows[n][3][d] * sg[d] * rows[n][7][d]) + 1) * rel[n])
                           for n in range(N)) / N for d in range(D)]
    out['grad'], out['gradS'] = gm + gl, gmS + glS
    return out


def estimate(objective, kind, df, target, lam, eps, alpha=None):
    """Est of objective in {'klvi', 'klvi_pd', 'chivi'} at lam on the draws eps."""
    eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
    with mp.workdps(DIGITS):
        mu, ls = _lam(lam)
        o = _estimate(objective, kind, df, target, mu, ls, eps, alpha)
        rows = o['rows']
        return Est(_val(o['value'], o['valueS']), _val(o['grad'], o['gradS']),
                   _val(o['lw'], o['lwS']), _val([r[5] for r in rows], [r[6] for r in rows]),
                   _val([r[1] for r in rows], [r[2] for r in rows]),
                   np.array([[float(v) for v in r[0]] for r in rows]))


def fd_check(objective, kind, df, target, lam, eps, alpha=None):
    """Largest relative gap between the restated gradient and central differences
    (h = 1e-20 scale, 50 digits) of the restated value: of the value itself for
    KLVI / KLVI_PD, of mean_n exp(alpha (lw_n - M)) with M held for CHIVI.  Scaled
    by the gradient entry's condition sum."""
    eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
    key = 'meanw' if objective == 'chivi' else 'value'
    with mp.workdps(DIGITS):
        mu, ls = _lam(lam)
        o = _estimate(objective, kind, df, target, mu, ls, eps, alpha)
        M0 = o.get('M')
        worst = mpf(0)
        lamv = mu + ls
        for j in range(len(lamv)):
            h = mpf(10) ** -20 * max(1, abs(lamv[j]))
            f = []
            for s in (1, -1):
                lj = list(lamv)
                lj[j] = lamv[j] + s * h
                f.append(_estimate(objective, kind, df, target, lj[:len(mu)], lj[len(mu):], eps,
                                   alpha, M0=M0, curvature=False)[key])
            fd = (f[0] - f[1]) / (2 * h)
            worst = max(worst, abs(fd - o['grad'][j]) / o['gradS'][j])
        return float(worst)


_GOLDEN = []


def golden(c):
    """The precomputed reference of a case marked golden (tests/golden/mf_mp.npz,
    written by tests/golden/make_mf_mp.py); the case's seeded inputs must hash to the
    digest stored beside it."""
    import os
    from tests import mf_cases
    if not _GOLDEN:
        _GOLDEN.append(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                            'golden', 'mf_mp.npz')))
    f, k = _GOLDEN[0], c['id']
    assert f[k + '|sha'].tobytes().decode() == mf_cases.digest(c), 'stale fixture: ' + k
    v = f[k + '|value']
    return Est(Val(float(v[0]), float(v[1]), float(v[2])), Val(*f[k + '|grad']),
               Val(*f[k + '|lw']), None, None, None)


def case_errors(c, v, g, lw=None, lq_at=None):
    """Errors per class of a case of tests/mf_cases.py: (value, gradient[, log
    weights, (log q, the x it was read at)]) against the case's reference, which is
    asserted finite first.  A case with planted overflow rows (c['over']): the
    reference's log weight there lies below the double range, the result must be
    exactly -inf there and finite on every other row."""
    if c.get('golden'):
        ref = golden(c)
    else:
        ref = estimate(c['objective'], c['kind'], c['df'], c['target'], c['lam'], c['eps'],
                       c['alpha'])
    over = np.asarray(c.get('over', np.zeros(len(c['eps']), dtype=bool)))
    assert finite(ref.value) and finite(ref.grad), c['id']
    # finite in multiprecision everywhere; below the double range on planted rows only
    assert np.all(np.isfinite(ref.lw.hi[~over])) and np.all(ref.lw.hi[over] == -np.inf), c['id']
    D = c['D']
    eg = units(g, ref.grad)
    out = {'value': float(units(v, ref.value)), 'mean': float(eg[:D].max()),
           'log_sigma': float(eg[D:].max())}
    if lw is not None:
        got = np.asarray(lw)
        if over.any():
            assert np.all(got[over] == -np.inf), got[over]
            assert np.all(np.isfinite(got[~over]))
        fin = ~over
        out['log_w'] = float(units(got[fin], Val(ref.lw.hi[fin], ref.lw.lo[fin],
                                                 ref.lw.S[fin])).max())
    if lq_at is not None:
        lq, x = lq_at
        if c.get('golden'):
            lq, x = lq[:4], x[:4]      # log q at the result's own x: live, the first rows
        out['log_q'] = float(units(lq, logdensity(c['kind'], c['df'], c['lam'], x)).max())
    return out


# ---- the updates ------------------------------------------------------------------
def adagrad_update(lam, window, lr, eps):
    """lam (P,) doubles, window: the gradients of the last min(i + 1, W) steps,
    oldest first, the current one last ((cnt, P) doubles).  -> (Val lam', step (P,))."""
    window = np.atleast_2d(np.asarray(window, dtype=np.float64))
    with mp.workdps(DIGITS):
        new, S, steps = [], [], []
        for p in range(len(lam)):
            q = mp.fsum(mpf(float(g)) ** 2 for g in window[:, p])
            t = mpf(float(lr)) * mpf(float(window[-1, p])) / mp.sqrt(mpf(float(eps)) + q)
            v = mpf(float(lam[p])) - t
            new.append(v)
            S.append(abs(v) + abs(t))
            steps.append(float(t))
        return _val(new, S), np.array(steps)


def ia_update(which, lam, grads, lr, eps):
    """One RMSProp-IA ('rmsprop', vb.py:446-460) or Adam-IA ('adam', vb.py:611-623)
    update at step i = len(grads) - 1 from lam (P,) and the gradients of steps 0..i
    ((i + 1, P) doubles), the moment state rebuilt exactly from them:
      RMSProp  s = g^2 (i = 0) else .9 s + (1 - .9) g^2;  lam - lr g / sqrt(eps + s)
      Adam     v = .9 g^2, m = .9 g (i = 0) else .999 v + (1 - .999) g^2, .9 m + (1 - .9) g;
               lam - lr [m / (1 - .9^(i+2))] / sqrt(eps + v / (1 - .999^(i+2)))
    (.9, .999 and their complements are the doubles).  -> (Val lam', step (P,))."""
    grads = np.atleast_2d(np.asarray(grads, dtype=np.float64))
    i = grads.shape[0] - 1
    with mp.workdps(DIGITS):
        b9, b999 = mpf(0.9), mpf(0.999)
        new, S, steps = [], [], []
        for p in range(len(lam)):
            g = [mpf(float(v)) for v in grads[:, p]]
            if which == 'rmsprop':
                s = g[0] * g[0]
                for k in range(1, i + 1):
                    s = b9 * s + (1 - b9) * g[k] * g[k]
                t = mpf(float(lr)) * g[i] / mp.sqrt(mpf(float(eps)) + s)
            else:
                v, m = b9 * g[0] * g[0], b9 * g[0]
                for k in range(1, i + 1):
                    v = b999 * v + (1 - b999) * g[k] * g[k]
                    m = b9 * m + (1 - b9) * g[k]
                mh, vh = m / (1 - b9 ** (i + 2)), v / (1 - b999 ** (i + 2))
                t = mpf(float(lr)) * mh / mp.sqrt(mpf(float(eps)) + vh)
            nv = mpf(float(lam[p])) - t
            new.append(nv)
            S.append(abs(nv) + abs(t))
            steps.append(float(t))
        return _val(new, S), np.array(steps)


# Worst error of the numpy oracle (oracle/vb_oracle.py) per class over every case of
# tests/mf_cases.py, in units of 2^-53 S; measured by tests/test_oracle_mf_mp.py,
# which asserts twice these figures.  The GPU tests allow the device 8 times them.
MF_ORACLE_ERR = {
    'value': 1.65,        # pair/mixture/D64/N127/klvi/t8
    'mean': 4.37,
    'log_sigma': 1.72,
    'log_q': 3.54,
    'log_w': 1.83,        # block/isogauss/D2/N300/chivi neginf (finite rows at -1.76e308)
    'adagrad': 1.41,      # one step of adagrad_optimize, every W / eps of UPDATE_CASES
    'rmsprop': 1.47,      # one RMSProp-IA step, eps 1e-300
    'adam': 4.97,         # one Adam-IA step, eps 1e-6
    'transform': 2.40,
    'entropy': 0.15,
    'moments': 5.48,
}
