"""Multiprecision restatement of the four built-in targets (mpmath, 50 digits),
their condition sums, and the off-centre edge point set; shared by the CPU test
that pins the numpy oracle (tests/test_oracle_targets_mp.py) and the GPU tests of
the target kernels (tests/test_gpu_targets_edges.py).

Written from the definitions in the docstring of oracle/targets_oracle.py:

  isogauss   log p = sum_d [-x_d^2/2 - log(2 pi)/2]
  mixture    log p = sum_d [log(exp(a_d) + exp(b_d)) - log 2],
             a = -(x+2)^2/2 - log(2 pi)/2, b = -(x-2)^2/2 - log(2 pi)/2
  funnel     v = x_1 ~ N(0, 1.35^2), every other x_d ~ N(0, exp(v)^2)
  eight_schools_ncp   -(mu/5)^2/2 - log1p((tau/5)^2) + u - sum th_j^2/2
                      - sum r_j^2/2,  tau = exp(u), r_j = (y_j - mu - tau th_j)/sigma_j

Error metric.  Beside each result stands its condition sum S: the sum of the
absolute values of the terms that are added to form it (for a result that is a
single product, S = |result|).  A comparison measures

    err = |got - ref| / (2^-53 S)

which stays O(1) for a correct double evaluation wherever the terms cancel (the
mixture's gradient -(x+2) + 4 w at x ~ 0, the funnel's d/dx_1 at z ~ 1); a plain
relative error does not.  The terms, per result:

  isogauss  lp: x^2/2, log(2pi)/2 per d;  g_d = -x_d: S = |x_d|
  mixture   lp: (|x|-2)^2/2, log(2pi)/2, log1p(exp(-4|x|)), log 2 per d
            g_d = -x - 2 + 4 w: |x|, 2, 4 w
  funnel    lp: (v/1.35)^2/2, log 1.35, log(2pi)/2; z_d^2/2, |v|, log(2pi)/2 per d != 1
            g_1: |v|/1.35^2; z_d^2, 1 per d != 1      g_d = -x_d exp(-2v): S = |g_d|
  8-schools lp: (mu/5)^2/2, log1p(w), |u|; th_j^2/2, r_j^2/2 per j
            g_mu: |mu|/25; |r_j|/sigma_j     g_u: 2w/(1+w), 1; |r_j tau th_j|/sigma_j
            g_th_j: |th_j|, |r_j| tau/sigma_j

References come back as a double pair (hi, lo), ref = hi + lo to ~2^-106, so the
reference's own rounding does not enter the error.
"""
import functools
from collections import namedtuple

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mpmath = None

DIGITS = 50
UNIT = 2.0 ** -53

ES_Y = (28, 8, -3, 7, -1, 1, 18, 12)
ES_SIGMA = (15, 10, 16, 11, 9, 11, 10, 18)

# lp_*: (n,), g_*: (n, D); ref = hi + lo, S the condition sum
Ref = namedtuple('Ref', 'lp_hi lp_lo lp_S g_hi g_lo g_S')


def available():
    return mpmath is not None


def _split(v):
    hi = float(v)
    return hi, float(v - mpf(hi))


# ---- per-coordinate forms of the separable targets --------------------------
def _iso1(x):
    half_l2pi = mp.log(2 * mp.pi) / 2
    q = x * x / 2
    return -q - half_l2pi, q + half_l2pi, -x, abs(x)


def _mix1(x):
    half_l2pi = mp.log(2 * mp.pi) / 2
    a = -(x + 2) ** 2 / 2 - half_l2pi
    b = -(x - 2) ** 2 / 2 - half_l2pi
    e = mp.exp(-abs(a - b))
    l1 = mp.log1p(e)
    lp = max(a, b) + l1 - mp.log(2)
    w = 1 / (1 + mp.exp(a - b))
    g = -(x + 2) + 4 * w
    s_lp = (abs(x) - 2) ** 2 / 2 + half_l2pi + l1 + mp.log(2)
    return lp, s_lp, g, abs(x) + 2 + 4 * w


def _separable(one, x):
    """Rows of a separable target: each distinct coordinate value is evaluated
    once, rows are summed in multiprecision."""
    n, D = x.shape
    uniq, inv = np.unique(x, return_inverse=True)
    inv = inv.reshape(x.shape)
    vals = [one(mpf(float(v))) for v in uniq]
    g_hi, g_lo, g_S = np.empty(len(uniq)), np.empty(len(uniq)), np.empty(len(uniq))
    for k, v in enumerate(vals):
        g_hi[k], g_lo[k] = _split(v[2])
        g_S[k] = float(v[3])
    lp_hi, lp_lo, lp_S = np.empty(n), np.empty(n), np.empty(n)
    for r in range(n):
        lp_hi[r], lp_lo[r] = _split(mp.fsum(vals[k][0] for k in inv[r]))
        lp_S[r] = float(mp.fsum(vals[k][1] for k in inv[r]))
    return Ref(lp_hi, lp_lo, lp_S, g_hi[inv], g_lo[inv], g_S[inv])


def _funnel_row(xs):
    """One funnel row at multiprecision coordinates xs: (lp, S_lp, [g_d], [S_d])."""
    D = len(xs)
    s0 = mpf('1.35')
    half_l2pi = mp.log(2 * mp.pi) / 2
    v = xs[1]
    zv = v / s0
    lp = -zv * zv / 2 - mp.log(s0) - half_l2pi
    s_lp = zv * zv / 2 + abs(mp.log(s0)) + half_l2pi
    gv = -v / s0 ** 2
    s_gv = abs(gv)
    inv_s2 = mp.exp(-2 * v)
    g, gS = [None] * D, [None] * D
    for d in range(D):
        if d == 1:
            continue
        xd = xs[d]
        z2 = xd * xd * inv_s2
        lp += -z2 / 2 - v - half_l2pi
        s_lp += z2 / 2 + abs(v) + half_l2pi
        gv += z2 - 1
        s_gv += z2 + 1
        g[d] = -xd * inv_s2
        gS[d] = abs(g[d])
    g[1], gS[1] = gv, s_gv
    return lp, s_lp, g, gS


def _es_row(xs):
    """One eight-schools row at multiprecision coordinates xs, as _funnel_row."""
    assert len(xs) == 10
    mu, u = xs[0], xs[1]
    tau = mp.exp(u)
    w = (tau / 5) ** 2
    l1 = mp.log1p(w)
    lp = -(mu / 5) ** 2 / 2 - l1 + u
    s_lp = (mu / 5) ** 2 / 2 + l1 + abs(u)
    gmu = -mu / 25
    s_gmu = abs(gmu)
    gu = -2 * w / (1 + w) + 1
    s_gu = 2 * w / (1 + w) + 1
    g, gS = [None] * 10, [None] * 10
    for j in range(8):
        th = xs[2 + j]
        sg = mpf(ES_SIGMA[j])
        res = (ES_Y[j] - mu - tau * th) / sg
        lp += -th * th / 2 - res * res / 2
        s_lp += th * th / 2 + res * res / 2
        gmu += res / sg
        s_gmu += abs(res / sg)
        gu += res * tau * th / sg
        s_gu += abs(res * tau * th / sg)
        g[2 + j] = -th + res * tau / sg
        gS[2 + j] = abs(th) + abs(res * tau / sg)
    g[0], gS[0], g[1], gS[1] = gmu, s_gmu, gu, s_gu
    return lp, s_lp, g, gS


def _sep_row(one):
    def row(xs):
        vals = [one(x) for x in xs]
        return (mp.fsum(v[0] for v in vals), mp.fsum(v[1] for v in vals),
                [v[2] for v in vals], [v[3] for v in vals])
    return row


def _rows(row, x, D_fixed=None):
    n, D = x.shape
    assert D_fixed is None or D == D_fixed
    out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
    for r in range(n):
        lp, s_lp, g, gS = row([mpf(float(v)) for v in x[r]])
        out.lp_hi[r], out.lp_lo[r] = _split(lp)
        out.lp_S[r] = float(s_lp)
        for d in range(D):
            out.g_hi[r, d], out.g_lo[r, d] = _split(g[d])
            # a gradient entry that is one product carries S = |the rounded entry|
            out.g_S[r, d] = abs(out.g_hi[r, d]) if gS[d] == abs(g[d]) else float(gS[d])
    return out


def _funnel(x):
    return _rows(_funnel_row, x)


def _eight_schools(x):
    return _rows(_es_row, x, 10)


# one row at multiprecision coordinates (a list of mpf, inside mp.workdps(DIGITS)):
# (lp, S_lp, [g_d], [S_d]) -- for references whose x is itself a multiprecision result
ROW = {'isogauss': _sep_row(_iso1), 'mixture': _sep_row(_mix1), 'funnel': _funnel_row,
       'eight_schools_ncp': _es_row}


_EVAL = {'isogauss': lambda x: _separable(_iso1, x), 'mixture': lambda x: _separable(_mix1, x),
         'funnel': _funnel, 'eight_schools_ncp': _eight_schools}


def reference(target, x):
    """Ref of `target` at the rows of x (n, D), evaluated with DIGITS digits."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    with mp.workdps(DIGITS):
        return _EVAL[target](x)


def errors(lp, g, ref):
    """Errors of a double evaluation (lp (n,), g (n, D)) in units of 2^-53 S:
    (per row, per gradient entry).  Where S = 0 the reference is exactly 0 and so
    must the result be (error 0, or inf)."""
    def units(got, hi, lo, S):
        got = np.asarray(got, dtype=np.float64)
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            d = np.abs((got - hi) - lo)
            e = np.where(S > 0, d / (UNIT * S), np.where(d == 0, 0.0, np.inf))
        return np.where(np.isfinite(got), e, np.inf)
    return units(lp, ref.lp_hi, ref.lp_lo, ref.lp_S), units(g, ref.g_hi, ref.g_lo, ref.g_S)


# ---- the edge point set -----------------------------------------------------
# per-coordinate centres of the separable targets: +-186.4 is where |4x| reaches
# exp_fast's -746 clamp, at +-177.5 exp(-|4x|) is subnormal
SEP_CENTRES = (0.0, 1e-9, 0.5, 3.0, 10.0, 40.0, 150.0, 177.5, 186.4)
FUNNEL_X1 = (-12.0, -6.0, -2.0, 0.0, 2.0, 5.0, 9.0)
FUNNEL_DIMS = (2, 10, 16, 17, 40, 512)
# the separable kernels: one wave per row below 512 columns (one and two passes of
# its 64 lanes), one 1024-thread block per row from 512 on
SEP_DIMS = (3, 70, 512)
ES_LOG_TAU = (-40.0, -8.0, -2.0, 0.0, 1.6, 4.0, 20.0)
ES_MU = (0.0, 30.0, -30.0)
# rows beside EightSchools::lp_tab's switch w = (tau / 5)^2 = 2^1000.  352 and 354.5
# both lie above it (w = 2^1011, 2^1018: the switch is at log tau = (1000 log 2 +
# log 25) / 2 = 348.183); 348.0 and 348.4 are its two sides (w = 2^999.5, 2^1000.6)
ES_SWITCH = (352.0, 354.5, 348.0, 348.4)
SEED = 20240519
JITTER = 1e-3          # relative (absolute at a centre of 0)
RANDOM_SHARE = 0.1     # rows kept at the standard-normal points of the older tests


def _jit(rs, c, k):
    """k jittered copies of centre c: c (1 + JITTER u), u uniform in (-1, 1); a
    centre of 0 moves by JITTER u."""
    u = rs.uniform(-1.0, 1.0, size=k)
    return c * (1.0 + JITTER * u) if c != 0.0 else JITTER * u


def sep_pool(copies=24):
    """Coordinate values of the separable targets: 0 exactly, and `copies` jittered
    values at +-c for every other centre, in centre order."""
    rs = np.random.RandomState(SEED)
    out = [np.zeros(1)]
    for c in SEP_CENTRES[1:]:
        out += [_jit(rs, c, copies), _jit(rs, -c, copies)]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def edge_points(target, D):
    """The edge rows of (target, D), at most 600, the last RANDOM_SHARE of them
    standard normal."""
    rs = np.random.RandomState(SEED + 1000 * sorted(_EVAL).index(target) + D)
    if target in ('isogauss', 'mixture'):
        pool = sep_pool()
        # rows of one centre each (the pool in centre order, padded with 0), then
        # rows that mix every magnitude
        n_own = -(-pool.size // D)
        own = np.zeros(n_own * D)
        own[:pool.size] = pool
        n_mix = max(8, min(200, 20000 // D) - n_own)
        rows = [own.reshape(n_own, D), rs.choice(pool, size=(n_mix, D))]
    elif target == 'funnel':
        k = 60 if D <= 40 else 8
        rows = []
        for c in FUNNEL_X1:
            blk = rs.randn(k + 1, D)
            blk[:k, 1] = _jit(rs, c, k)
            blk[0, 1] = c                       # the centre itself once
            blk[k, :] = 0.0                     # one row with every other coordinate 0
            blk[k, 1] = c
            rows.append(blk)
    else:
        rows = []
        for lt in ES_LOG_TAU:
            for m in ES_MU:
                blk = rs.randn(20, 10)
                blk[:, 0] = _jit(rs, m, 20) if m != 0.0 else 0.0
                blk[:, 1] = _jit(rs, lt, 20)
                blk[0, 1] = lt
                rows.append(blk)
        rows.append(es_switch_rows())
    x = np.concatenate(rows)
    n_rand = max(1, int(round(RANDOM_SHARE * x.shape[0] / (1.0 - RANDOM_SHARE))))
    x = np.concatenate([x, rs.randn(n_rand, x.shape[1])])
    assert x.shape[0] <= 600 and np.all(np.isfinite(x))
    x.setflags(write=False)
    return x


def es_switch_rows():
    """Per log tau of ES_SWITCH and mu in {0, 30}: one row with theta_tilde standard
    normal (log p ~ -tau^2: finite, the log1p far below its rounding) and one with
    theta_tilde = 0, where log1p(w) ~ 700 is a leading term of log p."""
    rs = np.random.RandomState(SEED + 7)
    rows = []
    for lt in ES_SWITCH:
        for m in (0.0, 30.0):
            a = rs.randn(10)
            b = np.zeros(10)
            a[0] = b[0] = m
            a[1] = b[1] = lt
            rows += [a, b]
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def edge_reference(target, D):
    """(points, Ref) of (target, D), computed once per process and shared."""
    x = edge_points(target, D)
    ref = reference(target, x)
    for a in ref:
        a.setflags(write=False)
    return x, ref


CASES = ([('isogauss', D) for D in SEP_DIMS] + [('mixture', D) for D in SEP_DIMS]
         + [('funnel', D) for D in FUNNEL_DIMS] + [('eight_schools_ncp', 10)])

# Worst error of the numpy oracle (oracle/targets_oracle.py) over the edge set of
# every D of a target, value and gradient entries together, in units of 2^-53 S;
# measured by tests/test_oracle_targets_mp.py, which asserts twice these figures.
# The GPU tests allow the kernels 8 times them.
ORACLE_ERR = {
    'isogauss': 6.13,            # value at D = 70 (3.25 at D = 3, 1.96 at 512); gradient exact
    'mixture': 6.94,             # value at D = 70 (3.40, 2.29); gradient 1.15
    'funnel': 5.55,              # value at D = 40; gradient 5.27 (D = 40), 4.44 (D = 2)
    # d/d theta_j = -th_j + r_j tau / sigma_j at mu = 30, log tau = 4, where y_j - mu -
    # tau th_j itself cancels (a sum inside a term: S does not see it); value 4.48
    'eight_schools_ncp': 9.89,
}
