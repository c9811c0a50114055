"""Multiprecision restatement of notebooks/psis.py (mpmath, 50 digits) and the
seeded edge-case set of the PSIS kernels; shared by the CPU test that pins the
numpy oracle (tests/test_oracle_psis_mp.py) and the GPU tests of vb_psis.hip
(tests/test_gpu_psis_edges.py, and the child process it starts).

What counts as exact input.  The shifted column x = lw - max(lw) is one IEEE
subtraction per element that every implementation performs identically, so the
float64 x is the reference's input.  The order statistic at ascending rank
n - Mt - 1 (Mt = ceil(min(0.2 n, 3 sqrt(n / Reff)))), the cutoff
max(x_sel, log(DBL_MIN)) (the float64 logarithm: a threshold, not a result) and
the tail membership x > cutoff are exact comparisons of doubles.  From there on
everything is mpmath at 50 digits: exp, y = exp(x) - exp(cutoff), the quadrature
(b_j, k_j, L_j, w_j, the w >= 10 eps filter), b-hat, k, sigma, the smoothed
quantiles log(gpinv((i + .5) / n2, k, sigma) + exp(cutoff)), the clamp at 0 and
the log-sum-exp of the whole column.

Ties.  Equal values inside a tail are ordered by ascending original index, as the
device sorts them ((key, index) on the candidate route, a stable sort of the
index-ordered compaction on the radix route).  np.argsort's default sort does not
promise this, so a comparison of the numpy oracle with this reference on a tail
that holds a tie compares the smoothed weights as sorted multisets.

Error metric, as tests/targets_mp.py: err = |got - ref| / (2^-53 S), with
S = max(1, |ref|) for k, sigma and sumlogs, S = max(1, |ref_i|) per smoothed log
weight, and S = |ref_i| for gpinv (a product of well-conditioned factors: a plain
relative error).  References come back as double pairs (hi, lo), ref = hi + lo.
"""
import functools
import math
from collections import namedtuple

import numpy as np

try:
    import mpmath
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mpmath = None

DIGITS = 50
UNIT = 2.0 ** -53
EPS = float(np.finfo(float).eps)
CUTOFFMIN = float(np.log(np.finfo(float).tiny))
K_MIN = 1.0 / 3.0              # the double the reference compares k with
TAIL_MAX = 8192                # vb_psis.hip kTailMax

# The largest error of oracle/psis_oracle.py against this reference over CASES,
# GPD_CASES, GPINV_CASES and SUMLOGS_CASES, in units of 2^-53 S; measured by
# tests/test_oracle_psis_mp.py, which asserts each at 2x.
PSIS_ORACLE_ERR = {
    'k': 233.4,         # offset_8192 (y = exp(x) - exp(cutoff) cancels in double)
    'sigma': 4.371,
    'lw': 309.9,        # smoothed log weights (mixed_t3_a)
    'quad_ks': 9.170,   # gpdfitnew(return_quadrature=True): ks
    'quad_w': 157.8,    #   and w
    'gpinv': 31.66,     # relative
    'sumlogs': 0.5914,
}

# The tolerances tests/test_gpu_bounds_psis.py already holds the kernels to
# (rtol, atol); no bound of the edge tests is looser.
EXISTING_TOL = {'k': (1e-10, 1e-12), 'sigma': (1e-10, 1e-12), 'lw': (1e-11, 1e-11),
                'quad_ks': (1e-10, 1e-12), 'quad_w': (1e-10, 1e-12),
                'gpinv': (1e-13, 0.0), 'sumlogs': (1e-13, 0.0)}
MARGIN = 8.0


def available():
    return mpmath is not None


def device_bound(quantity, ref, S):
    """|got - ref| allowed of a kernel: 8 x PSIS_ORACLE_ERR in units of 2^-53 S,
    capped by the tolerance of the existing tests for that quantity."""
    rtol, atol = EXISTING_TOL[quantity]
    return np.minimum(MARGIN * PSIS_ORACLE_ERR[quantity] * UNIT * S, atol + rtol * np.abs(ref))


# ---- the select route a column takes on the device (host restatement) --------
def dkey(x):
    """vb_psis.hip dkey: the order-preserving 64-bit key of a double."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def tail_len(n, Reff=1.0):
    return int(np.ceil(min(0.2 * n, 3 * np.sqrt(n / Reff))))


def candidates(lw, Reff=1.0):
    """The fast select's candidate count: draws whose 22-bit key prefix is at or
    above the prefix of the order statistic at ascending rank n - Mt - 1."""
    n, Mt = len(lw), tail_len(len(lw), Reff)
    p22 = dkey(lw) >> np.uint64(42)
    sel = np.partition(p22, n - Mt - 1)[n - Mt - 1]
    return int(np.sum(p22 >= sel))


def route(lw, Reff=1.0):
    """'fast' (two-digit select, candidate sort), 'radix' (8-pass select, LDS tail
    sort) or 'radix+devsort' (8-pass select, device radix sort of the tail)."""
    if tail_len(len(lw), Reff) > TAIL_MAX:
        return 'radix+devsort'
    return 'fast' if candidates(lw, Reff) <= TAIL_MAX else 'radix'


def shifted_tail(lw, Reff=1.0):
    """The exact part: x = lw - max, the cutoff, the tail indices in ascending
    (value, index) order."""
    x = np.asarray(lw, dtype=np.float64) - np.max(lw)
    n, Mt = len(x), tail_len(len(x), Reff)
    xs = np.partition(x, n - Mt - 1)[n - Mt - 1]
    cut = max(float(xs), CUTOFFMIN)
    tidx = np.flatnonzero(x > cut)
    order = tidx[np.lexsort((tidx, x[tidx]))]
    return x, cut, order


# ---- the reference -----------------------------------------------------------
def _split(v):
    if mp.isinf(v) or mp.isnan(v):
        return float(v), 0.0
    hi = float(v)
    return hi, float(v - mpf(hi))


def _split_all(vs):
    hi = np.array([float(v) for v in vs])
    lo = np.array([0.0 if not math.isfinite(h) else float(v - mpf(h)) for v, h in zip(vs, hi)])
    return hi, lo


def _gpdfit(y):
    """gpdfitnew (psis.py:266-331) of the ascending mpf list y.
    Returns k, sigma, ks (kept), w (kept, normalised)."""
    n = len(y)
    m = 30 + math.isqrt(n)
    q = int(n / 4 + 0.5) - 1
    bs = [(1 - mp.sqrt(mpf(m) / (mpf(j) - mpf(1) / 2))) / (3 * y[q]) + 1 / y[-1]
          for j in range(1, m + 1)]
    kq = [sum(mp.log1p(-b * v) for v in y) / n for b in bs]
    L = [n * (mp.log(-(b / k)) - k - 1) for b, k in zip(bs, kq)]
    w = [1 / sum(mp.exp(Li - Lj) for Li in L) for Lj in L]
    keep = [j for j in range(m) if w[j] >= 10 * mpf(EPS)]
    tot = sum(w[j] for j in keep)
    wn = [w[j] / tot for j in keep]
    b = sum(bs[j] * v for j, v in zip(keep, wn))
    k = sum(mp.log1p(-b * v) for v in y) / n
    sigma = -k / b
    a = 10
    k = k * n / (n + a) + mpf(a) / 2 / (n + a)
    ks = [kq[j] * n / (n + a) + mpf(a) / 2 / (n + a) for j in keep]
    return k, sigma, ks, wn


def _gpinv(p, k, sigma):
    """gpinv (psis.py:334-376) at one p; k, sigma mpf."""
    if sigma <= 0:
        return mp.nan
    if p == 0:
        return mpf(0)
    if p == 1:
        return mp.inf if k >= 0 else -sigma / k
    if not 0 < p < 1:
        return mp.nan
    if abs(k) < mpf(EPS):
        return -mp.log1p(-p) * sigma
    return mp.expm1(-k * mp.log1p(-p)) / k * sigma


PsisRef = namedtuple('PsisRef', 'k_hi k_lo k_S sigma_hi sigma_lo sigma_S n2 tail lw_hi lw_lo lw_S '
                                'smoothed clamped')


def _psislw(lw, Reff):
    mp.dps = DIGITS
    x, cut, order = shifted_tail(lw, Reff)
    n, n2 = len(x), len(order)
    ecut = mp.exp(mpf(cut))
    smoothed, clamped = False, 0
    vals = {}                 # index -> smoothed value (mpf)
    if n2 <= 4:
        k, sigma = mp.inf, mp.nan
    else:
        y = [mp.exp(mpf(float(v))) - ecut for v in x[order]]
        k, sigma, _, _ = _gpdfit(y)
        if k >= mpf(K_MIN):
            smoothed = True
            for i, idx in enumerate(order):
                qv = mp.log(_gpinv((mpf(i) + mpf(1) / 2) / n2, k, sigma) + ecut)
                clamped += qv > 0
                vals[int(idx)] = qv if qv <= 0 else mpf(0)
    # log-sum-exp of the column: each distinct untouched value once
    mask = np.ones(n, dtype=bool)
    if smoothed:
        mask[order] = False
    u, cnt = np.unique(x[mask], return_counts=True)
    eu = {}
    tot = mpf(0)
    for v, c in zip(u, cnt):
        fv = float(v)
        eu[fv] = mpf(fv) if np.isfinite(fv) else -mp.inf
        if np.isfinite(fv):
            tot += int(c) * mp.exp(mpf(fv))
    for qv in vals.values():
        tot += mp.exp(qv)
    lse = mp.log(tot)
    out = [vals[i] - lse if i in vals else eu[float(x[i])] - lse for i in range(n)]
    k_hi, k_lo = _split(k)
    s_hi, s_lo = _split(sigma)
    lw_hi, lw_lo = _split_all(out)
    S = lambda v: max(1.0, abs(v)) if math.isfinite(v) else 1.0
    lw_S = np.where(np.isfinite(lw_hi), np.maximum(1.0, np.abs(lw_hi)), 1.0)
    return PsisRef(k_hi, k_lo, S(k_hi), s_hi, s_lo, S(s_hi), n2, order, lw_hi, lw_lo, lw_S,
                   smoothed, int(clamped))


GpdRef = namedtuple('GpdRef', 'k_hi k_lo k_S sigma_hi sigma_lo sigma_S ks_hi ks_lo ks_S w_hi w_lo w_S')


def _gpdfit_ref(x):
    mp.dps = DIGITS
    y = [mpf(float(v)) for v in np.sort(np.asarray(x, dtype=np.float64))]
    k, sigma, ks, w = _gpdfit(y)
    k_hi, k_lo = _split(k)
    s_hi, s_lo = _split(sigma)
    ks_hi, ks_lo = _split_all(ks)
    w_hi, w_lo = _split_all(w)
    return GpdRef(k_hi, k_lo, max(1.0, abs(k_hi)), s_hi, s_lo, max(1.0, abs(s_hi)),
                  ks_hi, ks_lo, np.maximum(1.0, np.abs(ks_hi)), w_hi, w_lo,
                  np.maximum(1.0, np.abs(w_hi)))


def gpinv_ref(p, k, sigma):
    """(hi, lo, S) of gpinv at every p; k, sigma the doubles given."""
    mp.dps = DIGITS
    hi, lo = _split_all([_gpinv(mpf(float(v)), mpf(float(k)), mpf(float(sigma))) for v in p])
    return hi, lo, np.abs(hi)


def sumlogs_ref(x):
    mp.dps = DIGITS
    v = mp.log(sum(mp.exp(mpf(float(t))) for t in np.ravel(x) if t != -np.inf))
    hi, lo = _split(v)
    return hi, lo, max(1.0, abs(hi))


def err(got, hi, lo, S):
    """|got - (hi + lo)| / (2^-53 S); 0 where got and the reference are the same
    infinity or both NaN, inf where only one of them is."""
    got, hi, lo, S = np.broadcast_arrays(np.asarray(got, dtype=float), hi, lo, S)
    e = np.empty(got.shape)
    fin = np.isfinite(hi)
    with np.errstate(invalid='ignore', divide='ignore'):
        e[fin] = np.abs((got[fin] - hi[fin]) - lo[fin]) / (UNIT * S[fin])
    e[fin & (S == 0) & (got == hi)] = 0.0          # an exact zero, met exactly
    same = (got[~fin] == hi[~fin]) | (np.isnan(got[~fin]) & np.isnan(hi[~fin]))
    e[~fin] = np.where(same, 0.0, np.inf)
    e[np.isnan(e)] = np.inf
    return e


# ---- the case set ------------------------------------------------------------
def _tie_block(n, copies, seed, n_top=500):
    """n_top distinct values in (1, 5), `copies` of exactly 1.0, the rest below 1,
    shuffled.  (The exponent keeps k clear of 1/3: evenly spaced top values put
    it within 2e-4 of 1/3 at n_top = 6000.)"""
    rs = np.random.RandomState(seed)
    top = 1.0 + 4.0 * ((np.arange(n_top) + rs.uniform(0.05, 0.95, n_top)) / n_top) ** 1.05
    low = 1.0 - rs.gamma(2.0, 1.5, n - n_top - copies) - 1e-3
    x = np.concatenate([top, np.full(copies, 1.0), low])
    rs.shuffle(x)
    return x


def _offset(n, seed=None):
    rs = np.random.RandomState(1000 + n if seed is None else seed)
    return -1.0e6 + 1.3 * rs.standard_t(3, n)


def _few_above(n_above, seed):
    """n = 64, Mt = 13: ties at the order statistic leave n_above draws in the tail."""
    rs = np.random.RandomState(seed)
    x = np.concatenate([1.0 + rs.uniform(0.2, 3.0, n_above), np.full(24 - n_above, 1.0),
                        1.0 - rs.uniform(0.1, 6.0, 40)])
    rs.shuffle(x)
    return x


def _clamped():
    rs = np.random.RandomState(41)
    x = np.concatenate([1.5 * rs.standard_t(3, 60), -1000.0 + rs.randn(2000)])
    rs.shuffle(x)
    return x


def _with_neg_inf():
    rs = np.random.RandomState(43)
    x = rs.standard_t(3, 3000)
    x[::7] = -np.inf
    return x


def _ties_in_tail():
    rs = np.random.RandomState(47)
    return np.round(1.6 * rs.standard_t(2.5, 3000), 1)


# seeds of the columns whose k the reference places within 1e-3 of 1/3, one on
# either side (searched on the CPU with the numpy oracle, then confirmed by _psislw)
NEAR_THIRD_SEEDS = {'below': 8, 'above': 142}


def _near_third(seed):
    return np.random.RandomState(seed).exponential(1.0 / 3.0, 1000)


# name -> (builder, Reff).  Every array is seeded; build with case(name).
_BUILDERS = {
    'offset_4096': (lambda: _offset(4096), 1.0),
    'offset_8192': (lambda: _offset(8192), 1.0),
    'offset_8193': (lambda: _offset(8193), 1.0),
    'offset_20000': (lambda: _offset(20000, 21002), 1.0),   # (seed: no draw past -1e6 + 64)
    'tie_block_9000': (lambda: _tie_block(40000, 9000, 21), 1.0),
    'tie_block_40': (lambda: _tie_block(40000, 40, 22), 1.0),
    'n2_4': (lambda: _few_above(4, 31), 1.0),
    'n2_5': (lambda: _few_above(5, 32), 1.0),
    'all_equal_100': (lambda: np.full(100, -3.7), 1.0),
    'all_equal_9000': (lambda: np.full(9000, 2.25), 1.0),
    'clamped_cutoff': (_clamped, 1.0),
    'neg_inf': (_with_neg_inf, 1.0),
    'light_tail': (lambda: np.log1p(np.random.RandomState(51).uniform(size=2000)), 1.0),
    'heavy_tail': (lambda: 1.1 * np.random.RandomState(52).standard_t(2.5, 2000), 1.0),
    'near_third_below': (lambda: _near_third(NEAR_THIRD_SEEDS['below']), 1.0),
    'near_third_above': (lambda: _near_third(NEAR_THIRD_SEEDS['above']), 1.0),
    'ties_in_tail': (_ties_in_tail, 1.0),
    'mixed_t3_a': (lambda: 1.3 * np.random.RandomState(61).standard_t(3, 20000) - 2.0, 1.0),
    'mixed_t3_b': (lambda: 0.8 * np.random.RandomState(62).standard_t(3, 20000) + 4.0, 1.0),
    'mixed_tie_block': (lambda: _tie_block(20000, 9000, 63, n_top=300), 1.0),
}
# the cases given to mpmath (each also runs on the GPU)
CASES = tuple(_BUILDERS)
MIXED = ('mixed_t3_a', 'offset_20000', 'mixed_t3_b', 'mixed_tie_block')

# cases compared with the numpy oracle only (tails of 8192 draws and more)
_BIG_BUILDERS = {
    'mt_8192': (lambda: 1.2 * np.random.RandomState(71).standard_t(4, 40960), 1e-3),
    'mt_8193': (lambda: 1.2 * np.random.RandomState(72).standard_t(4, 40961), 1e-3),
    'mt_8193_tie_block': (lambda: _tie_block(40961, 3000, 73, n_top=6000), 1e-3),
    'quad_256': (lambda: 1.2 * np.random.RandomState(74).standard_t(4, 257640), 5e-4),
    'quad_257': (lambda: 1.2 * np.random.RandomState(75).standard_t(4, 257645), 5e-4),
}
BIG_CASES = tuple(_BIG_BUILDERS)
# the cases the GPU test runs down both select routes (a child process with
# VIABEL_AMD_PSIS_FAST_SELECT=0 against the default)
BOTH_ROUTES = ('offset_4096', 'offset_8192', 'offset_8193', 'offset_20000', 'tie_block_9000',
               'tie_block_40', 'mt_8192', 'mt_8193', 'mt_8193_tie_block')

# the route each case takes with the fast select enabled (asserted on the host)
ROUTES = {
    'offset_4096': 'fast', 'offset_8192': 'fast', 'offset_8193': 'radix', 'offset_20000': 'radix',
    'tie_block_9000': 'radix', 'tie_block_40': 'fast', 'n2_4': 'fast', 'n2_5': 'fast',
    'all_equal_100': 'fast', 'all_equal_9000': 'radix', 'clamped_cutoff': 'fast',
    'neg_inf': 'fast', 'light_tail': 'fast', 'heavy_tail': 'fast', 'near_third_below': 'fast',
    'near_third_above': 'fast', 'ties_in_tail': 'fast', 'mixed_t3_a': 'fast',
    'mixed_t3_b': 'fast', 'mixed_tie_block': 'radix',
    'mt_8192': 'radix', 'mt_8193': 'radix+devsort', 'mt_8193_tie_block': 'radix+devsort',
    'quad_256': 'radix+devsort', 'quad_257': 'radix+devsort',
}


@functools.lru_cache(maxsize=None)
def _case(name):
    build, reff = _BUILDERS[name] if name in _BUILDERS else _BIG_BUILDERS[name]
    a = np.asarray(build(), dtype=np.float64)
    a.setflags(write=False)
    return a, reff


def case(name):
    """(log weights (read-only), Reff) of a named case."""
    return _case(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The 50-digit reference of a named case of CASES; computed once per process."""
    lw, reff = case(name)
    return _psislw(lw, reff)


def psislw_reference(lw, Reff=1.0):
    return _psislw(np.asarray(lw, dtype=np.float64), Reff)


# gpdfitnew directly: name -> array (any order)
def _gpd_builders():
    rs = np.random.RandomState(81)
    p700 = rs.pareto(3.0, 700)
    rep = np.round(rs.pareto(2.0, 700) + 0.05, 1)
    return {
        'n2': np.array([0.7, 0.2]),
        'n3': np.array([1.5, 0.25, 0.6]),
        'n5': np.array([0.9, 0.1, 2.5, 0.4, 0.35]),
        'unsorted_700': p700,
        'repeated_700': rep,
    }


GPD_CASES = ('n2', 'n3', 'n5', 'unsorted_700', 'repeated_700')
# compared with the numpy oracle only
GPD_BIG = {'n8192': (82, 8192), 'n8193': (83, 8193), 'm256': (84, 51528), 'm257': (85, 51529)}


@functools.lru_cache(maxsize=None)
def gpd_case(name):
    if name in GPD_BIG:
        seed, n = GPD_BIG[name]
        a = np.random.RandomState(seed).pareto(3.0, n)
    else:
        a = _gpd_builders()[name]
    a = np.asarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gpd_reference(name):
    return _gpdfit_ref(gpd_case(name))


# gpinv: p grid (with both ends) and (k, sigma) on every branch
GPINV_P = np.concatenate([[0.0, 1.0, 2.0 ** -60, 1e-9, 1.0 - 2.0 ** -53],
                          (np.arange(40) + 0.5) / 40])
GPINV_CASES = ((0.4, 1.3), (-0.3, 2.0), (1e-18, 0.7), (1.0 / 3.0, 0.05), (1.27, 3e-3), (0.7, 40.0),
               (-2.5, 1.0))


def _sumlogs_builders():
    rs = np.random.RandomState(91)
    return {
        'spread': rs.randn(3000) * 20,
        'offset': -1.0e6 + rs.randn(513) * 3,
        'one_dominates': np.concatenate([[700.0], rs.randn(255) - 50.0]),
        'equal': np.full(1000, -12.5),
        'two': np.array([0.1, -0.3]),
    }


SUMLOGS_CASES = ('spread', 'offset', 'one_dominates', 'equal', 'two')


@functools.lru_cache(maxsize=None)
def sumlogs_case(name):
    a = _sumlogs_builders()[name]
    a.setflags(write=False)
    return a


# ---- what each case claims of its data (asserted on the host before a GPU call) --
# name -> (n, Mt, n2)
SHAPES = {
    'offset_4096': (4096, 192, 192), 'offset_8192': (8192, 272, 272),
    'offset_8193': (8193, 272, 272), 'offset_20000': (20000, 425, 425),
    'tie_block_9000': (40000, 600, 500), 'tie_block_40': (40000, 600, 600),
    'n2_4': (64, 13, 4), 'n2_5': (64, 13, 5), 'all_equal_100': (100, 20, 0),
    'all_equal_9000': (9000, 285, 0), 'clamped_cutoff': (2060, 137, 60),
    'neg_inf': (3000, 165, 165), 'light_tail': (2000, 135, 135), 'heavy_tail': (2000, 135, 135),
    'near_third_below': (1000, 95, 95), 'near_third_above': (1000, 95, 95),
    'ties_in_tail': (3000, 165, 161), 'mixed_t3_a': (20000, 425, 425),
    'mixed_t3_b': (20000, 425, 425), 'mixed_tie_block': (20000, 425, 300),
    'mt_8192': (40960, 8192, 8192), 'mt_8193': (40961, 8193, 8193),
    'mt_8193_tie_block': (40961, 8193, 6000),
    'quad_256': (257640, 51528, 51528), 'quad_257': (257645, 51529, 51529),
}
# tails that hold equal values (ordered by index; everywhere else the tail's values
# are distinct and its order is the only one)
TIED_TAILS = ('tie_block_40', 'ties_in_tail')


def check_case(name):
    """Assert on the host every property the case is there for."""
    lw, reff = case(name)
    n, Mt, n2 = SHAPES[name]
    x, cut, order = shifted_tail(lw, reff)
    assert (len(lw), tail_len(n, reff), len(order)) == (n, Mt, n2), name
    assert not np.any(np.isnan(lw)) and not np.any(lw == np.inf)
    assert route(lw, reff) == ROUTES[name], name
    cand = candidates(lw, reff)
    distinct = len(np.unique(x[order])) == n2
    assert distinct == (name not in TIED_TAILS), name
    if name.startswith('offset_'):
        assert len(np.unique(dkey(lw) >> np.uint64(42))) == 1 and cand == n
        # (a wave of sel_compact_kernel reads 512 elements of a column of >= 2048,
        # all candidates here: past kCompactWaveCap = 128 hits at n = 4096, 8192)
    if 'tie_block' in name:
        copies = int(np.sum(lw == 1.0))
        xs = np.sort(lw)[n - Mt - 1]
        assert copies in (40, 3000, 9000) and (xs == 1.0) == (name != 'tie_block_40')
        assert (cand > TAIL_MAX) == (copies + n2 > TAIL_MAX)
        assert np.all(lw[order] > 1.0) or name == 'tie_block_40'
    if name in ('n2_4', 'n2_5'):
        assert cut == np.sort(x)[n - Mt - 1] and np.sum(x == cut) == 24 - n2
    if name.startswith('all_equal'):
        assert np.all(lw == lw[0]) and cut == 0.0
    if name == 'clamped_cutoff':
        assert cut == CUTOFFMIN and np.sort(x)[n - Mt - 1] < CUTOFFMIN
    if name == 'neg_inf':
        assert np.array_equal(np.flatnonzero(np.isinf(lw)), np.arange(0, n, 7))
    if name in ('mt_8192', 'mt_8193'):
        assert n2 == Mt
    if name == 'mt_8193_tie_block':
        assert n2 < Mt
    if name.startswith('quad_'):
        assert 30 + math.isqrt(n2) == int(name[5:])
    if name in CASES and available():
        ref = reference(name)
        assert ref.n2 == n2
        if name == 'n2_4' or name.startswith('all_equal'):
            assert ref.k_hi == np.inf and not ref.smoothed
        if name == 'n2_5':
            assert np.isfinite(ref.k_hi)
        if name == 'clamped_cutoff':
            assert ref.k_hi > 1.0 and ref.smoothed
        if name == 'light_tail':
            assert ref.k_hi < -0.5 and not ref.smoothed
        if name == 'heavy_tail':
            assert ref.k_hi > K_MIN and ref.smoothed
        if name == 'near_third_below':
            assert K_MIN - 1e-3 < ref.k_hi < K_MIN and not ref.smoothed
        if name == 'near_third_above':
            assert K_MIN < ref.k_hi < K_MIN + 1e-3 and ref.smoothed
        if 'tie_block' in name:
            assert ref.k_hi > K_MIN + 0.05 and ref.smoothed and ref.clamped > 1   # q > 0 -> 0
