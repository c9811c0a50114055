"""Multiprecision restatement (mpmath, 50 digits) of the reductions behind
viabel_amd.bounds (viabel/bounds.py:127-192, np.cov / np.average) and the seeded
edge-case set of vb_bounds.hip; shared by the CPU test that pins the numpy oracle
(tests/test_oracle_bounds_mp.py) and the GPU tests (tests/test_gpu_bounds_edges.py,
and the child process it starts).

What counts as exact input.  The float64 log weights, samples, weights, alpha and
the given log_norm_bound are exact.  max(lw) is a comparison of doubles and is
compared exactly.  Everything else is mpmath at 50 digits: lw_i - max,
r_i = exp(alpha (lw_i - max)), the means, the population standard deviations
divided by sqrt(n), cubo = log(mean_r) / alpha + max, d = alpha / (alpha - 1)
(cubo - lnb); the column means, the centred powers and products; the weights
w_i = exp(lw_i - max lw) of the log-weighted covariance (not rounded to double,
and not flushed to zero where the double underflows).

Non-finite log weights follow numpy (bounds.py:142-192 evaluated by numpy):
  any -inf (not all)  mean_lw = -inf, se_lw = nan (x - mean holds -inf - -inf),
                      r_i = 0 for those draws, mean_r and se_r finite,
                      d = +inf without a log_norm_bound, finite with one;
  all -inf            max = -inf, lw - max = nan: mean_r, se_r, d nan;
                      mean_lw = -inf, se_lw = nan;
  any +inf or nan     lw - max holds a nan: every value but max and mean_lw is nan
                      (max is +inf, or nan as np.max propagates it; mean_lw is
                      +inf when the vector holds +inf and neither nan nor -inf).
With a log_norm_bound the device does not compute se_lw and returns nan for it;
the reference returns the value regardless and the tests skip that comparison.

Large sizes by multiset.  The reference is computed from np.unique(lw) and its
counts, so a case of ten million draws over 32 distinct doubles costs 32
exponentials.  Cases past 65537 elements are built that way (_multiset: the
values repeated by seeded counts, in a seeded permutation).

Error metric, as tests/psis_mp.py: err = |got - ref| / (2^-53 S), references as
double pairs (hi, lo).  S comes from the inputs and the reference alone:
  mean_lw   S = max |lw_i| over the finite lw_i
  mean_r    S = |ref|
  se_r      S = max(|ref|, mean_r / sqrt(n))
  se_lw     S = max(|ref|, max |lw| / sqrt(n))
  d_alpha   S = alpha / (alpha - 1) max(1, |max|, |lnb|, |log mean_r| / alpha)
  log max   exact
  c2, c4    S = sum over columns d of c_{p,d} kappa_d, c_{p,d} the column's own
            centred moment and kappa_d = max(1, max |x_d| / sd(x_d)) the
            cancellation in x - mean (a constant column has c_{p,d} = 0 and adds 0).
            (|ref| kappa with one kappa over all columns would be infinite as soon
            as one column is constant, and would let a well-scaled column hide
            behind an offset one; the per-column sum is never larger.)
  cov_ij    S = sqrt(ref_ii ref_jj) max(kappa_i, kappa_j), kappa from the rows of
            non-zero (double) weight and the weighted population sd
  mean_w    S = max |x| over the rows of non-zero weight
A scale of 0 (one row, a one-hot weight) asks for the exact value.

Constant vectors.  se_r of a constant vector is exactly 0 in every form (r = 1).
se_lw is exactly 0 whenever every partial sum of the vector is exact, which the
case 'const' arranges (-3.75: k * -3.75 is a double for every k < 2^50), so an
exact 0 is asked of every summation order.  At a value such as -3.7 the mean of
2049 copies is itself rounded in numpy as in any tree, and the tiny non-zero
se_lw that follows is held to the bound only ('const_inexact').
"""
import functools
import math

import numpy as np

from tests.psis_mp import DIGITS, UNIT, err, _split      # noqa: F401  (err: shared metric)

try:
    import mpmath
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mpmath = None

# vb_bounds.hip / vb_internal.hpp constants the cases are placed around
DIV_TWO_PASS_MIN_N = 1 << 16   # kDivTwoPassMinN: three-pass below, Welford from here on
RED_PER_BLOCK = 2048           # red_grid: one block per 2048 elements ...
RED_BLOCKS = 1024              # ... clamped at kRedBlocks
DIV2_PER_BLOCK = 8192          # div2_grid: 256 threads x kDivPer = 32
COL_CHUNK_ROWS = 4096          # col_chunks: rows per chunk ...
COL_CHUNKS_MAX = 512           # ... clamped at 512 chunks
COV_D_MAX = 64                 # kCovDMax: pair kernels up to here, the MFMA GEMM above

MARGIN = 8.0
QUANTITIES = ('d', 'mean_r', 'se_r', 'mean_lw', 'se_lw')
OUT7 = ('d', 'lnb', 'mean_r', 'se_r', 'mean_lw', 'se_lw', 'max')

# The largest error of the numpy oracle (oracle/bounds_oracle.py divergence_stats and
# wasserstein_bounds' moments; np.cov / np.average) against this reference over
# DIV_CASES, MOMENT_CASES and COV_CASES, in units of 2^-53 S, with the case that
# produced it; measured by tests/test_oracle_bounds_mp.py, which asserts each at 2x.
BOUNDS_ORACLE_ERR = {
    'd': (4.325, 'const_inexact_65537'),
    'mean_r': (9.974, 'normal_8392705_a2'),
    'se_r': (3.081, 'normal_8392705_a1.5'),
    'mean_lw': (4.325, 'const_inexact_65537'),
    'se_lw': (4.325, 'const_inexact_65537'),
    'c2': (1.644, 'rows_clamp_d2'),
    'c4': (1.596, 'n2_d1'),
    # rows_clamp_d2 alone: numpy's x.mean(axis=0) adds 2 097 153 rows in sequence, and
    # the shifted mean enters c4 in first order; kept apart so that every other case
    # keeps the tight figure
    'c4_rows_clamp': (3961.0, 'rows_clamp_d2'),
    'cov': (4.573, 'logw_1400_n255_d65'),
    'mean_w': (6.875, 'offset_n255_d65'),
}

# The tolerances tests/test_gpu_bounds_psis.py and tests/test_gpu_switches.py already
# hold the kernels to (rtol, atol); no bound of the edge tests is looser.
EXISTING_TOL = {'d': (1e-9, 1e-12), 'mean_r': (1e-12, 0.0), 'se_r': (1e-12, 0.0),
                'mean_lw': (1e-12, 0.0), 'se_lw': (1e-12, 0.0),
                'c2': (1e-9, 0.0), 'c4': (1e-9, 0.0), 'c4_rows_clamp': (1e-9, 0.0),
                'cov': (1e-9, 1e-12), 'mean_w': (1e-10, 1e-12)}


def available():
    return mpmath is not None


def device_bound(quantity, ref, S):
    """|got - ref| allowed of a kernel: 8 x BOUNDS_ORACLE_ERR in units of 2^-53 S,
    capped by the tolerance of the existing tests for that quantity (relative to the
    larger of |ref| and S, the scale those tests' inputs had)."""
    rtol, atol = EXISTING_TOL[quantity]
    S = np.asarray(S, dtype=float)
    with np.errstate(invalid='ignore'):
        cap = atol + rtol * np.maximum(np.abs(np.where(np.isfinite(ref), ref, 0.0)), S)
    return np.minimum(MARGIN * BOUNDS_ORACLE_ERR[quantity][0] * UNIT * S, cap)


# ---- host restatements of the launch arithmetic --------------------------------
def red_grid(n):
    return int(max(1, min((n + RED_PER_BLOCK - 1) // RED_PER_BLOCK, RED_BLOCKS)))


def div2_grid(n):
    return int(max(1, min((n + DIV2_PER_BLOCK - 1) // DIV2_PER_BLOCK, RED_BLOCKS)))


def div_form(n):
    return 'welford' if n >= DIV_TWO_PASS_MIN_N else 'three_pass'


def div_stream_remainder(n):
    """How many log weights div_stream reads in its remainder loop (after the 4-way
    unrolled part) at the two-pass grid of n."""
    st = div2_grid(n) * 256
    tid = np.arange(st)
    count = np.maximum(0, (n - tid + st - 1) // st)
    return int(np.sum(count % 4))


def col_chunks(n):
    nc = int(max(1, min((n + COL_CHUNK_ROWS - 1) // COL_CHUNK_ROWS, COL_CHUNKS_MAX)))
    return nc, (n + nc - 1) // nc


def cov_path(d):
    return 'pairs' if d <= COV_D_MAX else 'gemm'


# ---- the references --------------------------------------------------------------
def _pair(v):
    if isinstance(v, float):
        return v, 0.0
    return _split(v)


def _div_ref(lw, alpha, elbo):
    mp.dps = DIGITS
    lw = np.asarray(lw, dtype=np.float64)
    n = lw.size
    nan = float('nan')
    with np.errstate(invalid='ignore'):
        top = float(np.max(lw))
    out = {'max': (top, 0.0, 0.0)}
    A = mpf(float(alpha))
    if np.any(np.isnan(lw)) or np.any(lw == np.inf):
        for q in ('d', 'lnb', 'mean_r', 'se_r', 'mean_lw', 'se_lw'):
            out[q] = (nan, 0.0, 1.0)
        if not np.any(np.isnan(lw)) and not np.any(lw == -np.inf):
            out['mean_lw'] = out['lnb'] = (np.inf, 0.0, 1.0)      # a sum that holds +inf alone
        if elbo is not None:
            out['lnb'] = (float(elbo), 0.0, 1.0)
        return out
    u, c = np.unique(lw, return_counts=True)
    fin = np.isfinite(u)
    any_ninf = bool(np.any(~fin))
    uf = [mpf(float(v)) for v in u[fin]]
    cf = [int(k) for k in c[fin]]
    absmax = float(np.max(np.abs(u[fin]))) if fin.any() else 0.0
    sqn = mp.sqrt(n)
    if any_ninf:
        mean_lw, se_lw = -mp.inf, mp.nan
    else:
        mean_lw = sum(k * v for k, v in zip(cf, uf)) / n
        se_lw = mp.sqrt(sum(k * (v - mean_lw) ** 2 for k, v in zip(cf, uf)) / n) / sqn
    lnb = mpf(float(elbo)) if elbo is not None else mean_lw
    if not fin.any():
        mean_r = se_r = d = logmr = mp.nan
    else:
        r = [mp.exp(A * (v - mpf(top))) for v in uf]
        mean_r = sum(k * v for k, v in zip(cf, r)) / n
        var = sum(k * (v - mean_r) ** 2 for k, v in zip(cf, r)) + (n - sum(cf)) * mean_r ** 2
        se_r = mp.sqrt(var / n) / sqn
        logmr = mp.log(mean_r)
        cubo = logmr / A + mpf(top)
        d = mp.inf if lnb == -mp.inf else A / (A - 1) * (cubo - lnb)
    f = lambda v: abs(float(v)) if mp.isfinite(v) else 0.0
    out['mean_lw'] = _pair(mean_lw) + (absmax,)
    out['se_lw'] = _pair(se_lw) + (max(f(se_lw), absmax / math.sqrt(n)),)
    out['lnb'] = _pair(lnb) + (max(absmax, f(lnb)),)
    out['mean_r'] = _pair(mean_r) + (f(mean_r),)
    out['se_r'] = _pair(se_r) + (max(f(se_r), f(mean_r) / math.sqrt(n)),)
    a = float(alpha)
    out['d'] = _pair(d) + (a / (a - 1) * max(1.0, abs(top) if math.isfinite(top) else 0.0,
                                              f(lnb), f(logmr) / a),)
    return out


def _col_stats(u, c, wts=None):
    """Per column of the distinct rows u (counts c, or mpf weights wts): mean (mpf),
    centred rows (mpf lists per column), total weight."""
    n_rows, d = u.shape
    wt = [mpf(int(k)) for k in c] if wts is None else wts
    tot = sum(wt)
    cols, means = [], []
    for j in range(d):
        col = [mpf(float(v)) for v in u[:, j]]
        m = mp.fdot(wt, col) / tot
        means.append(m)
        cols.append([v - m for v in col])
    return means, cols, wt, tot


def _kappa(x, sd):
    """max(1, max |x_d| / sd_d) per column; inf where sd_d = 0."""
    mx = np.max(np.abs(x), axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = np.where(sd > 0, mx / sd, np.inf)
    return np.maximum(1.0, k)


def _moments_ref(x):
    """centered_moments (bounds.py:133-135): mean over rows of sum_d (x - mean)^p,
    p = 2, 4 -> {'c2': (hi, lo, S), 'c4': ...}."""
    mp.dps = DIGITS
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    u, c = np.unique(x, axis=0, return_counts=True)
    means, cols, wt, tot = _col_stats(u, c)
    c2d = [mp.fdot(wt, [v * v for v in col]) / n for col in cols]
    c4d = [mp.fdot(wt, [v ** 4 for v in col]) / n for col in cols]
    sd = np.array([float(mp.sqrt(v)) for v in c2d])
    kap = _kappa(x, sd)
    S2 = sum(float(v) * k for v, k in zip(c2d, kap) if v != 0)
    S4 = sum(float(v) * k for v, k in zip(c4d, kap) if v != 0)
    return {'c2': _split(sum(c2d)) + (S2,), 'c4': _split(sum(c4d)) + (S4,)}


def _cov_ref(x, w, log_w, ddof):
    """np.average(x.T, axis=1, weights) and np.cov(x.T, aweights=weights, ddof) with
    weights w, or exp(log_w - max log_w), or none -> mean (hi, lo, S) [d] and cov
    (hi, lo, S) [d, d].  A zero normaliser gives numpy's pattern: nan everywhere
    (np.cov multiplies the zero products by 1 / 0)."""
    mp.dps = DIGITS
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    if log_w is not None:
        lw = np.asarray(log_w, dtype=np.float64)
        top = float(np.max(lw))
        wts = [mp.exp(mpf(float(v)) - mpf(top)) if np.isfinite(v) else mpf(0) for v in lw]
        with np.errstate(under='ignore'):
            wd = np.exp(lw - top)
    elif w is not None:
        wd = np.asarray(w, dtype=np.float64)
        wts = [mpf(float(v)) for v in wd]
    else:
        wd = np.ones(n)
        wts = [mpf(1)] * n
    means, cols, wt, sw = _col_stats(x, None, wts)
    if w is None and log_w is None:
        fact = mpf(n - ddof)
    else:
        fact = sw if ddof == 0 else sw - ddof * sum(v * v for v in wt) / sw
    live = wd > 0
    mean_S = np.full(d, float(np.max(np.abs(x[live]))))
    m_hi = np.array([float(v) for v in means])
    m_lo = np.array([float(v - mpf(h)) for v, h in zip(means, m_hi)])
    hi, lo = np.empty((d, d)), np.zeros((d, d))
    if fact == 0:
        hi[:] = np.nan
        return (m_hi, m_lo, mean_S), (hi, lo, np.ones((d, d)))
    wcols = [[a * b for a, b in zip(wt, col)] for col in cols]
    pop = np.empty(d)
    for i in range(d):
        for j in range(i, d):
            s = mp.fdot(wcols[i], cols[j])
            v = s / fact
            hi[i, j] = hi[j, i] = float(v)
            lo[i, j] = lo[j, i] = float(v - mpf(hi[i, j]))
            if i == j:
                pop[i] = float(mp.sqrt(s / sw))
    kap = _kappa(x[live], pop)
    dg = np.sqrt(np.abs(np.diagonal(hi)))
    with np.errstate(invalid='ignore'):
        S = np.outer(dg, dg) * np.maximum.outer(kap, kap)
    S[np.isnan(S)] = 0.0                  # 0 x inf: a column without spread
    return (m_hi, m_lo, mean_S), (hi, lo, S)


# ---- the divergence cases --------------------------------------------------------
def _multiset(values, n, seed):
    """n draws over the distinct `values` (each at least once), seeded counts, in a
    seeded permutation."""
    rs = np.random.RandomState(seed)
    values = np.asarray(values, dtype=np.float64)
    k = len(values)
    assert len(np.unique(values)) == k <= 32 <= n
    counts = 1 + rs.multinomial(n - k, rs.dirichlet(np.ones(k)))
    a = np.repeat(values, counts)
    rs.shuffle(a)
    return a


def _values(kind, n, rs):
    if kind == 'normal':
        return rs.randn(n)
    if kind == 't':
        return rs.standard_t(1.5, n) * 30.0
    if kind == 'const':
        return np.full(n, -3.75)
    if kind == 'const_inexact':
        return np.full(n, -3.7)
    if kind == 'dominant':               # every other weight underflows at alpha > 1
        a = -800.0 + rs.randn(n)
        a[n // 3] = 0.25
        return a
    if kind == 'subnormal':              # exp(lw - max) down to and past 2^-1074
        a = rs.uniform(-760.0, 0.0, n)
        a[n // 2] = 0.0
        a[1] = -720.0
        a[0] = -750.0
        return a
    if kind == 'off700':
        return -700.0 + rs.randn(n)
    if kind == 'off1e6':
        return -1.0e6 + rs.randn(n)
    if kind == 'off1e8':
        return 1.0e8 + 1.0e-3 * rs.randn(n)
    if kind == 'one_ninf':
        a = rs.randn(n)
        a[n // 3] = -np.inf
        return a
    if kind == 'all_but_one_ninf':
        a = np.full(n, -np.inf)
        a[n - 2 if n > 1 else 0] = 0.3
        return a
    if kind == 'all_ninf':
        return np.full(n, -np.inf)
    raise KeyError(kind)


SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
EDGE_SIZES = (65535, 65536, 65537)
REMAINDER_FIRST = 65537        # the first n >= 2^16 with a non-empty remainder loop
REMAINDER_EMPTY = 65536
CLAMP_RED = RED_BLOCKS * RED_PER_BLOCK + 257        # 2 097 409: past red_grid's clamp
CLAMP_DIV2 = RED_BLOCKS * DIV2_PER_BLOCK + 4097     # 8 392 705: past div2_grid's clamp
SMALL_SIDE, BIG_SIDE = 2049, 65537
VALUE_KINDS = ('t', 'const', 'const_inexact', 'dominant', 'subnormal', 'off700', 'off1e6',
               'off1e8', 'one_ninf', 'all_but_one_ninf', 'all_ninf')
_KIND_ALPHA = {'t': 2.0, 'const': 3.0, 'const_inexact': 2.0, 'dominant': 1.0001,
               'subnormal': 2.0, 'off700': 50.0, 'off1e6': 1.5, 'off1e8': 2.0, 'one_ninf': 2.0,
               'all_but_one_ninf': 1.5, 'all_ninf': 2.0}


def _div_specs():
    """name -> (kind, n, alpha, elbo, full): full = every draw its own value,
    otherwise a multiset of 32."""
    s = {}
    for n in SMALL_SIZES + EDGE_SIZES + (CLAMP_RED, CLAMP_DIV2):
        for alpha in (2.0, 1.5):
            s['normal_%d_a%g' % (n, alpha)] = ('normal', n, alpha, None,
                                               n <= SMALL_SIZES[-1] or (n in EDGE_SIZES and alpha == 2.0))
    for kind in VALUE_KINDS:
        for n in (SMALL_SIDE, BIG_SIDE):
            s['%s_%d' % (kind, n)] = (kind, n, _KIND_ALPHA[kind], None, n == SMALL_SIDE)
    for n in (SMALL_SIDE, BIG_SIDE):
        s['normal_%d_a3_elbo' % n] = ('normal', n, 3.0, -0.7, n == SMALL_SIDE)
        s['normal_%d_a1.0001_elbo' % n] = ('normal', n, 1.0001, 0.05, n == SMALL_SIDE)
        s['normal_%d_a50' % n] = ('normal', n, 50.0, None, n == SMALL_SIDE)
        s['subnormal_%d_a1.5' % n] = ('subnormal', n, 1.5, None, n == SMALL_SIDE)
        s['one_ninf_%d_elbo' % n] = ('one_ninf', n, 2.0, -1.25, n == SMALL_SIDE)
        s['off1e8_%d_a1.5_elbo' % n] = ('off1e8', n, 1.5, 1.0e8 - 2.0e-3, n == SMALL_SIDE)
    return s


_DIV_SPECS = _div_specs()
DIV_CASES = tuple(_DIV_SPECS)
# the cases the GPU test runs in both forms (a child with VIABEL_AMD_DIV_TWO_PASS=0)
BOTH_FORMS = tuple(k for k, v in _DIV_SPECS.items() if v[1] >= DIV_TWO_PASS_MIN_N)
# 2^16 - 1 draws: the default must be the three-pass form, bit for bit
FORM_EDGE = ('normal_65535_a2', 'normal_65535_a1.5')
NINF_KINDS = ('one_ninf', 'all_but_one_ninf', 'all_ninf')


# a nan beside a -inf, one size on each side of 2^16: numpy gives nan for every
# statistic (the device's log max skips nan, np.max does not: it is not compared)
NAN_CASES = ('nan_ninf_2049', 'nan_ninf_65537')


@functools.lru_cache(maxsize=None)
def nan_case(name):
    n = int(name.rsplit('_', 1)[1])
    a = np.random.RandomState(7900 + n % 1000).randn(n)
    a[n // 3] = -np.inf
    a[n // 3 + 1] = 0.5               # a finite draw right after the -inf
    a[(2 * n) // 3] = np.nan
    a[5] = -np.inf
    a.setflags(write=False)
    return a, 2.0, None


@functools.lru_cache(maxsize=None)
def _div_case(name):
    kind, n, alpha, elbo, full = _DIV_SPECS[name]
    seed = 7000 + sorted(_DIV_SPECS).index(name)
    rs = np.random.RandomState(seed)
    if full or kind in ('const', 'const_inexact', 'all_ninf', 'all_but_one_ninf'):
        a = _values(kind, n, rs)
    elif kind == 'dominant':             # the dominant draw exactly once
        a = np.insert(_multiset(-800.0 + rs.randn(31), n - 1, seed + 1), n // 3, 0.25)
    else:
        vals = np.unique(_values(kind, 32, rs))
        assert len(vals) == 32
        a = _multiset(vals, n, seed + 1)
    a = np.asarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a, alpha, elbo


def div_case(name):
    """(log weights (read-only), alpha, log_norm_bound or None) of a named case."""
    return _div_case(name)


@functools.lru_cache(maxsize=None)
def div_reference(name):
    """{quantity: (hi, lo, S)} of a case of DIV_CASES; computed once per process."""
    return _div_ref(*div_case(name))


def div_reference_of(lw, alpha, elbo=None):
    return _div_ref(lw, alpha, elbo)


def check_div_case(name):
    """Assert on the host every property the case is named for."""
    kind, n, alpha, elbo, full = _DIV_SPECS[name]
    lw, a, e = div_case(name)
    assert lw.shape == (n,) and a == alpha > 1 and e == elbo
    assert div_form(n) == ('three_pass' if n < DIV_TWO_PASS_MIN_N else 'welford')
    assert (name in BOTH_FORMS) == (n >= 65536)
    if n > BIG_SIDE:
        assert len(np.unique(lw)) <= 32
    if n == REMAINDER_FIRST:
        assert div_stream_remainder(n) > 0
        assert all(div_stream_remainder(m) == 0 for m in range(DIV_TWO_PASS_MIN_N, n))
    if n == REMAINDER_EMPTY:
        assert div_stream_remainder(n) == 0
    if n == CLAMP_RED:
        assert (n + RED_PER_BLOCK - 1) // RED_PER_BLOCK > RED_BLOCKS == red_grid(n)
        assert div2_grid(n) < RED_BLOCKS
    if n == CLAMP_DIV2:
        assert (n + DIV2_PER_BLOCK - 1) // DIV2_PER_BLOCK > RED_BLOCKS == div2_grid(n)
        assert div_stream_remainder(n) > 0
    if kind in ('const', 'const_inexact'):
        assert np.all(lw == lw[0])
    if kind == 'const':
        assert float(lw[0]) * 2 ** 2 == int(float(lw[0]) * 2 ** 2)      # dyadic: sums exact
    if kind == 'dominant':
        top = np.max(lw)
        with np.errstate(under='ignore'):
            assert np.sum(np.exp(alpha * (lw - top)) > 0) == 1 and np.sum(lw == top) == 1
            assert np.sum(np.exp(lw - top) > 0) == 1
    if kind == 'subnormal':
        with np.errstate(under='ignore'):
            e1 = np.exp(lw - np.max(lw))
        tiny = np.finfo(float).tiny
        assert np.any((e1 > 0) & (e1 < tiny)) and np.any(e1 == 0) and np.any(e1 == 1)
    if kind.startswith('off'):
        off = {'off700': -700.0, 'off1e6': -1.0e6, 'off1e8': 1.0e8}[kind]
        assert np.all(np.abs(lw - off) < (1.0 if kind == 'off1e8' else 8.0))
        assert np.std(lw) > (1e-4 if kind == 'off1e8' else 0.3)
    if kind == 'one_ninf':
        assert np.sum(np.isneginf(lw)) >= 1 and np.sum(np.isfinite(lw)) >= n // 2
        assert full is False or np.sum(np.isneginf(lw)) == 1
    if kind == 'all_but_one_ninf':
        assert np.sum(np.isfinite(lw)) == 1 and np.sum(np.isneginf(lw)) == n - 1
    if kind == 'all_ninf':
        assert np.all(np.isneginf(lw))
    if kind not in NINF_KINDS:
        assert np.all(np.isfinite(lw))
    if available():
        ref = div_reference(name)
        if kind == 'dominant':
            assert abs(ref['mean_r'][0] * n - 1.0) < 1e-15
        if kind in ('const', 'const_inexact'):
            assert ref['se_r'][0] == 0.0 and ref['se_lw'][0] == 0.0 and ref['mean_r'][0] == 1.0
        if kind in ('one_ninf', 'all_but_one_ninf'):
            assert ref['mean_lw'][0] == -np.inf and np.isnan(ref['se_lw'][0])
            assert np.isfinite(ref['mean_r'][0]) and np.isfinite(ref['se_r'][0])
            assert ref['d'][0] == np.inf if elbo is None else np.isfinite(ref['d'][0])
        if kind == 'all_ninf':
            assert ref['max'][0] == -np.inf and ref['mean_lw'][0] == -np.inf
            assert all(np.isnan(ref[q][0]) for q in ('d', 'mean_r', 'se_r', 'se_lw'))


# ---- the moment cases ------------------------------------------------------------
CLAMP_ROWS = COL_CHUNKS_MAX * COL_CHUNK_ROWS + 1      # 2 097 153 rows: past col_chunks' clamp


def _moment_builders():
    def rn(seed, n, d):
        return np.random.RandomState(seed).randn(n, d)

    def clamp_rows():
        rs = np.random.RandomState(8101)
        rows = rs.randn(32, 2) * [1.0, 3.0] + [0.5, -2.0]
        idx = _multiset(np.arange(32.0), CLAMP_ROWS, 8102).astype(np.int64)
        return rows[idx]

    def const_col():
        x = rn(8105, 257, 3)
        x[:, 1] = 2.5
        return x

    return {
        'n1_d1': lambda: rn(8001, 1, 1) + 0.3,
        'n2_d1': lambda: rn(8002, 2, 1),
        'n257_d1': lambda: rn(8003, 257, 1) * 2.0 + 1.0,
        'n5_d3': lambda: rn(8004, 5, 3),
        'n4096_d2': lambda: rn(8005, 4096, 2),
        'n4097_d2': lambda: rn(8006, 4097, 2),
        'n300_d65': lambda: rn(8007, 300, 65) * np.linspace(0.5, 2.0, 65),
        'rows_clamp_d2': clamp_rows,
        'offset_1e8': lambda: 1.0e8 + 1.0e-3 * rn(8103, 257, 3),
        'scales_1e70': lambda: rn(8104, 300, 2) * [1.0e-70, 1.0e70],
        'const_column': const_col,
    }


_MOMENT_BUILDERS = _moment_builders()
MOMENT_CASES = tuple(_MOMENT_BUILDERS)
MOMENT_SHAPES = {'n1_d1': (1, 1), 'n2_d1': (2, 1), 'n257_d1': (257, 1), 'n5_d3': (5, 3),
                 'n4096_d2': (4096, 2), 'n4097_d2': (4097, 2), 'n300_d65': (300, 65),
                 'rows_clamp_d2': (CLAMP_ROWS, 2), 'offset_1e8': (257, 3),
                 'scales_1e70': (300, 2), 'const_column': (257, 3)}


@functools.lru_cache(maxsize=None)
def moment_case(name):
    a = np.ascontiguousarray(_MOMENT_BUILDERS[name](), dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def moment_reference(name):
    return _moments_ref(moment_case(name))


def moment_quantity(name, p):
    """The BOUNDS_ORACLE_ERR entry the p-th moment of a case is held to."""
    return 'c4_rows_clamp' if (name, p) == ('rows_clamp_d2', 4) else 'c%d' % p


def check_moment_case(name):
    x = moment_case(name)
    n, d = MOMENT_SHAPES[name]
    assert x.shape == (n, d) and np.all(np.isfinite(x))
    nc, rpc = col_chunks(n)
    if name == 'n4096_d2':
        assert (nc, rpc) == (1, 4096)
    if name == 'n4097_d2':
        assert (nc, rpc) == (2, 2049)
    if name == 'rows_clamp_d2':
        assert (n + COL_CHUNK_ROWS - 1) // COL_CHUNK_ROWS > COL_CHUNKS_MAX == nc and rpc == 4097
        assert len(np.unique(x, axis=0)) == 32
        assert red_grid(n * d) == RED_BLOCKS < (n * d) // RED_PER_BLOCK
    if name == 'n300_d65':
        assert d > 64                       # two column tiles of col_sum_kernel
    if name == 'offset_1e8':
        assert np.all(np.abs(x - 1.0e8) < 1.0)
    if name == 'scales_1e70':
        assert 1e-71 < np.std(x[:, 0]) < 1e-69 and 1e69 < np.std(x[:, 1]) < 1e71
    if name == 'const_column':
        assert np.all(x[:, 1] == 2.5) and np.std(x[:, 0]) > 0.5 < np.std(x[:, 2])


# ---- the covariance cases --------------------------------------------------------
# name -> (n, d, weights kind, ddof): weights None, 'uniform', 'one_hot', 'random',
# 'logw_1400' (log weights with spread 1400), 'logw_ninf' (log weights, -inf entries);
# 'offset' in the name: columns offset by 1e8 with spread 1e-3
COV_SPECS = {
    'n2_d1': (2, 1, None, 1), 'n3_d2': (3, 2, None, 1), 'n255_d2_ddof0': (255, 2, None, 0),
    'n4097_d2': (4097, 2, None, 1), 'n3_d63': (3, 63, None, 1), 'n257_d64': (257, 64, None, 1),
    'n257_d65': (257, 65, None, 1), 'n2_d65': (2, 65, None, 1), 'n3_d66': (3, 66, None, 1),
    'n3_d66_ddof0': (3, 66, None, 0),
    'uniform_n255_d2': (255, 2, 'uniform', 1), 'uniform_n3_d65_ddof0': (3, 65, 'uniform', 0),
    'one_hot_n255_d2_ddof0': (255, 2, 'one_hot', 0), 'one_hot_n255_d2_ddof1': (255, 2, 'one_hot', 1),
    'one_hot_n3_d65_ddof0': (3, 65, 'one_hot', 0), 'one_hot_n3_d65_ddof1': (3, 65, 'one_hot', 1),
    'random_n4097_d2': (4097, 2, 'random', 1), 'random_n257_d64': (257, 64, 'random', 1),
    'random_n257_d65_ddof0': (257, 65, 'random', 0),
    'logw_1400_n257_d2': (257, 2, 'logw_1400', 0), 'logw_1400_n255_d65': (255, 65, 'logw_1400', 1),
    'logw_ninf_n4097_d2': (4097, 2, 'logw_ninf', 1), 'logw_ninf_n3_d66': (3, 66, 'logw_ninf', 0),
    'offset_n257_d2': (257, 2, None, 1), 'offset_n255_d65': (255, 65, None, 1),
    'offset_random_n257_d3': (257, 3, 'random', 0),
}
COV_CASES = tuple(COV_SPECS)
# n257_d64 is the 64-column prefix of n257_d65 (pair path against GEMM path)
PREFIX_PAIR = ('n257_d64', 'n257_d65')


@functools.lru_cache(maxsize=None)
def cov_case(name):
    """(x [n, d], weights or None, log weights or None, ddof), read-only."""
    n, d, kind, ddof = COV_SPECS[name]
    if name in PREFIX_PAIR:
        x = np.random.RandomState(9000).randn(257, 65) * np.linspace(0.3, 3.0, 65) + 1.0
        x = np.ascontiguousarray(x[:, :d])
    else:
        rs = np.random.RandomState(9001 + COV_CASES.index(name))
        x = rs.randn(n, d) * (0.5 + rs.uniform(size=d))
        if name.startswith('offset'):
            x = 1.0e8 + 1.0e-3 * x
    rs = np.random.RandomState(9500 + COV_CASES.index(name))
    w = lw = None
    if kind == 'uniform':
        w = np.full(n, 0.25)
    elif kind == 'one_hot':
        w = np.zeros(n)
        w[n // 2] = 1.0
    elif kind == 'random':
        w = rs.gamma(0.7, 2.0, n)
    elif kind == 'logw_1400':
        lw = rs.uniform(-1400.0, 0.0, n) + 37.0
    elif kind == 'logw_ninf':
        lw = rs.randn(n) * 2.0
        lw[::2] = -np.inf
    for a in (x, w, lw):
        if a is not None:
            a.setflags(write=False)
    return x, w, lw, ddof


@functools.lru_cache(maxsize=None)
def cov_reference(name):
    """((mean hi, lo, S), (cov hi, lo, S)) of a case of COV_CASES."""
    x, w, lw, ddof = cov_case(name)
    return _cov_ref(x, w, lw, ddof)


def check_cov_case(name):
    n, d, kind, ddof = COV_SPECS[name]
    x, w, lw, dd = cov_case(name)
    assert x.shape == (n, d) and dd == ddof and x.flags.c_contiguous
    assert cov_path(d) == ('pairs' if d <= 64 else 'gemm')
    if d == 64:
        assert d * (d + 1) // 2 == 2080
    if name == PREFIX_PAIR[1]:
        assert np.array_equal(x[:, :64], cov_case(PREFIX_PAIR[0])[0])
    if n == 4097:
        assert col_chunks(n) == (2, 2049)
    if kind == 'logw_1400':
        with np.errstate(under='ignore'):
            wd = np.exp(lw - lw.max())
        assert np.ptp(lw) > 1300 and np.any(wd == 0) and np.sum(wd > 0) > d // 8
    if kind == 'logw_ninf':
        assert np.sum(np.isneginf(lw)) == (n + 1) // 2 and np.sum(np.isfinite(lw)) >= 1
    if kind == 'one_hot':
        assert np.sum(w) == 1.0 and np.count_nonzero(w) == 1
    if name.startswith('offset'):
        assert np.all(np.abs(x - 1.0e8) < 1.0)
    if available() and kind == 'one_hot':
        (_, _, _), (hi, lo, S) = cov_reference(name)
        assert np.all(hi == 0) if ddof == 0 else np.all(np.isnan(hi))
