"""Multiprecision restatement (mpmath, 50 digits) of compute_R_hat
(viabel/functions.py:8-31) and the seeded edge-case set of vb_rhat.hip; shared by
the CPU test that pins the numpy oracle (tests/test_oracle_rhat_mp.py) and the GPU
tests (tests/test_gpu_rhat_edges.py).

What counts as exact input.  The float64 chains [n_chains, n_iters, K], the segment
(start, len) and the jitter 1e-8 taken as that double.  From there on mpmath: the
half-chain means m_j (h = len / 2 draws each, half-chain j = 2 c + half), the
variances s_j^2 = sum (x - m_j)^2 / (h - 1), B = h sum (m_j - grand)^2 / (2 nc - 1),
W = nanmean_j s_j^2 + 1e-8, var_hat = (h - 1) / h + B / (h W), R-hat = sqrt(var_hat).
h = 1 follows numpy: every s_j^2 is 0 / 0 = nan, the nanmean of no value is nan,
so var_hat and R-hat are nan for every parameter.

Error metric, as tests/psis_mp.py: err = |got - ref| / (2^-53 S), references as
double pairs (hi, lo).  With T = B / (h W) the part of var_hat that holds rounding
error (the other, (h - 1) / h, is one division),
  var_hat   S = (h - 1) / h + T (kappa_W + kappa_B)
  R-hat     S = R + S_var / (2 R)
kappa_W = max(1, max |x| / sqrt(nanmean s_j^2)) is the cancellation in x - m_j and
kappa_B = max(1, max |m_j| sqrt(h) / sd(m_j)) that in m_j - grand (each m_j carries
the rounding of a sum of h draws); a term whose T is 0 (constant chains) adds 0.
"""
import functools
import math

import numpy as np

from tests.psis_mp import DIGITS, UNIT, err      # noqa: F401  (err: shared metric)

try:
    import mpmath
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mpmath = None

JITTER = 1e-8
BLOCK = 256                    # vb_rhat.hip: one thread per parameter, 256 a block
MARGIN = 8.0

# The largest error of oracle/functions_oracle.py compute_R_hat against this
# reference over CASES, in units of 2^-53 S, with the case that produced it;
# measured by tests/test_oracle_rhat_mp.py, which asserts each at 2x.
RHAT_ORACLE_ERR = {
    'var_hat': (1.277, 'nc2_len6_K256'),
    'rhat': (0.9359, 'nc2_len6_K257'),
}
# tests/test_gpu_ia.py already holds both to rtol 1e-12; no bound here is looser
EXISTING_RTOL = 1e-12


def available():
    return mpmath is not None


def device_bound(quantity, ref, S):
    return np.minimum(MARGIN * RHAT_ORACLE_ERR[quantity][0] * UNIT * S,
                      EXISTING_RTOL * np.maximum(np.abs(np.where(np.isfinite(ref), ref, 0.0)), S))


def _rhat_ref(chains, start, length):
    """(var_hat (hi, lo, S), rhat (hi, lo, S)), each [K]."""
    mp.dps = DIGITS
    nc, _, K = chains.shape
    h = length // 2
    out = np.full((6, K), np.nan)
    out[1] = out[4] = 0.0
    out[2] = out[5] = 1.0
    if h < 2:
        return tuple(out[:3]), tuple(out[3:])
    for p in range(K):
        halves = [[mpf(float(v)) for v in chains[c, start + k * h:start + (k + 1) * h, p]]
                  for c in range(nc) for k in range(2)]
        m = [sum(x) / h for x in halves]
        s2 = [sum((v - mj) ** 2 for v in x) / (h - 1) for x, mj in zip(halves, m)]
        grand = sum(m) / (2 * nc)
        sb = sum((mj - grand) ** 2 for mj in m)
        B = h * sb / (2 * nc - 1)
        W0 = sum(s2) / (2 * nc)
        T = B / (h * (W0 + mpf(JITTER)))
        var = mpf(h - 1) / h + T
        R = mp.sqrt(var)
        seg = chains[:, start:start + 2 * h, p]
        amax = float(np.max(np.abs(seg)))
        S = (h - 1) / h
        if T != 0:
            kw = max(1.0, amax / float(mp.sqrt(W0))) if W0 != 0 else 1.0
            kb = max(1.0, max(abs(float(v)) for v in m) * math.sqrt(h)
                     / float(mp.sqrt(sb / (2 * nc))))
            S += float(T) * (kw + kb)
        out[0, p] = float(var)
        out[1, p] = float(var - mpf(out[0, p]))
        out[2, p] = S
        out[3, p] = float(R)
        out[4, p] = float(R - mpf(out[3, p]))
        out[5, p] = out[3, p] + S / (2 * out[3, p])
    return tuple(out[:3]), tuple(out[3:])


# ---- the case set ------------------------------------------------------------
def _randn(seed, nc, n, K):
    rs = np.random.RandomState(seed)
    return rs.randn(nc, n, K) * (0.5 + rs.uniform(size=K)) + rs.randn(nc, 1, K) * 0.3


def _builders():
    b = {}
    for nc in (1, 2, 3):
        for ln in (2, 4, 6, 64):
            b['nc%d_len%d_K1' % (nc, ln)] = (
                lambda nc=nc, ln=ln: _randn(100 * nc + ln, nc, ln, 1), None)
    for K in (255, 256, 257):
        b['nc2_len6_K%d' % K] = (lambda K=K: _randn(500 + K, 2, 6, K), None)
    b['nc3_len2_K257'] = (lambda: _randn(601, 3, 2, 257), None)
    b['four_segments'] = (lambda: _randn(602, 2, 80, 5), ((0, 64), (3, 6), (11, 4), (16, 64)))
    b['with_len2_segment'] = (lambda: _randn(603, 2, 12, 3), ((0, 12), (5, 2), (2, 4)))
    b['constant'] = (lambda: np.full((2, 6, 3), 2.5), None)
    b['constant_inexact'] = (lambda: np.full((3, 64, 2), -3.7), None)
    b['constant_per_chain'] = (
        lambda: np.broadcast_to(np.array([1.5, -0.25])[:, None, None], (2, 6, 3)).copy(), None)
    b['offset_1e8'] = (lambda: 1.0e8 + 1.0e-3 * _randn(604, 3, 64, 4), None)

    def one_const():
        x = _randn(605, 2, 64, 257)
        x[:, :, 128] = 1.5
        return x
    b['one_constant_param'] = (one_const, None)
    return b


_BUILDERS = _builders()
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(chains [nc, n, K] read-only, segments ((start, len), ...))."""
    build, segs = _BUILDERS[name]
    x = np.ascontiguousarray(build(), dtype=np.float64)
    x.setflags(write=False)
    return x, (segs if segs is not None else ((0, x.shape[1]),))


@functools.lru_cache(maxsize=None)
def reference(name):
    """One (var_hat, rhat) reference per segment of the case."""
    x, segs = case(name)
    return tuple(_rhat_ref(x, s, ln) for s, ln in segs)


def check_case(name):
    x, segs = case(name)
    nc, n, K = x.shape
    assert nc in (1, 2, 3) and all(ln % 2 == 0 and 0 <= s and s + ln <= n for s, ln in segs)
    if name.startswith('nc') and name != 'nc3_len2_K257':
        assert (nc, n, K) == tuple(int(v) for v in name.replace('nc', '').replace('len', '')
                                   .replace('K', '').split('_'))
    if K in (255, 256, 257):
        assert ((K + BLOCK - 1) // BLOCK > 1) == (K == 257)
    if name == 'four_segments':
        assert len(segs) == 4 and len({s for s, _ in segs}) == 4 and len({l for _, l in segs}) == 3
    if name == 'with_len2_segment':
        assert segs[1][1] == 2
    if name.startswith('constant'):
        assert np.all(x == x[:, :1, :])
    if name == 'offset_1e8':
        assert np.all(np.abs(x - 1.0e8) < 1.0) and np.std(x) > 1e-4
    if name == 'one_constant_param':
        assert np.all(x[:, :, 128] == 1.5) and np.std(x[:, :, 127]) > 0.3 < np.std(x[:, :, 129])
    if available():
        for (s, ln), ((v_hi, _, v_S), _) in zip(segs, reference(name)):
            h = ln // 2
            assert np.all(np.isnan(v_hi)) if h == 1 else np.all(np.isfinite(v_hi))
            if name in ('constant', 'constant_inexact'):
                assert np.all(v_hi == (h - 1) / h) and np.all(v_S == (h - 1) / h)
            if name == 'one_constant_param':
                assert v_hi[128] == (h - 1) / h and np.all(np.delete(v_hi, 128) > (h - 1) / h)
