"""Cases of the Philox log-weight kernels for tests/test_oracle_logw_mp.py (CPU: the
oracle against the 50-digit reference of tests/logw_mp.py) and
tests/test_gpu_logw_edges.py (the device).  A case is one Philox stream of seed 0, a
family, a target and lam; for every (m, n) of c['calls'] the test takes a fresh family
and calls experiments.log_weights n times with m rows (steps step0, step0 + 1: the
second call must use the next step's draws).  Row r's draws do not depend on m, so
the reference of a step is built once for the most rows any call needs and shared.

Kernels ('kernel'): 'row' logw_row_kernel (D <= 16, instances DMAX 2 / 4 / 10 / 16),
'sep' logw_sep_kernel (separable targets, D > 16: 4 rows per block, 64 pairs per pass),
'mat' sample_bailey_kernel + target + launch_family_logdensity (the funnel at D > 16;
256 (row, pair) threads per block; D >= 512 switches the row kernels).

What is here, and what was thinned from the full product:
  grid    every D x m of each kernel at t(40) and central lam (0.3 randn), two steps
          (the row kernel's second step at m = 1 only: its 257-row references are the
          bulk of the reference's time);
          the target rotates over D instead of every target at every D (eight schools
          at D = 10, each other target at odd and even D of some instance)
  edges   one D per kernel instance (row 2, 3, 10, 15; sep 17; mat 17), every family (t
          at df 2.000001, 2.5, 40, 1e3, 1e6; Gaussian, not on 'mat': its Bailey
          sampler is the t family's) x every log sigma (-30, -3, 0, 5, 30, mixed), one
          step, a few rows; mu rotates through (0, +30, -30) with log sigma and the
          instance rather than being crossed with it, and is clipped to the target's
          edge domain of tests/targets_mp.py (funnel x_1 in [-12, 9], eight schools
          log tau in [-40, 20]).  The log scale coordinate of the funnel and of eight
          schools keeps log sigma = -3 throughout: at df -> 2 a draw of 1e3 sigma there
          sends exp(-2 x_1) past the double range.
  tails   the planted (stream, step) pairs of TAILS at df 2.000001, 40, 1e6 on all
          three kernels, 5 rows
  wide    one D = 512 funnel case at m = 5
"""
import numpy as np

SEED = 0
T_DFS = (2.000001, 2.5, 40.0, 1e3, 1e6)
FAMILIES = tuple(('t', df) for df in T_DFS) + (('gauss', None),)
LOG_SIGMAS = (-30.0, -3.0, 0.0, 5.0, 30.0, 'mixed')
MUS = (0.0, 30.0, -30.0)

# (class, stream, step, row, pair, c, a, b): Bailey variate 2 pair + c of `row` has the
# 40-bit a (U1 = (a + 1/2) 2^-40) and 24-bit b (U2 = b 2^-24) shown; found by
# scripts/find_logw_tail_streams.py (seed 0, rows < 5, pairs < 8, never column 1).
# a_lo: U1 < 2^-28; a_hi: U1 > 1 - 2^-28; b0 / bq1 / bh / bq3: cos(2 pi U2) at 1, 0, -1, 0
# and (+, -) one step of 2^-24 beside them.  c = 0 hits run the row kernel at D = 2 pair
# + 1, where the hit is the last pair's only column (14 of the 16).
TAILS = (
    ('a_hi', 3073648, 1, 3, 7, 0, 1099511627319, 6360676),
    ('a_hi', 126802, 1, 1, 2, 1, 1099511624104, 9552556),
    ('a_lo', 422259, 0, 1, 1, 1, 1232, 14184611),
    ('a_lo', 546450, 1, 2, 0, 0, 1354, 10977356),
    ('b0', 203468, 0, 0, 4, 0, 421111360782, 0),
    ('b0+', 83296, 1, 3, 2, 0, 251675748812, 1),
    ('b0-', 63074, 0, 3, 6, 0, 994007358017, 16777215),
    ('bh', 49447, 0, 1, 5, 0, 667348230624, 8388608),
    ('bh+', 340404, 0, 2, 1, 0, 806811825294, 8388609),
    ('bh-', 406472, 0, 1, 4, 0, 441842874855, 8388607),
    ('bq1', 115002, 1, 3, 3, 0, 436517106913, 4194304),
    ('bq1+', 225011, 0, 1, 5, 0, 755125282434, 4194305),
    ('bq1-', 95141, 0, 0, 4, 0, 206080979659, 4194303),
    ('bq3', 103461, 1, 4, 6, 0, 664496448235, 12582912),
    ('bq3+', 209175, 1, 2, 5, 0, 777328484191, 12582913),
    ('bq3-', 404654, 0, 0, 5, 0, 862306467260, 12582911),
)
TAIL_DFS = (2.000001, 40.0, 1e6)

ROW_DS = (1, 2, 3, 4, 5, 9, 10, 11, 15, 16)
ROW_MS = (1, 255, 256, 257)
SEP_DS = (17, 18, 127, 128, 129, 130)
SEP_MS = (1, 3, 4, 5)
# m on both sides of ceil(D / 2) m = 256, the sampler's 256-thread block
MAT_GRID = ((17, (28, 29)), (18, (28, 29)), (40, (12, 13)))
WIDE_D = 512                                     # kWideRowD
# the instance of the row kernel a D runs on
ROW_DMAX = {D: next(k for k in (2, 4, 10, 16) if D <= k) for D in range(1, 17)}

_LOG_SCALE = {'funnel': 1, 'eight_schools_ncp': 1}
_MU_CLIP = {'funnel': {1: (-12.0, 9.0)}, 'eight_schools_ncp': {1: (-40.0, 20.0)}}


def central_lam(D):
    return np.random.RandomState(D).randn(2 * D) * 0.3


def edge_lam(target, D, log_sigma, mu, salt):
    """lam at a log sigma of LOG_SIGMAS and a mu of MUS (each entry moved by 1e-2 randn
    so that none is a round number), within the target's domain (the header)."""
    rs = np.random.RandomState(1000 * salt + D)
    if log_sigma == 'mixed':
        ls = np.array([LOG_SIGMAS[(d + salt) % 5] for d in range(D)])
        m = np.array([MUS[(d + salt) % 3] for d in range(D)])
    else:
        ls, m = np.full(D, log_sigma), np.full(D, mu)
    ls = ls + 1e-2 * rs.randn(D)
    m = m + 1e-2 * rs.randn(D)
    if target in _LOG_SCALE and D > 1:
        ls[_LOG_SCALE[target]] = -3.0 + 1e-2 * rs.randn()
    for d, (lo, hi) in _MU_CLIP.get(target, {}).items():
        m[d] = min(max(m[d], lo), hi)
    return np.concatenate([m, ls])


def _case(cid, kernel, target, D, fam, lam, stream, calls, step0=0):
    """calls: (m, n) pairs -- a fresh family at step0, then n log_weights calls of m rows
    (steps step0 .. step0 + n - 1).  rows: per step, the rows its reference needs."""
    rows = {}
    for m, n in calls:
        for s in range(step0, step0 + n):
            rows[s] = max(rows.get(s, 0), m)
    return {'id': cid, 'kernel': kernel, 'target': target, 'D': D, 'kind': fam[0], 'df': fam[1],
            'lam': lam, 'stream': stream, 'calls': tuple(calls), 'step0': step0, 'rows': rows}


def _fam_id(fam):
    return 'gauss' if fam[0] == 'gauss' else 't%.7g' % fam[1]


def grid_cases():
    out = []
    rot = ('isogauss', 'mixture', 'funnel')
    for k, D in enumerate(ROW_DS):
        target = 'eight_schools_ncp' if D == 10 else rot[k % 3] if D > 1 else 'mixture'
        out.append(_case('grid/row/%s/D%d' % (target, D), 'row', target, D, ('t', 40.0),
                         central_lam(D), 500 + D, [(m, 2 if m == 1 else 1) for m in ROW_MS]))
    for k, D in enumerate(SEP_DS):
        target = rot[k % 2]
        out.append(_case('grid/sep/%s/D%d' % (target, D), 'sep', target, D, ('t', 40.0),
                         central_lam(D), 500 + D, [(m, 2) for m in SEP_MS]))
    for D, ms in MAT_GRID:
        out.append(_case('grid/mat/funnel/D%d' % D, 'mat', 'funnel', D, ('t', 40.0),
                         central_lam(D), 500 + D, [(m, 2) for m in ms]))
    out.append(_case('wide/mat/funnel/D%d' % WIDE_D, 'mat', 'funnel', WIDE_D, ('t', 40.0),
                     central_lam(WIDE_D), 500 + WIDE_D, [(5, 1)]))
    return out


EDGE_INSTANCES = (('row', 'mixture', 2, 7), ('row', 'funnel', 3, 7),
                  ('row', 'eight_schools_ncp', 10, 7), ('row', 'isogauss', 15, 7),
                  ('sep', 'mixture', 17, 5), ('mat', 'funnel', 17, 5))


def edge_cases():
    out = []
    for i, (kernel, target, D, m) in enumerate(EDGE_INSTANCES):
        for f, fam in enumerate(FAMILIES):
            if kernel == 'mat' and fam[0] == 'gauss':
                continue
            for k, ls in enumerate(LOG_SIGMAS):
                mu = MUS[(k + i + f) % 3]
                cid = 'edge/%s/%s/D%d/%s/ls%s/mu%g' % (kernel, target, D, _fam_id(fam), ls, mu)
                out.append(_case(cid, kernel, target, D, fam, edge_lam(target, D, ls, mu, i + 7 * k),
                                 2000 + 100 * i + 10 * f + k, [(m, 1)]))
    return out


def tail_cases():
    out = []
    rot = ('isogauss', 'mixture', 'funnel')
    for k, (cls, stream, step, row, pair, c, a, b) in enumerate(TAILS):
        col = 2 * pair + c
        Drow = col + 1
        trow = rot[k % 3] if Drow >= 2 else rot[k % 2]
        for kernel, target, D in (('row', trow, Drow), ('sep', rot[k % 2], 17),
                                  ('mat', 'funnel', 17)):
            for df in TAIL_DFS:
                cid = 'tail/%s/s%d/%s/%s/D%d/t%.7g' % (cls, stream, kernel, target, D, df)
                t = _case(cid, kernel, target, D, ('t', df), central_lam(D), stream, [(5, 1)], step)
                t['tail'] = (row, col, a, b)
                out.append(t)
    return out


def all_cases():
    return grid_cases() + edge_cases() + tail_cases()


CASES = all_cases()
BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)
