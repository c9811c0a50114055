"""Multiprecision restatement (mpmath, 50 digits) of the Philox log-weight draws and of
the log weights on them, from the draws' integers (oracle/rng_oracle.draw_ints), not
from libm doubles; shared by tests/test_oracle_logw_mp.py (which pins the C oracle's
draws and the numpy oracle's log weights) and tests/test_gpu_logw_edges.py (the device
kernels).  The family's log q, the targets and the condition sums are those of
tests/mf_mp.py and tests/targets_mp.py.

  t family (Bailey)   U1 = (a + 1/2) 2^-40, th = 2 pi b 2^-24, R = sqrt(df (U1^(-2/df) - 1)),
                      T = cos(th) R
  Gaussian family     u1 = (2 m1 + 1) 2^-53, th = 2 pi m2 2^-52, r = sqrt(-2 log u1),
                      (z0, z1) = r (cos th, sin th)
  x = mu + sigma T,  log q at the draw T (mf_mp._logq1),  log p at x (targets_mp.ROW),
  lw = log p - log q

Condition sums (errors are reported in units of 2^-53 S, mf_mp.units).

  draw     S_T = R (|cos th| (1 + kappa) + th |sin th|),  kappa = a e^a / (2 (e^a - 1)) at
           a = -(2 / df) log U1: the conditioning of expm1 under a relative error of the
           log, halved by the square root (1/2 at U1 -> 1, ~14 at df -> 2 and U1 = 2^-41).
           th |sin th| is the conditioning of the cosine under a relative error of its
           argument: a restatement that forms 2 pi U2 in doubles (the C oracle) rounds the
           argument, and beside the cosine's zeros that moves T by far more than |T|
           ulps (at b = 2^22 exactly the oracle's T is 6e-17 R where the true T is 0); the
           issue's |T| (1 + kappa) alone would measure the oracle at infinity there.  The
           Gaussian pair: S = r (|cos| + th |sin|) and r (|sin| + th |cos|).
  sample   |mu| + sigma S_T
  log_w    S of mean-field log weights (S_lp + sum_d |g_d| dx_d + S_lq, mf_mp), plus the
           draw's allowance through the derivative, sum_d |sigma_d g_d - d log q / d T_d|
           S_T,d ('direct': log q taken at the draw itself, the row kernel's t branch);
           'back' adds, for the paths that read log q back from the rounded x through
           z = (x - mu) / sigma, mf_mp's first-order term |d log q / d z| dx / sigma and
           the Lagrange remainder sup|d2 log q / d z2| / 2 (2^-53 dx / sigma)^2 in the
           same units (sup = 1, or (df + 1) / df for t): at log sigma = -30, |mu| = 30 the
           rounding of x moves z by 0.035, where a first-order term is no bound (it
           vanishes at z = 0, the error does not).  One unit of dx is what the rounding
           of x = mu + sigma T costs the oracle (two roundings) and the device (one fma);
           exp(log sigma) enters x and z alike and cancels.
"""
import functools
from collections import namedtuple

import numpy as np

from tests import mf_mp as mm
from tests import targets_mp as tm
from tests.targets_mp import DIGITS, UNIT, mpmath

if mpmath is not None:
    from mpmath import mp, mpf

# eps, x: Val (rows, D) in the draw / sample classes; lw_direct, lw_back: Val (rows,)
Ref = namedtuple('Ref', 'eps x lw_direct lw_back')


def available():
    return mpmath is not None


def _bailey(df, a, b):
    """(T, S_T) of one Bailey variate from its integers."""
    u1 = (mpf(int(a)) + mpf(1) / 2) / 2 ** 40
    th = 2 * mp.pi * mpf(int(b)) / 2 ** 24
    arg = -(2 / df) * mp.log(u1)
    em1 = mp.expm1(arg)
    kappa = arg * (em1 + 1) / (2 * em1)
    R = mp.sqrt(df * em1)
    cs = mp.cos(th)
    return cs * R, R * (abs(cs) * (1 + kappa) + th * abs(mp.sin(th)))


def _gauss_pair(m1, m2):
    """((z0, S0), (z1, S1)) of one Box-Muller pair from its mantissa integers."""
    u1 = (2 * mpf(int(m1)) + 1) / 2 ** 53
    th = 2 * mp.pi * mpf(int(m2)) / 2 ** 52
    r = mp.sqrt(-2 * mp.log(u1))
    cs, sn = mp.cos(th), mp.sin(th)
    return ((r * cs, r * (abs(cs) + th * abs(sn))), (r * sn, r * (abs(sn) + th * abs(cs))))


def draws(kind, df, ints, rows, D):
    """rows x D lists (T, S_T) of mp numbers; ints = rng_oracle.draw_ints(...)."""
    a, b, m1, m2 = ints
    dfm = None if df is None else mpf(float(df))
    out = []
    for r in range(rows):
        if kind == 'gauss':
            row = []
            for j in range((D + 1) // 2):
                row += list(_gauss_pair(m1[r, j], m2[r, j]))
            out.append(row[:D])
        else:
            out.append([_bailey(dfm, a[r, d], b[r, d]) for d in range(D)])
    return out


def _dlogq(kind, dfm, T):
    """(d log q / d T, sup |d2 log q / d T2|) of one coordinate."""
    if kind == 'gauss':
        return -T, mpf(1)
    return -(dfm + 1) * T / (dfm + T * T), (dfm + 1) / dfm


def reference(kind, df, target, lam, ints, rows):
    """Ref of `rows` log-weight draws of family (kind, df) at lam against target."""
    D = len(lam) // 2
    with mp.workdps(DIGITS):
        mu, ls = mm._lam(lam)
        sg = [mp.exp(v) for v in ls]
        dfm = None if df is None else mpf(float(df))
        tc = None if df is None else mm._t_const(dfm)
        e, eS, x, xS, lw, S_dir, S_back = [], [], [], [], [], [], []
        for row in draws(kind, df, ints, rows, D):
            T = [v[0] for v in row]
            ST = [v[1] for v in row]
            xs = [mu[d] + sg[d] * T[d] for d in range(D)]
            dx = [abs(mu[d]) + abs(sg[d] * T[d]) for d in range(D)]
            lp, s_lp, g, _ = tm.ROW[target](xs)
            q = [mm._logq1(kind, dfm, tc, ls[d], T[d]) for d in range(D)]
            dq = [_dlogq(kind, dfm, T[d]) for d in range(D)]
            s = (s_lp + mp.fsum(abs(g[d]) * dx[d] for d in range(D)) + mp.fsum(v[1] for v in q)
                 + mp.fsum(abs(sg[d] * g[d] - dq[d][0]) * ST[d] for d in range(D)))
            back = mp.fsum(abs(dq[d][0]) * dx[d] / sg[d]
                           + dq[d][1] / 2 * mpf(UNIT) * (dx[d] / sg[d]) ** 2 for d in range(D))
            e.append(T)
            eS.append(ST)
            x.append(xs)
            xS.append([abs(mu[d]) + sg[d] * ST[d] for d in range(D)])
            lw.append(lp - mp.fsum(v[0] for v in q))
            S_dir.append(s)
            S_back.append(s + back)
        return Ref(mm._val(e, eS), mm._val(x, xS), mm._val(lw, S_dir), mm._val(lw, S_back))


# ---- the cases' references: computed once per process and shared (about 20 s for all) ----
@functools.lru_cache(maxsize=None)
def _case_reference(cid, step):
    from oracle import rng_oracle as ro
    from tests import logw_cases as lc
    c = lc.BY_ID[cid]
    ints = ro.draw_ints(lc.SEED, c['stream'], step, c['rows'][step], c['D'])
    ref = reference(c['kind'], c['df'], c['target'], c['lam'], ints, c['rows'][step])
    for v in ref:
        for a in v:
            a.setflags(write=False)
    return ref


def case_reference(c, step):
    """The shared, read-only Ref of a case of tests/logw_cases.py at a step."""
    return _case_reference(c['id'], step)


def rows_of(val, m):
    """The first m rows of a Val."""
    return mm.Val(val.hi[:m], val.lo[:m], val.S[:m])


# Worst error of the oracle per class over every case of tests/logw_cases.py, in units
# of 2^-53 S: the C oracle's draws (oracle/vbrng.c, libm) against the multiprecision draw,
# the numpy oracle's transform and log_weights (oracle/vb_oracle.py) on those draws
# against the multiprecision sample and log weight ('back': the oracle reads log q back
# from x).  Measured by tests/test_oracle_logw_mp.py, which asserts twice these figures;
# the GPU test allows the device 8 times them.  'sample' and 'log_w' coincide with
# MF_ORACLE_ERR's 'transform' and 'log_w': where the new cases measure no worse, the
# existing figure stands (bar()).
LOGW_ORACLE_ERR = {
    'draw': 1.94,         # grid/mat/funnel/D40 (t40, central lam)
    'sample': 2.62,       # edge/row/eight_schools_ncp/D10/t2.5/ls5.0/mu0 (above 'transform' 2.40: this figure)
    'log_w': 1.79,        # tail/b0+/s83296/row/funnel/D5/t2.000001 (below MF_ORACLE_ERR's 1.83, which stands)
}
_SAME_AS = {'sample': 'transform', 'log_w': 'log_w'}


def oracle_figure(cls):
    old = mm.MF_ORACLE_ERR.get(_SAME_AS.get(cls))
    new = LOGW_ORACLE_ERR[cls]
    return old if old is not None and new <= old else new


def bar(cls):
    return 8.0 * oracle_figure(cls)
