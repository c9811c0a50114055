"""Multiprecision restatement (mpmath, 50 digits) of the regression target with a learned
scale or dispersion, its condition sums, and the edge data and rows; shared by the CPU
test that pins the numpy restatement of tests/aux_cases.py (tests/test_oracle_aux_mp.py)
and the GPU tests of the learned instances of vb_glm.hip (tests/test_gpu_aux_edges.py).

Written from the densities literally, not from the form the kernels evaluate
(z = [beta (p), lambda], theta = e^lambda, eta_m = x_m . beta + eta0_m, r = y - eta):

  beta_d ~ N(0, s^2):        -beta_d^2 / (2 s^2) - log(2 pi)/2 - log s
  theta ~ half-Cauchy(0, s_aux), in lambda with the Jacobian:
                             log(2 / (pi s_aux (1 + (theta / s_aux)^2))) + lambda
  gaussian   (sigma = theta) -log sigma - r^2 / (2 sigma^2) - log(2 pi)/2
  student_t  (sigma = theta) loggamma((nu+1)/2) - loggamma(nu/2) - log(nu pi)/2 - log sigma
                             - (nu+1)/2 log(1 + r^2 / (nu sigma^2))
  neg_binomial_2_log (phi = theta)
                             loggamma(y + phi) - loggamma(phi) - loggamma(y + 1)
                             + phi log(phi) - (phi + y) log(phi + e^eta) + y eta

The lambda gradient is mp.diff of that literal row density in lambda.  A central
difference at working precision w leaves an absolute error ~ 2^-w F, F the largest term of
the density (phi log phi ~ 1e176 at the far row of the dispersion), so a row is evaluated at
50 + 30 + 2 |lambda| / log(10) digits and rounded to the (hi, lo) pair from there.  The
coefficient gradient is the exact integer dot product of the 50-digit dl/deta with x, as in
tests/glm_mp.py; every eta is an exact dot product.

Error metric: that of tests/targets_mp.py, err = |got - ref| / (2^-53 S).  S is built as in
tests/glm_mp.py and tests/count_mp.py (a_m = sum_d |x_md beta_d| + |y_m| for gaussian and
student_t; + |eta0_m| + |lambda| instead of |y_m| for the negative binomial, where
zeta = eta - lambda is one more term of the inner sum) and also carries the terms that
lambda adds.  With q = r / sigma, w = 2 (lambda - log s_aux), sp / lg the softplus and the
logistic, zeta = eta - lambda:

  S_lp = sum_d beta_d^2 / (2 s^2) + p |log(2 pi)/2 + log s|           (prior of beta)
         + |log(2 / (pi s_aux))| + sp(w) + |lambda|                     (prior of lambda)
         + M |c_obs| + M |lambda| + sum_m [T(l_m) + |l'_m| a_m]         (gaussian, student_t;
                                                c_obs without its -log sigma)
         + sum_m loggamma(y_m + 1) + A + sum_m [T(l_m) + |l'_m| a_m]    (negative binomial)
         A = sum_j T_j log1p(j / phi) = sum_m [loggamma(y_m + phi) - loggamma(phi) - y_m log phi]
  S_g_d = |beta_d| / s^2 + sum_m [T(l'_m) + |l''_m| a_m] |x_md|         (d < p, as there,
                                                sigma = e^lambda, phi = e^lambda)
  S_g_lambda = 1 + 2 lg(w)                                              (prior of lambda)
         + M + sum_m [T(v_m) + |dv_m / deta| a_m],  v_m the observation's share:
           gaussian   v = q^2,                          |dv/deta| = 2 |q| / sigma
           student_t  v = (nu+1) q^2 / (nu + q^2),      |dv/deta| = 2 (nu+1) nu |q| / (nu + q^2)^2 / sigma
         + sum_m [(y_m + phi) lg(zeta_m) + phi sp(zeta_m) + |dv_m / dzeta| a_m] + |dA / dlambda|
           negative binomial: v = (y + phi) lg - phi sp, the pair that is subtracted,
           |dv/dzeta| = |(y + phi) lg (1 - lg) - phi lg|,  dA/dlambda = -sum_j T_j j / (phi + j)

  T(l), T(l'), |l''| per likelihood are those of tests/glm_mp.py and tests/count_mp.py.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import aux_cases as ac
from tests import count_cases as cc
from tests import glm_mp as gm
from tests.targets_mp import DIGITS, RANDOM_SHARE, UNIT, Ref, available, errors  # noqa: F401

try:
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mp = mpf = None

LOG10 = math.log(10.0)


def row_digits(lam):
    """Working digits of one row (module docstring)."""
    return DIGITS + 30 + int(2.0 * abs(lam) / LOG10)


def _row_density(lik, lam, etas, Y, ycount, nu, s_aux):
    """The literal log density of one row without the prior of beta, as a function of
    lambda (mpf): the observations and the prior of theta = e^lambda."""
    theta = mp.exp(lam)
    out = mp.log(2 / (mp.pi * s_aux * (1 + (theta / s_aux) ** 2))) + lam
    terms = []
    if lik == 'neg_binomial_2_log':
        lphi = mp.log(theta)
        lg_phi = mp.loggamma(theta)
        for v, c in ycount:
            terms.append(c * (mp.loggamma(v + theta) - lg_phi - mp.loggamma(v + 1)))
        for eta, yv in zip(etas, Y):
            terms.append(theta * lphi - (theta + yv) * mp.log(theta + mp.exp(eta)) + yv * eta)
        return out + mp.fsum(terms)
    half_l2pi = mp.log(2 * mp.pi) / 2
    if lik == 'gaussian':
        c = -mp.log(theta) - half_l2pi
        for eta, yv in zip(etas, Y):
            r = yv - eta
            terms.append(c - r * r / (2 * theta * theta))
    else:
        c = (mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2
             - mp.log(theta))
        for eta, yv in zip(etas, Y):
            r = yv - eta
            terms.append(c - (nu + 1) / 2 * mp.log(1 + r * r / (nu * theta * theta)))
    return out + mp.fsum(terms)


def _obs_terms(lik, eta, y, theta, nu):
    """(l', T(l), T(l'), |l''|, T(v), |dv/deta|) of one observation at scale / dispersion
    theta; all but the first as floats (module docstring)."""
    if lik == 'neg_binomial_2_log':
        e = mp.exp(eta)
        pr = e / (theta + e)                       # lg(zeta)
        sp = mp.log(theta + e) - mp.log(theta)     # sp(zeta)
        dl = y - (y + theta) * pr
        return (dl, float(abs(y * eta) + (y + theta) * sp), float(y + (y + theta) * pr),
                float((y + theta) * pr * (1 - pr)), float((y + theta) * pr + theta * sp),
                float(abs((y + theta) * pr * (1 - pr) - theta * pr)))
    r = y - eta
    q = r / theta
    if lik == 'gaussian':
        return (q / theta, float(q * q / 2), float(abs(q) / theta), float(1 / theta ** 2),
                float(q * q), float(2 * abs(q) / theta))
    k3, r2 = nu * theta * theta, r * r
    dl = (nu + 1) * r / (k3 + r2)
    return (dl, float((nu + 1) / 2 * mp.log(1 + q * q / nu)), float(abs(dl)),
            float((nu + 1) * abs(k3 - r2) / (k3 + r2) ** 2),
            float((nu + 1) * q * q / (nu + q * q)),
            float(2 * (nu + 1) * nu * abs(q) / (nu + q * q) ** 2 / theta))


def reference(x, y, z, likelihood='gaussian', df=None, offset=None, prior_scale=10.0,
              hyper_scale=5.0):
    """Ref of the learned model (x [M][p], y [M], ...) at the rows of z [n][p + 1]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    (M, p), n = x.shape, z.shape[0]
    D = p + 1
    assert z.shape[1] == D
    nb = likelihood == 'neg_binomial_2_log'
    eta0 = np.zeros(M) if offset is None else np.asarray(offset, dtype=np.float64)
    beta = z[:, :p]
    ix, ex = gm._ints(x)
    ib, eb = gm._ints(beta)
    eta_i = np.dot(ib, ix.T)                                  # exact, [n][M]
    a = np.abs(beta) @ np.abs(x).T
    vals, counts = np.unique(y, return_counts=True)
    T, _ = ac.dispersion_table(y) if nb else (np.zeros(0), 0.0)
    js = np.arange(T.size, dtype=float)
    out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
    for r in range(n):
        lam64 = float(z[r, p])
        with mp.workdps(row_digits(lam64)):
            s, s_aux = mpf(float(prior_scale)), mpf(float(hyper_scale))
            nu = mpf(float(df)) if likelihood == 'student_t' else None
            lam = mpf(lam64)
            theta = mp.exp(lam)
            Y = [mpf(v) for v in y.tolist()]
            ycount = [(mpf(v), c) for v, c in zip(vals.tolist(), counts.tolist())]
            etas = [mp.ldexp(mpf(int(eta_i[r, m])), ex + eb) + mpf(float(eta0[m]))
                    for m in range(M)]
            B = [mpf(v) for v in beta[r].tolist()]
            c_prior = mp.log(2 * mp.pi) / 2 + mp.log(s)
            ss = mp.fsum(B, squared=True) / (2 * s * s)

            def dens(L):
                return _row_density(likelihood, L, etas, Y, ycount, nu, s_aux)
            lp = dens(lam) - ss - p * c_prior
            gl = mp.diff(dens, lam)
            # condition sums
            am = a[r] + (np.abs(eta0) + abs(lam64) if nb else np.abs(y))
            dls = []
            t_l, t_g, d2, t_v, dv, adl = (np.empty(M) for _ in range(6))
            for m in range(M):
                dl, t_l[m], t_g[m], d2[m], t_v[m], dv[m] = _obs_terms(likelihood, etas[m], Y[m],
                                                                     theta, nu)
                dls.append(dl)
                adl[m] = abs(float(dl))
            w = 2 * (lam - mp.log(s_aux))
            sp_w = float(mp.log(1 + mp.exp(w)))
            lg_w = float(1 / (1 + mp.exp(-w)))
            s_lp = (float(ss) + float(p * abs(c_prior)) + float(abs(mp.log(2 / (mp.pi * s_aux))))
                    + sp_w + abs(lam64) + float(np.sum(t_l + adl * am)))
            s_gl = 1.0 + 2.0 * lg_w + float(np.sum(t_v + dv * am))
            if nb:
                ph = float(theta)
                with np.errstate(over='ignore'):
                    A = float(np.sum(T[1:] * np.log1p(js[1:] / ph))) if T.size > 1 else 0.0
                    dA = float(np.sum(T[1:] * (js[1:] / (ph + js[1:])))) if T.size > 1 else 0.0
                s_lp += float(sum(c * mp.loggamma(v + 1) for v, c in ycount)) + A
                s_gl += dA
            else:
                if likelihood == 'gaussian':
                    c_obs = mp.log(2 * mp.pi) / 2
                else:
                    c_obs = abs(mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2)
                                - mp.log(nu * mp.pi) / 2)
                s_lp += M * float(c_obs) + M * abs(lam64)
                s_gl += M
            out.lp_hi[r], out.lp_lo[r] = gm._split(lp)
            out.lp_S[r] = s_lp
            out.g_hi[r, p], out.g_lo[r, p] = gm._split(gl)
            out.g_S[r, p] = s_gl
            with mp.workdps(DIGITS + 30):
                il, el = gm._mp_ints([+v for v in dls])
            gi = np.dot(il, ix)                               # exact, [p]
            for d in range(p):
                g = mp.ldexp(mpf(int(gi[d])), el + ex) - B[d] / (s * s)
                out.g_hi[r, d], out.g_lo[r, d] = gm._split(g)
            # (|l''| = 1 / sigma^2 leaves the range at the far row lambda = log s_aux - 400:
            # S is then inf wherever an observation has a_m |x_md| > 0, and the entry is
            # only asked to be finite; 0 inf is taken as 0)
            with np.errstate(over='ignore', invalid='ignore'):
                cond = np.where(am > 0, d2 * am, 0.0)
                gs = np.where(np.abs(x) > 0, (t_g + cond)[:, None] * np.abs(x), 0.0).sum(axis=0)
            out.g_S[r, :p] = np.abs(beta[r]) / float(prior_scale) ** 2 + gs
    return out


# ---- the shapes (p, M, n): which instance each reaches --------------------------------
# The learned block is served by p as a fixed block with D = p is: p <= 16 the lane-per-row
# kernel (DP = 2, 4, 8, 16), p > 16 the matrix kernel (p <= 32 one LDS slice and NCT = 2,
# p <= 64 NCT = 4, above NCT = 8 and 128-column slabs); a chunk is 64 observations here.
SHAPES = (
    (1, 1, 1), (1, 65, 65),             # DP = 2; two row blocks and two chunks
    (3, 64, 63), (7, 129, 10),          # DP = 4, 8; three chunks
    (15, 65, 10), (16, 130, 70),        # the last lane-per-row sizes
    (17, 15, 15),                       # the first matrix size
    (31, 16, 16), (32, 17, 17), (33, 17, 17),      # one slice or two, lambda as column 32
    (63, 65, 16), (64, 65, 17), (65, 65, 17),      # NCT 4 -> 8
    (127, 70, 16), (128, 70, 17), (129, 70, 17),   # lambda at a slab edge, alone behind the
                                                   # last slab, behind a one-column slab
    (130, 321, 10),                     # two slabs and six chunks
)
SHAPES_VALUE = ((3, 65, 64), (20, 65, 17), (130, 321, 10))
SHAPE_TABLE = (2, 40, 17)
ALL_SHAPES = tuple(dict.fromkeys(SHAPES + SHAPES_VALUE + (SHAPE_TABLE,)))

PRIOR_SCALES = (1e-3, 3.0, 1e3)
HYPER_SCALES = (1e-3, 5.0, 1e3)
DFS = (0.5, 5.0, 1e6)
LAMS = {'scale': (math.log(1e-3), math.log(0.7), math.log(1e3)),
        'phi': (math.log(1e-3), 0.0, math.log(1e6))}
TAIL = 400.0                           # lambda - log s_aux of the softplus tail rows
ZETAS = (1e-9, -1e-9, 36.8, -36.8, 746.0, -746.0)      # eta - log phi of the placed observations
Y_EDGE = (0.0, 1.0, 7.0, 1000.0)
OFFSET_EDGE = (0.0, 1e-9, -1e-9, -30.0, 12.0)
# the responses of the negative binomial by shape: all zero (J = 0, no table), zeros and
# ones (J = 1, an empty sum), one y = 65536 among small counts
Y_KIND = {(3, 64, 63): 'zero', (33, 17, 17): 'zero', (7, 129, 10): 'binary',
          (64, 65, 17): 'binary', (15, 65, 10): 'big', (65, 65, 17): 'big'}
TABLE_KINDS = ('zero', 'binary', 'big')
Y_BIG = 65536.0
SEED = 20241021

Case = namedtuple('Case', 'x y offset kw z info')


def cases():
    """Every (likelihood, p, M, n) of the edge tests."""
    return [(lik, p, M, n) for p, M, n in ALL_SHAPES if (p, M, n) != SHAPE_TABLE
            for lik in ac.LIKELIHOODS]


def table_cases():
    """The J = 0, 1 and 65536 tables at SHAPE_TABLE."""
    return [('neg_binomial_2_log',) + SHAPE_TABLE + (kind,) for kind in TABLE_KINDS]


def case_kwargs(lik, i):
    li = ac.LIKELIHOODS.index(lik)
    return ac.model_kwargs(lik, df=DFS[i % 3], prior_scale=PRIOR_SCALES[(i + i // 3 + li) % 3],
                           hyper_scale=HYPER_SCALES[(i + li) % 3])


def _counts(rs, x, comp, M, kind):
    p = x.shape[1]
    offset = np.where(rs.rand(M) < 0.4, 0.0, np.log(rs.uniform(0.5, 4.0, M)))
    eta_t = x @ (0.5 * rs.randn(p) / math.sqrt(p) * comp)
    y = cc.draw_counts(rs, 'neg_binomial_2_log', eta_t + offset, 3.0)
    for j, v in enumerate(Y_EDGE):
        if 2 + j < M:
            y[2 + j] = v
    for j, v in enumerate(OFFSET_EDGE):
        m = (0, 2, 3, 4, 5)[j]
        if m < M:
            offset[m] = v
    if kind == 'zero':
        y[:] = 0.0
    elif kind == 'binary':
        y = np.minimum(y, 1.0)
        y[0] = 1.0
    elif kind == 'big':
        y = np.minimum(y, 9.0)
        y[M // 2] = Y_BIG
    return y, offset


@functools.lru_cache(maxsize=None)
def edge_case(lik, p, M, n, kind=None):
    """The seeded edge data and rows of one case.

    Data: tests/glm_mp.py's column roles (column 1 all zero, 2 scaled by 1e-6, 3 by 1e3, as
    far as p has room), observation 1 all zero (M >= 3).  gaussian, student_t: y = column 0
    of x exactly, so the row beta = e_0 has every residual exactly 0 (and d/dlambda = -M
    plus the prior's) and the rows (1 + 1e-9) e_0, (1 - 1e-12) e_0 and, for student_t,
    (1 + 1e6) e_0 have residuals of those sizes relative to y.  Negative binomial: counts
    drawn at phi = 3, Y_EDGE at observations 2..5, OFFSET_EDGE at 0, 2, 3, 4, 5, and the
    shapes of Y_KIND (or `kind`) all zero, zeros and ones, or one y = 65536.
    Rows, as many as the case has edge rows, the list rotated by the case's index so that a
    case with few rows starts elsewhere: beta = 0; the zero-residual row at a value of LAMS,
    at log s_aux - 400 and at log s_aux + 400 (for the negative binomial random small beta
    at both tails); random beta at lambda = log s_aux exactly and at log s_aux + 400; the
    small-residual rows; for the negative binomial one row per ZETAS that puts an
    observation with offset 0 at eta = lambda + zeta (beta along a random direction, as
    tests/count_mp.py places its etas); then 0.8 randn scaled by 1, min(1, s), 5, 0.01 in
    turn with lambda cycling over LAMS.  The last RANDOM_SHARE of the rows are 0.8 randn
    with lambda = log 0.7 (log 3) + 0.5 randn.  The 1e3 column's coefficient is scaled by
    1e-3 in every row."""
    i, li = ALL_SHAPES.index((p, M, n)), ac.LIKELIHOODS.index(lik)
    nb = lik == 'neg_binomial_2_log'
    kind = kind or Y_KIND.get((p, M, n))
    rs = np.random.RandomState(SEED + 100 * i + li + 7 * (TABLE_KINDS.index(kind) + 1 if kind else 0))
    kw = case_kwargs(lik, i)
    cols = {k: v for k, v in gm.special_columns(p).items() if k != 'ortho'}
    zero_obs = 1 if M >= 3 else None
    x = rs.randn(M, p)
    comp = np.ones(p)
    if 'zero' in cols:
        x[:, cols['zero']] = 0.0
    if 'small' in cols:
        x[:, cols['small']] *= 1e-6
    if 'big' in cols:
        x[:, cols['big']] *= 1e3
        comp[cols['big']] = 1e-3
    if zero_obs is not None:
        x[zero_obs] = 0.0
    if nb:
        y, offset = _counts(rs, x, comp, M, kind)
    else:
        y, offset = x[:, 0].copy(), None

    lams = LAMS['phi' if nb else 'scale']
    ls = math.log(kw['hyper_scale'])
    e0 = np.zeros(p)
    e0[0] = 1.0

    def rnd(scale=0.8):
        return rs.randn(p) * scale * comp

    edge, slots = [], []
    edge.append((np.zeros(p), lams[i % 3], 'zero beta'))
    if nb:
        edge.append((rnd(0.3), ls - TAIL, 'tail -'))
        edge.append((rnd(0.3), ls + TAIL, 'tail +'))
        edge.append((rnd(), ls, 'at s_aux'))
        free = np.nonzero((offset == 0.0) & (np.arange(M) != zero_obs))[0]
        for kz, v in enumerate(ZETAS):
            lam = lams[(i + kz) % 3]
            if free.size == 0:
                break
            for _ in range(400):
                u = rs.randn(p) * comp
                tgt = lam + v
                qv = (x @ u) * math.copysign(1.0, tgt)
                m = int(free[np.argmax(qv[free])])
                if not qv[m] > 0.0:
                    continue
                b = u * (tgt / (x[m] @ u))
                if abs((x[m] @ b - lam) - v) > max(1e-3 * abs(v), 1e-12):
                    continue
                edge.append((b, lam, 'zeta %g' % v))
                slots.append((m, v))
                break
    else:
        edge.append((e0.copy(), lams[(i + 1) % 3], 'zero residual'))
        edge.append((e0.copy(), ls - TAIL, 'zero residual, tail -'))
        edge.append((e0.copy(), ls + TAIL, 'zero residual, tail +'))
        edge.append((rnd(), ls, 'at s_aux'))
        edge.append((e0 * (1.0 + 1e-9), lams[(i + 2) % 3], 'residual 1e-9'))
        edge.append((e0 * (1.0 - 1e-12), lams[i % 3], 'residual 1e-12'))
        edge.append((rnd(), ls + TAIL, 'tail +'))
        if lik == 'student_t':
            edge.append((e0 * (1.0 + 1e6), lams[(i + 1) % 3], 'residual 1e6'))
    edge = edge[i % len(edge):] + edge[:i % len(edge)]

    n_rand = max(1, int(round(RANDOM_SHARE * n))) if n > 1 else 0
    n_edge = n - n_rand
    mags = (1.0, min(1.0, kw['prior_scale']), 5.0, 0.01)
    z = np.empty((n, p + 1))
    labels = []
    for r in range(n_edge):
        if r < len(edge):
            z[r, :p], z[r, p] = edge[r][0], edge[r][1]
            labels.append(edge[r][2])
        else:
            z[r, :p], z[r, p] = rnd(0.8 * mags[r % 4]), lams[(r + i) % 3]
            labels.append('edge randn')
    z[n_edge:, :p] = rs.randn(n_rand, p) * 0.8 * comp
    z[n_edge:, p] = math.log(3.0 if nb else 0.7) + 0.5 * rs.randn(n_rand)
    info = dict(cols=cols, zero_obs=zero_obs, n_edge=n_edge, labels=labels, slots=slots, kind=kind)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(z))
    # the float64 restatement stays finite on the whole case
    with np.errstate(over='raise', divide='raise', invalid='raise', under='ignore'):
        lp, g = ac.restatement(x, y, offset=offset, **kw)(z)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), (lik, p, M, n)
    for arr in (x, y, z) + (() if offset is None else (offset,)):
        arr.setflags(write=False)
    return Case(x, y, offset, kw, z, info)


@functools.lru_cache(maxsize=None)
def edge_reference(lik, p, M, n, kind=None):
    """(Case, Ref at case.z) of one case, computed once per process and shared."""
    c = edge_case(lik, p, M, n, kind)
    ref = reference(c.x, c.y, c.z, offset=c.offset, **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


# Worst error of the numpy restatement (tests/aux_cases.py) over cases() and table_cases()
# per likelihood, value and gradient entries together, in units of 2^-53 S; measured by
# tests/test_oracle_aux_mp.py, which asserts twice these figures.  The GPU tests allow the
# kernels 8 times them.
AUX_ORACLE_ERR = {
    # value at (p, M, n) = (130, 321, 10), row 9 (coefficients 2.59, lambda entry 0.77 there)
    'gaussian': 3.27,
    # value at (127, 70, 16), row 12 (coefficients 2.50, lambda entry 2.29 there)
    'student_t': 3.94,
    # coefficient 7 at (16, 130, 70), row 58: the order of the sum over m, as in
    # tests/count_mp.py's figure (value 1.00, lambda entry 2.07 in the same case)
    'neg_binomial_2_log': 10.88,
}
