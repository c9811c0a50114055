"""Multiprecision restatement of the two count likelihoods (mpmath, 50 digits) for the
regression and the multilevel target, their condition sums, and the edge data and rows;
shared by the CPU test that pins the numpy restatement of tests/count_cases.py and the
packer's c_data (tests/test_oracle_count_mp.py) and the GPU tests of the count instances
of vb_glm.hip and vb_mlm.hip (tests/test_gpu_count_edges.py).

Written from the probability mass functions, not from the form the kernels evaluate
(mu = e^eta, eta_m = x_m . beta + eta0_m, plus the group's intercept in the multilevel
target):

  poisson_log         log P(y) = y eta - e^eta - loggamma(y + 1)
  neg_binomial_2_log  log P(y) = loggamma(y + phi) - loggamma(phi) - loggamma(y + 1)
                                 + phi log(phi) - (phi + y) log(phi + e^eta) + y eta
  l' = d log P / d eta:  y - e^eta;   y - (y + phi) e^eta / (phi + e^eta)

with log(phi + e^eta) taken literally at 50 digits.  Priors, coordinates and the
multilevel terms are those of tests/glm_mp.py and tests/mlm_mp.py.

Error metric: that of tests/targets_mp.py, err = |got - ref| / (2^-53 S), S the sum of
the absolute values of the terms added to form the result, an observation's cancelling
inner sum eta carried through the term's derivative as in tests/glm_mp.py's docstring:

  S_lp  = (prior terms as there) + S_c + sum_m [T(l_m) + |l'_m| a_m]
  S_g_d = |beta_d| / s^2 + sum_m [T(l'_m) + |l''_m| a_m] |x_md|
  a_m   = sum_d |x_md beta_d| + |eta0_m|  (+ |a_eff| in the multilevel target)
          (+ |log phi| for the negative binomial: zeta = eta - log phi is one more term of
          the inner sum, and log phi is itself a rounded double)
  S_c   = sum_m [loggamma(y_m + 1) + sum_{j < y_m} log(1 + j / phi)]   (the second sum for
          the negative binomial only: loggamma(y + phi) - loggamma(phi) - y log(phi) as
          the non-negative terms it is made of); c_data itself is measured against S_c

  poisson_log         T(l) = |y eta| + e^eta              T(l') = y + e^eta    |l''| = e^eta
  neg_binomial_2_log  with zeta = eta - log phi, sp = log(1 + e^zeta), p = 1 / (1 + e^-zeta):
                      T(l) = |y eta| + (y + phi) sp       T(l') = y + (y + phi) p
                      |l''| = (y + phi) p (1 - p)

The multilevel S of the intercepts and of u are tests/mlm_mp.py's with R_m = T(l'_m) +
|l''_m| a_m.  Every eta is an exact integer dot product (tests/glm_mp.py's _ints) plus
the exact offset (and the 50-digit intercept), rounded once to 50 digits.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import count_cases as cc
from tests import glm_mp as gm
from tests import mlm_cases as mc
from tests import mlm_mp as mm
from tests import targets_mp as tm
from tests.targets_mp import DIGITS, RANDOM_SHARE, UNIT, Ref, errors   # noqa: F401

try:
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mp = mpf = None


def available():
    return tm.available()


SATURATED = 5000.0


# ---- the links, from the pmf ------------------------------------------------------
def _link(lik, eta, y, phi):
    """(l without the data-only constant, l', T(l), T(l'), |l''|) of one observation;
    the last three as floats."""
    if lik == 'neg_binomial_2_log' and abs(eta) > SATURATED:
        # e^-|eta| < 1e-2171 is taken as 0, as tests/mlm_mp.py does for the logit link (a
        # non-centred row at log tau = 20 has eta ~ 1e8, whose exponential costs mpmath
        # seconds): log(phi + e^eta) = max(eta, log phi) to 1e-2000 of the S it is measured in
        lphi = mp.log(phi)
        if eta > 0:
            return (y * (lphi + eta) + phi * lphi - (phi + y) * eta, -phi,
                    float(abs(y * eta) + (y + phi) * (eta - lphi)), float(2 * y + phi), 0.0)
        return y * eta, y, float(abs(y * eta)), float(y), 0.0
    e = mp.exp(eta)
    if lik == 'poisson_log':
        return y * eta - e, y - e, float(abs(y * eta) + e), float(y + e), float(e)
    lg = mp.log(phi + e)
    # log P without the three loggamma: the y log(phi) of the data-only constant restored
    l = phi * mp.log(phi) - (phi + y) * lg + y * eta + y * mp.log(phi)
    pr = e / (phi + e)
    sp = lg - mp.log(phi)
    return (l, y - (y + phi) * pr, float(abs(y * eta) + (y + phi) * sp),
            float(y + (y + phi) * pr), float((y + phi) * pr * (phi / (phi + e))))


def c_data_reference(y, lik, phi=None):
    """(sum_m c_m as (hi, lo), S_c): c_m = -loggamma(y + 1), plus loggamma(y + phi) -
    loggamma(phi) - y log(phi) for the negative binomial."""
    with mp.workdps(DIGITS):
        vals, counts = np.unique(np.asarray(y, dtype=np.float64), return_counts=True)
        tot, S = mpf(0), mpf(0)
        for v, c in zip(vals.tolist(), counts.tolist()):
            v = mpf(v)
            f = mp.loggamma(v + 1)
            cm, sm = -f, f
            if lik == 'neg_binomial_2_log':
                p = mpf(float(phi))
                r = mp.loggamma(v + p) - mp.loggamma(p) - v * mp.log(p)
                cm, sm = cm + r, sm + abs(r)
            tot, S = tot + c * cm, S + c * sm
        return gm._split(tot), float(S)


def _prep(lik, x, y, offset, phi):
    M = x.shape[0]
    eta0 = np.zeros(M) if offset is None else np.asarray(offset, dtype=np.float64)
    (c_hi, c_lo), s_c = c_data_reference(y, lik, phi)
    ph = mpf(float(phi)) if lik == 'neg_binomial_2_log' else None
    extra = np.abs(eta0) + (abs(math.log(phi)) if ph is not None else 0.0)
    return eta0, mpf(c_hi) + mpf(c_lo), s_c, ph, extra


def reference(x, y, beta, likelihood='poisson_log', phi=None, offset=None, prior_scale=10.0):
    """Ref of targets.regression's count models at the rows of beta [n][D]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    (M, D), n = x.shape, beta.shape[0]
    with mp.workdps(DIGITS):
        eta0, c_data, s_c, ph, extra = _prep(likelihood, x, y, offset, phi)
        s = mpf(float(prior_scale))
        c_prior = mp.log(2 * mp.pi) / 2 + mp.log(s)
        c_all = -D * c_prior + c_data
        s_const = float(D * abs(c_prior)) + s_c
        Y = [mpf(v) for v in y.tolist()]
        E0 = [mpf(v) for v in eta0.tolist()]
        ix, ex = gm._ints(x)
        ib, eb = gm._ints(beta)
        eta_i = np.dot(ib, ix.T)                              # exact, [n][M]
        a = np.abs(beta) @ np.abs(x).T + extra[None, :]
        out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
        t_l, t_g, d2, adl = np.empty(M), np.empty(M), np.empty(M), np.empty(M)
        for r in range(n):
            ls, dls = [], []
            for m in range(M):
                eta = mp.ldexp(mpf(eta_i[r, m]), ex + eb) + E0[m]
                l, dl, t_l[m], t_g[m], d2[m] = _link(likelihood, eta, Y[m], ph)
                ls.append(l)
                dls.append(dl)
                adl[m] = abs(float(dl))
            B = [mpf(v) for v in beta[r].tolist()]
            ss = mp.fsum(B, squared=True) / (2 * s * s)
            out.lp_hi[r], out.lp_lo[r] = gm._split(c_all - ss + mp.fsum(ls))
            out.lp_S[r] = float(ss) + s_const + float(np.sum(t_l + adl * a[r]))
            il, el = gm._mp_ints(dls)
            gi = np.dot(il, ix)                               # exact, [D]
            for d in range(D):
                g = mp.ldexp(mpf(gi[d]), el + ex) - B[d] / (s * s)
                out.g_hi[r, d], out.g_lo[r, d] = gm._split(g)
            out.g_S[r] = np.abs(beta[r]) / float(prior_scale) ** 2 + (t_g + d2 * a[r]) @ np.abs(x)
    return out


def mlm_reference(x, y, group, z, likelihood='poisson_log', phi=None, offset=None,
                  prior_scale=10.0, tau_scale=5.0, centered=False, n_groups=None):
    """Ref of targets.multilevel_regression's count models at the rows of z [n][p + 1 + G]
    (tests/mlm_mp.py's reference with the count links and the offset)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    group = np.asarray(group).astype(np.int64)
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    (M, p), n = x.shape, z.shape[0]
    G = int(group.max()) + 1 if n_groups is None else int(n_groups)
    D = p + 1 + G
    assert z.shape[1] == D
    members = [np.nonzero(group == g)[0] for g in range(G)]
    with mp.workdps(DIGITS):
        eta0, c_data, s_c, ph, extra = _prep(likelihood, x, y, offset, phi)
        s, st = mpf(float(prior_scale)), mpf(float(tau_scale))
        half_l2pi = mp.log(2 * mp.pi) / 2
        c_prior = half_l2pi + mp.log(s)
        c_tau = mp.log(2 / (mp.pi * st))
        c_all = -p * c_prior + c_data + c_tau - G * half_l2pi
        s_const = float(p * abs(c_prior) + abs(c_tau) + G * half_l2pi) + s_c
        Y = [mpf(v) for v in y.tolist()]
        E0 = [mpf(v) for v in eta0.tolist()]
        ix, ex = gm._ints(x)
        ib, eb = gm._ints(z[:, :p])
        xb_i = np.dot(ib, ix.T)                               # exact, [n][M]
        xb_abs = np.abs(z[:, :p]) @ np.abs(x).T + extra[None, :]
        out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
        t_l, R, adl, A = np.empty(M), np.empty(M), np.empty(M), np.empty(M)
        for r in range(n):
            B = [mpf(v) for v in z[r, :p].tolist()]
            u = mpf(float(z[r, p]))
            a = [mpf(v) for v in z[r, p + 1:].tolist()]
            tau = mp.exp(u)
            w = (tau / st) ** 2
            aeff = a if centered else [tau * v for v in a]
            ls, dls = [], []
            for m in range(M):
                ae = aeff[group[m]]
                eta = mp.ldexp(mpf(xb_i[r, m]), ex + eb) + ae + E0[m]
                l, dl, t_l[m], t_g, d2 = _link(likelihood, eta, Y[m], ph)
                ls.append(l)
                dls.append(dl)
                A[m] = xb_abs[r, m] + float(abs(ae))
                adl[m] = abs(float(dl))
                R[m] = t_g + d2 * A[m]
            ss = mp.fsum(B, squared=True) / (2 * s * s)
            l1 = mp.log1p(w)
            lp = c_all - ss - l1 + u + mp.fsum(ls)
            s_lp = float(ss) + s_const + float(l1) + float(abs(u)) + float(np.sum(t_l + adl * A))
            gw = 2 * w / (1 + w)
            gu, s_gu = 1 - gw, 1 + float(gw)
            if centered:
                zz = mp.fsum([(v / tau) ** 2 for v in a])
                lp -= G * u + zz / 2
                s_lp += float(G * abs(u) + zz / 2)
                gu += zz - G
                s_gu += float(zz) + G
            else:
                aa = mp.fsum(a, squared=True)
                lp -= aa / 2
                s_lp += float(aa / 2)
            for g in range(G):
                Sg = mp.fsum([dls[m] for m in members[g]])
                Rg = float(np.sum(R[members[g]]))
                if centered:
                    ga = Sg - a[g] / tau ** 2
                    s_ga = Rg + float(abs(a[g]) / tau ** 2)
                else:
                    ga = tau * Sg - a[g]
                    s_ga = float(tau) * Rg + float(abs(a[g]))
                    gu += tau * Sg * a[g]
                    s_gu += float(tau * abs(a[g])) * Rg
                out.g_hi[r, p + 1 + g], out.g_lo[r, p + 1 + g] = gm._split(ga)
                out.g_S[r, p + 1 + g] = s_ga
            out.lp_hi[r], out.lp_lo[r] = gm._split(lp)
            out.lp_S[r] = s_lp
            out.g_hi[r, p], out.g_lo[r, p] = gm._split(gu)
            out.g_S[r, p] = s_gu
            il, el = gm._mp_ints(dls)
            gi = np.dot(il, ix)                               # exact, [p]
            for d in range(p):
                gb = mp.ldexp(mpf(gi[d]), el + ex) - B[d] / (s * s)
                out.g_hi[r, d], out.g_lo[r, d] = gm._split(gb)
            out.g_S[r, :p] = np.abs(z[r, :p]) / float(prior_scale) ** 2 + R @ np.abs(x)
    return out


# ---- the regression shapes (D, M, n): which instance each reaches is in the docstring
# of tests/test_gpu_glm_edges.py ------------------------------------------------------
SHAPES_SMALL = ((1, 1, 1), (2, 65, 65), (4, 64, 63), (16, 130, 70))
SHAPES_MFMA = ((17, 15, 15), (33, 17, 17), (65, 65, 17), (129, 70, 17))
SHAPES_CHUNK = ((130, 321, 10),)
SHAPES_VALUE = ((3, 65, 64), (40, 321, 10))
ALL_SHAPES = SHAPES_SMALL + SHAPES_MFMA + SHAPES_CHUNK + SHAPES_VALUE
MLM_SHAPES = ((2, 1, 40), (3, 8, 129), (16, 70, 321), (17, 3, 65))    # of mlm_mp.SHAPES

PRIOR_SCALES = (1e-3, 3.0, 1e3)
PHIS = (1e-3, 1.0, 1e6)
Y_EDGE = (0.0, 1.0, 7.0, 1000.0)
OFFSET_EDGE = (0.0, 1e-9, -1e-9, -30.0, 12.0)
# eta of the placed observations: beside 0; where 1 + e^-|eta| rounds to 1; exp(-746)
# underflows to 0; +700 the last decade before exp's overflow (Poisson; +690 in the cases
# that have the 1e3 column, D >= 5); 709 where
# exp(-709) is subnormal (negative binomial, finite at any eta)
POIS_ETAS = (1e-9, -1e-9, 36.8, -36.8, -746.0, -800.0, 700.0)
NB_ETAS = (1e-9, -1e-9, 36.8, -36.8, 709.0, -709.0, 746.0, -746.0, 800.0, -800.0)
NB_ZETAS = (1e-9, -1e-9)              # eta = log(phi) + zeta
POIS_CAP = 705.0                      # no observation of a Poisson edge row above it (695
                                      # beside the 1e3 column)
ZERO_Y = ((3, 65, 64), (33, 17, 17), (3, 8, 129))       # shapes whose responses are all 0
SEED = 20240915

Case = namedtuple('Case', 'x y offset kw beta rows info')
MlmCase = namedtuple('MlmCase', 'x y group offset kw z')


def cases():
    """Every (likelihood, D, M, n) of the regression edge tests."""
    return [(lik, D, M, n) for D, M, n in ALL_SHAPES for lik in cc.LIKELIHOODS]


def mlm_cases():
    """Every (likelihood, centred, p, G, M) of the multilevel edge tests."""
    return [(lik, c, p, G, M) for (p, G, M) in MLM_SHAPES for c in mc.FORMS
            for lik in cc.LIKELIHOODS]


def case_kwargs(lik, i):
    li = cc.LIKELIHOODS.index(lik)
    return cc.model_kwargs(lik, phi=PHIS[(i + li) % 3], prior_scale=PRIOR_SCALES[(i + i // 3 + li) % 3])


def eta_targets(lik, kw):
    if lik == 'poisson_log':
        return list(POIS_ETAS)
    return [math.log(kw['phi']) + v for v in NB_ZETAS] + list(NB_ETAS)


def _edge_data(rs, lik, kw, x, eta_true, M, all_zero):
    """Responses and offsets: drawn from the model, then the edge values put at the
    observations after the all-zero one."""
    offset = np.where(rs.rand(M) < 0.4, 0.0, np.log(rs.uniform(0.5, 4.0, M)))
    y = cc.draw_counts(rs, lik, eta_true + offset, kw.get('phi'))
    for j, v in enumerate(Y_EDGE):
        if 2 + j < M:
            y[2 + j] = v
    for j, v in enumerate(OFFSET_EDGE):
        m = (0, 2, 3, 4, 5)[j]
        if m < M:
            offset[m] = v
    if all_zero:
        y[:] = 0.0
    return y, offset


@functools.lru_cache(maxsize=None)
def edge_case(lik, D, M, n):
    """The seeded edge data and rows of one regression case.

    Data: tests/glm_mp.py's column roles without the orthogonal one (column 1 all zero,
    2 scaled by 1e-6, 3 by 1e3, as far as D has room); observation 1 all zero (M >= 3);
    y = Y_EDGE at observations 2..5, all zero at the shapes of ZERO_Y; offsets 0 for two
    observations in five and log exposures in (0.5, 4) otherwise, OFFSET_EDGE at
    observations 0, 2, 3, 4, 5.
    Rows: 0 is beta = 0; from 2 on each row puts one observation at one value of
    eta_targets: beta = c u for a random direction u, the observation the one with the
    extreme x . u among those with offset 0, so every other eta - eta0 lies between 0 and
    the target or beyond 0 on the other side by the cloud's asymmetry; for the Poisson a
    direction is kept only if no observation passes POIS_CAP.  A case with fewer rows
    than targets starts the list at its own index, so every target is placed in several
    cases (info['slots'] = (row, observation, eta)).  The other edge rows are 0.8 randn
    scaled by 1, min(1, s), 5, 0.01 in turn, the last RANDOM_SHARE of the rows 0.8 randn;
    the 1e3 column's coefficient is scaled by 1e-3 in every row (e^eta must stay finite)."""
    i, li = ALL_SHAPES.index((D, M, n)), cc.LIKELIHOODS.index(lik)
    rs = np.random.RandomState(SEED + 100 * i + li)
    kw = case_kwargs(lik, i)
    cols = {k: v for k, v in gm.special_columns(D).items() if k != 'ortho'}
    zero_obs = 1 if M >= 3 else None
    x = rs.randn(M, D)
    comp = np.ones(D)
    if 'zero' in cols:
        x[:, cols['zero']] = 0.0
    if 'small' in cols:
        x[:, cols['small']] *= 1e-6
    if 'big' in cols:
        x[:, cols['big']] *= 1e3
        comp[cols['big']] = 1e-3
    if zero_obs is not None:
        x[zero_obs] = 0.0
    eta_t = x @ (0.5 * rs.randn(D) / math.sqrt(D) * comp)
    y, offset = _edge_data(rs, lik, kw, x, eta_t, M, (D, M, n) in ZERO_Y)

    n_rand = max(1, int(round(RANDOM_SHARE * n)))
    n_edge = n - n_rand
    mags = (1.0, min(1.0, kw['prior_scale']), 5.0, 0.01)
    beta = np.empty((n, D))
    for r in range(n_edge):
        beta[r] = rs.randn(D) * 0.8 * comp * mags[r % 4]
    beta[n_edge:] = rs.randn(n_rand, D) * 0.8 * comp
    info = dict(cols=cols, zero_obs=zero_obs, n_edge=n_edge, slots=[])
    if n_edge >= 1:
        beta[0] = 0.0
    free = np.nonzero((offset == 0.0) & (np.arange(M) != zero_obs))[0]
    targets = eta_targets(lik, kw)
    if 'big' in cols:
        # beside the 1e3 column the gradient's S = e^eta a_m |x_md| would pass 1.8e308
        targets = [690.0 if v == 700.0 else v for v in targets]
    targets = targets[i % len(targets):] + targets[:i % len(targets)]
    row = 2
    for v in targets:
        if row >= n_edge or free.size == 0:
            break
        for _ in range(400):
            u = rs.randn(D) * comp
            q = (x @ u) * math.copysign(1.0, v)
            m = int(free[np.argmax(q[free])])
            if not q[m] > 0.0:
                continue
            b = u * (v / (x[m] @ u))
            eta = x @ b + offset
            if abs(eta[m] - v) > 1e-3 * abs(v):
                continue
            if lik == 'poisson_log' and eta.max() > (POIS_CAP if 'big' not in cols else 695.0):
                continue
            beta[row] = b
            info['slots'].append((row, m, v))
            row += 1
            break

    rows = np.arange(n)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(beta))
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = cc.restatement(x, y, offset=offset, **kw)(beta)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), (lik, D, M, n)
    for arr in (x, y, offset, beta, rows):
        arr.setflags(write=False)
    return Case(x, y, offset, kw, beta, rows, info)


@functools.lru_cache(maxsize=None)
def edge_reference(lik, D, M, n):
    """(Case, Ref at case.beta) of one case, computed once per process and shared."""
    c = edge_case(lik, D, M, n)
    ref = reference(c.x, c.y, c.beta[c.rows], offset=c.offset, **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


# ---- the multilevel cases -----------------------------------------------------------
U_CENTRES = mm.U_CENTRES           # (-40, -8, -2, 0, 1.6, 4, 20)
BLOCK_ROWS = 3
MLM_FAR = {'poisson_log': 680.0, 'neg_binomial_2_log': 800.0}


def _mlm_eta(x, group, offset, zr, p, centered):
    tau = np.exp(zr[p])
    a = zr[p + 1:]
    return x @ zr[:p] + (a if centered else tau * a)[group] + offset


@functools.lru_cache(maxsize=None)
def mlm_edge_case(lik, centered, p, G, M):
    """The seeded data and edge rows of one multilevel case: the data of
    count_cases.mlm_make_data (group sizes of tests/mlm_cases.py: one large group, a
    singleton, an empty one as far as G has room) with Y_EDGE, OFFSET_EDGE and the
    all-zero responses of ZERO_Y as in edge_case; the rows of tests/mlm_mp.py's edge_case,
    a block of BLOCK_ROWS rows per log tau centre (and for the centred form a second block
    with a = tau randn), the last row of each a far row: beta and the intercepts scaled
    together so that the largest eta - eta0 is MLM_FAR (680 for the Poisson: the offsets reach 12, and the
    gradient's S = e^eta a_m |x_md| must stay below 1.8e308; the sign
    chosen so that it is the largest, 800 in absolute value for the negative binomial).
    The non-centred Poisson leaves out the centre log tau = 20, where tau at_g ~ 5e8 is
    past exp's range in every row."""
    i = MLM_SHAPES.index((p, G, M))
    li = cc.LIKELIHOODS.index(lik)
    kw = cc.mlm_model_kwargs(lik, centered, phi=PHIS[(i + li) % 3],
                             prior_scale=PRIOR_SCALES[(i + 1 + li) % 3])
    x, _, group, _ = cc.mlm_make_data(p, G, M, lik, seed=40 + i)
    rs = np.random.RandomState(SEED + 1000 * i + 10 * li + int(centered))
    eta_t = x @ (0.5 * rs.randn(p) / math.sqrt(p)) + (0.5 * rs.randn(G))[group]
    y, offset = _edge_data(rs, lik, kw, x, eta_t, M, (p, G, M) in ZERO_Y)
    D = p + 1 + G
    k = BLOCK_ROWS
    centres = [u for u in U_CENTRES if not (lik == 'poisson_log' and not centered and u > 10)]
    blocks = []
    for uc in centres:
        for own in ((False, True) if centered else (False,)):
            blk = rs.randn(k, D)
            blk[:, p] = tm._jit(rs, uc, k)
            blk[0, p] = uc
            tau = np.exp(blk[:, p:p + 1])
            if own:              # (Poisson: intercepts within exp's range, ~ +-80 at most)
                blk[:, p + 1:] *= np.minimum(tau, 20.0) if lik == 'poisson_log' else tau
            elif not centered and lik == 'poisson_log':
                blk[:, p + 1:] *= np.minimum(1.0, 20.0 / tau)
            far = blk[k - 1]
            d = _mlm_eta(x, group, 0.0, far, p, centered)
            top = float(np.max(np.abs(d)))
            if top > 0.0:
                f = MLM_FAR[lik] / top
                if lik == 'poisson_log' and np.max(d) < top:
                    f = -f
                far[:p] *= f
                far[p + 1:] *= f
            blocks.append(blk)
    z = np.concatenate(blocks)
    n_rand = max(1, int(round(RANDOM_SHARE * z.shape[0] / (1.0 - RANDOM_SHARE))))
    zr = rs.randn(n_rand, D)
    z = np.concatenate([z, zr])
    assert np.all(np.isfinite(z))
    if lik == 'poisson_log':
        top = max(float(np.max(_mlm_eta(x, group, offset, r, p, centered))) for r in z)
        assert top < 709.0, (lik, centered, p, G, M, top)
    for arr in (x, y, group, offset, z):
        arr.setflags(write=False)
    return MlmCase(x, y, group, offset, kw, z)


@functools.lru_cache(maxsize=None)
def mlm_edge_reference(lik, centered, p, G, M):
    c = mlm_edge_case(lik, centered, p, G, M)
    ref = mlm_reference(c.x, c.y, c.group, c.z, offset=c.offset, n_groups=G, **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


# Worst error of the numpy restatement (tests/count_cases.py) over cases() / mlm_cases()
# per target and likelihood, value and gradient entries together, and of the packer's
# c_data (targets.count_constant) over the same cases, in units of 2^-53 S; measured by
# tests/test_oracle_count_mp.py, which asserts twice these figures.  The GPU tests allow
# the kernels 8 times them.
COUNT_ORACLE_ERR = {
    # gradient column 14 at (D, M, n) = (16, 130, 70), row 26; the worst value is 2.24 at
    # (17, 15, 15)
    ('regression', 'poisson_log'): 2.42,
    # gradient column 7 at (130, 321, 10), row 2 (phi = 1e6): the order of the matrix
    # product's sum over m; the next is 7.43 at (16, 130, 70); the worst value is 3.97 at
    # (4, 64, 63)
    ('regression', 'neg_binomial_2_log'): 17.55,
    # centred, d a_2 (column 11) at (p, G, M) = (17, 3, 65), row 40; value 2.72
    ('multilevel', 'poisson_log'): 8.14,
    # centred, d beta_0 at (16, 70, 321), row 23; value 3.17
    ('multilevel', 'neg_binomial_2_log'): 13.63,
    # the packer's c_data against S_c over the same cases
    ('c_data', 'poisson_log'): 1.04,
    ('c_data', 'neg_binomial_2_log'): 0.74,
}
