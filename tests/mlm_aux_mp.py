"""Multiprecision restatement (mpmath, 50 digits) of the multilevel regression target with a
learned scale or dispersion, its condition sums, and the edge data and rows; shared by the
CPU test that pins the numpy restatement of tests/mlm_aux_cases.py
(tests/test_oracle_mlm_aux_mp.py) and the GPU test of the learned instances of vb_mlm.hip
(tests/test_gpu_mlm_aux_edges.py).

Written from the densities literally: the observations and the prior of theta = e^lambda are
tests/aux_mp.py's _row_density (the literal gaussian, student_t and negative binomial
densities and log(2 / (pi s_aux (1 + (theta / s_aux)^2))) + lambda), the lambda gradient is
mp.diff of it at aux_mp.row_digits(lambda) digits; the priors of beta, tau and the groups
are those of tests/mlm_mp.py; every x_m . beta is an exact integer dot product.

Error metric: that of tests/targets_mp.py, err = |got - ref| / (2^-53 S).  S is built as
tests/mlm_mp.py and tests/aux_mp.py build theirs.  The inner sum of an observation is
A_m = sum_d |x_md beta_d| + |a_eff| + |y_m| (gaussian, student_t) or + |eta0_m| + |lambda|
(negative binomial, zeta = eta - lambda), a_eff = a_g or tau at_g; with T(l), T(l'), |l''|,
T(v), |dv/deta| of aux_mp._obs_terms at sigma = e^lambda / phi = e^lambda and
R_m = T(l'_m) + |l''_m| A_m:

  S_lp     = mlm_mp's S_lp (c_obs without -log sigma) + |log(2 / (pi s_aux))| + softplus(w)
             + |lambda| + M |lambda|                          (gaussian, student_t)
             or + sum_m loggamma(y_m + 1) + A(phi)             (negative binomial)
  S_beta_d, S_a_g, S_at_g, S_u: mlm_mp's, over these R_m
  S_lambda = 1 + 2 logistic(w) + M + sum_m [T(v_m) + |dv_m/deta| A_m]   (gaussian, student_t)
             1 + 2 logistic(w) + sum_m [T(v_m) + |dv_m/dzeta| A_m] + |dA/dlambda|  (neg. binomial)
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import aux_cases as ac
from tests import aux_mp as am
from tests import count_cases as cc
from tests import glm_mp as gm
from tests import mlm_aux_cases as mac
from tests import mlm_cases as mc
from tests import mlm_mp as mm
from tests.targets_mp import DIGITS, RANDOM_SHARE, UNIT, Ref, available, errors  # noqa: F401

try:
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mp = mpf = None


def reference(x, y, group, z, likelihood='gaussian', df=None, offset=None, prior_scale=10.0,
              tau_scale=5.0, centered=False, n_groups=None, hyper_scale=5.0):
    """Ref of the learned model at the rows of z [n][p + 2 + G]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    group = np.asarray(group).astype(np.int64)
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    (M, p), n = x.shape, z.shape[0]
    G = int(group.max()) + 1 if n_groups is None else int(n_groups)
    D = p + 2 + G
    assert z.shape[1] == D
    nb = likelihood == 'neg_binomial_2_log'
    eta0 = np.zeros(M) if offset is None else np.asarray(offset, dtype=np.float64)
    members = [np.nonzero(group == g)[0] for g in range(G)]
    ix, ex = gm._ints(x)
    ib, eb = gm._ints(z[:, :p])
    xb_i = np.dot(ib, ix.T)                                   # exact, [n][M]
    xb_abs = np.abs(z[:, :p]) @ np.abs(x).T
    vals, counts = np.unique(y, return_counts=True)
    T, _ = ac.dispersion_table(y) if nb else (np.zeros(0), 0.0)
    js = np.arange(T.size, dtype=float)
    out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
    for r in range(n):
        lam64 = float(z[r, D - 1])
        with mp.workdps(am.row_digits(lam64)):
            s, st, s_aux = (mpf(float(v)) for v in (prior_scale, tau_scale, hyper_scale))
            nu = mpf(float(df)) if likelihood == 'student_t' else None
            half_l2pi = mp.log(2 * mp.pi) / 2
            c_prior = half_l2pi + mp.log(s)
            c_tau = mp.log(2 / (mp.pi * st))
            lam = mpf(lam64)
            theta = mp.exp(lam)
            Y = [mpf(v) for v in y.tolist()]
            ycount = [(mpf(v), c) for v, c in zip(vals.tolist(), counts.tolist())]
            B = [mpf(v) for v in z[r, :p].tolist()]
            u = mpf(float(z[r, p]))
            a = [mpf(v) for v in z[r, p + 1:p + 1 + G].tolist()]
            tau = mp.exp(u)
            w = (tau / st) ** 2
            aeff = a if centered else [tau * v for v in a]
            etas = [mp.ldexp(mpf(int(xb_i[r, m])), ex + eb) + aeff[group[m]] + mpf(float(eta0[m]))
                    for m in range(M)]

            def dens(L):
                return am._row_density(likelihood, L, etas, Y, ycount, nu, s_aux)
            ss = mp.fsum(B, squared=True) / (2 * s * s)
            l1 = mp.log1p(w)
            lp = dens(lam) - ss - p * c_prior + c_tau - l1 + u - G * half_l2pi
            gl = mp.diff(dens, lam)
            # the observations' derivatives and condition terms
            A = xb_abs[r] + np.array([float(abs(aeff[g])) for g in group])
            A = A + (np.abs(eta0) + abs(lam64) if nb else np.abs(y))
            dls = []
            t_l, t_g, d2, t_v, dv, adl = (np.empty(M) for _ in range(6))
            for m in range(M):
                dl, t_l[m], t_g[m], d2[m], t_v[m], dv[m] = am._obs_terms(likelihood, etas[m], Y[m],
                                                                        theta, nu)
                dls.append(dl)
                adl[m] = abs(float(dl))
            with np.errstate(over='ignore', invalid='ignore'):
                R = t_g + np.where(A > 0, d2 * A, 0.0)
            wl = 2 * (lam - mp.log(s_aux))
            sp_w = float(mp.log(1 + mp.exp(wl)))
            lg_w = float(1 / (1 + mp.exp(-wl)))
            s_lp = (float(ss) + float(p * abs(c_prior)) + float(abs(c_tau)) + float(l1)
                    + float(abs(u)) + G * float(half_l2pi)
                    + float(abs(mp.log(2 / (mp.pi * s_aux)))) + sp_w + abs(lam64)
                    + float(np.sum(t_l + adl * A)))
            s_gl = 1.0 + 2.0 * lg_w + float(np.sum(t_v + dv * A))
            if nb:
                ph = float(theta)
                with np.errstate(over='ignore'):
                    At = float(np.sum(T[1:] * np.log1p(js[1:] / ph))) if T.size > 1 else 0.0
                    dA = float(np.sum(T[1:] * (js[1:] / (ph + js[1:])))) if T.size > 1 else 0.0
                s_lp += float(sum(c * mp.loggamma(v + 1) for v, c in ycount)) + At
                s_gl += dA
            else:
                if likelihood == 'gaussian':
                    c_obs = half_l2pi
                else:
                    c_obs = abs(mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2)
                                - mp.log(nu * mp.pi) / 2)
                s_lp += M * float(c_obs) + M * abs(lam64)
                s_gl += M
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
            out.g_hi[r, D - 1], out.g_lo[r, D - 1] = gm._split(gl)
            out.g_S[r, D - 1] = s_gl
            with mp.workdps(DIGITS + 30):
                il, el = gm._mp_ints([+v for v in dls])
            gi = np.dot(il, ix)                               # exact, [p]
            for d in range(p):
                gb = mp.ldexp(mpf(int(gi[d])), el + ex) - B[d] / (s * s)
                out.g_hi[r, d], out.g_lo[r, d] = gm._split(gb)
            out.g_S[r, :p] = np.abs(z[r, :p]) / float(prior_scale) ** 2 + R @ np.abs(x)
    return out


# ---- shapes, scales and rows -----------------------------------------------------------
SHAPES = mm.SHAPES                 # each PP instance, the tile kernel, split and empty groups
U_CENTRES = (-8.0, 0.0, 4.0)
U_WIDE = (-40.0, 40.0)
LAMS = am.LAMS
TAIL = am.TAIL                     # |lambda - log s_aux| and |u| of the rows of far_rows
RESID_FAR = mm.RESID_FAR
ZETAS = am.ZETAS
DFS = am.DFS
PRIOR_SCALES = am.PRIOR_SCALES
HYPER_SCALES = am.HYPER_SCALES
TAU_SCALES = (1e-3, 2.0, 1e3)
SHAPE_TABLE = (3, 8, 129)
TABLE_KINDS = am.TABLE_KINDS
Y_BIG = am.Y_BIG
SEED = 20250301

Case = namedtuple('Case', 'x y group offset kw z')


def cases():
    """Every (likelihood, centred, p, G, M) of the edge tests."""
    return [(lik, c, p, G, M) for (p, G, M) in SHAPES for c in mac.FORMS for lik in mac.LIKELIHOODS]


def table_cases():
    return [('neg_binomial_2_log', False) + SHAPE_TABLE + (kind,) for kind in TABLE_KINDS]


def case_kwargs(lik, centered, i):
    li = mac.LIKELIHOODS.index(lik)
    return mac.model_kwargs(lik, centered, df=DFS[i % 3],
                            prior_scale=PRIOR_SCALES[(i + i // 3 + li) % 3],
                            tau_scale=TAU_SCALES[(i + li + int(centered)) % 3],
                            hyper_scale=HYPER_SCALES[(i + li) % 3])


def _data(lik, p, G, M, i, kind):
    if lik != 'neg_binomial_2_log':
        return mc.make_data(p, G, M, lik, seed=40 + i) + (None,)
    x, y, group, offset = cc.mlm_make_data(p, G, M, lik, seed=40 + i)
    offset = np.where(np.arange(M) % 5 < 2, 0.0, offset)      # 40 % of the offsets exactly 0
    if kind == 'zero':
        y = np.zeros(M)
    elif kind == 'binary':
        y = np.minimum(y, 1.0)
        y[0] = 1.0
    elif kind == 'big':
        y = np.minimum(y, 9.0)
        y[M // 2] = Y_BIG
    return x, y, group, offset


def _eta(x, group, zr, p, G, centered, offset):
    a = zr[p + 1:p + 1 + G]
    eta = x @ zr[:p] + (a if centered else np.exp(zr[p]) * a)[group]
    return eta if offset is None else eta + offset


@functools.lru_cache(maxsize=None)
def edge_case(lik, centered, p, G, M, kind=None):
    """The seeded data and edge rows of one case (n <= 40).  Rows: U_CENTRES x the three
    lambda centres of LAMS, the other coordinates standard normal (centred form: a = tau
    randn, the prior's own region); one row each at u = -40, +40 with the intercept of
    order one at +40 (a_eff ~ randn) and, in the centred form, a = tau randn at -40; the
    far rows: gaussian, student_t one row per lambda centre
    with beta and the intercepts scaled together so that max |y - eta| ~ RESID_FAR;
    negative binomial one row per ZETAS with beta = 0 and every intercept at lambda + zeta,
    so the observations whose offset is 0 sit at eta - lambda = zeta; then RANDOM_SHARE
    standard-normal rows."""
    i = SHAPES.index((p, G, M))
    li = mac.LIKELIHOODS.index(lik)
    nb = lik == 'neg_binomial_2_log'
    x, y, group, offset = _data(lik, p, G, M, i, kind)
    kw = case_kwargs(lik, centered, i)
    rs = np.random.RandomState(SEED + 1000 * i + 10 * li + int(centered)
                               + 7 * (TABLE_KINDS.index(kind) + 1 if kind else 0))
    lams = LAMS['phi' if nb else 'scale']
    D = p + 2 + G
    rows = []

    def row(u, lam, own=centered):
        zr = rs.randn(D)
        zr[p], zr[D - 1] = u, lam
        if own:
            zr[p + 1:p + 1 + G] *= math.exp(u)
        return zr

    for uc in U_CENTRES:
        for lam in lams:
            rows.append(row(uc, lam))
    for k, uw in enumerate(U_WIDE):
        zr = row(uw, lams[(i + k) % 3], own=centered and uw < 0)
        if not centered:
            zr[p + 1:p + 1 + G] *= math.exp(-uw)          # a_eff = tau at ~ randn
        rows.append(zr)
    if nb:
        for k, v in enumerate(ZETAS):
            lam = lams[(i + k) % 3]
            zr = row(0.0, lam, own=False)
            zr[:p] = 0.0
            zr[p + 1:p + 1 + G] = lam + v
            rows.append(zr)
    else:
        for k, lam in enumerate(lams):
            zr = row(U_CENTRES[(i + k) % 3], lam)
            top = float(np.max(np.abs(_eta(x, group, zr, p, G, centered, None))))
            f = RESID_FAR / top
            zr[:p] *= f
            zr[p + 1:p + 1 + G] *= f
            rows.append(zr)
    z = np.array(rows)
    n_rand = max(1, int(round(RANDOM_SHARE * z.shape[0] / (1.0 - RANDOM_SHARE))))
    zr = rs.randn(n_rand, D)
    zr[:, D - 1] = math.log(3.0 if nb else 0.7) + 0.5 * zr[:, D - 1]
    z = np.concatenate([z, zr])
    assert np.all(np.isfinite(z)) and z.shape[0] <= 40
    for arr in (x, y, group, z) + (() if offset is None else (offset,)):
        arr.setflags(write=False)
    return Case(x, y, group, offset, kw, z)


@functools.lru_cache(maxsize=None)
def edge_reference(lik, centered, p, G, M, kind=None):
    """(Case, Ref at case.z) of one case, computed once per process and shared."""
    c = edge_case(lik, centered, p, G, M, kind)
    ref = reference(c.x, c.y, c.group, c.z, offset=c.offset, n_groups=G, **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


def far_rows(c, p, G, seed=0):
    """Four rows past the double range of sigma^2, phi, tau^2: lambda - log s_aux = -400,
    +400 and u = -400, +400, the other coordinates standard normal."""
    D = p + 2 + G
    z = np.random.RandomState(SEED + seed).randn(4, D)
    ls = math.log(c.kw['hyper_scale'])
    z[0, D - 1], z[1, D - 1] = ls - TAIL, ls + TAIL
    z[2, p], z[3, p] = -TAIL, TAIL
    return z


# Worst error of the numpy restatement (tests/mlm_aux_cases.py) over cases() and
# table_cases() per form, value and gradient entries together, in units of 2^-53 S;
# measured by tests/test_oracle_mlm_aux_mp.py, which asserts twice these figures.  The GPU
# test allows the kernels 8 times them.  Keyed by `centered`.
MLM_AUX_ORACLE_ERR = {
    # non-centred: value at (p, G, M) = (16, 70, 321), student_t, row 11 (the far row at
    # u = -8, lambda = log 1e-3)
    False: 3.89,
    # centred: value at (2, 1, 40), gaussian, row 4 (u = 0, lambda = log 0.7)
    True: 5.65,
}
