"""Multiprecision restatement of the regression targets (mpmath, 50 digits), their
condition sums, and the edge data and rows; shared by the CPU test that pins the
numpy restatement (tests/test_oracle_glm_mp.py) and the GPU tests of vb_glm.hip
(tests/test_gpu_glm_edges.py).

Written from the definitions in the docstring of tests/glm_cases.py, every constant
kept (s the prior scale, eta_m = x_m . beta, r_m = y_m - eta_m):

  log p(beta) = sum_d [-beta_d^2 / (2 s^2) - log(2 pi)/2 - log s] + M c_obs + sum_m l_m
  gaussian         l = -r^2 / (2 sigma^2),              c_obs = -log(2 pi)/2 - log sigma
  student_t        l = -(nu+1)/2 log1p(r^2 / (nu sigma^2)),
                   c_obs = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2 - log sigma
  bernoulli_logit  l = y eta - max(eta, 0) - log1p(exp(-|eta|)),   c_obs = 0
  d log p / d beta_d = -beta_d / s^2 + sum_m l'_m x_md,  l' = dl / d eta:
  gaussian l' = r / sigma^2, student_t l' = (nu+1) r / (nu sigma^2 + r^2),
  bernoulli_logit l' = y - p, p = 1 / (1 + exp(-eta))

Error metric: that of tests/targets_mp.py, err = |got - ref| / (2^-53 S), S the
condition sum of the result.  A term here contains a cancelling sum (eta = x . beta
and the residual y - eta), which a sum of the terms' absolute values alone would not
see (the note on targets_mp.ORACLE_ERR['eight_schools_ncp']); S carries it through
the term's derivative.  Per observation a_m = sum_d |x_md beta_d| (+ |y_m| for
gaussian and student_t), l' and l'' the derivatives of l in eta:

  S_lp  = sum_d beta_d^2 / (2 s^2) + D |log(2 pi)/2 + log s| + M |c_obs|
          + sum_m [T(l_m) + |l'_m| a_m]
  S_g_d = |beta_d| / s^2 + sum_m [T(l'_m) + |l''_m| a_m] |x_md|

T the sum of the absolute values of the terms that are added:

  gaussian         T(l) = r^2 / (2 sigma^2)                    T(l') = |r| / sigma^2
  student_t        T(l) = (nu+1)/2 log1p(r^2 / (nu sigma^2))   T(l') = |l'|
  bernoulli_logit  T(l) = |y eta| + max(eta, 0) + log1p(exp(-|eta|))      T(l') = y + p

  |l''|: gaussian 1 / sigma^2, student_t (nu+1) |nu sigma^2 - r^2| / (nu sigma^2 + r^2)^2,
  bernoulli_logit p (1 - p)

S_g_d is 0 only where beta_d = 0 meets an all-zero column of X; there the gradient is
exactly 0 and errors() asks for exactly 0.

How it is evaluated.  x, y and beta are doubles, so every eta is an exact dot product:
the doubles are scaled to integers and the products summed in Python integers (what
mp.fdot does, at the speed of an object-array matmul), each eta formed once per (row,
observation) and rounded once to 50 digits.  The link and its derivative are evaluated
in mpmath; the gradient's sum over m is again an exact integer dot product of the
50-digit l' with x.  S is a sum of non-negative terms and only a scale: it is summed in
float64 from the multiprecision per-observation terms.  References come back as a
double pair (hi, lo) in the Ref tuple of targets_mp.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import glm_cases as gc
from tests.targets_mp import DIGITS, RANDOM_SHARE, UNIT, Ref, available, errors  # noqa: F401

try:
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mp = mpf = None


# ---- exact integer forms -------------------------------------------------------
def _ints(a):
    """(object array of Python ints I, e) with a = I 2^e exactly."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mant = np.ldexp(m, 53).astype(np.int64)
    e = e.astype(np.int64) - 53
    nz = mant != 0
    e0 = int(e[nz].min()) if nz.any() else 0
    vals = [int(mm) << (int(ee) - e0) if mm else 0
            for mm, ee in zip(mant.ravel().tolist(), e.ravel().tolist())]
    out = np.empty(len(vals), dtype=object)
    out[:] = vals
    return out.reshape(a.shape), e0


def _mp_ints(v):
    """The same for a list of mpf."""
    parts = [t._mpf_ for t in v]
    exps = [p[2] for p in parts if p[1]]
    e0 = min(exps) if exps else 0
    out = np.empty(len(parts), dtype=object)
    out[:] = [(-(p[1] << (p[2] - e0)) if p[0] else p[1] << (p[2] - e0)) if p[1] else 0
              for p in parts]
    return out, e0


def _split(v):
    hi = float(v)
    return hi, float(v - mpf(hi))


# ---- the links ------------------------------------------------------------------
def _link(lik, eta, y, nu, sig):
    """(l, l', T(l), T(l'), |l''|) of one observation; the last three as floats."""
    if lik == 'gaussian':
        r = y - eta
        q = r * r / (2 * sig * sig)
        return -q, r / (sig * sig), float(q), float(abs(r) / (sig * sig)), float(1 / (sig * sig))
    if lik == 'student_t':
        r = y - eta
        r2, k3 = r * r, nu * sig * sig
        l = -(nu + 1) / 2 * mp.log1p(r2 / k3)
        dl = (nu + 1) * r / (k3 + r2)
        d2 = (nu + 1) * abs(k3 - r2) / (k3 + r2) ** 2
        return l, dl, float(-l), float(abs(dl)), float(d2)
    e = mp.exp(-abs(eta))
    l1 = mp.log1p(e)
    pos = eta if eta > 0 else mpf(0)
    p = 1 / (1 + e) if eta >= 0 else e / (1 + e)
    return (y * eta - pos - l1, y - p, float(abs(y * eta) + pos + l1), float(y + p),
            float(e / (1 + e) ** 2))


def reference(x, y, beta, likelihood='student_t', df=None, scale=1.0, prior_scale=10.0):
    """Ref of the model (x [M][D], y [M], ...) at the rows of beta [n][D]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    (M, D), n = x.shape, beta.shape[0]
    with mp.workdps(DIGITS):
        s = mpf(float(prior_scale))
        sig = mpf(float(scale)) if likelihood != 'bernoulli_logit' else None
        nu = mpf(float(df)) if likelihood == 'student_t' else None
        half_l2pi = mp.log(2 * mp.pi) / 2
        c_prior = half_l2pi + mp.log(s)
        if likelihood == 'gaussian':
            c_obs = -half_l2pi - mp.log(sig)
        elif likelihood == 'student_t':
            c_obs = (mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2
                     - mp.log(sig))
        else:
            c_obs = mpf(0)
        c_all = -D * c_prior + M * c_obs
        s_const = float(D * abs(c_prior) + M * abs(c_obs))
        Y = [mpf(v) for v in y.tolist()]
        ix, ex = _ints(x)
        ib, eb = _ints(beta)
        eta_i = np.dot(ib, ix.T)                              # exact, [n][M]
        a = np.abs(beta) @ np.abs(x).T
        if likelihood != 'bernoulli_logit':
            a = a + np.abs(y)[None, :]
        out = Ref(*(np.empty(n) for _ in range(3)), *(np.empty((n, D)) for _ in range(3)))
        t_l, t_g, d2 = np.empty(M), np.empty(M), np.empty(M)
        adl = np.empty(M)
        for r in range(n):
            ls, dls = [], []
            for m in range(M):
                eta = mp.ldexp(mpf(eta_i[r, m]), ex + eb)
                l, dl, t_l[m], t_g[m], d2[m] = _link(likelihood, eta, Y[m], nu, sig)
                ls.append(l)
                dls.append(dl)
                adl[m] = abs(float(dl))
            B = [mpf(v) for v in beta[r].tolist()]
            ss = mp.fsum(B, squared=True) / (2 * s * s)
            out.lp_hi[r], out.lp_lo[r] = _split(c_all - ss + mp.fsum(ls))
            out.lp_S[r] = float(ss) + s_const + float(np.sum(t_l + adl * a[r]))
            il, el = _mp_ints(dls)
            gi = np.dot(il, ix)                               # exact, [D]
            for d in range(D):
                g = mp.ldexp(mpf(gi[d]), el + ex) - B[d] / (s * s)
                out.g_hi[r, d], out.g_lo[r, d] = _split(g)
            out.g_S[r] = np.abs(beta[r]) / float(prior_scale) ** 2 + (t_g + d2 * a[r]) @ np.abs(x)
    return out


# ---- the shapes: the smallest that reach each path of vb_glm.hip ----------------------
# lane-per-row kernel, D <= 16: DP = 2, 4, 8, 16 and both sides of each; M around the
# 64-observation tile; n around one 64-lane block
SHAPES_SMALL = ((1, 1, 1), (2, 65, 65), (4, 64, 63), (5, 63, 64), (8, 129, 10), (9, 65, 10),
                (16, 130, 70))
# the 256-thread launch of the lane-per-row kernel (n > 4096); student_t only, the
# reference on SAMPLE_ROWS rows
SHAPE_256 = (2, 25, 4097)
SAMPLE_ROWS = 64
# matrix kernel: the D boundaries 32 / 33 (one LDS slice becomes two, NCT 2 -> 4),
# 64 / 65 (NCT 4 -> 8), 128 / 129 (a second column slab), three slabs at 257
SHAPES_MFMA = ((17, 15, 15), (32, 16, 16), (33, 17, 17), (64, 65, 16), (65, 65, 17),
               (96, 129, 10), (128, 70, 16), (129, 70, 17), (130, 129, 10), (257, 70, 8))
# six observation chunks, the last of one observation
SHAPES_CHUNK = ((40, 321, 10), (130, 321, 10))
# value only (GRAD = false): both kernels, one and several LDS slices
SHAPES_VALUE = ((3, 65, 64), (20, 65, 17), (40, 321, 10), (130, 321, 10))
ALL_SHAPES = tuple(dict.fromkeys(SHAPES_SMALL + (SHAPE_256,) + SHAPES_MFMA + SHAPES_CHUNK
                                 + SHAPES_VALUE))

PRIOR_SCALES = (1e-3, 3.0, 1e3)
SCALES = (1e-3, 0.7, 1e3)
DFS = (0.5, 5.0, 1e6)
# |eta| of the logistic rows: beside 0; where 1 + e^-|eta| rounds to 1; exp(-709) is
# subnormal and exp(-746) underflows to 0; the saturated rows of test_gpu_glm.py.
# eta = 0 exactly comes from the beta = 0 row and the all-zero observation
BERN_ETAS = (1e-9, 36.8, 709.0, 746.0, 800.0)
# shapes whose bernoulli responses are all 0 / all 1
BERN_Y = {(3, 65, 64): 0.0, (20, 65, 17): 1.0}
SEED = 20240611

Case = namedtuple('Case', 'x y kw beta rows info')


def cases():
    """Every (likelihood, D, M, n) of the edge tests."""
    out = [(lik, D, M, n) for D, M, n in ALL_SHAPES if (D, M, n) != SHAPE_256
           for lik in gc.LIKELIHOODS]
    return out + [('student_t',) + SHAPE_256]


def case_kwargs(lik, D, M, n):
    """The model's constants: the nine (df, scale) pairs and the three prior scales
    cycle over the shapes, shifted per likelihood."""
    i, li = ALL_SHAPES.index((D, M, n)), gc.LIKELIHOODS.index(lik)
    return gc.model_kwargs(lik, df=DFS[i % 3], scale=SCALES[(i // 3 + li) % 3],
                           prior_scale=PRIOR_SCALES[(i + i // 3 + li) % 3])


def special_columns(D):
    """Columns of X with a role, as far as D has room: the gradient column orthogonal
    to one row's residuals is the last one, the all-zero column 1, the columns scaled
    by 1e-6 and 1e3 are 2 and 3."""
    cols = {}
    if D >= 2:
        cols['ortho'] = D - 1
    if D >= 3:
        cols['zero'] = 1
    if D >= 4:
        cols['small'] = 2
    if D >= 5:
        cols['big'] = 3
    return cols


def _dl64(lik, kw, eta, y):
    if lik == 'gaussian':
        return (y - eta) / kw['scale'] ** 2
    if lik == 'student_t':
        r = y - eta
        return (kw['df'] + 1) * r / (kw['df'] * kw['scale'] ** 2 + r * r)
    e = np.exp(-np.abs(eta))
    return y - np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


@functools.lru_cache(maxsize=None)
def edge_case(lik, D, M, n):
    """The seeded edge data and rows of one case.

    Data: column roles as special_columns; observation 1 all zero (M >= 3).  gaussian
    and student_t: y_1 = 0 (a residual of exactly 0 at every row) and, at the anchor
    row 2, residuals of +-1e-9 (observations 2, 3), of +-1e-12 |y| (4, 5) and, for
    student_t, of +-1e6 (6, 7).  bernoulli_logit: mixed responses, or all 0 / all 1
    at the shapes of BERN_Y.
    Rows: 0 is beta = 0; 1 has beta = 0 in the last column, whose data are then made
    orthogonal to that row's l' to 1e-12 of the norms; bernoulli_logit rows from 2 on
    put chosen observations at +-BERN_ETAS, each value once with y = 0 and once with
    y = 1 (min-norm beta over the plain columns, as test_logistic_saturated_rows_stay_
    finite builds +-800); the other edge rows are 0.8 randn scaled by 1, min(1, s), 5,
    0.01 in turn (the 1e3 column's coefficient by 1e-3); the last RANDOM_SHARE of the
    rows are the 0.8 randn points of test_gpu_glm.py."""
    i, li = ALL_SHAPES.index((D, M, n)), gc.LIKELIHOODS.index(lik)
    rs = np.random.RandomState(SEED + 100 * i + li)
    kw = case_kwargs(lik, D, M, n)
    cols = special_columns(D)
    plain = [d for d in range(D) if d not in cols.values()]
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
    eta_t = x @ (rs.randn(D) / math.sqrt(D) * comp)
    if lik == 'gaussian':
        y = eta_t + kw['scale'] * rs.randn(M)
    elif lik == 'student_t':
        y = eta_t + kw['scale'] * rs.standard_t(max(kw['df'], 2.0), M)
    else:
        y = (rs.rand(M) < 1.0 / (1.0 + np.exp(-eta_t))).astype(float)
        if (D, M, n) in BERN_Y:
            y[:] = BERN_Y[(D, M, n)]
        elif M >= 4:
            y[2], y[3] = 0.0, 1.0

    n_rand = max(1, int(round(RANDOM_SHARE * n)))
    n_edge = n - n_rand
    mags = (1.0, min(1.0, kw['prior_scale']), 5.0, 0.01)
    beta = np.empty((n, D))
    for r in range(n_edge):
        beta[r] = rs.randn(D) * 0.8 * comp * mags[r % 4]
    beta[n_edge:] = rs.randn(n_rand, D) * 0.8
    info = dict(cols=cols, zero_obs=zero_obs, n_edge=n_edge, slots=[], resid={})
    if n_edge >= 1:
        beta[0] = 0.0
    ortho = cols.get('ortho') if (n_edge >= 2 and M >= 4) else None
    if ortho is not None:
        beta[1] = rs.randn(D) * 0.8 * comp
        beta[1, ortho] = 0.0

    if lik != 'bernoulli_logit':
        if zero_obs is not None:
            y[zero_obs] = 0.0
        if n_edge >= 3:
            if ortho is not None:
                beta[2, ortho] = 0.0
            eta_a = x @ beta[2]
            feats = [(2, 'abs', 1e-9), (3, 'abs', -1e-9), (4, 'rel', 1e-12), (5, 'rel', -1e-12)]
            if lik == 'student_t':
                feats += [(6, 'abs', 1e6), (7, 'abs', -1e6)]
            for m, kind, v in feats:
                if m < M:
                    y[m] = eta_a[m] + v if kind == 'abs' else eta_a[m] * (1.0 + v)
                    info['resid'][m] = (kind, v)
    elif plain:
        # rows that put observations at chosen eta; the group beside 0 apart from the rest
        k = min(len(plain), 8)
        row = 2
        for group in (BERN_ETAS[:1], BERN_ETAS[1:]):
            slots = [(sg * v, yv) for v in group for sg in (1.0, -1.0) for yv in (0.0, 1.0)]
            for c0 in range(0, len(slots), k):
                if row >= n_edge:
                    break
                obs, vals = [], []
                for v, yv in slots[c0:c0 + k]:
                    free = [m for m in range(M) if m != zero_obs and y[m] == yv and m not in obs]
                    if free:
                        obs.append(free[(row * 7) % len(free)])
                        vals.append(v)
                if not obs:
                    continue
                xt = x[np.ix_(obs, plain)]
                beta[row] = 0.0
                if 'zero' in cols:               # free: it does not move any eta
                    beta[row, cols['zero']] = 0.8 * rs.randn()
                beta[row, plain] = np.linalg.lstsq(xt, np.array(vals), rcond=None)[0]
                got = x[obs] @ beta[row]
                assert np.all(np.abs(got - vals) <= 1e-3 * np.abs(vals)), (lik, D, M, n, got, vals)
                info['slots'] += [(row, m, v, float(y[m])) for m, v in zip(obs, vals)]
                row += 1

    if ortho is not None:
        # the last column against l' of row 1, which does not depend on it (beta = 0 there)
        dl = _dl64(lik, kw, x @ beta[1], y)
        keep = np.arange(M) != zero_obs
        w = dl[keep]
        if float(w @ w) > 0.0:
            v = rs.randn(int(keep.sum()))
            for _ in range(2):
                v = v - (v @ w) / (w @ w) * w
            v = v + 1e-12 * np.linalg.norm(v) / np.linalg.norm(w) * w
            x[keep, ortho] = v
            info['ortho_row'] = 1

    rows = np.arange(n)
    if n > 4 * SAMPLE_ROWS:
        rows = np.unique(np.concatenate([[0, 1, 2], np.round(np.linspace(0, n - 1, SAMPLE_ROWS - 3))
                                         ]).astype(np.int64))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.all(np.isfinite(beta))
    # the float64 restatement stays finite on the whole case
    with np.errstate(over='raise', divide='raise', invalid='raise'):
        lp, g = gc.restatement(x, y, **kw)(beta)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), (lik, D, M, n)
    for arr in (x, y, beta, rows):
        arr.setflags(write=False)
    return Case(x, y, kw, beta, rows, info)


@functools.lru_cache(maxsize=None)
def edge_reference(lik, D, M, n):
    """(Case, Ref at case.beta[case.rows]) of one case, computed once per process and
    shared."""
    c = edge_case(lik, D, M, n)
    ref = reference(c.x, c.y, c.beta[c.rows], **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


# Worst error of the numpy restatement (tests/glm_cases.py) over cases() per
# likelihood, value and gradient entries together, in units of 2^-53 S; measured by
# tests/test_oracle_glm_mp.py, which asserts twice these figures.  The GPU tests
# allow the kernels 8 times them.
GLM_ORACLE_ERR = {
    # gradient column 0 at (D, M, n) = (20, 65, 17), row 3 (scale 0.7, prior scale 3);
    # the worst value is 2.07 at (16, 130, 70)
    'gaussian': 3.65,
    # gradient column 57 at (128, 70, 16), row 5 (nu = 1e6, sigma = 1e3): the order of the
    # matrix product's sum over m beside the two +-1e6 residuals, whose l' = +-0.5 cancel
    # (the same terms summed by math.fsum: 1.4; one after another: 8.0); value 3.36 at
    # (5, 63, 64)
    'student_t': 11.27,
    # value at (130, 321, 10), row 2, the row with observations at eta = +-1e-9 (prior
    # scale 1e-3); the worst gradient entry is 2.70 at (9, 65, 10)
    'bernoulli_logit': 7.72,
}
