"""Multiprecision restatement of the multilevel regression target (mpmath, 50 digits),
its condition sums and its edge data and rows; shared by the CPU test that pins the
numpy restatement of tests/mlm_cases.py (tests/test_oracle_mlm_mp.py) and the GPU test of
vb_mlm.hip (tests/test_gpu_mlm_edges.py).  In the style of tests/glm_mp.py (whose exact
integer dot products and links it reuses) and tests/hier_mp.py.

The model is the one in the docstring of tests/mlm_cases.py.  Error metric: that of
tests/targets_mp.py, err = |got - ref| / (2^-53 S), S the sum of the absolute values of
the terms added to form the result.  An observation's term contains the cancelling inner
sum eta_m = x_m . beta + a_eff (a_eff = a_g, or tau at_g), which S carries through the
term's derivative as tests/glm_mp.py does: A_m = sum_d |x_md beta_d| + |a_eff| (+ |y_m|
for gaussian and student_t), T, l', l'' as there, R_m = T(l'_m) + |l''_m| A_m:

  S_lp     = sum_d beta_d^2 / (2 s^2) + p |log(2 pi)/2 + log s| + M |c_obs|
             + |log(2 / (pi s_tau))| + log1p(w) + |u| + G log(2 pi)/2
             + sum_m [T(l_m) + |l'_m| A_m]
             + (centred: G |u| + sum (a_g / tau)^2 / 2;  non-centred: sum at_g^2 / 2)
  S_beta_d = |beta_d| / s^2 + sum_m R_m |x_md|
  centred      S_a_g = sum_{m in g} R_m + |a_g| / tau^2
               S_u   = 1 + 2 w / (1 + w) + sum (a_g / tau)^2 + G
  non-centred  S_at_g = tau sum_{m in g} R_m + |at_g|
               S_u   = 1 + 2 w / (1 + w) + tau sum_g |at_g| sum_{m in g} R_m
"""
import functools
from collections import namedtuple

import numpy as np

from tests import glm_mp as gm
from tests import mlm_cases as mc
from tests import targets_mp as tm
from tests.targets_mp import DIGITS, RANDOM_SHARE, UNIT, Ref, errors   # noqa: F401

try:
    from mpmath import mp, mpf
except Exception:                      # the CPU tests skip without it
    mp = mpf = None


def available():
    return tm.available()


LOGIT_SATURATED = 5000.0


def _link(lik, eta, y, nu, sig):
    """tests/glm_mp.py's _link.  Past |eta| = LOGIT_SATURATED the logit link's
    exp(-|eta|) < 1e-2171 is taken as 0 (a non-centred row at log tau = 20 has eta ~ 1e8,
    whose exponential costs mpmath seconds): the terms it would add are below 1e-2000 of
    the S they are measured against."""
    if lik == 'bernoulli_logit' and abs(eta) > LOGIT_SATURATED:
        pos = eta if eta > 0 else mpf(0)
        pr = mpf(1) if eta > 0 else mpf(0)
        return y * eta - pos, y - pr, float(abs(y * eta) + pos), float(y + pr), 0.0
    return gm._link(lik, eta, y, nu, sig)


def reference(x, y, group, z, likelihood='gaussian', df=None, scale=1.0, prior_scale=10.0,
              tau_scale=5.0, centered=False, n_groups=None):
    """Ref of the model at the rows of z [n][p + 1 + G]."""
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
        s, st = mpf(float(prior_scale)), mpf(float(tau_scale))
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
        c_tau = mp.log(2 / (mp.pi * st))
        c_all = -p * c_prior + M * c_obs + c_tau - G * half_l2pi
        s_const = float(p * abs(c_prior) + M * abs(c_obs) + abs(c_tau) + G * half_l2pi)
        Y = [mpf(v) for v in y.tolist()]
        ix, ex = gm._ints(x)
        ib, eb = gm._ints(z[:, :p])
        xb_i = np.dot(ib, ix.T)                               # exact, [n][M]
        xb_abs = np.abs(z[:, :p]) @ np.abs(x).T
        if likelihood != 'bernoulli_logit':
            xb_abs = xb_abs + np.abs(y)[None, :]
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
                eta = mp.ldexp(mpf(xb_i[r, m]), ex + eb) + ae
                l, dl, t_l[m], t_g, d2 = _link(likelihood, eta, Y[m], nu, sig)
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


# ---- the shapes (p, G, M): the smallest that reach each instance of vb_mlm.hip ---------
# lane-per-row kernel (p <= 16; PP = 2, 4, 8, 16): G = 1 in one chunk; G = 8 over three
# chunks, the large group spanning chunk boundaries, one group empty; G = 70 (more groups
# than a tile) over six chunks, most groups empty or small; two chunks at PP = 8.
# tile kernel: p = 17 (two column slices, the second of one column) and p = 40.
SHAPES = ((2, 1, 40), (3, 8, 129), (5, 8, 65), (16, 70, 321), (17, 3, 65), (40, 5, 130))
U_CENTRES = tm.ES_LOG_TAU          # (-40, -8, -2, 0, 1.6, 4, 20)
BLOCK_ROWS = 4                     # rows per log tau centre and block
ETA_FAR = 40.0                     # |eta| reached by the far rows of the logit link
RESID_FAR = 1e6                    # |y - eta| reached by the far rows of the location links
SEED = 20240702

Case = namedtuple('Case', 'x y group kw z')


def cases():
    """Every (likelihood, centred, p, G, M) of the edge tests."""
    return [(lik, c, p, G, M) for (p, G, M) in SHAPES for c in mc.FORMS for lik in mc.LIKELIHOODS]


def _eta(x, group, zr, p, centered):
    tau = np.exp(zr[p])
    a = zr[p + 1:]
    return x @ zr[:p] + (a if centered else tau * a)[group]


@functools.lru_cache(maxsize=None)
def edge_case(lik, centered, p, G, M):
    """The seeded data and edge rows of one case.  Per log tau centre of U_CENTRES a block
    of BLOCK_ROWS rows with the other coordinates standard normal and log tau jittered
    (the centre itself once); the centred form has a second block per centre with
    a = tau randn, the prior's own region.  The last row of every block is a far row:
    beta and the intercepts scaled together so that max |eta| = ETA_FAR (logit) or
    max |y - eta| ~ RESID_FAR (gaussian, student_t).  The last RANDOM_SHARE of the rows
    are standard normal."""
    i = SHAPES.index((p, G, M))
    li = mc.LIKELIHOODS.index(lik)
    x, y, group = mc.make_data(p, G, M, lik, seed=40 + i)
    kw = mc.model_kwargs(lik, centered)
    rs = np.random.RandomState(SEED + 1000 * i + 10 * li + int(centered))
    D = p + 1 + G
    k = BLOCK_ROWS
    blocks = []
    for uc in U_CENTRES:
        for own in ((False, True) if centered else (False,)):
            blk = rs.randn(k, D)
            blk[:, p] = tm._jit(rs, uc, k)
            blk[0, p] = uc
            if own:
                blk[:, p + 1:] *= np.exp(blk[:, p:p + 1])
            far = blk[k - 1]
            eta = _eta(x, group, far, p, centered)
            top = float(np.max(np.abs(eta)))
            if top > 0.0:
                f = (ETA_FAR if lik == 'bernoulli_logit' else RESID_FAR) / top
                far[:p] *= f
                far[p + 1:] *= f
            blocks.append(blk)
    z = np.concatenate(blocks)
    n_rand = max(1, int(round(RANDOM_SHARE * z.shape[0] / (1.0 - RANDOM_SHARE))))
    z = np.concatenate([z, rs.randn(n_rand, D)])
    assert np.all(np.isfinite(z))
    for arr in (x, y, group, z):
        arr.setflags(write=False)
    return Case(x, y, group, kw, z)


@functools.lru_cache(maxsize=None)
def edge_reference(lik, centered, p, G, M):
    """(Case, Ref at case.z) of one case, computed once per process and shared."""
    c = edge_case(lik, centered, p, G, M)
    ref = reference(c.x, c.y, c.group, c.z, n_groups=G, **c.kw)
    for arr in ref:
        arr.setflags(write=False)
    return c, ref


# Worst error of the numpy restatement (tests/mlm_cases.py) over cases() per form, value
# and gradient entries together, in units of 2^-53 S; measured by
# tests/test_oracle_mlm_mp.py, which asserts twice these figures.  The GPU test allows
# the kernels 8 times them.  Keyed by `centered`.
MLM_ORACLE_ERR = {
    # non-centred: d at_69 (column 86) at (p, G, M) = (16, 70, 321), bernoulli_logit, row 27
    # (the far row at log tau = 20.003: tau S_g against at_g)
    False: 3.32,
    # centred: d u (column 2) at (2, 1, 40), student_t, row 35
    # (log tau = 1.599)
    True: 3.85,
}
