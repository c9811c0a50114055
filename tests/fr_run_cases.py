"""Shapes, seeded initial parameters and the bar algebra of
tests/test_gpu_fr_run_edges.py: the device runs (vb_capi.hip advance_fr_steps) of the
Cholesky full-rank Gaussian family ('frg', vb_frg.hip) and of the low-rank-plus-diagonal
family ('lrg', vb_lrg.hip), step by step.

A shape is (D,) for 'frg' and (D, R) for 'lrg'.  The target is isogauss throughout: the
condition sums of frg_mp.np_scales / lrg_mp.np_scales are written for it.

Bars.  One step's error is measured in units of 2^-53 S_u,

    S_u = |lam'| + |step| + r G,

as tests/test_gpu_mf_edges.py does.  G carries the gradient's allowed error through
d step / d g and d step / d q of the update in use (adagrad_carried, ia_carried).  The
reference gradient is the numpy restatement's (tests/frg_cases.py, tests/lrg_cases.py),
not a 50-digit one, so the allowed distance between the kernel's gradient and the
reference's is the kernel's allowance, 8 x the family's gradient record, plus the
restatement's own distance from 50 digits, 1 x the same record: 9 x *_ORACLE_ERR[grad]
units of S_g.  The bar stays 8 x MF_ORACLE_ERR[update], so 8 x MF_ORACLE_ERR[update] x r =
9 x *_ORACLE_ERR[grad], that is r = (9 / 8) *_ORACLE_ERR[grad] / MF_ORACLE_ERR[update].
Every figure is a reference-side record of the repository; none comes from a kernel."""
import numpy as np

from tests import frg_cases as fc
from tests import lrg_cases as lc
from tests import mf_cases as mc

LR0 = 0.05
SEED, STREAM = 3, 5
ALPHA = 2.0
MARGIN = 8.0

# (W, steps, eps, lr_end): W = 1, the wrap at periods 2, 10 and 17, eps << g^2, W past
# the step count, learning_rate_end
WINDOWS = [u for u in mc.UPDATE_CASES if u[0] in (1, 2, 10, 17, 50)]
SHORT = [(2, 5, 0.1, None), (10, 21, 0.1, 0.002)]
assert len(WINDOWS) == 11 and all(u in WINDOWS for u in SHORT)

# frg: P = 2, 152, 170, 594: one tile; one full tile row (mean tile + one diagonal
# tile); a partial second row (the mean tile tj = -1 of row 1 beside a partial diagonal
# tile, 2 blocks); three rows, 9 tiles over 3 blocks
FRG_SHAPES = [(1,), (16,), (17,), (33,)]
# lrg: P = D (R + 2) = 3; exactly the 256 entries of one block; 260, into a second
# block; R = D at the rank limit (P = 323)
LRG_SHAPES = [(1, 1), (64, 2), (65, 2), (17, 17)]
SHAPES = {'frg': FRG_SHAPES, 'lrg': LRG_SHAPES}
# (one block, more than one block) for CHIVI / KLVI_PD; the shape of the several-problem,
# history, host-noise and IA tests
OBJ_SHAPES = {'frg': [(16,), (33,)], 'lrg': [(64, 2), (65, 2)]}
ONE_SHAPE = {'frg': (17,), 'lrg': (65, 2)}


def tag(kind, shape):
    return kind + '-' + 'x'.join('%d' % v for v in shape)


def n_free(kind, shape):
    return fc.n_free(*shape) if kind == 'frg' else lc.n_free(*shape)


def noise_width(kind, shape):
    return sum(shape)


def restatement(kind, shape):
    return fc.CholeskyGaussian(*shape) if kind == 'frg' else lc.LowRankGaussian(*shape)


def lam0(kind, shape, seed=0):
    """Seeded start: mu ~ 0.3 N(0, 1), M_ii / log_d uniform in [-1, 0.5], off-diagonals /
    B ~ 0.05 N(0, 1): every restatement value and condition sum stays finite over the
    step counts of the tests."""
    D = shape[0]
    rs = np.random.RandomState(4000 + 97 * sum(shape) + 7 * len(shape) + seed)
    mu = 0.3 * rs.randn(D)
    dg = rs.uniform(-1.0, 0.5, D)
    if kind == 'frg':
        M = np.tril(0.05 * rs.randn(D, D))
        M[np.diag_indices(D)] = dg
        return np.concatenate([mu, M[np.tril_indices(D)]])
    return lc.pack(mu, dg, 0.05 * rs.randn(D, shape[1]))


def value_grad(kind, ofam, objective, lam, draws):
    """The restatement's (value, gradient) on isogauss at lam on the draws."""
    from oracle.targets_oracle import isogauss
    m = fc if kind == 'frg' else lc
    n = draws.shape[0]
    if objective == 'klvi':
        return m.klvi_value_grad(ofam, isogauss, lam, n, draws=draws)
    if objective == 'klvi_pd':
        return m.klvi_pd_value_grad(ofam, isogauss, lam, n, draws=draws)
    return m.chivi_value_grad(ofam, isogauss, lam, n, ALPHA, draws=draws)


def _keys(kind, objective):
    if objective == 'chivi':
        return 'chivi_value', 'chivi_grad'
    if objective == 'klvi_pd':
        # the Cholesky family's KLVI_PD gradient is KLVI's (frg_mp.FRG_ORACLE_ERR)
        return 'klvi_pd_value', 'klvi_grad' if kind == 'frg' else 'klvi_pd_grad'
    return 'klvi_value', 'klvi_grad'


def scales(kind, ofam, objective, lam, draws):
    """(S of the value, S [P] of the gradient) from the family's np_scales."""
    alpha = ALPHA if objective == 'chivi' else None
    if kind == 'frg':
        from tests import frg_mp
        S = frg_mp.np_scales(lam, draws, alpha)
    else:
        from tests import lrg_mp
        S = lrg_mp.np_scales(ofam, lam, draws, alpha)
    kv, kg = _keys(kind, objective)
    return float(S[kv]), np.asarray(S[kg], dtype=float)


def records(kind, objective):
    """(value record, gradient record) of the family's restatement against 50 digits."""
    if kind == 'frg':
        from tests.frg_mp import FRG_ORACLE_ERR as rec
    else:
        from tests.lrg_mp import LRG_ORACLE_ERR as rec
    kv, kg = _keys(kind, objective)
    return rec[kv], rec[kg]


def grad_weight(kind, objective, update):
    """r of the module docstring; update in {'adagrad', 'rmsprop', 'adam'}."""
    from tests.mf_mp import MF_ORACLE_ERR
    return (MARGIN + 1.0) / MARGIN * records(kind, objective)[1] / MF_ORACLE_ERR[update]


def adagrad_carried(G, GS, step, lr, eps):
    """G, GS: the window's gradients and their S ((cnt, P), oldest first, the current
    one last).  q = eps + sum g_k^2;  lr S_g / sqrt(q) + |step| / q sum_k |g_k| S_g,k."""
    q = eps + np.sum(G * G, axis=0)
    return lr * GS[-1] / np.sqrt(q) + np.abs(step) / q * np.sum(np.abs(G) * GS, axis=0)


def ia_carried(which, G, GS, step, lr, eps):
    """The gradient-carried terms of step i = len(G) - 1 of RMSProp-IA / Adam-IA
    (tests/test_gpu_mf_edges.py test_ia_update_step_by_step)."""
    i = G.shape[0] - 1
    if which == 'rmsprop':
        ck = np.array([1.0 if i == 0 else (0.9 ** i if k == 0 else 0.1 * 0.9 ** (i - k))
                       for k in range(i + 1)])
        den = eps + np.sum(ck[:, None] * G * G, axis=0)
        return (lr * GS[i] / np.sqrt(den)
                + np.abs(step) / den * np.sum(ck[:, None] * np.abs(G) * GS, axis=0))
    ak = np.array([(0.9 ** (i + 1) if k == 0 else 0.1 * 0.9 ** (i - k)) for k in range(i + 1)])
    bk = np.array([(0.9 * 0.999 ** i if k == 0 else 0.001 * 0.999 ** (i - k))
                   for k in range(i + 1)])
    ak, bk = ak / (1 - 0.9 ** (i + 2)), bk / (1 - 0.999 ** (i + 2))
    den = eps + np.sum(bk[:, None] * G * G, axis=0)
    return (lr * np.sum(ak[:, None] * GS, axis=0) / np.sqrt(den)
            + np.abs(step) / den * np.sum(bk[:, None] * np.abs(G) * GS, axis=0))


def fused_cases():
    """Item list of the fused one-problem test: (kind, shape, objective, N, W, steps, eps,
    lr_end).  KLVI at every shape, the whole window list at the two smallest shapes of
    each family and SHORT at the larger ones; CHIVI and KLVI_PD on SHORT at OBJ_SHAPES;
    CHIVI at N = 17 once per family (the weights prologue of every block over more
    samples than one MFMA k-group / one chain step)."""
    out = []
    for kind in ('frg', 'lrg'):
        for k, shape in enumerate(SHAPES[kind]):
            for u in (WINDOWS if k < 2 else SHORT):
                out.append((kind, shape, 'klvi', 5) + u)
        for shape in OBJ_SHAPES[kind]:
            for obj in ('chivi', 'klvi_pd'):
                for u in SHORT:
                    out.append((kind, shape, obj, 3 if obj == 'klvi_pd' else 5) + u)
        out.append((kind, ONE_SHAPE[kind], 'chivi', 17) + SHORT[0])
    return out


def case_id(c):
    kind, shape, obj, N, W, steps, eps, lr_end = c
    return '%s/%s/N%d/W%d/s%d/eps%g/end%s' % (tag(kind, shape), obj, N, W, steps, eps, lr_end)
