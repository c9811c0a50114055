"""Device model plugins: numpy restatements (log p and gradient) of the three shipped
models of viabel_amd/models, their data packers, and the built code objects -- shared by
tests/test_plugin_host.py (no GPU) and tests/test_gpu_plugin.py."""
import math
import os

import numpy as np

from tests.conftest import ROOT

MODELS = os.path.join(ROOT, 'viabel_amd', 'models')
RR_DMAX = 32     # models/robust_regression.hip
LAUNCH = {'robust_regression': (256, 4, RR_DMAX), 'banana': (256, 256, 0),
          'isogauss_raw': (128, 128, 0)}


def hsaco(name):
    """The built code object of a shipped model, compiled through plugin.compile when the
    library's build has not made it."""
    from viabel_amd import plugin
    path = os.path.join(MODELS, name + '.hsaco')
    if not os.path.exists(path):
        plugin.compile(os.path.join(MODELS, name + '.hip'), path)
    return path


def robust_regression_data(M, D, seed=0):
    rs = np.random.RandomState(1000 * D + M + seed)
    x = rs.randn(M, D)
    y = x @ rs.randn(D) / math.sqrt(D) + rs.standard_t(5, M)
    return x, y


def robust_regression_block(x, y, nu):
    """[M, nu, X [M][D], y [M]]"""
    return np.concatenate([[float(x.shape[0]), float(nu)], np.ravel(x), y])


def robust_regression(x, y, nu):
    """beta ~ normal(0, 10), y ~ student_t(nu, x beta, 1), Stan's constants dropped (the
    form of tests/notebook_cases.robust_regression_target for any x, y, nu)."""
    def f(b):
        b = np.atleast_2d(b)
        r = y[None, :] - b @ x.T
        lp = (-0.5 * np.sum((b / 10.0) ** 2, axis=1)
              - (nu + 1) / 2 * np.sum(np.log1p(r ** 2 / nu), axis=1))
        g = -b / 100.0 + ((nu + 1) * r / (nu + r ** 2)) @ x
        return lp, g
    return f


def banana(scale=10.0, curvature=0.03):
    """models/banana.hip: x_1 ~ N(0, s^2), x_2 + b x_1^2 - s^2 b ~ N(0, 1), the rest N(0, 1),
    constants dropped; D = 1 keeps the first factor."""
    s2, b = scale * scale, curvature

    def f(x):
        x = np.atleast_2d(x)
        g = -x.copy()
        lp = -0.5 * x[:, 0] ** 2 / s2 - 0.5 * np.sum(x[:, 2:] ** 2, axis=1)
        g[:, 0] = -x[:, 0] / s2
        if x.shape[1] >= 2:
            t = x[:, 1] + b * x[:, 0] ** 2 - s2 * b
            lp = lp - 0.5 * t * t
            g[:, 0] -= 2.0 * b * x[:, 0] * t
            g[:, 1] = -t
        return lp, g
    return f


def isogauss(x):
    x = np.atleast_2d(x)
    return np.sum(-0.5 * x * x - 0.5 * math.log(2 * math.pi), axis=1), -x
