"""Shapes and runner of the column-pair kernel's bit-exactness fixture
(tests/golden/sep_bits.npz, written by scripts/make_sep_bits_fixture.py, compared by
tests/test_gpu_sep_bits.py).

Config 3's path (mean-field Gaussian KLVI + adagrad, isotropic Gaussian target, Philox
draws, DeviceRun) at the smallest shapes that reach every path of sep_kernel's
optimisation instance:

* D = 2 081: 1 041 column pairs, which sep_split deals as 16 pairs in four 4-pair
  waves and 1 025 pairs in 1-pair waves; the last pair has one column.
* N in {1, 15, 16, 17, 64, 65, 128}: the pipelined first row alone, full rows and the
  ragged remainder row of both bodies (16 and 64 lanes per pair).
* W in {1, 10, 16}: the register window with one slot, with the benchmark's ten and
  full.
* 9 steps in launches of 5, 3 and 1: a full group of four value partials and a tail
  in one launch, partial groups only in the others; the window wraps (W = 1) and
  resumes across launches; the three history rows come from two launches.

A case's lam, smooth and three history rows are 5 x 4 162 doubles, 21 cases 3.5 MB: too
much to commit.  The fixture keeps every bit all the same: per case the sha256 of the
full lam / hist / vals / smooth bytes (compared for equality), and -- so that a
mismatch shows where -- the values themselves at COLS (every column of the 4-pair
waves, the first, some middle and the last 1-pair waves, single-column pair included)
and all of vals.
"""
import hashlib

import numpy as np

D = 2081
NS = (1, 15, 16, 17, 64, 65, 128)
WS = (1, 10, 16)
LAUNCHES = (5, 3, 1)
N_ITERS = sum(LAUNCHES)
LR, EPS, SEED, STREAM = 0.01, 0.1, 0, 1
# columns 0..31: the sixteen pairs of the 4-pair waves; 32..47: the first two blocks
# of 1-pair waves; 1 024..1 039 and 2 065..2 080: middle and last 1-pair waves
COLS = np.concatenate([np.arange(0, 48), np.arange(1024, 1040), np.arange(2065, 2081)])
PCOLS = np.concatenate([COLS, D + COLS])      # means, then log scales
CASES = [(n, w) for n in NS for w in WS]


def init_params():
    return np.concatenate([np.linspace(-1.0, 1.0, D), np.linspace(-0.5, 0.3, D)])


def run_case(n, w):
    """(lam [2D], hist [3][2D], vals [9], smooth [2D]) of one case on the loaded library."""
    from viabel_amd import targets, vb
    fam = vb.mean_field_gaussian_variational_family(D, rng='philox')
    obj = vb.black_box_klvi(fam, targets.isogauss(D), n)
    run = vb.DeviceRun(obj, N_ITERS, init_params()[None, :], window=w, learning_rate=LR,
                       epsilon=EPS)
    done = 0
    for cs in LAUNCHES:
        run.advance_philox(cs, SEED, STREAM, done)
        done += cs
    lam, hist, vals, smooth = run.result()
    return lam[0], hist[0], vals[0], smooth[0]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def record(n, w):
    """The fixture's entries of one case."""
    lam, hist, vals, smooth = run_case(n, w)
    assert hist.shape == (N_ITERS - 3 * N_ITERS // 4, 2 * D)
    return {'lam': lam[PCOLS], 'hist': hist[:, PCOLS], 'vals': vals, 'smooth': smooth[PCOLS],
            'sha256': digest(lam, hist, vals, smooth)}
