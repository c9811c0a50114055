"""bench.py's --dump-outputs writer and the --full gate (host logic, no GPU)."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _results(n_hist, P=2000, n_iters=50):
    rs = np.random.RandomState(1)
    return (rs.randn(1, P), rs.randn(1, n_hist, P), rs.randn(1, n_iters), rs.randn(1, P))


def _load(d):
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def test_small_history_is_written_whole(tmp_path):
    lam, hist, vals, smooth = _results(7)
    bench.dump_outputs(str(tmp_path / 'o'), lam, hist, vals, smooth)
    out = _load(tmp_path / 'o')
    assert sorted(out) == ['hist', 'hist_rows', 'lam', 'smooth', 'vals']
    assert all(a.dtype == np.float64 for a in out.values())
    for name, a in (('lam', lam), ('hist', hist), ('vals', vals), ('smooth', smooth)):
        assert np.array_equal(out[name], a)
    assert np.array_equal(out['hist_rows'], np.arange(7.0))


def test_large_history_is_a_fixed_sample_within_the_size_limit(tmp_path, monkeypatch):
    # the threshold scaled down with the shapes: 16 rows of 2000 doubles
    monkeypatch.setattr(bench, 'DUMP_HIST_BYTES', 16 * 2000 * 8)
    lam, hist, vals, smooth = _results(41)
    bench.dump_outputs(str(tmp_path / 'a'), lam, hist, vals, smooth)
    bench.dump_outputs(str(tmp_path / 'b'), lam, hist, vals, smooth)
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    rows = a['hist_rows'].astype(int)
    assert len(rows) == 16 and len(set(rows)) == 16 and rows[-1] == 40
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(a['hist'], hist[:, rows])
    assert a['hist'].nbytes <= bench.DUMP_HIST_BYTES
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_legs_need_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--legs', 'cfg1'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and '--full' in r.stderr
