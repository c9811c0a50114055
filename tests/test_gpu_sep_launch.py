"""Launch timing of the column-pair path from device stamps (vb_run_set_timing /
vb_run_launch_times): sep_kernel's blocks stamp their entry, sep_values_kernel's the
time after their store, and the host makes no call for the record ahead of the launch.

Shape: tests/sep_bits_cases.py's D = 2 081 (both wave kinds, a ragged last wave), N = 5,
W = 10.  The library runs on a torch stream here so that torch events bracket its work.
"""
import ctypes

import numpy as np
import pytest

from tests import sep_bits_cases as sc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason='needs an MI355X')]

N, W = 5, 10
K = 20               # steps of the bracketed launch
# Event-pair time minus stamp time of one K-step launch may be at most this.  It is
# three times the spread (max - min) of the event-pair time over 20 repetitions of this
# same launch, measured on the build before the stamps (HIP-event records inside the
# library): 7.88 us (38.40 ... 46.28 us), profiles/sep_launch/stamp_vs_event.log.  (A second
# run of that measurement, on another machine, gave 3.64 us; the first one stands.)
MARGIN_SPREAD_US = 7.88
MARGIN_US = 3.0 * MARGIN_SPREAD_US


def make_run(n_iters, timing):
    from viabel_amd import targets, vb
    fam = vb.mean_field_gaussian_variational_family(sc.D, rng='philox')
    obj = vb.black_box_klvi(fam, targets.isogauss(sc.D), N)
    run = vb.DeviceRun(obj, n_iters, sc.init_params()[None, :], window=W, learning_rate=sc.LR,
                       epsilon=sc.EPS)
    if timing is not None:
        run.set_timing(timing)
    return run


_KEPT = []   # the module's context outlives every run made on it (runs point at it)


@pytest.fixture()
def torch_stream():
    """The library's default context on a torch stream for the test, then back."""
    import torch
    from viabel_amd import _native as nat
    saved_ctx, saved_dev = dict(nat._ctx), list(nat._default_device)
    if not _KEPT:
        stream = torch.cuda.Stream(device=0)
        _KEPT.extend([stream, nat.Context(0, ctypes.c_void_p(stream.cuda_stream))])
    stream, ctx = _KEPT
    nat._ctx[0] = ctx
    nat._default_device[0] = 0
    with torch.cuda.stream(stream):
        yield stream
        torch.cuda.synchronize()
    nat._ctx.clear()
    nat._ctx.update(saved_ctx)
    nat._default_device[:] = saved_dev


def bracketed_launch(run, stream, steps, step0):
    """One advance between two torch events on the library's stream: (event seconds,
    the launch records of the call)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    run.advance_philox(steps, sc.SEED, sc.STREAM, step0)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, run.launch_times()


def warmed_run(stream, n_iters):
    """A timed run after one K-step launch whose records are dropped."""
    run = make_run(n_iters, True)
    run.advance_philox(K, sc.SEED, sc.STREAM, 0)
    assert [k for k, _ in run.launch_times()] == [K]
    return run


def test_stamps_agree_with_events(torch_stream):
    run = warmed_run(torch_stream, 3 * K + 7)
    assert run.launch_times() == []          # the warm-up's records were dropped
    t_ev, rec = bracketed_launch(run, torch_stream, K, K)
    assert len(rec) == 1 and rec[0][0] == K
    t_st = rec[0][1]
    print('event %.2f us, stamps %.2f us, difference %.2f us'
          % (t_ev * 1e6, t_st * 1e6, (t_ev - t_st) * 1e6))
    assert 0.0 < t_st <= t_ev
    assert (t_ev - t_st) * 1e6 <= MARGIN_US
    # two launches in a row: two records in launch order, read from re-armed slots
    run.advance_philox(K, sc.SEED, sc.STREAM, 2 * K)
    run.advance_philox(7, sc.SEED, sc.STREAM, 3 * K)
    rec = run.launch_times()
    assert [k for k, _ in rec] == [K, 7]
    assert all(0.0 < t < 1e-2 for _, t in rec), rec
    assert run.launch_times() == []


def test_more_launches_than_one_block_of_slots(torch_stream):
    """Slots come in blocks of 64: a 65th launch between two reads takes a new block."""
    n = 131
    run = make_run(n, True)
    for s in range(n):
        run.advance_philox(1, sc.SEED, sc.STREAM, s)
    rec = run.launch_times()
    assert [k for k, _ in rec] == [1] * n
    assert all(0.0 < t < 1e-2 for _, t in rec), (min(rec), max(rec))
    assert run.launch_times() == []


def test_timing_off_leaves_no_trace(torch_stream):
    outs = {}
    for timing in (False, True, None):
        run = make_run(sc.N_ITERS, timing)
        done = 0
        for cs in sc.LAUNCHES:
            run.advance_philox(cs, sc.SEED, sc.STREAM, done)
            done += cs
        rec = run.launch_times()
        assert [k for k, _ in rec] == (list(sc.LAUNCHES) if timing else [])
        outs[timing] = run.result()
    for other in (True, None):
        for a, b in zip(outs[False], outs[other]):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    assert all(np.all(np.isfinite(a)) for a in outs[False])
