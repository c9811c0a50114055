#!/usr/bin/env python
"""Find the planted-tail (stream, step) pairs of tests/logw_cases.py (TAILS), once.

Scans Philox streams of seed 0 (oracle/vbrng.c vbo_scan_tails; about 2^28 blocks, a
few seconds) for Bailey variates with
  a < 2^12 (U1 < 2^-28),  a > 2^40 - 2^12 (U1 -> 1),
  b in {0, 2^22, 2^23, 3 2^22} and their +-1 neighbours (mod 2^24)
in a row r < ROWS and a pair j < PAIRS, so that one hit serves the row kernel (D = 2 j
+ 1 or 2 j + 2 <= 16), the wave-per-row kernel and the materialised path (D = 17, m =
5).  Prints, per class, the first hits as rows (class, stream, step, row, pair, c, a,
b) to paste into logw_cases.TAILS: for every class one hit in a last odd column (c = 0:
D = 2 j + 1) where the scan has one, and never column 1 (the funnel's log scale, where
a draw of 1e6 sigma leaves the double range).

  python scripts/find_logw_tail_streams.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import rng_oracle as ro   # noqa: E402

ROWS, PAIRS, STEPS = 5, 8, 2
STREAMS = 1 << 22            # x 2 steps x 5 rows x 8 pairs = 2^28.3 blocks
CHUNK = 1 << 16
CENTRES = {0: 'b0', 1 << 22: 'bq1', 1 << 23: 'bh', 3 << 22: 'bq3'}


def classify(a, b):
    if a < (1 << 12):
        return 'a_lo'
    if a > (1 << 40) - (1 << 12):
        return 'a_hi'
    for k, name in CENTRES.items():
        d = (b - k + (1 << 23)) % (1 << 24) - (1 << 23)
        if abs(d) <= 1:
            return name + {-1: '-', 0: '', 1: '+'}[d]
    raise AssertionError((a, b))


def main():
    found = {}
    for s0 in range(1, STREAMS, CHUNK):
        for h in ro.scan_tails(0, s0, min(CHUNK, STREAMS - s0), STEPS, ROWS, PAIRS):
            s, st, r, j, c, a, b = (int(v) for v in h)
            if 2 * j + c == 1:
                continue
            found.setdefault(classify(a, b), []).append((s, st, r, j, c, a, b))
    for cls in sorted(found):
        hits = found[cls]
        odd = [h for h in hits if h[4] == 0 and h[3] >= 1]
        pick = (odd[:1] + [h for h in hits if h not in odd[:1]])[:2 if cls[0] == 'a' else 1]
        for h in pick:
            print("    ('%s', %d, %d, %d, %d, %d, %d, %d)," % ((cls,) + h))
    print('# classes:', {k: len(v) for k, v in sorted(found.items())})


if __name__ == '__main__':
    main()
