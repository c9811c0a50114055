"""A/B of library builds on the headline's launch pair (sep_kernel + sep_values_kernel),
from the launch times bench.py collects (run_cfg3 / vb_run_set_timing) and from its wall
clock.  The launch times are the library's own records -- HIP events up to the build that
moved them to device stamps, stamps (first block's entry to the value reduction's last
store) since -- so across that change only the wall figures compare like with like.

  python scripts/ab_sep_launch.py [--rounds R] [--steps K --warmup W] LIB_A LIB_B

Every measurement is a fresh process that loads one library (VIABEL_AMD_LIB) and runs
bench.py's own config-3 run (default: the plain run, 2 000 steps after 100, i.e. seven
256-step launches and one of 208).  Rounds alternate the order (A B, B A, ...): the second
process of a back-to-back pair measures slower with identical libraries.
One JSON line per process -- the median and the extremes of its 256-step (or, for short
runs, its longest) launches, in us -- then a summary line per library: the median over
processes of those medians, and their spread (max - min), and the same two figures of
the wall time per step (bench.py's ms_per_step x 1 000).  LIB_A == LIB_B gives the spread
of the method itself.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from viabel_amd import _native as nat
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    nat.use_stream(0, stream.cuda_stream)
    elapsed, launches, run = bench.run_cfg3(torch, stream, dev, bench.N, steps, warmup, 0, None)
    kmax = max(k for k, _, _ in launches)
    us = sorted(t * 1e6 for k, _, t in launches if k == kmax)
    print(json.dumps({'lib': os.path.basename(nat.LIB_PATH), 'build': nat.lib().vb_build_id().decode(),
                      'steps_per_launch': kmax, 'launches': len(us),
                      'launch_us_median': round(statistics.median(us), 2),
                      'launch_us_min': round(us[0], 2), 'launch_us_max': round(us[-1], 2),
                      'us_per_step_wall': round(elapsed / steps * 1e6, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('libs', nargs='*')
    args = ap.parse_args()
    if args.child:
        return child(args.steps, args.warmup)
    if len(args.libs) != 2:
        ap.error('two libraries (they may be the same file)')
    med = {0: [], 1: []}
    wall = {0: [], 1: []}
    for r in range(args.rounds):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            env = dict(os.environ, VIABEL_AMD_LIB=os.path.abspath(args.libs[which]),
                       VIABEL_AMD_PROGRESS='0')
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--steps',
                                  str(args.steps), '--warmup', str(args.warmup)], env=env,
                                 stdout=subprocess.PIPE, text=True, timeout=300)
            if out.returncode != 0:       # a failed process ends the comparison
                sys.exit(out.returncode if out.returncode > 0 else 1)
            rec = json.loads(out.stdout.strip().split('\n')[-1])
            rec.update(round=r, side='AB'[which])
            print(json.dumps(rec), flush=True)
            med[which].append(rec['launch_us_median'])
            wall[which].append(rec['us_per_step_wall'])
    for which in (0, 1):
        print(json.dumps({'side': 'AB'[which], 'lib': os.path.basename(args.libs[which]),
                          'median_of_medians_us': round(statistics.median(med[which]), 2),
                          'spread_us': round(max(med[which]) - min(med[which]), 2),
                          'medians_us': med[which],
                          'wall_us_per_step_median': round(statistics.median(wall[which]), 3),
                          'wall_us_per_step_spread': round(max(wall[which]) - min(wall[which]), 3),
                          'wall_us_per_step': wall[which]}), flush=True)


if __name__ == '__main__':
    main()
