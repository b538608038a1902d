#!/usr/bin/env python
"""GPU: one training step under the self-supervised loss, native program (Trainer(loss='selfsup', native_step=True), DESIGN.md
§26) beside the autograd path (the default), HPLFlowNet, equal-count batches: the table of profiles/rNN_selfsup_native_bench.txt.

Two trainers live for the whole run (one per path); per batch size their lattices are built once, outside the timing, and
blocks of `--steps` steps alternate between the two paths `--rounds` times.  A block is timed from a synchronised start to a
synchronised end (host wall time, Adam step included); per path the median, minimum and maximum ms per step over the blocks."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--points', type=int, default=8192)
    ap.add_argument('--batches', default='1,2,4')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--k', type=int, default=8)
    a = ap.parse_args()
    from hplflownet_amd import engine
    from hplflownet_amd.synthetic import synthetic_pair
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    opts = {'k': a.k}
    trainers = (('native', engine.Trainer('HPLFlowNet', dev, init='hash', loss='selfsup', selfsup=opts, native_step=True)),
                ('autograd', engine.Trainer('HPLFlowNet', dev, init='hash', loss='selfsup', selfsup=opts)))
    pool = []
    for s in range(4):
        trio = synthetic_pair(a.points, 300 + s)
        pool.append(tuple(torch.from_numpy(np.ascontiguousarray(x.T)).to(dev) for x in trio))
    print('# python tools/selfsup_native_bench.py --points %d --steps %d --rounds %d --k %d   (HPLFlowNet, hash init, frustum pairs; '
          'one MI355X; lattices built outside the timing; blocks alternate between the paths)' % (a.points, a.steps, a.rounds, a.k))
    print('%-3s %-9s %12s %19s %10s %12s' % ('B', 'path', 'ms/step', '(min .. max)', 'pairs/s', 'native steps'))
    for B in [int(x) for x in a.batches.split(',')]:
        p1, p2, sf = (torch.stack([pool[b % len(pool)][j] for b in range(B)]) for j in range(3))
        runs = {}
        for name, tr in trainers:
            lat = tr.gen.build_native_batch(p1, p2, for_training=True)
            runs[name] = (tr, lat, [])
            tr.train_step_batch(p1, p2, sf, lat)                   # (the plan, the workspace, the optimiser state)
        for _ in range(a.rounds):
            for name, tr in trainers:
                _, lat, ms = runs[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.train_step_batch(p1, p2, sf, lat)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
        for name, tr in trainers:
            ms = runs[name][2]
            med = float(np.median(ms))
            print('%-3d %-9s %12.2f %19s %10.1f %12d' % (B, name, med, '(%.2f .. %.2f)' % (min(ms), max(ms)), B * 1e3 / med,
                                                         tr.native_steps))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
