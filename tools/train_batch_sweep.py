#!/usr/bin/env python
"""GPU: training throughput of the trainer's pipeline (engine.Trainer.train_epoch: fused lattice builds on a producer thread and a
side stream, the native training step -- TrainPlan.step / step_batch --, the flat Adam step) over B x N, HPLFlowNet: one table for
profiles/rNN_train_batch_sweep.txt.

For every N and every B > 1, a B = 1 run and a B run alternate `--repeats` times in the same process (a fresh Trainer each run,
the same pairs).  Per run: ms per step and pairs/s over `--pairs` pairs after `--warmup` pairs, torch.cuda.max_memory_allocated
over the timed pairs, and the program's largest matrix at that batch (TrainPlan.largest_matrix: the plan refuses batches whose
largest matrix reaches 2 GiB, the kernels' 32-bit offsets)."""
import argparse
import collections
import gc
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Pool(object):
    """`count` samples cycling over a few device-resident pairs."""

    def __init__(self, pairs, count):
        self.pairs, self.count = pairs, count

    def __len__(self):
        return self.count

    def __getitem__(self, i):
        return self.pairs[i % len(self.pairs)]

    def point_counts(self, i):
        p = self.pairs[i % len(self.pairs)]
        return p[0].shape[-1], p[1].shape[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--points', default='2048,8192')
    ap.add_argument('--batches', default='2,4,8')
    ap.add_argument('--pairs', type=int, default=128, help='timed pairs per run (a multiple of every B)')
    ap.add_argument('--warmup', type=int, default=16, help='pairs of the untimed epoch before (a multiple of every B)')
    ap.add_argument('--repeats', type=int, default=2, help='alternating B = 1 / B runs per (N, B)')
    ap.add_argument('--max-points', type=int, default=65536, help='refuse B x N above this (memory of the shared GPU)')
    a = ap.parse_args()
    from hplflownet_amd import engine
    from hplflownet_amd.synthetic import synthetic_pair
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)

    def run(n, B, pairs):
        tr = engine.Trainer('HPLFlowNet', dev, init='hash')
        tr.train_epoch(Pool(pairs, a.warmup), batch_size=B)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        steps0 = tr.native_steps
        t0 = time.perf_counter()
        loss = tr.train_epoch(Pool(pairs, a.pairs), batch_size=B)          # (ends in a host read of the loss: synchronised)
        dt = time.perf_counter() - t0
        steps = tr.native_steps - steps0
        mem = torch.cuda.max_memory_allocated(dev)
        big = None
        if B > 1:
            p1 = torch.stack([p[0] for p in pairs[:B]])
            p2 = torch.stack([p[1] for p in pairs[:B]])
            lat = tr.gen.build_native_batch(p1, p2, for_training=True)
            arr, nl, _ = tr.tplan.tables(lat)
            big = tr.tplan.largest_matrix(arr, nl)
        else:
            lat = tr.gen.build_native(pairs[0][0], pairs[0][1]).device_lattice().prepare(True)
            arr, nl, _ = tr.tplan.tables(lat)
            big = tr.tplan.largest_matrix(arr, nl)
        del tr, lat
        gc.collect()
        torch.cuda.empty_cache()
        assert steps == a.pairs // B, (steps, a.pairs, B)          # every step took the native program
        return dt * 1e3 / steps, a.pairs / dt, mem, big, loss

    print('# python tools/train_batch_sweep.py --pairs %d --warmup %d --repeats %d   (HPLFlowNet, hash init, frustum pairs; one '
          'MI355X; engine.Trainer.train_epoch: producer-thread fused lattice builds + native step + flat Adam)'
          % (a.pairs, a.warmup, a.repeats))
    print('# median over the repeats (min .. max pairs/s); x B=1: against the B = 1 runs alternated with that B; peak memory: '
          'max_memory_allocated over the timed pairs; largest matrix: the program\'s at that batch')
    print('%-6s %-3s %9s %9s %19s %8s %9s %22s' % ('N', 'B', 'ms/step', 'pairs/s', '(min .. max)', 'x B=1', 'peak GB',
                                                   'largest matrix'))
    for n in [int(x) for x in a.points.split(',')]:
        pairs = []
        for s in range(16):
            trio = synthetic_pair(n, 300 + s)
            pairs.append(tuple(torch.from_numpy(np.ascontiguousarray(x.T)).to(dev) for x in trio))
        rows = collections.OrderedDict()
        for B in [int(x) for x in a.batches.split(',')]:
            if B * n > a.max_points:
                print('# N = %d, B = %d: skipped (B x N > %d)' % (n, B, a.max_points))
                continue
            for _ in range(a.repeats):
                for b in (1, B):
                    rows.setdefault((b, B), []).append(run(n, b, pairs))
        for B in [int(x) for x in a.batches.split(',')]:
            if (B, B) not in rows:
                continue
            base = float(np.median([r[1] for r in rows[(1, B)]]))
            for b in (1, B):
                rs = rows[(b, B)]
                rate = float(np.median([r[1] for r in rs]))
                ms = float(np.median([r[0] for r in rs]))
                big = rs[0][3]
                print('%-6d %-3d %9.2f %9.1f %19s %8.2f %9.2f %22s' % (
                    n, b, ms, rate, '(%.1f .. %.1f)' % (min(r[1] for r in rs), max(r[1] for r in rs)), rate / base,
                    max(r[2] for r in rs) / 1e9, '%d x %d, %.3f GiB' % (big[1], big[2], big[0] / 2.0 ** 30)))
            print('#')
        sys.stdout.flush()


if __name__ == '__main__':
    main()
