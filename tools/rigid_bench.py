#!/usr/bin/env python
"""GPU: time per ops.rigid_fit call (hpl_rigid_fit) at iters = 4 -- the table of profiles/rigid_fit_bench.txt.

Shapes: B = 1 x N = 8 192 (one sampled pair), a ragged B = 16 with counts in [4 096, 8 192], B = 1 x N = 450 000 (a dense
frame).  The scene is the tests' (one rigid motion, 25 % movers, 1 cm noise).  Per shape: warm-up calls, then --repeats
timings of device events around --calls back-to-back calls each; the table gives the median, the fastest and the slowest
repeat per call, and the same for iters = 0 (3 launches) so that the cost of a round shows.  --out FILE also writes the table
there.  --shape I / --iters T restrict the run to one shape / one setting (for a kernel trace of that shape alone)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def per_call_us(fn, calls, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shape', type=int, default=None, choices=[0, 1, 2])
    ap.add_argument('--iters', type=int, default=None)
    a = ap.parse_args()
    from hplflownet_amd import ops
    from rigid_oracle import scene
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    shapes = [('B = 1 x N = 8192', [8192]), ('ragged B = 16, N_b in [4096, 8192]', [int(x) for x in rng.randint(4096, 8193, 16)]),
              ('B = 1 x N = 450000', [450000])]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per ops.rigid_fit call: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up calls' % (
                 a.repeats, a.calls, a.warmup), '']
    for name, counts in shapes if a.shape is None else shapes[a.shape:a.shape + 1]:
        parts = [scene(n, 90 + i) for i, n in enumerate(counts)]
        t = lambda k: torch.from_numpy(np.ascontiguousarray(np.concatenate([x[k] for x in parts], 1))).to(dev)     # noqa: E731
        pc, flow = t(0), t(1).t().contiguous().t()                      # the flow as the models return it: point-major rows
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        out = torch.empty((pc.shape[1], 3), device=dev)
        row = '%-38s points %7d' % (name, pc.shape[1])
        for iters in (4, 0) if a.iters is None else (a.iters,):
            med, lo, hi = per_call_us(lambda: ops.rigid_fit(pc, flow, iters=iters, tau=0.1, prefix=prefix, out=out), a.calls,
                                      a.repeats, a.warmup)
            row += '   iters = %d (%2d launches): %8.1f (%.1f .. %.1f)' % (iters, 2 * (iters + 1) + 1, med, lo, hi)
        R, _, stats, _ = ops.rigid_fit(pc, flow, iters=4, tau=0.1, prefix=prefix, out=out)
        row += '   inlier share %.4f' % float(stats[:, 1].mean())
        lines.append(row)
        print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
