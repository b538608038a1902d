#!/usr/bin/env python
"""GPU: time per ops.motion_segment call (hpl_motion_segment) at eps = 0.5 -- the table of
profiles/segment_bench.txt.

Shapes: B = 1 x N = 8 192 with 25 % movers (one sampled pair), B = 1 x N = 450 000 with 25 % and with 100 % movers (a dense
frame).  The cloud is uniform in the tests' volume (30 x 4 x 33 m); the movers are the points of three 2.5 m slabs across x
(25 %), or every point, with a second flow.  Per shape: warm-up calls, then --repeats timings of device events around --calls
back-to-back calls each; the table gives the median, the fastest and the slowest repeat per call and what the call found.
--out FILE also writes the table there.  --shape I restricts the run to one shape (for a kernel trace of that shape alone)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def frame(n, share, seed):
    r = np.random.RandomState(seed)
    p = np.stack([r.uniform(-15, 15, n), r.uniform(-2, 2, n), r.uniform(2, 35, n)]).astype(np.float32)
    moving = (np.floor((p[0] + 15) / 2.5) % 4 == 0) if share < 1 else np.ones(n, bool)
    f = (0.01 * r.normal(size=(3, n))).astype(np.float32)
    f[0, moving] += 1.0
    return p, f, np.where(moving, 1.0, 0.01).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shape', type=int, default=None, choices=[0, 1, 2])
    a = ap.parse_args()
    from hplflownet_amd import ops
    dev = torch.device('cuda:0')
    shapes = [('B = 1 x N = 8192, 25 % movers', 8192, 0.25), ('B = 1 x N = 450000, 25 % movers', 450000, 0.25),
              ('B = 1 x N = 450000, 100 % movers', 450000, 1.0)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per ops.motion_segment call (tau 0.1, eps 0.5, dv 0.3, min_points 5, max_objects 256): median (fastest .. slowest) '
             'of %d repeats of %d back-to-back calls, %d warm-up calls' % (a.repeats, a.calls, a.warmup), '']
    for i, (name, n, share) in enumerate(shapes if a.shape is None else shapes[a.shape:a.shape + 1]):
        p, f, r = frame(n, share, 90 + i)
        pc, res = torch.from_numpy(p).to(dev), torch.from_numpy(r).to(dev)
        flow = torch.from_numpy(f).to(dev).t().contiguous().t()          # the flow as the models return it: point-major rows
        out = torch.empty(n, dtype=torch.int32, device=dev)
        fn = lambda: ops.motion_segment(pc, flow, res, tau=0.1, eps=0.5, dv=0.3, min_points=5, out=out)     # noqa: E731
        med, lo, hi = per_call_us(fn, a.calls, a.repeats, a.warmup)
        st = fn()[3][0].tolist()
        row = '%-34s %9.1f (%.1f .. %.1f)   movers %d objects %d points in objects %d' % (name, med, lo, hi, st[0], st[1], st[2])
        lines.append(row)
        print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
