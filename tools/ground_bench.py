#!/usr/bin/env python
"""GPU: time per ops.ground_fit call (hpl_ground_fit) -- the table of profiles/ground_bench.txt.

Shapes: B = 1 x n = 8 192 (one sampled cloud), a ragged B = 16 with counts in [4 096, 8 192], and B = 2 x n = 450 000 (a whole
KITTI pair).  The scenes are the tests' generator's (half ground, 3 cm noise).  Per shape and setting: warm-up calls, then
--repeats timings of device events around --calls back-to-back calls each; the table gives the median, the fastest and the
slowest repeat per call.  Settings: hyps 256 and 1024 at refine 0 and 2, and hyps 1 at refine 0 -- everything but the vote
(the same launches, a vote of one hypothesis) --, so that the vote (a column minus that one), the refinement's dependent
launches (refine 2 minus refine 0) and the rest (hypotheses, pick, classification, compaction) can be read apart.  The numpy
restatement on the host is timed once per shape (hyps 256, refine 2).  --out FILE also writes the table there; --shape I
restricts the run to one shape."""
import argparse
import os
import sys
import time

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
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shape', type=int, default=None, choices=[0, 1, 2])
    ap.add_argument('--no-host', action='store_true', help='skip the timing of the numpy restatement')
    a = ap.parse_args()
    from hplflownet_amd import ops
    import ground_oracle as G
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    shapes = [('B = 1 x n = 8192', [8192]), ('ragged B = 16, n_b in [4096, 8192]', [int(x) for x in rng.randint(4096, 8193, 16)]),
              ('B = 2 x n = 450000', [450000, 450000])]
    settings = [(1, 0), (256, 0), (256, 2), (1024, 0), (1024, 2)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per ops.ground_fit call (tau 0.1, cut 0.3, tilt 20): median (fastest .. slowest) of %d repeats of %d back-to-back '
             'calls, %d warm-up calls; launches = 6 + 2 refine' % (a.repeats, a.calls, a.warmup), '']
    for name, counts in shapes if a.shape is None else shapes[a.shape:a.shape + 1]:
        host = np.concatenate([G.scene(n, 70 + i)[0] for i, n in enumerate(counts)], axis=1)
        pc = torch.from_numpy(host).to(dev)
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        row = '%-36s points %7d' % (name, pc.shape[1])
        for hyps, refine in settings:
            med, lo, hi = per_call_us(lambda: ops.ground_fit(pc, prefix=prefix, hyps=hyps, refine=refine), a.calls, a.repeats, a.warmup)
            row += '   hyps %4d refine %d: %8.1f (%.1f .. %.1f)' % (hyps, refine, med, lo, hi)
        stats = ops.ground_fit(pc, prefix=prefix, hyps=256, refine=2)[1].cpu().numpy()
        row += '   kept share %.4f' % (stats[:, 3].sum() / float(pc.shape[1]))
        if not a.no_host:
            t0 = time.perf_counter()
            want = G.ground_fit(host, prefix, hyps=256, refine=2)
            row += '   numpy restatement (hyps 256, refine 2): %.1f ms' % ((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(want['stats'][:, :3], stats[:, :3])
        lines.append(row)
        print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
