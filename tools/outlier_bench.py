#!/usr/bin/env python
"""GPU: time per ops.outlier_filter call (hpl_outlier_filter) -- the table of profiles/outlier_bench.txt.

Shapes at radius 1: B = 1 x 8 192 and B = 16 x 8 192 points of the tests' scene with strays (tests/outlier_oracle.py: the surface
scene of the normals tests and 2 % strays above it), and B = 1 x 450 000 points of that scene; the statistical mode at k = 8,
16 and 32 and the radius mode (min_neighbors 5).  Per shape: warm-up calls, then --repeats timings of device events around
back-to-back calls; the table gives the median, the fastest and the slowest repeat per call.  The split of a call into its
launches -- keys, the radix sort, the search, the two sums, thresh, classify, scan, emit -- comes with --split from one profiled
run per shape (torch.profiler's kernel records), where the profiler is available.

Beside it at 8 192 points the composition a user would write in torch on the device: cdist, topk, mean / std, mask (no radius,
float32 sums), and ops.normals(return_neighbors=True) plus torch (the sorted grid's neighbours, then sqrt, mean, std, mask).
The worst case for the grid: all points in one cell.  Nothing here is a pass bar.  --out FILE also writes the table there."""
import argparse
import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LAUNCHES = ('k_outlier_keys', 'k_outlier_search', 'k_outlier_sum1', 'k_outlier_sum2', 'k_outlier_thresh', 'k_outlier_classify',
            'k_outlier_scan', 'k_outlier_emit')


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


def kernel_split_us(fn, calls=5):
    """'name us, ...' per call from the profiler's kernel records (what is no kernel of the op counts as the sort), or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        us = collections.OrderedDict((name, 0.0) for name in LAUNCHES[:1] + ('sort',) + LAUNCHES[1:])
        for ev in prof.events():
            if 'cuda' not in str(ev.device_type).lower():
                continue
            t = float(getattr(ev, 'device_time', 0.0) or getattr(ev, 'cuda_time', 0.0) or 0.0)
            us[next((name for name in LAUNCHES if name in ev.name), 'sort')] += t
        if us['k_outlier_search'] <= 0:
            return None
        return ', '.join('%s %.1f' % (name.replace('k_outlier_', ''), v / calls) for name, v in us.items() if v > 0)
    except Exception as e:                       # noqa: BLE001 (a measurement helper: say what happened and go on)
        print('profiler unavailable: %r' % (e,), flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--split', action='store_true', help='also profile one run per shape for the per-launch split')
    ap.add_argument('--small', action='store_true', help='tiny shapes: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    from hplflownet_amd import ops
    import outlier_oracle as O
    dev = torch.device('cuda:0')
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
    one, big = (512, 2000) if a.small else (8192, 450000)
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per call: median (fastest .. slowest) of %d repeats of back-to-back calls; radius 1.0, std_ratio 2.0' % a.repeats, '']

    def say(row):
        lines.append(row)
        print(row, flush=True)
    modes = [('statistical k =  8', dict(k=8)), ('statistical k = 16', dict(k=16)), ('statistical k = 32', dict(k=32)),
             ('radius, 5 neighbours ', dict(mode='radius', min_neighbors=5))]
    # (name, counts, calls, warm-up calls)
    shapes = [('B = 1 x %d' % one, [one], 50, 10), ('B = 16 x %d' % one, [one] * 16, 20, 5), ('B = 1 x %d' % big, [big], 3, 2)]
    for name, counts, calls, warmup in shapes:
        pc = t(np.concatenate([O.scene(n, n // 50, 90 + i)[0] for i, n in enumerate(counts)], 1))
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        keep = torch.empty(pc.shape[1], dtype=torch.uint8, device=dev)
        for mname, kw in modes:
            fn = lambda: ops.outlier_filter(pc, radius=1.0, prefix=prefix, out=keep, **kw)                         # noqa: E731
            med, lo, hi = per_call_us(fn, calls, a.repeats, warmup)
            res = fn()
            split = kernel_split_us(fn) if a.split else None
            say('%-16s %s  %2d calls a repeat   ops.outlier_filter %10.1f (%.1f .. %.1f)   %s   mean count %.2f, kept %.4f' % (
                name, mname, calls, med, lo, hi, ('profiled kernel time: ' + split) if split else 'launch split not measured',
                float(res[3].float().mean()), float(res[0].float().mean())))

    # the compositions in torch at one cloud
    pc = t(O.scene(one, one // 50, 90)[0])
    keep = torch.empty(one, dtype=torch.uint8, device=dev)

    def composed():                              # all pairs, the 16 nearest others, mean / std, mask
        p = pc.t()
        d = torch.cdist(p, p)
        m = d.topk(17, dim=1, largest=False).values[:, 1:].mean(1)
        return m <= m.mean() + 2.0 * m.std()

    def through_normals():                       # the sorted grid's neighbours (the point itself is the first), then torch
        d2 = ops.normals(pc, k=17, radius=1.0, return_neighbors=True)[4][:, 1:]
        m = torch.where(torch.isinf(d2), torch.ones_like(d2), d2.sqrt()).mean(1)
        return m <= m.mean() + 2.0 * m.std()
    native = lambda: ops.outlier_filter(pc, k=16, radius=1.0, out=keep)        # noqa: E731
    rows = []
    for _ in range(2):
        rows.append((per_call_us(composed, 10, a.repeats, 3), per_call_us(through_normals, 20, a.repeats, 5),
                     per_call_us(native, 50, a.repeats, 10)))
    say('')
    say('the torch compositions at %d points, k = 16, us per call, two alternating passes:' % one)
    for (c, g, n_) in rows:
        say('   cdist + topk + mean / std + mask: %10.1f (%.1f .. %.1f)   ops.normals(k = 17, return_neighbors) + torch: %8.1f '
            '(%.1f .. %.1f)   ops.outlier_filter: %8.1f (%.1f .. %.1f)   ratios %.2f, %.2f' % (
                c + g + n_ + (c[0] / n_[0], g[0] / n_[0])))

    # the worst case: every point in one cell -- every point compares with every other
    n = 256 if a.small else 8192
    rng = np.random.RandomState(1)
    p1 = t((np.array([[3.2], [0.2], [10.2]]) + rng.uniform(0, 0.6, (3, n))).astype(np.float32))
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    say('')
    for mname, kw in modes:
        med, lo, hi = per_call_us(lambda: ops.outlier_filter(p1, radius=1.0, out=keep, **kw), 10, a.repeats, 3)
        say('all %d points in one cell, %s: %10.1f (%.1f .. %.1f) us per call' % (n, mname, med, lo, hi))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
