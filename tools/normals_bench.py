#!/usr/bin/env python
"""GPU: time per ops.normals call (hpl_normals) -- the table of profiles/normals_bench.txt.

Shapes at k = 16, radius 1: B = 1 x 8 192 and B = 16 x 8 192 points of the tests' surface scene (tests/normals_oracle.py: a
16 x 16 m ground, two walls and a half sphere), and B = 1 x 450 000 points of that scene, about 1 100 points per square metre
of surface -- the density of a lidar frame near the sensor.  k = 8 and 32 at 8 192.  Per shape: warm-up calls, then --repeats
timings of device events around back-to-back calls; the table gives the median, the fastest and the slowest repeat per call.
The split of a call into its launches -- keys and the radix sort against the search-and-PCA kernel -- comes with --split from one
profiled run per shape (torch.profiler's kernel records), where the profiler is available.

Beside each shape ops.icp(iters = 0) on the same cloud as src and dst: one 1-nearest pass over the same grid.  At 8 192 the
composition a user would write in torch on the device: cdist, topk, gather, linalg.eigh (no radius, no tie rule, float32).
The worst case for the grid: all points in one cell.  Nothing here is a pass bar.  --out FILE also writes the table there."""
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


def kernel_split_us(fn, calls=5):
    """(keys + sort, search + PCA) in us per call from the profiler's kernel records, or None where it gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        search = rest = 0.0
        for ev in prof.events():
            if 'cuda' not in str(ev.device_type).lower():
                continue
            us = float(getattr(ev, 'device_time', 0.0) or getattr(ev, 'cuda_time', 0.0) or 0.0)
            if 'k_normals<' in ev.name or 'k_normalsILi' in ev.name:
                search += us
            else:
                rest += us
        return (rest / calls, search / calls) if search > 0 else None
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
    import normals_oracle as O
    dev = torch.device('cuda:0')
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
    one, big = (512, 2000) if a.small else (8192, 450000)
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per call: median (fastest .. slowest) of %d repeats of back-to-back calls; radius 1.0' % a.repeats, '']

    def say(row):
        lines.append(row)
        print(row, flush=True)
    # (name, counts, k, calls, warm-up calls)
    shapes = [('B = 1 x %d, k = 16' % one, [one], 16, 50, 10), ('B = 16 x %d, k = 16' % one, [one] * 16, 16, 20, 5),
              ('B = 1 x %d, k = 16' % big, [big], 16, 3, 2), ('B = 1 x %d, k = 8' % one, [one], 8, 50, 10),
              ('B = 1 x %d, k = 32' % one, [one], 32, 50, 10)]
    for name, counts, k, calls, warmup in shapes:
        pc = t(np.concatenate([O.scene(n, 90 + i) for i, n in enumerate(counts)], 1))
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        out = torch.empty((3, pc.shape[1]), device=dev)
        flow = torch.empty((pc.shape[1], 3), device=dev)
        fn = lambda: ops.normals(pc, k=k, radius=1.0, prefix=prefix, out=out)                                  # noqa: E731
        nn = lambda: ops.icp(pc, pc, iters=0, max_dist=1.0, src_prefix=prefix, dst_prefix=prefix, out=flow)    # noqa: E731
        med, lo, hi = per_call_us(fn, calls, a.repeats, warmup)
        imed, ilo, ihi = per_call_us(nn, calls, a.repeats, warmup)
        count = fn()[2]
        split = kernel_split_us(fn) if a.split else None
        say('%-26s %2d calls a repeat   ops.normals %10.1f (%.1f .. %.1f)   %s   ops.icp(iters = 0) on the same cloud %10.1f '
            '(%.1f .. %.1f)   mean count %.2f, %.4f of the points with three neighbours' % (
                name, calls, med, lo, hi,
                'keys + sort %.1f, search + PCA %.1f (profiled kernel time)' % split if split else 'launch split not measured',
                imed, ilo, ihi, float(count.float().mean()), float((count >= 3).float().mean())))

    # the composition in torch at one cloud: all pairs, top k, gathered neighbours, float32 covariance, eigh
    pc = t(O.scene(one, 90))
    out = torch.empty((3, one), device=dev)

    def composed():
        p = pc.t()
        d = torch.cdist(p, p)
        idx = d.topk(16, dim=1, largest=False).indices
        nb = p[idx]
        c = nb - nb.mean(1, keepdim=True)
        return torch.linalg.eigh(c.transpose(1, 2) @ c)[1][:, :, 0]
    native = lambda: ops.normals(pc, k=16, radius=1.0, out=out)        # noqa: E731
    rows = []
    for _ in range(2):
        rows.append((per_call_us(composed, 10, a.repeats, 3), per_call_us(native, 50, a.repeats, 10)))
    say('')
    say('the torch composition at %d points, k = 16, us per call, two alternating passes:' % one)
    for (c, n_) in rows:
        say('   cdist + topk + gather + linalg.eigh: %10.1f (%.1f .. %.1f)   ops.normals: %8.1f (%.1f .. %.1f)   ratio %.2f' % (
            c + n_ + (c[0] / n_[0],)))

    # the worst case: every point in one cell -- every point compares with every other
    n = 256 if a.small else 8192
    rng = np.random.RandomState(1)
    p1 = t((np.array([[3.2], [0.2], [10.2]]) + rng.uniform(0, 0.6, (3, n))).astype(np.float32))
    out = torch.empty((3, n), device=dev)
    say('')
    for k in (8, 16, 32):
        med, lo, hi = per_call_us(lambda: ops.normals(p1, k=k, radius=1.0, out=out), 10, a.repeats, 3)
        say('all %d points in one cell, k = %2d: %10.1f (%.1f .. %.1f) us per call' % (n, k, med, lo, hi))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
