#!/usr/bin/env python
"""GPU: time per ops.icp call (hpl_icp) at the defaults (max_dist 1.0, tau 0.3, tol 0, from identity) -- the
table of profiles/icp_bench.txt.

Shapes: B = 1 x N = M = 8 192 (one sampled pair), B = 16 x 8 192, B = 1 x N = M = 450 000 (a dense frame); the scene is the
tests' (tests/icp_oracle.py: one rigid motion, 10 % movers, 10 % clutter, 1 cm noise, uniform in a 30 x 4 x 33 m box, so the
450 000-point pair holds about 114 points per 1 m cell and a query compares with about 3 000 candidates -- denser than a lidar
frame away from the sensor).  Per shape and for iters = 1 and 30: warm-up calls, then --repeats timings of device events around
back-to-back calls; the table gives the median, the fastest and the slowest repeat per call, and the rounds the pairs ran
before their bitwise fixpoints (later rounds of a finished pair return at once).

One round composed from the older ops at 8 192 -- the moved cloud by torch, ops.knn_interpolate(k = 1) for the brute-force
match, ops.rigid_fit(iters = 0) for the solve; no max_dist gate, no robust weight -- against ops.icp(iters = 1): the ratio is
reported, it is not a pass bar.  The worst case for the grid: all points of both clouds in one cell.  --out FILE also writes
the table there."""
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
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--metric', default='point', choices=['point', 'plane'],
                    help='plane: instead of the tables above, point-to-plane (DESIGN.md §29) against point-to-point on a pair whose '
                         'clouds are sampled independently from the same surfaces: a round, a run to the fixpoint, rounds, error')
    ap.add_argument('--small', action='store_true', help='tiny shapes: a rehearsal of the script, not a measurement')
    a = ap.parse_args()
    from hplflownet_amd import ops
    import icp_oracle as O
    dev = torch.device('cuda:0')
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
    one, big = (512, 2000) if a.small else (8192, 450000)
    # (name, counts, calls, warm-up calls)
    shapes = [('B = 1 x N = M = %d' % one, [one], 50, 10), ('B = 16 x N = M = %d' % one, [one] * 16, 20, 5),
              ('B = 1 x N = M = %d' % big, [big], 3, 2)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per ops.icp call (max_dist 1.0, tau 0.3, tol 0, from identity): median (fastest .. slowest) of %d repeats of '
             'back-to-back calls' % a.repeats, '']

    def say(row):
        lines.append(row)
        print(row, flush=True)
    if a.metric == 'plane':
        import icp_plane_oracle as Q
        say('src and dst sampled independently from the same surfaces (tests/icp_plane_oracle.pair), dst moved by the scene\'s motion;')
        say('normals of dst by ops.normals(k = 16, radius = 1), timed apart; R / t: largest entry off the true motion')
        for n, calls, warmup in ((one, 50, 10), (big, 3, 2)):
            src, dst = (t(x) for x in Q.pair(n, 7))
            out = torch.empty((n, 3), device=dev)
            nrm = ops.normals(dst, k=16, radius=1.0)[0]
            med, lo, hi = per_call_us(lambda: ops.normals(dst, k=16, radius=1.0), calls, a.repeats, warmup)
            say('N = M = %d: ops.normals(dst) %.1f (%.1f .. %.1f)' % (n, med, lo, hi))
            for metric, kw in (('point', {}), ('plane', dict(metric='plane', dst_normal=nrm))):
                row = '   %-5s' % metric
                for iters in (0, 1, 30):
                    fn = lambda: ops.icp(src, dst, iters=iters, out=out, **kw)       # noqa: E731
                    med, lo, hi = per_call_us(fn, calls, a.repeats, warmup)
                    row += '   iters = %2d: %10.1f (%.1f .. %.1f)' % (iters, med, lo, hi)
                R, tt, stats, _ = fn()
                row += '   rounds run %2d, R off by %.3g, t by %.3g m' % (
                    int(stats[0, 5]), float(np.abs(R[0].cpu().numpy() - O.TRUE_R).max()), float(np.abs(tt[0].cpu().numpy() - O.TRUE_T).max()))
                say(row)
        if a.out:
            with open(a.out, 'w') as fd:
                fd.write('\n'.join(lines) + '\n')
        return
    for name, counts, calls, warmup in shapes:
        parts = [O.scene(n, 90 + i) for i, n in enumerate(counts)]
        src, dst = t(np.concatenate([x[0] for x in parts], 1)), t(np.concatenate([x[1] for x in parts], 1))
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        out = torch.empty((src.shape[1], 3), device=dev)
        row = '%-28s %d calls a repeat' % (name, calls)
        for iters in (1, 30):
            fn = lambda: ops.icp(src, dst, iters=iters, src_prefix=prefix, dst_prefix=prefix, out=out)       # noqa: E731
            med, lo, hi = per_call_us(fn, calls, a.repeats, warmup)
            stats = fn()[2]
            row += '   iters = %2d (%2d launches + sort): %10.1f (%.1f .. %.1f), rounds run %.1f' % (
                iters, 2 * iters + 3, med, lo, hi, float(stats[:, 5].mean()))
        row += '   matched %.4f' % float(stats[:, 1].mean())
        say(row)

    # one round from the older ops against ops.icp(iters = 1), alternating in the same process
    src, dst = (t(x) for x in O.scene(one, 90))
    R = torch.eye(3, device=dev)
    tt = torch.zeros(3, 1, device=dev)
    vals = dst.t().contiguous()
    out = torch.empty((one, 3), device=dev)

    def composed():
        y = R @ src + tt
        q = ops.knn_interpolate(dst, vals, y, k=1)                    # the nearest dst point's coordinates, [N, 3]
        return ops.rigid_fit(src, q.t() - src, iters=0, out=out)
    native = lambda: ops.icp(src, dst, iters=1, out=out)               # noqa: E731
    rows = []
    for _ in range(2):
        rows.append((per_call_us(composed, 50, a.repeats, 10), per_call_us(native, 50, a.repeats, 10)))
    say('')
    say('one round at N = M = %d, us per call, two alternating passes:' % one)
    for (c, n_) in rows:
        say('   torch move + ops.knn_interpolate(k = 1) + ops.rigid_fit(iters = 0): %8.1f (%.1f .. %.1f)   ops.icp(iters = 1): %8.1f '
            '(%.1f .. %.1f)   ratio %.2f' % (c + n_ + (c[0] / n_[0],)))

    # the worst case: every point of both clouds in one cell -- every query compares with every dst point
    n = 256 if a.small else 8192
    rng = np.random.RandomState(1)
    d1 = t((np.array([[3.2], [0.2], [10.2]]) + rng.uniform(0, 0.6, (3, n))).astype(np.float32))
    s1 = t((np.array([[3.2], [0.2], [10.2]]) + rng.uniform(0, 0.6, (3, n))).astype(np.float32))
    out = torch.empty((n, 3), device=dev)
    say('')
    for iters in (0, 1):
        med, lo, hi = per_call_us(lambda: ops.icp(s1, d1, iters=iters, out=out), 10, a.repeats, 3)
        say('all %d + %d points in one cell, iters = %d (%d matching passes): %10.1f (%.1f .. %.1f) us per call' % (
            n, n, iters, iters + 1, med, lo, hi))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
