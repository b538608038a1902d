#!/usr/bin/env python
"""GPU: time per ops.fps call (hpl_fps) -- the table of profiles/fps_bench.txt.

Shapes (n points, m samples): (8 192, 1 024), (32 768, 8 192), (capacity, 8 192) with the resident path's capacity, (450 000,
8 192) -- a whole frame down to the network's size --, and ragged batches of 16 clouds; uniform clouds, three attribute channels
ride along.  Each shape on both kernel paths where the resident one takes it.  Then the crossover: both paths over n at m =
1 024, which is where `auto` would have to switch if the rounds path won below the capacity.  Per row: warm-up calls, then
--repeats timings of device events around --calls back-to-back calls each; the table gives the median, the fastest and the
slowest repeat per call, and the time per round.

The comparator is a torch loop on the same device, m rounds of (gather the sample, d2, minimum, argmax) with no host
synchronisation inside -- what a user writes without this op; its indices are checked against the call's.  A ragged batch
costs it one loop per cloud.  --out FILE also writes the table there; --only-resident N,M times that one shape on the resident
path alone (for comparing builds of the kernel with other workgroup shapes, loaded through HPL_LIB)."""
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


def torch_fps(pc, m):
    """m rounds by torch alone, from point 0: the indices (m,) int64.  Nothing is read back inside."""
    D = torch.full((pc.shape[1],), float('inf'), device=pc.device)
    idx = torch.empty(m, dtype=torch.int64, device=pc.device)
    s = torch.zeros(1, dtype=torch.int64, device=pc.device)
    for j in range(m):
        idx[j:j + 1] = s
        d = pc - pc.index_select(1, s)
        D = torch.minimum(D, (d * d).sum(dim=0))
        s = torch.argmax(D).view(1)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-resident', action='append', default=[], metavar='N,M')
    a = ap.parse_args()
    from hplflownet_amd import ops
    import fps_oracle as FO
    dev = torch.device('cuda:0')
    cap = ops.fps_resident_capacity()
    lines = ['%s on %s; resident capacity %d points' % (os.path.basename(__file__), torch.cuda.get_device_name(0), cap),
             'us per call: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up call(s); 3 attribute '
             'channels' % (a.repeats, a.calls, a.warmup), '']

    def emit(row):
        lines.append(row)
        print(row, flush=True)

    def clouds(counts, seed):
        pc = torch.from_numpy(np.concatenate([FO.cloud(n, seed + i, extent=40.0) for i, n in enumerate(counts)], axis=1)).to(dev)
        return pc, torch.randn((3, pc.shape[1]), device=dev), np.concatenate([[0], np.cumsum(counts)]).tolist()

    def time_path(pc, attr, prefix, m, path):
        med, lo, hi = per_call_us(lambda: ops.fps(pc, m, attr, prefix=prefix, path=path), a.calls, a.repeats, a.warmup)
        return med, '%-8s %10.1f (%.1f .. %.1f)  %6.2f us a round' % (path, med, lo, hi, med / m)

    if a.only_resident:
        for spec in a.only_resident:
            n, m = (int(x) for x in spec.split(','))
            pc, attr, prefix = clouds([n], 1)
            emit('n = %d, m = %d   %s' % (n, m, time_path(pc, attr, prefix, m, 'resident')[1]))
    else:
        rng = np.random.RandomState(0)
        ragged = lambda total, least: [int(x) for x in rng.multinomial(total - 16 * least, np.ones(16) / 16) + least]     # noqa: E731
        shapes = [('B = 1 x n = 8192', [8192], 1024), ('B = 1 x n = 32768', [32768], 8192), ('B = 1 x n = capacity', [cap], 8192),
                  ('B = 1 x n = 450000', [450000], 8192), ('ragged B = 16, 100191 points', ragged(100191, 2048), 1024),
                  ('ragged B = 16, 1600000 points', ragged(1600000, 50000), 1024)]
        for name, counts, m in shapes:
            pc, attr, prefix = clouds(counts, 70)
            cells, meds = [], {}
            for path in ('resident', 'rounds'):
                if path == 'resident' and max(counts) > cap:
                    cells.append('%-8s %s' % (path, 'does not take it'))
                    continue
                meds[path], text = time_path(pc, attr, prefix, m, path)
                cells.append(text)
            ours = ops.fps(pc, m, attr, prefix=prefix)[2]
            tm = max(1, a.calls // 3)

            def loop():
                return [torch_fps(pc[:, prefix[b]:prefix[b + 1]], m) for b in range(len(counts))]
            tmed, tlo, thi = per_call_us(loop, tm, min(a.repeats, 3), 1)
            same = all(torch.equal(t, ours[b].long()) for b, t in enumerate(loop()))
            emit('%-32s m %5d   %s   %s   torch loop %11.1f (%.1f .. %.1f)  %6.2f us a round   torch / call (the path auto takes) %6.1f   same indices: %s'
                 % (name, m, cells[0], cells[1], tmed, tlo, thi, tmed / (m * len(counts)), tmed / meds.get('resident', meds['rounds']), same))
        emit('')
        emit('crossover at m = 1024 (the path auto would have to leave below the capacity, if any):')
        for n in (1024, 2048, 4096, 8192, cap // 2 + 1, cap):
            pc, attr, prefix = clouds([n], 5)
            r1, t1 = time_path(pc, attr, prefix, 1024, 'resident')
            r2, t2 = time_path(pc, attr, prefix, 1024, 'rounds')
            emit('n = %6d   %s   %s   rounds / resident %5.2f' % (n, t1, t2, r2 / r1))
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
