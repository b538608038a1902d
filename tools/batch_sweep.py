#!/usr/bin/env python
"""GPU: pipelined pairs/s of batched inference (HPLFlowNet, fused lattice builds of B pairs on a producer thread and a
side stream, one batched forward per build) over B x N: one table for profiles/rNN_batch_sweep.txt.

The B = 1 and B = 8 runs of every N alternate `--repeats` times in the same process (spread reported); the other batch
sizes run once.  Per run: pairs/s over `--pairs` pairs after `--warmup` pairs and the range-guard second passes of the
fp16-pair kernel (hpl_plan_guard_trips).  (No launch leaves the fp16-pair form for lack of split-K scratch at any M: the
split count keeps splits x row tiles <= 256, so its partial tiles never exceed the executor's 64 MiB -- DESIGN.md.)"""
import argparse
import collections
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--points', default='500,1024,2048,8192')
    ap.add_argument('--batches', default='1,2,4,8,16')
    ap.add_argument('--pairs', type=int, default=256, help='timed pairs per run (rounded up to whole batches)')
    ap.add_argument('--warmup', type=int, default=32, help='pairs before the clock starts')
    ap.add_argument('--repeats', type=int, default=3, help='alternating B = 1 / B = 8 runs per N')
    a = ap.parse_args()
    import hplflownet_amd as H
    from hplflownet_amd.lattice import LatticePipeline
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair
    dev = torch.device('cuda:0')
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True, bcn_use_bias=True,
                                 bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    model = H.HPLFlowNet(args)
    fill_module_(model, 1.0, 'hash')
    model = model.to(dev).eval()
    gen = H.GenerateDataUnsymmetric(args, device=dev, wide_up=model.lattice_hint())
    plan = model.forward_plan()
    main_s = torch.cuda.current_stream(dev)

    def run(n, B, pool):
        total = a.warmup + a.pairs
        total = (total + B - 1) // B * B
        side = torch.cuda.Stream(device=dev, priority=-1)
        pipe = LatticePipeline(gen, lambda i: pool[i % len(pool)], 0, total, depth=2, stream=side, native=True, threaded=True,
                               batch=B)
        keep = collections.deque()
        trips0 = plan.guard_trips()
        done, t0, first = 0, None, 0
        try:
            with torch.no_grad():
                while done < total:
                    if t0 is None and done >= a.warmup:
                        torch.cuda.synchronize()
                        t0, first = time.perf_counter(), done
                    (i, (p1, p2)), lat, ev = pipe.get()
                    main_s.wait_event(ev)
                    flow = model(p1, p2, lat) if p1.dim() == 3 else model(p1[None], p2[None], lat)
                    fin = torch.cuda.Event()
                    fin.record(main_s)
                    keep.append((lat, p1, p2, flow, fin))
                    while len(keep) > 3:
                        keep.popleft()[-1].synchronize()
                    done += B if p1.dim() == 3 else 1
            torch.cuda.synchronize()
        finally:
            pipe.close()
        dt = time.perf_counter() - t0
        return (done - first) / dt, plan.guard_trips() - trips0

    print('# python tools/batch_sweep.py --pairs %d --warmup %d --repeats %d   (HPLFlowNet, hash fill, frustum pairs; one MI355X;'
          ' pipelined: batched fused lattice builds on a producer thread + side stream, one batched forward per build)'
          % (a.pairs, a.warmup, a.repeats))
    print('%-7s %-4s %10s %10s %10s %9s %12s' % ('N', 'B', 'pairs/s', 'min', 'max', 'x B=1', 'guard trips'))
    for n in [int(x) for x in a.points.split(',')]:
        pool = []
        for s in range(16):
            p1, p2, _ = synthetic_pair(n, 100 + s)
            pool.append((torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev), torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)))
        res = collections.OrderedDict((B, []) for B in [int(x) for x in a.batches.split(',')])
        extra = collections.OrderedDict()
        for r in range(a.repeats):            # B = 1 and B = 8 alternate
            for B in (1, 8):
                if B in res:
                    rate, g = run(n, B, pool)
                    res[B].append(rate)
                    extra[B] = extra.get(B, 0) + g
        for B in res:
            if not res[B]:
                rate, g = run(n, B, pool)
                res[B].append(rate)
                extra[B] = g
        base = float(np.median(res[1])) if res.get(1) else None
        for B, rates in res.items():
            med = float(np.median(rates))
            print('%-7d %-4d %10.1f %10.1f %10.1f %9s %12d' % (n, B, med, min(rates), max(rates),
                                                             '%.2f' % (med / base) if base else '-', extra[B]))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
