#!/usr/bin/env python
"""GPU: pipelined pairs/s of ragged batched inference (HPLFlowNet, fused lattice builds on a producer thread and a side stream,
one forward per build) on KITTI-like streams whose frames have their own point counts: one table for
profiles/rNN_ragged_sweep.txt.

Streams (N1 = N2 within a frame, frustum pairs):
  uniform  counts uniform in [4096, 8192];
  short3   8192 points, every 3rd frame short (uniform in [3000, 6000], as allow_less_points leaves a frame).
Modes, alternated `--repeats` times in one process (spread reported):
  B1       one pair per build and forward;
  eq8      --batch-size 8 with equal-count grouping (engine.batch_groups: runs of equal counts);
  rg4/rg8  --batch-size 4 / 8 --ragged (engine.ragged_groups, lists through LatticePipeline(ragged=True));
  same8    equal-count batches of 8 pairs of the stream's mean count: the same total points as rg8, for reference."""
import argparse
import collections
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stream_counts(kind, n, seed):
    rng = np.random.RandomState(seed)
    if kind == 'uniform':
        return [int(x) for x in rng.randint(4096, 8193, n)]
    return [int(rng.randint(3000, 6001)) if i % 3 == 2 else 8192 for i in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--streams', default='uniform,short3')
    ap.add_argument('--modes', default='B1,eq8,rg4,rg8,same8')
    ap.add_argument('--pairs', type=int, default=192, help='timed pairs per run (whole groups)')
    ap.add_argument('--warmup', type=int, default=24, help='pairs before the clock starts')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--frames', type=int, default=24, help='distinct frames of a stream (cycled)')
    a = ap.parse_args()
    import hplflownet_amd as H
    from hplflownet_amd.engine import batch_groups, ragged_groups
    from hplflownet_amd.lattice import LatticePipeline
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair
    dev = torch.device('cuda:0')
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True, bcn_use_bias=True,
                                 bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    model = H.HPLFlowNet(args)
    fill_module_(model, 1.0, 'hash')
    model = model.to(dev).eval()
    gen = H.GenerateDataUnsymmetric(args, device=dev, wide_up=model.lattice_hint())
    main_s = torch.cuda.current_stream(dev)

    def frames(counts, seed):
        out = []
        for i, n in enumerate(counts):
            p1, p2, _ = synthetic_pair(n, seed + i)
            out.append((torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev), torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)))
        return out

    def run(pool, mode):
        total = a.warmup + a.pairs
        counts = [(int(pool[i % len(pool)][0].shape[1]),) * 2 for i in range(total)]
        ragged = mode.startswith('rg')
        B = 1 if mode == 'B1' else int(mode[2:]) if ragged or mode.startswith('eq') else int(mode[4:])
        groups = None
        if B > 1:
            groups = ragged_groups(counts, B) if ragged else batch_groups(counts, B)
        side = torch.cuda.Stream(device=dev, priority=-1)
        pipe = LatticePipeline(gen, lambda i: pool[i % len(pool)], 0, total, depth=2, stream=side, native=True, threaded=True,
                               batch=B, groups=groups, ragged=ragged)
        sizes = [len(g) for g in groups] if groups is not None else [1] * total
        keep = collections.deque()
        done, t0, first = 0, None, 0
        try:
            with torch.no_grad():
                for k in range(len(sizes)):
                    if t0 is None and done >= a.warmup:
                        torch.cuda.synchronize()
                        t0, first = time.perf_counter(), done
                    (i, (p1, p2)), lat, ev = pipe.get()
                    main_s.wait_event(ev)
                    if isinstance(p1, list) or p1.dim() == 3:
                        flow = model(p1, p2, lat)
                    else:
                        flow = model(p1[None], p2[None], lat)
                    fin = torch.cuda.Event()
                    fin.record(main_s)
                    keep.append((lat, p1, p2, flow, fin))
                    while len(keep) > 3:
                        keep.popleft()[-1].synchronize()
                    done += sizes[k]
            torch.cuda.synchronize()
        finally:
            pipe.close()
        return (done - first) / (time.perf_counter() - t0), len(sizes) / float(total)

    modes = a.modes.split(',')
    print('# python tools/ragged_sweep.py --pairs %d --warmup %d --repeats %d --frames %d   (HPLFlowNet, hash fill, frustum pairs; '
          'one MI355X; pipelined: fused lattice builds on a producer thread + side stream, one forward per build)'
          % (a.pairs, a.warmup, a.repeats, a.frames))
    print('%-8s %-6s %10s %10s %10s %9s %14s' % ('stream', 'mode', 'pairs/s', 'min', 'max', 'x B1', 'builds/pair'))
    for si, kind in enumerate(a.streams.split(',')):
        counts = stream_counts(kind, a.frames, 7 + si)
        pool = frames(counts, 500 + 100 * si)
        mean_n = int(round(np.mean(counts)))
        same = frames([mean_n] * a.frames, 900 + 100 * si)
        res = collections.OrderedDict((m, []) for m in modes)
        per = {}
        for r in range(a.repeats):
            for m in modes:
                rate, bp = run(same if m.startswith('same') else pool, m)
                res[m].append(rate)
                per[m] = bp
        base = float(np.median(res['B1'])) if res.get('B1') else None
        for m, rates in res.items():
            med = float(np.median(rates))
            print('%-8s %-6s %10.1f %10.1f %10.1f %9s %14.3f' % (kind, m, med, min(rates), max(rates),
                                                               '%.2f' % (med / base) if base else '-', per[m]))
        print('# %s: mean points per frame %d (same8 runs 8 x %d)' % (kind, mean_n, mean_n))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
