#!/usr/bin/env python
"""GPU: time per ops.selfsup_loss call with gradient (hpl_selfsup_loss) at k = 8 -- the table of
profiles/selfsup_bench.txt.

Shapes: B = 1 x N1 = N2 = 8 192 (one sampled pair), a ragged B = 16 with counts in [4 096, 8 192], and a skewed pair of
8 192 points whose whole pc2 sits next to ONE warped point (that point's incoming list is the cloud).  The clouds are the
synthetic pairs of the tests (synthetic.synthetic_pair), the flow their ground truth plus 5 cm noise.  Per shape: warm-up
calls, then --repeats timings of device events around --calls back-to-back calls each; the table gives the median, the
fastest and the slowest repeat per call, with and without the gradient.  --train-step also times one autograd training step
of HPLFlowNet at N = 8 192 (Trainer(native_step=False)) with the supervised loss and with this one, alternating, the lattice
built once outside the timing: what the loss costs next to the step it belongs to.  --out FILE also writes the table there."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--train-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from hplflownet_amd import engine, ops
    from hplflownet_amd.synthetic import synthetic_pair
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    shapes = [('B = 1 x N = 8192', [8192], False), ('ragged B = 16, N_b in [4096, 8192]', [int(x) for x in rng.randint(4096, 8193, 16)], False),
              ('skewed B = 1 x N = 8192', [8192], True)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per ops.selfsup_loss call, k = %d: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up calls'
             % (a.k, a.repeats, a.calls, a.warmup), '']
    for name, counts, skew in shapes:
        xs, fs, qs = [], [], []
        for i, n in enumerate(counts):
            pc1, pc2, sf = synthetic_pair(n, 90 + i)
            f = (sf + np.random.RandomState(i).normal(0, 0.05, sf.shape)).astype(np.float32)
            if skew:
                pc2 = ((pc1 + f)[100:101] + np.random.RandomState(1).normal(0, 0.01, pc2.shape)).astype(np.float32)
            xs.append(pc1.T)
            fs.append(f)
            qs.append(pc2.T)
        t = lambda parts, ax: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, ax), dtype=np.float32)).to(dev)     # noqa: E731
        x, flow, q = t(xs, 1), t(fs, 0), t(qs, 1)                       # the flow as the models return it: point-major rows
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        out = torch.empty((x.shape[1], 3), device=dev)
        row = '%-38s points %7d' % (name, x.shape[1])
        for grad in (True, False):
            med, lo, hi = per_call_us(lambda: ops.selfsup_loss(x, flow, q, a.k, 1.0, 1.0, prefix, prefix, need_grad=grad,
                                                               out=out if grad else None), a.calls, a.repeats, a.warmup)
            row += '   %s: %8.1f (%.1f .. %.1f)' % ('loss + gradient' if grad else 'loss alone', med, lo, hi)
        loss, _, _, nn21, _ = ops.selfsup_loss(x, flow, q, a.k, 1.0, 1.0, prefix, prefix, return_neighbors=True)
        row += '   largest Chamfer in-degree %d   L of pair 0 %.5f' % (int(torch.bincount(nn21[nn21 >= 0]).max()), float(loss[0, 0]))
        lines.append(row)
        print(row, flush=True)
    if a.train_step:
        pc1, pc2, sf = (torch.from_numpy(np.ascontiguousarray(t.T)).to(dev) for t in synthetic_pair(8192, 0))
        trs = {name: engine.Trainer('HPLFlowNet', dev, init='hash', native_step=False, loss=name) for name in ('epe3d', 'selfsup')}
        lats = {name: tr._single_lattice(pc1, pc2) for name, tr in trs.items()}
        res = {name: [] for name in trs}
        for rnd in range(4):                                            # alternating; the first round warms up
            for name, tr in trs.items():
                med, lo, hi = per_call_us(lambda: tr.train_step(pc1, pc2, sf, lats[name]), 5, 3, 2 if rnd == 0 else 0)
                if rnd:
                    res[name].append(med)
        lines.append('')
        for name in trs:
            row = 'autograd training step, HPLFlowNet N = 8192, loss %-8s us per step, medians of 3 alternating rounds: %s' % (
                name, ' '.join('%.0f' % v for v in res[name]))
            lines.append(row)
            print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
