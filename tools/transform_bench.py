#!/usr/bin/env python
"""GPU: the data transforms on the host (data.Augmentation / ProcessData, numpy) against the device (data.DeviceAugmentation /
DeviceProcessData, hpl_transform_pair), per sample and end to end -- one table for profiles/rNN_transform_bench.txt
(DESIGN.md §15).

Part 1, per sample: the published settings (engine.AUG_TOGETHER / AUG_PC2 / DATA_PROCESS, num_points 8192; ProcessData with
the evaluation protocol's allow_less_points) on synthetic frames of M points, M in --sizes.  Host: median of --host-reps
calls.  Device: median of --reps calls after 3 warm-up calls; a call is the pinned-stage copy of the raw numpy clouds, the
launches and the one count read-back (the call returns with its outputs on the device).

Part 2, end to end: `engine --dataset FlyingThings3DSubset` trains --epochs epochs (HPLFlowNet, hash init) on a synthetic
tree of --frames training samples of --points-per-frame points each (a few distinct frames, the directories linked to
them), with and without --device-transforms, for each --train-batch-size in --batch-sizes.  pairs/s of the last epoch:
its training samples over the time between the log lines of the two last epochs (it includes one validation pair)."""
import argparse
import builtins
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def per_sample(sizes, host_reps, reps, dev):
    from hplflownet_amd import data as D
    from hplflownet_amd.engine import AUG_PC2, AUG_TOGETHER, DATA_PROCESS
    from hplflownet_amd.synthetic import synthetic_pair
    rows = []
    for M in sizes:
        pc1, pc2, _ = synthetic_pair(M, 5)
        kinds = (('Augmentation', D.Augmentation(AUG_TOGETHER, AUG_PC2, DATA_PROCESS, 8192, False, seed=1),
                  D.DeviceAugmentation(AUG_TOGETHER, AUG_PC2, DATA_PROCESS, 8192, False, seed=1, device=dev)),
                 ('ProcessData', D.ProcessData(DATA_PROCESS, 8192, True, seed=0),
                  D.DeviceProcessData(DATA_PROCESS, 8192, True, seed=0, device=dev)))
        for name, host, device in kinds:
            th = []
            for _ in range(host_reps):
                t = time.perf_counter()
                host((pc1, pc2))
                th.append(time.perf_counter() - t)
            for _ in range(3):
                device((pc1, pc2))
            torch.cuda.synchronize()
            td = []
            for _ in range(reps):
                t = time.perf_counter()
                out = device((pc1, pc2))
                td.append(time.perf_counter() - t)
            assert out[0] is not None and tuple(out[0].shape) == (3, 8192)
            rows.append((M, name, 1e3 * np.median(th), 1e3 * np.median(td), 1e3 * min(td), 1e3 * max(td)))
    return rows


def make_tree(root, frames, points, distinct=4):
    from hplflownet_amd.synthetic import synthetic_pair
    src = os.path.join(root, 'frames')
    flip = np.array([-1, 1, -1], np.float32)
    for k in range(distinct):
        d = os.path.join(src, str(k))
        os.makedirs(d)
        pc1, pc2, _ = synthetic_pair(points, 100 + k)
        np.save(os.path.join(d, 'pc1.npy'), pc1 * flip)
        np.save(os.path.join(d, 'pc2.npy'), pc2 * flip)
    for split, count in (('train', 4 * frames), ('val', 4)):          # the reader takes every 4th directory
        for i in range(count):
            d = os.path.join(root, 'FlyingThings3D_subset_processed_35m', split, '%07d' % i)
            os.makedirs(d)
            for nm in ('pc1.npy', 'pc2.npy'):
                os.symlink(os.path.join(src, str(i % distinct), nm), os.path.join(d, nm))


def train_rate(root, frames, epochs, B, device_transforms):
    from hplflownet_amd import engine
    argv = ['--points', '8192', '--epochs', str(epochs), '--dataset', 'FlyingThings3DSubset', '--data-root', root,
            '--train-batch-size', str(B)] + (['--device-transforms'] if device_transforms else [])
    stamps = []
    real = builtins.print

    def grab(*a, **k):
        if a and str(a[0]).startswith('epoch'):
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
    builtins.print = grab
    try:
        engine.main(argv)
    finally:
        builtins.print = real
    return frames / (stamps[-1] - stamps[-2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='100000,250000,450000')
    ap.add_argument('--host-reps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=32, help='training samples per epoch')
    ap.add_argument('--points-per-frame', type=int, default=250000)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--batch-sizes', default='1,8')
    ap.add_argument('--skip-train', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    print('# python tools/transform_bench.py %s' % ' '.join(sys.argv[1:]))
    print('# per sample, ms (num_points 8192; host: median of %d, device: median / min / max of %d incl. copy and read-back)'
          % (a.host_reps, a.reps))
    print('%-8s %-13s %10s %10s %10s %10s %8s' % ('M', 'transform', 'host', 'device', 'dev min', 'dev max', 'x'))
    for M, name, h, d, lo, hi in per_sample([int(s) for s in a.sizes.split(',')], a.host_reps, a.reps, dev):
        print('%-8d %-13s %10.2f %10.3f %10.3f %10.3f %8.1f' % (M, name, h, d, lo, hi, h / d))
    sys.stdout.flush()
    if a.skip_train:
        return
    root = tempfile.mkdtemp(prefix='hpl_tfbench_')
    try:
        make_tree(root, a.frames, a.points_per_frame)
        print('# end to end: engine training, HPLFlowNet, %d samples of %d points per epoch, pairs/s of epoch %d of %d'
              % (a.frames, a.points_per_frame, a.epochs, a.epochs))
        print('%-4s %14s %14s %8s' % ('B', 'host pairs/s', 'device pairs/s', 'x'))
        for B in [int(b) for b in a.batch_sizes.split(',')]:
            h = train_rate(root, a.frames, a.epochs, B, False)
            d = train_rate(root, a.frames, a.epochs, B, True)
            print('%-4d %14.2f %14.2f %8.2f' % (B, h, d, d / h))
            sys.stdout.flush()
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
