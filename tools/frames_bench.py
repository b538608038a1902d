#!/usr/bin/env python
"""GPU: time per ops.frames_from_kitti / ops.frames_from_ft3d call (hpl_frames_from_*) -- the table of
profiles/frames_bench.txt.

Shapes: one 375 x 1242 KITTI frame, one 540 x 960 FlyingThings3D frame (near cut -35), and a batch of 16 of each.  The frames
are the tests' generator's (about 70 % of the pixels valid).  Per shape: warm-up calls, then --repeats timings of device events
around --calls back-to-back calls each; the table gives the median, the fastest and the slowest repeat per call.  Beside each,
measured in the same run: the numpy restatement of tests/frames_oracle.py on the host (the median of three runs over the same
frames), and a torch device-to-device copy of as many bytes as the call's inputs and outputs hold together -- the bandwidth
floor of anything that reads the maps once and writes the clouds once (the call reads the maps twice: count, then emit).
--out FILE also writes the table there."""
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


def host_us(fn):
    out = []
    for _ in range(3):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from hplflownet_amd import ops
    import frames_oracle as FO
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    P = FO.read_P('000000')
    shapes = [('KITTI 375 x 1242', 'kitti', 1, 375, 1242), ('FlyingThings3D 540 x 960, near -35', 'ft3d', 1, 540, 960),
              ('KITTI 16 x 375 x 1242', 'kitti', 16, 375, 1242), ('FlyingThings3D 16 x 540 x 960, near -35', 'ft3d', 16, 540, 960)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per call: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up calls'
             % (a.repeats, a.calls, a.warmup), '']
    for name, form, B, H, W in shapes:
        hh, ww, N = [H] * B, [W] * B, B * H * W
        if form == 'kitti':
            frames = [FO.kitti_raw(rng, H, W) for _ in range(B)]
            planes = [torch.from_numpy(np.concatenate([fr[k].reshape((-1,) + fr[k].shape[2:]) for fr in frames])).to(dev) for k in range(3)]
            call = lambda: ops.frames_from_kitti(planes[0], planes[1], planes[2], [P] * B, hh, ww)                  # noqa: E731
            host = lambda: [FO.kitti_frame(*fr, P) for fr in frames]                                               # noqa: E731
            per_pixel = 2 + 2 + 6 + 28
        else:
            frames = [FO.ft3d_raw(rng, H, W) for _ in range(B)]
            planes = [torch.from_numpy(np.concatenate([fr[k].reshape((-1,) + fr[k].shape[2:]) for fr in frames])).to(dev) for k in range(5)]
            call = lambda: ops.frames_from_ft3d(*planes, hh, ww, near=-35.0)                                        # noqa: E731
            host = lambda: [FO.ft3d_frame(*fr, near=-35.0) for fr in frames]                                       # noqa: E731
            per_pixel = 4 + 4 + 8 + 1 + 1 + 28
        med, lo, hi = per_call_us(call, a.calls, a.repeats, a.warmup)
        counts = call()[3].cpu().numpy()
        want = host()
        assert counts.tolist() == [len(w[2]) for w in want]                  # the same correspondences
        hus = host_us(host)
        src = torch.empty(N * per_pixel // 2, dtype=torch.uint8, device=dev)                # read N * per_pixel / 2, write as many
        dst = torch.empty_like(src)
        cmed, clo, chi = per_call_us(lambda: dst.copy_(src), a.calls, a.repeats, a.warmup)
        row = ('%-42s pixels %8d  valid %8d   call %8.1f (%.1f .. %.1f)   %6.2f GB/s of inputs + outputs   numpy on the host %10.0f'
               '   host / call %7.1f   copy of %d bytes a pixel %8.1f (%.1f .. %.1f)   call / copy %5.2f'
               % (name, N, int(counts.sum()), med, lo, hi, N * per_pixel / med * 1e-3, hus, hus / med, per_pixel, cmed, clo, chi,
                  med / cmed))
        lines.append(row)
        print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
