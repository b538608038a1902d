#!/usr/bin/env python
"""GPU: time per ops.voxel_downsample call (hpl_voxel_downsample) -- the table of profiles/voxel_bench.txt.

Shapes: n = 8 192 at voxel 0.1 (a sampled cloud), a ragged B = 16 of 100 191 points at 0.1, n = 450 000 (a whole frame) at
0.1 and 0.3, and 450 000 points in ONE voxel (the skewed case: one wave owns every addition).  The scenes are the tests'
generator's at lidar ranges; three attribute channels ride along, mode centroid.  Per shape: warm-up calls, then --repeats
timings of device events around --calls back-to-back calls each; the table gives the median, the fastest and the slowest repeat
per call.  Beside each: the radix sort alone on the call's own keys and bits (libhplbcl_diag's hpl_diag_sort_pairs64 -- the
floor of any sort-based voxel grid) with the call's multiple of it, and a torch composition of the same result on the same
device -- torch.unique(cells, dim=0, return_inverse=True) and index_add_ in float64 for the coordinate and attribute means
(no representative, no ordered sum) -- with its multiple of the call.  --out FILE also writes the table there."""
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


def keys_of(pc, prefix, voxel):
    """The call's 64-bit keys (cloud digit, three biased 19-bit cells; every point of the scenes is valid) and their bits."""
    cell = torch.floor(pc.double() * (1.0 / float(np.float32(voxel)))).long() + (1 << 18)
    cloud = torch.bucketize(torch.arange(pc.shape[1], device=pc.device), torch.tensor(prefix[1:], device=pc.device), right=True)
    key = (cloud << 57) | (cell[0] << 38) | (cell[1] << 19) | cell[2]
    return key, 57 + max(1, (len(prefix) - 2).bit_length())


def torch_composition(pc, attr, prefix, voxel):
    """The means by torch alone: one row per distinct (cloud, cell), float64 sums by index_add_ (atomics: no fixed order)."""
    cell = torch.floor(pc.double() * (1.0 / float(np.float32(voxel)))).long()
    cloud = torch.bucketize(torch.arange(pc.shape[1], device=pc.device), torch.tensor(prefix[1:], device=pc.device), right=True)
    rows, inv = torch.unique(torch.cat([cloud[None], cell]).t(), dim=0, return_inverse=True)
    V = rows.shape[0]
    vals = torch.cat([pc, attr]).double()
    sums = torch.zeros((vals.shape[0], V), dtype=torch.float64, device=pc.device).index_add_(1, inv, vals)
    cnt = torch.zeros(V, dtype=torch.float64, device=pc.device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float64))
    return (sums / cnt).float(), inv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from hplflownet_amd import _lib, ops
    import voxel_oracle as VO
    dev = torch.device('cuda:0')
    diag = _lib.load_diag()
    rng = np.random.RandomState(0)
    ragged = [int(x) for x in rng.multinomial(100191 - 16 * 2048, np.ones(16) / 16) + 2048]
    shapes = [('B = 1 x n = 8192, voxel 0.1', [8192], 0.1), ('ragged B = 16, 100191 points, voxel 0.1', ragged, 0.1),
              ('B = 1 x n = 450000, voxel 0.1', [450000], 0.1), ('B = 1 x n = 450000, voxel 0.3', [450000], 0.3),
              ('B = 1 x n = 450000 in ONE voxel', [450000], 1000.0)]
    lines = ['%s on %s' % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             'us per call: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up calls; 3 attribute '
             'channels, mode centroid' % (a.repeats, a.calls, a.warmup), '']
    for name, counts, voxel in shapes:
        host = np.concatenate([VO.scene(n, 70 + i) for i, n in enumerate(counts)], axis=1)
        if voxel >= 1000.0:
            host = np.abs(host) + np.float32(1.0)             # every point inside the cell (0, 0, 0)
        pc = torch.from_numpy(host).to(dev)
        attr = torch.randn((3, pc.shape[1]), device=dev)
        prefix = np.concatenate([[0], np.cumsum(counts)]).tolist()
        med, lo, hi = per_call_us(lambda: ops.voxel_downsample(pc, attr, voxel=voxel, prefix=prefix), a.calls, a.repeats, a.warmup)
        out = ops.voxel_downsample(pc, attr, voxel=voxel, prefix=prefix)
        stats = out[5].cpu().numpy()
        V, longest = int(stats[:, 0].sum()), int(out[2].max())
        # the sort alone, on the same keys over the same bits
        key, bits = keys_of(pc, prefix, voxel)
        N = key.numel()
        val = torch.arange(N, dtype=torch.int32, device=dev)
        key_out, val_out = torch.empty_like(key), torch.empty_like(val)
        need = diag.hpl_diag_sort_pairs64(None, None, None, None, N, bits, None, 0, None)
        temp = torch.empty(max(int(need), 1), dtype=torch.uint8, device=dev)

        def sort_alone():
            rc = diag.hpl_diag_sort_pairs64(key.data_ptr(), key_out.data_ptr(), val.data_ptr(), val_out.data_ptr(), N, bits,
                                            temp.data_ptr(), temp.numel(), _lib.stream())
            assert rc == 0, rc
        smed, slo, shi = per_call_us(sort_alone, a.calls, a.repeats, a.warmup)
        assert int((key_out[1:] != key_out[:-1]).sum()) + 1 == V          # the same voxels
        # the torch composition
        tmed, tlo, thi = per_call_us(lambda: torch_composition(pc, attr, prefix, voxel), max(1, a.calls // 10), a.repeats, 2)
        means, inv = torch_composition(pc, attr, prefix, voxel)
        assert means.shape[1] == V
        err = float((means[:, inv] - torch.cat([out[0], out[1]])[:, out[4].long()]).abs().max())
        row = ('%-42s points %7d  voxels %7d  longest run %6d   call %9.1f (%.1f .. %.1f)   sort alone (%d bits) %8.1f (%.1f .. %.1f)'
               '   call / sort %5.2f   torch.unique + index_add_ %10.1f (%.1f .. %.1f)   torch / call %6.2f   max |torch - call| %.2g'
               % (name, N, V, longest, med, lo, hi, bits, smed, slo, shi, med / smed, tmed, tlo, thi, tmed / med, err))
        lines.append(row)
        print(row, flush=True)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
