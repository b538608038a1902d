#!/usr/bin/env python
"""GPU: time per ops.render_maps / ops.maps_to_kitti call (hpl_render_maps, hpl_maps_to_kitti) -- the table of
profiles/render_bench.txt.

Shapes: one sampled cloud of 8 192 points into 375 x 1 242, one dense frame (every valid pixel of a generated KITTI frame, about
70 % of 465 750, back-projected by ops.frames_from_kitti), a batch of 16 such frames, and 65 536 points that all fall into one
pixel (the contended case); each at footprints 0 and 1.  Per shape: warm-up calls, then --repeats timings of device events
around --calls back-to-back calls each; the table gives the median, the fastest and the slowest repeat per call.  Beside each,
measured in the same run: a torch composition of the same z-buffer (project, pack (bits(zc) << 32) | index into int64 keys,
scatter_reduce(..., 'amin') once per footprint offset, resolve) and a torch device-to-device copy of as many bytes as the call
reads and writes -- the bandwidth floor.  The library honours HPL_LIB: run the tool again with a build of csrc/render.hip made
with -DHPL_RENDER_NO_SKIP to time the splat without its look before the atomic.  --out FILE also writes the table there."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from frames_bench import per_call_us  # noqa: E402


def torch_zbuffer(pc, cam, H, W, r, near=1e-3):
    """The composition a user would write: winner and depth of ONE cloud (3, n) in torch ops."""
    f, cx, cy, kx, ky, kz = cam
    X, Y, Z = pc[0], pc[1], pc[2]
    zc = Z + kz
    u = ((X * f + cx * Z) + kx) / zc
    v = ((Y * f + cy * Z) + ky) / zc
    ru, rv = torch.round(u), torch.round(v)
    inside = torch.isfinite(pc).all(dim=0) & (zc >= near) & (ru >= 0) & (ru <= W - 1) & (rv >= 0) & (rv <= H - 1)
    idx = torch.nonzero(inside).squeeze(1)
    j, i = ru[idx].long(), rv[idx].long()
    key = (zc[idx].view(torch.int32).long() << 32) | idx
    zbuf = torch.full((H * W,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=pc.device)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ii, jj = i + dy, j + dx
            ok = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
            zbuf.scatter_reduce_(0, (ii * W + jj)[ok], key[ok], 'amin')
    covered = zbuf != torch.iinfo(torch.int64).max
    winner = torch.where(covered, zbuf & 0xffffffff, torch.full_like(zbuf, -1)).int()
    depth = torch.where(covered, (zbuf >> 32).int().view(torch.float32), torch.zeros((), device=pc.device))
    return winner, depth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from hplflownet_amd import ops
    import frames_oracle as FO
    import render_oracle as RO
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    P = FO.read_P('000000')
    cam = tuple(float(c) for c in RO.camera_of_P(P))
    H, W = 375, 1242

    def dense(B):
        frames = [FO.kitti_raw(rng, H, W) for _ in range(B)]
        planes = [torch.from_numpy(np.concatenate([fr[k].reshape((-1,) + fr[k].shape[2:]) for fr in frames])).to(dev) for k in range(3)]
        pc1, pc2, _, counts = ops.frames_from_kitti(planes[0], planes[1], planes[2], [P] * B, [H] * B, [W] * B)
        n = counts.cpu().tolist()
        keep = torch.cat([torch.arange(b * H * W, b * H * W + n[b]) for b in range(B)]).to(dev)
        return pc1[:, keep].contiguous(), pc2[:, keep].contiguous(), [0] + list(np.cumsum(n))

    sampled = torch.from_numpy(np.ascontiguousarray(RO.random_cloud(rng, 8192, H, W, camera=cam, margin=0.0).T)).to(dev)
    one_pixel = torch.from_numpy(np.ascontiguousarray(RO.back_project(
        np.full(65536, 600.2), np.full(65536, 180.1), 5.0 + rng.permutation(65536) * 1e-3, cam).T)).to(dev)
    d1 = dense(1)
    d16 = dense(16)
    shapes = [('sampled cloud, 8 192 points', sampled, None, [0, 8192], 1), ('dense frame, %d points' % d1[2][-1], d1[0], d1[1], d1[2], 1),
              ('16 dense frames, %d points' % d16[2][-1], d16[0], d16[1], d16[2], 16),
              ('65 536 points into one pixel', one_pixel, None, [0, 65536], 1)]
    lines = ['%s on %s%s' % (os.path.basename(__file__), torch.cuda.get_device_name(0),
                             ' with HPL_LIB=%s' % os.path.basename(os.environ['HPL_LIB']) if os.environ.get('HPL_LIB') else ''),
             'images of %d x %d; us per call: median (fastest .. slowest) of %d repeats of %d back-to-back calls, %d warm-up calls'
             % (H, W, a.repeats, a.calls, a.warmup), '']
    for name, pc, pc2, prefix, B in shapes:
        N, M = pc.shape[1], B * H * W
        for r in (0, 1):
            call = lambda: ops.render_maps(pc, [cam] * B, [H] * B, [W] * B, footprint=r, rel_tol=0.02, prefix=prefix)      # noqa: E731
            us = per_call_us(call, a.calls, a.repeats, a.warmup)
            # what the call moves once: the cloud, pixel_of, visible, winner, depth, and the z-buffer written and read
            nbytes = 12 * N + 4 * N + N + 4 * M + 4 * M + 16 * M
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = per_call_us(lambda: dst.copy_(src), a.calls, a.repeats, a.warmup)
            lines.append('%-36s footprint %d  render_maps %9.1f (%9.1f .. %9.1f)   copy of %6.1f MB %8.1f   x %.1f' % (
                name, r, us[0], us[1], us[2], nbytes / 1e6, copy[0], us[0] / copy[0]))
            if B == 1:
                comp = per_call_us(lambda: torch_zbuffer(pc, cam, H, W, r), max(1, a.calls // 4), 3, 1)
                lines.append('%-36s              torch composition %9.1f (%9.1f .. %9.1f)   x %.1f of render_maps' % (
                    '', comp[0], comp[1], comp[2], comp[0] / us[0]))
                w, d = torch_zbuffer(pc, cam, H, W, r)
                got = ops.render_maps(pc, [cam], [H], [W], footprint=r, prefix=prefix)
                same = bool(torch.equal(w, got[1]) and torch.equal(d.view(torch.int32), got[2].view(torch.int32)))
                lines.append('%-36s              the composition\'s winner and depth equal the call\'s: %s' % ('', same))
            if pc2 is not None:
                kus = per_call_us(lambda: ops.maps_to_kitti(pc, pc2, [P] * B, [H] * B, [W] * B, footprint=r, prefix=prefix),
                                  a.calls, a.repeats, a.warmup)
                lines.append('%-36s              maps_to_kitti %9.1f (%9.1f .. %9.1f)' % ('', kus[0], kus[1], kus[2]))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as fd:
            fd.write(text + '\n')


if __name__ == '__main__':
    main()
