#!/usr/bin/env python
"""Generate tests/golden/metrics2d.npz (and tests/golden/kitti_calib/) by running the REFERENCE's own metrics.

Runs only where the reference exists (tools/ref_import.REF).  The inputs are seeded random point sets; the file holds the
reference's outputs for them: evaluation_utils.evaluate_3d, utils/geometry.get_batch_2d_flow and evaluation_utils.evaluate_2d,
exactly as evaluation_bnn.py:64-80 chains them (pc2 = pc1 + gt, predicted pc2 = pc1 + pred).

Sets (key prefix):
  ft3d         2 048 points under the FlyingThings3D camera (the defaults of geometry.project_3d_to_2d), then the threshold
               points: for every threshold of the six metrics -- 3D error 0.05 / 0.1 / 0.3, 3D relative error 0.05 / 0.1,
               2D error 3 px, 2D relative error 0.05 -- a point whose fp32 value is the threshold itself and one a ulp either
               side (found by search below), with the other predicate of its OR kept out of the way
  kitti<i>     three KITTI frames with different P_rect_02 (frame 000000 among them), 1 024 points each plus their own 2D
               threshold points; the frames' calib_cam_to_cam files are copied verbatim to tests/golden/kitti_calib/

Per set: <p>_pc1, <p>_gt, <p>_pred (N, 3) float32; <p>_camera (6,) float32 (f, cx, cy, constx, consty, constz);
<p>_ref (6,) the reference's EPE3D, ACC3DS, ACC3DR, Outliers3D, EPE2D, ACC2D of the whole set; <p>_nthr the number of trailing
threshold points; <p>_thr_ref (nthr, 6) the same six values of each threshold point alone; <p>_thr_target (nthr,) float32 the
value each threshold point was built to hit.
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from ref_import import REF, install_shims  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
FT3D = (-1050., 479.5, 269.5, 0., 0., 0.)
F32 = np.float32


def kitti_camera(path):
    """utils/geometry.py:15-31 restated for one file (the reference inlines it in get_batch_2d_flow)."""
    with open(path) as fd:
        line = [ln for ln in fd.readlines() if ln.startswith('P_rect_02')][0]
    P = np.array([float(v) for v in line.split()[1:]], dtype=np.float32).reshape(3, 4)
    return np.array([-P[0, 0], P[0, 2], P[1, 2], P[0, 3], P[1, 3], P[2, 3]], np.float32)


def per_point(pc1, gt, pred, cam):
    """The per-point quantities in the reference's float32 order: err3, rel3, err2, rel2 (for the search only; the stored
    values are the reference's)."""
    f, cx, cy, kx, ky, kz = [F32(c) for c in cam]
    d = gt - pred
    err = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    rel = err / (np.sqrt((gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1]) + gt[:, 2] * gt[:, 2]) + F32(1e-4))

    def proj(p):
        return ((p[:, 0] * f + cx * p[:, 2] + kx) / (p[:, 2] + kz), (p[:, 1] * f + cy * p[:, 2] + ky) / (p[:, 2] + kz))
    x1, y1 = proj(pc1)
    xg, yg = proj(pc1 + gt)
    xp, yp = proj(pc1 + pred)
    fxg, fyg, fxp, fyp = xg - x1, yg - y1, xp - x1, yp - y1
    ex, ey = fxg - fxp, fyg - fyp
    e2 = np.sqrt(ex * ex + ey * ey)
    r2 = e2 / (np.sqrt(fxg * fxg + fyg * fyg) + F32(1e-5))
    return err, rel, e2, r2


def search(rng, cam, which, target, gen):
    """A point (pc1, gt, pred) whose quantity `which` (0 err3, 1 rel3, 2 err2, 3 rel2) is exactly the fp32 `target`: random
    (pc1, gt, direction v) from gen, pred = gt + s v with s bisected to the crossing, then the x of pred nudged by a few ulps."""
    for _ in range(50):
        K = 20000
        pc1, gt, v = gen(rng, K)
        lo, hi = np.zeros(K), np.full(K, 4.0)
        for _ in range(60):
            mid = (lo + hi) / 2
            q = (gt + mid[:, None] * v).astype(np.float32)
            val = per_point(pc1, gt, q, cam)[which]
            up = val > target
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        q = (gt + hi[:, None] * v).astype(np.float32)
        for k in range(-40, 41):
            qq = q.copy()
            qq[:, 0] = np.nextafter(q[:, 0], np.float32(np.inf) if k > 0 else np.float32(-np.inf)) if k else q[:, 0]
            for _ in range(abs(k) - 1):
                qq[:, 0] = np.nextafter(qq[:, 0], np.float32(np.inf) if k > 0 else np.float32(-np.inf))
            hit = np.nonzero(per_point(pc1, gt, qq, cam)[which] == target)[0]
            if hit.size:
                i = hit[0]
                return pc1[i], gt[i], qq[i]
    raise RuntimeError('no point found for quantity %d = %r' % (which, target))


def unit(rng, K):
    v = rng.normal(size=(K, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def cloud(rng, K):
    return np.stack([rng.uniform(-8, 8, K), rng.uniform(-3, 3, K), rng.uniform(4, 30, K)], 1).astype(np.float32)


def gen_gt(norm_lo, norm_hi, small_pc1=False, lateral=False):
    """pc1 (small x: fine steps of pc1 + pred), gt of norm in [lo, hi] (lateral: along x, near the camera -- a 2D flow of
    60 px or more), pred's direction from gt mostly along x."""
    def g(rng, K):
        pc1 = cloud(rng, K)
        if small_pc1:
            pc1[:, 0] = rng.uniform(-1e-3, 1e-3, K)
            pc1[:, 1] = rng.uniform(-1e-3, 1e-3, K)
        d = unit(rng, K)
        if lateral:
            pc1[:, 2] = rng.uniform(4, 8, K)
            d = d * 0.1 + np.array([1.0, 0, 0])
            d /= np.linalg.norm(d, axis=1, keepdims=True)
        gt = (d * rng.uniform(norm_lo, norm_hi, (K, 1))).astype(np.float32)
        v = unit(rng, K) * 0.2 + np.array([1.0, 0, 0])
        return pc1, gt, v / np.linalg.norm(v, axis=1, keepdims=True)
    return g


def threshold_points(rng, cam, with_3d=True):
    """(pc1, gt, pred, target) rows for every threshold (see the module docstring)."""
    # quantity, threshold, point generator keeping the other predicate of the OR out of the way
    specs = []
    if with_3d:
        specs += [(0, 0.05, gen_gt(0.3, 0.5)), (0, 0.1, gen_gt(0.3, 0.5)), (0, 0.3, gen_gt(4.0, 6.0)),
                  (1, 0.05, gen_gt(3.5, 4.5)), (1, 0.1, gen_gt(1.8, 2.2))]
    specs += [(2, 3.0, gen_gt(0.005, 0.02, True)), (3, 0.05, gen_gt(1.5, 2.0, True, True))]
    rows = []
    for which, thr, gen in specs:
        t = F32(thr)
        for target in (np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))):
            p, g, q = search(rng, cam, which, target, gen)
            rows.append((p, g, q, target))
    return rows


def random_set(rng, n):
    pc1 = cloud(rng, n)
    gt = rng.normal(0, 0.3, (n, 3)).astype(np.float32)
    pred = (gt + rng.normal(0, 0.06, (n, 3)) * rng.uniform(0, 3, (n, 1))).astype(np.float32)
    return pc1, gt, pred


def main():
    install_shims('dict')
    if not hasattr(np, 'float'):
        np.float = float            # evaluation_utils uses np.float (removed in numpy >= 1.24): alias for the calls
    import evaluation_utils as EU
    from utils import geometry as G

    def ref6(pc1, gt, pred, path):
        m3 = EU.evaluate_3d(pred, gt)
        fp, fg = G.get_batch_2d_flow(pc1[None], (pc1 + gt)[None], (pc1 + pred)[None], [path])
        m2 = EU.evaluate_2d(fp, fg)
        return np.array(list(m3) + list(m2), np.float64)

    calib_src = os.path.join(REF, 'utils', 'calib_cam_to_cam')
    frames, seen = [], set()
    for fn in sorted(os.listdir(calib_src)):
        cam = tuple(kitti_camera(os.path.join(calib_src, fn)))
        if cam not in seen:
            seen.add(cam)
            frames.append(fn[:-4])
        if len(frames) == 3:
            break
    assert frames[0] == '000000'
    out = {'kitti_frames': np.array(frames)}
    sets = [('ft3d', np.array(FT3D, np.float32), 'FlyingThings3D/val/0000000', 2048, True)]
    sets += [('kitti%d' % i, kitti_camera(os.path.join(calib_src, fr + '.txt')), 'KITTI_processed_occ_final/' + fr, 1024, False)
             for i, fr in enumerate(frames)]
    rng = np.random.RandomState(14)
    for pre, cam, path, n, with_3d in sets:
        pc1, gt, pred = random_set(rng, n)
        thr = threshold_points(rng, cam, with_3d)
        tp = np.array([r[0] for r in thr], np.float32)
        tg = np.array([r[1] for r in thr], np.float32)
        tq = np.array([r[2] for r in thr], np.float32)
        pc1, gt, pred = np.concatenate([pc1, tp]), np.concatenate([gt, tg]), np.concatenate([pred, tq])
        thr_ref = np.stack([ref6(tp[i:i + 1], tg[i:i + 1], tq[i:i + 1], path) for i in range(len(thr))])
        # the search's restatement agrees with the reference on every threshold point (else the point proves nothing)
        e3, r3, e2, r2 = per_point(tp, tg, tq, cam)
        assert np.array_equal(thr_ref[:, 0], e3) and np.array_equal(thr_ref[:, 4].astype(np.float32), e2), pre
        out[pre + '_pc1'], out[pre + '_gt'], out[pre + '_pred'] = pc1, gt, pred
        out[pre + '_camera'] = np.asarray(cam, np.float32)
        out[pre + '_ref'] = ref6(pc1, gt, pred, path)
        out[pre + '_nthr'] = np.int64(len(thr))
        out[pre + '_thr_ref'] = thr_ref
        out[pre + '_thr_target'] = np.array([r[3] for r in thr], np.float32)
        print(pre, path, n, '+', len(thr), 'threshold points', out[pre + '_ref'])
    np.savez_compressed(os.path.join(GOLD, 'metrics2d.npz'), **out)
    dst = os.path.join(GOLD, 'kitti_calib')
    os.makedirs(dst, exist_ok=True)
    for fr in frames:
        shutil.copyfile(os.path.join(calib_src, fr + '.txt'), os.path.join(dst, fr + '.txt'))
    print('frames', frames)


if __name__ == '__main__':
    main()
