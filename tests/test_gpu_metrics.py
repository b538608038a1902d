"""GPU: hpl_flow_metrics (csrc/metrics.hip) against the reference's metrics and the float32 restatement of
tests/test_metrics_cpu.py, its bit-stability over layouts and batch positions, its argument checks, and Trainer.validate /
the CLI reporting EPE2D / Acc2D from the readers' cameras."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import ROOT  # noqa: E402
from test_metrics_cpu import CALIB, GOLD, SETS, _kitti_tree, pair_values, point_metrics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FT3D = (-1050., 479.5, 269.5, 0., 0., 0.)


def cols(a):
    """(N, 3) host array -> (3, N) contiguous device tensor."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).T)).to(DEV)


def run(preds, gts, pc1s, cams, rows=None):
    from hplflownet_amd import ops
    out = torch.full((rows or len(preds), 8), -7.0, dtype=torch.float64, device=DEV)
    ops.flow_metrics_pairs(preds, gts, pc1s, cams, out)
    return out.cpu().numpy()


def values(w, cam=True):
    """8 words -> the six values in the fixture's order (EPE3D, ACC3DS, ACC3DR, Outliers3D, EPE2D, ACC2D)."""
    n = w[0]
    return np.array([w[1] / n, w[2] / n, w[3] / n, w[4] / n] + ([w[5] / n, w[6] / n] if cam else []))


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLD, 'metrics2d.npz'))


def test_kernel_reproduces_the_reference_on_the_fixture(fixture):
    z = fixture
    for name in SETS:
        pc1, gt, pred, cam = z[name + '_pc1'], z[name + '_gt'], z[name + '_pred'], tuple(float(c) for c in z[name + '_camera'])
        n, k = pc1.shape[0], int(z[name + '_nthr'])
        w = run([cols(pred)], [cols(gt)], [cols(pc1)], [cam])[0]
        ref = z[name + '_ref']
        assert w[0] == n and w[7] == 0.0
        for j, slot in ((1, 2), (2, 3), (3, 4), (5, 6)):               # counts: exactly the reference's
            assert w[slot] == round(ref[j] * n), (name, slot, w, ref * n)
        got = values(w)
        for j in (0, 4):                                                # means within 2e-6 relative
            assert abs(got[j] - ref[j]) <= 2e-6 * abs(ref[j]), (name, j, got[j], ref[j])
        # each threshold point as a pair of its own, all in one launch: errors to the bit, predicates as the reference's
        tp = [(cols(pred[i:i + 1]), cols(gt[i:i + 1]), cols(pc1[i:i + 1])) for i in range(n - k, n)]
        W = run([t[0] for t in tp], [t[1] for t in tp], [t[2] for t in tp], [cam] * k)
        tr = z[name + '_thr_ref']
        assert np.array_equal(W[:, 1], tr[:, 0]) and np.array_equal(W[:, 5], tr[:, 4]), name
        assert np.array_equal(W[:, [2, 3, 4, 6]], tr[:, [1, 2, 3, 5]]), (name, W[:, [2, 3, 4, 6]], tr[:, [1, 2, 3, 5]])


def _random_pair(seed, n):
    rng = np.random.RandomState(seed)
    pc1 = np.stack([rng.uniform(-10, 10, n), rng.uniform(-3, 3, n), rng.uniform(2, 35, n)], 1).astype(np.float32)
    gt = rng.normal(0, 0.4, (n, 3)).astype(np.float32)
    pred = (gt + rng.normal(0, 0.05, (n, 3)) * rng.uniform(0, 4, (n, 1))).astype(np.float32)
    return pc1, gt, pred


def test_counts_equal_the_restatement_on_random_points(fixture):
    cams = [FT3D] + [tuple(float(c) for c in fixture['kitti%d_camera' % i]) for i in range(3)]
    data = [_random_pair(30 + i, 100000) for i in range(len(cams))]
    W = run([cols(d[2]) for d in data], [cols(d[1]) for d in data], [cols(d[0]) for d in data], cams)
    for w, (pc1, gt, pred), cam in zip(W, data, cams):
        pm = point_metrics(pc1, gt, pred, cam)
        assert [w[2], w[3], w[4], w[6]] == [float(pm[k].sum()) for k in ('acc3ds', 'acc3dr', 'out3', 'acc2d')]
        want = pair_values(pm)
        assert abs(w[1] / w[0] - want[0]) <= 1e-12 * want[0] and abs(w[5] / w[0] - want[4]) <= 1e-12 * want[4]


def test_identical_bits_across_layouts():
    """(3, N) contiguous, the transposed view of a point-major [N][3] buffer (the forward's flow), column slices of wider buffers."""
    pc1, gt, pred = _random_pair(7, 5000)
    base = run([cols(pred)], [cols(gt)], [cols(pc1)], [FT3D])[0]
    pm = [torch.from_numpy(a).to(DEV).t() for a in (pred, gt, pc1)]          # (3, N) views, strides (1, 3)
    assert pm[0].stride() == (1, 3)
    wide = []
    for a in (pred, gt, pc1):
        buf = torch.full((3, 5000 + 29), float('nan'), device=DEV)
        buf[:, 11:11 + 5000] = cols(a)
        wide.append(buf[:, 11:11 + 5000])
    for views in (pm, wide, [pm[0], wide[1], cols(pc1)]):
        w = run(views[:1], views[1:2], views[2:], [FT3D])[0]
        assert np.array_equal(w.view(np.int64), base.view(np.int64)), (w, base)


def test_identical_bits_alone_or_anywhere_in_a_batch(fixture):
    kc = tuple(float(c) for c in fixture['kitti0_camera'])
    counts = [1, 37, 8192, 163840]
    pairs = [_random_pair(100 + i, counts[i % 4]) for i in range(64)]
    dev = [tuple(cols(a) for a in p) for p in pairs]
    cams = [(FT3D, None, kc)[i % 3] for i in range(64)]
    W = run([d[2] for d in dev], [d[1] for d in dev], [d[0] for d in dev], cams)
    for i in range(64):
        alone = run([dev[i][2]], [dev[i][1]], [dev[i][0]], [cams[i]])[0]
        if cams[i] is None:
            assert (W[i, 5], W[i, 6]) == (-7.0, -7.0) and (alone[5], alone[6]) == (-7.0, -7.0)     # no camera: slots untouched
        assert np.array_equal(W[i].view(np.int64), alone.view(np.int64)), i
    # the pair of 163 840 points with the KITTI camera at positions 0, 17 and 63 of 64-pair batches
    t = dev[3]
    ref = run([t[2]], [t[1]], [t[0]], [kc])[0]
    for pos in (0, 17, 63):
        order = [j for j in range(64) if j != 3]
        order.insert(pos, 3)
        cs = [kc if j == 3 else cams[j] for j in order]
        Wp = run([dev[j][2] for j in order], [dev[j][1] for j in order], [dev[j][0] for j in order], cs)
        assert np.array_equal(Wp[pos].view(np.int64), ref.view(np.int64)), pos


def test_bad_arguments_raise_and_launch_nothing():
    import ctypes
    from hplflownet_amd import _lib, ops
    from hplflownet_amd._lib import HplError
    pc1, gt, pred = _random_pair(3, 64)
    p = [cols(a) for a in (pred, gt, pc1)]
    out = torch.full((70, 8), -7.0, dtype=torch.float64, device=DEV)
    bad = [lambda: ops.flow_metrics_pairs([], [], [], [], out),                                       # batch 0
           lambda: ops.flow_metrics_pairs([p[0]] * 65, [p[1]] * 65, [p[2]] * 65, [None] * 65, out),     # batch 65
           lambda: ops.flow_metrics_pairs([p[0][:, :0]], [p[1][:, :0]], [p[2][:, :0]], [None], out)]   # no points
    stage = ops.MetricsStage(1, DEV)

    def raw(**kw):
        d = ops._metrics_desc(p[0], p[1], p[2], FT3D)
        for k, v in kw.items():
            setattr(d, k, v)
        ctypes.memmove(stage.host.data_ptr(), ctypes.byref(d), ops.MetricsStage.SIZE)
        _lib.check(_lib.load().hpl_flow_metrics(stage.host.data_ptr(), 1, stage.dev.data_ptr(), out.data_ptr(), _lib.stream()),
                   'hpl_flow_metrics')
    bad += [lambda: raw(pred=None), lambda: raw(gt=None), lambda: raw(pc1=None), lambda: raw(n=0), lambda: raw(gt_sp=-1),
            lambda: raw(pc1_sc=-3)]
    for f in bad:
        with pytest.raises(HplError):
            f()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    raw()                                                                              # the same call with good arguments runs
    assert out[0, 0].item() == 64.0


def _ft3d_tree(root, count, n):
    from hplflownet_amd.synthetic import synthetic_pair
    for i in range(count):
        d = os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        pc1, pc2, _ = synthetic_pair(n[i] if isinstance(n, list) else n, 60 + i)
        flip = np.array([-1, 1, -1], np.float32)
        np.save(os.path.join(d, 'pc1.npy'), pc1 * flip)
        np.save(os.path.join(d, 'pc2.npy'), pc2 * flip)


def test_validate_reports_six_metrics_per_pair(tmp_path):
    from hplflownet_amd import data as D
    from hplflownet_amd.engine import Trainer
    root = str(tmp_path)
    _ft3d_tree(root, 6, [700, 700, 512, 700, 700, 600])
    ds = D.FlyingThings3DSubset(False, None, root, full=True, device=DEV)
    tr = Trainer('HPLFlowNetShallow', torch.device(DEV), init='hash')
    res = tr.validate(ds)
    assert list(res) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert [i for i, _ in tr.val_pairs] == list(range(6))
    keys = list(res)
    with torch.no_grad():
        for i, v in tr.val_pairs:
            s_ = ds[i]
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))[0]
            pm = point_metrics(*[a.t().cpu().numpy() for a in (s_[0], s_[2], flow)], FT3D)
            want = pair_values(pm)
            got = np.array([v[k] for k in keys])
            assert np.allclose(got, want, rtol=1e-5, atol=0), (i, got, want)
    for k in keys:
        assert abs(res[k] - np.mean([v[k] for _, v in tr.val_pairs])) < 1e-12
    single = dict(tr.val_pairs)
    for kw in ({'batch_size': 4}, {'batch_size': 4, 'ragged': True}):
        r = tr.validate(ds, **kw)
        assert list(r) == keys and [i for i, _ in tr.val_pairs] == list(range(6))
        for i, v in tr.val_pairs:
            for k in keys:
                assert abs(v[k] - single[i][k]) < 2e-4 * max(1.0, abs(single[i][k])), (kw, i, k, v[k], single[i][k])


def test_kitti_evaluation_uses_each_returned_frames_camera(tmp_path, fixture):
    from hplflownet_amd import data as D
    from hplflownet_amd import engine
    root = str(tmp_path)
    frames = [str(f) for f in fixture['kitti_frames']]
    # frames[1] lies beyond the depth cut: its sample falls through to frames[2], whose camera it must carry
    for fr in frames:
        d = os.path.join(root, 'KITTI_processed_occ_final', fr)
        os.makedirs(d)
        rng = np.random.RandomState(int(fr))
        pc = np.stack([rng.uniform(-5, 5, 900), rng.uniform(-1, 1, 900), rng.uniform(3, 30, 900)], 1).astype(np.float32)
        if fr == frames[1]:
            pc[:, 2] += 40.
        np.save(os.path.join(d, 'pc1.npy'), pc)
        np.save(os.path.join(d, 'pc2.npy'), pc + rng.normal(0, 0.1, pc.shape).astype(np.float32))
    cams = {fr: tuple(float(c) for c in fixture['kitti%d_camera' % i]) for i, fr in enumerate(frames)}
    ds = D.KITTI(D.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root, device=DEV, calib_dir=CALIB)
    tr = engine.Trainer('HPLFlowNetShallow', torch.device(DEV), init='hash')
    res = tr.validate(ds)
    assert list(res)[-2:] == ['EPE2D', 'Acc2D']
    ds2 = D.KITTI(D.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root, device=DEV, calib_dir=CALIB)
    with torch.no_grad():
        for (i, v), fr in zip(tr.val_pairs, [frames[0], frames[2], frames[2]]):
            s_ = ds2[i]
            assert s_.camera == cams[fr]
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))[0]
            arrs = [a.t().cpu().numpy() for a in (s_[0], s_[2], flow)]
            want = pair_values(point_metrics(*arrs, cams[fr]))
            assert abs(v['EPE2D'] - want[4]) <= 1e-5 * want[4] and v['Acc2D'] == want[5], (i, v, want)
            other = pair_values(point_metrics(*arrs, cams[frames[1]]))
            assert other[4] != want[4]
    # the CLI: the same numbers with --kitti-calib; the four 3D metrics and a note without it
    out = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'KITTI', '--data-root', root,
                       '--kitti-calib', CALIB])
    assert list(out) == list(res) and all(abs(out[k] - res[k]) <= 1e-5 * max(1.0, abs(res[k])) for k in res), (out, res)
    out4 = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'KITTI', '--data-root', root])
    assert list(out4) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers']


def test_two_ranks_one_with_an_empty_shard(tmp_path):
    """Two ranks over gloo on the one GPU; one validation sample, so rank 1's shard is empty: both ranks issue the same collective
    (six keys decided by the reader) and return the same values."""
    root = str(tmp_path)
    _ft3d_tree(root, 1, 512)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='2', LOCAL_RANK='0',
               HPL_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    code = ('import json, sys; from hplflownet_amd import engine; '
            'r = engine.main(["--arch", "HPLFlowNetShallow", "--points", "512", "--evaluate", "--dataset", "FlyingThings3DSubset", '
            '"--data-root", sys.argv[1]]); print("RESULT " + json.dumps(r))')
    procs = [subprocess.Popen([sys.executable, '-c', code, root], cwd=ROOT, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in (1, 0)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = []
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
        res.append(json.loads([ln for ln in so.splitlines() if ln.startswith('RESULT ')][-1][7:]))
    assert list(res[0]) == list(res[1]) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert res[0] == res[1] and all(np.isfinite(v) for v in res[0].values())
