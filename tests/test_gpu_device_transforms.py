"""GPU: hpl_transform_pair (csrc/transforms.hip) and data.DeviceAugmentation / DeviceProcessData: the
reference's vectors bit for bit through the test hook, the device's own stream against the numpy restatement of
tests/test_device_transforms_cpu.py, the sampling rules, determinism and uniformity, the readers and the engine."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import GOLD  # noqa: E402
from test_device_transforms_cpu import F, oracle, replay_choice, replay_draws, transform_all, valid_mask  # noqa: E402
from test_metrics_cpu import CALIB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def to_params(P):
    from hplflownet_amd._lib import TransformParams
    p = TransformParams()
    p.m[:] = np.asarray(P['m'], np.float32).ravel().tolist()
    p.shift[:] = np.asarray(P['shift'], np.float32).ravel().tolist()
    p.m2[:] = np.asarray(P['m2'], np.float32).ravel().tolist()
    p.shift2[:] = np.asarray(P['shift2'], np.float32).ravel().tolist()
    p.jitter_sigma1, p.jitter_clip1, p.jitter_sigma2, p.jitter_clip2 = P['sigma1'], P['clip1'], P['sigma2'], P['clip2']
    p.depth_threshold = P['T']
    p.no_corr, p.num_points, p.allow_less_points, p.augment = int(P['no_corr']), P['num_points'], int(P['less']), int(P['augment'])
    p.seed, p.counter = P['seed'], P['counter']
    return p


def dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def run(runner, p1, p2, P, **hook):
    out = runner.run(p1, p2, to_params(P), **{k: dev(v, torch.int32 if k.startswith('sel') else torch.float32)
                                              for k, v in hook.items()})
    torch.cuda.synchronize()
    return None if out[0] is None else [o.cpu().numpy() for o in out]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def aug_params(rng, clip, no_corr, n, T=35.0, seed=11, counter=0, less=False):
    from hplflownet_amd.data import _rot_y
    m = np.diag(rng.uniform(0.95, 1.05, 3).astype(np.float32)).dot(_rot_y(rng.uniform(-0.17, 0.17), np.float32).T)
    return dict(T=T, no_corr=no_corr, num_points=n, less=less, augment=True, seed=seed, counter=counter, sigma1=0.01,
                clip1=clip, sigma2=0.01, clip2=clip, m=m, shift=rng.uniform(-1, 1, 3).astype(np.float32),
                m2=_rot_y(rng.uniform(-0.05, 0.05), np.float32), shift2=rng.uniform(-0.3, 0.3, 3).astype(np.float32))


def pd_params(n, T=35.0, no_corr=False, less=False, seed=3, counter=0):
    e = np.eye(3, dtype=np.float32)
    z = np.zeros(3, np.float32)
    return dict(T=T, no_corr=no_corr, num_points=n, less=less, augment=False, seed=seed, counter=counter, sigma1=0.,
                clip1=0., sigma2=0., clip2=0., m=e, shift=z, m2=e, shift2=z)


def cloud(M, seed, far=0.0):
    rng = np.random.RandomState(seed)
    p1 = rng.uniform(-8, 8, (M, 3)).astype(np.float32)
    p1[:, 2] = rng.uniform(1.5, 45 + far, M)
    return p1, (p1 + rng.normal(0, 0.3, (M, 3))).astype(np.float32)


@pytest.fixture(scope='module')
def runner():
    from hplflownet_amd import ops
    return ops.TransformRunner(DEV)


def test_reference_vectors_bit_for_bit_through_the_hook(runner):
    G = np.load(os.path.join(GOLD, 'transforms.npz'))
    for tag, kind, kw, seed in F.CASES:
        p1, p2 = F.cloud_pair(seed)
        rng = np.random.RandomState(seed)
        for suf in ('', '_b'):
            P, j1, j2 = replay_draws(kind, kw, rng, p1.shape[0])
            a, b, _ = transform_all(p1, p2, P, j1, j2)
            s1, s2 = replay_choice(P, valid_mask(a, b, P['T']), rng)
            hook = {k: v for k, v in (('jitter1', j1), ('jitter2', j2), ('sel1', s1), ('sel2', s2)) if v is not None}
            out = run(runner, p1, p2, P, **hook)
            for k, v in zip(('pc1', 'pc2', 'sf'), out):
                g = G['%s_%s%s' % (tag, k, suf)]
                assert v.T.dtype == g.dtype and v.T.shape == g.shape, (tag, k, suf, v.shape, g.shape)
                assert np.array_equal(bits(v.T), bits(g)), (tag, k, suf)


@pytest.mark.parametrize('M', [1000, 450000])
@pytest.mark.parametrize('no_corr', [False, True])
def test_own_stream_matches_the_restatement(runner, M, no_corr):
    p1, p2 = cloud(M, M + no_corr)
    for clip in (0.0, 0.02):
        rng = np.random.RandomState(M + 7 * no_corr)
        P = aug_params(rng, clip, no_corr, 8192 if M > 8192 else 256, seed=2 ** 40 + 17, counter=2 ** 33 + 5)
        want, _, counts = oracle(p1, p2, P)
        got = run(runner, p1, p2, P)
        assert runner.last_counts == counts
        for w, g in zip(want, got):
            assert w.shape == g.shape
            if clip == 0:
                assert np.array_equal(bits(g), bits(w))
            else:
                assert (np.abs(g - w) <= np.spacing(np.abs(w))).all(), np.abs(g - w).max()
                assert np.mean(g == w) > 0.999
    # the selected indices themselves: ProcessData mode with the point index written into x
    p1[:, 0] = np.arange(M, dtype=np.float32)
    p2[:, 0] = p1[:, 0]
    P = pd_params(8192 if M > 8192 else 256, no_corr=no_corr, seed=99, counter=4)
    _, (i1, i2), counts = oracle(p1, p2, P)
    got = run(runner, p1, p2, P)
    assert runner.last_counts == counts
    assert np.array_equal(got[0][0].astype(np.int64), i1) and np.array_equal(got[1][0].astype(np.int64), i2)
    assert (i1 != i2).any() == no_corr


def test_sampling_rules(runner):
    M = 2000
    p1, p2 = cloud(M, 5)
    p1[:, 0] = np.arange(M, dtype=np.float32)
    p2[:, 0] = p1[:, 0]
    near = np.nonzero((p1[:, 2] < 35) & (p2[:, 2] < 35))[0]
    V = near.size
    assert 0 < V < M
    # fewer valid than num_points: rejected without allow_less_points, every valid point in index order with it
    assert run(runner, p1, p2, pd_params(V + 1)) is None and runner.last_counts == (V, 0)
    for P in (pd_params(V + 1, less=True), pd_params(0), pd_params(-1, no_corr=True)):
        out = run(runner, p1, p2, P)
        assert runner.last_counts == (V, V)
        assert np.array_equal(out[0][0], near.astype(np.float32)) and np.array_equal(out[1][0], near.astype(np.float32))
    # no cut when DEPTH_THRESHOLD <= 0
    for T in (0.0, -1.0):
        out = run(runner, p1, p2, pd_params(-1, T=T))
        assert runner.last_counts == (M, M) and np.array_equal(out[0][0], np.arange(M, dtype=np.float32))
    # no valid point at all: rejected even with allow_less_points
    assert run(runner, p1 + np.float32([0, 0, 100]), p2 + np.float32([0, 0, 100]), pd_params(10, less=True)) is None
    assert runner.last_counts == (0, 0)
    # ProcessData mode: the raw rows, sf = pc2 - pc1; corr: the same indices for both clouds and sf following cloud 1
    out = run(runner, p1, p2, pd_params(300))
    idx = out[0][0].astype(np.int64)
    assert len(set(idx.tolist())) == 300 and set(idx.tolist()) <= set(near.tolist())
    assert np.array_equal(bits(out[0]), bits(p1[idx].T)) and np.array_equal(bits(out[1]), bits(p2[idx].T))
    assert np.array_equal(bits(out[2]), bits((p2[idx] - p1[idx]).T))
    out = run(runner, p1, p2, pd_params(300, no_corr=True))
    i1, i2 = out[0][0].astype(np.int64), out[1][0].astype(np.int64)
    assert (i1 != i2).any() and np.array_equal(bits(out[2]), bits((p2[i1] - p1[i1]).T))
    # augmentation with corr: sf follows cloud 1 (before cloud 2's jitter), cloud 2 is cloud 1's rows
    p1, p2 = cloud(M, 6)                    # (an index in x would rotate into z: real coordinates)
    P = aug_params(np.random.RandomState(1), 0.0, False, 300)
    a, b, sf = transform_all(p1, p2, P)
    out = run(runner, p1, p2, P)
    rows = [int(np.nonzero(np.all(a == r, 1))[0][0]) for r in out[0].T]
    assert np.array_equal(bits(out[1]), bits(b[rows].T)) and np.array_equal(bits(out[2]), bits(sf[rows].T))


def test_determinism_next_call_and_busy_stream():
    from hplflownet_amd import data as D
    from hplflownet_amd.engine import AUG_PC2, AUG_TOGETHER, DATA_PROCESS
    p1, p2 = cloud(60000, 9)
    tg = dict(AUG_TOGETHER, jitter_clip=0.02)

    def seq(busy):
        t = D.DeviceAugmentation(tg, AUG_PC2, DATA_PROCESS, 4096, False, seed=123, device=DEV)
        outs = []
        side = torch.cuda.Stream(DEV)
        x = torch.randn(2048, 2048, device=DEV)
        for _ in range(3):
            if busy:
                with torch.cuda.stream(side):
                    for _ in range(20):
                        x = x @ x
                        x = x / x.norm()
            outs.append([o.cpu().numpy() for o in t((p1, p2))])
        torch.cuda.synchronize()
        return outs

    a, b = seq(False), seq(True)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(bits(u), bits(v))
    assert not np.array_equal(a[0][0], a[1][0]) and not np.array_equal(a[1][0], a[2][0])


def test_inclusion_is_uniform(runner):
    from scipy import stats
    M, k = 64, 16
    p1, p2 = cloud(M, 2)
    p1[:, 0] = np.arange(M, dtype=np.float32)
    p1[:, 2] = p2[:, 2] = 1.0
    cnt = np.zeros(M)
    P = pd_params(k, seed=77)
    d1, d2 = dev(p1), dev(p2)
    for c in range(4000):
        P['counter'] = c
        out = runner.run(d1, d2, to_params(P))
        cnt[out[0][0].long().cpu().numpy()] += 1
    assert cnt.sum() == 4000 * k
    assert stats.chisquare(cnt).pvalue > 1e-3


def _ft3d_tree(root, split, count, n, far=()):
    from hplflownet_amd.synthetic import synthetic_pair
    for i in range(count):
        d = os.path.join(root, 'FlyingThings3D_subset_processed_35m', split, '%07d' % i)
        os.makedirs(d)
        pc1, pc2, _ = synthetic_pair(n, 70 + i)
        if i in far:
            pc1[:, 2] += 60.
            pc2[:, 2] += 60.
        flip = np.array([-1, 1, -1], np.float32)
        np.save(os.path.join(d, 'pc1.npy'), pc1 * flip)
        np.save(os.path.join(d, 'pc2.npy'), pc2 * flip)


def test_reader_returns_device_samples_and_falls_through(tmp_path):
    from hplflownet_amd import data as D
    from hplflownet_amd.engine import AUG_PC2, AUG_TOGETHER, DATA_PROCESS
    root = str(tmp_path)
    _ft3d_tree(root, 'train', 3, 900, far=(1,))
    t = D.DeviceAugmentation(AUG_TOGETHER, AUG_PC2, DATA_PROCESS, 512, False, seed=1, device=DEV)
    ds = D.FlyingThings3DSubset(True, t, root, full=True, device=DEV)
    assert ds.point_counts(0) == (512, 512)
    for i in range(3):
        s_ = ds[i]
        assert isinstance(s_, D.Sample) and s_.camera == D.FT3D_CAMERA
        assert all(x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (3, 512) and x.is_contiguous() for x in s_)
        assert float(s_[0][2].max()) < 35.0 and float(s_[1][2].max()) < 35.0
    assert t.calls == 4                      # frame 1 lies beyond the cut: its call was rejected and frame 2 served it


def test_engine_trains_and_evaluates_with_device_transforms(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    _ft3d_tree(root, 'train', 8, 800)           # every 4th directory: 2 training and 2 validation pairs
    _ft3d_tree(root, 'val', 8, 800)
    for B in ('1', '2'):
        ck = os.path.join(root, 'ck%s' % B)
        best = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--epochs', '1', '--dataset', 'FlyingThings3DSubset',
                            '--data-root', root, '--device-transforms', '--train-batch-size', B, '--ckpt-dir', ck])
        assert np.isfinite(best) and os.path.isfile(os.path.join(ck, 'checkpoint.pth.tar'))
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--batch-size', '2', '--dataset',
                       'FlyingThings3DSubset', '--data-root', root, '--device-transforms',
                       '--resume', os.path.join(root, 'ck2', 'checkpoint.pth.tar')])
    assert list(res) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D'] and all(np.isfinite(v) for v in res.values())


def test_kitti_ragged_evaluation_with_device_transforms(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    frames = sorted(f[:-4] for f in os.listdir(CALIB))
    for j, fr in enumerate(frames):
        d = os.path.join(root, 'KITTI_processed_occ_final', fr)
        os.makedirs(d)
        rng = np.random.RandomState(int(fr))
        n = 700 + 150 * j
        pc = np.stack([rng.uniform(-5, 5, n), rng.uniform(-1, 1, n), rng.uniform(3, 30, n)], 1).astype(np.float32)
        np.save(os.path.join(d, 'pc1.npy'), pc)
        np.save(os.path.join(d, 'pc2.npy'), pc + rng.normal(0, 0.1, pc.shape).astype(np.float32))
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '800', '--evaluate', '--batch-size', '2', '--ragged',
                       '--dataset', 'KITTI', '--data-root', root, '--kitti-calib', CALIB, '--device-transforms'])
    assert list(res) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D'] and all(np.isfinite(v) for v in res.values())
