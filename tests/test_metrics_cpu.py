"""CPU: the evaluation metrics' per-point contract and the cameras the 2D metrics need.

tests/golden/metrics2d.npz holds the reference's own evaluate_3d / get_batch_2d_flow / evaluate_2d on point sets under the
FlyingThings3D camera and three KITTI calibrations (tools/make_metrics_fixture.py), threshold points included.  `point_metrics`
below restates that arithmetic in float32 numpy, operation by operation -- the contract hpl_flow_metrics implements on the
device (tests/test_gpu_metrics.py compares the two)."""
import os

import numpy as np
import pytest

from common import ROOT

GOLD = os.path.join(ROOT, 'tests', 'golden')
CALIB = os.path.join(GOLD, 'kitti_calib')
SETS = ('ft3d', 'kitti0', 'kitti1', 'kitti2')
F32 = np.float32


def point_metrics(pc1, gt, pred, cam):
    """(N, 3) float32 arrays and a camera (f, cx, cy, constx, consty, constz) -> per-point err3, the three 3D predicates, err2
    and the 2D predicate, in the reference's float32 order (evaluation_utils.py:4-36, utils/geometry.py:42-65)."""
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
    return {'err3': err, 'acc3ds': (err < F32(0.05)) | (rel < F32(0.05)), 'acc3dr': (err < F32(0.1)) | (rel < F32(0.1)),
            'out3': (err > F32(0.3)) | (rel > F32(0.1)), 'err2': e2, 'acc2d': (e2 < F32(3.)) | (r2 < F32(0.05))}


def pair_values(pm):
    """Per-point metrics -> the six per-pair values (fp64 sums over the count, as hpl_flow_metrics' fold gives them)."""
    n = float(pm['err3'].size)
    return np.array([pm['err3'].astype(np.float64).sum() / n, pm['acc3ds'].sum() / n, pm['acc3dr'].sum() / n,
                     pm['out3'].sum() / n, pm['err2'].astype(np.float64).sum() / n, pm['acc2d'].sum() / n])


@pytest.fixture(scope='module')
def fixture():
    return np.load(os.path.join(GOLD, 'metrics2d.npz'))


@pytest.mark.parametrize('name', SETS)
def test_restatement_reproduces_the_reference(fixture, name):
    z = fixture
    pc1, gt, pred, cam = z[name + '_pc1'], z[name + '_gt'], z[name + '_pred'], z[name + '_camera']
    got, ref = pair_values(point_metrics(pc1, gt, pred, cam)), z[name + '_ref']
    n = pc1.shape[0]
    for k in (1, 2, 3, 5):                                      # counts: exactly
        assert round(got[k] * n) == round(ref[k] * n) and abs(ref[k] * n - round(ref[k] * n)) < 1e-6, (name, k, got, ref)
    for k in (0, 4):                                            # means: fp64 sums here, numpy's float32 pairwise means there
        assert abs(got[k] - ref[k]) <= 2e-6 * abs(ref[k]), (name, k, got[k], ref[k])
    # every threshold point alone: its error is the reference's to the bit and its predicates agree
    k = int(z[name + '_nthr'])
    assert k >= 6
    tr = z[name + '_thr_ref']
    pm = point_metrics(pc1[-k:], gt[-k:], pred[-k:], cam)
    assert np.array_equal(pm['err3'].astype(np.float64), tr[:, 0]) and np.array_equal(pm['err2'].astype(np.float64), tr[:, 4])
    for col, key in ((1, 'acc3ds'), (2, 'acc3dr'), (3, 'out3'), (5, 'acc2d')):
        assert np.array_equal(pm[key].astype(np.float64), tr[:, col]), (name, key)


def test_fixture_sits_on_every_threshold(fixture):
    """The threshold points hit their fp32 targets: each threshold itself and one ulp either side."""
    z = fixture
    pm = point_metrics(*[z['ft3d_' + s][-21:] for s in ('pc1', 'gt', 'pred')], z['ft3d_camera'])
    want = []
    for t in (0.05, 0.1, 0.3, 0.05, 0.1, 3.0, 0.05):
        t = F32(t)
        want += [np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))]
    assert np.array_equal(z['ft3d_thr_target'], np.array(want, np.float32))
    assert np.array_equal(pm['err3'][:9], z['ft3d_thr_target'][:9])
    assert np.array_equal(pm['err2'][15:18], z['ft3d_thr_target'][15:18])


def test_kitti_calibration_parser(fixture):
    from hplflownet_amd.data import read_kitti_camera
    frames = [str(f) for f in fixture['kitti_frames']]
    assert '000000' in frames and sorted(os.listdir(CALIB)) == sorted(f + '.txt' for f in frames)
    cams = []
    for i, fr in enumerate(frames):
        cam = read_kitti_camera(os.path.join(CALIB, fr + '.txt'))       # 000000.txt: its P_rect_00 line is malformed
        assert np.array_equal(np.array(cam, np.float32), fixture['kitti%d_camera' % i]) and cam[5] != 0.0
        assert all(isinstance(c, float) and float(np.float32(c)) == c for c in cam)
        cams.append(cam)
    assert len(set(cams)) == 3


def _ft3d_tree(root, count=3, n=64):
    for i in range(count):
        d = os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        rng = np.random.RandomState(i)
        for nm in ('pc1', 'pc2'):
            np.save(os.path.join(d, nm + '.npy'), rng.uniform(1, 10, (n, 3)).astype(np.float32))


def _kitti_tree(root, frames, far=()):
    for fr in frames:
        d = os.path.join(root, 'KITTI_processed_occ_final', fr)
        os.makedirs(d)
        rng = np.random.RandomState(int(fr))
        pc = rng.uniform(-1, 1, (80, 3)).astype(np.float32)
        pc[:, 2] = 50. if fr in far else rng.uniform(2, 30, 80)
        np.save(os.path.join(d, 'pc1.npy'), pc)
        np.save(os.path.join(d, 'pc2.npy'), pc + 0.05)


def test_readers_report_their_cameras(tmp_path, fixture):
    from hplflownet_amd.data import FT3D_CAMERA, KITTI, FlyingThings3DSubset, ProcessData
    from hplflownet_amd.engine import DATA_PROCESS
    root = str(tmp_path)
    _ft3d_tree(root)
    ft = FlyingThings3DSubset(False, None, root, full=True, device='cpu')
    assert ft.has_cameras and ft[2].camera == FT3D_CAMERA == (-1050., 479.5, 269.5, 0., 0., 0.)
    frames = [str(f) for f in fixture['kitti_frames']]
    _kitti_tree(root, frames, far=(frames[1],))
    plain = KITTI(None, root, device='cpu')
    assert not plain.has_cameras and plain[0].camera is None
    cams = {fr: tuple(float(c) for c in fixture['kitti%d_camera' % i]) for i, fr in enumerate(frames)}
    # every point of frames[1] is beyond the depth cut: ProcessData rejects it and the reader falls through to frames[2] --
    # the sample carries frames[2]'s camera, not that of the frame it was asked for
    k = KITTI(ProcessData(DATA_PROCESS, 64, True, seed=0), root, device='cpu', calib_dir=CALIB)
    assert k.has_cameras
    assert [k[i].camera for i in range(3)] == [cams[frames[0]], cams[frames[2]], cams[frames[2]]]
    assert float(k[1][0][2].max()) < 35.                   # (points of frames[2]: frames[1] lies beyond the cut)
    # a calibration directory that misses a frame fails at construction and names it
    part = tmp_path / 'calib_part'
    part.mkdir()
    for fr in frames[:2]:
        (part / (fr + '.txt')).write_text(open(os.path.join(CALIB, fr + '.txt')).read())
    with pytest.raises(FileNotFoundError, match=frames[2] + '.txt'):
        KITTI(None, root, device='cpu', calib_dir=str(part))


def test_key_set_comes_from_the_reader(tmp_path):
    """validate's keys are decided without samples: a _Shard with no sample reports the keys of the full reader."""
    from hplflownet_amd import engine
    from hplflownet_amd.data import KITTI, FlyingThings3DSubset
    root = str(tmp_path)
    _ft3d_tree(root, count=1)
    ft = FlyingThings3DSubset(False, None, root, device='cpu')
    empty, full = engine._Shard(ft, 1, 2), engine._Shard(ft, 0, 2)
    assert len(empty) == 0 and len(full) == 1
    six = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert engine.metric_keys(empty) == engine.metric_keys(full) == engine.metric_keys(ft) == six
    _kitti_tree(root, ['000000'])
    ki = KITTI(None, root, device='cpu')
    assert engine.metric_keys(engine._Shard(ki, 3, 4)) == engine.metric_keys(ki) == six[:4]
    assert engine.metric_keys(engine._Shard(KITTI(None, root, device='cpu', calib_dir=CALIB), 3, 4)) == six
    assert not engine.SyntheticPairs.has_cameras and engine.metric_keys([]) == six[:4]


def test_cli_kitti_calib(tmp_path):
    from hplflownet_amd import engine
    a = engine.parse_args(['--evaluate', '--dataset', 'KITTI', '--data-root', str(tmp_path), '--kitti-calib', CALIB])
    assert a.kitti_calib == CALIB
    assert engine.parse_args(['--evaluate', '--dataset', 'KITTI', '--data-root', str(tmp_path)]).kitti_calib is None
    for bad in (['--evaluate', '--dataset', 'KITTI', '--kitti-calib', str(tmp_path / 'missing')],
                ['--evaluate', '--dataset', 'FlyingThings3DSubset', '--kitti-calib', CALIB],
                ['--evaluate', '--kitti-calib', CALIB]):
        with pytest.raises(SystemExit):
            engine.parse_args(bad)


def test_fold_of_the_eight_words():
    from hplflownet_amd import ops
    w = [4.0, 2.0, 1.0, 2.0, 3.0, 10.0, 4.0, 0.0]
    assert ops.flow_metrics_fold(w) == {'EPE3D': 0.5, 'Acc3DS': 0.25, 'Acc3DR': 0.5, 'Outliers': 0.75, 'EPE2D': 2.5, 'Acc2D': 1.0}
    assert list(ops.flow_metrics_fold(w, camera=False)) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers']
