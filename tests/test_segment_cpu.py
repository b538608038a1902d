"""CPU: hpl_motion_segment's declaration, export and refusals (no device needed), its workspace size, the numpy restatement
tests/segment_oracle.py on a hand-built example and on the scene the GPU tests use (so that their comparison is known to be
non-trivial), and the engine's --segment arguments and key set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
from segment_oracle import SCENE_KW, movers, scene, segment, segment_batch

I64 = ctypes.c_int64


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_motion_segment\s*\(', body)
    assert re.search(r'\bint64_t\s+hpl_motion_segment_workspace_bytes\s*\(', body)
    assert 'hpl_motion_segment' in _lib.EXPORTS and 'hpl_motion_segment_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_motion_segment') and hasattr(_lib.load(), 'hpl_motion_segment_workspace_bytes')
    from hplflownet_amd import build
    assert 'motion_segment.hip' in build.SOURCES


def call(pc=8, pc_ld=100, flow=8, sc=1, sp=3, residual=8, batch=1, prefix=(0, 100), tau=0.1, eps=0.5, dv=float('inf'),
         min_points=5, max_objects=256, labels=8, info=8, motion=8, stats=8, ws=256, ws_bytes=1 << 24):
    """hpl_motion_segment with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    return _lib.load().hpl_motion_segment(pc, pc_ld, flow, sc, sp, residual, batch, prefix, tau, eps, dv, min_points,
                                          max_objects, labels, info, motion, stats, ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1),
    dict(tau=0.0), dict(tau=-0.1), dict(tau=float('inf')), dict(tau=float('nan')),
    dict(eps=0.0), dict(eps=-1.0), dict(eps=float('inf')), dict(eps=float('nan')),
    dict(dv=0.0), dict(dv=-0.3), dict(dv=float('nan')),
    dict(min_points=0), dict(min_points=-5), dict(max_objects=0), dict(max_objects=4097), dict(max_objects=-1),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(pc_ld=99),
    dict(sc=0), dict(sp=0), dict(sc=-1), dict(sc=50, sp=1), dict(sc=1, sp=2),
    dict(pc=None), dict(flow=None), dict(residual=None), dict(labels=None), dict(info=None), dict(motion=None),
    dict(stats=None), dict(prefix=None), dict(ws=None),
    dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_motion_segment_workspace_bytes(1, 100) - 1),
    dict(pc=6), dict(flow=2), dict(residual=9), dict(labels=10), dict(info=6), dict(motion=5), dict(stats=7), dict(ws=8), dict(ws=128),
    dict(prefix=(0, 2 ** 31 // 3 + 1), pc_ld=2 ** 31, ws_bytes=1 << 40), dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert b'hpl_motion_segment' in _lib.load().hpl_last_error()


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, tau=1e-3, eps=7.0, dv=0.1, min_points=1, max_objects=4096, sc=7, sp=1) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_motion_segment_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(1, -1) == -1 and f(1, 2 ** 31 // 3 + 1) == -1
    ns = [0, 1, 3, 1024, 1025, 4099, 8192, 8193, 100000, 450000, 2 ** 20, 2 ** 20 + 1, 2 ** 24]
    for b in (1, 2, 16, 64):
        vals = [f(b, n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in vals) and vals == sorted(vals)
        assert all(f(b + 1, n) >= f(b, n) for n in ns if b < 64)
    assert f(1, 450000) < 64 << 20                            # a few arrays of N words and the sorts' temporaries


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc, fl, r = torch.zeros(3, 10), torch.zeros(10, 3), torch.zeros(10)
    with pytest.raises(_lib.HplError):
        ops.motion_segment(pc, fl, r)                         # host tensors: no CPU fallback
    for kw in (dict(tau=0.0), dict(eps=float('nan')), dict(dv=0.0), dict(min_points=0), dict(min_points=2.5), dict(max_objects=4097),
               dict(max_objects=True)):
        with pytest.raises(_lib.HplError):
            ops.motion_segment(pc, fl, r, **kw)


# ----------------------------------------------------------------------------- the restatement
def test_hand_built_example():
    """Eight points: a triple chained along x (0 - 1 - 2: 0 and 2 are only linked through 1), a pair, a loner, a point below
    tau and one that is near the triple but flows differently."""
    p = np.array([[0.0, 0.4, 0.8, 5.0, 5.3, 9.0, 0.2, 0.4],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.1],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    f = np.zeros((3, 8), np.float32)
    f[0, 7] = 1.0
    f[1, :3] = [0.0, 0.2, 0.4]                                # 0 and 2 also differ by more than dv: linked through 1 only
    r = np.array([1, 1, 1, 1, 1, 1, 0.05, 1], np.float32)
    order = [2, 7, 0, 3, 6, 1, 5, 4]                          # shuffled: the triple is (2, 5, 0) -> root 0
    p, f, r = p[:, order], f[:, order], r[order]
    o = segment(p, f, r, tau=0.1, eps=0.5, dv=0.3, min_points=2, max_objects=4)
    assert o['labels'].tolist() == [0, -2, 0, 1, -1, 0, -2, 1]
    assert o['obj_info'].tolist() == [[0, 3], [3, 2], [-1, 0], [-1, 0]]
    assert o['stats'].tolist() == [7, 2, 5, 0]
    assert np.allclose(o['obj_motion'][0], [0.4, 0, 0, 0, 0.2, 0]) and np.allclose(o['obj_motion'][1], [5.15, 0, 0, 0, 0, 0])
    assert not o['obj_motion'][2:].any()
    assert segment(p, f, r, tau=0.1, eps=0.5, dv=float('inf'), min_points=2)['stats'].tolist() == [7, 2, 6, 0]   # 7 joins the triple
    one = segment(p, f, r, tau=0.1, eps=0.5, dv=0.3, min_points=1, max_objects=2)
    assert one['stats'].tolist() == [7, 4, 7, 0] and one['labels'].tolist() == [0, 1, 0, 2, -1, 0, 3, 2]
    assert one['obj_info'].tolist() == [[0, 3], [1, 1]]       # the table holds the first two; the labels run on
    # pairs of a batch never link, wherever they are
    both = segment_batch(np.concatenate([p, p], 1), np.concatenate([f, f], 1), np.concatenate([r, r]), [0, 8, 16],
                         tau=0.1, eps=0.5, dv=0.3, min_points=2, max_objects=4)
    assert both[0].tolist() == o['labels'].tolist() * 2 and both[3].tolist() == [[7, 2, 5, 0]] * 2


def test_range_and_non_finite_points():
    p = np.array([[0.0, 1e30, 0.1, np.nan, 131300.0, 131100.0], [0.0] * 6, [0.0] * 6], np.float32)
    f = np.zeros((3, 6), np.float32)
    r = np.array([1, 1, np.nan, 1, 1, 1], np.float32)
    mov, oob = movers(p, f, r, 0.1, 0.5)
    # cells of 0.5005 m, |cell| <= 2^18 - 2: coordinates up to 131 201 m are representable
    assert mov.tolist() == [True, False, False, False, False, True] and oob.tolist() == [False, True, False, False, True, False]
    o = segment(p, f, r, min_points=1)
    assert o['labels'].tolist() == [0, -3, -1, -1, -3, 1] and o['stats'].tolist() == [2, 2, 2, 2]


@pytest.mark.parametrize('n', [1000, 4099])
def test_scene_has_exactly_its_six_boxes(n):
    p, f, r, per = scene(n)
    mov, oob = movers(p, f, r, SCENE_KW['tau'], SCENE_KW['eps'])
    assert mov[-6 * per:].all() and not mov[:-6 * per].any() and not oob.any()
    # no residual near tau: the mover set has no ties
    assert float(np.abs(r.astype(np.float64) - np.float64(np.float32(0.1))).min()) >= 1e-3
    o = segment(p, f, r, min_points=5, **SCENE_KW)
    assert o['stats'].tolist() == [6 * per, 6, 6 * per, 0]
    assert o['obj_info'][:7].tolist() == [[n - (6 - k) * per, per] for k in range(6)] + [[-1, 0]]
    assert np.array_equal(o['labels'][-6 * per:], np.repeat(np.arange(6), per))


def test_small_scene_fragments_into_noise():
    p, f, r, per = scene(300)
    o1, o5 = segment(p, f, r, min_points=1, **SCENE_KW), segment(p, f, r, min_points=5, **SCENE_KW)
    print('N = 300: %d components, %d of at least 5 points, %d noise points' % (o1['stats'][1], o5['stats'][1], (o5['labels'] == -2).sum()))
    assert o1['stats'][0] == 6 * per == 90 and 12 <= o1['stats'][1] <= 18
    assert 6 <= o5['stats'][1] < o1['stats'][1] and (o5['labels'] == -2).sum() >= 5
    assert o5['stats'][2] == 90 - (o5['labels'] == -2).sum()


# ----------------------------------------------------------------------------- engine
def test_engine_argument_errors():
    from hplflownet_amd import engine
    ok = engine.parse_args(['--evaluate', '--rigid-refine', '--segment'])
    assert ok.segment == {'eps': 0.5, 'dv': float('inf'), 'min_points': 5} and ok.rigid == {'iters': 4, 'tau': 0.1}
    assert engine.parse_args(['--evaluate', '--rigid-refine', '--segment', '--segment-eps', '1.0', '--segment-dv', '0.3',
                              '--segment-min-points', '3']).segment == {'eps': 1.0, 'dv': 0.3, 'min_points': 3}
    assert engine.parse_args(['--evaluate', '--rigid-refine']).segment is None
    for extra in (['--segment'], ['--evaluate', '--segment'], ['--rigid-refine', '--segment'],
                  ['--evaluate', '--rigid-refine', '--segment-eps', '1.0'], ['--evaluate', '--rigid-refine', '--segment-dv', '1.0'],
                  ['--evaluate', '--rigid-refine', '--segment-min-points', '3'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-eps', '0'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-eps', 'inf'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-eps', 'nan'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-dv', '0'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-dv', 'nan'],
                  ['--evaluate', '--rigid-refine', '--segment', '--segment-min-points', '0']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


class _NoSamples(object):
    has_cameras = True

    def __len__(self):
        return 0


def test_validate_key_set_on_a_stub():
    """An empty shard reports (and would reduce) the reader's keys: without segment exactly the keys of before."""
    from hplflownet_amd import engine
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
    base = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    rigid = base + ['rigid_' + k for k in base] + ['rigid_inliers', 'rigid_angle_deg', 'rigid_trans']
    assert list(tr.validate(_NoSamples())) == base and list(tr.validate(_NoSamples(), segment=None)) == base
    assert list(tr.validate(_NoSamples(), rigid={'iters': 2, 'tau': 0.1}, segment=None)) == rigid
    res = tr.validate(_NoSamples(), rigid={'iters': 2, 'tau': 0.1}, segment={'eps': 1.0})
    assert list(res) == rigid + ['seg_objects', 'seg_moving', 'seg_noise']
    for bad in (dict(segment={'eps': 1.0}), dict(rigid={'iters': 2}, segment={'radius': 1.0}), dict(rigid={'iters': 2}, segment={'eps': 0.0}),
                dict(rigid={'iters': 2}, segment={'dv': float('nan')}), dict(rigid={'iters': 2}, segment={'min_points': 0})):
        with pytest.raises(_lib.HplError):
            tr.validate(_NoSamples(), **bad)
