"""CPU: hpl_object_fit's declaration, export and refusals (no device needed), its workspace arithmetic, the numpy restatement
tests/object_fit_oracle.py on closed-form cases, the margin at tau of the scene the GPU tests use (their comparison of inlier
masks against numpy then has no ties), and the engine's --object-refine arguments and key order."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import object_fit_oracle as oracle
import rigid_oracle
from common import ROOT
from hplflownet_amd import _lib
from object_fit_oracle import MAX_OBJECTS, N, SEED, SIZES, TAU

I64 = ctypes.c_int64


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_object_fit\s*\(', body) and re.search(r'\bint64_t\s+hpl_object_fit_workspace_bytes\s*\(', body)
    assert 'hpl_object_fit' in _lib.EXPORTS and 'hpl_object_fit_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_object_fit') and hasattr(_lib.load(), 'hpl_object_fit_workspace_bytes')
    from hplflownet_amd import build
    assert 'object_fit.hip' in build.SOURCES


def call(pc=8, pc_ld=100, flow=8, sc=1, sp=3, weight=None, labels=8, batch=1, prefix=(0, 100), max_objects=16, iters=4, tau=0.1,
         Rt=8, stats=8, residual=None, refined=8, ws=256, ws_bytes=1 << 24):
    """hpl_object_fit with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    return _lib.load().hpl_object_fit(pc, pc_ld, flow, sc, sp, weight, labels, batch, prefix, max_objects, iters, tau, Rt, stats,
                                      residual, refined, ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1),
    dict(max_objects=0), dict(max_objects=-1), dict(max_objects=4097),
    dict(iters=-1), dict(iters=17),
    dict(tau=0.0), dict(tau=-0.1), dict(tau=float('inf')), dict(tau=float('nan')),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(pc_ld=99),
    dict(sc=0), dict(sp=0), dict(sc=-1), dict(sc=50, sp=1), dict(sc=1, sp=2),
    dict(pc=None), dict(flow=None), dict(labels=None), dict(Rt=None), dict(stats=None), dict(prefix=None), dict(ws=None),
    dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_object_fit_workspace_bytes(1, 100, 16) - 1),
    dict(max_objects=4096, ws_bytes=_lib.load().hpl_object_fit_workspace_bytes(1, 100, 4095) - 1),
    dict(pc=6), dict(flow=2), dict(weight=9), dict(labels=10), dict(Rt=10), dict(stats=6), dict(residual=5), dict(refined=7),
    dict(ws=8), dict(ws=128),
    dict(prefix=(0, 2 ** 31 // 3 + 1), pc_ld=2 ** 31, ws_bytes=1 << 50), dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_object_fit')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, iters=0, tau=1e-3, sc=7, sp=1, max_objects=4096, refined=None) == 0
    assert call(batch=64, prefix=(0,) * 65, weight=8, residual=8, iters=16, max_objects=1) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_object_fit_workspace_bytes
    assert f(0, 10, 1) == -1 and f(65, 10, 1) == -1 and f(1, -1, 1) == -1 and f(1, 2 ** 31 // 3 + 1, 1) == -1
    assert f(1, 10, 0) == -1 and f(1, 10, -1) == -1 and f(1, 10, 4097) == -1
    ns = [0, 1, 3, 1023, 1024, 1025, 8192, N, 450000, 2 ** 27]
    for b in (1, 2, 16, 63, 64):
        for m in (1, 12, 256, 4095, 4096):
            vals = [f(b, n, m) for n in ns]
            assert all(v > 0 and v % 256 == 0 for v in vals) and vals == sorted(vals)
            assert all(f(b + 1, n, m) >= f(b, n, m) for n in ns if b < 64)
            assert all(f(b, n, m + 1) >= f(b, n, m) for n in ns if m < 4096)
    # 16 bytes of keys and values, a 32-byte record, and 16 doubles per span and per (pair, object) slot
    assert f(1, 450000, 256) >= 48 * 450000 + 128 * (450000 // 1024 + 256 + 1)
    assert f(64, 0, 4096) >= 128 * (64 * 4096 + 1)


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc, fl, lab = torch.zeros(3, 10), torch.zeros(10, 3), torch.zeros(10, dtype=torch.int32)
    with pytest.raises(_lib.HplError):
        ops.object_fit(pc, fl, lab)                           # host tensors: no CPU fallback
    for kw in (dict(iters=-1), dict(iters=17), dict(iters=2.0), dict(tau=0.0), dict(tau=float('nan')), dict(max_objects=0),
               dict(max_objects=4097), dict(max_objects=True)):
        with pytest.raises(_lib.HplError):
            ops.object_fit(pc, fl, lab, **kw)


# ----------------------------------------------------------------------------- the restatement
def test_an_exact_motion_per_object_is_recovered():
    """Three objects with an exact rigid motion each, interleaved with unlabelled points, and objects of 1 and 2 members."""
    rng = np.random.RandomState(1)
    truth = [(rigid_oracle.rotation((1, 2, 3), 0.7), np.array([1.0, -2.0, 3.0])),
             (rigid_oracle.rotation((0, 0, 1), 3.0), np.zeros(3)),
             (rigid_oracle.rotation((0.1, 1, 0.05), 0.03), rigid_oracle.TRUE_T)]
    sizes = [40, 3, 200, 1, 2]
    labels = rng.permutation(np.concatenate([np.full(n, k) for k, n in enumerate(sizes)] + [np.full(60, -1), np.full(7, 9)]))
    p = rng.uniform(-10, 10, (3, len(labels)))
    f = rng.normal(size=p.shape)
    for k, (R, t) in enumerate(truth):
        f[:, labels == k] = (R @ p + t[:, None] - p)[:, labels == k]
    before = f.astype(np.float32).T.copy()
    fits, residual, refined = oracle.fit_objects(p.astype(np.float32), f.astype(np.float32), labels, max_objects=8, refined=before,
                                                 residual=np.full(len(labels), -1.0))
    assert len(fits) == 1 and len(fits[0]) == 8 and [o is None for o in fits[0]] == [False] * 5 + [True] * 3
    for k, (R, t) in enumerate(truth):
        o = fits[0][k]
        assert o['status'] == 1 and np.array_equal(o['members'], np.flatnonzero(labels == k))
        assert np.abs(o['R'] - R).max() <= 1e-5 and np.abs(o['t'] - t).max() <= 2e-4 and o['inlier'].all()
    for k in (3, 4):                                          # fewer than 3 members: no fit
        o = fits[0][k]
        assert o['status'] == 0 and np.array_equal(o['R'], np.eye(3)) and not o['t'].any() and not o['inlier'].any()
        assert np.allclose(o['residual'], np.linalg.norm(f[:, labels == k], axis=0), atol=1e-5)
    listed = (labels >= 0) & (labels < 8)
    assert (residual[~listed] == -1).all() and (residual[listed] >= 0).all()               # written at the members alone
    untouched = ~listed | (labels >= 3)
    assert np.array_equal(refined[untouched], before[untouched]) and np.abs(refined - before).max() <= 1e-4


def test_batches_number_their_objects_per_pair():
    p, f, labels, _ = oracle.scene()
    one = oracle.fit_objects(p[:, :3000], f[:, :3000], labels[:3000], iters=1)
    two = oracle.fit_objects(np.concatenate([p[:, 5000:5100], p[:, :3000]], 1), np.concatenate([f[:, 5000:5100], f[:, :3000]], 1),
                             np.concatenate([labels[5000:5100], labels[:3000]]), iters=1, prefix=[0, 100, 100, 3100])
    assert len(two[0]) == 3 and all(o is None for o in two[0][1])
    for a, b in zip(one[0][0], two[0][2]):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a['R'], b['R']) and np.array_equal(a['members'] + 100, b['members'])
    assert np.array_equal(one[1], two[1][100:], equal_nan=True)


@pytest.mark.parametrize('weighted', [False, True])
def test_scene_has_a_margin_at_tau(weighted):
    """No member's residual at the last solve lies within 1e-4 of tau, for every iters the GPU tests run; and at iters = 4 the
    inliers of every large object are exactly its undisplaced (and live) members, in float64 and in float32."""
    p, f, labels, displaced = oracle.scene()
    assert p.shape == (3, N) and N == 24001 and [int((labels == k).sum()) for k in range(len(SIZES))] == list(SIZES)
    w = rigid_oracle.weights(N, SEED) if weighted else None
    live = np.ones(N, bool) if w is None else np.nan_to_num(w, nan=0.0) > 0
    for iters in (0, 1, 2, 4):
        fits = oracle.fit_objects(p, f, labels, w, iters=iters)[0][0]
        assert [o is None for o in fits] == [False] * len(SIZES) + [True] * (MAX_OBJECTS - len(SIZES))
        margin = min(float(np.abs(o['residual'] - np.float64(np.float32(TAU))).min()) for o in fits if o is not None)
        print('weighted %s iters %d: nearest residual to tau at %.3g' % (weighted, iters, margin))
        assert margin >= 1e-4
    f32 = oracle.fit_objects(p, f, labels, w, dtype=np.float32)[0][0]
    assert [o['status'] for o in fits[:len(SIZES)]] == [0, 0] + [1] * 10
    for k in range(4, len(SIZES)):
        idx = fits[k]['members']
        assert np.array_equal(fits[k]['inlier'], ~displaced[idx] & live[idx]) and np.array_equal(f32[k]['inlier'], fits[k]['inlier'])
        assert displaced[idx].sum() == SIZES[k] // 5


def test_non_finite_variant_keeps_every_large_object_fitted():
    p, f, labels, _ = oracle.scene()
    q, g, w = oracle.with_non_finite(p, f, labels, rigid_oracle.weights(N, SEED))
    assert np.isnan(q).sum() == 2 and np.isinf(q).sum() == 1 and np.isinf(g).sum() == 2
    with np.errstate(invalid='ignore'):
        fits = oracle.fit_objects(q, g, labels, w)[0][0]
    assert [o['status'] for o in fits[:len(SIZES)]] == [0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]


# ----------------------------------------------------------------------------- engine
def test_engine_argument_errors():
    from hplflownet_amd import engine
    base = ['--evaluate', '--rigid-refine', '--segment']
    assert engine.parse_args(base + ['--object-refine']).objects == {'iters': 4, 'tau': 0.1}
    assert engine.parse_args(base + ['--rigid-iters', '2', '--rigid-tau', '0.25', '--object-refine']).objects == \
        {'iters': 2, 'tau': 0.25}                             # the fit's values
    assert engine.parse_args(base + ['--object-refine', '--object-iters', '0', '--object-tau', '0.3']).objects == \
        {'iters': 0, 'tau': 0.3}
    assert engine.parse_args(base).objects is None and engine.parse_args(['--evaluate']).objects is None
    for extra in (['--object-refine'], ['--evaluate', '--object-refine'], ['--evaluate', '--rigid-refine', '--object-refine'],
                  ['--evaluate', '--segment', '--object-refine'], ['--rigid-refine', '--segment', '--object-refine'],
                  base + ['--object-iters', '3'], base + ['--object-tau', '0.1'],
                  base + ['--object-refine', '--object-iters', '17'], base + ['--object-refine', '--object-iters', '-1'],
                  base + ['--object-refine', '--object-tau', '0'], base + ['--object-refine', '--object-tau', 'inf'],
                  base + ['--object-refine', '--object-tau', 'nan']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


class _NoSamples(object):
    has_cameras = True

    def __len__(self):
        return 0


def test_validate_key_order_on_a_stub():
    """An empty shard reports (and would reduce) the reader's keys: the new ones behind every key of before, changing none."""
    from hplflownet_amd import engine
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
    base = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    rigid, seg = {'iters': 2, 'tau': 0.1}, {'eps': 1.0}
    before = list(tr.validate(_NoSamples(), rigid=rigid, segment=seg))
    assert list(tr.validate(_NoSamples(), rigid=rigid, segment=seg, objects=None)) == before
    new = ['piecewise_' + k for k in base] + ['piecewise_object_inliers']
    for objects in ({}, {'iters': 0}, {'tau': 0.3}, {'iters': 16, 'tau': 1.0}):
        assert list(tr.validate(_NoSamples(), rigid=rigid, segment=seg, objects=objects)) == before + new
    icp = {'iters': 5}
    with_icp = list(tr.validate(_NoSamples(), rigid=rigid, segment=seg, icp=icp))
    assert list(tr.validate(_NoSamples(), rigid=rigid, segment=seg, icp=icp, objects={})) == with_icp + new
    for kw in (dict(objects={}), dict(rigid=rigid, objects={}), dict(rigid=rigid, segment=seg, objects={'iterations': 2}),
               dict(rigid=rigid, segment=seg, objects=4), dict(rigid=rigid, segment=seg, objects={'iters': 17}),
               dict(rigid=rigid, segment=seg, objects={'tau': 0.0}), dict(rigid=rigid, segment=seg, objects={'tau': float('nan')})):
        with pytest.raises(_lib.HplError):
            tr.validate(_NoSamples(), **kw)
    assert engine.object_options({}, rigid) == rigid and engine.segment_options(seg)['eps'] == 1.0
    with pytest.raises(_lib.HplError):
        engine.segment_options({'eps': 1.0, 'iters': 2})      # (the segment options take no key of the object fits)
