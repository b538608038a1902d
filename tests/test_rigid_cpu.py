"""CPU: hpl_rigid_fit's declaration, export and refusals (no device needed), the numpy restatement tests/rigid_oracle.py on
closed-form cases, the convergence of the scene the GPU tests use (with the margin at tau that makes their mask comparisons
free of ties), and the engine's --rigid-refine arguments and key set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
from rigid_oracle import TRUE_R, TRUE_T, fit, kabsch, rotation, scene, weights

I64 = ctypes.c_int64
#: the cases tests/test_gpu_rigid.py compares against the restatement: (N, seed)
CASES = [(3, 3), (37, 37), (1000, 1000), (4099, 4099)]


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_rigid_fit\s*\(', body) and re.search(r'\bint64_t\s+hpl_rigid_fit_workspace_bytes\s*\(', body)
    assert 'hpl_rigid_fit' in _lib.EXPORTS and 'hpl_rigid_fit_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_rigid_fit')
    from hplflownet_amd import build
    assert 'rigid_fit.hip' in build.SOURCES


def call(pc=8, pc_ld=100, flow=8, sc=1, sp=3, weight=None, batch=1, prefix=(0, 100), iters=4, tau=0.1, Rt=8, stats=8,
         residual=None, refined=8, ws=8, ws_bytes=1 << 20):
    """hpl_rigid_fit with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    return _lib.load().hpl_rigid_fit(pc, pc_ld, flow, sc, sp, weight, batch, prefix, iters, tau, Rt, stats, residual, refined,
                                     ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1), dict(iters=-1), dict(iters=17),
    dict(tau=0.0), dict(tau=-0.1), dict(tau=float('inf')), dict(tau=float('nan')),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(pc_ld=99),
    dict(sc=0), dict(sp=0), dict(sc=-1), dict(sc=50, sp=1), dict(sc=1, sp=2),
    dict(pc=None), dict(flow=None), dict(Rt=None), dict(stats=None), dict(prefix=None), dict(ws=None),
    dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_rigid_fit_workspace_bytes(1, 100) - 1),
    dict(pc=6), dict(flow=2), dict(weight=9), dict(Rt=10), dict(stats=6), dict(residual=5), dict(refined=7), dict(ws=12),
    dict(prefix=(0, 2 ** 31 // 3 + 1), pc_ld=2 ** 31, ws_bytes=1 << 40), dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert b'hpl_rigid_fit' in _lib.load().hpl_last_error()


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, iters=0, tau=1e-3, sc=7, sp=1) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_rigid_fit_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(1, -1) == -1 and f(1, 2 ** 31 // 3 + 1) == -1
    ns = [0, 1, 3, 1024, 1025, 8192, 450000, 2 ** 29]
    for b in (1, 2, 16, 64):
        vals = [f(b, n) for n in ns]
        assert all(v > 0 and v % 8 == 0 for v in vals) and vals == sorted(vals)
        assert all(f(b + 1, n) >= f(b, n) for n in ns if b < 64)
    assert f(1, 450000) < 1 << 20                             # 16 doubles per 1024 points


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc, fl = torch.zeros(3, 10), torch.zeros(10, 3)
    with pytest.raises(_lib.HplError):
        ops.rigid_fit(pc, fl)                                 # host tensors: no CPU fallback
    for kw in (dict(iters=-1), dict(iters=17), dict(iters=2.0), dict(tau=0.0), dict(tau=float('nan'))):
        with pytest.raises(_lib.HplError):
            ops.rigid_fit(pc, fl, **kw)


# ----------------------------------------------------------------------------- the restatement
def test_kabsch_recovers_an_exact_motion():
    rng = np.random.RandomState(0)
    for axis, angle, t in (((1, 2, 3), 0.7, (1, -2, 3)), ((0, 0, 1), 3.0, (0, 0, 0)), ((0.1, 1, 0.05), 0.03, TRUE_T)):
        R = rotation(axis, angle)
        p = rng.uniform(-10, 10, (3, 50))
        q = R @ p + np.asarray(t, np.float64)[:, None]
        dp, dq = p - p.mean(1, keepdims=True), q - q.mean(1, keepdims=True)
        got = kabsch(dp @ dq.T)
        assert np.abs(got - R).max() <= 1e-12
        assert np.abs(q.mean(1) - got @ p.mean(1) - t).max() <= 1e-12


def mirror_scene(n=500, seed=4):
    """A nearly planar cloud and its mirror image: the orthogonal matrix that fits best is a reflection."""
    rng = np.random.RandomState(seed)
    c = np.array([[3.0], [1.0], [20.0]])
    d = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.normal(0, 0.01, n)])
    p = (c + d).astype(np.float32)
    q = c + np.diag([-1.0, 1.0, 1.0]) @ (p.astype(np.float64) - c) + np.array([[0.2], [0.0], [-0.5]])
    return p, (q - p).astype(np.float32)


def test_planar_reflection_still_gives_a_rotation():
    p, f = mirror_scene()
    P, Q = p.astype(np.float64), p.astype(np.float64) + f
    dp, dq = P - P.mean(1, keepdims=True), Q - Q.mean(1, keepdims=True)
    U, _, Vt = np.linalg.svd(dp @ dq.T)
    assert np.linalg.det(Vt.T @ U.T) < 0                      # the unconstrained solution is the reflection
    R = kabsch(dp @ dq.T)
    assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    o = fit(p, f, None, 0, 0.1)
    assert o['status'] == 1 and abs(np.linalg.det(o['R']) - 1) <= 1e-12


@pytest.mark.parametrize('n,seed', CASES)
@pytest.mark.parametrize('weighted', [False, True])
def test_scene_converges_with_a_margin_at_tau(n, seed, weighted):
    p, f, static = scene(n, seed)
    w = weights(n, seed) if weighted else None
    live = np.ones(n, bool) if w is None else np.nan_to_num(w, nan=0.0) > 0
    o = fit(p, f, w, 4, 0.1)
    assert o['status'] == 1
    assert np.array_equal(o['inlier'], static & live)         # the inlier set is the static set, exactly
    if n >= 37:                                               # (three noisy points fit themselves, not the true motion)
        assert np.abs(o['R'] - TRUE_R).max() <= 2e-3 and np.abs(o['t'] - TRUE_T).max() <= 2e-2
    for iters in (0, 4):                                      # no residual near tau: GPU mask comparisons have no ties
        r = fit(p, f, w, iters, 0.1)['residual']
        margin = float(np.abs(r - np.float64(np.float32(0.1))).min())
        print('N = %d weighted %s iters %d: nearest residual to tau at %.3g' % (n, weighted, iters, margin))
        assert margin >= 1e-4
    if n >= 37:                                               # fewer solves have not converged on every scene (N = 1000)
        o32 = fit(p, f, w, 4, 0.1, np.float32)
        assert np.array_equal(o32['inlier'], o['inlier'])


def test_degenerate_inputs_give_status_0():
    p, f, _ = scene(50, 1)
    for w, pp, ff in ((np.zeros(50, np.float32), p, f), (np.full(50, np.nan, np.float32), p, f), (None, p[:, :1], f[:, :1]),
                      (None, p[:, :2], f[:, :2]), (None, p[:, :0], f[:, :0])):
        o = fit(pp, ff, w, 4, 0.1)
        assert o['status'] == 0 and np.array_equal(o['R'], np.eye(3)) and not o['t'].any() and not o['inlier'].any()
        assert np.array_equal(o['refined'], ff.T) and np.isfinite(o['residual']).all() and o['share'] == 0
        assert np.allclose(o['residual'], np.linalg.norm(ff.astype(np.float64), axis=0), atol=1e-6)


# ----------------------------------------------------------------------------- engine
def test_engine_argument_errors():
    from hplflownet_amd import engine
    ok = engine.parse_args(['--evaluate', '--rigid-refine'])
    assert ok.rigid == {'iters': 4, 'tau': 0.1}
    assert engine.parse_args(['--evaluate', '--rigid-refine', '--rigid-iters', '0', '--rigid-tau', '0.25']).rigid == \
        {'iters': 0, 'tau': 0.25}
    assert engine.parse_args(['--evaluate']).rigid is None
    for extra in (['--rigid-refine'], ['--evaluate', '--rigid-iters', '3'], ['--evaluate', '--rigid-tau', '0.1'],
                  ['--evaluate', '--rigid-refine', '--rigid-iters', '17'], ['--evaluate', '--rigid-refine', '--rigid-iters', '-1'],
                  ['--evaluate', '--rigid-refine', '--rigid-tau', '0'], ['--evaluate', '--rigid-refine', '--rigid-tau', 'inf'],
                  ['--evaluate', '--rigid-refine', '--rigid-tau', 'nan']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


class _NoSamples(object):
    has_cameras = True

    def __len__(self):
        return 0


def test_validate_key_set_on_a_stub():
    """An empty shard reports (and would reduce) the reader's keys: without rigid exactly the keys of before."""
    from hplflownet_amd import engine
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
    base = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert list(tr.validate(_NoSamples())) == base
    assert list(tr.validate(_NoSamples(), rigid=None)) == base
    res = tr.validate(_NoSamples(), rigid={'iters': 2, 'tau': 0.1})
    assert list(res) == base + ['rigid_' + k for k in base] + ['rigid_inliers', 'rigid_angle_deg', 'rigid_trans']
    with pytest.raises(_lib.HplError):
        tr.validate(_NoSamples(), rigid={'iterations': 2})
