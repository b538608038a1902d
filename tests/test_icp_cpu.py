"""CPU: hpl_icp's declaration, export and refusals (no device needed), its workspace arithmetic, the numpy restatement
tests/icp_oracle.py (the vectorised match against a plain double loop, ties included; the scene the GPU tests use converges
from identity), the wrapper's refusals and the engine's --baseline icp arguments and key set."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import icp_oracle as O

I64 = ctypes.c_int64
BIG = 2 ** 31 // 3 + 1


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_icp\s*\(', body) and re.search(r'\bint64_t\s+hpl_icp_workspace_bytes\s*\(', body)
    assert 'hpl_icp' in _lib.EXPORTS and 'hpl_icp_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_icp') and hasattr(_lib.load(), 'hpl_icp_workspace_bytes')
    from hplflownet_amd import build
    assert 'icp.hip' in build.SOURCES


def call(src=256, src_ld=100, dst=512, dst_ld=80, weight=None, init=None, batch=1, sprefix=(0, 100), dprefix=(0, 80), iters=4,
         max_dist=1.0, tau=0.3, tol_rot=0.0, tol_trans=0.0, Rt=768, stats=1024, match=None, dist2=None, flow=1280, ws=4096,
         ws_bytes=1 << 24):
    """hpl_icp with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    sprefix = (I64 * len(sprefix))(*sprefix) if sprefix is not None else None
    dprefix = (I64 * len(dprefix))(*dprefix) if dprefix is not None else None
    return _lib.load().hpl_icp(src, src_ld, dst, dst_ld, weight, init, batch, sprefix, dprefix, iters, max_dist, tau, tol_rot,
                               tol_trans, Rt, stats, match, dist2, flow, ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(src=None), dict(dst=None), dict(Rt=None), dict(stats=None), dict(sprefix=None), dict(dprefix=None), dict(ws=None),
    dict(batch=0), dict(batch=65, sprefix=(0,) * 66, dprefix=(0,) * 66), dict(batch=-1),
    dict(iters=-1), dict(iters=65),
    dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float('inf')), dict(max_dist=float('nan')),
    dict(tau=0.0), dict(tau=-0.1), dict(tau=float('inf')), dict(tau=float('nan')),
    dict(tol_rot=-1e-6), dict(tol_trans=-1e-6), dict(tol_rot=float('nan')), dict(tol_trans=float('nan')),
    dict(sprefix=(1, 100)), dict(dprefix=(1, 80)),
    dict(batch=2, sprefix=(0, 60, 50), dprefix=(0, 40, 80)), dict(batch=2, sprefix=(0, 50, 100), dprefix=(0, 50, 40)),
    dict(src_ld=99), dict(dst_ld=79),
    dict(src=258), dict(dst=513), dict(weight=9), dict(init=6), dict(Rt=770), dict(stats=1027), dict(match=5), dict(dist2=7),
    dict(flow=1282),
    dict(ws=4096 + 128), dict(ws=4100), dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_icp_workspace_bytes(1, 100, 80) - 1),
    dict(sprefix=(0, BIG), src_ld=2 ** 31, ws_bytes=1 << 50), dict(dprefix=(0, BIG), dst_ld=2 ** 31, ws_bytes=1 << 50),
    dict(sprefix=(0, 2 ** 60), src_ld=2 ** 60, ws_bytes=1 << 62), dict(dprefix=(0, 2 ** 60), dst_ld=2 ** 60, ws_bytes=1 << 62),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_icp')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(sprefix=(0, 0), src_ld=0) == 0
    assert call(sprefix=(0, 0), src_ld=0, dprefix=(0, 0), dst_ld=0, dst=None, iters=0, tol_rot=1.0, tol_trans=float('inf')) == 0
    assert call(batch=3, sprefix=(0, 0, 0, 0), dprefix=(0, 80, 80, 80), iters=64, max_dist=1e-3, tau=1e3, flow=None) == 0
    assert call(sprefix=(0, 0), src_ld=0, ws_bytes=_lib.load().hpl_icp_workspace_bytes(1, 0, 80)) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_icp_workspace_bytes
    assert f(0, 10, 10) == -1 and f(65, 10, 10) == -1 and f(-1, 10, 10) == -1
    assert f(1, -1, 10) == -1 and f(1, 10, -1) == -1 and f(1, BIG, 10) == -1 and f(1, 10, BIG) == -1 and f(1, 2 ** 60, 1) == -1
    assert f(1, BIG - 1, BIG - 1) > 0 and f(64, 0, 0) > 0
    ns = [0, 1, 3, 255, 1024, 1025, 8192, 8193, 100191, 450000, 2 ** 27]
    for b in (1, 2, 16, 64):
        for fixed in (0, 1025, 450000):
            by_src = [f(b, n, fixed) for n in ns]
            by_dst = [f(b, fixed, n) for n in ns]
            assert all(v > 0 and v % 256 == 0 for v in by_src + by_dst)
            assert by_src == sorted(by_src) and by_dst == sorted(by_dst)
            assert all(f(b + 1, n, fixed) >= f(b, n, fixed) for n in ns if b < 64)
    assert f(1, 450000, 450000) < 64 << 20                    # 48 bytes per dst point and the sort's room


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    a, b = torch.zeros(3, 10), torch.zeros(3, 12)
    with pytest.raises(_lib.HplError):
        ops.icp(a, b)                                         # host tensors: no CPU fallback
    for kw in (dict(iters=-1), dict(iters=65), dict(iters=2.0), dict(iters=True), dict(max_dist=0.0), dict(max_dist=float('inf')),
               dict(tau=0.0), dict(tau=float('nan')), dict(tol_rot=-1.0), dict(tol_trans=float('nan'))):
        with pytest.raises(_lib.HplError):
            ops.icp(a, b, **kw)


# ----------------------------------------------------------------------------- the restatement
def loop_match(src, dst, R, t, max_dist):
    """The match by a plain double loop over scalars: float32 arithmetic one operation at a time."""
    f = np.float32
    R64, t64 = np.asarray(R, f).astype(np.float64), np.asarray(t, f).astype(np.float64)
    md2 = f(f(max_dist) * f(max_dist))
    inv = 1.0 / (1.001 * np.float64(f(max_dist)))
    n, m = src.shape[1], dst.shape[1]
    idx, d2o = np.full(n, -1, np.int32), np.full(n, np.inf, f)

    def cell_ok(v):
        return all(np.isfinite(x) and abs(np.floor(np.float64(x) * inv)) <= 2 ** 18 - 2 for x in v)

    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            p = src[:, i].astype(np.float64)
            q = [f(((R64[k, 0] * p[0] + R64[k, 1] * p[1]) + R64[k, 2] * p[2]) + t64[k]) for k in range(3)]
            if not cell_ok(q):
                continue
            best, bj = f(np.inf), -1
            for j in range(m):
                if not cell_ok(dst[:, j]):
                    continue
                dx, dy, dz = f(q[0] - dst[0, j]), f(q[1] - dst[1, j]), f(q[2] - dst[2, j])
                d2 = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
                if d2 < best:                                 # ascending j: a tie keeps the smaller index
                    best, bj = d2, j
            if bj >= 0 and best <= md2:
                idx[i], d2o[i] = bj, best
    return idx, d2o


def small_clouds(seed, n, m):
    """Clouds on a coarse lattice of positions (many exact ties and duplicates), with non-finite and far points."""
    rng = np.random.RandomState(seed)
    src = (rng.randint(-6, 7, (3, n)) * 0.25).astype(np.float32)
    dst = (rng.randint(-6, 7, (3, m)) * 0.25).astype(np.float32)
    if m >= 8:
        dst[:, 3] = dst[:, 1]                                 # duplicates
        dst[0, 4] = np.nan
        dst[2, 5] = np.inf
        dst[:, 6] = 1e7
    if n >= 8:
        src[1, 2] = np.nan
        src[:, 3] = -1e7
        src[0, 4] = -np.inf
    return src, dst


@pytest.mark.parametrize('n,m,seed', [(1, 1, 0), (3, 5, 1), (40, 60, 2), (61, 33, 3)])
@pytest.mark.parametrize('motion', ['identity', 'moved'])
def test_vectorised_match_equals_the_double_loop(n, m, seed, motion):
    src, dst = small_clouds(seed, n, m)
    R, t = O.IDENTITY if motion == 'identity' else (O.rotation((0, 0, 1), np.pi / 2).astype(np.float32),
                                                     np.array([0.25, -0.5, 0.0], np.float32))
    for max_dist in (0.25, 0.6, 3.0):
        a, b = O.match(src, dst, R, t, max_dist), loop_match(src, dst, R, t, max_dist)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    if n >= 8 and motion == 'identity':
        idx, d2 = O.match(src, dst, R, t, 3.0)
        assert (idx[[2, 3, 4]] == -1).all() and np.isinf(d2[[2, 3, 4]]).all()
        assert not np.isin(idx, [3, 4, 5, 6]).any()          # the duplicate loses its ties; the others take no part
        assert (idx >= 0).sum() >= n - 3


def test_a_point_exactly_at_max_dist_is_accepted():
    src = np.zeros((3, 1), np.float32)
    dst = np.array([[0.5, 0.5000001], [0, 0], [0, 0]], np.float32)
    idx, d2 = O.match(src, dst, *O.IDENTITY, 0.5)
    assert idx[0] == 0 and d2[0] == np.float32(0.25)
    idx, _ = O.match(src, dst[:, 1:], *O.IDENTITY, 0.5)
    assert idx[0] == -1


@pytest.mark.parametrize('n', [300, 1025])
def test_scene_converges_from_identity(n):
    """The scene of the GPU tests: the chained restatement reaches a bitwise fixpoint within a few rounds and lands at least
    ten times nearer the true motion than identity is."""
    src, dst = O.scene(n, n)
    c = O.chain(src, dst, iters=30)
    eR, et = np.abs(c['R32'] - O.TRUE_R).max(), np.abs(c['t32'] - O.TRUE_T).max()
    print('n = %d: %d rounds, R off by %.3g, t by %.3g m' % (n, c['rounds'], eR, et))
    assert c['status'] == 1 and c['rounds'] < 30
    assert eR <= 0.1 * np.abs(np.eye(3) - O.TRUE_R).max() and et <= 0.1 * np.abs(O.TRUE_T).max()
    again = O.round_(src, dst, c['R32'], c['t32'])
    assert np.array_equal(again['R32'], c['R32']) and np.array_equal(again['t32'], c['t32'])


def test_degenerate_inputs_fail_and_keep_the_motion():
    src, dst = O.scene(50, 1)
    init = (O.TRUE_R.astype(np.float32), O.TRUE_T.astype(np.float32))
    for s, d, w in ((src[:, :2], dst, None), (src[:, :0], dst, None), (src, dst[:, :0], None), (src, dst + 100, None),
                    (src, dst, np.zeros(50, np.float32)), (src, dst, np.full(50, np.nan, np.float32))):
        c = O.chain(s, d, init=init, iters=5, w=w)
        assert c['status'] == 0 and np.array_equal(c['R32'], init[0]) and np.array_equal(c['t32'], init[1])


# ----------------------------------------------------------------------------- engine
def test_engine_argument_errors():
    from hplflownet_amd import engine
    ok = engine.parse_args(['--evaluate', '--baseline', 'icp'])
    assert ok.icp == {'iters': 30, 'max_dist': 1.0, 'tau': 0.3, 'init': 'identity'}
    got = engine.parse_args(['--evaluate', '--baseline', 'icp', '--icp-iters', '0', '--icp-max-dist', '0.5', '--icp-tau', '0.1',
                             '--icp-init', 'rigid', '--rigid-refine'])
    assert got.icp == {'iters': 0, 'max_dist': 0.5, 'tau': 0.1, 'init': 'rigid'}
    assert engine.parse_args(['--evaluate']).icp is None
    base = ['--evaluate', '--baseline', 'icp']
    for extra in (['--baseline', 'icp'], ['--evaluate', '--baseline', 'ndt'], ['--evaluate', '--icp-iters', '3'],
                  ['--evaluate', '--icp-max-dist', '1'], ['--evaluate', '--icp-tau', '0.3'], ['--evaluate', '--icp-init', 'identity'],
                  base + ['--icp-iters', '65'], base + ['--icp-iters', '-1'], base + ['--icp-max-dist', '0'],
                  base + ['--icp-max-dist', 'inf'], base + ['--icp-max-dist', 'nan'], base + ['--icp-tau', '0'],
                  base + ['--icp-tau', '-1'], base + ['--icp-tau', 'nan'], base + ['--icp-init', 'rigid'],
                  base + ['--icp-init', 'flow']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


class _NoSamples(object):
    has_cameras = True

    def __len__(self):
        return 0


def test_validate_key_set_on_a_stub():
    """An empty shard reports (and would reduce) the reader's keys: without icp exactly the keys of before."""
    from hplflownet_amd import engine
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
    base = ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert list(tr.validate(_NoSamples(), icp=None)) == base
    res = tr.validate(_NoSamples(), icp={'iters': 2})
    assert list(res) == base + ['icp_' + k for k in base] + ['icp_matched', 'icp_rmse', 'icp_angle_deg', 'icp_trans', 'icp_rounds']
    res = tr.validate(_NoSamples(), rigid={'iters': 2, 'tau': 0.1}, icp={'init': 'rigid'})
    assert list(res)[-11:] == ['icp_' + k for k in base] + ['icp_matched', 'icp_rmse', 'icp_angle_deg', 'icp_trans', 'icp_rounds']
    for bad in ({'iterations': 2}, {'init': 'rigid'}, {'init': 'flow'}):
        with pytest.raises(_lib.HplError):
            tr.validate(_NoSamples(), icp=bad)
