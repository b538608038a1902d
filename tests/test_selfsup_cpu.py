"""CPU: hpl_selfsup_loss's declaration, export and refusals (no device needed), the numpy restatement tests/selfsup_oracle.py
against finite differences and on its edge cases, the engine's --loss arguments and the trainer's choice of loss."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
from selfsup_oracle import nearest, pair, selfsup

I64 = ctypes.c_int64


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_selfsup_loss\s*\(', body)
    assert re.search(r'\bint64_t\s+hpl_selfsup_loss_workspace_bytes\s*\(', body)
    assert 'hpl_selfsup_loss' in _lib.EXPORTS and 'hpl_selfsup_loss_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_selfsup_loss') and hasattr(_lib.load(), 'hpl_selfsup_loss_workspace_bytes')
    from hplflownet_amd import build
    assert 'selfsup_loss.hip' in build.SOURCES


PC1, FLOW, PC2, LOSS, DFLOW, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x100000


def call(pc1=PC1, ld1=100, flow=FLOW, sc=1, sp=3, pc2=PC2, ld2=100, batch=1, prefix1=(0, 100), prefix2=(0, 100), k=8, wc=1.0,
         ws_=1.0, loss=LOSS, dflow=DFLOW, nn12=None, nn21=None, nbr=None, ws=WS, ws_bytes=1 << 24):
    """hpl_selfsup_loss with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix1 = (I64 * len(prefix1))(*prefix1) if prefix1 is not None else None
    prefix2 = (I64 * len(prefix2))(*prefix2) if prefix2 is not None else None
    return _lib.load().hpl_selfsup_loss(pc1, ld1, flow, sc, sp, pc2, ld2, batch, prefix1, prefix2, k, wc, ws_, loss, dflow, nn12,
                                        nn21, nbr, ws, ws_bytes, None)


BIG = 2 ** 31 // 3 + 1


@pytest.mark.parametrize('kw', [
    # ranges
    dict(batch=0), dict(batch=65, prefix1=(0,) * 66, prefix2=(0,) * 66), dict(batch=-1), dict(k=-1), dict(k=9),
    dict(k=0), dict(wc=-1.0), dict(ws_=-0.5), dict(wc=float('inf')), dict(ws_=float('inf')),
    # NaN weights
    dict(wc=float('nan')), dict(ws_=float('nan')),
    # a bad prefix
    dict(prefix1=(1, 100)), dict(prefix2=(1, 100)), dict(batch=2, prefix1=(0, 60, 50), prefix2=(0, 50, 100)),
    dict(batch=2, prefix1=(0, 50, 100), prefix2=(0, 60, 50)),
    # ld below its count
    dict(ld1=99), dict(ld2=99),
    # flow strides
    dict(sc=0), dict(sp=0), dict(sc=-1), dict(sc=50, sp=1), dict(sc=1, sp=2),
    # null or misaligned arrays
    dict(pc1=None), dict(flow=None), dict(pc2=None), dict(loss=None), dict(prefix1=None), dict(prefix2=None), dict(ws=None),
    dict(pc1=PC1 + 2), dict(flow=FLOW + 1), dict(pc2=PC2 + 2), dict(loss=LOSS + 3), dict(dflow=DFLOW + 2), dict(nn12=6),
    dict(nn21=5), dict(nbr=7), dict(ws=WS + 128),
    # a short workspace
    dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_selfsup_loss_workspace_bytes(1, 100, 100, 8) - 1),
    # counts >= 2^31 / 3 (and k N1 >= 2^31)
    dict(prefix1=(0, BIG), ld1=2 ** 31, ws_bytes=1 << 50), dict(prefix2=(0, BIG), ld2=2 ** 31, ws_bytes=1 << 50),
    dict(prefix1=(0, 2 ** 60), ld1=2 ** 60, ws_bytes=1 << 62), dict(prefix1=(0, 2 ** 29), ld1=2 ** 29, k=4, ws_bytes=1 << 50),
    # dflow overlapping an input
    dict(dflow=PC1 + 4), dict(dflow=PC1 - 4), dict(dflow=FLOW), dict(dflow=PC2 + 8), dict(dflow=PC1 + 4 * 250, ld1=1000),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert b'hpl_selfsup_loss' in _lib.load().hpl_last_error()


def test_accepted_arguments_reach_no_launch_when_empty():
    """N1 = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(prefix1=(0, 0), ld1=0) == 0
    assert call(prefix1=(0, 0), ld1=0, prefix2=(0, 0), ld2=0, dflow=None) == 0
    assert call(batch=3, prefix1=(0, 0, 0, 0), prefix2=(0, 10, 10, 100), ld1=0, k=0, ws_=0.0, wc=0.0, sc=7, sp=1) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_selfsup_loss_workspace_bytes
    assert f(0, 10, 10, 8) == -1 and f(65, 10, 10, 8) == -1 and f(1, -1, 10, 8) == -1 and f(1, 10, -1, 8) == -1
    assert f(1, 10, 10, -1) == -1 and f(1, 10, 10, 9) == -1 and f(1, BIG, 10, 1) == -1 and f(1, 10, BIG, 1) == -1
    assert f(1, 2 ** 29, 10, 4) == -1 and f(1, 2 ** 29, 10, 3) > 0
    ns = [0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 131072, 450000, 2 ** 27]
    for b in (1, 2, 16, 64):
        for k in (0, 1, 3, 8):
            for n_fixed in (0, 1000):
                v1 = [f(b, n, n_fixed, k) for n in ns]
                v2 = [f(b, n_fixed, n, k) for n in ns]
                assert all(v > 0 and v % 256 == 0 for v in v1 + v2) and v1 == sorted(v1) and v2 == sorted(v2)
            assert all(f(b + 1, n, n, k) >= f(b, n, n, k) for n in ns if b < 64)
            assert all(f(b, n, n, k + 1) >= f(b, n, n, k) for n in ns if k < 8)
    assert f(16, 131072, 131072, 8) < 64 << 20


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc, fl = torch.zeros(3, 10), torch.zeros(10, 3)
    with pytest.raises(_lib.HplError):
        ops.selfsup_loss(pc, fl, pc)                          # host tensors: no CPU fallback
    for kw in (dict(k=-1), dict(k=9), dict(k=2.0), dict(k=True), dict(k=0), dict(w_chamfer=-1.0), dict(w_smooth=float('nan')),
               dict(w_chamfer=float('inf')), dict(w_smooth='x')):
        with pytest.raises(_lib.HplError):
            ops.selfsup_loss(pc, fl, pc, **kw)


# ----------------------------------------------------------------------------- the restatement
def grid_pair(seed=0):
    """40 points on a jittered 5 x 4 x 2 grid of spacing 1, a small flow, and pc2 = the warped cloud moved a little: every
    nearest point is about 0.05 away, every runner-up about 1."""
    rng = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(4.0), np.arange(2.0), indexing='ij')).reshape(3, -1)
    x = (g + rng.uniform(-0.15, 0.15, g.shape)).astype(np.float32)
    f = rng.uniform(-0.05, 0.05, g.shape).astype(np.float32)
    q = (x + f + rng.uniform(-0.04, 0.04, g.shape))[:, rng.permutation(40)].astype(np.float32)
    return x, f, q


def margins(x, f, q):
    """The smallest gap between the nearest and the second d2 of both Chamfer directions, and between consecutive d2 of the
    graph's k + 1 nearest (float64)."""
    p = x.astype(np.float64) + f
    gaps = []
    for a, b in ((p, q.astype(np.float64)), (q.astype(np.float64), p)):
        d = np.sort(((a[:, :, None] - b[:, None, :]) ** 2).sum(0), axis=1)
        gaps.append((d[:, 1] - d[:, 0]).min())
    d = ((x[:, :, None].astype(np.float64) - x[:, None, :]) ** 2).sum(0)
    np.fill_diagonal(d, np.inf)
    gaps.append(np.diff(np.sort(d, axis=1)[:, :9], axis=1).min())
    return gaps


def test_oracle_gradient_against_finite_differences():
    """Central differences of the oracle's L (evaluated in float64) in EVERY flow component of a 40-point pair.  The loss is
    quadratic in the flow while the assignments hold, so the central difference is exact up to rounding."""
    x, f, q = grid_pair()
    k, wc, ws, h = 8, 0.75, 1.5, 1e-3
    gaps = margins(x, f, q)
    print('smallest d2 gaps: p->q %.3g, q->p %.3g, graph %.3g' % tuple(gaps))
    # a flow step of h moves a Chamfer d2 by about 2 |d| h <= 2 * 2 * 1e-3: the runner-up is >= 10 x that away
    assert gaps[0] >= 0.04 and gaps[1] >= 0.04 and gaps[2] > 1e-6
    f64 = f.astype(np.float64)

    def run(flow64):
        o = pair(x, flow64, q, k, wc, ws, real=np.float64)
        return {'L': o['L'], 'dflow64': o['dflow'], 'nn12': o['nn12'], 'nn21': o['nn21'], 'nbr': o['nbr']}
    base = run(f64)
    g = base['dflow64']
    worst = 0.0
    for i in range(40):
        for c in range(3):
            lo, hi = f64.copy(), f64.copy()
            lo[c, i] -= h
            hi[c, i] += h
            a, b = run(lo), run(hi)
            for key in ('nn12', 'nn21', 'nbr'):
                assert np.array_equal(a[key], base[key]) and np.array_equal(b[key], base[key]), (i, c, key)
            fd = (b['L'] - a['L']) / (2 * h)
            worst = max(worst, abs(fd - g[i, c]))
    bar = 1e-9 * np.abs(g).max()
    print('largest |fd - grad| %.3g, bar %.3g (max |grad| %.3g)' % (worst, bar, np.abs(g).max()))
    assert worst <= bar
    # and the float32 entry point agrees with the real-number evaluation to float32 accuracy
    o32 = selfsup(x, f, q, k, wc, ws)
    assert np.abs(o32['dflow64'] - g).max() <= 1e-5 * np.abs(g).max() and abs(o32['loss64'][0, 0] - base['L']) <= 1e-5 * base['L']
    for key in ('nn12', 'nn21', 'nbr'):
        assert np.array_equal(o32[key], base[key])


def test_oracle_duplicates_ties_and_self_exclusion():
    # points 0 and 1 coincide, 2 and 3 are equally far from them
    x = np.array([[0, 0, 1, -1, 5], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float32)
    idx, d2 = nearest(x, x, 3, exclude_self=True)
    assert idx[:, 0].tolist() == [1, 2, 3] and idx[:, 1].tolist() == [0, 2, 3]        # the twin at distance 0 is a neighbour
    assert d2[0, 0] == 0 and d2[0, 1] == 0
    assert idx[:, 2].tolist() == [0, 1, 3] and idx[:, 4].tolist() == [2, 0, 1]        # ties go to the smaller index
    f = np.zeros_like(x)
    o = selfsup(x, f, x, k=3)
    assert o['nn12'].tolist() == [0, 0, 2, 3, 4] and o['nn21'].tolist() == [0, 0, 2, 3, 4]
    assert np.array_equal(o['loss'], np.zeros((1, 4), np.float32)) and not o['dflow'].any()


def test_oracle_small_pairs_and_empty_sides():
    rng = np.random.RandomState(3)
    x, f, q = (rng.normal(size=(3, 2)).astype(np.float32) for _ in range(3))
    o = selfsup(x, f, q, k=8)                                 # fewer than k + 1 points: k_i = 1
    assert o['nbr'][:, 0].tolist() == [1] + [-1] * 7 and o['nbr'][:, 1].tolist() == [0] + [-1] * 7
    d = (f[:, 0].astype(np.float64) - f[:, 1]) ** 2
    assert abs(o['loss64'][0, 3] - d.sum()) <= 1e-15 * d.sum()
    o1 = selfsup(x[:, :1], f[:, :1], q, k=8)                  # one point: no neighbour, S = 0
    assert o1['loss64'][0, 3] == 0 and (o1['nbr'] == -1).all() and np.isfinite(o1['dflow64']).all()
    o2 = selfsup(x, f, q[:, :0], k=2)                         # N2 = 0
    assert o2['loss64'][0, 1] == 0 and o2['loss64'][0, 2] == 0 and (o2['nn12'] == -1).all()
    assert o2['loss64'][0, 0] == o2['loss64'][0, 3] and np.isfinite(o2['dflow64']).all() and o2['dflow64'].any()
    o3 = selfsup(x[:, :0], f[:, :0], q, k=2)                  # N1 = 0
    assert not o3['loss64'].any() and (o3['nn21'] == -1).all() and o3['dflow'].shape == (0, 3)
    o4 = selfsup(x, f, q, k=0, ws=0.0)                        # no graph
    assert o4['loss64'][0, 3] == 0 and o4['nbr'].shape == (0, 2)
    assert o4['loss64'][0, 0] == o4['loss64'][0, 1] + o4['loss64'][0, 2]
    full = selfsup(x, f, q, k=2, ws=0.0)
    assert np.array_equal(full['dflow64'], o4['dflow64'])
    # batches: a pair's results do not depend on its place
    xb, fb, qb = np.concatenate([x, x[:, :1]], 1), np.concatenate([f, f[:, :1]], 1), np.concatenate([q[:, :0], q], 1)
    ob = selfsup(xb, fb, qb, k=8, prefix1=[0, 2, 2, 3], prefix2=[0, 0, 0, 2])
    assert np.array_equal(ob['loss64'][0], selfsup(x, f, q[:, :0], k=8)['loss64'][0]) and not ob['loss64'][1].any()
    assert np.array_equal(ob['loss64'][2], o1['loss64'][0]) and np.array_equal(ob['dflow64'][2:], o1['dflow64'])


# ----------------------------------------------------------------------------- engine
def test_engine_argument_errors():
    from hplflownet_amd import engine
    assert engine.parse_args([]).loss == 'epe3d' and engine.parse_args([]).selfsup is None
    assert engine.parse_args(['--loss', 'selfsup']).selfsup == {'k': 8, 'w_chamfer': 1.0, 'w_smooth': 1.0}
    a = engine.parse_args(['--loss', 'selfsup', '--selfsup-k', '3', '--selfsup-chamfer-weight', '0.5',
                           '--selfsup-smooth-weight', '0'])
    assert a.selfsup == {'k': 3, 'w_chamfer': 0.5, 'w_smooth': 0.0}
    for extra in (['--selfsup-k', '3'], ['--selfsup-chamfer-weight', '1'], ['--selfsup-smooth-weight', '1'],
                  ['--loss', 'epe3d', '--selfsup-k', '3'], ['--loss', 'chamfer'], ['--loss', 'selfsup', '--selfsup-k', '0'],
                  ['--loss', 'selfsup', '--selfsup-k', '9'], ['--loss', 'selfsup', '--selfsup-chamfer-weight', '-1'],
                  ['--loss', 'selfsup', '--selfsup-smooth-weight', 'nan'], ['--loss', 'selfsup', '--selfsup-smooth-weight', 'inf'],
                  ['--loss', 'selfsup', '--evaluate']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


def test_trainer_refuses_an_unknown_loss():
    from hplflownet_amd import engine
    with pytest.raises(_lib.HplError):
        engine.Trainer('HPLFlowNetShallow', 'cpu', loss='nope')
    for bad in (dict(loss='epe3d', selfsup={'k': 3}), dict(loss='selfsup', selfsup={'K': 3}), dict(loss='selfsup', selfsup={'k': 9}),
                dict(loss='selfsup', selfsup={'w_smooth': float('nan')}), dict(loss='selfsup', selfsup={'k': 0})):
        with pytest.raises(_lib.HplError):
            engine.Trainer('HPLFlowNetShallow', 'cpu', **bad)
    assert engine.selfsup_options('selfsup', {'k': 4}) == {'k': 4, 'w_chamfer': 1.0, 'w_smooth': 1.0}
    assert engine.selfsup_options('selfsup', {'k': 0, 'w_smooth': 0}) == {'k': 0, 'w_chamfer': 1.0, 'w_smooth': 0.0}
    assert engine.selfsup_options('epe3d', None) is None


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((3, 1), 0.5))

    def forward(self, pc1, pc2, lat):
        return pc1 * self.w


class _Poison(object):
    """Any use of the ground-truth flow fails the test."""

    def __getattr__(self, name):
        raise AssertionError('the self-supervised step read sf.%s' % name)

    def __getitem__(self, i):
        raise AssertionError('the self-supervised step indexed sf')


def test_selfsup_step_never_reads_sf(monkeypatch):
    """Trainer.train_step with loss='selfsup' on a stub model and a stub of the device loss: the loss is called with the
    trainer's options and the ground-truth flow is never touched (a poisoned object, then a tensor of NaN)."""
    from hplflownet_amd import engine
    calls = []

    def fake_loss(flow, pc1, pc2, **kw):
        calls.append(kw)
        assert tuple(pc1.shape) == (1, 3, 6) and tuple(pc2.shape) == (1, 3, 5) and tuple(flow.shape) == (1, 3, 6)
        return (flow - pc2.mean()).square().mean(), None
    monkeypatch.setattr(engine, 'selfsup_loss', fake_loss)
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = _Stub(), torch.device('cpu')
    tr.loss, tr.selfsup = 'selfsup', engine.selfsup_options('selfsup', {'k': 3})
    tr.native_step, tr.tplan, tr.reducer = False, None, None
    tr.opt = torch.optim.Adam(tr.model.parameters(), lr=1e-2)
    pc1, pc2 = torch.randn(3, 6), torch.randn(3, 5)
    lat = object()
    before = tr.model.w.detach().clone()
    for sf in (_Poison(), torch.full((3, 6), float('nan'))):
        loss = tr.train_step(pc1, pc2, sf, lat)
        assert torch.isfinite(loss) and torch.isfinite(tr.model.w).all()
    assert not torch.equal(tr.model.w.detach(), before)
    assert calls == [{'k': 3, 'w_chamfer': 1.0, 'w_smooth': 1.0}] * 2
    tr.loss = 'epe3d'                                         # the default path does read it
    with pytest.raises(AssertionError):
        tr.train_step(pc1, pc2, _Poison(), lat)
