"""CPU: hpl_fps's declaration, export, refusals and workspace size (no device needed), the properties of the numpy restatement
tests/fps_oracle.py -- non-increasing distances, distinct indices, the covering radius, the k-centre bound, the tie rule, the stop
rule, overflow --, and the argument errors of ops.fps, flownet.fps_sample, data.KITTI(fps=...) and the engine's --fps."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import fps_oracle as FO

I64 = ctypes.c_int64
NAN, INF = float('nan'), float('inf')
BIG = (2 ** 31 + 2) // 3


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_fps\s*\(', body) and re.search(r'\bint64_t\s+hpl_fps_workspace_bytes\s*\(', body)
    assert re.search(r'\bint\s+hpl_fps_resident_capacity\s*\(', body)
    assert 'no NaN can arise' in hdr                          # the header says what an overflowing d2 is
    for name in ('hpl_fps', 'hpl_fps_workspace_bytes', 'hpl_fps_resident_capacity'):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    from hplflownet_amd import build, ops
    assert 'fps.hip' in build.SOURCES
    import hplflownet_amd
    assert hplflownet_amd.fps_sample is hplflownet_amd.flownet.fps_sample
    cap = ops.fps_resident_capacity()
    assert cap >= 8192 and cap % 64 == 0                      # a sampled cloud of the network's size fits one workgroup


# ----------------------------------------------------------------------------- the restatement's properties
def brute(pc, m, start=0):
    """Plain Python over float32 scalars: the definition once more, point by point."""
    n = pc.shape[1]
    D = [np.float32(np.inf)] * n
    idx, dist, s = [start], [np.float32(np.inf)], start
    while True:
        for i in range(n):
            dx, dy, dz = (pc[k, i] - pc[k, s] for k in range(3))
            D[i] = min(D[i], (dx * dx + dy * dy) + dz * dz)
        s = max(range(n), key=lambda i: (D[i], -i))
        if len(idx) == m or D[s] == 0:
            return idx, dist, D
        idx.append(s)
        dist.append(D[s])


def test_restatement_against_the_brute_force():
    for n, m, start in ((1, 3, 0), (2, 2, 1), (40, 40, 7), (150, 20, 0), (64, 70, 63)):
        pc = FO.cloud(n, 3 + n)
        o = FO.sample_cloud(pc, m, start=start)
        idx, dist, D = brute(pc, m, start)
        assert o['count'] == len(idx) == min(n, m) and o['idx'][:o['count']].tolist() == idx
        assert o['dist'][:o['count']].tobytes() == np.array(dist, np.float32).tobytes()
        assert o['cover'].tobytes() == np.array(D, np.float32).tobytes()
        assert (o['idx'][o['count']:] == -1).all() and not o['dist'][o['count']:].any()


@pytest.mark.parametrize('n,m', [(1000, 64), (8192, 512), (30000, 1024)])
def test_properties_and_the_k_centre_bound(n, m):
    pc = FO.cloud(n, n)
    attr = np.random.RandomState(1).normal(0, 1, (2, n)).astype(np.float32)
    o = FO.sample_cloud(pc, m, attr, start=n // 3)
    idx, dist, cover, count = o['idx'], o['dist'], o['cover'], o['count']
    assert count == m and idx[0] == n // 3 and dist[0] == np.inf
    assert (np.diff(dist[1:]) <= 0).all()                     # exactly: min is exact
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < n
    assert cover.max() <= dist[count - 1] and not cover[idx].any() and (cover >= 0).all()
    assert np.array_equal(o['out_pc'], pc[:, idx]) and np.array_equal(o['out_attr'], attr[:, idx])
    # the covering radius is each point's distance to its nearest sample, whatever the order of selection (float64 check)
    d = ((pc.astype(np.float64)[:, :, None] - pc.astype(np.float64)[:, None, idx[:64]]) ** 2).sum(axis=0).min(axis=1)
    assert (d >= cover.astype(np.float64) * (1 - 1e-5)).all()             # (64 of the m samples: an upper bound on cover)
    # FPS is a 2-approximation of the best covering radius, so its squared radius is at most 4 x that of ANY m-subset
    rng = np.random.RandomState(n)
    p64 = pc.astype(np.float64)
    sq = (p64 ** 2).sum(axis=0)
    for _ in range(5):
        sub = rng.choice(n, m, replace=False)
        d2 = sq[:, None] + sq[None, sub] - 2.0 * (p64.T @ p64[:, sub])       # float64: an error of 1e-12 against a margin of 10 x
        r2 = float(d2.min(axis=1).max())
        print('n %d m %d: squared covering radius %.4f, of a random subset %.4f, ratio %.3f' % (n, m, cover.max(), r2, cover.max() / r2))
        assert float(cover.max()) <= 4.0 * r2


def test_the_tie_rule_on_the_integer_grid():
    o = FO.sample_cloud(FO.grid(6), 8)
    assert o['idx'][:5].tolist() == [0, 215, 17, 102, 182]
    assert o['dist'][:5].tolist() == [INF, 75.0, 29.0, 29.0, 29.0]
    assert o['count'] == 8 and o['valid'] == 216 and o['nonfinite'] == 0
    full = FO.sample_cloud(FO.grid(6), 300)
    assert full['count'] == 216 and sorted(full['idx'][:216].tolist()) == list(range(216)) and (full['idx'][216:] == -1).all()
    assert full['dist'][215] == 1.0 and not full['cover'].any()


def test_the_stop_rule_and_the_start():
    five = FO.cloud(5, 9)
    pc = np.tile(five, (1, 4))                                # five positions, four times over
    o = FO.sample_cloud(pc, 10)
    assert o['count'] == 5 and sorted(o['idx'][:5].tolist()) == [0, 1, 2, 3, 4] and (o['idx'][5:] == -1).all()
    assert not o['dist'][5:].any() and not o['out_pc'][:, 5:].any() and not o['cover'].any() and (o['dist'][1:5] > 0).all()
    o = FO.sample_cloud(pc, 10, start=13)                     # a later copy starts: it is the sample, its twins never are
    assert o['count'] == 5 and o['idx'][0] == 13 and sorted((o['idx'][:5] % 5).tolist()) == [0, 1, 2, 3, 4]
    bad = pc.copy()
    bad[1, 0] = NAN
    bad[2, 7] = INF
    for start in (None, 0, 7):                                # a start that is not finite falls back to the smallest valid index
        o = FO.sample_cloud(bad, 10, start=start)
        assert o['idx'][0] == 1 and o['count'] == 5 and o['valid'] == 18 and o['nonfinite'] == 2
        assert 0 not in o['idx'] and 7 not in o['idx'] and o['cover'][0] == 0 and o['cover'][7] == 0
    assert FO.sample_cloud(bad, 10, start=3)['idx'][0] == 3
    none = np.full((3, 6), NAN, np.float32)
    o = FO.sample_cloud(none, 4, start=2)
    assert o['count'] == 0 and (o['idx'] == -1).all() and o['valid'] == 0 and o['nonfinite'] == 6 and not o['cover'].any()
    o = FO.sample_cloud(np.zeros((3, 0), np.float32), 4)
    assert o['count'] == 0 and (o['idx'] == -1).all() and o['cover'].shape == (0,)
    # an underflowing d2 is a coincidence too: 1e-30 apart, d2 = 0 in float32
    near = np.array([[0, 1e-30, 1.0], [0, 0, 0], [0, 0, 0]], np.float32)
    o = FO.sample_cloud(near, 3)
    assert o['count'] == 2 and o['idx'].tolist() == [0, 2, -1]


def test_overflow_is_an_ordinary_value():
    pc = np.array([[3e38, -3e38, 0.0, 3e38, 1.0], [0, 0, 0, 3e38, 0], [0, 0, 0, 0, 0]], np.float32)
    o = FO.sample_cloud(pc, 5)
    assert o['count'] == 5 and o['idx'].tolist() == [0, 1, 2, 3, 4]        # every d2 to 0 and to 1 is +inf: the smaller index
    assert o['dist'].tolist() == [INF, INF, INF, INF, 1.0] and not np.isnan(o['dist']).any() and not np.isnan(o['cover']).any()
    o = FO.sample_cloud(pc, 2)
    assert o['cover'].tolist() == [0.0, 0.0, INF, INF, INF]


def test_a_batch_is_its_clouds():
    parts = [FO.cloud(n, 40 + n) for n in (70, 0, 9)]
    pc, prefix = np.concatenate(parts, axis=1), [0, 70, 70, 79]
    attr = np.arange(79, dtype=np.float32)[None]
    o = FO.sample(pc, 12, attr, start=[5, 0, 8], prefix=prefix, path=2)
    assert o['idx'].shape == (3, 12) and o['out_pc'].shape == (3, 36) and o['out_attr'].shape == (1, 36) and o['cover'].shape == (79,)
    assert o['stats'].tolist() == [[12, 70, 0, 2], [0, 0, 0, 2], [9, 9, 0, 2]]
    assert o['idx'][0, 0] == 5 and o['idx'][2, 0] == 8 and (o['idx'][1] == -1).all() and (o['idx'][2, 9:] == -1).all()
    assert np.array_equal(o['out_attr'][0, 24:33], 70 + o['idx'][2, :9])  # the channel rides with its point


# ----------------------------------------------------------------------------- refusals without a device
def call(pc=4096, pc_ld=100, attr=None, attr_ld=100, channels=0, batch=1, prefix=(0, 100), start=None, m=10, path=0,
         idx=1 << 20, dist=2 << 20, out_pc=3 << 20, out_ld=None, out_attr=None, out_attr_ld=None, cover=4 << 20, stats=5 << 20,
         ws=6 << 20, ws_bytes=1 << 24):
    """hpl_fps with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    start = (ctypes.c_int32 * len(start))(*start) if start is not None else None
    M = max(batch, 0) * max(m, 0)
    return _lib.load().hpl_fps(pc, pc_ld, attr, attr_ld, channels, batch, prefix, start, m, path, idx, dist, out_pc,
                               M if out_ld is None else out_ld, out_attr, M if out_attr_ld is None else out_attr_ld, cover, stats,
                               ws, ws_bytes, None)


ATTR = dict(attr=7 << 20, channels=3, out_attr=8 << 20)
CAP = _lib.load().hpl_fps_resident_capacity()


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1), dict(channels=-1), dict(channels=9, attr=7 << 20),
    dict(channels=1), dict(path=3), dict(path=-1), dict(m=0), dict(m=-1), dict(m=BIG, out_ld=1 << 40, ws_bytes=1 << 40),
    dict(batch=2, prefix=(0, 50, 100), m=BIG // 2 + 1, out_ld=1 << 40), dict(m=2 ** 40, out_ld=1 << 50),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(prefix=None),
    dict(start=(100,)), dict(start=(-1,)), dict(batch=2, prefix=(0, 60, 100), start=(59, 40)),
    dict(pc_ld=99), dict(out_ld=9), dict(ATTR, attr_ld=99), dict(ATTR, out_attr_ld=9),
    dict(pc=None), dict(idx=None), dict(dist=None), dict(out_pc=None), dict(stats=None), dict(ws=None),
    dict(pc=4098), dict(idx=(1 << 20) + 2), dict(dist=(2 << 20) + 1), dict(out_pc=(3 << 20) + 3), dict(cover=(4 << 20) + 2),
    dict(stats=(5 << 20) + 1), dict(ATTR, attr=(7 << 20) + 2), dict(ATTR, out_attr=(8 << 20) + 1),
    dict(ws=(6 << 20) + 128), dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_fps_workspace_bytes(1, 100, 10, 0) - 1),
    dict(prefix=(0, BIG), pc_ld=2 ** 31, ws_bytes=1 << 40), dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
    dict(out_pc=4096), dict(out_pc=4096 + 4 * 299), dict(out_pc=4096 - 4 * 29), dict(idx=4096 + 4 * 150), dict(dist=4096),
    dict(cover=4096 + 4 * 299), dict(stats=4096 + 4 * 200), dict(ATTR, out_attr=4096), dict(ATTR, out_pc=(7 << 20) + 4 * 299),
    dict(ATTR, idx=(7 << 20) + 4 * 250), dict(ATTR, out_attr=(7 << 20) - 4 * 29),
    dict(path=1, prefix=(0, CAP + 1), pc_ld=CAP + 1), dict(path=1, batch=2, prefix=(0, 5, CAP + 6), pc_ld=CAP + 6),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_fps:')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments; the start of an empty cloud is ignored."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, start=(7, -3, 0), path=2, m=8192, cover=None, **ATTR) == 0
    assert call(batch=64, prefix=(0,) * 65, channels=8, attr=7 << 20, out_attr=None, path=1, m=1) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_fps_workspace_bytes
    assert f(0, 10, 1, 0) == -1 and f(65, 10, 1, 0) == -1 and f(-1, 10, 1, 0) == -1
    assert f(1, -1, 1, 0) == -1 and f(1, BIG, 1, 0) == -1 and f(1, 2 ** 40, 1, 0) == -1
    assert f(1, 10, 0, 0) == -1 and f(1, 10, -1, 0) == -1 and f(1, 10, BIG, 0) == -1 and f(64, 10, BIG // 64 + 1, 0) == -1
    assert f(1, 10, 1, -1) == -1 and f(1, 10, 1, 9) == -1
    assert f(1, BIG - 1, BIG - 1, 8) > 0 and f(64, 0, 1, 0) >= 0 and f(64, 10, (BIG - 1) // 64, 0) > 0
    ns = [0, 1, 3, 1024, 1025, 8192, 100191, 450000, 2 ** 29]
    for b in (1, 2, 16, 64):
        vals = [f(b, n, 8192, 3) for n in ns]
        assert all(v >= 0 and v % 256 == 0 for v in vals) and vals == sorted(vals)
        assert all(f(b + 1, n, 8192, 3) >= f(b, n, 8192, 3) for n in ns if b < 64)
    assert f(1, 450000, 8192, 8) < 2 << 20                    # four bytes a point and the candidate keys


# ----------------------------------------------------------------------------- the Python layers' argument errors
def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        ops.fps(pc, 4)                                        # a host tensor: no CPU fallback
    assert ops.fps_args('x', 7, 64, 'rounds') == (7, 2) and ops.fps_args('x', BIG - 1, 1) == (BIG - 1, 0)
    for m, batch, path in ((0, 1, 'auto'), (-3, 1, 'auto'), (True, 1, 'auto'), (2.0, 1, 'auto'), ('4', 1, 'auto'), (None, 1, 'auto'),
                           (BIG, 1, 'auto'), (BIG // 64 + 1, 64, 'auto'), (4, 1, 'fast'), (4, 1, 1), (4, 1, None)):
        with pytest.raises(_lib.HplError) as e:
            ops.fps_args('who', m, batch, path)
        assert str(e.value).startswith('who: ')


def test_fps_sample_refuses_host_tensors_and_bad_forms():
    from hplflownet_amd import flownet
    a = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        flownet.fps_sample(a, a, num_points=4)                # host tensors
    for args, kw in (((a, torch.zeros(3, 9)), {}), ((a, a, torch.zeros(3, 9)), {}), (([a], [a, a]), {}),
                     ((a, None, torch.zeros(3, 9)), {}), ((torch.zeros(10, 3), a), {}), (([],), {}),
                     (([a] * 33, [a] * 33), dict(corr=False)), (([a] * 65, [a] * 65), {}), (([a] * 65,), {}),
                     ((a, a), dict(num_points=0)), ((a, a), dict(num_points=2.5)), ((a, a), dict(num_points=True)),
                     ((a, a), dict(num_points=BIG)), ((a, a), dict(start=[0], seed=1)), ((a, a), dict(seed=-1)),
                     ((a, a), dict(seed=1.5))):
        with pytest.raises(_lib.HplError) as e:
            flownet.fps_sample(*args, **kw)
        assert 'host' not in str(e.value) and 'device tensor' not in str(e.value), (args, kw)


def test_engine_argument_errors():
    from hplflownet_amd import engine
    base = ['--dataset', 'KITTI', '--evaluate', '--data-root', '/nowhere']
    assert engine.parse_args(base).fps is None and engine.parse_args([]).fps is None
    assert engine.parse_args(base + ['--fps', '2048']).fps == 2048
    a = engine.parse_args(base + ['--fps', '1', '--voxel', '0.3', '--ground', 'plane'])
    assert a.fps == 1 and a.voxel == 0.3
    for extra in (['--fps', '2048'], ['--dataset', 'FlyingThings3DSubset', '--data-root', '/nowhere', '--fps', '2048'],
                  base + ['--fps', '0'], base + ['--fps', '-4'], base + ['--fps', '2.5'], base + ['--fps', 'x'], base + ['--fps']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


def test_reader_refuses_fps_on_a_cpu_device(tmp_path):
    from hplflownet_amd import data
    d = tmp_path / 'KITTI_processed_occ_final' / '000000'
    d.mkdir(parents=True)
    pc = FO.cloud(64, 0, extent=3.0).T.copy()
    np.save(str(d / 'pc1.npy'), pc)
    np.save(str(d / 'pc2.npy'), pc)
    for kw in (dict(device='cpu', fps=16), dict(device='cuda', fps=0), dict(device='cuda', fps=-1), dict(device='cuda', fps=2.0),
               dict(device='cuda', fps=True), dict(device='cuda', fps='16')):
        with pytest.raises(_lib.HplError) as e:
            data.KITTI(None, str(tmp_path), **kw)
        assert 'fps' in str(e.value)
    plain = data.KITTI(None, str(tmp_path), device='cpu')      # off by default: the reference's reader, on any device
    assert plain.fps is None
    o1, o2 = plain.load(str(d))
    keep = ~((pc[:, 1] < -1.4) & (pc[:, 1] < -1.4))
    assert np.array_equal(o1, pc[keep]) and np.array_equal(o2, pc[keep])
