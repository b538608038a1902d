"""CPU: hpl_voxel_downsample's declaration, export and refusals (no device needed), its workspace size, the numpy restatement
tests/voxel_oracle.py against a dictionary-of-lists brute force and on the cell edges, and the argument errors of
flownet.voxel_downsample, data.KITTI(voxel=...) and the engine's --voxel."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import voxel_oracle as VO

I64 = ctypes.c_int64
NAN, INF = float('nan'), float('inf')
LIM = 2 ** 18 - 2


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_voxel_downsample\s*\(', body)
    assert re.search(r'\bint64_t\s+hpl_voxel_downsample_workspace_bytes\s*\(', body)
    assert 'hpl_voxel_downsample' in _lib.EXPORTS and 'hpl_voxel_downsample_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_voxel_downsample')
    from hplflownet_amd import build
    assert 'voxel_grid.hip' in build.SOURCES
    import hplflownet_amd
    assert hplflownet_amd.voxel_downsample is hplflownet_amd.flownet.voxel_downsample


# ----------------------------------------------------------------------------- the restatement against a brute force
def brute(pc, attr, voxel, origin, mode):
    """Dictionary of lists, Python floats (float64) for the cells and the sums, numpy float32 scalars for the nearest rule."""
    n = pc.shape[1]
    inv = 1.0 / float(np.float32(voxel))
    org = [float(np.float32(o)) for o in origin]
    boxes, nonfinite, oob = {}, 0, 0
    voxel_of = [-1] * n
    for i in range(n):
        p = [float(pc[k, i]) for k in range(3)]
        if not all(math.isfinite(x) for x in p):
            nonfinite += 1
            continue
        cell = tuple(math.floor((p[k] - org[k]) * inv) for k in range(3))
        if any(abs(c) > LIM for c in cell):
            oob += 1
            continue
        boxes.setdefault(cell, []).append(i)
    out = []
    for v, cell in enumerate(sorted(boxes)):
        members = boxes[cell]
        cen = []
        for k in range(3):
            s = 0.0
            for i in members:
                s = s + float(pc[k, i])
            cen.append(np.float32(s / float(len(members))))
        best, rep = None, -1
        for i in members:
            dx, dy, dz = (np.float32(pc[k, i]) - cen[k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            if best is None or d2 < best:
                best, rep = d2, i
        means = []
        for c in range(0 if attr is None else attr.shape[0]):
            s = 0.0
            for i in members:
                s = s + float(attr[c, i])
            means.append(np.float32(s / float(len(members))))
        for i in members:
            voxel_of[i] = v
        point = [pc[k, rep] for k in range(3)] if mode == 'nearest' else cen
        chans = [attr[c, rep] for c in range(len(means))] if mode == 'nearest' else means
        out.append((point, chans, len(members), rep))
    return out, voxel_of, [len(out), sum(len(m) for m in boxes.values()), nonfinite, oob]


def same_as_brute(pc, attr, voxel, origin, mode):
    got = VO.downsample_cloud(pc, attr, voxel, origin, mode)
    rows, voxel_of, stats = brute(pc, attr, voxel, origin, mode)
    V, n = len(rows), pc.shape[1]
    assert got['stats'].tolist() == stats and got['voxel_of'].tolist() == voxel_of
    for v, (point, chans, cnt, rep) in enumerate(rows):
        assert got['out_pc'][:, v].tobytes() == np.array(point, np.float32).tobytes(), v
        assert got['count'][v] == cnt and got['rep'][v] == rep
        if attr is not None:
            assert got['out_attr'][:, v].tobytes() == np.array(chans, np.float32).tobytes(), v
    assert not got['out_pc'][:, V:].any() and not got['count'][V:].any() and (got['rep'][V:] == -1).all()
    assert got['out_pc'].shape == (3, n) and (attr is None or not got['out_attr'][:, V:].any())
    return got


@pytest.mark.parametrize('mode', ['centroid', 'nearest'])
def test_restatement_against_the_brute_force(mode):
    rng = np.random.RandomState(0)
    for n, voxel, C in ((1, 0.5, 0), (2, 0.5, 1), (40, 0.7, 3), (300, 1.5, 8), (300, 100.0, 2), (257, 0.05, 6)):
        pc = VO.scene(max(n, 10), 7 + n, extent=5.0)[:, :n]
        attr = rng.normal(0, 1, (C, n)).astype(np.float32) if C else None
        got = same_as_brute(pc, attr, voxel, (0.25, -1.0, 3.0), mode)
        assert got['stats'][1] == n and 1 <= got['stats'][0] <= n
    # a run longer than the restatement's own switch-over, non-finite points, duplicates and signed zeros
    pc = rng.uniform(-0.5, 0.5, (3, 150)).astype(np.float32)
    pc[:, 100:110] = pc[:, 90:100]
    pc[:, 110:115] = np.float32(-0.0)
    pc[1, 3], pc[2, 50], pc[0, 77] = np.nan, np.inf, -np.inf
    attr = rng.normal(0, 1, (2, 150)).astype(np.float32)
    attr[0, 5], attr[1, 6] = np.nan, np.inf
    for voxel, org in ((0.5, (0, 0, 0)), (4.0, (0, 0, 0)), (4.0, (-2, -2, -2))):
        got = same_as_brute(pc, attr, voxel, org, mode)
        assert got['stats'][2] == 3
    assert got['stats'][0] == 1 and got['count'][0] == 147 > VO.SHORT


# ----------------------------------------------------------------------------- cell edges
def test_cell_edges():
    v = 0.25                                                  # exact in float32: k * v is exact too
    pts = np.array([[0.0, -0.0, 0.25, -0.25, 0.5, -1e-30, 0.2499999, 1e-30],
                    [0.0] * 8, [0.0] * 8], np.float32)
    c, fin, valid = VO.cells(pts, v)
    assert c[0].tolist() == [0, 0, 1, -1, 2, -1, 0, 0] and valid.all() and fin.all()
    # the two limits are in range, one cell further is out; a non-zero origin shifts the grid
    edge = np.array([[LIM * v, -LIM * v, (LIM + 1) * v, -(LIM + 1) * v, (LIM + 1) * v - 1e-2, -LIM * v - 1e-2],
                     [0.0] * 6, [0.0] * 6], np.float32)
    c, fin, valid = VO.cells(edge, v)
    assert c[0].tolist() == [LIM, -LIM, LIM + 1, -(LIM + 1), LIM, -(LIM + 1)]
    assert valid.tolist() == [True, True, False, False, True, False] and fin.all()
    c, fin, valid = VO.cells(edge, v, origin=(v, 0, 0))
    assert c[0].tolist() == [LIM - 1, -LIM - 1, LIM, -LIM - 2, LIM - 1, -LIM - 2]
    assert valid.tolist() == [True, False, True, False, True, False]
    for axis in range(3):                                     # every axis has the limit
        p = np.zeros((3, 2), np.float32)
        p[axis] = [LIM * v, (LIM + 1) * v]
        assert VO.cells(p, v)[2].tolist() == [True, False]
    o = VO.downsample_cloud(edge, None, v)
    # the voxels come in ascending signed cell order: -LIM (one member), then LIM (two)
    assert o['stats'].tolist() == [2, 3, 0, 3] and o['voxel_of'].tolist() == [1, 0, -1, -1, 1, -1]
    assert o['count'].tolist() == [1, 2, 0, 0, 0, 0] and o['rep'][:2].tolist() in ([1, 0], [1, 4]) and (o['rep'][2:] == -1).all()
    # negative coordinates floor away from zero, and the order is lexicographic x, then y, then z
    p = np.array([[-0.1, -0.1, 0.1, -0.1], [0.1, -0.1, -0.3, -0.1], [0.0, 0.3, 0.0, -0.3]], np.float32)
    o = VO.downsample_cloud(p, None, 0.25, mode='nearest')
    assert o['stats'].tolist() == [4, 4, 0, 0] and o['rep'][:4].tolist() == [3, 1, 0, 2]
    assert np.array_equal(o['out_pc'][:, :4], p[:, [3, 1, 0, 2]])
    # non-finite points: counted, no member
    q = np.array([[0.1, np.nan, 0.1, np.inf], [0.1, 0.1, 0.1, 0.1], [0.1, 0.1, -np.inf, 0.1]], np.float32)
    o = VO.downsample_cloud(q, None, 1.0)
    assert o['stats'].tolist() == [1, 1, 3, 0] and o['voxel_of'].tolist() == [0, -1, -1, -1]


def test_outputs_are_consistent():
    rng = np.random.RandomState(3)
    parts = [VO.scene(n, 20 + n, extent=8.0) for n in (300, 1, 700)]
    parts.insert(1, parts[0][:, :0])
    pc = np.concatenate(parts, axis=1)
    pc[0, 5], pc[1, 400] = np.nan, 1e9                        # one non-finite, one out of range
    prefix = [0, 300, 300, 301, 1001]
    attr = rng.normal(0, 1, (3, pc.shape[1])).astype(np.float32)
    for mode in ('centroid', 'nearest'):
        o = VO.downsample(pc, attr, 0.8, (0, 0, 0), mode, prefix)
        assert o['stats'][:, 1:].sum() == pc.shape[1] and o['stats'][0, 2] == 1 and o['stats'][3, 3] == 1
        for b in range(4):
            p0, p1, V = prefix[b], prefix[b + 1], o['stats'][b, 0]
            assert o['count'][p0:p0 + V].sum() == o['stats'][b, 1] and (o['count'][p0:p0 + V] >= 1).all()
            assert np.array_equal(o['voxel_of'][o['rep'][p0:p0 + V]], np.arange(p0, p0 + V))
            assert not o['count'][p0 + V:p1].any() and (o['rep'][p0 + V:p1] == -1).all()
            assert not o['out_pc'][:, p0 + V:p1].any() and not o['out_attr'][:, p0 + V:p1].any()
            w = o['voxel_of'][p0:p1]
            assert ((w == -1) | ((w >= p0) & (w < p0 + V))).all()
            assert np.array_equal(np.bincount(w[w >= 0] - p0, minlength=V), o['count'][p0:p0 + V])
        if mode == 'nearest':                                 # a subset of the input, attributes with their points
            V = o['stats'][3, 0]
            r = o['rep'][301:301 + V]
            assert np.array_equal(o['out_pc'][:, 301:301 + V], pc[:, r]) and np.array_equal(o['out_attr'][:, 301:301 + V], attr[:, r])


# ----------------------------------------------------------------------------- refusals without a device
def call(pc=4096, pc_ld=100, attr=None, attr_ld=100, channels=0, batch=1, prefix=(0, 100), voxel=0.1, origin=(0, 0, 0), mode=0,
         out_pc=1 << 20, out_ld=100, out_attr=None, out_attr_ld=100, count=2 << 20, rep=3 << 20, voxel_of=4 << 20, stats=5 << 20,
         ws=6 << 20, ws_bytes=1 << 24):
    """hpl_voxel_downsample with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    origin = (ctypes.c_float * 3)(*origin) if origin is not None else None
    return _lib.load().hpl_voxel_downsample(pc, pc_ld, attr, attr_ld, channels, batch, prefix, voxel, origin, mode, out_pc, out_ld,
                                            out_attr, out_attr_ld, count, rep, voxel_of, stats, ws, ws_bytes, None)


ATTR = dict(attr=7 << 20, channels=3, out_attr=8 << 20)


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1), dict(channels=-1), dict(channels=9, attr=7 << 20),
    dict(channels=1), dict(mode=2), dict(mode=-1), dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=INF), dict(voxel=NAN),
    dict(origin=(0, INF, 0)), dict(origin=(NAN, 0, 0)), dict(origin=(0, 0, -INF)), dict(origin=None),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(prefix=None),
    dict(pc_ld=99), dict(out_ld=99), dict(ATTR, attr_ld=99), dict(ATTR, out_attr_ld=99),
    dict(pc=None), dict(out_pc=None), dict(stats=None), dict(ws=None),
    dict(pc=4098), dict(out_pc=(1 << 20) + 2), dict(count=(2 << 20) + 1), dict(rep=(3 << 20) + 3), dict(voxel_of=(4 << 20) + 2),
    dict(stats=(5 << 20) + 1), dict(ATTR, attr=(7 << 20) + 2), dict(ATTR, out_attr=(8 << 20) + 1),
    dict(ws=(6 << 20) + 128), dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_voxel_downsample_workspace_bytes(1, 100, 0) - 1),
    dict(prefix=(0, 2 ** 31 // 3 + 1), pc_ld=2 ** 31, out_ld=2 ** 31, ws_bytes=1 << 40),
    dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, out_ld=2 ** 60, ws_bytes=1 << 62),
    dict(out_pc=4096), dict(out_pc=4096 + 4 * 299), dict(out_pc=4096 - 4 * 299), dict(count=4096 + 4 * 150), dict(rep=4096),
    dict(voxel_of=4096 + 4 * 299), dict(stats=4096 + 4 * 200), dict(ATTR, out_attr=4096), dict(ATTR, out_pc=(7 << 20) + 4 * 299),
    dict(ATTR, count=(7 << 20) + 4 * 250), dict(ATTR, out_attr=(7 << 20) - 4 * 299),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_voxel_downsample')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments; arrays that only touch do not overlap."""
    assert call(prefix=(0, 0), pc_ld=0, out_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, out_ld=0, mode=1, voxel=1e-30, origin=(1e30, -5, 0), count=None, rep=None,
                voxel_of=None, **ATTR) == 0
    assert call(batch=64, prefix=(0,) * 65, channels=8, attr=7 << 20, out_attr=None) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_voxel_downsample_workspace_bytes
    assert f(0, 10, 0) == -1 and f(65, 10, 0) == -1 and f(-1, 10, 0) == -1
    assert f(1, -1, 0) == -1 and f(1, 2 ** 31 // 3 + 1, 0) == -1 and f(1, 2 ** 40, 0) == -1
    assert f(1, 10, -1) == -1 and f(1, 10, 9) == -1
    assert f(1, 2 ** 31 // 3, 8) > 0 and f(64, 0, 0) >= 0
    ns = [0, 1, 3, 1024, 1025, 8192, 100191, 450000, 2 ** 29]
    for b in (1, 2, 16, 64):
        for c in (0, 1, 8):
            vals = [f(b, n, c) for n in ns]
            assert all(v >= 0 and v % 256 == 0 for v in vals) and vals == sorted(vals)
            assert all(f(b + 1, n, c) >= f(b, n, c) for n in ns if b < 64)
            assert all(f(b, n, c + 1) >= f(b, n, c) for n in ns if c < 8)
    assert f(1, 450000, 8) < 64 << 20                         # 36 bytes a point and the sort's room


# ----------------------------------------------------------------------------- the Python layers' argument errors
def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        ops.voxel_downsample(pc)                              # a host tensor: no CPU fallback
    for kw in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=NAN), dict(voxel=INF), dict(voxel=1e39), dict(voxel=1e-50),
               dict(voxel='x'), dict(voxel=True), dict(origin=(0, 0)), dict(origin=(0, NAN, 0)), dict(origin=(0, 0, INF)),
               dict(origin=(1e39, 0, 0)), dict(origin=None), dict(mode='mean'), dict(mode=0), dict(mode=None)):
        with pytest.raises(_lib.HplError) as e:
            ops.voxel_downsample(pc, **kw)
        assert list(kw)[0] in str(e.value)
    assert ops.voxel_args('x', 0.1, (1, 2, 3), 'nearest') == (float(np.float32(0.1)), [1.0, 2.0, 3.0], 1)


def test_voxel_downsample_refuses_host_tensors_and_bad_forms():
    from hplflownet_amd import flownet
    a = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        flownet.voxel_downsample(a, a)                        # host tensors
    for args, kw in (((a, torch.zeros(3, 9)), {}), ((a, a, torch.zeros(3, 9)), {}), (([a], [a, a]), {}),
                     ((a, None, torch.zeros(3, 9)), {}), ((torch.zeros(10, 3), a), {}), (([],), {}),
                     (([a] * 33, [a] * 33), dict(corr=False)), (([a] * 65, [a] * 65), {}), (([a] * 65,), {}),
                     ((a, a), dict(voxel=0.0)), ((a, a), dict(voxel=NAN)), ((a, a), dict(mode='median')),
                     ((a, a), dict(origin=(0, 0)))):
        with pytest.raises(_lib.HplError) as e:
            flownet.voxel_downsample(*args, **kw)
        assert 'host' not in str(e.value) and 'device tensor' not in str(e.value), (args, kw)


def test_engine_argument_errors():
    from hplflownet_amd import engine
    base = ['--dataset', 'KITTI', '--evaluate', '--data-root', '/nowhere']
    a = engine.parse_args(base)
    assert a.voxel is None and a.voxel_mode is None and engine.parse_args([]).voxel is None
    a = engine.parse_args(base + ['--voxel', '0.2'])
    assert a.voxel == 0.2 and a.voxel_mode is None
    a = engine.parse_args(base + ['--voxel', '0.3', '--voxel-mode', 'nearest', '--ground', 'plane'])
    assert a.voxel == 0.3 and a.voxel_mode == 'nearest'
    for extra in (['--voxel', '0.2'], ['--dataset', 'FlyingThings3DSubset', '--data-root', '/nowhere', '--voxel', '0.2'],
                  base + ['--voxel', '0'], base + ['--voxel', '-0.1'], base + ['--voxel', 'inf'], base + ['--voxel', 'nan'],
                  base + ['--voxel', 'x'], base + ['--voxel'], base + ['--voxel-mode', 'nearest'],
                  base + ['--voxel', '0.2', '--voxel-mode', 'mean']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


def test_reader_refuses_voxels_on_a_cpu_device(tmp_path):
    from hplflownet_amd import data
    d = tmp_path / 'KITTI_processed_occ_final' / '000000'
    d.mkdir(parents=True)
    pc = VO.scene(64, 0).T
    np.save(str(d / 'pc1.npy'), pc)
    np.save(str(d / 'pc2.npy'), pc)
    for kw in (dict(device='cpu', voxel=0.2), dict(device='cuda', voxel=0.0), dict(device='cuda', voxel=NAN),
               dict(device='cuda', voxel=-1), dict(device='cuda', voxel=0.2, voxel_mode='mean'),
               dict(device='cuda', voxel_mode='nearest'), dict(device='cpu', voxel_mode='nearest')):
        with pytest.raises(_lib.HplError) as e:
            data.KITTI(None, str(tmp_path), **kw)
        assert 'voxel' in str(e.value)
    plain = data.KITTI(None, str(tmp_path), device='cpu')      # off by default: the reference's reader, on any device
    assert plain.voxel is None
    o1, o2 = plain.load(str(d))
    keep = ~((pc[:, 1] < -1.4) & (pc[:, 1] < -1.4))
    assert np.array_equal(o1, pc[keep]) and np.array_equal(o2, pc[keep])
