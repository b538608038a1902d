"""CPU: hpl_outlier_filter's declaration, export and refusals (no device needed), its workspace arithmetic, the numpy restatement
tests/outlier_oracle.py (the vectorised neighbourhoods against a plain double loop: ties, duplicates, the self-exclusion by
index; closed forms; the condition of the scene) and the argument checks of the wrappers, data.KITTI and the engine."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import outlier_oracle as O

I64 = ctypes.c_int64
BIG = 2 ** 31 // 3 + 1


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_outlier_filter\s*\(', body)
    assert re.search(r'\bint64_t\s+hpl_outlier_filter_workspace_bytes\s*\(', body)
    assert 'hpl_outlier_filter' in _lib.EXPORTS and 'hpl_outlier_filter_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_outlier_filter') and hasattr(_lib.load(), 'hpl_outlier_filter_workspace_bytes')
    from hplflownet_amd import build
    assert 'outlier_filter.hip' in build.SOURCES
    import hplflownet_amd
    assert hasattr(hplflownet_amd, 'remove_outliers') and 'remove_outliers' in hplflownet_amd.__doc__
    text = open(os.path.join(ROOT, 'hplflownet_amd', 'csrc', 'outlier_filter.hip')).read()
    assert '#include "grid_common.h"' in text and 'grid_store(' in text and 'room_next_pow2' in text
    assert 'atomic' not in re.sub(r'//.*', '', text)           # no atomic of any kind: every sum has a fixed order


WS = 1 << 20                                                  # a fake workspace address, far from the fake arrays
STAT, RAD = 0, 1


def call(pc=4096, pc_ld=100, batch=1, prefix=(0, 100), mode=STAT, k=16, radius=1.0, std_ratio=2.0, min_neighbors=0, keep=8192,
         keep_idx=12288, mean_dist=16384, count=20480, nbr_d2=None, thresh=24576, stats=28672, ws=WS, ws_bytes=1 << 24):
    """hpl_outlier_filter with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    return _lib.load().hpl_outlier_filter(pc, pc_ld, batch, prefix, mode, k, radius, std_ratio, min_neighbors, keep, keep_idx,
                                          mean_dist, count, nbr_d2, thresh, stats, ws, ws_bytes, None)


RADIUS_MODE = dict(mode=RAD, min_neighbors=2, mean_dist=None)


@pytest.mark.parametrize('kw', [
    dict(pc=None), dict(prefix=None), dict(thresh=None), dict(stats=None), dict(ws=None),
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1),
    dict(mode=2), dict(mode=-1),
    dict(k=0), dict(k=33), dict(k=-1),
    dict(radius=0.0), dict(radius=-1.0), dict(radius=float('inf')), dict(radius=float('nan')),
    dict(RADIUS_MODE, radius=0.0), dict(RADIUS_MODE, radius=float('nan')),
    dict(std_ratio=-0.5), dict(std_ratio=float('inf')), dict(std_ratio=float('nan')),
    dict(RADIUS_MODE, min_neighbors=0), dict(RADIUS_MODE, min_neighbors=-3),
    dict(RADIUS_MODE, mean_dist=16384), dict(RADIUS_MODE, nbr_d2=32768),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)),
    dict(prefix=(0, BIG), pc_ld=2 ** 31, ws_bytes=1 << 50),
    dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
    dict(prefix=(0, 2 ** 27), pc_ld=2 ** 27, k=16, nbr_d2=1 << 40, ws=1 << 50, ws_bytes=1 << 50),
    dict(pc_ld=99),
    dict(pc=4098), dict(keep_idx=12289), dict(mean_dist=16386), dict(count=20481), dict(nbr_d2=32770), dict(thresh=24578),
    dict(stats=28673),
    dict(ws=WS + 128), dict(ws=WS + 4), dict(ws_bytes=0),
    dict(ws_bytes=_lib.load().hpl_outlier_filter_workspace_bytes(1, 100) - 1),
    dict(keep=4096), dict(keep=4096 + 4 * 299), dict(keep_idx=4096 + 400), dict(mean_dist=4096 - 396), dict(count=4096 + 800),
    dict(nbr_d2=4096 + 1196), dict(thresh=4096 + 4), dict(stats=4096 + 1184),
    dict(keep=WS), dict(keep_idx=WS + 256), dict(mean_dist=WS - 396), dict(count=WS + 1024), dict(nbr_d2=WS + 2048),
    dict(thresh=WS + 512), dict(stats=WS - 12),
    dict(keep=12288 + 399), dict(keep_idx=16384 - 396), dict(count=16384), dict(nbr_d2=20480 + 396), dict(thresh=28672 - 12),
    dict(stats=8192 + 96), dict(thresh=28672),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_outlier_filter')


@pytest.mark.parametrize('kw,words', [
    (dict(pc=None), b'null pointer'), (dict(mode=2), b'mode = 2 (0 statistical, 1 radius)'), (dict(k=33), b'k = 33 (1 .. 32)'),
    (dict(radius=0.0), b'radius must be finite and > 0'), (dict(std_ratio=-1.0), b'std_ratio must be finite and >= 0'),
    (dict(RADIUS_MODE, min_neighbors=0), b'min_neighbors = 0 (>= 1)'),
    (dict(RADIUS_MODE, mean_dist=16384), b'the radius mode has no mean_dist and no nbr_d2'),
    (dict(batch=65, prefix=(0,) * 66), b'batch 65 (1 .. 64)'), (dict(prefix=(1, 100)), b'the prefix must start at 0'),
    (dict(pc_ld=99), b'row stride 99 below 100 points'), (dict(count=20481), b'arrays must be 4-byte aligned'),
    (dict(ws=WS + 128), b'the workspace must be 256-byte aligned'), (dict(keep=4096), b'an output overlaps the input'),
    (dict(keep=WS), b'an output overlaps the workspace'), (dict(count=16384), b'two outputs overlap'),
    (dict(prefix=(0, BIG), pc_ld=2 ** 31, ws_bytes=1 << 50), b'points pass the 32-bit element limit (N < 2^31 / 3)'),
    (dict(prefix=(0, 2 ** 27), pc_ld=2 ** 27, k=16, nbr_d2=1 << 40, ws=1 << 50, ws_bytes=1 << 50), b'(N k < 2^31)'),
])
def test_refusals_say_what_is_wrong(kw, words):
    assert call(**kw) == -1
    err = _lib.load().hpl_last_error()
    assert err.startswith(b'hpl_outlier_filter: ') and words in err, err


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments; the limits themselves are accepted."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(prefix=(0, 0), pc_ld=0, k=1, radius=1e-3, std_ratio=0.0, keep=None, keep_idx=None, mean_dist=None, count=None) == 0
    assert call(batch=64, prefix=(0,) * 65, k=32, radius=1e30, nbr_d2=65536, thresh=1 << 17, stats=1 << 18) == 0
    assert call(prefix=(0, 0), ws_bytes=_lib.load().hpl_outlier_filter_workspace_bytes(1, 0)) == 0
    assert call(prefix=(0, 0), keep=4096, keep_idx=4096, nbr_d2=WS) == 0          # nothing to overlap but thresh and stats
    assert call(prefix=(0, 0), mode=RAD, min_neighbors=2 ** 31 - 1, mean_dist=None, k=0, std_ratio=-1.0) == 0
    assert call(prefix=(0, 0), mode=STAT, min_neighbors=-5) == 0                  # what a mode does not read is not checked


def test_workspace_bytes():
    f = _lib.load().hpl_outlier_filter_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(-1, 10) == -1
    assert f(1, -1) == -1 and f(1, BIG) == -1 and f(1, 2 ** 60) == -1
    assert f(1, BIG - 1) > 0 and f(64, 0) > 0
    ns = [0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 450000, 2 ** 27]
    for b in (1, 2, 16, 64):
        got = [f(b, n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in got) and got == sorted(got)
        assert all(f(b, n) >= f(1, n) for n in ns)            # a cloud more: a workgroup's partials more
    g = _lib.load().hpl_normals_workspace_bytes
    assert all(f(1, n) >= g(1, n) + 8 * n for n in ns)        # hpl_normals' grid, and mean_dist and count a point
    assert f(1, 450000) < 64 << 20


def test_wrappers_refuse_before_the_library():
    from hplflownet_amd import ops, remove_outliers
    a = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        ops.outlier_filter(a)                                 # a host tensor: no CPU fallback
    for kw in (dict(k=0), dict(k=33), dict(k=8.0), dict(k=True), dict(radius=0.0), dict(radius=float('inf')),
               dict(radius=float('nan')), dict(radius=-1.0), dict(std_ratio=-1.0), dict(std_ratio=float('inf')),
               dict(std_ratio=float('nan')), dict(mode='median'), dict(mode=0), dict(min_neighbors=2),
               dict(mode='radius'), dict(mode='radius', min_neighbors=0), dict(mode='radius', min_neighbors=2.0),
               dict(mode='radius', min_neighbors=2 ** 31), dict(mode='radius', min_neighbors=2, return_neighbors=True)):
        with pytest.raises(_lib.HplError, match='outlier_filter'):
            ops.outlier_filter(a, **kw)
    with pytest.raises(_lib.HplError, match='min_neighbors'):
        ops.outlier_args('x', 'statistical', 16, 1.0, 2.0, 3)
    assert ops.outlier_args('x', 'statistical', 8, 2, 0, None) == (0, 8, 2.0, 0.0, 0)
    assert ops.outlier_args('x', 'radius', 16, 0.5, 2.0, 4) == (1, 0, 0.5, 0.0, 4)
    for args, kw in (((a,), {}), (([],), {}), ((torch.zeros(10),), {})):
        with pytest.raises(_lib.HplError):
            remove_outliers(*args, **kw)
    for kw in (dict(by='pc2'), dict(by=None), dict(k=0), dict(mode='radius'), dict(prefix=[0, 10]), dict(return_neighbors=True),
               dict(out=None), dict(corr=False, return_mask=True), dict(std_ratio=-1)):
        with pytest.raises(_lib.HplError, match='remove_outliers'):
            remove_outliers(a, a, **kw)
    # by either cloud, or every cloud on its own: 2 B clouds a call, so 32 pairs; by pc1: 64
    for n, kw in ((33, {}), (33, dict(corr=False)), (65, dict(by='pc1'))):
        with pytest.raises(_lib.HplError, match=r'remove_outliers: %d pairs \(1 \.\. %d a call\)' % (n, 32 if n == 33 else 64)):
            remove_outliers([a] * n, [a] * n, **kw)
    with pytest.raises(_lib.HplError, match='outlier_filter: pc must be'):    # 64 pairs by pc1 reach the op (which has no CPU path)
        remove_outliers([a] * 64, [a] * 64, by='pc1')
    with pytest.raises(_lib.HplError, match='as many points'):
        remove_outliers(a, torch.zeros(3, 11))


def test_kitti_refuses_a_wrong_outlier_option(tmp_path):
    from hplflownet_amd import data
    for device, outlier in (('cpu', {}), ('cuda', {'k': 0}), ('cuda', {'voxel': 1.0}), ('cuda', ['k']), ('cuda', {'by': 'pc2'}),
                            ('cuda', {'mode': 'radius'}), ('cuda', {'min_neighbors': 2}), ('cuda', {'radius': 0})):
        with pytest.raises(_lib.HplError, match='KITTI: outlier'):
            data.KITTI(None, str(tmp_path), device=device, outlier=outlier)
    with pytest.raises(_lib.HplError, match='there is no CPU fallback'):
        data.KITTI(None, str(tmp_path), device='cpu', outlier={'k': 8})
    with pytest.raises(RuntimeError, match='Found 0 files'):  # the option itself passes: the empty folder is what stops it
        data.KITTI(None, str(tmp_path), device='cuda', outlier={'mode': 'radius', 'min_neighbors': 3, 'radius': 0.5, 'by': 'pc1'})
    import inspect
    assert 'outlier' in inspect.signature(data.KITTIRaw.__init__).parameters


def test_engine_outlier_arguments():
    from hplflownet_amd import engine
    base = ['--evaluate', '--dataset', 'KITTI', '--data-root', '/nowhere']
    assert engine.parse_args(base).outlier_filter is None
    assert engine.parse_args(base + ['--outlier', 'statistical']).outlier_filter == {
        'mode': 'statistical', 'k': 16, 'radius': 1.0, 'std_ratio': 2.0}
    assert engine.parse_args(base + ['--outlier', 'statistical', '--outlier-k', '8', '--outlier-radius', '2.5',
                                     '--outlier-std-ratio', '0']).outlier_filter == {
        'mode': 'statistical', 'k': 8, 'radius': 2.5, 'std_ratio': 0.0}
    assert engine.parse_args(base + ['--outlier', 'radius', '--outlier-min-neighbors', '5', '--outlier-radius', '0.5']
                             ).outlier_filter == {'mode': 'radius', 'radius': 0.5, 'min_neighbors': 5}
    assert engine.parse_args(base + ['--outlier', 'radius']).outlier_filter == {'mode': 'radius', 'radius': 1.0, 'min_neighbors': 2}
    for extra in (['--evaluate', '--outlier', 'statistical'], base + ['--outlier', 'median'], base + ['--outlier-k', '8'],
                  base + ['--outlier-radius', '1'], base + ['--outlier-std-ratio', '1'], base + ['--outlier-min-neighbors', '2'],
                  base + ['--outlier', 'statistical', '--outlier-k', '0'], base + ['--outlier', 'statistical', '--outlier-k', '33'],
                  base + ['--outlier', 'statistical', '--outlier-min-neighbors', '2'],
                  base + ['--outlier', 'statistical', '--outlier-std-ratio', '-1'],
                  base + ['--outlier', 'statistical', '--outlier-std-ratio', 'nan'],
                  base + ['--outlier', 'radius', '--outlier-k', '8'], base + ['--outlier', 'radius', '--outlier-std-ratio', '1'],
                  base + ['--outlier', 'radius', '--outlier-min-neighbors', '0'],
                  base + ['--outlier', 'radius', '--outlier-radius', '0'], base + ['--outlier', 'radius', '--outlier-radius', 'inf']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


# ----------------------------------------------------------------------------- the restatement
def lattice_cloud(seed, n):
    """A cloud on a coarse lattice of positions (many exact ties and duplicates), with non-finite and far points."""
    rng = np.random.RandomState(seed)
    pc = (rng.randint(-4, 5, (3, n)) * 0.25).astype(np.float32)
    if n >= 8:
        pc[:, 3] = pc[:, 1]                                   # duplicates
        pc[0, 4] = np.nan
        pc[2, 5] = np.inf
        pc[:, 6] = 1e7
    return pc


def bits(x):
    return np.asarray(x, np.float32).view(np.int32)


@pytest.mark.parametrize('n,seed', [(1, 0), (3, 1), (40, 2), (61, 3)])
@pytest.mark.parametrize('k', [1, 8, 17])
def test_vectorised_neighbourhood_equals_the_double_loop(n, seed, k):
    pc = lattice_cloud(seed, n)
    for radius in (0.25, 0.6, 3.0):
        a, b = O.neighbourhoods(pc, k, radius, chunk=16), O.neighbourhoods_loop(pc, k, radius)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
        for mode, kw in (('statistical', dict(k=k, std_ratio=1.0)), ('radius', dict(min_neighbors=2))):
            x, y = O.outlier_filter(pc, mode, radius=radius, **kw), O.outlier_filter(pc, mode, radius=radius, loop=True, **kw)
            for key in ('keep', 'keep_idx', 'count', 'stats', 'thresh'):
                assert np.array_equal(x[key], y[key]), key
            if mode == 'statistical':
                assert np.array_equal(bits(x['mean_dist']), bits(y['mean_dist'])) and np.array_equal(bits(x['nbr_d2']), bits(y['nbr_d2']))
    if n >= 8:
        total, nd2 = O.neighbourhoods(pc, k, 3.0)
        assert (total[[4, 5, 6]] == 0).all() and np.isinf(nd2[[4, 5, 6]]).all()  # (1e7 m is outside the cells' range)
        assert nd2[1, 0] == 0 and nd2[3, 0] == 0              # the duplicate is a neighbour at d2 = 0; the point itself is none
        r = O.outlier_filter(pc, k=k, radius=3.0)
        assert (r['keep'][[4, 5, 6]] == 0).all() and np.isinf(r['mean_dist'][[4, 5, 6]]).all() and r['stats'][0, 3] == 3
        assert O.neighbourhoods(pc, k, 50.0)[0][6] == 0       # at this radius it takes part, alone: nobody but itself


def test_self_exclusion_is_by_index_and_ties_need_no_rule():
    pc = np.zeros((3, 5), np.float32)                         # five indices at one position
    total, nd2 = O.neighbourhoods(pc, 8, 1.0)
    assert (total == 4).all() and (nd2[:, :4] == 0).all() and np.isinf(nd2[:, 4:]).all()
    r = O.outlier_filter(pc, k=4, radius=1.0, std_ratio=0.0)
    assert (r['mean_dist'] == 0).all() and r['keep'].all() and list(r['thresh'][0]) == [0, 0, 0, 0]
    r = O.outlier_filter(pc, 'radius', radius=1.0, min_neighbors=4)
    assert (r['count'] == 4).all() and r['keep'].all()
    assert not O.outlier_filter(pc, 'radius', radius=1.0, min_neighbors=5)['keep'].any()


def test_batches_search_their_own_cloud():
    pc = np.concatenate([lattice_cloud(5, 30), lattice_cloud(6, 20), lattice_cloud(7, 25)], 1)
    prefix = [0, 30, 30, 50, 75]
    got = O.outlier_filter(pc, k=8, radius=0.6, prefix=prefix)
    assert (got['stats'][1] == 0).all() and (got['thresh'][1] == 0).all()
    for b, (p0, p1) in enumerate(zip(prefix, prefix[1:])):
        alone = O.outlier_filter(pc[:, p0:p1], k=8, radius=0.6)
        assert np.array_equal(bits(got['mean_dist'][p0:p1]), bits(alone['mean_dist']))
        assert np.array_equal(got['keep'][p0:p1], alone['keep']) and np.array_equal(got['stats'][b], alone['stats'][0])
        assert np.array_equal(got['keep_idx'][p0:p1], np.where(alone['keep_idx'] >= 0, alone['keep_idx'] + p0, -1))
        assert np.array_equal(bits(got['thresh'][b]), bits(alone['thresh'][0]))


def test_a_point_exactly_at_the_radius_is_a_neighbour():
    pc = np.array([[0, 0.5, 0.5000001], [0, 0, 0], [0, 0, 0]], np.float32)
    total, nd2 = O.neighbourhoods(pc, 3, 0.5)
    assert total[0] == 1 and nd2[0, 0] == np.float32(0.25) and np.isinf(nd2[0, 1])


# ----------------------------------------------------------------------------- closed forms
def test_the_unit_cube():
    pc = np.array([[i, j, l] for i in (0, 1) for j in (0, 1) for l in (0, 1)], np.float32).T
    r = O.outlier_filter(pc, k=3, radius=1.5, std_ratio=0.0)
    assert (r['mean_dist'] == 1).all() and (r['count'] == 3).all()
    assert list(r['thresh'][0]) == [1, 0, 1, 0] and list(r['thresh64'][0]) == [1, 0, 1]
    assert r['keep'].all() and list(r['keep_idx']) == list(range(8)) and list(r['stats'][0]) == [8, 8, 0, 0]


def test_a_lone_point_has_the_radius_and_is_kept():
    for radius in (0.75, 2.0):
        r = O.outlier_filter(np.array([[1.0], [2.0], [3.0]], np.float32), k=5, radius=radius, std_ratio=0.0)
        assert r['mean_dist'][0] == np.float32(radius) and r['count'][0] == 0
        assert list(r['thresh'][0]) == [np.float32(radius), 0, np.float32(radius), 0]       # n' = 1: sigma is 0
        assert r['keep'][0] == 1 and list(r['stats'][0]) == [1, 1, 0, 0]


def test_a_stray_pair_does_not_look_dense():
    pc = np.array([[0, 0.1], [0, 0], [0, 0]], np.float32)
    r = O.outlier_filter(pc, k=4, radius=2.0)
    d2 = np.float32(np.float32(0.1) * np.float32(0.1))
    want = np.float32((np.sqrt(np.float64(d2)) + 3 * 2.0) / 4)
    assert (r['mean_dist'] == want).all() and (r['count'] == 1).all() and abs(float(want) - 1.525) < 1e-6


# ----------------------------------------------------------------------------- the condition of the scene
SCENES = [(300, 10, 8, 4.0), (1025, 25, 16, 2.0), (3000, 60, 16, 2.0), (3000, 60, 32, 2.0), (3000, 60, 8, 1.0)]


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('n,n_out,k,radius', SCENES)
def test_scene_strays_are_removed_and_the_surface_stays(n, n_out, k, radius, seed):
    pc, stray = O.scene(n, n_out, seed)
    assert pc.shape == (3, n) and stray.sum() == n_out and (pc[1, stray] >= 4.5).all() and (pc[1, ~stray] < 3).all()
    r = O.outlier_filter(pc, k=k, radius=radius, std_ratio=2.0)
    kept = r['keep'].astype(bool)
    print('n = %d, %d strays, k = %d, radius %g, seed %d: strays removed %.1f %%, surface kept %.1f %%' % (
        n, n_out, k, radius, seed, 100 * (~kept[stray]).mean(), 100 * kept[~stray].mean()))
    assert not kept[stray].any()
    assert kept[~stray].mean() >= 0.95
