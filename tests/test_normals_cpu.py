"""CPU: hpl_normals' declaration, export and refusals (no device needed), its workspace arithmetic, the numpy restatement
tests/normals_oracle.py (the vectorised neighbourhood against a plain double loop, ties included; the surface scene gives
well-separated normals) and the wrappers' refusals; the same for hpl_icp_plane (point-to-plane ICP on those normals): its
refusals and workspace, the metric arguments of ops.icp / icp_register / the engine, and the restatement's convergence."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import normals_oracle as O

I64 = ctypes.c_int64
BIG = 2 ** 31 // 3 + 1


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_normals\s*\(', body) and re.search(r'\bint64_t\s+hpl_normals_workspace_bytes\s*\(', body)
    assert 'hpl_normals' in _lib.EXPORTS and 'hpl_normals_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_normals') and hasattr(_lib.load(), 'hpl_normals_workspace_bytes')
    from hplflownet_amd import build
    assert 'normals.hip' in build.SOURCES
    import hplflownet_amd
    assert hasattr(hplflownet_amd, 'estimate_normals') and 'estimate_normals' in hplflownet_amd.__doc__


WS = 1 << 20                                                  # a fake workspace address, far from the fake arrays


def call(pc=4096, pc_ld=100, batch=1, prefix=(0, 100), k=16, radius=1.0, view=None, normal=8192, normal_ld=100, curvature=16384,
         count=20480, nbr=None, nbr_d2=None, ws=WS, ws_bytes=1 << 24):
    """hpl_normals with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    view = (ctypes.c_float * len(view))(*view) if view is not None else None
    return _lib.load().hpl_normals(pc, pc_ld, batch, prefix, k, radius, view, normal, normal_ld, curvature, count, nbr, nbr_d2,
                                   ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(pc=None), dict(normal=None), dict(prefix=None), dict(ws=None),
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1),
    dict(k=2), dict(k=33), dict(k=0), dict(k=-1),
    dict(radius=0.0), dict(radius=-1.0), dict(radius=float('inf')), dict(radius=float('nan')),
    dict(view=(0.0, float('nan'), 0.0)), dict(view=(float('inf'), 0.0, 0.0)),
    dict(batch=2, prefix=(0, 50, 100), view=(0.0, 0.0, 0.0, 0.0, 0.0, float('-inf'))),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)),
    dict(prefix=(0, BIG), pc_ld=2 ** 31, normal_ld=2 ** 31, ws_bytes=1 << 50),
    dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, normal_ld=2 ** 60, ws_bytes=1 << 62),
    dict(prefix=(0, 2 ** 27), pc_ld=2 ** 27, normal_ld=2 ** 27, k=16, nbr=1 << 40, ws=1 << 50, ws_bytes=1 << 50),
    dict(prefix=(0, 2 ** 27), pc_ld=2 ** 27, normal_ld=2 ** 27, k=32, nbr_d2=1 << 40, ws=1 << 50, ws_bytes=1 << 50),
    dict(pc_ld=99), dict(normal_ld=99),
    dict(pc=4098), dict(normal=8193), dict(curvature=16386), dict(count=20481), dict(nbr=32770), dict(nbr_d2=36865),
    dict(ws=WS + 128), dict(ws=WS + 4), dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_normals_workspace_bytes(1, 100) - 1),
    dict(normal=4096), dict(normal=4096 + 4 * 299), dict(normal=4096 - 4 * 299), dict(curvature=4096 + 400), dict(count=4096 + 800),
    dict(nbr=4096), dict(nbr_d2=4096 + 1196),
    dict(normal=WS), dict(curvature=WS + 256), dict(count=WS - 396), dict(nbr=WS + 1024), dict(nbr_d2=WS + 2048),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_normals')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments; the limits themselves are accepted."""
    assert call(prefix=(0, 0), pc_ld=0, normal_ld=0) == 0
    assert call(prefix=(0, 0), pc_ld=0, normal_ld=0, k=3, radius=1e-3, view=(1.0, 2.0, 3.0), curvature=None, count=None) == 0
    assert call(batch=64, prefix=(0,) * 65, k=32, radius=1e30, nbr=32768, nbr_d2=65536) == 0
    assert call(prefix=(0, 0), ws_bytes=_lib.load().hpl_normals_workspace_bytes(1, 0)) == 0
    assert call(prefix=(0, 0), normal=4096, curvature=4096, nbr=WS) == 0     # nothing to overlap


def test_workspace_bytes():
    f = _lib.load().hpl_normals_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(-1, 10) == -1
    assert f(1, -1) == -1 and f(1, BIG) == -1 and f(1, 2 ** 60) == -1
    assert f(1, BIG - 1) > 0 and f(64, 0) > 0
    ns = [0, 1, 3, 255, 256, 257, 1024, 1025, 8192, 8193, 100191, 450000, 2 ** 27]
    for b in (1, 2, 16, 64):
        got = [f(b, n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in got) and got == sorted(got)
        assert got == [f(1, n) for n in ns]                   # the clouds share one grid: the batch costs nothing
    assert f(1, 450000) < 64 << 20                            # 48 bytes per point and the sort's room


def test_wrappers_refuse_before_the_library():
    from hplflownet_amd import estimate_normals, ops
    a = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        ops.normals(a)                                        # a host tensor: no CPU fallback
    for kw in (dict(k=2), dict(k=33), dict(k=8.0), dict(k=True), dict(radius=0.0), dict(radius=float('inf')),
               dict(radius=float('nan')), dict(radius=-1.0)):
        with pytest.raises(_lib.HplError):
            ops.normals(a, **kw)
    with pytest.raises(_lib.HplError):
        estimate_normals(a)
    with pytest.raises(_lib.HplError):
        estimate_normals([])
    with pytest.raises(_lib.HplError):
        estimate_normals(torch.zeros(10))


# ----------------------------------------------------------------------------- the restatement
def loop_neighbourhoods(pc, k, radius):
    """The neighbourhoods of one cloud by a plain double loop over scalars: float32 arithmetic one operation at a time."""
    f = np.float32
    r2 = f(f(radius) * f(radius))
    inv = 1.0 / (1.001 * np.float64(f(radius)))
    n = pc.shape[1]
    count, nbr, nd2 = np.zeros(n, np.int32), np.full((n, k), -1, np.int32), np.full((n, k), np.inf, f)

    def part(v):
        return all(np.isfinite(x) and abs(np.floor(np.float64(x) * inv)) <= 2 ** 18 - 2 for x in v)

    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            if not part(pc[:, i]):
                continue
            found = []
            for j in range(n):
                if not part(pc[:, j]):
                    continue
                dx, dy, dz = f(pc[0, i] - pc[0, j]), f(pc[1, i] - pc[1, j]), f(pc[2, i] - pc[2, j])
                d2 = f(f(f(dx * dx) + f(dy * dy)) + f(dz * dz))
                if d2 <= r2:
                    found.append((d2, j))
            found.sort()                                      # (d2, j) ascending
            found = found[:k]
            count[i] = len(found)
            for t, (d2, j) in enumerate(found):
                nbr[i, t], nd2[i, t] = j, d2
    return count, nbr, nd2


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


@pytest.mark.parametrize('n,seed', [(1, 0), (3, 1), (40, 2), (61, 3)])
@pytest.mark.parametrize('k', [3, 8, 17])
def test_vectorised_neighbourhood_equals_the_double_loop(n, seed, k):
    pc = lattice_cloud(seed, n)
    for radius in (0.25, 0.6, 3.0):
        a, b = O.neighbourhoods(pc, k, radius, chunk=16), loop_neighbourhoods(pc, k, radius)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    if n >= 8:
        count, nbr, _ = O.neighbourhoods(pc, k, 3.0)
        assert (count[[4, 5, 6]] == 0).all() and not np.isin(nbr, [4, 5, 6]).any()       # (1e7 m is outside the cells' range)
        far = O.neighbourhoods(pc, k, 50.0)
        assert far[0][6] == 1 and far[1][6, 0] == 6           # at this radius it takes part, alone
        assert nbr[1, 0] == 1 and nbr[1, 1] == 3 and nbr[3, 0] == 1 and nbr[3, 1] == 3      # equal d2: the smaller index first


def test_batches_search_their_own_cloud():
    pc = np.concatenate([lattice_cloud(5, 30), lattice_cloud(6, 20), lattice_cloud(7, 25)], 1)
    prefix = [0, 30, 30, 50, 75]
    got = O.neighbourhoods(pc, 8, 0.6, prefix)
    for p0, p1 in zip(prefix, prefix[1:]):
        alone = O.neighbourhoods(pc[:, p0:p1], 8, 0.6)
        assert np.array_equal(got[0][p0:p1], alone[0])
        assert np.array_equal(got[1][p0:p1], np.where(alone[1] >= 0, alone[1] + p0, -1))
        assert np.array_equal(got[2][p0:p1].view(np.int32), alone[2].view(np.int32))


def test_a_point_exactly_at_the_radius_is_a_neighbour():
    pc = np.array([[0, 0.5, 0.5000001], [0, 0, 0], [0, 0, 0]], np.float32)
    count, nbr, nd2 = O.neighbourhoods(pc, 3, 0.5)
    assert count[0] == 2 and list(nbr[0]) == [0, 1, -1] and nd2[0, 1] == np.float32(0.25)


@pytest.mark.parametrize('n,k,radius', [(1025, 16, 1.0), (1025, 32, 1.5)])
def test_scene_has_separated_normals(n, k, radius):
    """The share of the scene's points whose smallest eigenvalue stands apart (the condition of the GPU comparison), and the
    normals of the ground's points."""
    pc = O.scene(n, 1)
    r = O.normals(pc, k, radius)
    has = r['count'] >= 3
    share = (r['gap'][has] >= 1e-3).mean()
    print('n = %d, k = %d, radius %g: %.1f %% with three neighbours, %.1f %% of them with gap >= 1e-3' % (
        n, k, radius, 100 * has.mean(), 100 * share))
    assert share >= 0.95
    assert np.allclose(np.linalg.norm(r['n64'][:, r['valid']], axis=0), 1.0, atol=1e-12)
    assert (r['normal'][:, ~r['valid']] == 0).all()
    s = -(r['n64'] * pc.astype(np.float64)).sum(0)
    assert (s[r['valid']] >= 0).all()                         # towards the origin


def test_a_plane_gives_its_normal_and_viewpoints_flip_it():
    rng = np.random.RandomState(3)
    pc = np.stack([rng.uniform(-1, 1, 200), np.full(200, 0.5), rng.uniform(-1, 1, 200)]).astype(np.float32)
    below = O.normals(pc, 8, 1.0)                             # the origin lies below the plane y = 0.5
    above = O.normals(pc, 8, 1.0, viewpoint=(0, 2, 0))
    assert below['valid'].all() and np.abs(below['n64'] - np.array([[0], [-1.0], [0]])).max() < 1e-9
    assert np.abs(above['n64'] - np.array([[0], [1.0], [0]])).max() < 1e-9
    assert np.abs(below['curvature']).max() < 1e-12


# ----------------------------------------------------------------------------- hpl_icp_plane
def test_icp_plane_is_declared_exported_and_shares_icp_common():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_icp_plane\s*\(', body) and re.search(r'\bint64_t\s+hpl_icp_plane_workspace_bytes\s*\(', body)
    assert 'hpl_icp_plane' in _lib.EXPORTS and hasattr(_lib.load(), 'hpl_icp_plane')
    from hplflownet_amd import build
    assert 'icp_plane.hip' in build.SOURCES
    csrc = os.path.join(ROOT, 'hplflownet_amd', 'csrc')
    for name in ('icp.hip', 'icp_plane.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "icp_common.h"' in text and 'match_point(const' not in text      # one definition, in the header
    assert 'match_point(const' in open(os.path.join(csrc, 'icp_common.h')).read()


def plane_call(src=256, src_ld=100, dst=512, dst_ld=80, nrm=2048, nrm_ld=80, weight=None, init=None, batch=1, sprefix=(0, 100),
               dprefix=(0, 80), iters=4, max_dist=1.0, tau=0.3, tol_rot=0.0, tol_trans=0.0, Rt=768, stats=1024, match=None,
               dist2=None, flow=1280, ws=4096, ws_bytes=1 << 24):
    """hpl_icp_plane with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    sprefix = (I64 * len(sprefix))(*sprefix) if sprefix is not None else None
    dprefix = (I64 * len(dprefix))(*dprefix) if dprefix is not None else None
    return _lib.load().hpl_icp_plane(src, src_ld, dst, dst_ld, nrm, nrm_ld, weight, init, batch, sprefix, dprefix, iters, max_dist,
                                     tau, tol_rot, tol_trans, Rt, stats, match, dist2, flow, ws, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(src=None), dict(dst=None), dict(nrm=None), dict(Rt=None), dict(stats=None), dict(sprefix=None), dict(dprefix=None),
    dict(ws=None), dict(batch=0), dict(batch=65, sprefix=(0,) * 66, dprefix=(0,) * 66), dict(batch=-1),
    dict(iters=-1), dict(iters=65),
    dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float('inf')), dict(max_dist=float('nan')),
    dict(tau=0.0), dict(tau=-0.1), dict(tau=float('inf')), dict(tau=float('nan')),
    dict(tol_rot=-1e-6), dict(tol_trans=-1e-6), dict(tol_rot=float('nan')), dict(tol_trans=float('nan')),
    dict(sprefix=(1, 100)), dict(dprefix=(1, 80)),
    dict(batch=2, sprefix=(0, 60, 50), dprefix=(0, 40, 80)), dict(batch=2, sprefix=(0, 50, 100), dprefix=(0, 50, 40)),
    dict(src_ld=99), dict(dst_ld=79), dict(nrm_ld=79),
    dict(src=258), dict(dst=513), dict(nrm=2050), dict(weight=9), dict(init=6), dict(Rt=770), dict(stats=1027), dict(match=5),
    dict(dist2=7), dict(flow=1282),
    dict(ws=4096 + 128), dict(ws=4100), dict(ws_bytes=0),
    dict(ws_bytes=_lib.load().hpl_icp_plane_workspace_bytes(1, 100, 80) - 1),
    dict(sprefix=(0, BIG), src_ld=2 ** 31, ws_bytes=1 << 50),
    dict(dprefix=(0, BIG), dst_ld=2 ** 31, nrm_ld=2 ** 31, ws_bytes=1 << 50),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_icp_plane_refusals_without_a_device(kw):
    assert plane_call(**kw) == -1                             # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_icp_plane')


def test_icp_plane_empty_calls_and_workspace_bytes():
    assert plane_call(sprefix=(0, 0), src_ld=0) == 0
    assert plane_call(sprefix=(0, 0), src_ld=0, dprefix=(0, 0), dst_ld=0, nrm_ld=0, dst=None, nrm=None, iters=0) == 0
    f, g = _lib.load().hpl_icp_plane_workspace_bytes, _lib.load().hpl_icp_workspace_bytes
    assert f(0, 10, 10) == -1 and f(65, 10, 10) == -1 and f(1, -1, 10) == -1 and f(1, 10, BIG) == -1 and f(1, BIG, 10) == -1
    ns = [0, 1, 3, 255, 1024, 1025, 8192, 8193, 100191, 450000, 2 ** 27]
    for b in (1, 2, 16, 64):
        for fixed in (0, 1025, 450000):
            by_src, by_dst = [f(b, n, fixed) for n in ns], [f(b, fixed, n) for n in ns]
            assert all(v > 0 and v % 256 == 0 for v in by_src + by_dst)
            assert by_src == sorted(by_src) and by_dst == sorted(by_dst)
            assert all(f(b, n, fixed) >= g(b, n, fixed) for n in ns)         # 28 sums a workgroup where hpl_icp keeps 16


def test_icp_wrappers_refuse_a_wrong_metric_before_the_library():
    from hplflownet_amd import icp_register, ops
    a, b = torch.zeros(3, 10), torch.zeros(3, 12)
    for kw in (dict(metric='plane'), dict(metric='line'), dict(dst_normal=b), dict(metric='point', dst_normal=b)):
        with pytest.raises(_lib.HplError, match='metric'):
            ops.icp(a, b, **kw)
    for kw in (dict(metric='line'), dict(normals=b), dict(metric='point', normals=b)):
        with pytest.raises(_lib.HplError, match='metric'):
            icp_register(a, b, **kw)


def test_the_plane_restatement_converges_where_the_surfaces_are_sampled_independently():
    """CPU only: on the pair of the GPU tests the point-to-plane chain reaches a bitwise fixpoint and ends nearer the true
    translation than 30 point-to-point rounds."""
    import icp_oracle as P
    import icp_plane_oracle as Q
    src, dst = Q.pair(1025, 1025)
    nrm = O.normals(dst, 16, 1.0)['normal']
    c, p = Q.chain(src, dst, nrm, iters=30), P.chain(src, dst, iters=30)
    et, pt = np.abs(c['t32'] - P.TRUE_T).max(), np.abs(p['t32'] - P.TRUE_T).max()
    print('plane: %d rounds, t off by %.3g m; point: %d rounds, t off by %.3g m' % (c['rounds'], et, p['rounds'], pt))
    assert c['status'] == 1 and c['rounds'] < 30 and et < pt
    again = Q.round_(src, dst, nrm, c['R32'], c['t32'])
    assert np.array_equal(again['R32'], c['R32']) and np.array_equal(again['t32'], c['t32'])


def test_engine_icp_metric_arguments_and_validate_keys():
    from hplflownet_amd import engine
    base = ['--evaluate', '--baseline', 'icp']
    assert engine.parse_args(base).icp == {'iters': 30, 'max_dist': 1.0, 'tau': 0.3, 'init': 'identity'}
    got = engine.parse_args(base + ['--icp-metric', 'plane', '--icp-normals-k', '8', '--icp-normals-radius', '1.5'])
    assert got.icp == {'iters': 30, 'max_dist': 1.0, 'tau': 0.3, 'init': 'identity', 'metric': 'plane', 'normals_k': 8,
                       'normals_radius': 1.5}
    assert engine.parse_args(base + ['--icp-metric', 'point']).icp['metric'] == 'point'
    for extra in (['--evaluate', '--icp-metric', 'plane'], base + ['--icp-metric', 'line'], base + ['--icp-normals-k', '8'],
                  base + ['--icp-metric', 'point', '--icp-normals-k', '8'], base + ['--icp-metric', 'plane', '--icp-normals-k', '2'],
                  base + ['--icp-metric', 'plane', '--icp-normals-k', '33'], base + ['--icp-normals-radius', '1'],
                  base + ['--icp-metric', 'plane', '--icp-normals-radius', '0'],
                  base + ['--icp-metric', 'plane', '--icp-normals-radius', 'inf'],
                  base + ['--icp-metric', 'plane', '--icp-normals-radius', 'nan']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)

    class NoSamples(object):
        has_cameras = True

        def __len__(self):
            return 0
    tr = engine.Trainer.__new__(engine.Trainer)
    tr.model, tr.device = torch.nn.Identity(), torch.device('cpu')
    keys = list(tr.validate(NoSamples(), icp={'iters': 2}))
    assert list(tr.validate(NoSamples(), icp={'iters': 2, 'metric': 'plane', 'normals_k': 8, 'normals_radius': 2.0})) == keys
    assert list(tr.validate(NoSamples(), icp={'metric': 'point'})) == keys
    for bad in ({'metric': 'line'}, {'normals_k': 8}, {'metric': 'point', 'normals_radius': 1.0}):
        with pytest.raises(_lib.HplError):
            tr.validate(NoSamples(), icp=bad)
