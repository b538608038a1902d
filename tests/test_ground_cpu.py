"""CPU: hpl_ground_fit's declaration, export and refusals (no device needed), its workspace size, the numpy restatement
tests/ground_oracle.py -- Philox against the library's host entry, the fitted plane against the generator's truth, the tilt
gate --, the engine's --ground arguments and the reader's refusal of a CPU device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT
from hplflownet_amd import _lib
import ground_oracle as G

I64 = ctypes.c_int64
SEEDS = range(20)


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+hpl_ground_fit\s*\(', body) and re.search(r'\bint64_t\s+hpl_ground_fit_workspace_bytes\s*\(', body)
    assert 'hpl_ground_fit' in _lib.EXPORTS and 'hpl_ground_fit_workspace_bytes' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'hpl_ground_fit')
    from hplflownet_amd import build
    assert 'ground_fit.hip' in build.SOURCES
    # Philox lives in one shared header: the transforms and the ground fit both include it, neither defines it
    csrc = os.path.join(ROOT, 'hplflownet_amd', 'csrc')
    for name in ('transforms.hip', 'ground_fit.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "philox.h"' in text and '0xD2511F53' not in text
    assert '0xD2511F53' in open(os.path.join(csrc, 'philox.h')).read()


def test_philox_restatement_matches_the_library():
    lib = _lib.load()
    rng = np.random.RandomState(0)
    cases = [((0, 0, 0, 0), (0, 0)), ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF)), ((5, 1, 0, G.PURPOSE), (7, 0))]
    cases += [(tuple(int(x) for x in rng.randint(0, 2 ** 32, 4, dtype=np.uint64)),
               tuple(int(x) for x in rng.randint(0, 2 ** 32, 2, dtype=np.uint64))) for _ in range(50)]
    for cnt, key in cases:
        out = (ctypes.c_uint32 * 4)()
        assert lib.hpl_philox4x32_10((ctypes.c_uint32 * 4)(*cnt), (ctypes.c_uint32 * 2)(*key), out) == 0
        assert list(out) == G.philox4x32_10(np.array(cnt, np.uint32), key).tolist()
    # the published known-answer vectors of Philox4x32-10 (Random123's kat_vectors)
    assert G.philox4x32_10(np.zeros(4, np.uint32), (0, 0)).tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    # vectorised over the hypotheses, and the indices stay inside the cloud
    d = G.draws(4099, 1024, seed=3, call=(1 << 40) + 5)
    assert d.shape == (1024, 3) and d.min() >= 0 and d.max() < 4099
    one = G.philox4x32_10(np.array([77, 5, 1 << 8, G.PURPOSE], np.uint32), (3, 0))
    assert d[77].tolist() == [(int(w) * 4099) >> 32 for w in one[:3]]


def call(pc=8, pc_ld=100, batch=1, prefix=(0, 100), up=(0, 1, 0), min_cos=0.9, hyps=64, tau=0.1, refine=2, cut=0.3, plane=8,
         stats=8, votes=None, height=None, ground=None, keep=8, ws=8, ws_bytes=1 << 24):
    """hpl_ground_fit with fake (never dereferenced) device addresses: every refusal comes before any launch."""
    prefix = (I64 * len(prefix))(*prefix) if prefix is not None else None
    up = (ctypes.c_float * 3)(*up) if up is not None else None
    return _lib.load().hpl_ground_fit(pc, pc_ld, batch, prefix, up, min_cos, hyps, tau, refine, cut, 0, 0, plane, stats, votes,
                                      height, ground, keep, ws, ws_bytes, None)


NAN, INF = float('nan'), float('inf')


@pytest.mark.parametrize('kw', [
    dict(batch=0), dict(batch=65, prefix=(0,) * 66), dict(batch=-1), dict(hyps=0), dict(hyps=1025), dict(hyps=-1),
    dict(refine=-1), dict(refine=9), dict(tau=0.0), dict(tau=-0.1), dict(tau=INF), dict(tau=NAN),
    dict(cut=-0.1), dict(cut=INF), dict(cut=NAN), dict(min_cos=0.0), dict(min_cos=-0.5), dict(min_cos=1.5), dict(min_cos=NAN),
    dict(up=(0, 0, 0)), dict(up=(0, INF, 0)), dict(up=(NAN, 1, 0)), dict(up=None),
    dict(prefix=(1, 100)), dict(batch=2, prefix=(0, 60, 50)), dict(pc_ld=99),
    dict(pc=None), dict(plane=None), dict(stats=None), dict(prefix=None), dict(ws=None),
    dict(ws_bytes=0), dict(ws_bytes=_lib.load().hpl_ground_fit_workspace_bytes(1, 100, 64) - 1),
    dict(pc=6), dict(plane=10), dict(stats=6), dict(votes=5), dict(height=7), dict(keep=9), dict(ws=12),
    dict(prefix=(0, 2 ** 31 // 3 + 1), pc_ld=2 ** 31, ws_bytes=1 << 40), dict(prefix=(0, 2 ** 60), pc_ld=2 ** 60, ws_bytes=1 << 62),
], ids=lambda kw: '-'.join('%s' % k for k in kw))
def test_refusals_without_a_device(kw):
    assert call(**kw) == -1                                   # HPL_EINVAL
    assert b'hpl_ground_fit' in _lib.load().hpl_last_error()


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch, whatever the (valid) other arguments."""
    assert call(prefix=(0, 0), pc_ld=0) == 0
    assert call(batch=3, prefix=(0, 0, 0, 0), pc_ld=0, hyps=1024, refine=0, cut=0.0, min_cos=1.0, up=(0, 0, -2), ground=3) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_ground_fit_workspace_bytes
    assert f(0, 10, 64) == -1 and f(65, 10, 64) == -1 and f(1, -1, 64) == -1 and f(1, 2 ** 31 // 3 + 1, 64) == -1
    assert f(1, 10, 0) == -1 and f(1, 10, 1025) == -1
    ns = [0, 1, 3, 1024, 1025, 8192, 450000, 2 ** 29]
    for b in (1, 2, 16, 64):
        for h in (1, 64, 1024):
            vals = [f(b, n, h) for n in ns]
            assert all(v > 0 and v % 8 == 0 for v in vals) and vals == sorted(vals)
            assert all(f(b + 1, n, h) >= f(b, n, h) for n in ns if b < 64)
            assert all(f(b, n, h + 1) >= f(b, n, h) for n in ns if h < 1024)
    assert f(2, 900000, 1024) < 1 << 20                       # records, counts and 84 bytes per 1024 points


def test_wrapper_refuses_before_the_library():
    from hplflownet_amd import ops
    pc = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        ops.ground_fit(pc)                                    # a host tensor: no CPU fallback
    for kw in (dict(hyps=0), dict(hyps=1025), dict(hyps=2.0), dict(refine=-1), dict(refine=9), dict(tau=0.0), dict(tau=NAN),
               dict(cut=-1.0), dict(cut=INF), dict(max_tilt_deg=90.0), dict(max_tilt_deg=-1.0), dict(max_tilt_deg=NAN),
               dict(up=(0, 0, 0)), dict(up=(0, 1)), dict(up=(0, NAN, 1)), dict(seed=-1), dict(call=1 << 64)):
        with pytest.raises(_lib.HplError):
            ops.ground_fit(pc, **kw)
    assert ops.ground_min_cos(0.0) == 1.0 and ops.ground_min_cos(20.0) == float(G.min_cos_of(20.0))


def test_remove_ground_refuses_host_tensors_and_bad_forms():
    from hplflownet_amd import flownet
    a = torch.zeros(3, 10)
    with pytest.raises(_lib.HplError):
        flownet.remove_ground(a, a)                           # host tensors
    for args, kw in (((a, torch.zeros(3, 9)), {}), ((a, a, torch.zeros(3, 9)), {}), (([a], [a, a]), {}),
                     ((a, a), dict(return_votes=True)), ((a, a), dict(corr=False, return_mask=True)),
                     ((torch.zeros(10, 3), a), {}), (([a] * 33, [a] * 33), {})):
        with pytest.raises(_lib.HplError):
            flownet.remove_ground(*args, **kw)


# ----------------------------------------------------------------------------- the restatement
def worst_of(n, hyps, tilt, **scene_kw):
    """The largest angle (degrees) to the true normal and the largest offset error (metres) over the seeds."""
    ang = off = 0.0
    for seed in SEEDS:
        pc, truth = G.scene(n, seed, **scene_kw)
        o = G.fit(pc, hyps=hyps, tau=0.1, refine=2, seed=seed, max_tilt_deg=tilt)
        assert o['status'] == 1 and o['rounds'] == 2
        assert o['plane64'][:3] @ truth['up'] > 0 and abs(np.linalg.norm(o['plane64'][:3]) - 1) <= 1e-12
        ang = max(ang, G.angle_deg(o['plane64'][:3], truth['normal']))
        off = max(off, abs(o['plane64'][3] - truth['d']))
    return ang, off


@pytest.mark.parametrize('n', [1000, 4099])
def test_restatement_finds_the_true_plane(n):
    ang, off = worst_of(n, 128, 20.0)
    print('ground 50 %%, n = %d, 128 hypotheses: worst angle %.4f deg, worst offset %.2f mm' % (n, ang, off * 1e3))
    assert ang <= 0.1 and off <= 0.02


@pytest.mark.parametrize('n', [1000, 4099])
def test_restatement_finds_the_ground_beside_a_larger_wall(n):
    ang, off = worst_of(n, 512, 20.0, ground=0.3, wall=0.4)
    print('ground 30 %%, wall 40 %%, n = %d, 512 hypotheses: worst angle %.4f deg, worst offset %.2f mm' % (n, ang, off * 1e3))
    assert ang <= 0.1 and off <= 0.02


@pytest.mark.parametrize('n', [1000, 4099])
def test_an_open_gate_returns_the_wall(n):
    """The same wall-dominant scenes with the gate at 89.9 degrees: the wall collects more votes, so the gate did the work.
    (The wall's normal is at 90 degrees from up, 0.1 degrees outside even this gate, so the winner is a wall plane leaning that
    much or more: the bar is 1 degree from the wall's normal, against 85 for the ground's.)"""
    wins = 0
    for seed in SEEDS:
        pc, truth = G.scene(n, seed, ground=0.3, wall=0.4)
        o = G.fit(pc, hyps=512, tau=0.1, refine=2, seed=seed, max_tilt_deg=89.9)
        wins += G.angle_deg(o['plane64'][:3], truth['wall_normal']) <= 1.0
    assert wins == len(SEEDS)


def test_other_up_axes_and_a_larger_tilt():
    for up, vec in (('z', (0, 0, 1)), ('x', (1, 0, 0))):
        pc, truth = G.scene(4099, 1, tilt_deg=12.0, height=2.3, up=up)
        o = G.fit(pc, up=vec, hyps=128, seed=1)
        assert G.angle_deg(o['plane64'][:3], truth['normal']) <= 0.1 and abs(o['plane64'][3] - truth['d']) <= 0.02
    pc, truth = G.scene(1000, 2, tilt_deg=12.0)
    o = G.fit(pc, hyps=256, seed=2, max_tilt_deg=5.0)        # the ground is outside the gate: whatever wins is not it
    assert o['status'] == 0 or G.angle_deg(o['plane64'][:3], truth['up']) <= 5.0 + 1e-3


def jacobi_smallest(C):
    """The library's method for the refinement's normal: cyclic Jacobi sweeps on the symmetric 3x3 matrix."""
    A, V = C.copy(), np.eye(3)
    for _ in range(12):
        off = (A * A).sum() - (np.diag(A) ** 2).sum()
        if not off > 1e-32 * (A * A).sum():
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0.0:
                continue
            theta = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(t * t + 1.0)
            J = np.eye(3)
            J[p, p] = J[q, q] = c
            J[p, q], J[q, p] = t * c, -t * c
            A, V = J.T @ A @ J, V @ J
    v = V[:, int(np.argmin(np.diag(A)))]
    return v / np.sqrt(v @ v)


def test_jacobi_and_eigh_agree_on_the_scenes():
    """The GPU refinement test allows 2^-22 between the library (Jacobi) and the restatement (eigh).  Both are backward stable:
    the eigenvector's error is about eps |C| / gap, and on a ground sheet that spans tens of metres with centimetre noise the
    smallest eigenvalue is separated from the next by about the largest itself, so the two agree to a few 1e-16 .. 1e-13 --
    nine orders below the bar."""
    worst = 0.0
    for n, seed in ((1000, 0), (4099, 1), (4099, 2)):
        pc, _ = G.scene(n, seed)
        o = G.fit(pc, hyps=64, refine=0, seed=seed)
        inl = np.abs(G.heights(pc, o['plane64'])) <= 0.1
        dp = pc.astype(np.float64)[:, inl] - pc.astype(np.float64)[:, :1]
        mu = dp.mean(1)
        C = dp @ dp.T - np.outer(inl.sum() * mu, mu)
        e, j = np.linalg.eigh(C)[1][:, 0], jacobi_smallest(C)
        worst = max(worst, min(np.abs(e - j).max(), np.abs(e + j).max()))
    print('largest |eigh - Jacobi| over the normals: %.3g' % worst)
    assert worst <= 1e-12


def test_degenerate_clouds_have_status_0():
    pc, _ = G.scene(50, 1)
    line = np.stack([np.arange(40.0), 2 * np.arange(40.0), -np.arange(40.0)]).astype(np.float32)
    for cloud in (pc[:, :0], pc[:, :1], pc[:, :2], line, np.full((3, 10), np.nan, np.float32)):
        o = G.ground_fit(cloud, hyps=64)
        n = cloud.shape[1]
        assert o['stats'].tolist() == [[0, -1, 0, n]] and not o['plane'].any() and not o['ground'].any()
        assert (o['votes'] == -1).all() and not o['height'].any() and o['keep_idx'].tolist() == list(range(n))


# ----------------------------------------------------------------------------- engine, reader
def test_engine_argument_errors():
    from hplflownet_amd import engine
    base = ['--dataset', 'KITTI', '--evaluate', '--data-root', '/nowhere']
    assert engine.parse_args(base).ground == 'threshold' and engine.parse_args(base).ground_fit is None
    assert engine.parse_args([]).ground_fit is None
    assert engine.parse_args(base + ['--ground', 'plane']).ground_fit == \
        {'tau': 0.1, 'cut': 0.3, 'hyps': 256, 'max_tilt_deg': 20.0, 'up': (0.0, 1.0, 0.0)}
    got = engine.parse_args(base + ['--ground', 'plane', '--ground-tau', '0.2', '--ground-cut', '0', '--ground-hyps', '1024',
                                    '--ground-tilt', '35', '--ground-up', '0', '0', '-1']).ground_fit
    assert got == {'tau': 0.2, 'cut': 0.0, 'hyps': 1024, 'max_tilt_deg': 35.0, 'up': (0.0, 0.0, -1.0)}
    plane = base + ['--ground', 'plane']
    for extra in (['--ground', 'plane'], ['--dataset', 'FlyingThings3DSubset', '--data-root', '/nowhere', '--ground', 'plane'],
                  base + ['--ground', 'ransac'], base + ['--ground-tau', '0.1'], base + ['--ground-cut', '0.3'],
                  base + ['--ground-hyps', '64'], base + ['--ground-tilt', '10'], base + ['--ground-up', '0', '1', '0'],
                  base + ['--ground', 'threshold', '--ground-tau', '0.1'],
                  plane + ['--ground-tau', '0'], plane + ['--ground-tau', 'inf'], plane + ['--ground-tau', 'nan'],
                  plane + ['--ground-cut', '-0.1'], plane + ['--ground-cut', 'nan'], plane + ['--ground-hyps', '0'],
                  plane + ['--ground-hyps', '1025'], plane + ['--ground-tilt', '90'], plane + ['--ground-tilt', '-1'],
                  plane + ['--ground-up', '0', '0', '0'], plane + ['--ground-up', '0', 'nan', '1'], plane + ['--ground-up', '0', '1']):
        with pytest.raises(SystemExit):
            engine.parse_args(extra)


def test_reader_refuses_plane_removal_on_a_cpu_device(tmp_path):
    from hplflownet_amd import data
    d = tmp_path / 'KITTI_processed_occ_final' / '000000'
    d.mkdir(parents=True)
    pc = G.scene(64, 0)[0].T
    np.save(str(d / 'pc1.npy'), pc)
    np.save(str(d / 'pc2.npy'), pc)
    with pytest.raises(_lib.HplError):
        data.KITTI(None, str(tmp_path), remove_ground='plane', device='cpu')
    for kw in (dict(remove_ground='ransac'), dict(remove_ground=True, ground={'tau': 0.1}),
               dict(remove_ground='plane', device='cuda', ground={'seed': 1})):
        with pytest.raises(_lib.HplError):
            data.KITTI(None, str(tmp_path), **kw)
    # the threshold rule and no removal work on a CPU device as before
    for rg, want in ((True, pc[~(pc[:, 1] < -1.4)]), (False, pc)):
        got = data.KITTI(None, str(tmp_path), remove_ground=rg, device='cpu').load(str(d))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
