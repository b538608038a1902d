"""CPU: the numpy restatement of the device transforms (hpl_transform_pair, csrc/transforms.hip) -- Philox4x32-10 against its
known answers, the fmaf chain against the reference's vectors with the reference's own draws -- the host Philox of the
library, the --device-transforms command line and the argument refusals of the new ABI entries.

The restatement (`replay_draws`, `oracle`) is what tests/test_gpu_device_transforms.py compares the device against."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import GOLD, ROOT  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_transform_fixture as F  # noqa: E402

M32 = np.uint64(0xFFFFFFFF)
KNOWN = [  # (counter, key, output) of Philox4x32-10 (Random123's known answers)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
    """Philox4x32-10 of four counter words (scalars or equal-shape arrays) under a two-word key -> four uint32 arrays."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & M32 for c in counter]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def draws(M, seed, counter, purpose):
    """The Philox words of points 0 .. M-1 for one call and purpose (0 / 1 jitter, 2 / 3 selection keys)."""
    i = np.arange(M, dtype=np.uint64)
    return philox((i, counter & 0xFFFFFFFF, counter >> 32, purpose), (seed & 0xFFFFFFFF, seed >> 32))


def jitter(M, seed, counter, purpose, sigma, clip):
    """clip(sigma * N(0, 1), -clip, clip) as float32 from Box-Muller in fp64 (three normals a point); clip == 0: -0."""
    if clip == 0:
        return np.full((M, 3), -0.0, np.float32)
    w = [x.astype(np.float64) for x in draws(M, seed, counter, purpose)]
    s32 = 2.0 ** -32
    r0, t0 = np.sqrt(-2.0 * np.log((w[0] + 1.0) * s32)), 6.283185307179586 * (w[1] * s32)
    r1, t1 = np.sqrt(-2.0 * np.log((w[2] + 1.0) * s32)), 6.283185307179586 * (w[3] * s32)
    n = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], 1)
    return np.minimum(np.maximum(sigma * n, -clip), clip).astype(np.float32)


def sel_keys(M, seed, counter, purpose):
    w = draws(M, seed, counter, purpose)
    return ((w[0].astype(np.uint64) << np.uint64(32)) | w[1].astype(np.uint64)) >> np.uint64(1)


def fmaf(a, b, c):
    """float32 fused multiply-add (the product exact in extended precision, one rounding to float32 in effect)."""
    L = np.longdouble
    return (np.asarray(a, np.float32).astype(L) * L(np.float32(b)) + np.asarray(c, np.float32).astype(L)).astype(np.float32)


def dot_chain(p, m):
    """p . m of (M, 3) float32 by (3, 3) float32 as numpy computes it: fma(z, m[2][c], fma(y, m[1][c], x * m[0][c]))."""
    return np.stack([fmaf(p[:, 2], m[2, c], fmaf(p[:, 1], m[1, c], p[:, 0] * m[0, c])) for c in range(3)], 1)


def transform_all(p1, p2, P, j1=None, j2=None):
    """(a, b, sf) of every point.  P: dict of the hpl_transform_params values (numpy float32 m / shift / m2 / shift2)."""
    if not P['augment']:
        return p1, p2, p2 - p1
    M = p1.shape[0]
    if j1 is None:
        j1 = jitter(M, P['seed'], P['counter'], 0, P['sigma1'], P['clip1'])
    bias = P['shift'].reshape(1, 3) + j1
    a = dot_chain(p1, P['m']) + bias
    b = dot_chain(p2, P['m']) + bias
    b = dot_chain(b, np.ascontiguousarray(P['m2'].T)) + P['shift2'].reshape(1, 3)
    sf = b - a
    if not P['no_corr']:
        if j2 is None:
            j2 = jitter(M, P['seed'], P['counter'], 1, P['sigma2'], P['clip2'])
        b = b + j2
    return a, b, sf


def valid_mask(a, b, T):
    T = np.float32(T)
    return (a[:, 2] < T) & (b[:, 2] < T) if T > 0 else np.ones(a.shape[0], bool)


def oracle(p1, p2, P, j1=None, j2=None, sel1=None, sel2=None):
    """What hpl_transform_pair emits -> (pc1, pc2, sf) as (3, k) float32 or None, (i1, i2), (valid, k)."""
    a, b, sf = transform_all(p1, p2, P, j1, j2)
    idx = np.nonzero(valid_mask(a, b, P['T']))[0]
    V, n = idx.size, P['num_points']
    if V == 0:
        return None, (None, None), (0, 0)
    if sel1 is not None:
        i1 = np.asarray(sel1)
        i2 = np.asarray(sel2) if P['no_corr'] else i1
    elif n <= 0 or (V < n and P['less']):
        i1 = i2 = idx
    elif V < n:
        return None, (None, None), (V, 0)
    else:
        def pick(purpose):
            key = sel_keys(p1.shape[0], P['seed'], P['counter'], purpose)[idx]
            return idx[np.lexsort((idx, key))[:n]]
        i1 = pick(2)
        i2 = pick(3) if P['no_corr'] else i1
    return (a[i1].T.copy(), b[i2].T.copy(), sf[i1].T.copy()), (i1, i2), (V, len(i1))


def params_dict(kind, kw, seed=0, counter=0):
    """The params of a fixture case (DEPTH_THRESHOLD, NO_CORR, num_points, allow_less_points of kw) with identity motion and
    no jitter; replay_draws fills in the augmentation scalars."""
    dp = kw['dp']
    P = dict(T=dp['DEPTH_THRESHOLD'], no_corr=bool(dp['NO_CORR']), num_points=kw['n'], less=bool(kw['less']),
             augment=kind == 'Augmentation', seed=seed, counter=counter, sigma1=0., clip1=0., sigma2=0., clip2=0.,
             m=np.eye(3, dtype=np.float32), shift=np.zeros(3, np.float32), m2=np.eye(3, dtype=np.float32),
             shift2=np.zeros(3, np.float32))
    return P


def replay_draws(kind, kw, rng, M):
    """One call of the reference's transform replayed from `rng` (np.random.seed order, transforms.py:565-632): the scalars,
    jitter 1, jitter 2 (if corr) -> (P, j1, j2); the caller draws the choice on the mask."""
    from hplflownet_amd.data import _rot_y
    P = params_dict(kind, kw)
    j1 = j2 = None
    if kind == 'Augmentation':
        tg, q = kw['tg'], kw['p2']
        scale = np.diag(rng.uniform(tg['scale_low'], tg['scale_high'], 3).astype(np.float32))
        P['m'] = scale.dot(_rot_y(rng.uniform(-tg['degree_range'], tg['degree_range']), np.float32).T)
        P['shift'] = rng.uniform(-tg['shift_range'], tg['shift_range'], (1, 3)).astype(np.float32).ravel()
        j1 = np.clip(tg['jitter_sigma'] * rng.randn(M, 3), -tg['jitter_clip'], tg['jitter_clip']).astype(np.float32)
        P['m2'] = _rot_y(rng.uniform(-q['degree_range'], q['degree_range']), np.float32)
        P['shift2'] = rng.uniform(-q['shift_range'], q['shift_range'], (1, 3)).astype(np.float32).ravel()
        if not P['no_corr']:
            j2 = np.clip(q['jitter_sigma'] * rng.randn(M, 3), -q['jitter_clip'], q['jitter_clip']).astype(np.float32)
    return P, j1, j2


def replay_choice(P, mask, rng):
    """The reference's rng.choice on the valid indices (None when it does not draw)."""
    idx = np.nonzero(mask)[0]
    n = P['num_points']
    if n <= 0 or idx.size < n or idx.size == 0:
        return None, None
    i1 = rng.choice(idx, size=n, replace=False)
    i2 = rng.choice(idx, size=n, replace=False) if P['no_corr'] else None
    return i1.astype(np.int32), (i2.astype(np.int32) if i2 is not None else None)


# --------------------------------------------------------------------------- tests
def test_numpy_philox_known_answers():
    for ctr, key, want in KNOWN:
        got = [int(x) for x in philox(ctr, key)]
        assert got == list(want), ([hex(x) for x in got], ctr, key)


def test_library_philox_matches_known_answers_and_restatement():
    from hplflownet_amd import _lib
    lib = _lib.load()
    U4, U2 = ctypes.c_uint32 * 4, ctypes.c_uint32 * 2
    for ctr, key, want in KNOWN:
        out = U4()
        assert lib.hpl_philox4x32_10(U4(*ctr), U2(*key), out) == 0
        assert list(out) == list(want)
    rng = np.random.RandomState(5)
    for _ in range(50):
        ctr, key = rng.randint(0, 2 ** 32, 4, dtype=np.uint64), rng.randint(0, 2 ** 32, 2, dtype=np.uint64)
        out = U4()
        assert lib.hpl_philox4x32_10(U4(*[int(c) for c in ctr]), U2(*[int(k) for k in key]), out) == 0
        assert list(out) == [int(x) for x in philox(ctr, key)]
    assert lib.hpl_philox4x32_10(None, U2(), U4()) == -1


def test_restated_arithmetic_reproduces_reference_vectors():
    """With the reference's own draws the restatement (the device's fmaf chain) gives tests/golden/transforms.npz bit for bit."""
    G = np.load(os.path.join(GOLD, 'transforms.npz'))
    for tag, kind, kw, seed in F.CASES:
        p1, p2 = F.cloud_pair(seed)
        rng = np.random.RandomState(seed)
        for suf in ('', '_b'):
            P, j1, j2 = replay_draws(kind, kw, rng, p1.shape[0])
            a, b, _ = transform_all(p1, p2, P, j1, j2)
            s1, s2 = replay_choice(P, valid_mask(a, b, P['T']), rng)
            out, _, _ = oracle(p1, p2, P, j1, j2, s1, s2)
            for k, v in zip(('pc1', 'pc2', 'sf'), out):
                g = G['%s_%s%s' % (tag, k, suf)]
                assert g.dtype == v.dtype and g.shape == v.T.shape, (tag, k)
                assert np.array_equal(g.view(np.uint32), np.ascontiguousarray(v.T).view(np.uint32)), (tag, k, suf)


def test_selection_keys_order_uniformly_on_the_host():
    """The k-smallest-key rule itself: inclusion counts of 16 out of 64 over 4 000 calls are uniform (chi-square)."""
    from scipy import stats
    cnt = np.zeros(64)
    for c in range(4000):
        key = sel_keys(64, 7, c, 2)
        cnt[np.lexsort((np.arange(64), key))[:16]] += 1
    assert stats.chisquare(cnt).pvalue > 1e-3


def test_parse_args_device_transforms(tmp_path):
    from hplflownet_amd.engine import parse_args
    root = str(tmp_path)
    a = parse_args(['--dataset', 'FlyingThings3DSubset', '--data-root', root, '--device-transforms', '--train-batch-size', '2'])
    assert a.device_transforms and a.train_batch_size == 2
    a = parse_args(['--dataset', 'KITTI', '--data-root', root, '--evaluate', '--batch-size', '2', '--ragged',
                    '--device-transforms'])
    assert a.device_transforms and a.ragged
    assert not parse_args(['--dataset', 'KITTI', '--data-root', root, '--evaluate']).device_transforms
    assert not parse_args([]).device_transforms
    with pytest.raises(SystemExit):
        parse_args(['--device-transforms'])
    with pytest.raises(SystemExit):
        parse_args(['--dataset', 'synthetic', '--evaluate', '--device-transforms'])


def test_transform_entries_refuse_bad_arguments_without_a_gpu():
    from hplflownet_amd import _lib
    lib = _lib.load()
    P = _lib.TransformParams()
    P.num_points = 500
    fake = 1 << 20                                   # never dereferenced: every refusal comes before a copy or launch
    big = 1 << 40

    def call(pc1=fake, pc2=fake, M=1000, params=ctypes.byref(P), sel1=None, sel2=None, n_sel=0, out=fake, cap=1000,
             counts=fake, ws=fake, wsb=big):
        return lib.hpl_transform_pair(pc1, pc2, M, params, None, None, sel1, sel2, n_sel, out, out, out, cap, counts, ws, wsb,
                                      None)

    cases = [
        (dict(pc1=None), b'null'),
        (dict(params=None), b'null'),
        (dict(counts=None), b'null'),
        (dict(M=0), b'points'),
        (dict(M=-5), b'points'),
        (dict(M=2 ** 31), b'points'),
        (dict(M=2 ** 31 - 1), b'points'),
        (dict(pc2=fake + 2), b'aligned'),
        (dict(out=fake + 1), b'aligned'),
        (dict(ws=fake + 64), b'256-byte'),
        (dict(wsb=16), b'workspace'),
        (dict(cap=499), b'capacity'),
        (dict(M=400, cap=399), b'capacity'),
        (dict(sel2=fake), b'sel'),
        (dict(sel1=fake, n_sel=0), b'hook'),
        (dict(sel1=fake, n_sel=1001), b'hook'),
    ]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.hpl_last_error(), (kw, lib.hpl_last_error())
    P.no_corr = 1
    assert call(sel1=fake, n_sel=10) == -1 and b'sel' in lib.hpl_last_error()
    P.no_corr, P.jitter_clip1 = 0, -1.0
    assert call() == -1 and b'clip' in lib.hpl_last_error()
    cap = ctypes.c_int64()
    assert lib.hpl_transform_capacity(1000, 8192, ctypes.byref(cap)) == 0 and cap.value == 1000
    assert lib.hpl_transform_capacity(10 ** 6, 8192, ctypes.byref(cap)) == 0 and cap.value == 8192
    assert lib.hpl_transform_capacity(777, -1, ctypes.byref(cap)) == 0 and cap.value == 777
    assert lib.hpl_transform_capacity(0, 10, ctypes.byref(cap)) == -1
    assert lib.hpl_transform_capacity(2 ** 31, 10, ctypes.byref(cap)) == -1
    assert lib.hpl_transform_workspace_bytes(0) == 0 and lib.hpl_transform_workspace_bytes(2 ** 31) == 0
