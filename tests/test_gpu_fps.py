"""GPU: hpl_fps / ops.fps, flownet.fps_sample, data.KITTI(fps=...) and engine --fps against the numpy restatement
tests/fps_oracle.py.  Every output equals the restatement bit for bit, on both kernel paths: the only float operations are the
subtractions, products and sums of d2 in a stated order and an exact min, and the selection is an integer maximum, so nothing
here has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import fps_oracle as FO
from batch64 import counts64, prefix_of
from hplflownet_amd import _lib, data, flownet, ops

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
KEYS = ('out_pc', 'out_attr', 'idx', 'dist', 'cover', 'stats')
PATHS = {'resident': 1, 'rounds': 2}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(pc, m, attr=None, start=None, prefix=None, path='auto', **kw):
    """ops.fps of host arrays (or device tensors) -> dict of host arrays."""
    t = pc if torch.is_tensor(pc) else dev(pc)
    a = attr if attr is None or torch.is_tensor(attr) else dev(attr)
    out = ops.fps(t, m, a, start=start, prefix=prefix, path=path, return_cover=True, **kw)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in zip(KEYS, out)}


def assert_same(got, want, what=''):
    for k in KEYS:
        if want[k] is None or got[k] is None:
            assert want[k] is None and got[k] is None, (what, k)
        else:
            g, w = torch.from_numpy(np.asarray(got[k])), torch.from_numpy(np.asarray(want[k]))
            assert g.dtype == w.dtype and torch.equal(g, w), (what, k, np.flatnonzero((g != w).numpy().reshape(-1))[:8])


def kinds(n, seed):
    """Four clouds of n points: uniform; the integer grid (ties on every round); a few positions many times over (it stops early);
    uniform with points that are not finite, the first one among them."""
    k = 1
    while k ** 3 < n:
        k += 1
    dup = np.tile(FO.cloud(max(1, n // 4), seed + 1), (1, 5))[:, :n]
    bad = FO.cloud(n, seed + 2)
    bad[0, 0] = np.nan
    if n > 2:
        bad[1, n // 2], bad[2, n - 1] = np.inf, -np.inf
    return [FO.cloud(n, seed), FO.grid(k)[:, :n], dup, bad]


# ----------------------------------------------------------------------------- both paths, forced, at every small size
@pytest.mark.parametrize('path', ['resident', 'rounds'])
@pytest.mark.parametrize('n', SIZES)
def test_both_paths_equal_the_restatement(n, path):
    parts = kinds(n, 7 * n)
    pc, prefix = np.concatenate(parts, axis=1), prefix_of([n] * len(parts))
    attr = np.random.RandomState(n).normal(0, 1, (2, pc.shape[1])).astype(np.float32)
    # the start: none; then given -- in the middle, the last point, a twin of point 0, and the cloud's NaN
    starts = (None, [n // 2, n - 1, min(n - 1, max(1, n // 4)), 0])
    for m in sorted({1, 2, min(n, 64) if n > 65 else n, min(n + 5, 64) if n > 65 else n + 5}):
        for start in starts:
            want = FO.sample(pc, m, attr, start, prefix, PATHS[path])
            assert_same(run(pc, m, attr, start, prefix, path), want, (n, m, path, start))
            if m >= n + 5:                                    # the grid is exhausted, the duplicates stop early
                assert want['stats'][1, 0] == n and want['stats'][2, 0] == max(1, n // 4) and want['stats'][3, 1] < n


# ----------------------------------------------------------------------------- the resident path's capacity
def test_the_resident_boundary():
    cap = ops.fps_resident_capacity()
    big = FO.cloud(cap + 1, 5, extent=50.0)
    both = np.concatenate([big[:, :cap - 1], big[:, 1:]], axis=1)             # n = capacity - 1 and n = capacity in one call
    prefix = [0, cap - 1, 2 * cap - 1]
    assert_same(run(both, 8, None, [cap - 2, cap - 1], prefix, 'resident'), FO.sample(both, 8, None, [cap - 2, cap - 1], prefix, 1))
    got = run(big, 8, None, [cap])                            # n = capacity + 1: auto takes the rounds
    assert got['stats'][0].tolist() == [8, cap + 1, 0, 2]
    assert_same(got, FO.sample(big, 8, None, [cap], None, 2))
    assert run(big[:, :cap], 8)['stats'][0, 3] == 1           # (and the resident path when the cloud fits)
    with pytest.raises(_lib.HplError) as e:
        run(big, 8, path='resident')
    assert _lib.load().hpl_last_error().startswith(b'hpl_fps: a cloud of %d points' % (cap + 1)) and 'hpl_fps: a cloud' in str(e.value)


# ----------------------------------------------------------------------------- the rounds path's workgroups
def test_rounds_over_several_workgroups():
    """A workgroup of the rounds path takes 1 024 points, more once a cloud would need over 256 of them.  Clouds of 3 workgroups
    with a partial last one, of exactly 256 workgroups and of 206 wider ones; an outlier at the last index makes the last
    workgroup win round 1, and the start lies in the first."""
    for n, m in ((2 * 1024 + 300, 40), (256 * 1024, 3), (256 * 1024 + 777, 3)):
        pc = FO.cloud(n, n % 1000)
        pc[:, n - 1] = [500.0, -500.0, 500.0]
        attr = np.arange(n, dtype=np.float32)[None]
        want = FO.sample(pc, m, attr, [3], None, 2)
        assert want['idx'][0, :2].tolist() == [3, n - 1]
        assert_same(run(pc, m, attr, [3], path='rounds'), want, n)


# ----------------------------------------------------------------------------- ragged batches
def cloud_bits(o, b, m, p0, p1):
    return (o['out_pc'][:, b * m:(b + 1) * m].tobytes(), o['out_attr'][:, b * m:(b + 1) * m].tobytes(), o['idx'][b].tobytes(),
            o['dist'][b].tobytes(), o['cover'][p0:p1].tobytes(), o['stats'][b].tobytes())


@pytest.mark.parametrize('path', ['resident', 'rounds'])
def test_ragged_batches_equal_their_clouds(path):
    # three clouds, the middle one empty, the last one stopping early beside one that does not
    parts = [FO.cloud(300, 1), FO.cloud(0, 2), np.tile(FO.cloud(9, 3), (1, 30))]
    pc, prefix = np.concatenate(parts, axis=1), [0, 300, 300, 570]
    attr = np.random.RandomState(3).normal(0, 1, (3, 570)).astype(np.float32)
    want = FO.sample(pc, 20, attr, None, prefix, PATHS[path])
    assert want['stats'].tolist() == [[20, 300, 0, PATHS[path]], [0, 0, 0, PATHS[path]], [9, 270, 0, PATHS[path]]]
    assert_same(run(pc, 20, attr, None, prefix, path), want)
    # B = 64 (tests/batch64.py): empty clouds at the ends and around 32, clouds of 2 100 and 1 025 points over several workgroups
    counts = counts64()
    parts = [FO.cloud(n, 100 + i) for i, n in enumerate(counts)]
    parts[13] = np.tile(FO.cloud(5, 13), (1, 8))[:, :counts[13]]              # 37 points at 5 positions
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(counts)
    attr = np.random.RandomState(4).normal(0, 1, (2, pc.shape[1])).astype(np.float32)
    start = [max(0, n - 1) for n in counts]
    m = 48
    got = run(pc, m, attr, start, prefix, path)
    assert_same(got, FO.sample(pc, m, attr, start, prefix, PATHS[path]))
    assert got['stats'][13, 0] == 5 and got['stats'][40, 0] == m and got['stats'][0].tolist() == [0, 0, 0, PATHS[path]]
    for b, n in enumerate(counts):
        if n:
            p0, p1 = prefix[b], prefix[b + 1]
            alone = run(pc[:, p0:p1], m, attr[:, p0:p1], [start[b]], [0, n], path)
            assert cloud_bits(got, b, m, p0, p1) == cloud_bits(alone, 0, m, 0, n), b


# ----------------------------------------------------------------------------- strides, channels, the workspace
def pair(n, seed, extent=6.0):
    """A corresponding pair: sf a small flow, pc2 = pc1 + sf in float32, so that pc2 - pc1 is sf again bit for bit."""
    p1 = FO.cloud(n, seed, extent=extent)
    p2 = p1 + np.random.RandomState(seed).normal(0, 0.05, p1.shape).astype(np.float32)
    return p1, p2, p2 - p1


@pytest.mark.parametrize('path', ['resident', 'rounds'])
def test_strided_views_channels_and_the_workspace(path):
    n, m = 1500, 33
    p1, p2, sf = pair(n, 21)
    prefix = [0, 700, n]
    wide = torch.full((3, n + 21), float('nan'), device='cuda')
    wide[:, 9:9 + n] = dev(p1)
    for C in (1, 8):
        attr = np.concatenate([p2, sf, p1[:2]])[:C]
        wattr = torch.full((C, n + 3), float('nan'), device='cuda')
        wattr[:, 1:1 + n] = dev(attr)
        out = torch.full((3, 2 * m + 11), float('nan'), device='cuda')
        res = ops.fps(wide[:, 9:9 + n], m, wattr[:, 1:1 + n], prefix=prefix, path=path, return_cover=True, out=out[:, 2:2 + 2 * m])
        assert res[0].data_ptr() == out[:, 2:].data_ptr() and torch.isnan(out[:, :2]).all() and torch.isnan(out[:, 2 + 2 * m:]).all()
        want = FO.sample(p1, m, attr, None, prefix, PATHS[path])
        assert_same({k: x.cpu().numpy() for k, x in zip(KEYS, res)}, want, C)
    assert torch.equal(res[1][:3] - res[0], res[1][3:6])      # pc2' - pc1' == sf', exactly: a pair stays a pair
    with pytest.raises(_lib.HplError):
        ops.fps(wide[:, 9:9 + n], 500, prefix=prefix, path=path, out=wide[:, 3:1003])     # an output over its input
    # a second and a third call on the same workspace: another cloud in between, then the same bits again
    first = run(p1, m, attr, None, prefix, path)
    run(FO.cloud(n, 99, extent=900.0), 2 * m, None, None, [0, n], path)
    assert_same(run(p1, m, attr, None, prefix, path), first)
    assert_same(first, want)


# ----------------------------------------------------------------------------- flownet.fps_sample
def eq(t, a):
    return t.dtype == torch.float32 and torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)))


@pytest.mark.parametrize('form', ['single', 'batch', 'list'])
def test_fps_sample_forms(form):
    if form == 'single':
        ps = [pair(700, 31)]
        args = [dev(x) for x in ps[0]]
    elif form == 'batch':
        ps = [pair(600, 32), pair(600, 33)]
        args = [dev(np.stack([p[k] for p in ps])) for k in range(3)]
    else:
        ps = [pair(300, 34), pair(1025, 35), pair(57, 36)]
        args = [[dev(p[k]) for p in ps] for k in range(3)]
    B, K = len(ps), 128
    # corr=True: pc1 decides, pc2 and sf ride as six channels
    o1, o2, osf, stats, ix = flownet.fps_sample(*args, num_points=K, corr=True, return_index=True)
    assert stats.shape == (B, 4) and len(o1) == len(o2) == len(osf) == len(ix) == B
    for b, (p1, p2, sf) in enumerate(ps):
        w = FO.sample_cloud(p1, K, np.concatenate([p2, sf]))
        c = w['count']
        assert c == min(K, p1.shape[1]) and stats[b, :3].tolist() == [c, p1.shape[1], 0] and o1[b].shape == (3, c)
        assert eq(o1[b], w['out_pc'][:, :c]) and eq(o2[b], w['out_attr'][:3, :c]) and eq(osf[b], w['out_attr'][3:, :c])
        assert ix[b].dtype == torch.int64 and np.array_equal(ix[b].cpu().numpy(), w['idx'][:c])
        assert torch.equal(o2[b] - o1[b], osf[b]) and eq(o1[b], p1[:, w['idx'][:c]])
    assert flownet.fps_sample(args[0], args[1], num_points=K)[2] is None
    alone = flownet.fps_sample(args[0], num_points=K)
    assert alone[1] is None and alone[2] is None and all(torch.equal(x, y) for x, y in zip(alone[0], o1))
    # a seed draws every cloud's start on the host; a start is taken as it is
    sizes = [p[0].shape[1] for p in ps]
    rs = np.random.RandomState(5)
    drawn = [int(rs.randint(0, n)) for n in sizes]
    seeded = flownet.fps_sample(*args, num_points=K, seed=5, return_index=True)
    given = flownet.fps_sample(*args, num_points=K, start=drawn, return_index=True)
    for b in range(B):
        assert int(seeded[4][b][0]) == drawn[b] and torch.equal(seeded[4][b], given[4][b]) and torch.equal(seeded[0][b], given[0][b])
    # corr=False: every cloud on its own, as two separate calls; sf with pc1
    o1, o2, osf, stats, ix = flownet.fps_sample(*args, num_points=K, corr=False, return_index=True)
    s1 = flownet.fps_sample(args[0], None, args[2], num_points=K, return_index=True)
    s2 = flownet.fps_sample(args[1], num_points=K, return_index=True)
    assert stats.shape == (2, B, 4) and torch.equal(stats[0], s1[3]) and torch.equal(stats[1], s2[3]) and len(ix) == 2 * B
    for b in range(B):
        assert torch.equal(o1[b], s1[0][b]) and torch.equal(o2[b], s2[0][b]) and torch.equal(osf[b], s1[2][b])
        assert torch.equal(ix[b], s1[4][b]) and torch.equal(ix[B + b], s2[4][b])
        w = FO.sample_cloud(ps[b][1], K)
        assert eq(o2[b], w['out_pc'][:, :w['count']])


# ----------------------------------------------------------------------------- the reader and the engine
def test_reader_and_engine_sample_frames(tmp_path):
    from hplflownet_amd import engine
    root = tmp_path / 'KITTI_processed_occ_final'
    frames = {}
    for f, n in enumerate((2600, 900, 3100)):
        d = root / ('%06d' % f)
        d.mkdir(parents=True)
        p1, p2, _ = pair(n, 50 + f, extent=8.0)
        frames[f] = (str(d), np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T))
        np.save(str(d / 'pc1.npy'), frames[f][1])
        np.save(str(d / 'pc2.npy'), frames[f][2])
    K = 1024
    reader = data.KITTI(None, str(tmp_path), device='cuda', fps=K)
    for f, (path, a1, a2) in frames.items():
        keep = ~((a1[:, 1] < -1.4) & (a2[:, 1] < -1.4))          # the ground rule first
        w = FO.sample_cloud(a1[keep].T, K, a2[keep].T)
        c = w['count']
        o1, o2 = reader.load(path)
        assert c == min(K, keep.sum()) and (c == K) == (f != 1) and o1.shape == o2.shape == (c, 3)      # exactly K, or what there is
        assert np.array_equal(o1, w['out_pc'][:, :c].T) and np.array_equal(o2, w['out_attr'][:, :c].T)
    both = data.KITTI(None, str(tmp_path), device='cuda', voxel=0.5, fps=256)                          # behind the voxel grid
    v = data.KITTI(None, str(tmp_path), device='cuda', voxel=0.5).load(frames[0][0])
    o1, o2 = both.load(frames[0][0])
    w = FO.sample_cloud(v[0].T, 256, v[1].T)
    assert len(v[0]) > 256 and np.array_equal(o1, w['out_pc'].T) and np.array_equal(o2, w['out_attr'].T)
    s = reader[2]                                             # through __getitem__ (no transform): device tensors (3, K)
    o1, o2 = reader.load(frames[2][0])
    assert s[0].shape == (3, K) and torch.equal(s[0], dev(o1.T)) and torch.equal(s[1], dev(o2.T))
    res = engine.main(['--dataset', 'KITTI', '--evaluate', '--fps', '1024', '--batch-size', '2', '--ragged', '--data-root',
                       str(tmp_path), '--points', '8192', '--arch', 'HPLFlowNetShallow'])
    assert res and all(np.isfinite(v) for v in res.values()), res


# ----------------------------------------------------------------------------- the library call itself
def test_null_optional_outputs():
    n, m = 500, 20
    pc, attr = FO.cloud(n, 8), FO.cloud(n, 9)
    want = FO.sample(pc, m, attr, None, None, 1)
    t_pc, t_attr = dev(pc), dev(attr)
    idx = torch.full((m,), -7, dtype=torch.int32, device='cuda')
    dist, o_pc = torch.full((m,), -7.0, device='cuda'), torch.full((3, m), -7.0, device='cuda')
    stats = torch.full((1, 4), -7, dtype=torch.int32, device='cuda')
    lib = _lib.load()
    ws = torch.empty(lib.hpl_fps_workspace_bytes(1, n, m, 3), dtype=torch.uint8, device='cuda')
    _lib.check(lib.hpl_fps(t_pc.data_ptr(), n, t_attr.data_ptr(), n, 3, 1, (ctypes.c_int64 * 2)(0, n), None, m, 1, idx.data_ptr(),
                           dist.data_ptr(), o_pc.data_ptr(), m, None, m, None, stats.data_ptr(), ws.data_ptr(), ws.numel(),
                           _lib.stream()), 'hpl_fps')
    got = dict(out_pc=o_pc.cpu().numpy(), out_attr=None, idx=idx.cpu().numpy()[None], dist=dist.cpu().numpy()[None], cover=None,
               stats=stats.cpu().numpy())
    assert_same(got, dict(want, out_attr=None, cover=None))
