"""GPU: hpl_voxel_downsample / ops.voxel_downsample, flownet.voxel_downsample, data.KITTI(voxel=...) and engine --voxel
 against the numpy restatement tests/voxel_oracle.py.  Every output equals the restatement: the integers
exactly, the floats bit for bit (a NaN equals a NaN) -- the only operations are float64 additions in a stated order, one
division and one rounding, so nothing here has a tolerance.  The reduction takes a run of at most 32 members by one lane and
a longer one by its wave in chunks of 64: the built runs of 16, 17, 32, 33, 63, 64, 65 and 129 members lie either side of
both."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_oracle as VO
from batch64 import counts64, prefix_of
from hplflownet_amd import _lib, data, flownet, ops

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4099]
RUNS = [16, 17, 32, 33, 63, 64, 65, 129]                     # the lane / wave switch-over is 32, a wave's chunk 64
KEYS = ('out_pc', 'out_attr', 'count', 'rep', 'voxel_of', 'stats')
FLOATS = ('out_pc', 'out_attr')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(pc, attr=None, prefix=None, **kw):
    """ops.voxel_downsample of host arrays (or device tensors) -> dict of host arrays."""
    t = pc if torch.is_tensor(pc) else dev(pc)
    a = attr if attr is None or torch.is_tensor(attr) else dev(attr)
    out = ops.voxel_downsample(t, a, prefix=prefix, **kw)
    return {k: (None if x is None else x.cpu().numpy()) for k, x in zip(KEYS, out)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def assert_same(got, want, what=''):
    for k in KEYS:
        if want[k] is None or got[k] is None:
            assert want[k] is None and got[k] is None, (what, k)
        else:
            assert same_bits(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k] != want[k]).reshape(-1))[:8])


def box(n, seed, mean=4.0, lo=-3.0):
    """n uniform points in a cube that holds about n / mean unit cells, from `lo` on (it straddles 0 on every axis)."""
    side = max(1.0, (n / mean) ** (1.0 / 3.0))
    return (np.random.RandomState(seed).uniform(0, side, (3, n)) + lo).astype(np.float32)


def built_runs(seed):
    """A cloud whose voxels at edge 1 hold exactly RUNS members each, in random order."""
    rng = np.random.RandomState(seed)
    parts = [rng.uniform(0.05, 0.95, (3, m)) + np.array([[3.0 * i - 7], [-2.0], [5.0]]) for i, m in enumerate(RUNS)]
    pc = np.concatenate(parts, axis=1)
    return pc[:, rng.permutation(pc.shape[1])].astype(np.float32)


@pytest.fixture(scope='module')
def ragged():
    parts = [box(n, 10 + i) for i, n in enumerate(SIZES)] + [built_runs(5)]
    pc = np.concatenate(parts, axis=1)
    attr = np.random.RandomState(1).normal(0, 2, (8, pc.shape[1])).astype(np.float32)
    return pc, attr, prefix_of([p.shape[1] for p in parts])


# ----------------------------------------------------------------------------- the ragged batch, every channel count
@pytest.mark.parametrize('channels', [0, 1, 3, 6, 8])
def test_ragged_batch_equals_the_restatement(ragged, channels):
    pc, attr, prefix = ragged
    a = attr[:channels] if channels else None
    for mode in ('centroid', 'nearest'):
        # short runs (about 4 members a voxel, the built cloud's runs of 16 .. 129 beside them)
        want = VO.downsample(pc, a, 1.0, (0, 0, 0), mode, prefix)
        cnt = want['count'][prefix[-2]:prefix[-2] + want['stats'][-1, 0]]
        assert sorted(cnt.tolist()) == RUNS and 3.0 < want['stats'][-2, 1] / want['stats'][-2, 0] < 6.0
        assert_same(run(pc, a, prefix, voxel=1.0, mode=mode), want, (mode, 'short'))
        # one cell holds each whole cloud: runs of 1 .. 4099
        want = VO.downsample(pc, a, 1000.0, (-500, -500, -500), mode, prefix)
        assert want['stats'][:, 0].tolist() == [1] * len(want['stats']) and want['count'][prefix[-3]] == 4099
        assert_same(run(pc, a, prefix, voxel=1000.0, origin=(-500, -500, -500), mode=mode), want, (mode, 'one cell'))


# ----------------------------------------------------------------------------- row strides, optional outputs
def raw(pc, attr, prefix, voxel, mode, pad=0, skip=()):
    """The library call itself on buffers whose rows are `pad` elements apart beyond N, NaN / -7 filled; the outputs named in
    `skip` are NULL.  -> dict of host arrays (the padding included for the two float outputs)."""
    N, C, B = pc.shape[1], 0 if attr is None else attr.shape[0], len(prefix) - 1
    ld = N + pad
    fbuf = lambda rows: torch.full((max(rows, 1), ld), float('nan'), device='cuda')                     # noqa: E731
    ibuf = lambda: torch.full((N,), -7, dtype=torch.int32, device='cuda')                               # noqa: E731
    t_pc, t_attr, o_pc, o_attr = fbuf(3), fbuf(C), fbuf(3), fbuf(C)
    t_pc[:, :N] = dev(pc)
    if C:
        t_attr[:C, :N] = dev(attr)
    count, rep, voxel_of = ibuf(), ibuf(), ibuf()
    stats = torch.full((B, 4), -7, dtype=torch.int32, device='cuda')
    lib = _lib.load()
    nbytes = lib.hpl_voxel_downsample_workspace_bytes(B, N, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    keep = lambda name, t: None if name in skip else t.data_ptr()                                       # noqa: E731
    _lib.check(lib.hpl_voxel_downsample(t_pc.data_ptr(), ld, t_attr.data_ptr() if C else None, ld, C, B,
                                        (ctypes.c_int64 * (B + 1))(*prefix), voxel, (ctypes.c_float * 3)(0, 0, 0),
                                        VO.MODES[mode], o_pc.data_ptr(), ld, keep('out_attr', o_attr) if C else None, ld,
                                        keep('count', count), keep('rep', rep), keep('voxel_of', voxel_of), stats.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream()), 'hpl_voxel_downsample')
    return dict(out_pc=o_pc.cpu().numpy(), out_attr=o_attr[:C].cpu().numpy() if C else None, count=count.cpu().numpy(),
                rep=rep.cpu().numpy(), voxel_of=voxel_of.cpu().numpy(), stats=stats.cpu().numpy())


def test_row_strides_and_null_outputs(ragged):
    pc, attr, prefix = ragged
    N = pc.shape[1]
    for mode in ('centroid', 'nearest'):
        want = VO.downsample(pc, attr[:3], 1.0, (0, 0, 0), mode, prefix)
        got = raw(pc, attr[:3], prefix, 1.0, mode, pad=37)
        assert np.isnan(got['out_pc'][:, N:]).all() and np.isnan(got['out_attr'][:, N:]).all()        # the padding is untouched
        assert_same(dict(got, out_pc=got['out_pc'][:, :N], out_attr=got['out_attr'][:, :N]), want, mode)
        for name in ('out_attr', 'count', 'rep', 'voxel_of'):
            got = raw(pc, attr[:3], prefix, 1.0, mode, pad=5, skip=(name,))
            left = got[name] if name != 'out_attr' else got[name][:, :N]
            assert (np.isnan(left) if name == 'out_attr' else left == -7).all(), name                 # nobody wrote there
            for k in KEYS:
                if k != name:
                    assert same_bits(got[k][:, :N] if k in FLOATS else got[k], want[k]), (mode, name, k)
    # the wrapper reads strided views in place and writes a strided `out`
    wide = torch.full((3, N + 21), float('nan'), device='cuda')
    wide[:, 9:9 + N] = dev(pc)
    wattr = torch.full((6, N + 3), float('nan'), device='cuda')
    wattr[:, 1:1 + N] = dev(attr[:6])
    out = torch.full((3, N + 11), float('nan'), device='cuda')
    res = ops.voxel_downsample(wide[:, 9:9 + N], wattr[:, 1:1 + N], voxel=1.0, prefix=prefix, out=out[:, 2:2 + N])
    assert res[0].data_ptr() == out[:, 2:].data_ptr() and torch.isnan(out[:, :2]).all() and torch.isnan(out[:, 2 + N:]).all()
    assert_same({k: x.cpu().numpy() for k, x in zip(KEYS, res)}, VO.downsample(pc, attr[:6], 1.0, (0, 0, 0), 'centroid', prefix))
    with pytest.raises(_lib.HplError):
        ops.voxel_downsample(wide[:, 9:9 + N], voxel=1.0, prefix=prefix, out=wide[:, 3:3 + N])      # an output over its input


# ----------------------------------------------------------------------------- non-finite and out-of-range points
def test_invalid_points_and_non_finite_attributes():
    rng = np.random.RandomState(2)
    a, b, c = box(700, 31), box(300, 32), box(40, 33)
    bad = [3, 64, 65, 255, 256, 511, 699]
    a[0, bad[0]], a[1, bad[1]], a[2, bad[2]], a[0, bad[3]] = np.nan, np.inf, -np.inf, np.nan
    a[1, bad[4]], a[2, bad[5]], a[0, bad[6]] = 1e9, -3e5, 2.7e5                     # finite, but beyond +-(2^18 - 2) cells
    b[:, ::2] = np.nan                                                                # cloud 1: nothing valid at all
    b[0, 1::2] = 1e30
    pc = np.concatenate([a, b, c], axis=1)
    prefix = [0, 700, 1000, 1040]
    attr = rng.normal(0, 1, (3, 1040)).astype(np.float32)
    attr[0, 10], attr[1, 20], attr[2, 1010] = np.nan, np.inf, -np.inf                 # valid points with non-finite attributes
    attr[:, bad] = np.nan                                                             # (of invalid points: they reach nobody)
    for mode in ('centroid', 'nearest'):
        want = VO.downsample(pc, attr, 1.0, (0, 0, 0), mode, prefix)
        got = run(pc, attr, prefix, voxel=1.0, mode=mode)
        assert_same(got, want, mode)
        assert got['stats'][0, 1:].tolist() == [693, 4, 3] and got['stats'][1].tolist() == [0, 0, 150, 150]
        assert (got['voxel_of'][bad] == -1).all() and (got['voxel_of'][700:1000] == -1).all()
        assert not np.isin(got['rep'][:got['stats'][0, 0]], bad).any()
        assert not got['out_pc'][:, 700:1000].any() and not got['count'][700:1000].any() and (got['rep'][700:1000] == -1).all()
        assert np.isfinite(got['out_pc']).all()
        if mode == 'centroid':                                # a non-finite attribute reaches its own voxel's mean alone
            where = {ch: set(np.flatnonzero(~np.isfinite(got['out_attr'][ch])).tolist()) for ch in range(3)}
            assert where == {0: {got['voxel_of'][10]}, 1: {got['voxel_of'][20]}, 2: {got['voxel_of'][1010]}}


def test_duplicates_and_ties_go_to_the_smaller_index():
    pc = np.zeros((3, 12), np.float32)
    pc[:, :] = [[0.5], [0.5], [0.5]]
    pc[:, [7, 3]] = [[0.25, 0.75], [0.5, 0.5], [0.5, 0.5]]    # cell 0: two members equidistant from the centroid, 7 and 3
    pc[:, [7, 3]] += np.float32(8.0)                          # (moved to the cell (8, 8, 8))
    pc[:, [1, 4, 9]] = [[-1.5], [2.5], [0.5]]                 # three copies of one point
    pc[:, [0, 2, 5]] = np.array([[20.25, 20.5, 20.75], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]])     # the middle one is the centroid
    for mode in ('centroid', 'nearest'):
        got = run(pc, None, voxel=1.0, mode=mode)
        assert_same(got, VO.downsample(pc, None, 1.0, (0, 0, 0), mode))
        V = got['stats'][0, 0]
        assert V == 4 and got['stats'][0].tolist() == [4, 12, 0, 0]
        # ascending cells: (-2, 2, 0), (0, 0, 0), (8, 8, 8), (20, 0, 0)
        assert got['count'][:4].tolist() == [3, 4, 2, 3] and got['rep'][:4].tolist() == [1, 6, 3, 2]
        assert got['out_pc'][:, 2].tolist() == ([8.75, 8.5, 8.5] if mode == 'nearest' else [8.5, 8.5, 8.5])


# ----------------------------------------------------------------------------- batch invariance
def cloud_bits(o, p0, p1, b):
    shift = lambda x: np.where(x >= 0, x - p0, -1)            # noqa: E731
    return (o['out_pc'][:, p0:p1].tobytes(), o['out_attr'][:, p0:p1].tobytes(), o['count'][p0:p1].tobytes(),
            shift(o['rep'][p0:p1]).tobytes(), shift(o['voxel_of'][p0:p1]).tobytes(), o['stats'][b].tobytes())


def test_a_batch_of_64_clouds_equals_its_clouds():
    """B = 64 (tests/batch64.py), empty clouds at the ends and around 32: the restatement's outputs, and every cloud's outputs
    are the bits of that cloud run alone with prefix = [0, n]."""
    counts = counts64()
    parts = [box(max(n, 1), 100 + i, mean=6.0)[:, :n] for i, n in enumerate(counts)]
    parts[40] = np.concatenate([built_runs(6), box(counts[40], 7)], axis=1)[:, :counts[40]]
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(counts)
    attr = np.random.RandomState(4).normal(0, 1, (2, pc.shape[1])).astype(np.float32)
    for mode in ('centroid', 'nearest'):
        got = run(pc, attr, prefix, voxel=1.0, mode=mode)
        assert_same(got, VO.downsample(pc, attr, 1.0, (0, 0, 0), mode, prefix), mode)
        assert got['count'].max() >= 129
        for b, n in enumerate(counts):
            if n == 0:
                assert got['stats'][b].tolist() == [0, 0, 0, 0]
                continue
            p0, p1 = prefix[b], prefix[b + 1]
            alone = run(pc[:, p0:p1], attr[:, p0:p1], [0, n], voxel=1.0, mode=mode)
            assert cloud_bits(got, p0, p1, b) == cloud_bits(alone, 0, n, 0), (mode, b)


def test_the_same_bits_beside_a_busy_stream(ragged):
    pc, attr, prefix = ragged
    t, a = dev(pc), dev(attr[:3])
    first = run(t, a, prefix, voxel=1.0)
    side = torch.cuda.Stream()
    x = torch.randn(2048, 2048, device='cuda')
    with torch.cuda.stream(side):
        for _ in range(20):
            x = (x @ x).tanh_()
    other = torch.cuda.Stream()
    other.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(other):
        busy = ops.voxel_downsample(t, a, voxel=1.0, prefix=prefix)
    other.synchronize()
    side.synchronize()
    assert_same({k: v.cpu().numpy() for k, v in zip(KEYS, busy)}, first)


# ----------------------------------------------------------------------------- flownet.voxel_downsample
def pair(n, seed, extent=6.0):
    """A corresponding pair: sf a small flow, pc2 = pc1 + sf in float32, so that pc2 - pc1 is sf again bit for bit."""
    p1 = VO.scene(n, seed, extent=extent)
    p2 = p1 + np.random.RandomState(seed).normal(0, 0.05, p1.shape).astype(np.float32)
    return p1, p2, p2 - p1


def eq(t, a):
    return t.dtype == torch.float32 and same_bits(t.cpu().numpy(), np.ascontiguousarray(a))


@pytest.mark.parametrize('form', ['single', 'batch', 'list'])
def test_voxel_downsample_forms(form):
    if form == 'single':
        ps = [pair(700, 31)]
        args = [dev(x) for x in ps[0]]
    elif form == 'batch':
        ps = [pair(600, 32), pair(600, 33)]
        args = [dev(np.stack([p[k] for p in ps])) for k in range(3)]
    else:
        ps = [pair(300, 34), pair(1025, 35), pair(257, 36)]
        args = [[dev(p[k]) for p in ps] for k in range(3)]
    B, voxel = len(ps), 0.5
    for mode in ('centroid', 'nearest'):
        # corr=True: pc1's cells decide, pc2 and sf ride as six channels
        o1, o2, osf, stats, vo, rp = flownet.voxel_downsample(*args, voxel=voxel, mode=mode, corr=True, return_index=True)
        assert stats.shape == (B, 4) and len(o1) == len(o2) == len(osf) == len(vo) == len(rp) == B
        for b, (p1, p2, sf) in enumerate(ps):
            w = VO.downsample_cloud(p1, np.concatenate([p2, sf]), voxel, (0, 0, 0), mode)
            V = w['stats'][0]
            assert 1 < V < p1.shape[1] and stats[b].tolist() == w['stats'].tolist()
            assert eq(o1[b], w['out_pc'][:, :V]) and eq(o2[b], w['out_attr'][:3, :V]) and eq(osf[b], w['out_attr'][3:, :V])
            assert np.array_equal(vo[b].cpu().numpy(), w['voxel_of']) and np.array_equal(rp[b].cpu().numpy(), w['rep'][:V])
            if mode == 'nearest':                             # a pair stays a pair, exactly
                assert eq(o2[b] - o1[b], osf[b].cpu().numpy()) and eq(o1[b], p1[:, w['rep'][:V]])
            # a per-voxel result goes back to every point
            back = o1[b][:, vo[b]]
            assert back.shape == (3, p1.shape[1]) and (vo[b] >= 0).all()
            assert float((back - dev(p1)).abs().max()) <= voxel * 1.0001          # (the same cell: a sanity check, no bar)
        assert flownet.voxel_downsample(args[0], args[1], voxel=voxel, mode=mode)[2] is None
        alone = flownet.voxel_downsample(args[0], voxel=voxel, mode=mode)
        assert alone[1] is None and alone[2] is None and all(torch.equal(x, y) for x, y in zip(alone[0], o1))
        # corr=False: every cloud on its own, as two separate calls; sf with pc1
        o1, o2, osf, stats, vo, rp = flownet.voxel_downsample(*args, voxel=voxel, mode=mode, corr=False, return_index=True)
        s1 = flownet.voxel_downsample(args[0], None, args[2], voxel=voxel, mode=mode, return_index=True)
        s2 = flownet.voxel_downsample(args[1], voxel=voxel, mode=mode, return_index=True)
        assert stats.shape == (2, B, 4) and torch.equal(stats[0], s1[3]) and torch.equal(stats[1], s2[3]) and len(vo) == 2 * B
        for b in range(B):
            assert torch.equal(o1[b], s1[0][b]) and torch.equal(o2[b], s2[0][b]) and torch.equal(osf[b], s1[2][b])
            assert torch.equal(vo[b], s1[4][b]) and torch.equal(vo[B + b], s2[4][b])
            assert torch.equal(rp[b], s1[5][b]) and torch.equal(rp[B + b], s2[5][b])
            w = VO.downsample_cloud(ps[b][1], None, voxel, (0, 0, 0), mode)
            assert eq(o2[b], w['out_pc'][:, :w['stats'][0]])


# ----------------------------------------------------------------------------- the reader and the engine
def test_reader_and_engine_put_frames_on_the_grid(tmp_path):
    from hplflownet_amd import engine
    root = tmp_path / 'KITTI_processed_occ_final'
    frames = {}
    for f, n in enumerate((2600, 1800, 3100)):
        d = root / ('%06d' % f)
        d.mkdir(parents=True)
        p1, p2, _ = pair(n, 50 + f, extent=8.0)
        frames[f] = (str(d), np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T))
        np.save(str(d / 'pc1.npy'), frames[f][1])
        np.save(str(d / 'pc2.npy'), frames[f][2])
    for mode in ('centroid', 'nearest'):
        reader = data.KITTI(None, str(tmp_path), device='cuda', voxel=0.2, voxel_mode=mode)
        for f, (path, a1, a2) in frames.items():
            keep = ~((a1[:, 1] < -1.4) & (a2[:, 1] < -1.4))      # the ground rule first
            w = VO.downsample_cloud(a1[keep].T, a2[keep].T, 0.2, (0, 0, 0), mode)
            V = w['stats'][0]
            o1, o2 = reader.load(path)
            assert 0 < V < keep.sum() < len(a1) and o1.shape == o2.shape == (V, 3)
            assert same_bits(o1, w['out_pc'][:, :V].T) and same_bits(o2, w['out_attr'][:, :V].T)
    s = reader[1]                                             # through __getitem__ (no transform): device tensors (3, V)
    o1, o2 = reader.load(frames[1][0])
    assert torch.equal(s[0], dev(o1.T)) and torch.equal(s[1], dev(o2.T))
    res = engine.main(['--dataset', 'KITTI', '--evaluate', '--voxel', '0.2', '--batch-size', '2', '--ragged', '--data-root',
                       str(tmp_path), '--points', '8192', '--arch', 'HPLFlowNetShallow'])
    assert res and all(np.isfinite(v) for v in res.values()), res


# ----------------------------------------------------------------------------- the workload's size
def test_a_frame_of_100000_points():
    pc = VO.scene(100000, 9)
    attr = np.random.RandomState(9).normal(0, 1, (3, pc.shape[1])).astype(np.float32)
    want = VO.downsample(pc, attr, 0.1)
    assert 50000 < want['stats'][0, 0] < 100000 and want['stats'][0, 1] == 100000
    assert_same(run(pc, attr, voxel=0.1), want)
    want = VO.downsample(pc, attr, 4.0, mode='nearest')
    assert want['count'].max() > 128 and want['stats'][0, 0] < 2000
    assert_same(run(pc, attr, voxel=4.0, mode='nearest'), want)
