"""GPU: hpl_ground_fit / ops.ground_fit, flownet.remove_ground and data.KITTI(remove_ground='plane') against
the numpy restatement tests/ground_oracle.py.  The vote kernel takes S = 1024 points and Hc = 64 hypotheses a workgroup."""
import numpy as np
import pytest
import torch

import ground_oracle as G
from batch64 import counts64
from hplflownet_amd import _lib, data, flownet, ops

pytestmark = pytest.mark.gpu

S, HC = 1024, 64
SIZES = [3, 255, 256, 257, S - 1, S, S + 1, 4099]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(pc, prefix=None, **kw):
    """ops.ground_fit of a host cloud (or a device tensor) -> dict of host arrays."""
    t = pc if torch.is_tensor(pc) else dev(pc)
    out = ops.ground_fit(t, prefix=prefix, return_votes=True, return_height=True, **kw)
    return dict(zip(('plane', 'stats', 'ground', 'keep_idx', 'votes', 'height'), (x.cpu().numpy() for x in out)))


def prefix_of(clouds):
    p = [0]
    for c in clouds:
        p.append(p[-1] + c.shape[1])
    return p


def cloud(n, seed=None, **kw):
    return G.scene(n, n if seed is None else seed, **kw)[0]


def ulps(a, b):
    """The distance of two float32 arrays in units of the last place (both finite, same sign or zero)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32), x.view(np.int32).astype(np.int64))  # noqa: E731
    return np.abs(key(a) - key(b))


def same_classification(pc, prefix, got, cut):
    """height, ground, keep_idx and the kept counts are the restatement's classification of the device's own float32 plane."""
    h, g, k, kept = G.classify_batch(pc, prefix, got['plane'], got['stats'][:, 0], cut)
    assert np.array_equal(got['height'], h, equal_nan=True)
    assert np.array_equal(got['ground'], g) and np.array_equal(got['keep_idx'], k) and np.array_equal(got['stats'][:, 3], kept)


@pytest.fixture(scope='module')
def clouds():
    return [cloud(n) for n in SIZES]


# ----------------------------------------------------------------------------- votes, winner, plane
@pytest.mark.parametrize('hyps', [1, 63, 64, 65, 1024])               # (Hc + 1 = 65)
def test_votes_and_winner_are_exact(clouds, hyps):
    pc, prefix = np.concatenate(clouds, axis=1), prefix_of(clouds)
    got = run(pc, prefix, hyps=hyps, refine=0, seed=11, call=hyps)
    want = G.ground_fit(pc, prefix, hyps=hyps, refine=0, seed=11, call=hyps)
    assert np.array_equal(got['votes'], want['votes'])
    assert np.array_equal(got['stats'][:, :3], want['stats'][:, :3])
    worst = int(ulps(got['plane'], want['plane']).max())
    print('hyps %d: plane at refine = 0 within %d float32 ulp of the restatement' % (hyps, worst))
    assert worst <= 2
    same_classification(pc, prefix, got, 0.3)
    if hyps >= 63:
        assert (want['stats'][1:, 0] == 1).all()              # every scene of 255 points and more is fitted


def test_votes_of_a_large_cloud():
    pc = cloud(100000, 7)
    got = run(pc, hyps=256, refine=0, seed=5)
    want = G.ground_fit(pc, hyps=256, refine=0, seed=5)
    assert np.array_equal(got['votes'], want['votes']) and np.array_equal(got['stats'][:, :3], want['stats'][:, :3])
    assert int(ulps(got['plane'], want['plane']).max()) <= 2
    same_classification(pc, [0, pc.shape[1]], got, 0.3)


def test_the_scan_past_its_first_chunk():
    """Clouds that own 1, 0, 255, 257 and 256 workgroups of S points in one batch.  The per-cloud scan (k_ground_scan,
    DESIGN.md §35) takes a cloud's workgroups 256 at a time: the fourth cloud's last workgroup gets its offset from the carry of
    the first chunk, and no cloud but the first starts at workgroup 0.  That cloud holds 501 non-finite points (kept, height
    NaN), its lone last point among them; about half of every large cloud is ground, so the -1 fill behind the kept count
    spans many workgroups."""
    sizes = [1, 0, 255 * S, 256 * S + 1, 256 * S]
    assert [-(-n // S) for n in sizes] == [1, 0, 255, 257, 256]
    parts = [cloud(max(n, 300), 200 + i)[:, :n] for i, n in enumerate(sizes)]
    rng = np.random.RandomState(8)
    bad = np.append(rng.choice(256 * S, 500, replace=False), 256 * S)
    parts[3][rng.randint(0, 3, bad.size), bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.randint(0, 3, bad.size)]
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(parts)
    got = run(pc, prefix, hyps=64, refine=0, seed=13)
    assert got['stats'][:, 0].tolist() == [0, 0, 1, 1, 1]
    same_classification(pc, prefix, got, 0.3)
    kept = got['stats'][:, 3].tolist()
    assert kept[:2] == [1, 0] and all(0.3 * n < k < 0.7 * n for n, k in zip(sizes[2:], kept[2:]))
    assert np.isnan(got['height'][prefix[3] + bad]).all() and np.isin(prefix[3] + bad, got['keep_idx']).all()
    assert got['keep_idx'][prefix[3] + kept[3] - 1] == prefix[3] + 256 * S       # the last workgroup's one point, kept last


def test_invalid_hypotheses_count_minus_one():
    """A draw of a non-finite point, collinear (here: repeated) draws and a failed gate each give votes -1."""
    rng = np.random.RandomState(3)
    pc = G.scene(400, 3, ground=0.4, wall=0.3)[0]
    pc[:, 0:60] = pc[:, 60:61]                                # 60 copies of one point: q = 0 when two draws meet there
    bad = rng.permutation(np.arange(61, 400))[:60]
    pc[rng.randint(0, 3, 60), bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.randint(0, 3, 60)]
    kw = dict(hyps=512, seed=2, max_tilt_deg=20.0)
    a, m, q, valid = G.hypotheses(pc, (0, 1, 0), G.min_cos_of(20.0), 512, 0.1, 2, 0)
    i = G.draws(400, 512, 2, 0)
    nonfinite = ~np.isfinite(pc).all(0)[i].all(1)
    with np.errstate(all='ignore'):
        assert nonfinite.any() and (q == 0).any() and (~valid & ~nonfinite & (q > 0)).any() and valid.any()     # each kind occurs
    got, want = run(pc, refine=0, **kw), G.ground_fit(pc, refine=0, **kw)
    assert np.array_equal(got['votes'], want['votes']) and np.array_equal(got['votes'][0] == -1, ~valid)
    assert np.array_equal(got['stats'][:, :3], want['stats'][:, :3])
    for cut in (0.0, 0.3):                                    # invalid points are kept, their height NaN
        got = run(pc, refine=2, cut=cut, **kw)
        same_classification(pc, [0, 400], got, cut)
        inv = ~np.isfinite(pc).all(0)
        assert np.isnan(got['height'][inv]).all() and not got['ground'][inv].any() and np.isin(np.flatnonzero(inv), got['keep_idx']).all()
        assert got['ground'].any() and not np.isnan(got['height'][~inv]).any()


def test_degenerate_clouds():
    """Clouds of 0, 1 and 2 points and an all-collinear cloud have status 0 and the identity keep_idx, beside a fitted one."""
    line = np.stack([np.arange(300.0), 2 * np.arange(300.0), -np.arange(300.0)]).astype(np.float32)
    full = cloud(257)
    parts = [full[:, :0], full[:, :1], line, full[:, :2], full, np.full((3, 5), np.nan, np.float32)]
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(parts)
    got = run(pc, prefix, hyps=65, refine=1)
    want = G.ground_fit(pc, prefix, hyps=65, refine=1)
    assert got['stats'].tolist() == want['stats'].tolist()
    assert got['stats'][:, 0].tolist() == [0, 0, 0, 0, 1, 0] and got['stats'][[0, 1, 2, 3, 5]].tolist() == \
        [[0, -1, 0, 0], [0, -1, 0, 1], [0, -1, 0, 300], [0, -1, 0, 2], [0, -1, 0, 5]]
    assert np.array_equal(got['votes'], want['votes']) and (got['votes'][[0, 1, 2, 3, 5]] == -1).all()
    same_classification(pc, prefix, got, 0.3)
    for b in (1, 2, 3, 5):
        sl = slice(prefix[b], prefix[b + 1])
        assert not got['plane'][b].any() and not got['ground'][sl].any() and not got['height'][sl].any()
        assert got['keep_idx'][sl].tolist() == list(range(prefix[b], prefix[b + 1]))
    # an empty batch launches nothing
    e = run(pc[:, :0], [0, 0, 0], hyps=7)
    assert e['stats'].tolist() == [[0, -1, 0, 0]] * 2 and not e['plane'].any() and (e['votes'] == -1).all() and e['keep_idx'].size == 0


def test_ties_go_to_the_smallest_hypothesis():
    """Points exactly on an integer grid in the plane y = -2 (every product and sum of the test is exact, so s = 0 for each of
    them whatever three of them span the hypothesis) and a few points off it: the grid's hypotheses tie."""
    gx, gz = np.meshgrid(np.arange(-8, 8), np.arange(3, 19))
    grid = np.stack([gx.ravel(), np.full(gx.size, -2), gz.ravel()]).astype(np.float32)
    off = np.array([[0.5, 1.25, 7.0], [-3.0, 2.5, 11.0], [4.0, 0.75, 5.5]], np.float32).T
    pc = np.concatenate([grid, off], axis=1)[:, np.random.RandomState(0).permutation(grid.shape[1] + 3)]
    got, want = run(pc, hyps=256, refine=0, tau=0.05), G.ground_fit(pc, hyps=256, refine=0, tau=0.05)
    v = want['votes'][0]
    assert (v == grid.shape[1]).sum() > 10 and v.max() == grid.shape[1]
    assert np.array_equal(got['votes'], want['votes'])
    assert got['stats'][0, :3].tolist() == [1, int(np.flatnonzero(v == v.max())[0]), grid.shape[1]]
    assert got['plane'][0].tolist() == [0.0, 1.0, 0.0, 2.0]
    same_classification(pc, [0, pc.shape[1]], run(pc, hyps=256, refine=0, tau=0.05, cut=0.0), 0.0)


# ----------------------------------------------------------------------------- refinement
REFINE_SCENES = [dict(n=1000, seed=1), dict(n=4099, seed=2), dict(n=4099, seed=3, ground=0.3, wall=0.4), dict(n=257, seed=4, up='z')]


@pytest.mark.parametrize('refine', [1, 2, 8])
def test_refinement_against_the_restatement(refine):
    """Each normal component within 2^-22 of the restatement's, d within 2^-22 max(1, |d|): two float32 roundings of float64
    values that agree to about 1e-13 (tests/test_ground_cpu.py) differ by at most one ulp, 2^-23 below 1; the bar doubles it."""
    parts = [G.scene(**kw)[0] for kw in REFINE_SCENES[:3]]
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(parts)
    kw = dict(hyps=512, refine=refine, seed=9)
    got, want = run(pc, prefix, **kw), G.ground_fit(pc, prefix, **kw)
    zup = G.scene(**REFINE_SCENES[3])[0]
    gz, wz = run(zup, up=(0, 0, 1), **kw), G.ground_fit(zup, up=(0, 0, 1), **kw)
    assert want['rounds'] == [refine] * 3 and wz['rounds'] == [refine]
    worst_n = worst_d = 0.0
    for g, w in ((got, want), (gz, wz)):
        assert np.array_equal(g['stats'][:, :3], w['stats'][:, :3])
        dn = np.abs(g['plane'][:, :3].astype(np.float64) - w['plane64'][:, :3]).max()
        dd = (np.abs(g['plane'][:, 3].astype(np.float64) - w['plane64'][:, 3]) / np.maximum(1.0, np.abs(w['plane64'][:, 3]))).max()
        worst_n, worst_d = max(worst_n, dn), max(worst_d, dd)
    print('refine %d: largest |n - restatement| %.3g, largest |d - restatement| / max(1, |d|) %.3g (2^-22 = %.3g; the float32 '
          'rounding of the restatement itself is up to 2^-24 = %.3g of that)' % (refine, worst_n, worst_d, 2.0 ** -22, 2.0 ** -24))
    assert worst_n <= 2.0 ** -22 and worst_d <= 2.0 ** -22
    same_classification(pc, prefix, got, 0.3)
    same_classification(zup, [0, zup.shape[1]], gz, 0.3)


def test_a_round_without_inliers_keeps_the_ransac_plane():
    """tau = 1e-30: the winner's first point has height exactly 0 (d is minus the same sum), nothing else is within tau."""
    pc = cloud(1000, 5)
    kw = dict(hyps=64, tau=1e-30, seed=4)
    assert G.fit(pc, refine=2, **kw)['rounds'] == 0 and G.fit(pc, refine=2, **kw)['status'] == 1
    first, kept = run(pc, refine=0, **kw), run(pc, refine=2, **kw)
    assert first['stats'][0, 0] == 1 and np.array_equal(first['plane'].view(np.int32), kept['plane'].view(np.int32))
    assert np.array_equal(first['stats'], kept['stats']) and np.array_equal(first['height'], kept['height'])


def test_a_round_outside_the_gate_keeps_the_ransac_plane():
    """A ground at 20.1 degrees under a 20 degree gate: hypotheses that lean inside the gate win, the least-squares plane of
    their inliers is the true one, outside it."""
    pc = G.scene(4099, 6, tilt_deg=20.1)[0]
    kw = dict(hyps=512, seed=6, max_tilt_deg=20.0)
    o = G.fit(pc, refine=2, **kw)
    assert o['status'] == 1 and o['rounds'] == 0
    assert G.fit(pc, refine=2, hyps=512, seed=6, max_tilt_deg=25.0)['rounds'] == 2       # (the gate is what stops it)
    first, kept = run(pc, refine=0, **kw), run(pc, refine=2, **kw)
    assert first['stats'][0, 0] == 1 and np.array_equal(first['plane'].view(np.int32), kept['plane'].view(np.int32))
    assert np.array_equal(first['stats'], kept['stats'])


# ----------------------------------------------------------------------------- batch invariance
def bits(o, p0, p1, b):
    return (o['plane'][b].tobytes(), o['stats'][b].tobytes(), o['votes'][b].tobytes(), o['height'][p0:p1].tobytes(),
            o['ground'][p0:p1].tobytes(), np.where(o['keep_idx'][p0:p1] >= 0, o['keep_idx'][p0:p1] - p0, -1).tobytes())


def test_a_cloud_has_the_same_bits_anywhere():
    parts = [cloud(1025, 21), cloud(300, 22)[:, :0], cloud(2051, 23, ground=0.3, wall=0.4), cloud(300, 24)[:, :2], cloud(255, 25)]
    kw = dict(hyps=65, refine=2, seed=3, call=12)
    alone = [bits(run(p, **kw), 0, p.shape[1], 0) for p in parts]
    for order in ([0, 1, 2, 3, 4], [4, 2, 3, 0, 1]):
        sel = [parts[i] for i in order]
        prefix = prefix_of(sel)
        wide = torch.full((3, prefix[-1] + 37), float('nan'), device='cuda')
        wide[:, 5:5 + prefix[-1]] = dev(np.concatenate(sel, axis=1))
        view = wide[:, 5:5 + prefix[-1]]                     # pc_ld > N, and every cloud starts at an odd element
        assert view.stride(0) == prefix[-1] + 37
        first = run(view, prefix, **kw)
        for j, i in enumerate(order):
            assert bits(first, prefix[j], prefix[j + 1], j) == alone[i], (order, i)
        again = run(view, prefix, **kw)
        assert all(np.array_equal(first[k], again[k], equal_nan=True) for k in first)
        side = torch.cuda.Stream()
        a = torch.randn(2048, 2048, device='cuda')
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a).tanh_()
        busy = run(view, prefix, **kw)
        side.synchronize()
        assert all(np.array_equal(first[k], busy[k], equal_nan=True) for k in first)


def test_a_batch_of_64_clouds_equals_its_clouds():
    """B = 64 (tests/batch64.py): every cloud's outputs are the bits of that cloud run alone with prefix = [0, n]; votes and
    winners are the restatement's, the refined planes of the clouds of 300 points and more lie within the bar of
    test_refinement_against_the_restatement, and a cloud of fewer than 3 points has status 0 in both runs."""
    counts = counts64()
    parts = [cloud(max(n, 300), 100 + i)[:, :n] for i, n in enumerate(counts)]
    pc, prefix = np.concatenate(parts, axis=1), prefix_of(parts)
    kw = dict(hyps=65, refine=2, seed=3, call=12)
    got, want = run(pc, prefix, **kw), G.ground_fit(pc, prefix, **kw)
    assert np.array_equal(got['votes'], want['votes']) and np.array_equal(got['stats'][:, :3], want['stats'][:, :3])
    same_classification(pc, prefix, got, 0.3)
    for b, n in enumerate(counts):
        alone = run(parts[b], [0, n], **kw)
        assert bits(got, prefix[b], prefix[b + 1], b) == bits(alone, 0, n, 0), b
        if n < 3:
            assert got['stats'][b].tolist() == alone['stats'][0].tolist() == [0, -1, 0, n]
        if n >= 300:
            assert want['rounds'][b] == 2 and got['stats'][b, 0] == 1
            w = want['plane64'][b]
            assert np.abs(got['plane'][b, :3].astype(np.float64) - w[:3]).max() <= 2.0 ** -22, b
            assert abs(float(got['plane'][b, 3]) - w[3]) / max(1.0, abs(w[3])) <= 2.0 ** -22, b


# ----------------------------------------------------------------------------- remove_ground, reader
def pair(n, seed, **kw):
    """A corresponding pair: pc2 = pc1 + a small flow; -> pc1, pc2, sf (3, n) float32."""
    p1 = cloud(n, seed, **kw)
    sf = np.random.RandomState(seed).normal(0, 0.05, p1.shape).astype(np.float32)
    return p1, p1 + sf, sf


def want_pair(p1s, p2s, **kw):
    both = list(p1s) + list(p2s)
    o = G.ground_fit(np.concatenate(both, axis=1), prefix_of(both), **kw)
    return o, prefix_of(both)


def eq(t, a):
    return t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize('form', ['single', 'batch', 'list'])
def test_remove_ground_forms(form):
    kw = dict(hyps=128, seed=1, call=3)
    if form == 'single':
        ps = [pair(700, 31)]
        args = [dev(x) for x in ps[0]]
    elif form == 'batch':
        ps = [pair(600, 32), pair(600, 33)]
        args = [dev(np.stack([p[k] for p in ps])) for k in range(3)]
    else:
        ps = [pair(300, 34), pair(1025, 35), pair(257, 36)]
        args = [[dev(p[k]) for p in ps] for k in range(3)]
    B = len(ps)
    want, prefix = want_pair([p[0] for p in ps], [p[1] for p in ps], **kw)
    g = want['ground'].astype(bool)
    # corr=True: the pair rule
    o1, o2, osf, planes, stats, masks = flownet.remove_ground(*args, corr=True, return_mask=True, **kw)
    assert planes.shape == (2, B, 4) and stats.shape == (2, B, 4) and np.array_equal(stats.cpu().numpy().reshape(-1, 4), want['stats'])
    for b, (p1, p2, sf) in enumerate(ps):
        keep = ~(g[prefix[b]:prefix[b + 1]] & g[prefix[B + b]:prefix[B + b + 1]])
        assert 0 < keep.sum() < keep.size and np.array_equal(masks[b], keep)
        assert eq(o1[b], p1[:, keep]) and eq(o2[b], p2[:, keep]) and eq(osf[b], sf[:, keep])
    assert flownet.remove_ground(args[0], args[1], **kw)[2] is None
    # corr=False: every cloud on its own, sf with pc1
    o1, o2, osf, planes, stats = flownet.remove_ground(*args, corr=False, **kw)
    for b, (p1, p2, sf) in enumerate(ps):
        k1, k2 = ~g[prefix[b]:prefix[b + 1]], ~g[prefix[B + b]:prefix[B + b + 1]]
        assert eq(o1[b], p1[:, k1]) and eq(o2[b], p2[:, k2]) and eq(osf[b], sf[:, k1])


def test_remove_ground_with_z_up_and_unequal_clouds():
    p1, p2 = cloud(900, 41, up='z', height=2.0), cloud(1100, 42, up='z', height=2.0)
    kw = dict(up=(0, 0, 1), hyps=128, cut=0.2)
    want, prefix = want_pair([p1], [p2], **kw)
    o1, o2, osf, planes, stats = flownet.remove_ground(dev(p1), dev(p2), corr=False, **kw)
    g = want['ground'].astype(bool)
    assert eq(o1[0], p1[:, ~g[:900]]) and eq(o2[0], p2[:, ~g[900:]]) and osf is None
    assert np.array_equal(stats.cpu().numpy().reshape(-1, 4), want['stats']) and (want['stats'][:, 0] == 1).all()
    assert (planes.cpu().numpy()[:, 0, 2] > 0.99).all()      # the normals point along z
    assert 0.3 * 900 < g[:900].sum() < 0.7 * 900
    with pytest.raises(_lib.HplError):
        flownet.remove_ground(dev(p1), dev(p2), corr=True, **kw)


def test_reader_removes_the_ground_by_fitted_planes(tmp_path):
    root = tmp_path / 'KITTI_processed_occ_final'
    frames = {}
    for f in (0, 1, 2):
        d = root / ('%06d' % f)
        d.mkdir(parents=True)
        p1, p2, _ = pair(600 + 7 * f, 50 + f, height=1.7, tilt_deg=3.0 * f)
        frames[f] = (str(d), np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T))
        np.save(str(d / 'pc1.npy'), frames[f][1])
        np.save(str(d / 'pc2.npy'), frames[f][2])
    ground = dict(hyps=128, tau=0.1, cut=0.25)
    reader = data.KITTI(None, str(tmp_path), remove_ground='plane', device='cuda', ground=ground)
    got = {}
    for f in (2, 0, 1, 0, 2):                                 # any order, any repetition: call is the frame number
        path, a1, a2 = frames[f]
        want, prefix = want_pair([a1.T], [a2.T], seed=0, call=f, **ground)
        g = want['ground'].astype(bool)
        keep = ~(g[:len(a1)] & g[len(a1):])
        o1, o2 = reader.load(path)
        assert 0 < keep.sum() < keep.size and np.array_equal(o1, a1[keep]) and np.array_equal(o2, a2[keep])
        assert f not in got or (np.array_equal(got[f][0], o1) and np.array_equal(got[f][1], o2))
        got[f] = (o1, o2)
    s = reader[1]                                             # through __getitem__ (no transform): device tensors (3, K)
    assert torch.equal(s[0], dev(got[1][0].T)) and torch.equal(s[1], dev(got[1][1].T))
    # the reference's rule is untouched
    plain = data.KITTI(None, str(tmp_path), remove_ground=True, device='cuda')
    for f, (path, a1, a2) in frames.items():
        keep = ~((a1[:, 1] < -1.4) & (a2[:, 1] < -1.4))
        o1, o2 = plain.load(path)
        assert np.array_equal(o1, a1[keep]) and np.array_equal(o2, a2[keep])
