"""GPU: hpl_outlier_filter / ops.outlier_filter, flownet.remove_outliers, data.KITTI(outlier=...) and engine --outlier (DESIGN.md
§33) against the numpy restatement tests/outlier_oracle.py.  Per point -- count, the bits of nbr_d2, the bits of mean_dist --
the device EQUALS the restatement (the float64 root and quotient are correctly rounded on both sides).  mu, sigma and T are held
to 2^-22 relative: one float32 rounding (2^-24) and two fixed-order float64 sums of at most a few thousand terms against
numpy's (far below 2^-40), where sigma > 1e-3 mu; a smaller sigma is held to 2^-22 mu absolute (a shift of mu by its own
rounding moves sigma by no more than that shift).  keep, keep_idx and stats EQUAL the classification the restatement makes
from the DEVICE's mean_dist and thresh.  A cloud has the same bits alone, anywhere in a batch, through strided views, twice
and beside a busy stream."""
import ctypes

import numpy as np
import pytest
import torch

import outlier_oracle as O
from batch64 import counts64, prefix_of
from normals_oracle import scene as surface_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAR = 2.0 ** -22
F = np.float32
KEYS = ('keep', 'keep_idx', 'mean_dist', 'count', 'thresh', 'stats', 'nbr_d2')


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(pc, mode='statistical', prefix=None, **kw):
    """-> dict of host arrays (mean_dist and nbr_d2 None in radius mode)."""
    from hplflownet_amd import ops
    got = ops.outlier_filter(pc if torch.is_tensor(pc) else dev(pc), mode=mode, prefix=prefix, return_neighbors=mode == 'statistical',
                             **kw)
    torch.cuda.synchronize()
    return {key: (None if v is None else v.cpu().numpy()) for key, v in zip(KEYS, got + (None,))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same(a, b, p0=0):
    """Two results bit for bit; b's packed indices shifted by p0."""
    for key in KEYS:
        x, y = a[key], b[key]
        if x is None or y is None:
            assert x is None and y is None, key
        elif key == 'keep_idx':
            assert np.array_equal(x, np.where(y >= 0, y + p0, y)), key
        elif x.dtype == np.float32:
            assert np.array_equal(bits(x), bits(y)), key
        else:
            assert np.array_equal(x, y), key


# ----------------------------------------------------------------------------- the clouds
def doctored(n, kind):
    """'scene': the surface scene with, as far as n allows, duplicates, a point exactly at the radius 1 of another and one a
    float past it, isolated points, points on cell borders (multiples of the cell edge 1.001), NaN / inf points and points at
    1e7 m.  'lattice': a 0.25 m lattice, most d2 tied.  'one_cell': every point inside one cell."""
    rng = np.random.RandomState(n)
    if kind == 'lattice':
        return (rng.randint(-4, 5, (3, n)) * 0.25).astype(F)
    if kind == 'one_cell':
        return rng.uniform(0.05, 0.95, (3, n)).astype(F)
    if n < 255:
        return rng.uniform(-0.4, 0.4, (3, n)).astype(F)
    pc = surface_scene(n, n)
    pc[:, 3] = pc[:, 1]
    pc[:, 10] = pc[:, 1]                                       # three indices in one place
    pc[:, 5], pc[:, 6], pc[:, 7] = (np.nan, 1, 5), (1, 1, np.inf), (1, -np.inf, 5)
    pc[:, 8], pc[:, 9] = 1e7, (1e7, 0, 5)
    pc[:, 20] = (100, 0, 0)
    pc[:, 21] = (101, 0, 0)                                    # d2 = 1 = radius^2: a neighbour of point 20
    pc[:, 22] = (np.nextafter(F(99), F(-np.inf)), 0, 0)        # a float past it: none
    pc[:, 23] = (-200, 50, 50)                                 # alone
    edge = F(1.001)
    for t in range(12):                                        # on the borders of the cells, in one, two and three coordinates
        pc[:, 30 + t] = np.array([F(edge * F(t % 4 - 1)), F(-1.5) if t % 3 else F(edge * F(-2)), F(5) if t % 2 else F(edge * F(5))], F)
    pc[:, 42] = (0.0, -1.5, 5.0)
    pc[:, 43] = (-0.0, -1.5, 5.0)
    return pc


_NEIGH = {}


def oracle_neighbourhoods(n, kind):
    """The restatement's search at k = 32, once per cloud: a shorter list is its head."""
    if (n, kind) not in _NEIGH:
        pc = doctored(n, kind)
        _NEIGH[(n, kind)] = (pc, O.in_range(pc, 1.0)) + O.neighbourhoods(pc, 32, 1.0)
    return _NEIGH[(n, kind)]


def check_statistical(got, pc, part, total, nd2, k, radius, std_ratio, prefix=None):
    """Everything the statistical mode returns against the restatement (total, nd2: its search, nd2 at least k wide)."""
    prefix = [0, pc.shape[1]] if prefix is None else prefix
    mean, count = O.mean_distance(nd2[:, :k], total, k, radius, part)
    assert np.array_equal(got['count'], count)
    assert np.array_equal(bits(got['nbr_d2']), bits(np.where(np.arange(k)[None, :] < count[:, None], nd2[:, :k], F(np.inf))))
    assert np.array_equal(bits(got['mean_dist']), bits(mean))
    want = O.thresholds(mean, part, prefix, std_ratio)
    assert got['thresh'].dtype == np.float32 and (got['thresh'][:, 3] == 0).all()
    for b in range(len(prefix) - 1):
        mu, sigma, T = want[b]
        g = got['thresh'][b].astype(np.float64)
        print('cloud %d: mu %.9g (device %.9g), sigma %.9g (%.9g), T %.9g (%.9g)' % (b, mu, g[0], sigma, g[1], T, g[2]))
        assert abs(g[0] - mu) <= BAR * mu
        if sigma > 1e-3 * mu:
            assert abs(g[1] - sigma) <= BAR * sigma and abs(g[2] - T) <= BAR * T
        else:
            assert abs(g[1] - sigma) <= BAR * mu and abs(g[2] - T) <= BAR * T + BAR * mu
            assert sigma != 0 or g[1] == 0
    keep, keep_idx, stats = O.classify(part, prefix, 'statistical', mean_dist=got['mean_dist'], thresh=got['thresh'])
    assert np.array_equal(got['keep'], keep) and np.array_equal(got['keep_idx'], keep_idx) and np.array_equal(got['stats'], stats)


def check_radius(got, part, total, min_neighbors, prefix=None):
    prefix = [0, len(part)] if prefix is None else prefix
    count = np.where(part, total, 0).astype(np.int32)
    keep, keep_idx, stats = O.classify(part, prefix, 'radius', count=count, min_neighbors=min_neighbors)
    assert got['mean_dist'] is None and not got['thresh'].any()
    assert np.array_equal(got['count'], count) and np.array_equal(got['keep'], keep)
    assert np.array_equal(got['keep_idx'], keep_idx) and np.array_equal(got['stats'], stats)


CLOUDS = [(1, 'scene'), (2, 'scene'), (3, 'scene'), (255, 'scene'), (257, 'scene'), (257, 'lattice'), (1025, 'scene'),
          (1025, 'one_cell'), (3000, 'scene')]
IDS = ['%d-%s' % c for c in CLOUDS]


# ----------------------------------------------------------------------------- 1. the statistical mode
@pytest.mark.parametrize('k', [1, 8, 9, 16, 17, 32])
@pytest.mark.parametrize('n,kind', CLOUDS, ids=IDS)
def test_statistical_equals_the_restatement(n, kind, k):
    pc, part, total, nd2 = oracle_neighbourhoods(n, kind)
    got = run(pc, k=k, radius=1.0, std_ratio=1.5)
    check_statistical(got, pc, part, total, nd2, k, 1.0, 1.5)
    if kind == 'scene' and n >= 255:                          # the doctored points did what they are there for
        c, m = got['count'], got['mean_dist']
        assert (c[[5, 6, 7, 8, 9]] == 0).all() and np.isinf(m[[5, 6, 7, 8, 9]]).all() and not got['keep'][[5, 6, 7, 8, 9]].any()
        assert c[20] == 1 and c[21] == 1 and c[22] == 0 and c[23] == 0 and m[22] == 1 and m[23] == 1 and m[20] == 1
        assert got['nbr_d2'][1, 0] == 0 and (k < 2 or got['nbr_d2'][1, 1] == 0) and got['stats'][0, 3] == 5
    if kind == 'one_cell' and k == 32:
        assert (got['count'] == 32).all()
    if n == 1:
        assert got['mean_dist'][0] == 1 and got['keep'][0] == 1 and list(got['thresh'][0]) == [1, 0, 1, 0]


def test_far_points_take_part_when_the_cells_are_large():
    """At 1e7 m a float32 step is 1 m: out of range at radius 1, with radius 64 the points are neighbours like any others."""
    rng = np.random.RandomState(5)
    pc = (1e7 + rng.randint(-100, 101, (3, 200))).astype(F)
    pc[:, 0] = 3e7                                            # past the cells' range even so
    got = run(pc, k=8, radius=1.0)
    assert not got['keep'].any() and list(got['stats'][0]) == [0, 0, 0, 200] and not got['thresh'].any()
    assert (got['keep_idx'] == -1).all() and np.isinf(got['mean_dist']).all() and not got['count'].any()
    part = O.in_range(pc, 64.0)
    total, nd2 = O.neighbourhoods(pc, 8, 64.0)
    assert not part[0] and part[1:].all() and total[1:].min() >= 1
    check_statistical(run(pc, k=8, radius=64.0, std_ratio=1.0), pc, part, total, nd2, 8, 64.0, 1.0)
    check_radius(run(pc, 'radius', radius=64.0, min_neighbors=5), part, total, 5)


def test_the_last_cells_of_the_key_and_the_ones_past_them():
    """tests/grid_edge.py: clusters in the cells +-(2^18 - 2) of each axis find each other and nothing else; the clusters one cell
    further out, within the radius of them, take no part."""
    import grid_edge as E
    pc, inside, cluster = E.cloud()
    E.check_cells(pc, inside, cluster)
    part = O.in_range(pc, 1.0)
    total, nd2 = O.neighbourhoods(pc, 8, 1.0)
    assert np.array_equal(part, inside) and (total[inside] == 3).all() and (total[~inside] == 0).all()
    got = run(pc, k=8, radius=1.0)
    check_statistical(got, pc, part, total, nd2, 8, 1.0, 2.0)
    assert not got['keep'][~inside].any() and list(got['stats'][0][[0, 3]]) == [24, 24]
    check_radius(run(pc, 'radius', radius=1.0, min_neighbors=3), part, total, 3)


def test_the_cube_has_no_spread():
    pc = np.array([[i, j, l] for i in (0, 1) for j in (0, 1) for l in (0, 1)], F).T
    got = run(pc, k=3, radius=1.5, std_ratio=0.0)
    assert (got['mean_dist'] == 1).all() and list(got['thresh'][0]) == [1, 0, 1, 0]          # sigma exactly 0
    assert got['keep'].all() and list(got['keep_idx']) == list(range(8)) and list(got['stats'][0]) == [8, 8, 0, 0]
    pair = run(np.array([[0, 0.1], [0, 0], [0, 0]], F), k=4, radius=2.0)
    assert (pair['mean_dist'] == F((np.sqrt(np.float64(F(0.1) * F(0.1))) + 6.0) / 4)).all()   # a stray pair does not look dense


def test_more_partials_than_one_run_of_the_fold():
    """20 000 points: 20 workgroups of 1024 in the cloud, more than the 16 strided runs of the fold."""
    pc, stray = O.scene(20000, 400, 4)
    part = O.in_range(pc, 1.0)
    total, nd2 = O.neighbourhoods(pc, 8, 1.0, chunk=512)
    got = run(pc, k=8, radius=1.0, std_ratio=2.0)
    check_statistical(got, pc, part, total, nd2, 8, 1.0, 2.0)
    assert not got['keep'][stray].any()


# ----------------------------------------------------------------------------- 2. the radius mode
@pytest.mark.parametrize('min_neighbors', [1, 2, 5, 'N'])
@pytest.mark.parametrize('n,kind', CLOUDS, ids=IDS)
def test_radius_equals_the_restatement(n, kind, min_neighbors):
    pc, part, total, _ = oracle_neighbourhoods(n, kind)
    m = n if min_neighbors == 'N' else min_neighbors
    check_radius(run(pc, 'radius', radius=1.0, min_neighbors=m), part, total, m)
    if kind == 'one_cell':
        assert total.max() > 32                               # not capped


def test_radius_mode_at_other_radii():
    pc, _, _, _ = oracle_neighbourhoods(1025, 'scene')
    for radius, m in ((0.25, 1), (2.5, 40)):
        part = O.in_range(pc, radius)
        total, _ = O.neighbourhoods(pc, 1, radius)
        got = run(pc, 'radius', radius=radius, min_neighbors=m)
        check_radius(got, part, total, m)
        assert 0 < got['stats'][0, 1] < got['stats'][0, 0]


def test_the_scan_past_its_first_chunk():
    """Clouds that own 1, 0, 255, 257 and 256 workgroups of 1024 points in one batch, radius mode.  The per-cloud scan
    (k_outlier_scan) takes a cloud's workgroups 256 at a time: the fourth cloud's last workgroup gets its
    offset from the carry of the first chunk, and no cloud but the first starts at workgroup 0.  The points are uniform in a
    cube of 64 m, at most one per cubic metre -- one per cell of 1.001 m, 4.2 neighbours within the radius of 1 m on average,
    so that min_neighbors = 4 keeps about half --, with 1000 NaN points in the fourth cloud, whose participating count then
    differs from its size and from its kept count, and its last five points in one place: the lone point of its last workgroup
    is kept.  The all-pairs restatement is too slow here: keep_idx and stats are held to the returned mask, the mask itself to
    the restatement in the clouds of up to 1024 points, for which a sixth cloud of 300 points, denser, with 5 NaN, is added."""
    sizes = [1, 0, 255 * 1024, 256 * 1024 + 1, 256 * 1024]
    assert [-(-n // 1024) for n in sizes] == [1, 0, 255, 257, 256]
    rng = np.random.RandomState(12)
    clouds = [rng.uniform(0, 64, (3, n)).astype(F) for n in sizes]
    clouds[3][:, -5:] = np.array([[32.5], [32.5], [32.5]], F)
    nans = rng.choice(sizes[3] - 5, 1000, replace=False)
    clouds[3][rng.randint(0, 3, 1000), nans] = np.nan
    sizes.append(300)                                         # behind them, for the restatement: a 6 m cube, 5.8 neighbours on average
    clouds.append(rng.uniform(0, 6, (3, 300)).astype(F))
    clouds[5][:, :5] = np.nan
    pc, pre = np.concatenate(clouds, 1), prefix_of(sizes)
    got = run(pc, 'radius', prefix=pre, radius=1.0, min_neighbors=4)
    finite = ~np.isnan(pc).any(0)
    for b, (p0, p1) in enumerate(zip(pre, pre[1:])):
        mask = got['keep'][p0:p1].astype(bool)
        idx, part = p0 + np.flatnonzero(mask), int(finite[p0:p1].sum())
        assert np.array_equal(got['keep_idx'][p0:p0 + len(idx)], idx) and (got['keep_idx'][p0 + len(idx):p1] == -1).all(), b
        assert got['stats'][b].tolist() == [part, len(idx), part - len(idx), p1 - p0 - part], b
        assert not mask[~finite[p0:p1]].any()
        if p1 - p0 <= 1024:
            assert np.array_equal(mask, O.outlier_filter(clouds[b], 'radius', radius=1.0, min_neighbors=4)['keep'].astype(bool))
        else:
            assert 0.3 * (p1 - p0) < len(idx) < 0.8 * (p1 - p0)
    assert 50 < got['stats'][5, 1] < 250 and got['stats'][5, 3] == 5
    assert got['stats'][3, 3] == 1000 and got['keep'][pre[4] - 1] == 1 and got['keep_idx'][pre[3] + got['stats'][3, 1] - 1] == pre[4] - 1


# ----------------------------------------------------------------------------- 3. what the filter is for
@pytest.mark.parametrize('n,n_out,k,radius', [(300, 10, 8, 4.0), (1025, 25, 16, 2.0), (3000, 60, 16, 2.0), (3000, 60, 32, 2.0),
                                              (3000, 60, 8, 1.0)])
def test_scene_strays_are_removed_and_the_surface_stays(n, n_out, k, radius):
    pc, stray = O.scene(n, n_out, 1)
    got = run(pc, k=k, radius=radius, std_ratio=2.0)
    kept = got['keep'].astype(bool)
    print('n = %d, %d strays, k = %d, radius %g: strays removed %.1f %%, surface kept %.1f %%' % (
        n, n_out, k, radius, 100 * (~kept[stray]).mean(), 100 * kept[~stray].mean()))
    assert not kept[stray].any()
    assert kept[~stray].mean() >= 0.95
    assert got['stats'][0, 1] == kept.sum() and np.array_equal(got['keep_idx'][:kept.sum()], np.nonzero(kept)[0])


# ----------------------------------------------------------------------------- 4. bits
def cloud_of(n, seed):
    return O.scene(n, n // 50, 100 + seed)[0] if n >= 8 else np.random.RandomState(seed).uniform(-0.3, 0.3, (3, n)).astype(F)


MODES = [('statistical', dict(k=9, radius=1.5, std_ratio=1.0)), ('radius', dict(radius=1.0, min_neighbors=4))]


def alone_equals_batch(counts):
    clouds = [cloud_of(n, i) for i, n in enumerate(counts)]
    pre = prefix_of(counts)
    for mode, kw in MODES:
        got = run(np.concatenate(clouds, 1), mode, prefix=pre, **kw)
        for b, n in enumerate(counts):
            sl = slice(pre[b], pre[b + 1])
            if n == 0:
                assert not got['stats'][b].any() and not got['thresh'][b].any()
                continue
            one = run(clouds[b], mode, **kw)
            part = {key: (None if got[key] is None else got[key][b:b + 1] if key in ('thresh', 'stats') else got[key][sl]) for key in KEYS}
            same(part, one, pre[b])
    return got


def test_ragged_batches_and_empty_clouds_equal_their_clouds():
    got = alone_equals_batch([300, 0, 1025, 37, 3, 1, 0, 2100])
    assert got['stats'][:, 1].tolist()[1] == 0 and got['stats'][7, 0] == 2100
    alone_equals_batch([0, 0, 700])


def test_a_batch_of_64_clouds_equals_its_clouds():
    alone_equals_batch(counts64())


def test_strided_views_are_read_in_place_and_nothing_else_is_written():
    from hplflownet_amd import ops
    n = 700
    pc = O.scene(n, 14, 3)[0]
    want = run(pc, k=16, radius=1.0)
    wide = torch.full((3, n + 7), float('nan'), device=DEV)
    wide[:, 3:3 + n] = dev(pc)
    guard = torch.full((3, n), 77, dtype=torch.uint8, device=DEV)
    got = ops.outlier_filter(wide[:, 3:3 + n], k=16, radius=1.0, return_neighbors=True, out=guard[1])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == guard[1].data_ptr()
    same({key: (None if v is None else v.cpu().numpy()) for key, v in zip(KEYS, got[:6] + (got[6],))}, want)
    assert bool((guard[0] == 77).all()) and bool((guard[2] == 77).all())
    assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + n:]).all()) and torch.equal(wide[:, 3:3 + n], dev(pc))


def test_same_bits_twice_and_beside_a_busy_stream():
    counts = [300, 0, 1025, 37, 513]
    pc = np.concatenate([cloud_of(n, i) for i, n in enumerate(counts)], 1)
    pre = prefix_of(counts)
    t = dev(pc)
    for mode, kw in MODES:
        first = run(t, mode, prefix=pre, **kw)
        same(first, run(t, mode, prefix=pre, **kw))
        side = torch.cuda.Stream()
        a = torch.randn(2048, 2048, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = torch.tanh(a @ a * 1e-3)
        same(first, run(t, mode, prefix=pre, **kw))


def test_optional_outputs_may_be_null():
    """The C entry with keep, keep_idx, mean_dist, count and nbr_d2 NULL: thresh and stats are the full call's."""
    from hplflownet_amd import _lib
    lib = _lib.load()
    counts = [700, 0, 1300]
    pre = prefix_of(counts)
    t = dev(np.concatenate([cloud_of(n, 20 + i) for i, n in enumerate(counts)], 1))
    N, B = t.shape[1], len(counts)
    ws = torch.empty(lib.hpl_outlier_filter_workspace_bytes(B, N), dtype=torch.uint8, device=DEV)
    for mode, kw in MODES:
        want = run(t, mode, prefix=pre, **kw)
        thresh = torch.full((B, 4), -1.0, device=DEV)
        stats = torch.full((B, 4), -1, dtype=torch.int32, device=DEV)
        keep = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
        for outs in ((None, None), (keep.data_ptr(), None)):
            rc = lib.hpl_outlier_filter(t.data_ptr(), N, B, (ctypes.c_int64 * (B + 1))(*pre), 0 if mode == 'statistical' else 1,
                                        kw.get('k', 0), kw['radius'], kw.get('std_ratio', 0.0), kw.get('min_neighbors', 0), outs[0],
                                        outs[1], None, None, None, thresh.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _lib.stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.hpl_last_error()
            assert np.array_equal(bits(thresh.cpu().numpy()), bits(want['thresh'])) and np.array_equal(stats.cpu().numpy(), want['stats'])
        assert np.array_equal(keep.cpu().numpy(), want['keep'])


# ----------------------------------------------------------------------------- 5. wrappers
def test_op_refusals_and_shapes():
    from hplflownet_amd import _lib, ops
    a = torch.zeros(3, 10, device=DEV)
    for kw in (dict(k=0), dict(k=33), dict(k=16.0), dict(radius=0.0), dict(radius=float('nan')), dict(std_ratio=-1.0),
               dict(mode='radius'), dict(min_neighbors=2), dict(mode='radius', min_neighbors=0),
               dict(prefix=[0, 4]), dict(prefix=[1, 10]), dict(prefix=[0, 12, 10]), dict(prefix=[0] * 65 + [10]),
               dict(out=torch.zeros(10, dtype=torch.uint8)), dict(out=torch.zeros(10, device=DEV)),
               dict(out=torch.zeros(20, dtype=torch.uint8, device=DEV)[::2]), dict(out=torch.zeros(11, dtype=torch.uint8, device=DEV))):
        with pytest.raises(_lib.HplError):
            ops.outlier_filter(a, **kw)
    for bad in (a.double(), torch.zeros(10, 3, device=DEV), a.clone().requires_grad_(), a.cpu(), a[None]):
        with pytest.raises(_lib.HplError):
            ops.outlier_filter(bad)
    got = ops.outlier_filter(a, k=3)                          # ten indices in one place
    assert [tuple(x.shape) for x in got if x is not None] == [(10,), (10,), (10,), (10,), (1, 4), (1, 4)]
    assert got[0].dtype == torch.uint8 and bool(got[0].all()) and got[1].tolist() == list(range(10)) and not bool(got[2].any())
    assert got[3].tolist() == [3] * 10 and got[5].tolist() == [[10, 10, 0, 0]]
    rad = ops.outlier_filter(a, mode='radius', min_neighbors=10)
    assert rad[2] is None and rad[3].tolist() == [9] * 10 and not bool(rad[0].any()) and rad[1].tolist() == [-1] * 10
    empty = ops.outlier_filter(torch.zeros(3, 0, device=DEV), prefix=[0, 0, 0], return_neighbors=True)
    assert [tuple(x.shape) for x in empty] == [(0,), (0,), (0,), (0,), (2, 4), (2, 4), (0, 16)]
    assert not bool(empty[4].any()) and not bool(empty[5].any())


def pair(n, seed):
    """A corresponding pair with strays: sf a small flow, pc2 = pc1 + sf in float32, so that pc2 - pc1 is sf again bit for bit;
    five points of pc2 alone are thrown far off, each somewhere else."""
    p1 = O.scene(n, n // 40, seed)[0]
    rng = np.random.RandomState(seed)
    p2 = p1 + rng.normal(0, 0.05, p1.shape).astype(F)
    p2[:, rng.choice(n, 5, replace=False)] += (F(30) * np.arange(1, 6, dtype=F))[None, :]   # each alone
    return p1, p2, p2 - p1


def teq(t, a):
    return t.dtype == torch.float32 and np.array_equal(bits(t.cpu().numpy()), bits(a))


@pytest.mark.parametrize('form', ['single', 'batch', 'list'])
def test_remove_outliers_forms(form):
    from hplflownet_amd import flownet, ops
    if form == 'single':
        ps = [pair(700, 31)]
        args = [dev(x) for x in ps[0]]
    elif form == 'batch':
        ps = [pair(600, 32), pair(600, 33)]
        args = [dev(np.stack([p[i] for p in ps])) for i in range(3)]
    else:
        ps = [pair(300, 34), pair(1025, 35), pair(257, 36)]
        args = [[dev(p[i]) for p in ps] for i in range(3)]
    B = len(ps)
    kw = dict(k=8, radius=2.0, std_ratio=2.0)
    pre = prefix_of([p[0].shape[1] for p in ps] * 2)
    both = ops.outlier_filter(dev(np.concatenate([p[0] for p in ps] + [p[1] for p in ps], 1)), prefix=pre, **kw)
    keep = both[0].cpu().numpy().astype(bool)
    # corr=True, by='either': the ops composed by hand over the 2 B clouds
    o1, o2, osf, thresh, stats, masks = flownet.remove_outliers(*args, return_mask=True, **kw)
    assert thresh.shape == (2, B, 4) and stats.shape == (2, B, 4) and torch.equal(thresh.view(-1, 4), both[4])
    assert torch.equal(stats.view(-1, 4), both[5]) and len(o1) == len(o2) == len(osf) == len(masks) == B
    for b, (p1, p2, sf) in enumerate(ps):
        m = keep[pre[b]:pre[b + 1]] & keep[pre[B + b]:pre[B + b + 1]]
        assert np.array_equal(masks[b], m) and 0 < m.sum() < len(m)
        assert teq(o1[b], p1[:, m]) and teq(o2[b], p2[:, m]) and teq(osf[b], sf[:, m])
        assert teq(o2[b] - o1[b], osf[b].cpu().numpy())       # a pair stays a pair, exactly
    assert sum(m.sum() for m in masks) < keep[:pre[B]].sum()      # somewhere pc2 alone decided
    assert flownet.remove_outliers(args[0], args[1], **kw)[2] is None
    # by='pc1': pc1's clouds decide
    one = ops.outlier_filter(dev(np.concatenate([p[0] for p in ps], 1)), prefix=pre[:B + 1], **kw)
    k1 = one[0].cpu().numpy().astype(bool)
    for extra in (dict(), dict(return_mask=True)):
        res = flownet.remove_outliers(*args, by='pc1', **kw, **extra)
        assert torch.equal(res[3], one[4]) and torch.equal(res[4], one[5]) and res[4].shape == (B, 4)
        for b, (p1, p2, sf) in enumerate(ps):
            m = k1[pre[b]:pre[b + 1]]
            assert teq(res[0][b], p1[:, m]) and teq(res[1][b], p2[:, m]) and teq(res[2][b], sf[:, m])
            assert teq(res[1][b] - res[0][b], res[2][b].cpu().numpy())
            assert not extra or np.array_equal(res[5][b], m)
    alone = flownet.remove_outliers(args[0], **kw)            # without pc2: pc1 decides
    assert alone[1] is None and alone[2] is None and all(torch.equal(x, y) for x, y in zip(alone[0], res[0]))
    # corr=False: every cloud on its own; sf with pc1
    o1, o2, osf, thresh, stats = flownet.remove_outliers(*args, corr=False, **kw)
    assert torch.equal(thresh.view(-1, 4), both[4]) and torch.equal(stats.view(-1, 4), both[5])
    for b, (p1, p2, sf) in enumerate(ps):
        m1, m2 = keep[pre[b]:pre[b + 1]], keep[pre[B + b]:pre[B + b + 1]]
        assert teq(o1[b], p1[:, m1]) and teq(o2[b], p2[:, m2]) and teq(osf[b], sf[:, m1])
    # the radius mode goes through the same path
    r = flownet.remove_outliers(*args, mode='radius', radius=1.0, min_neighbors=3, by='pc1')
    rk = ops.outlier_filter(dev(np.concatenate([p[0] for p in ps], 1)), mode='radius', radius=1.0, min_neighbors=3, prefix=pre[:B + 1])
    assert all(teq(r[0][b], ps[b][0][:, rk[0].cpu().numpy().astype(bool)[pre[b]:pre[b + 1]]]) for b in range(B))


# ----------------------------------------------------------------------------- the reader and the engine
def test_reader_and_engine_remove_the_strays(tmp_path):
    from hplflownet_amd import data, engine, flownet
    root = tmp_path / 'KITTI_processed_occ_final'
    frames = {}
    for f, n in enumerate((2600, 1800, 3100)):
        d = root / ('%06d' % f)
        d.mkdir(parents=True)
        p1, p2, _ = pair(n, 50 + f)
        frames[f] = (str(d), np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T))
        np.save(str(d / 'pc1.npy'), frames[f][1])
        np.save(str(d / 'pc2.npy'), frames[f][2])
    for outlier in (dict(k=8, radius=2.0), dict(mode='radius', radius=1.0, min_neighbors=3, by='pc1')):
        reader = data.KITTI(None, str(tmp_path), device='cuda', outlier=outlier)
        for f, (path, a1, a2) in frames.items():
            ground = ~((a1[:, 1] < -1.4) & (a2[:, 1] < -1.4))    # the ground rule first
            m = flownet.remove_outliers(dev(a1[ground].T), dev(a2[ground].T), return_mask=True, **outlier)[-1][0]
            o1, o2 = reader.load(path)
            assert 0 < m.sum() < ground.sum() < len(a1) and o1.shape == o2.shape == (m.sum(), 3)
            assert np.array_equal(bits(o1), bits(a1[ground][m])) and np.array_equal(bits(o2), bits(a2[ground][m]))
    res = engine.main(['--dataset', 'KITTI', '--evaluate', '--outlier', 'statistical', '--outlier-k', '8', '--outlier-radius', '2',
                       '--batch-size', '2', '--ragged', '--data-root', str(tmp_path), '--points', '8192', '--arch',
                       'HPLFlowNetShallow'])
    assert res and all(np.isfinite(v) for v in res.values()), res
    assert (res['outlier_mode'], res['outlier_k'], res['outlier_radius'], res['outlier_std_ratio']) == (0.0, 8.0, 2.0, 2.0)
    assert 'outlier_min_neighbors' not in res
