"""GPU: hpl_normals / ops.normals / estimate_normals against the numpy restatement tests/normals_oracle.py.
The neighbourhoods (count, indices, the bits of d2) must EQUAL the restatement's; normals and curvature are compared where the
restatement's smallest eigenvalue stands apart, within the rounding of a float64 unit vector to float32 on both sides (2^-25
each, and the two float64 eigenvectors differ by far less at a relative gap of 1e-3): 2^-23, derived and not measured.  A cloud
has the same bits alone, anywhere in a batch, through strided views, twice and beside a busy stream."""
import numpy as np
import pytest
import torch

import normals_oracle as O
from batch64 import counts64, prefix_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BAR = 2.0 ** -23
F = np.float32


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(pc, k=16, radius=1.0, viewpoint=None, prefix=None):
    from hplflownet_amd import ops
    out = ops.normals(dev(pc), k=k, radius=radius, viewpoint=viewpoint, prefix=prefix, return_neighbors=True)
    torch.cuda.synchronize()
    return out                                   # normal, curvature, count, nbr, nbr_d2


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- 1. neighbourhoods are exact
def doctored(n, kind):
    """The clouds of the neighbourhood tests.  'scene': the surface scene with, as far as n allows, duplicates (ties decided by
    index), a point exactly at the radius 1 of another and one a float past it, isolated points, points on cell borders
    (multiples of the cell edge 1.001), NaN / inf points and points at 1e7 m.  'lattice': a 0.25 m lattice, most d2 tied.
    'one_cell': every point inside one cell."""
    rng = np.random.RandomState(n)
    if kind == 'lattice':
        return (rng.randint(-4, 5, (3, n)) * 0.25).astype(F)
    if kind == 'one_cell':
        return rng.uniform(0.05, 0.95, (3, n)).astype(F)
    if n < 255:
        pc = rng.uniform(-0.4, 0.4, (3, n)).astype(F)
        if n >= 4:
            pc[:, 3] = pc[:, 0]
        return pc
    pc = O.scene(n, n)
    pc[:, 3] = pc[:, 1]
    pc[:, 10] = pc[:, 1]                                       # three points in one place
    pc[:, 5], pc[:, 6], pc[:, 7] = (np.nan, 1, 5), (1, 1, np.inf), (1, -np.inf, 5)
    pc[:, 8], pc[:, 9] = 1e7, (1e7, 0, 5)
    pc[:, 20] = (100, 0, 0)
    pc[:, 21] = (101, 0, 0)                                    # d2 = 1 = radius^2: a neighbour of point 20
    pc[:, 22] = (np.nextafter(F(99), F(-np.inf)), 0, 0)        # a float past it: none
    pc[:, 23] = (-200, 50, 50)                                 # alone
    edge = F(1.001)
    for t in range(12):                                        # on the borders of the cells, in one, two and three coordinates
        c = np.array([F(edge * F(t % 4 - 1)), F(-1.5) if t % 3 else F(edge * F(-2)), F(5) if t % 2 else F(edge * F(5))], F)
        pc[:, 30 + t] = c
    pc[:, 42] = (0.0, -1.5, 5.0)
    pc[:, 43] = (-0.0, -1.5, 5.0)
    return pc


_NEIGH = {}


def oracle_neighbourhoods(n, kind):
    """The restatement at k = 32, once per cloud: a shorter list is its head."""
    if (n, kind) not in _NEIGH:
        pc = doctored(n, kind)
        _NEIGH[(n, kind)] = (pc,) + O.neighbourhoods(pc, 32, 1.0)
    return _NEIGH[(n, kind)]


CLOUDS = [(1, 'scene'), (3, 'scene'), (4, 'scene'), (4, 'lattice'), (255, 'scene'), (257, 'scene'), (257, 'lattice'), (1025, 'scene'),
          (1025, 'one_cell'), (3000, 'scene')]


@pytest.mark.parametrize('k', [3, 8, 9, 16, 17, 32])
@pytest.mark.parametrize('n,kind', CLOUDS, ids=['%d-%s' % c for c in CLOUDS])
def test_neighbourhoods_equal_the_restatement(n, kind, k):
    pc, count, nbr, nd2 = oracle_neighbourhoods(n, kind)
    got = run(pc, k=k, radius=1.0)
    assert np.array_equal(got[2].cpu().numpy(), np.minimum(count, k))
    assert np.array_equal(got[3].cpu().numpy(), nbr[:, :k])
    assert np.array_equal(got[4].cpu().numpy().view(np.int32), nd2[:, :k].view(np.int32))
    if kind == 'scene' and n >= 255:                          # the doctored points did what they are there for
        c = got[2].cpu().numpy()
        assert (c[[5, 6, 7, 8, 9]] == 0).all() and c[20] == 2 and c[21] == 2 and c[22] == 1 and c[23] == 1
        assert list(got[3][1, :3].cpu()) == [1, 3, 10] and list(got[3][10, :3].cpu()) == [1, 3, 10]
    if kind == 'one_cell' and k == 32:
        assert (got[2].cpu().numpy() == 32).all()


def test_far_points_take_part_when_the_cells_are_large():
    """At 1e7 m a float32 step is 1 m: with radius 64 the cell numbers fit and the points are neighbours like any others."""
    rng = np.random.RandomState(5)
    pc = (1e7 + rng.randint(-100, 101, (3, 200))).astype(F)
    pc[:, 0] = 3e7                                            # past the cells' range even so
    want = O.neighbourhoods(pc, 8, 64.0)
    got = run(pc, k=8, radius=64.0)
    assert want[0][0] == 0 and want[0][1:].min() >= 1 and want[0].max() == 8
    assert np.array_equal(got[2].cpu().numpy(), want[0]) and np.array_equal(got[3].cpu().numpy(), want[1])
    assert np.array_equal(got[4].cpu().numpy().view(np.int32), want[2].view(np.int32))


def test_the_last_cells_of_the_key_and_the_ones_past_them():
    """tests/grid_edge.py: clusters in the cells +-(2^18 - 2) of each axis find each other and nothing else; the clusters one cell
    further out, within the radius of them, take no part (tests/test_grid_edge.py checks the cloud on the CPU)."""
    import grid_edge as E
    pc, inside, cluster = E.cloud()
    E.check_cells(pc, inside, cluster)
    want = O.normals(pc, 8, 1.0)
    normal, curv, count, nbr, nd2 = [x.cpu().numpy() for x in run(pc, k=8, radius=1.0)]
    assert np.array_equal(count, want['count']) and np.array_equal(nbr, want['nbr'])
    assert np.array_equal(nd2.view(np.int32), want['nbr_d2'].view(np.int32))
    assert (count[inside] == 4).all() and (count[~inside] == 0).all()
    assert (cluster[nbr[inside, :4]] == cluster[inside][:, None]).all()           # nothing from another edge, nothing from outside
    assert (nbr[~inside] == -1).all() and (normal[:, ~inside] == 0).all() and (curv[~inside] == 0).all()
    cmp_ = want['valid'] & (want['gap'] >= 1e-3)
    assert np.array_equal(cmp_, inside)                                            # every inner point has a normal that stands apart
    assert np.abs(normal.astype(np.float64) - want['normal'].astype(np.float64))[:, cmp_].max() <= BAR


# ----------------------------------------------------------------------------- 2. normals and curvature
_NORMALS = {}


def oracle_normals(n, k, radius):
    if (n, k, radius) not in _NORMALS:
        pc = O.scene(n, 7)
        _NORMALS[(n, k, radius)] = (pc, O.normals(pc, k, radius))
    return _NORMALS[(n, k, radius)]


@pytest.mark.parametrize('n,k,radius', [(300, 16, 2.0), (1025, 8, 1.0), (1025, 16, 1.0), (1025, 32, 1.5), (3000, 8, 1.0),
                                        (3000, 16, 1.0), (3000, 32, 1.5)])
def test_normals_and_curvature_against_the_restatement(n, k, radius):
    pc, want = oracle_normals(n, k, radius)
    got = [x.cpu().numpy() for x in run(pc, k=k, radius=radius)]
    assert np.array_equal(got[2], want['count']) and np.array_equal(got[3], want['nbr'])
    has = want['count'] >= 3
    cmp_ = has & (want['gap'] >= 1e-3)
    share = cmp_.sum() / max(has.sum(), 1)
    err = np.abs(got[0].astype(np.float64) - want['normal'].astype(np.float64))[:, cmp_].max()
    wc = want['curvature'].astype(np.float64)
    cerr = (np.abs(got[1].astype(np.float64) - wc) - (BAR * wc + 1e-12))[cmp_].max()
    print('n = %d, k = %d, radius %g: %d of %d points with three neighbours compared (%.1f %%); normal off by %.3g (bar %.3g), '
          'curvature past its bar by %.3g' % (n, k, radius, cmp_.sum(), has.sum(), 100 * share, err, BAR, cerr))
    assert share >= 0.95
    assert err <= BAR
    assert cerr <= 0
    # the rest: unit normals where the restatement has one, zeros where it has none
    length = np.sqrt((got[0].astype(np.float64) ** 2).sum(0))
    assert np.abs(length[want['valid']] - 1).max() <= 2 * BAR
    assert (got[0][:, ~want['valid']] == 0).all() and (got[1][~want['valid']] == 0).all()
    assert (got[1] >= 0).all() and (got[1] <= F(1 / 3) + F(BAR)).all()


def test_collinear_neighbours_and_coincident_points():
    """An exactly collinear neighbourhood has two zero eigenvalues: the normal is some unit vector perpendicular to the line.
    Points all in one place have no direction at all: no normal."""
    d = np.array([1.0, 2.0, -1.0])
    line = (np.arange(12)[None, :] * 0.125 * d[:, None]).astype(F)                # exact in float32
    heap = np.tile(np.array([[40.0], [3.0], [-7.0]], F), (1, 5))
    two = np.array([[80.0, 80.25], [0, 0], [0, 0]], F)                             # fewer than three neighbours
    pc = np.concatenate([line, heap, two], 1)
    want = O.normals(pc, 8, 1.0)
    normal, curv, count, _, _ = [x.cpu().numpy() for x in run(pc, k=8, radius=1.0)]
    assert np.array_equal(count, want['count']) and (count[:12] >= 3).all() and (count[12:17] == 5).all() and (count[17:] == 2).all()
    n64 = normal[:, :12].astype(np.float64)
    assert np.abs(np.sqrt((n64 ** 2).sum(0)) - 1).max() <= 2 * BAR
    assert np.abs((n64 * (d / np.linalg.norm(d))[:, None]).sum(0)).max() <= 2 * BAR
    assert np.abs(curv[:12]).max() <= 1e-12
    assert (normal[:, 12:] == 0).all() and (curv[12:] == 0).all()


# ----------------------------------------------------------------------------- 3. exact geometry
UNIT = np.array([1.0, 2.0, 2.0]) / 3.0


def tilted_plane(n=400, seed=11):
    """Noise-free points of the plane (1, 2, 2) . x = 27 through (3, 6, 6): c + a u + b v with u = (2, 1, -2), v = (2, -2, 1) and
    a, b multiples of 1/64 -- every coordinate exact in float32."""
    rng = np.random.RandomState(seed)
    a, b = rng.randint(-64, 65, n) / 64.0, rng.randint(-64, 65, n) / 64.0
    p = np.array([[3.0], [6.0], [6.0]]) + a * np.array([[2.0], [1.0], [-2.0]]) + b * np.array([[2.0], [-2.0], [1.0]])
    assert np.array_equal(p.astype(F).astype(np.float64), p)
    return p.astype(F)


def test_a_plane_gives_its_normal_and_the_viewpoint_its_sign():
    pc = tilted_plane()
    normal, curv, count, _, _ = [x.cpu().numpy() for x in run(pc, k=16, radius=1.0)]
    ok = count >= 3
    assert ok.mean() > 0.95
    assert np.abs(normal[:, ok] + UNIT[:, None]).max() <= BAR                       # the origin lies on the negative side
    assert np.abs(curv).max() <= 1e-12
    flipped = run(pc, k=16, radius=1.0, viewpoint=(10.0, 20.0, 20.0))
    assert np.abs(flipped[0].cpu().numpy()[:, ok] - UNIT[:, None]).max() <= BAR
    assert torch.equal(bits(flipped[0]) & 0x7fffffff, bits(dev(normal)) & 0x7fffffff) and same(flipped[1:], run(pc, k=16, radius=1.0)[1:])
    # per-cloud viewpoints in a batch: the cloud twice, seen from either side
    both = run(np.concatenate([pc, pc], 1), k=16, radius=1.0, viewpoint=[[0, 0, 0], [10, 20, 20]], prefix=[0, 400, 800])
    assert torch.equal(bits(both[0][:, :400]), bits(dev(normal))) and torch.equal(bits(both[0][:, 400:]), bits(flipped[0]))
    one = run(np.concatenate([pc, pc], 1), k=16, radius=1.0, viewpoint=(10, 20, 20), prefix=[0, 400, 800])
    assert torch.equal(bits(one[0][:, :400]), bits(flipped[0])) and torch.equal(bits(one[0][:, 400:]), bits(flipped[0]))


def test_a_viewpoint_on_the_point_itself_takes_the_positive_first_component():
    """s == 0: the viewpoint IS point 0, so v - p = 0 exactly and the sign comes from the first non-zero component."""
    pc = tilted_plane()
    view = tuple(float(x) for x in pc[:, 0])
    want = O.normals(pc, 16, 1.0, viewpoint=view)
    got = run(pc, k=16, radius=1.0, viewpoint=view)[0].cpu().numpy()
    assert want['count'][0] >= 3 and want['normal'][0, 0] > 0 and got[0, 0] > 0
    assert np.abs(got[:, 0] - UNIT).max() <= BAR
    # an axis-aligned plane: the eigenvector is exactly (0, 0, 1), its first non-zero component the last
    flat = pc.copy()
    flat[2] = 2.0
    view = tuple(float(x) for x in flat[:, 0])
    got = run(flat, k=16, radius=1.0, viewpoint=view)
    assert got[2][0] >= 3 and got[0][:, 0].cpu().tolist() == [0.0, 0.0, 1.0]


# ----------------------------------------------------------------------------- 4. bits
def cloud_of(n, seed):
    return O.scene(n, 100 + seed) if n >= 8 else np.random.RandomState(seed).uniform(-0.3, 0.3, (3, n)).astype(F)


def alone_equals_batch(counts, k, radius):
    clouds = [cloud_of(n, i) for i, n in enumerate(counts)]
    pre = prefix_of(counts)
    views = [(float(i % 3), -1.0, float(i % 5)) for i in range(len(counts))]
    got = run(np.concatenate(clouds, 1), k=k, radius=radius, viewpoint=views, prefix=pre)
    for b, n in enumerate(counts):
        if n == 0:
            continue
        one = run(clouds[b], k=k, radius=radius, viewpoint=views[b])
        sl = slice(pre[b], pre[b + 1])
        assert same((got[0][:, sl], got[1][sl], got[2][sl], got[4][sl]), (one[0], one[1], one[2], one[4])), b
        assert torch.equal(got[3][sl], torch.where(one[3] >= 0, one[3] + pre[b], one[3])), b
    return got


def test_ragged_batches_and_empty_clouds_equal_their_clouds():
    got = alone_equals_batch([300, 0, 1025, 37, 3, 1, 0, 513], 16, 2.0)
    assert int(got[2][:300].max()) == 16
    alone_equals_batch([0, 0, 700], 9, 1.0)


def test_a_batch_of_64_clouds_equals_its_clouds():
    alone_equals_batch(counts64(), 8, 2.0)


def test_strided_views_are_read_in_place_and_nothing_else_is_written():
    from hplflownet_amd import ops
    n = 700
    pc = O.scene(n, 3)
    want = run(pc, k=16, radius=1.0)
    wide = torch.full((3, n + 7), float('nan'), device=DEV)
    wide[:, 3:3 + n] = dev(pc)
    guard = torch.full((5, n + 4), float('nan'), device=DEV)
    out = guard[1:4, 2:2 + n]
    got = ops.normals(wide[:, 3:3 + n], k=16, radius=1.0, return_neighbors=True, out=out)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr() and same(want, got)
    assert bool(torch.isnan(guard[0]).all()) and bool(torch.isnan(guard[4]).all())
    assert bool(torch.isnan(guard[:, :2]).all()) and bool(torch.isnan(guard[:, 2 + n:]).all())
    assert bool(torch.isnan(wide[:, :3]).all()) and bool(torch.isnan(wide[:, 3 + n:]).all()) and torch.equal(wide[:, 3:3 + n], dev(pc))


def test_same_bits_twice_and_beside_a_busy_stream():
    from hplflownet_amd import ops
    counts = [300, 0, 1025, 37, 513]
    pc = np.concatenate([cloud_of(n, i) for i, n in enumerate(counts)], 1)
    pre = prefix_of(counts)
    first = run(pc, k=16, radius=1.5, prefix=pre)
    assert same(first, run(pc, k=16, radius=1.5, prefix=pre))
    t = dev(pc)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            a = torch.tanh(a @ a * 1e-3)
    busy = ops.normals(t, k=16, radius=1.5, prefix=pre, return_neighbors=True)
    torch.cuda.synchronize()
    assert same(first, busy)


# ----------------------------------------------------------------------------- 5. wrappers
def test_op_refusals():
    from hplflownet_amd import _lib, ops
    a = torch.zeros(3, 10, device=DEV)
    for kw in (dict(k=2), dict(k=33), dict(k=16.0), dict(radius=0.0), dict(radius=float('inf')), dict(radius=float('nan')),
               dict(prefix=[0, 4]), dict(prefix=[1, 10]), dict(prefix=[0, 12, 10]), dict(prefix=[0] * 65 + [10]),
               dict(viewpoint=(0.0, 1.0)), dict(viewpoint=[[0, 0, 0], [1, 1, 1]]), dict(viewpoint='up'),
               dict(viewpoint=[[0, 0, 0]] * 3, prefix=[0, 5, 10]),
               dict(out=torch.zeros(3, 10)), dict(out=torch.zeros(10, 3, device=DEV)), dict(out=torch.zeros(3, 10, device=DEV).double()),
               dict(out=torch.zeros(3, 20, device=DEV)[:, ::2]), dict(out=torch.zeros(3, 10, device=DEV, requires_grad=True))):
        with pytest.raises(_lib.HplError):
            ops.normals(a, **kw)
    for bad in (a.double(), torch.zeros(10, 3, device=DEV), a.clone().requires_grad_(), a.cpu(), a[None]):
        with pytest.raises(_lib.HplError):
            ops.normals(bad)
    with pytest.raises(_lib.HplError, match='hpl_normals: the viewpoint of cloud 1 is not finite'):       # the C entry's words
        ops.normals(a, viewpoint=[[0, 0, 0], [0, float('nan'), 0]], prefix=[0, 5, 10])
    with pytest.raises(_lib.HplError, match='hpl_normals: an output overlaps the input'):
        ops.normals(a, out=a)
    got = ops.normals(a, k=3, viewpoint=(1, 2, 3))
    assert [tuple(x.shape) for x in got] == [(3, 10), (10,), (10,)] and int(got[2].min()) == 3 and not bool(got[0].any())
    empty = ops.normals(torch.zeros(3, 0, device=DEV), prefix=[0, 0, 0], return_neighbors=True)
    assert [tuple(x.shape) for x in empty] == [(3, 0), (0,), (0,), (0, 16), (0, 16)]


def test_estimate_normals_takes_the_three_forms():
    import hplflownet_amd as H
    from hplflownet_amd import _lib, ops
    n, B = 700, 3
    p = torch.stack([dev(O.scene(n, 40 + i)) for i in range(B)])
    packed = p.transpose(0, 1).reshape(3, B * n)
    pre = prefix_of([n] * B)
    view = [[0, 0, 0], [0, 5, 0], [1, 1, 1]]
    want = ops.normals(packed, k=8, radius=1.5, viewpoint=view, prefix=pre)
    got = H.estimate_normals(p, k=8, radius=1.5, viewpoint=view)                     # (B, 3, N)
    assert got[0].shape == (B, 3, n) and got[1].shape == (B, n) and got[2].shape == (B, n)
    assert all(same((got[0][b], got[1][b], got[2][b]), (want[0][:, pre[b]:pre[b + 1]], want[1][pre[b]:pre[b + 1]],
                                                        want[2][pre[b]:pre[b + 1]])) for b in range(B))
    one = H.estimate_normals(p[1], k=8, radius=1.5, viewpoint=view[1])               # (3, N): one cloud
    assert one[0].shape == (3, n) and same(one, (got[0][1], got[1][1], got[2][1]))
    ns = (700, 300, 512)                                                             # a list of ragged clouds
    clouds = [p[b][:, :ns[b]] for b in range(B)]
    rp = prefix_of(list(ns))
    wantl = ops.normals(torch.cat(clouds, 1), k=8, radius=1.5, prefix=rp)
    gotl = H.estimate_normals([clouds[0], clouds[1][None], clouds[2]], k=8, radius=1.5)
    assert [tuple(x.shape) for x in gotl[0]] == [(3, 700), (1, 3, 300), (3, 512)] and same(wantl[1:], gotl[1:])
    assert all(torch.equal(bits(x.reshape(3, -1)), bits(wantl[0][:, rp[b]:rp[b + 1]])) for b, x in enumerate(gotl[0]))
    gotp = H.estimate_normals(torch.cat(clouds, 1), list(ns), k=8, radius=1.5)       # a packed cloud with its counts
    assert same(wantl, gotp)
    for bad in ((torch.cat(clouds, 1), [700, 300]), (p[0][0],), ([],), (clouds, [700, 300, 500])):
        with pytest.raises(_lib.HplError):
            H.estimate_normals(*bad)
