"""GPU: hpl_render_maps / hpl_maps_to_kitti through ops, flownet and the engine.  The device's outputs equal the
numpy restatement tests/render_oracle.py bit for bit: pixel_of, winner, depth, attr_map, visible, stats and the five KITTI
planes.  Both sides compute in float32 with one rounding per operation and the z-buffer is an integer minimum, so nothing here
has a tolerance.  A workgroup takes 256 points (or pixels) of one cloud (or frame): the shapes lie either side of a wave, a
workgroup and several, and clouds and frames inside a batch start at every residue mod 4."""
import os

import numpy as np
import pytest
import torch

import frames_oracle as FO
import render_oracle as RO
from batch64 import counts64
from common import ROOT
from hplflownet_amd import _lib, data, flownet, ops

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))
KEYS = ('pixel_of', 'winner', 'depth', 'attr_map', 'visible', 'stats')
COUNTS = [1, 63, 65, 255, 256, 257, 1025]
SIZES = [(1, 1), (1, 1025), (37, 131), (3, 1300)]


def run(clouds, cameras, sizes, attrs=None, out=None, wide=0, **kw):
    """ONE ops.render_maps call over the clouds ([n_b, 3] host arrays) -> dict of host arrays.  wide > 0: pc and attrs are views
    of buffers `wide` columns wider."""
    pc, prefix = RO.pack(clouds)
    N = pc.shape[1]
    t = torch.from_numpy(pc).cuda()
    a = None if attrs is None else torch.from_numpy(np.ascontiguousarray(np.concatenate(attrs, axis=1))).cuda()
    if wide:
        buf = torch.full((3, N + wide), float('nan'), device='cuda')
        buf[:, 3:3 + N] = t
        t = buf[:, 3:3 + N]
        if a is not None:
            abuf = torch.full((a.shape[0], N + wide), float('nan'), device='cuda')
            abuf[:, 1:1 + N] = a
            a = abuf[:, 1:1 + N]
    res = ops.render_maps(t, cameras, [s[0] for s in sizes], [s[1] for s in sizes], attrs=a, prefix=prefix, out=out, **kw)
    return {k: None if x is None else x.cpu().numpy() for k, x in zip(KEYS, res)}


def check(got, want):
    for k in ('pixel_of', 'winner', 'visible', 'stats'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, got['stats'], want['stats'])
    assert FO.same_bits(got['depth'], want['depth'])
    assert (got['attr_map'] is None) == (want['attr_map'] is None)
    if want['attr_map'] is not None:
        assert FO.same_bits(got['attr_map'], want['attr_map'])


def both(clouds, cameras, sizes, attrs=None, **kw):
    got, want = run(clouds, cameras, sizes, attrs, **kw), RO.render_batch(clouds, cameras, sizes, attrs, **{k: v for k, v in kw.items() if k != 'wide'})
    check(got, want)
    return got, want


# ----------------------------------------------------------------------------- sizes and offsets
@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_sizes_alone(size):
    rng = np.random.RandomState(size[0] * 7919 + size[1])
    for n in COUNTS:
        pc = RO.random_cloud(rng, n, *size, bad=0.1)
        attrs = [rng.randn(3, n).astype(f32)]
        got, want = both([pc], [RO.KITTI_CAMERA], [size], attrs, footprint=n % 2, rel_tol=0.02)
    assert want['stats'][0, 0] > 0 and want['stats'][0, 1] > 0


def test_sizes_together_start_at_every_residue():
    rng = np.random.RandomState(77)
    counts = [1, 65, 257, 63, 255, 256, 1025]
    sizes = [(1, 1), (1, 1025), (1, 1), (37, 131), (3, 1300), (5, 7), (37, 131)]
    assert set(int(s) % 4 for s in np.cumsum([0] + counts)[:-1]) == {0, 1, 2, 3}
    assert set(int(s) % 4 for s in np.cumsum([0] + [h * w for h, w in sizes])[:-1]) == {0, 1, 2, 3}
    clouds = [RO.random_cloud(rng, n, *s, bad=0.05) for n, s in zip(counts, sizes)]
    cams = [RO.KITTI_CAMERA if b % 2 else RO.camera_of_P(FO.read_P(FO.CALIB_NAMES[b % 3])) for b in range(len(counts))]
    attrs = [rng.randn(2, n).astype(f32) for n in counts]
    for r in (0, 1):
        both(clouds, cams, sizes, attrs, footprint=r, rel_tol=0.01, abs_tol=0.05)


def test_empty_clouds_and_empty_images_inside_a_batch():
    rng = np.random.RandomState(5)
    some = RO.random_cloud(rng, 300, 9, 31)
    none = np.zeros((0, 3), f32)
    clouds = [none, some, some, none, some]
    sizes = [(9, 31), (0, 7), (9, 31), (0, 0), (5, 0)]
    got, want = both(clouds, [RO.KITTI_CAMERA] * 5, sizes, [rng.randn(1, len(c)).astype(f32) for c in clouds], footprint=1)
    assert want['stats'][:, 0].tolist()[1] == 0 and want['stats'][2, 0] > 0 and (got['winner'][:9 * 31] == -1).all()
    # all clouds empty with pixels, and all images empty with points: the launches of the other side still run
    got, _ = both([none, none], [RO.KITTI_CAMERA] * 2, [(3, 5), (2, 2)])
    assert (got['winner'] == -1).all() and not got['depth'].any() and not got['stats'].any()
    got, _ = both([some, some], [RO.KITTI_CAMERA] * 2, [(0, 5), (0, 0)])
    assert (got['pixel_of'] == -1).all() and not got['visible'].any()
    res = ops.render_maps(torch.zeros((3, 0), device='cuda'), [RO.KITTI_CAMERA], [0], [9])
    assert res[5].tolist() == [[0, 0, 0, 0]] and res[1].numel() == 0


def test_64_clouds_each_as_alone():
    rng = np.random.RandomState(64)
    counts = counts64()
    sizes = [(0, 5) if i % 7 == 3 else (1 + i % 5, 3 + (7 * i) % 29) for i in range(64)]
    sizes[40], sizes[50] = (37, 131), (3, 1300)
    clouds = [RO.random_cloud(rng, n, *(s if s[0] else (4, 4)), bad=0.1) for n, s in zip(counts, sizes)]
    cams = [RO.camera_of_P(FO.read_P(FO.CALIB_NAMES[i % 3])) for i in range(64)]
    attrs = [rng.randn(8, n).astype(f32) for n in counts]
    got, _ = both(clouds, cams, sizes, attrs, footprint=1, rel_tol=0.02)
    p0 = q0 = 0
    for i in range(64):
        n, m = counts[i], sizes[i][0] * sizes[i][1]
        if n + m:                                             # the device's own single-cloud run
            alone = run([clouds[i]], [cams[i]], [sizes[i]], [attrs[i]], footprint=1, rel_tol=0.02)
            for k, (a, b) in (('pixel_of', (p0, p0 + n)), ('visible', (p0, p0 + n)), ('winner', (q0, q0 + m)), ('depth', (q0, q0 + m))):
                assert FO.same_bits(got[k][a:b], alone[k]), (i, k)
            assert FO.same_bits(got['attr_map'][:, q0:q0 + m], alone['attr_map']) and np.array_equal(got['stats'][i], alone['stats'][0])
        p0, q0 = p0 + n, q0 + m


# ----------------------------------------------------------------------------- ties, borders, points that must not project
def test_half_pixel_ties_and_borders():
    W, H = 6, 5
    below = float(np.nextafter(f32(-0.5), f32(-1)))
    us = [0.5, 1.5, 2.5, 3.5, 4.5, -0.5, -0.50001, below, W - 0.5, W - 1.0, -1.0, float(W), 2.0, 2.0, 2.0, 2.0]
    vs = [1.0] * 12 + [-1.0, float(H), -0.5, H - 0.5]
    pc = RO.exact_points(us, vs)
    _, u, _ = RO.project(pc, RO.EXACT_CAMERA)
    assert u.tolist() == [float(f32(x)) for x in us]          # the projection is exact: the ties are ties
    got, want = both([pc], [RO.EXACT_CAMERA], [(H, W)])
    assert got['pixel_of'].tolist() == [6, 8, 8, 10, 10, 6, -1, -1, -1, 11, -1, -1, -1, -1, 2, 26]
    both([RO.exact_points(vs, us)], [RO.EXACT_CAMERA], [(W, H)])                 # the same along v


def test_points_that_must_not_project():
    near = f32(0.25)
    zs = [near, np.nextafter(near, f32(0)), f32(0), f32(-2)]
    pc = np.stack([np.zeros(4, f32), np.zeros(4, f32), np.array(zs, f32)], axis=1)
    bad = np.array([[np.inf, 0, 2], [0, -np.inf, 2], [0, 0, np.inf], [np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan],
                    [3e38, 0, 2], [-3e38, 0, 2], [0, 3e38, 2], [4e9, 0, 2], [0, 3e9, 2], [-4e9, 0, 2], [2.2e9, 2.2e9, 2]], f32)
    got, want = both([np.concatenate([pc, bad])], [RO.EXACT_CAMERA], [(5, 5)], near=0.25)
    assert got['pixel_of'].tolist() == [0] + [-1] * 16 and got['stats'].tolist() == [[1, 1, 1, 9]]
    assert got['winner'].tolist() == [0] + [-1] * 24          # no write anywhere else


# ----------------------------------------------------------------------------- contention
@pytest.mark.parametrize('equal', [False, True], ids=['distinct', 'equal'])
def test_4096_points_into_one_pixel(equal):
    rng = np.random.RandomState(12)
    n = 4096
    z = np.full(n, 2.0) if equal else rng.permutation(n) * 0.01 + 2.0
    pc = RO.back_project(np.full(n, 7.2), np.full(n, 3.9), z, RO.KITTI_CAMERA)
    if equal:
        pc[:] = pc[0]
    for r in (0, 1):
        got, want = both([pc], [RO.KITTI_CAMERA], [(9, 15)], footprint=r, rel_tol=0.0 if equal else 0.5)
        assert (got['pixel_of'] == 4 * 15 + 7).all() and got['stats'][0, 1] == (2 * r + 1) ** 2
        first = 0 if equal else int(np.argmin(pc[:, 2]))
        assert got['winner'][4 * 15 + 7] == first and got['stats'][0, 2] == (n if equal else want['stats'][0, 2])


# ----------------------------------------------------------------------------- footprint
@pytest.mark.parametrize('r', [1, 4])
def test_footprint_is_clipped_at_the_corners(r):
    H, W = 11, 13
    us, vs = [0.0, W - 1.0, 0.0, W - 1.0], [0.0, 0.0, H - 1.0, H - 1.0]
    pc = RO.exact_points(us, vs)
    got, _ = both([pc], [RO.EXACT_CAMERA], [(H, W)], footprint=r)
    win = got['winner'].reshape(H, W)
    assert (win[:r + 1, :r + 1] == 0).all() and (win[:r + 1, -r - 1:] == 1).all() and (win[-r - 1:, :r + 1] == 2).all()
    assert (win[-r - 1:, -r - 1:] == 3).all() and (win >= 0).sum() == 4 * (r + 1) ** 2


def test_a_near_footprint_hides_a_far_point():
    pc = np.concatenate([RO.exact_points([5.0], [5.0], 4.0), RO.exact_points([4.0], [4.0], 2.0)])
    got, _ = both([pc], [RO.EXACT_CAMERA], [(9, 9)], footprint=1)
    assert got['visible'].tolist() == [0, 1] and got['winner'][5 * 9 + 5] == 1
    got, _ = both([pc], [RO.EXACT_CAMERA], [(9, 9)], footprint=0)
    assert got['visible'].tolist() == [1, 1]


# ----------------------------------------------------------------------------- tolerances
def test_tolerances_either_side_of_the_threshold():
    z, k = f32(8.0), f32(1.01)
    far = z * k
    pc = np.concatenate([RO.exact_points([1.0], [1.0], 8.0), np.array([[1.0 * far / 2, 1.0 * far / 2, far]], f32)])
    _, u, v = RO.project(pc, RO.EXACT_CAMERA)
    assert np.rint(u).tolist() == [1, 1] and np.rint(v).tolist() == [1, 1]
    seen = {}
    for name, rel in (('0', 0.0), ('below', float(np.nextafter(f32(0.01), f32(0)))), ('at', float(f32(0.01))),
                      ('above', float(np.nextafter(f32(0.01), f32(1)))), ('0.02', 0.02)):
        got, _ = both([pc], [RO.EXACT_CAMERA], [(3, 3)], rel_tol=rel)
        seen[name] = got['visible'].tolist()
    assert seen['0'] == [1, 0] and seen['0.02'] == [1, 1]     # (between them the restatement decides: 1 + rel_tol rounds)
    gap = float(far - z)                                      # exact: the depths are within a factor of two
    for name, tol in (('half', gap / 2), ('below', float(np.nextafter(f32(gap), f32(0)))), ('at', gap),
                      ('above', float(np.nextafter(f32(gap), f32(1))))):
        got, _ = both([pc], [RO.EXACT_CAMERA], [(3, 3)], abs_tol=tol)
        seen['abs ' + name] = got['visible'].tolist()
    assert seen['abs half'] == [1, 0] and seen['abs at'] == [1, 1] and seen['abs above'] == [1, 1]


# ----------------------------------------------------------------------------- channels and views
@pytest.mark.parametrize('C', [0, 1, 8])
def test_channels_and_strided_views(C):
    rng = np.random.RandomState(20 + C)
    counts, sizes = [257, 65], [(9, 31), (5, 7)]
    clouds = [RO.random_cloud(rng, n, *s) for n, s in zip(counts, sizes)]
    attrs = [rng.randn(C, n).astype(f32) for n in counts] if C else None
    M = sum(h * w for h, w in sizes)
    both(clouds, [RO.KITTI_CAMERA] * 2, sizes, attrs, wide=9, footprint=1)
    if C:
        widebuf = torch.full((C, M + 11), 7.0, device='cuda')
        got = run(clouds, [RO.KITTI_CAMERA] * 2, sizes, attrs, out=widebuf[:, 4:4 + M], wide=9, footprint=1)
        check(got, RO.render_batch(clouds, [RO.KITTI_CAMERA] * 2, sizes, attrs, footprint=1))
        assert (widebuf[:, :4] == 7).all() and (widebuf[:, 4 + M:] == 7).all()
    else:
        with pytest.raises(_lib.HplError, match='no attrs'):
            run(clouds, [RO.KITTI_CAMERA] * 2, sizes, None, out=torch.empty((1, M), device='cuda'))


def test_an_output_overlapping_an_input_is_refused():
    rng = np.random.RandomState(21)
    n, size = 200, (10, 20)
    buf = torch.zeros((4, 200), device='cuda')
    buf[:3] = torch.from_numpy(RO.pack([RO.random_cloud(rng, n, *size)])[0]).cuda()
    attrs = torch.zeros((1, n), device='cuda')
    with pytest.raises(_lib.HplError, match='overlaps an input'):
        ops.render_maps(buf[:3], [RO.KITTI_CAMERA], [size[0]], [size[1]], attrs=attrs, out=buf[2:3])
    with pytest.raises(_lib.HplError, match='overlaps an input'):
        ops.render_maps(buf[:3], [RO.KITTI_CAMERA], [size[0]], [size[1]], attrs=buf[3:4], out=buf[3:4])
    ops.render_maps(buf[:3], [RO.KITTI_CAMERA], [size[0]], [size[1]], attrs=attrs, out=buf[3:4])
    for bad in (dict(footprint=5), dict(footprint=True), dict(rel_tol=-0.1), dict(abs_tol=float('nan')), dict(near=0.0)):
        with pytest.raises(_lib.HplError):
            ops.render_maps(buf[:3], [RO.KITTI_CAMERA], [size[0]], [size[1]], **bad)
    with pytest.raises(_lib.HplError):
        ops.render_maps(buf[:3], [RO.KITTI_CAMERA], [size[0], 3], [size[1], 3])          # two frames, one cloud
    with pytest.raises(_lib.HplError):
        ops.render_maps(buf[:3], [(0.0, 1, 1, 0, 0, 0)], [size[0]], [size[1]])


# ----------------------------------------------------------------------------- KITTI round trip on the device
def kitti_frames():
    frames = [(GOLD['kitti%d_disp1' % k], GOLD['kitti%d_disp2' % k], GOLD['kitti%d_flow' % k], FO.read_P(str(GOLD['kitti%d_calib' % k])))
              for k in range(3)]
    rng = np.random.RandomState(34)
    for k, (H, W, lo, extreme) in enumerate([(37, 131, 256, False), (3, 1300, 1, False), (1, 1, 256, False), (19, 50, 256, True),
                                              (48, 97, 16, False)]):
        frames.append(FO.kitti_raw(rng, H, W, p_valid=1.0 if H * W == 1 else 0.7, extreme=extreme, lo=lo) + (FO.read_P(FO.CALIB_NAMES[k % 3]),))
    return frames


def test_kitti_round_trip_on_the_device():
    frames = kitti_frames()
    hh, ww = [fr[0].shape[0] for fr in frames], [fr[0].shape[1] for fr in frames]
    cat = lambda k, tail=(): torch.from_numpy(np.concatenate([np.ascontiguousarray(fr[k]).reshape((-1,) + tail) for fr in frames])).cuda()
    Ps = [fr[3] for fr in frames]
    pc1, pc2, pixel, counts = ops.frames_from_kitti(cat(0), cat(1), cat(2, (3,)), Ps, hh, ww)
    # a frame's valid correspondences lead its range; the zeros behind them are no points
    prefix = [0] + list(np.cumsum([h * w for h, w in zip(hh, ww)]))
    cnt = counts.cpu().tolist()
    keep = torch.cat([torch.arange(prefix[b], prefix[b] + cnt[b]) for b in range(len(frames))]).cuda()
    cprefix = [0] + list(np.cumsum(cnt))
    d1, d2, fl = ops.maps_to_kitti(pc1[:, keep], pc2[:, keep], Ps, hh, ww, prefix=cprefix)
    d1, d2, fl = d1.cpu().numpy(), d2.cpu().numpy(), fl.cpu().numpy()
    for b, fr in enumerate(frames):
        e1, e2, ef = RO.expected_raw(*fr[:3])
        q0, q1 = prefix[b], prefix[b + 1]
        assert np.array_equal(d1[q0:q1].reshape(e1.shape), e1) and np.array_equal(d2[q0:q1].reshape(e2.shape), e2), b
        assert np.array_equal(fl[q0:q1].reshape(ef.shape), ef), b


def test_maps_to_kitti_equals_the_restatement_off_the_round_trip():
    """Clouds that are no back-projection: several points a pixel, partners behind the camera, non-finite points, footprints."""
    rng = np.random.RandomState(35)
    counts, sizes = [1025, 0, 257, 63], [(9, 31), (3, 3), (0, 4), (37, 131)]
    Ps = [FO.read_P(FO.CALIB_NAMES[b % 3]) for b in range(4)]
    c1 = [RO.random_cloud(rng, n, *(s if s[0] else (4, 4)), camera=RO.camera_of_P(P), bad=0.1) for n, s, P in zip(counts, sizes, Ps)]
    c2 = [c + rng.uniform(-0.5, 0.5, c.shape).astype(f32) for c in c1]
    c2[0][::7, 2] = -3.0
    c2[0][::11, 0] = np.nan
    (p1, prefix), (p2, _) = RO.pack(c1), RO.pack(c2)
    for r in (0, 2):
        got = ops.maps_to_kitti(torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda(), Ps, [s[0] for s in sizes], [s[1] for s in sizes],
                                footprint=r, prefix=prefix, baseline=0.5)
        got = [x.cpu().numpy() for x in got]
        q0 = 0
        for b, (H, W) in enumerate(sizes):
            w1, w2, wf = RO.maps_to_kitti(c1[b], c2[b], Ps[b], H, W, baseline=0.5, footprint=r)
            m = H * W
            assert np.array_equal(got[0][q0:q0 + m], w1.reshape(-1)) and np.array_equal(got[1][q0:q0 + m], w2.reshape(-1)), (r, b)
            assert np.array_equal(got[2][q0:q0 + m], wf.reshape(-1, 3)), (r, b)
            q0 += m
        assert got[2][:9 * 31, 2].any() and (got[1][:9 * 31] == 0)[got[0][:9 * 31] > 0].any()


# ----------------------------------------------------------------------------- the wrappers
def test_wrappers_take_a_cloud_a_batch_and_a_list():
    rng = np.random.RandomState(40)
    size, cam = (19, 31), RO.KITTI_CAMERA
    a, b = RO.random_cloud(rng, 300, *size), RO.random_cloud(rng, 300, *size)
    c = RO.random_cloud(rng, 77, 5, 9)
    ta, tb, tc = (torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in (a, b, c))
    wa, wb = (RO.render_maps(x, cam, *size, footprint=1, rel_tol=0.02) for x in (a, b))
    wc = RO.render_maps(c, cam, 5, 9, footprint=1, rel_tol=0.02)
    one = flownet.visibility(ta, cam, size)
    assert one.dtype == torch.bool and tuple(one.shape) == (300,) and np.array_equal(one.cpu().numpy(), wa['visible'] == 1)
    two = flownet.visibility(torch.stack([ta, tb]), cam, size)
    assert tuple(two.shape) == (2, 300) and np.array_equal(two.cpu().numpy(), np.stack([wa['visible'], wb['visible']]) == 1)
    lst = flownet.visibility([ta, tc], [cam, cam], [size, (5, 9)])
    assert [tuple(x.shape) for x in lst] == [(300,), (77,)] and np.array_equal(lst[1].cpu().numpy(), wc['visible'] == 1)
    attrs = [torch.from_numpy(rng.randn(2, 300).astype(f32)).cuda(), torch.from_numpy(rng.randn(2, 77).astype(f32)).cuda()]
    winner, depth, amap, vis, pix, stats = flownet.render_maps([ta, tc], cam, [size, (5, 9)], attrs=attrs, footprint=1, rel_tol=0.02)
    for k, (w, n, s) in enumerate(((wa, 300, size), (wc, 77, (5, 9)))):
        assert tuple(winner[k].shape) == s and np.array_equal(winner[k].cpu().numpy().reshape(-1), w['winner'])
        assert FO.same_bits(depth[k].cpu().numpy().reshape(-1), w['depth']) and tuple(amap[k].shape) == (2,) + s
        want_map = RO.render_maps(a if k == 0 else c, cam, *s, attrs[k].cpu().numpy(), footprint=1)['attr_map']
        assert FO.same_bits(amap[k].cpu().numpy().reshape(2, -1), want_map)
        assert np.array_equal(vis[k].cpu().numpy(), w['visible'] == 1) and np.array_equal(pix[k].cpu().numpy(), w['pixel_of'])
        assert stats[k] == w['stats'].tolist()


def test_visibility_of_a_wall_behind_a_wall():
    rng = np.random.RandomState(41)
    H, W = 40, 90
    pc, is_front = RO.two_walls(rng, H, W, per_pixel=2.0)
    vis = flownet.visibility(torch.from_numpy(np.ascontiguousarray(pc.T)).cuda(), RO.KITTI_CAMERA, (H, W)).cpu().numpy()
    want = RO.render_maps(pc, RO.KITTI_CAMERA, H, W, footprint=1, rel_tol=0.02)['visible'] == 1
    assert vis[is_front].all()                                # nothing is in front of the front wall
    assert np.array_equal(vis[~is_front], want[~is_front])
    hidden = ~vis[~is_front]
    assert 0.5 < hidden.mean() < 0.75                         # the front wall covers two thirds of the image


# ----------------------------------------------------------------------------- end to end
def test_engine_writes_kitti_maps(tmp_path):
    from hplflownet_amd import engine
    rng = np.random.RandomState(50)
    raw, calib, out = str(tmp_path / 'kraw'), str(tmp_path / 'calib'), str(tmp_path / 'maps')
    kframes = [FO.kitti_raw(rng, 36 + k, 120 + 7 * k, p_valid=0.9, lo=3200) for k in range(3)]
    FO.write_kitti_tree(raw, calib, kframes, FO.CALIB_NAMES)
    common = ['--evaluate', '--dataset', 'KITTI', '--raw-root', raw, '--kitti-calib', calib, '--batch-size', '2', '--ragged',
              '--points', '8192', '--arch', 'HPLFlowNetShallow']
    res = engine.main(common + ['--write-kitti', out, '--write-footprint', '1'])
    assert res and all(np.isfinite(v) for v in res.values()) and 'EPE2D' in res, res
    for k, nm in enumerate(FO.CALIB_NAMES):
        shape = kframes[k][0].shape
        d0, d1, fl = (data.read_png(os.path.join(out, sub, nm + '_10.png')) for sub in ('disp_0', 'disp_1', 'flow'))
        assert d0.dtype == d1.dtype == fl.dtype == np.uint16 and d0.shape == d1.shape == shape and fl.shape == shape + (3,)
        assert d0.any() and set(np.unique(fl[..., 2]).tolist()) <= {0, 1} and ((fl[..., 2] == 1) <= (d0 > 0)).all()
    # fed with the ground-truth flow, the frames' own maps come back
    frames = [fr + (FO.read_P(nm),) for fr, nm in zip(kframes, FO.CALIB_NAMES)]
    pc1, pc2, _, _ = flownet.frames_from_kitti(frames)
    maps = flownet.flow_to_kitti_maps(pc1, [b - a for a, b in zip(pc1, pc2)], [fr[3] for fr in frames], [fr[0].shape for fr in frames])
    for fr, (d0, d1, fl) in zip(frames, maps):
        e0, e1, ef = RO.expected_raw(*fr[:3])
        assert np.array_equal(d0, e0) and np.array_equal(d1, e1) and np.array_equal(fl, ef)
        p = str(tmp_path / 'back.png')
        data.write_png(p, fl)
        assert np.array_equal(data.read_png(p), ef)
