"""CPU: the declaration, export and refusals of hpl_render_maps / hpl_maps_to_kitti and their workspace query (no device
needed), the numpy restatement tests/render_oracle.py on hand-computed cases, data.write_png against data.read_png and Pillow,
and the round-trip condition of DESIGN.md §34: a KITTI frame back-projected by the restatement of hpl_frames_from_kitti comes
back from the restatement of hpl_maps_to_kitti as its raw maps, exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

from common import ROOT
from hplflownet_amd import _lib, data
import frames_oracle as FO
import render_oracle as RO

I64, I32, F32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_float
f32 = np.float32
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('hpl_render_maps', 'int'), ('hpl_maps_to_kitti', 'int'), ('hpl_render_workspace_bytes', 'int64_t')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), body)
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    from hplflownet_amd import build
    assert 'render.hip' in build.SOURCES
    import hplflownet_amd
    for name in ('render_maps', 'visibility', 'flow_to_kitti_maps'):
        assert getattr(hplflownet_amd, name) is getattr(hplflownet_amd.flownet, name)


# ----------------------------------------------------------------------------- refusals without a device
CAM_OK = (-721.5, 609.5, 172.8, 44.8, 0.2, 0.0027)
P_OK = (721.5, 0, 609.5, 44.8, 0, 721.5, 172.8, 0.2, 0, 0, 1, 0.0027)
SHAPES = dict(batch=1, prefix=(0, 50), height=(10,), width=(10,), pprefix=(0, 100), footprint=0, ws=0x700000, ws_bytes=1 << 20)
MAPS_BASE = dict(SHAPES, pc=0x100000, pc_ld=50, attr=0x110000, attr_ld=50, channels=2, camera=CAM_OK, rel_tol=0.0, abs_tol=0.0,
                 near=1e-3, pixel_of=0x200000, winner=0x210000, depth=0x220000, attr_map=0x230000, attr_map_ld=100,
                 visible=0x240000, stats=0x250000)
KITTI_BASE = dict(SHAPES, pc1=0x100000, ld1=50, pc2=0x110000, ld2=50, P=P_OK, baseline=0.54, disp1=0x200000, disp2=0x210000,
                  flow=0x220000)


def _arr(ctype, values):
    return None if values is None else (ctype * len(values))(*values)


def call_maps(**kw):
    a = dict(MAPS_BASE, **kw)
    return _lib.load().hpl_render_maps(a['pc'], a['pc_ld'], a['attr'], a['attr_ld'], a['channels'], a['batch'], _arr(I64, a['prefix']),
                                       _arr(F32, a['camera']), _arr(I32, a['height']), _arr(I32, a['width']), _arr(I64, a['pprefix']),
                                       a['footprint'], a['rel_tol'], a['abs_tol'], a['near'], a['pixel_of'], a['winner'], a['depth'],
                                       a['attr_map'], a['attr_map_ld'], a['visible'], a['stats'], a['ws'], a['ws_bytes'], None)


def call_kitti(**kw):
    a = dict(KITTI_BASE, **kw)
    return _lib.load().hpl_maps_to_kitti(a['pc1'], a['ld1'], a['pc2'], a['ld2'], a['batch'], _arr(I64, a['prefix']),
                                         _arr(I32, a['height']), _arr(I32, a['width']), _arr(I64, a['pprefix']), _arr(F32, a['P']),
                                         a['baseline'], a['footprint'], a['disp1'], a['disp2'], a['flow'], a['ws'], a['ws_bytes'], None)


BIG = (2 ** 31 + 2) // 3
INF, NAN = float('inf'), float('nan')
COMMON_REFUSALS = [
    dict(batch=0), dict(batch=65), dict(batch=-1),
    dict(prefix=None), dict(height=None), dict(width=None), dict(pprefix=None), dict(ws=None),
    dict(prefix=(1, 51)), dict(batch=2, prefix=(0, 60, 50), height=(10, 0), width=(10, 0), pprefix=(0, 100, 100)),
    dict(height=(-10,), width=(-10,)), dict(height=(-1,), width=(-100,)),
    dict(pprefix=(1, 101)), dict(pprefix=(0, 99)), dict(pprefix=(0, 101)), dict(width=(11,)),
    dict(batch=2, prefix=(0, 50, 50), height=(10, 0), width=(10, 5), pprefix=(0, 100, 90)),
    dict(batch=2, prefix=(0, 50, 50), height=(5, 10), width=(10, 5), pprefix=(0, 60, 100)),
    dict(footprint=-1), dict(footprint=5),
    dict(ws=0x700080), dict(ws_bytes=0), dict(ws_bytes=799), dict(ws_bytes=1023),
    dict(height=(1,), width=(BIG,), pprefix=(0, BIG), ws_bytes=1 << 40, attr_map_ld=1 << 31),
    dict(height=(2 ** 31 - 1,), width=(2 ** 31 - 1,), pprefix=(0, (2 ** 31 - 1) ** 2), ws_bytes=1 << 62, attr_map_ld=1 << 39),
]
MAPS_REFUSALS = COMMON_REFUSALS + [
    dict(pc=None), dict(camera=None), dict(pixel_of=None), dict(winner=None), dict(depth=None), dict(visible=None), dict(stats=None),
    dict(attr=None), dict(channels=-1), dict(channels=9),
    dict(prefix=(0, BIG), pc_ld=BIG, attr_ld=BIG),
    dict(pc_ld=49), dict(attr_ld=49), dict(attr_map_ld=99), dict(pc_ld=(1 << 40) + 1), dict(attr_ld=1 << 62), dict(attr_map_ld=1 << 41),
    dict(pc=0x100002), dict(attr=0x110001), dict(pixel_of=0x200002), dict(winner=0x210001), dict(depth=0x220003),
    dict(attr_map=0x230002), dict(stats=0x250002),
    dict(camera=(0.0,) + CAM_OK[1:]), dict(camera=(INF,) + CAM_OK[1:]), dict(camera=(NAN,) + CAM_OK[1:]),
    dict(batch=2, prefix=(0, 20, 50), height=(5, 10), width=(10, 5), pprefix=(0, 50, 100), camera=CAM_OK + (0.0,) + CAM_OK[1:]),
    dict(rel_tol=-1e-6), dict(rel_tol=INF), dict(rel_tol=NAN), dict(abs_tol=-1.0), dict(abs_tol=INF), dict(abs_tol=NAN),
    dict(near=0.0), dict(near=-1.0), dict(near=INF), dict(near=NAN),
    # an output on an input, on another output, on the workspace (the last element of one on the first of the other included)
    dict(pixel_of=0x100000), dict(winner=0x100000 + 4 * 149), dict(depth=0x110000 + 4 * 99), dict(visible=0x100000 + 4),
    dict(stats=0x110000), dict(attr_map=0x100000), dict(attr_map=0x110000 - 4 * 199), dict(pc=0x230000 + 4 * 199),
    dict(ws=0x100000, pc=0x100100), dict(winner=0x200000 + 4 * 49), dict(depth=0x210000 + 4 * 99), dict(visible=0x220000 + 4 * 99),
    dict(stats=0x240000 + 48), dict(attr_map=0x250000 + 12), dict(ws=0x230000 + 256), dict(pixel_of=0x700000 + 796),
]
KITTI_REFUSALS = COMMON_REFUSALS + [
    dict(pc1=None), dict(pc2=None), dict(P=None), dict(disp1=None), dict(disp2=None), dict(flow=None),
    dict(prefix=(0, BIG), ld1=BIG, ld2=BIG),
    dict(ld1=49), dict(ld2=49), dict(ld1=(1 << 40) + 1), dict(ld2=1 << 62),
    dict(pc1=0x100002), dict(pc2=0x110001), dict(disp1=0x200001), dict(disp2=0x210001), dict(flow=0x220001),
    dict(P=P_OK[:1] + (1e-3,) + P_OK[2:]), dict(P=P_OK[:4] + (0.5,) + P_OK[5:]), dict(P=P_OK[:8] + (0.1,) + P_OK[9:]),
    dict(P=P_OK[:9] + (0.1,) + P_OK[10:]), dict(P=P_OK[:5] + (700.0,) + P_OK[6:]),
    dict(P=(0.0,) + P_OK[1:5] + (0.0,) + P_OK[6:]), dict(P=(INF,) + P_OK[1:5] + (INF,) + P_OK[6:]),
    dict(P=(NAN,) + P_OK[1:5] + (NAN,) + P_OK[6:]), dict(baseline=NAN), dict(baseline=INF),
    dict(batch=2, prefix=(0, 20, 50), height=(5, 10), width=(10, 5), pprefix=(0, 50, 100), P=P_OK + P_OK[:1] + (2.0,) + P_OK[2:]),
    dict(disp1=0x100000), dict(disp2=0x110000 + 4 * 149), dict(flow=0x100000 + 8), dict(pc2=0x220000 + 596),
    dict(disp2=0x200000 + 198), dict(flow=0x210000 + 198), dict(ws=0x220000 + 512), dict(disp1=0x700000 + 798),
]


@pytest.mark.parametrize('kw', MAPS_REFUSALS, ids=lambda kw: ','.join(kw))
def test_render_maps_refusals_without_a_device(kw):
    assert call_maps(**kw) == -1                              # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_render_maps')


@pytest.mark.parametrize('kw', KITTI_REFUSALS, ids=lambda kw: ','.join(kw))
def test_maps_to_kitti_refusals_without_a_device(kw):
    assert call_kitti(**kw) == -1
    assert _lib.load().hpl_last_error().startswith(b'hpl_maps_to_kitti')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 with M = 0 returns HPL_OK before any launch (maps_to_kitti: M = 0 alone): arrays that only touch, no channels and
    no attribute arrays, 64 empty frames."""
    empty = dict(prefix=(0, 0), height=(0,), width=(7,), pprefix=(0, 0))
    assert call_maps(pc_ld=0, attr_ld=0, attr_map_ld=0, **empty) == 0
    assert call_maps(pc_ld=0, channels=0, attr=None, attr_map=None, attr_map_ld=0, ws_bytes=0, **empty) == 0
    assert call_kitti(ld1=0, ld2=0, ws_bytes=0, **empty) == 0
    assert call_kitti(prefix=(0, 50), height=(0,), width=(7,), pprefix=(0, 0)) == 0        # points, but no pixel
    assert call_kitti(disp1=0x200002, disp2=0x210006, flow=0x220002, ld1=0, ld2=0, **empty) == 0
    many = dict(batch=64, prefix=(0,) * 65, height=(0,) * 64, width=tuple(range(64)), pprefix=(0,) * 65)
    assert call_maps(camera=CAM_OK * 64, pc_ld=0, attr_ld=0, attr_map_ld=0, **many) == 0
    assert call_kitti(P=P_OK * 64, ld1=0, ld2=0, **many) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_render_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(-1, 10) == -1
    assert f(1, -1) == -1 and f(1, BIG) == -1 and f(1, 2 ** 40) == -1
    assert f(1, BIG - 1) >= 8 * (BIG - 1) and f(64, 0) == 0
    ms = [0, 1, 31, 32, 33, 1025, 4847, 465750, 16 * 465750, 2 ** 29]
    for b in (1, 2, 64):
        vals = [f(b, m) for m in ms]
        assert all(v % 256 == 0 and 8 * m <= v < 8 * m + 256 for v, m in zip(vals, ms)) and vals == sorted(vals)


# ----------------------------------------------------------------------------- the restatement on hand-computed cases
def test_projection_is_exact_for_the_exact_camera():
    pc = RO.exact_points([0.5, 1.5, 2.5, -0.5, 3.0], [0.0, 0.5, 1.5, 2.0, -0.5])
    zc, u, v = RO.project(pc, RO.EXACT_CAMERA)
    assert zc.tolist() == [2.0] * 5 and u.tolist() == [0.5, 1.5, 2.5, -0.5, 3.0] and v.tolist() == [0.0, 0.5, 1.5, 2.0, -0.5]


def test_half_pixel_ties_go_to_even_and_borders():
    # u = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; -0.5 -> -0.0 (inside); 3.5 -> 4 = W: outside; 3.4999 inside; just below -0.5: outside
    us = [0.5, 1.5, 2.5, -0.5, 3.5, 3.25, float(np.nextafter(f32(-0.5), f32(-1)))]
    r = RO.render_maps(RO.exact_points(us, [1.0] * len(us)), RO.EXACT_CAMERA, 3, 4)
    assert r['pixel_of'].tolist() == [4, 6, 6, 4, -1, 7, -1]
    assert r['winner'].tolist() == [-1] * 4 + [0, -1, 1, 5] + [-1] * 4         # equal depths: the smaller index wins
    assert r['stats'].tolist() == [5, 3, 5, 0]                                  # every inside point is as near as its pixel's winner
    vs = [0.5, 1.5, 2.5, -0.5, float(np.nextafter(f32(-0.5), f32(-1)))]
    r = RO.render_maps(RO.exact_points([1.0] * len(vs), vs), RO.EXACT_CAMERA, 3, 4)
    assert r['pixel_of'].tolist() == [1, 9, 9, 1, -1]


def test_nearest_wins_and_tolerances():
    near_pt, far_pt = RO.exact_points([1.0], [1.0], 2.0), RO.exact_points([1.0], [1.0], 4.0)
    pc = np.concatenate([far_pt, near_pt, RO.exact_points([2.0], [0.0], 8.0)])
    attrs = np.array([[10.0, 20.0, 30.0]], f32)
    r = RO.render_maps(pc, RO.EXACT_CAMERA, 2, 3, attrs)
    assert r['pixel_of'].tolist() == [4, 4, 2] and r['winner'].tolist() == [-1, -1, 2, -1, 1, -1]
    assert r['depth'].tolist() == [0, 0, 8, 0, 2, 0] and r['attr_map'].tolist() == [[0, 0, 30, 0, 20, 0]]
    assert r['visible'].tolist() == [0, 1, 1] and r['stats'].tolist() == [3, 2, 2, 0]
    assert RO.render_maps(pc, RO.EXACT_CAMERA, 2, 3, rel_tol=1.0)['visible'].tolist() == [1, 1, 1]     # 4 <= 2 * (1 + 1)
    assert RO.render_maps(pc, RO.EXACT_CAMERA, 2, 3, rel_tol=0.99)['visible'].tolist() == [0, 1, 1]
    assert RO.render_maps(pc, RO.EXACT_CAMERA, 2, 3, abs_tol=2.0)['visible'].tolist() == [1, 1, 1]
    assert RO.render_maps(pc, RO.EXACT_CAMERA, 2, 3, abs_tol=1.99)['visible'].tolist() == [0, 1, 1]


def test_footprint_is_clipped_and_hides():
    # a near point at the corner (0, 0) with footprint 1 covers 4 pixels; a far point at (1, 1) loses its own pixel to it
    pc = np.concatenate([RO.exact_points([1.0], [1.0], 4.0), RO.exact_points([0.0], [0.0], 2.0)])
    r = RO.render_maps(pc, RO.EXACT_CAMERA, 3, 3, footprint=1)
    assert r['winner'].tolist() == [1, 1, 0, 1, 1, 0, 0, 0, 0] and r['visible'].tolist() == [0, 1]
    assert r['stats'].tolist() == [2, 9, 1, 0]
    r0 = RO.render_maps(pc, RO.EXACT_CAMERA, 3, 3, footprint=0)
    assert r0['winner'].tolist() == [1, -1, -1, -1, 0, -1, -1, -1, -1] and r0['visible'].tolist() == [1, 1]
    r4 = RO.render_maps(pc[1:], RO.EXACT_CAMERA, 7, 6, footprint=4)
    assert (r4['winner'].reshape(7, 6) == 0).sum() == 25 and (r4['winner'].reshape(7, 6)[:5, :5] == 0).all()


def test_points_that_must_not_project():
    near = f32(1e-3)
    zs = [near, np.nextafter(near, f32(0)), f32(0), f32(-2)]
    pc = np.stack([np.zeros(4, f32), np.zeros(4, f32), np.array(zs, f32)], axis=1)
    bad = np.array([[np.inf, 0, 2], [0, -np.inf, 2], [0, 0, np.inf], [np.nan, 0, 2], [0, np.nan, 2], [0, 0, np.nan],
                    [3e38, 0, 2], [-3e38, 0, 2], [4e9, 0, 2], [0, 3e9, 2]], f32)
    r = RO.render_maps(np.concatenate([pc, bad]), RO.EXACT_CAMERA, 5, 5)
    assert r['pixel_of'].tolist() == [0] + [-1] * 13             # zc == near projects; u = +-inf or >= 2^31 is outside
    assert r['stats'].tolist() == [1, 1, 1, 3 + 6]              # below near, 0, negative; the six non-finite points
    assert r['winner'].tolist() == [0] + [-1] * 24


def test_empty_cloud_and_empty_image():
    r = RO.render_maps(np.zeros((0, 3), f32), RO.EXACT_CAMERA, 2, 2, np.zeros((3, 0), f32))
    assert r['winner'].tolist() == [-1] * 4 and r['attr_map'].shape == (3, 4) and r['stats'].tolist() == [0, 0, 0, 0]
    r = RO.render_maps(RO.exact_points([0.0], [0.0]), RO.EXACT_CAMERA, 0, 5)
    assert r['pixel_of'].tolist() == [-1] and r['visible'].tolist() == [0] and r['stats'].tolist() == [0, 0, 0, 0]


def test_maps_to_kitti_by_hand():
    """P00 = 256, baseline 1, no offsets: fb = 256, a point at Z has disparity 256 / Z and raw value 65536 / Z (less the 1e-5)."""
    P = np.array([256, 0, 0, 0, 0, 256, 0, 0, 0, 0, 1, 0], f32).reshape(3, 4)
    # camera f = -256: u = -256 X / Z.  pc1 at pixel (1, 2) with Z = 4: X = -2 * 4 / 256, Y = -1 * 4 / 256
    pc1 = np.array([[-2 * 4 / 256.0, -1 * 4 / 256.0, 4.0], [-2 * 8 / 256.0, -1 * 8 / 256.0, 8.0]], f32)
    pc2 = np.array([[-3.5 * 2 / 256.0, -0.75 * 2 / 256.0, 2.0], [0, 0, 1.0]], f32)
    d1, d2, fl = RO.maps_to_kitti(pc1, pc2, P, 3, 4, baseline=1.0)
    e1, e2, ef = np.zeros((3, 4), np.uint16), np.zeros((3, 4), np.uint16), np.zeros((3, 4, 3), np.uint16)
    e1[1, 2], e2[1, 2], ef[1, 2] = 16384, 32768, (32768 + 96, 32768 - 16, 1)       # 65536 / 4, 65536 / 2, 1.5 px, -0.25 px
    assert np.array_equal(d1, e1) and np.array_equal(d2, e2) and np.array_equal(fl, ef)
    pc2[0, 2] = -1.0                                                               # the partner is behind the camera
    d1, d2, fl = RO.maps_to_kitti(pc1, pc2, P, 3, 4, baseline=1.0)
    assert d1[1, 2] == 16384 and not d2.any() and not fl.any()
    d1, _, _ = RO.maps_to_kitti(np.array([[0, 0, 1e-2]], f32), np.array([[0, 0, 1e9]], f32), P, 1, 1, baseline=1.0)
    assert d1[0, 0] == 65535                                                       # clamped


# ----------------------------------------------------------------------------- write_png
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('channels', [1, 3])
def test_write_png_round_trips(tmp_path, dtype, channels):
    rng = np.random.RandomState(3 + channels)
    for shape in ((1, 1), (9, 13), (5, 1), (1, 7), (37, 131)):
        full = shape + ((3,) if channels == 3 else ())
        for arr in (rng.randint(0, np.iinfo(dtype).max + 1, size=full).astype(dtype), np.zeros(full, dtype),
                    np.full(full, np.iinfo(dtype).max, dtype)):
            p = str(tmp_path / 'x.png')
            data.write_png(p, arr)
            got = data.read_png(p)
            assert got.dtype == dtype and got.shape == full and np.array_equal(got, arr), shape
    with pytest.raises(ValueError):
        data.write_png(str(tmp_path / 'y.png'), np.zeros((3, 3), np.int32))
    with pytest.raises(ValueError):
        data.write_png(str(tmp_path / 'y.png'), np.zeros((3, 3, 2), np.uint8))
    with pytest.raises(ValueError):
        data.write_png(str(tmp_path / 'y.png'), np.zeros((0, 3), np.uint8))


def test_write_png_is_read_by_pillow(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(5)
    arr = rng.randint(0, 65536, size=(21, 34)).astype(np.uint16)
    p = str(tmp_path / 'grey16.png')
    data.write_png(p, arr)
    with Image.open(p) as im:
        assert im.size == (34, 21) and np.array_equal(np.asarray(im).astype(np.uint16), arr)
    rgb = rng.randint(0, 256, size=(5, 9, 3)).astype(np.uint8)
    data.write_png(p, rgb)
    with Image.open(p) as im:
        assert np.array_equal(np.asarray(im), rgb)


# ----------------------------------------------------------------------------- the round-trip condition
def round_trip_frames():
    """(name, disp1, disp2, flow, P): the KITTI frames of the golden fixture and fuzzed frames over the three calibrations --
    disparities over the generator's whole range 1 .. 39999 raw units (0.004 .. 156 px) and the extreme values 1 and 65535."""
    frames = [('golden%d' % k, GOLD['kitti%d_disp1' % k], GOLD['kitti%d_disp2' % k], GOLD['kitti%d_flow' % k],
               FO.read_P(str(GOLD['kitti%d_calib' % k]))) for k in range(3)]
    rng = np.random.RandomState(34)
    for k, (H, W, lo, extreme) in enumerate([(37, 131, 256, False), (3, 1300, 1, False), (1, 1, 256, False), (19, 50, 256, True),
                                              (48, 97, 16, False), (2, 1242, 256, False)]):
        nm = FO.CALIB_NAMES[k % 3]
        frames.append(('fuzz%d_%s' % (k, nm),) + FO.kitti_raw(rng, H, W, p_valid=1.0 if H * W == 1 else 0.7, extreme=extreme, lo=lo) +
                      (FO.read_P(nm),))
    return frames


ROUND_TRIP = round_trip_frames()


@pytest.mark.parametrize('frame', ROUND_TRIP, ids=[f[0] for f in ROUND_TRIP])
def test_round_trip_condition(frame):
    _, d1, d2, fl, P = frame
    assert P[0, 3] != 0 and P[2, 3] != 0
    H, W = d1.shape
    pc1, pc2, pixel = FO.kitti_frame(d1, d2, fl, P)
    r1, r2, rf = RO.maps_to_kitti(pc1, pc2, P, H, W, footprint=0)
    e1, e2, ef = RO.expected_raw(d1, d2, fl)
    assert len(pixel) == int(RO.valid_kitti(d1, d2, fl).sum())
    assert np.array_equal(r1, e1) and np.array_equal(r2, e2) and np.array_equal(rf, ef)
