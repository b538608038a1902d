"""CPU: the numpy restatement tests/frames_oracle.py against the reference's outputs (tests/golden/frames.npz), the declaration,
export and refusals of hpl_frames_from_kitti / hpl_frames_from_ft3d (no device needed), the workspace size, hpl_png_unfilter
through data.read_png against a writer that forces every row filter, read_pfm, read_flo, and the raw readers' file listing and
error messages."""
import ctypes
import os
import re

import numpy as np
import pytest

from common import ROOT
from hplflownet_amd import _lib, data
import frames_oracle as FO

I64, I32, F32 = ctypes.c_int64, ctypes.c_int32, ctypes.c_float
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))
FT3D_KEYS = ('disp', 'dchange', 'flow', 'occ1', 'occ2')


def test_header_declares_and_library_exports():
    hdr = open(os.path.join(ROOT, 'include', 'hpl_bcl.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, ret in (('hpl_frames_from_kitti', 'int'), ('hpl_frames_from_ft3d', 'int'), ('hpl_frames_workspace_bytes', 'int64_t'),
                      ('hpl_png_unfilter', 'int')):
        assert re.search(r'\b%s\s+%s\s*\(' % (ret, name), body)
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    from hplflownet_amd import build
    assert 'frames.hip' in build.SOURCES
    import hplflownet_amd
    assert hplflownet_amd.frames_from_kitti is hplflownet_amd.flownet.frames_from_kitti
    assert hplflownet_amd.frames_from_ft3d is hplflownet_amd.flownet.frames_from_ft3d


# ----------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize('k', range(3))
def test_kitti_restatement_equals_the_reference(k):
    P = FO.read_P(str(GOLD['kitti%d_calib' % k]))
    assert P[0, 3] != 0 and P[2, 3] != 0
    pc1, pc2, pixel = FO.kitti_frame(GOLD['kitti%d_disp1' % k], GOLD['kitti%d_disp2' % k], GOLD['kitti%d_flow' % k], P)
    assert len(pixel) > 0 and np.all(np.diff(pixel) > 0)
    assert FO.same_bits(pc1, GOLD['kitti%d_pc1' % k]) and FO.same_bits(pc2, GOLD['kitti%d_pc2' % k])


@pytest.mark.parametrize('k', range(2))
@pytest.mark.parametrize('tag,near', [('all', None), ('near', -35.0)])
def test_ft3d_restatement_equals_the_reference(k, tag, near):
    frame = [GOLD['ft3d%d_%s' % (k, key)] for key in FT3D_KEYS]
    pc1, pc2, pixel = FO.ft3d_frame(*frame, near=near)
    assert len(pixel) > 0 and np.all(np.diff(pixel) > 0)
    assert FO.same_bits(pc1, GOLD['ft3d%d_%s_pc1' % (k, tag)]) and FO.same_bits(pc2, GOLD['ft3d%d_%s_pc2' % (k, tag)])
    if k == 0 and near is None:              # the fixture does hold the IEEE cases
        assert np.isnan(GOLD['ft3d0_all_pc1']).any() and np.isinf(GOLD['ft3d0_all_pc2']).any()
    if near is not None:
        assert not np.isnan(pc1[:, 2]).any() and not np.isnan(pc2[:, 2]).any()


def test_same_bits_is_strict():
    a = np.array([0.0, 1.0, np.nan], np.float32)
    assert FO.same_bits(a, a.copy())
    assert not FO.same_bits(a, np.array([-0.0, 1.0, np.nan], np.float32))
    assert not FO.same_bits(a, np.array([0.0, 1.0, 2.0], np.float32))
    assert not FO.same_bits(a, np.array([0.0, np.nextafter(np.float32(1), np.float32(2)), np.nan], np.float32))


def test_packed_layout():
    r = [(np.ones((2, 3), np.float32), 2 * np.ones((2, 3), np.float32), np.array([1, 4], np.int32)),
         (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32))]
    o1, o2, px, n = FO.packed(r, [6, 2])
    assert n.tolist() == [2, 0] and px.tolist() == [1, 4, -1, -1, -1, -1, -1, -1]
    assert o1[:, :2].min() == 1 and o2[:, :2].min() == 2 and not o1[:, 2:].any() and not o2[:, 2:].any()


# ----------------------------------------------------------------------------- refusals without a device
P_OK = (721.5, 0, 609.5, 44.8, 0, 721.5, 172.8, 0.2, 0, 0, 1, 0.0027)
BASE = dict(batch=1, height=(10,), width=(10,), prefix=(0, 100), out1=0x300000, ld1=100, out2=0x400000, ld2=100, pixel=0x500000,
            counts=0x600000, ws=0x700000, ws_bytes=1 << 20)
KITTI_BASE = dict(BASE, disp1=0x100000, disp2=0x110000, flow=0x120000, P=P_OK, baseline=0.54)
FT3D_BASE = dict(BASE, disp=0x100000, dchange=0x110000, flow=0x120000, occ1=0x130000, occ2=0x140000, f=-1050.0, cx=479.5, cy=269.5,
                 use_near=1, near=-35.0)


def _arr(ctype, values):
    return None if values is None else (ctype * len(values))(*values)


def call_kitti(**kw):
    a = dict(KITTI_BASE, **kw)
    return _lib.load().hpl_frames_from_kitti(a['disp1'], a['disp2'], a['flow'], a['batch'], _arr(I32, a['height']), _arr(I32, a['width']),
                                             _arr(I64, a['prefix']), _arr(F32, a['P']), a['baseline'], a['out1'], a['ld1'], a['out2'],
                                             a['ld2'], a['pixel'], a['counts'], a['ws'], a['ws_bytes'], None)


def call_ft3d(**kw):
    a = dict(FT3D_BASE, **kw)
    return _lib.load().hpl_frames_from_ft3d(a['disp'], a['dchange'], a['flow'], a['occ1'], a['occ2'], a['batch'], _arr(I32, a['height']),
                                            _arr(I32, a['width']), _arr(I64, a['prefix']), a['f'], a['cx'], a['cy'], a['use_near'],
                                            a['near'], a['out1'], a['ld1'], a['out2'], a['ld2'], a['pixel'], a['counts'], a['ws'],
                                            a['ws_bytes'], None)


BIG = (2 ** 31 + 2) // 3
COMMON_REFUSALS = [
    dict(batch=0), dict(batch=65), dict(batch=-1),
    dict(height=None), dict(width=None), dict(prefix=None), dict(out1=None), dict(out2=None), dict(counts=None), dict(ws=None),
    dict(flow=None),
    dict(height=(-1,), width=(-100,)), dict(width=(-10,), height=(-10,)),
    dict(prefix=(1, 101)), dict(prefix=(0, 99)), dict(prefix=(0, 101)), dict(height=(10,), width=(11,)),
    dict(batch=2, height=(10, 0), width=(10, 5), prefix=(0, 100, 90)),
    dict(batch=2, height=(5, 10), width=(10, 5), prefix=(0, 60, 100)),
    dict(ld1=99), dict(ld2=99),
    dict(out1=0x300002), dict(out2=0x400001), dict(pixel=0x500002), dict(counts=0x600003), dict(ws=0x700002),
    dict(ws_bytes=0), dict(ws_bytes=255),
    dict(height=(1,), width=(BIG,), prefix=(0, BIG), ld1=1 << 31, ld2=1 << 31, ws_bytes=1 << 40),
    dict(height=(2 ** 31 - 1,), width=(2 ** 31 - 1,), prefix=(0, (2 ** 31 - 1) ** 2), ld1=1 << 62, ld2=1 << 62, ws_bytes=1 << 62),
    dict(out1=0x120000), dict(out2=0x120000 + 4), dict(pixel=0x120000), dict(counts=0x120000),
    dict(out1=0x120000 - 4 * 299), dict(flow=0x300000 + 4 * 299),
    dict(ld1=1 << 62), dict(ld2=(1 << 40) + 1),                                   # (with a valid N: the extents must not overflow)
    dict(out2=0x300000), dict(out2=0x300000 + 4 * 299), dict(pixel=0x300000 + 4 * 150), dict(counts=0x400000 + 4 * 299),
    dict(counts=0x500000 + 4 * 99), dict(ws=0x300000 + 4 * 200), dict(ws=0x600000),
]
KITTI_REFUSALS = COMMON_REFUSALS + [
    dict(disp1=None), dict(disp2=None), dict(P=None),
    dict(disp1=0x100001), dict(disp2=0x110001), dict(flow=0x120001),
    dict(out1=0x100000 + 196), dict(out2=0x110000), dict(disp1=0x500000 + 396),
    dict(P=P_OK[:1] + (1e-3,) + P_OK[2:]), dict(P=P_OK[:4] + (0.5,) + P_OK[5:]), dict(P=P_OK[:8] + (0.1,) + P_OK[9:]),
    dict(P=P_OK[:9] + (0.1,) + P_OK[10:]), dict(P=P_OK[:5] + (700.0,) + P_OK[6:]),
    dict(P=(0.0,) + P_OK[1:5] + (0.0,) + P_OK[6:]), dict(P=(float('inf'),) + P_OK[1:5] + (float('inf'),) + P_OK[6:]),
    dict(P=(float('nan'),) + P_OK[1:5] + (float('nan'),) + P_OK[6:]), dict(baseline=float('nan')), dict(baseline=float('inf')),
    dict(batch=2, height=(5, 10), width=(10, 5), prefix=(0, 50, 100), P=P_OK + P_OK[:1] + (2.0,) + P_OK[2:]),
]
FT3D_REFUSALS = COMMON_REFUSALS + [
    dict(disp=None), dict(dchange=None), dict(occ1=None), dict(occ2=None),
    dict(disp=0x100002), dict(dchange=0x110001), dict(flow=0x120002),
    dict(out1=0x100000 + 396), dict(out2=0x110000), dict(pixel=0x130000 + 96), dict(counts=0x140000 + 99), dict(occ2=0x600000 + 3),
    dict(use_near=2), dict(use_near=-1), dict(near=float('nan')),
]


@pytest.mark.parametrize('kw', KITTI_REFUSALS, ids=lambda kw: ','.join(kw))
def test_kitti_refusals_without_a_device(kw):
    assert call_kitti(**kw) == -1                             # HPL_EINVAL
    assert _lib.load().hpl_last_error().startswith(b'hpl_frames_from_kitti')


@pytest.mark.parametrize('kw', FT3D_REFUSALS, ids=lambda kw: ','.join(kw))
def test_ft3d_refusals_without_a_device(kw):
    assert call_ft3d(**kw) == -1
    assert _lib.load().hpl_last_error().startswith(b'hpl_frames_from_ft3d')


def test_accepted_arguments_reach_no_launch_when_empty():
    """N = 0 returns HPL_OK before any launch; the misalignments that ARE allowed, arrays that only touch, a NULL pixel."""
    empty = dict(height=(0,), width=(7,), prefix=(0, 0), ld1=0, ld2=0)
    assert call_kitti(**empty) == 0 and call_ft3d(**empty) == 0
    assert call_kitti(pixel=None, disp1=0x100002, disp2=0x110006, flow=0x120002, **empty) == 0
    assert call_ft3d(pixel=None, occ1=0x130001, occ2=0x140003, use_near=0, near=float('nan'), **empty) == 0
    many = dict(batch=64, height=(0,) * 64, width=tuple(range(64)), prefix=(0,) * 65, ld1=0, ld2=0)
    assert call_kitti(P=P_OK * 64, **many) == 0 and call_ft3d(**many) == 0


def test_workspace_bytes():
    f = _lib.load().hpl_frames_workspace_bytes
    assert f(0, 10) == -1 and f(65, 10) == -1 and f(-1, 10) == -1
    assert f(1, -1) == -1 and f(1, BIG) == -1 and f(1, 2 ** 40) == -1
    assert f(1, BIG - 1) > 0 and f(64, 0) > 0
    ns = [0, 1, 3, 1023, 1024, 1025, 8192, 465750, 518400, 16 * 518400, 2 ** 29]
    for b in (1, 2, 16, 63):
        vals = [f(b, n) for n in ns]
        assert all(v > 0 and v % 256 == 0 for v in vals) and vals == sorted(vals)
        assert all(f(b + 1, n) >= f(b, n) for n in ns)
    assert f(16, 16 * 518400) < 1 << 16                       # four bytes per 1024 pixels


# ----------------------------------------------------------------------------- the PNG reader
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('channels', [1, 3])
def test_read_png_undoes_every_filter(tmp_path, dtype, channels):
    rng = np.random.RandomState(7 + channels)
    for shape in ((9, 13), (1, 1), (5, 1), (1, 6), (12, 40)):
        full = shape + ((3,) if channels == 3 else ())
        smooth = np.cumsum(rng.randint(0, 40, size=full), axis=1).astype(dtype)      # (filters matter on smooth rows)
        noisy = rng.randint(0, np.iinfo(dtype).max + 1, size=full).astype(dtype)
        for arr in (smooth, noisy):
            for filters in (0, 1, 2, 3, 4, FO.mixed_filters(shape[0]), FO.mixed_filters(shape[0], 3)):
                p = str(tmp_path / 'x.png')
                FO.write_png(p, arr, filters, idat_split=0 if isinstance(filters, int) else 50)
                got = data.read_png(p)
                assert got.dtype == dtype and got.shape == full and np.array_equal(got, arr), (shape, filters)


def test_forced_filters_reach_the_file():
    """The writer's rows do carry the filter asked for, and filtering changes the bytes (so the reader's inverse is exercised)."""
    raw = np.cumsum(np.ones((4, 24), np.int64), axis=1).astype(np.uint8)
    rows = [FO.png_filter_rows(raw, 3, [f] * 4) for f in range(5)]
    assert [int(r[1, 0]) for r in rows] == [0, 1, 2, 3, 4]
    assert all(not np.array_equal(rows[0][:, 1:], r[:, 1:]) for r in rows[1:])


def test_read_png_against_pillow(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.RandomState(3)
    arr = rng.randint(0, 65536, size=(17, 29)).astype(np.uint16)
    p = str(tmp_path / 'g16.png')
    FO.write_png(p, arr, FO.mixed_filters(17))
    assert np.array_equal(np.asarray(Image.open(p)).astype(np.uint16), arr)           # our writer, Pillow's reader
    q = str(tmp_path / 'pil16.png')
    Image.fromarray(arr).save(q)
    assert np.array_equal(data.read_png(q), arr)                                      # Pillow's writer, our reader
    rgb = rng.randint(0, 256, size=(11, 7, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(q)
    assert np.array_equal(data.read_png(q), rgb)


def test_read_png_refuses_what_it_does_not_read(tmp_path):
    arr = np.arange(12, dtype=np.uint8).reshape(3, 4)
    p = str(tmp_path / 'bad.png')
    for kw, word in ((dict(interlace=1), 'interlace'), (dict(colour=3), 'colour type 3'), (dict(colour=4), 'colour type 4'),
                     (dict(colour=6), 'colour type 6'), (dict(depth=4), '4 bits'), (dict(depth=1), '1 bits')):
        FO.write_png(p, arr, 0, **kw)
        with pytest.raises(ValueError, match=word):
            data.read_png(p)
    blob = FO.png_bytes(arr)
    for bad, word in ((b'JUNK' + blob[4:], 'not a PNG'), (blob[:-20], 'cut short|no IHDR'), (blob[:40] + b'\x00' + blob[41:], 'CRC')):
        with open(p, 'wb') as fd:
            fd.write(bad)
        with pytest.raises(ValueError, match=word):
            data.read_png(p)
    filtered = FO.png_filter_rows(arr, 1, [0, 0, 0])
    filtered[1, 0] = 5                                                                # a filter type that does not exist
    import struct
    import zlib
    body = b'\x89PNG\r\n\x1a\n' + FO._chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 3, 8, 0, 0, 0, 0)) + \
        FO._chunk(b'IDAT', zlib.compress(filtered.tobytes())) + FO._chunk(b'IEND', b'')
    with open(p, 'wb') as fd:
        fd.write(body)
    with pytest.raises(_lib.HplError, match='filter type 5'):
        data.read_png(p)


def test_png_unfilter_arguments():
    f = _lib.load().hpl_png_unfilter
    buf = (ctypes.c_uint8 * 8)(1, 1, 1, 1, 2, 1, 1, 1)
    assert f(buf, 2, 4, 1) == 0 and list(buf) == [1, 1, 2, 3, 2, 2, 3, 4]
    assert f(None, 0, 4, 1) == 0 and f(buf, 0, 1, 8) == 0
    for args in ((None, 1, 4, 1), (buf, -1, 4, 1), (buf, 2, 0, 1), (buf, 2, 4, 0), (buf, 2, 4, 9)):
        assert f(*args) == -1 and _lib.load().hpl_last_error().startswith(b'hpl_png_unfilter')


# ----------------------------------------------------------------------------- PFM and .flo
@pytest.mark.parametrize('little', [True, False])
def test_read_pfm_both_endiannesses(tmp_path, little):
    rng = np.random.RandomState(5)
    for shape in ((7, 11), (1, 1), (6, 5, 3)):
        arr = rng.randn(*shape).astype(np.float32)
        arr.flat[-1] = np.nan
        p = str(tmp_path / 'x.pfm')
        FO.write_pfm(p, arr, little=little, scale=2.5)
        got = data.read_pfm(p)
        assert got.dtype == np.float32 and got.flags['C_CONTIGUOUS'] and FO.same_bits(got, arr)
    raw = open(p, 'rb').read()
    assert np.frombuffer(raw[-4 * 15:], '<f4' if little else '>f4').tolist() == arr[0].reshape(-1).tolist()    # bottom row last


def test_read_pfm_and_flo_refuse_malformed_files(tmp_path):
    p = str(tmp_path / 'x.pfm')
    for blob, word in ((b'P5\n3 2\n-1.0\n' + bytes(24), 'not a PFM'), (b'Pf\n3x2\n-1.0\n' + bytes(24), 'malformed'),
                       (b'Pf\n3 2\nabc\n' + bytes(24), 'malformed'), (b'Pf\n3 2\n-1.0\n' + bytes(20), 'values')):
        with open(p, 'wb') as fd:
            fd.write(blob)
        with pytest.raises(ValueError, match=word):
            data.read_pfm(p)
    q = str(tmp_path / 'x.flo')
    import struct
    for blob, word in ((b'PIEX' + struct.pack('<ii', 2, 2) + bytes(32), 'PIEH'), (b'PIEH' + struct.pack('<ii', 2, 2) + bytes(31), 'bytes'),
                       (b'PIEH\x01', 'cut short')):
        with open(q, 'wb') as fd:
            fd.write(blob)
        with pytest.raises(ValueError, match=word):
            data.read_flo(q)


def test_read_flo(tmp_path):
    flow = np.random.RandomState(9).randn(5, 8, 2).astype(np.float32)
    p = str(tmp_path / 'x.flo')
    FO.write_flo(p, flow)
    got = data.read_flo(p)
    assert got.dtype == np.float32 and got.shape == (5, 8, 2) and FO.same_bits(got, flow)


# ----------------------------------------------------------------------------- the raw classes' listing and messages
def _kitti_tree(tmp_path, names=FO.CALIB_NAMES):
    rng = np.random.RandomState(11)
    raw, calib = str(tmp_path / 'raw'), str(tmp_path / 'calib')
    FO.write_kitti_tree(raw, calib, [FO.kitti_raw(rng, 4, 6) for _ in names], names)
    return raw, calib


def _ft3d_tree(tmp_path, names=('0000001', '0000002', '0000003', '0000004', '0000005')):
    rng = np.random.RandomState(12)
    raw = str(tmp_path / 'ftraw')
    for split in ('train', 'val'):
        FO.write_ft3d_tree(raw, split, [FO.ft3d_raw(rng, 3, 5) for _ in names], names)
    return raw


def test_raw_classes_refuse_a_host_device(tmp_path):
    raw, calib = _kitti_tree(tmp_path)
    with pytest.raises(_lib.HplError, match='no CPU fallback'):
        data.KITTIRaw(None, raw, calib, device='cpu')
    with pytest.raises(_lib.HplError, match='no CPU fallback'):
        data.FlyingThings3DRaw(False, None, _ft3d_tree(tmp_path), device='cpu')


def test_kitti_raw_listing_and_messages(tmp_path):
    raw, calib = _kitti_tree(tmp_path)
    ds = data.KITTIRaw(None, raw, calib)                      # (construction lists files; it touches no device)
    assert [os.path.basename(s) for s in ds.samples] == sorted(FO.CALIB_NAMES) and len(ds) == 3 and ds._found == 3
    assert ds.has_cameras and ds.camera_of(ds.samples[1]) == data.read_kitti_camera(os.path.join(calib, '000155.txt'))
    assert FO.same_bits(ds.P['000157'], FO.read_P('000157'))
    assert 'found 3 sample directories' in ds.check_counts()
    d1, d2, fl = data.read_kitti_raw_frame(raw, '000155')
    assert d1.dtype == np.uint16 and d1.shape == (4, 6) and fl.shape == (4, 6, 3)
    with pytest.raises(FileNotFoundError, match='calib_dir'):
        data.KITTIRaw(None, raw, None)
    with pytest.raises(FileNotFoundError, match='calib_dir'):
        data.KITTIRaw(None, raw, str(tmp_path / 'nowhere'))
    os.remove(os.path.join(calib, '000155.txt'))
    with pytest.raises(FileNotFoundError, match='000155.txt'):
        data.KITTIRaw(None, raw, calib)
    os.remove(os.path.join(raw, 'training', 'flow_occ', '000000_10.png'))
    with pytest.raises(FileNotFoundError, match='flow_occ.*000000_10.png'):
        data.KITTIRaw(None, raw, calib)
    with pytest.raises(FileNotFoundError, match='not a directory'):
        data.KITTIRaw(None, str(tmp_path / 'calib'), calib)
    with pytest.raises(_lib.HplError, match='remove_ground'):
        data.KITTIRaw(None, raw, calib, remove_ground='maybe')
    FO.write_png(os.path.join(raw, 'training', 'disp_occ_0', '000157_10.png'), np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError, match='16-bit greyscale'):
        data.read_kitti_raw_frame(raw, '000157')


def test_ft3d_raw_listing_and_messages(tmp_path):
    raw = _ft3d_tree(tmp_path)
    val = data.FlyingThings3DRaw(False, None, raw)
    assert [os.path.basename(s) for s in val.samples] == ['0000001', '0000005'] and val._found == 5 and val.near == -35.0
    assert val.root == os.path.join(raw, 'val') and val.has_cameras
    full = data.FlyingThings3DRaw(True, None, raw, near=None, full=True)
    assert len(full) == 5 and full.root == os.path.join(raw, 'train') and 'the published split has 19640' in full.check_counts()
    frame = data.read_ft3d_raw_frame(os.path.join(raw, 'val'), '0000002')
    assert [x.dtype for x in frame] == [np.float32, np.float32, np.float32, np.uint8, np.uint8]
    assert [x.shape for x in frame] == [(3, 5), (3, 5), (3, 5, 2), (3, 5), (3, 5)]
    os.remove(os.path.join(raw, 'val', 'flow', 'left', 'into_future', '0000003.flo'))
    with pytest.raises(FileNotFoundError, match='0000003.flo'):
        data.FlyingThings3DRaw(False, None, raw)
    with pytest.raises(FileNotFoundError, match='not a directory'):
        data.FlyingThings3DRaw(False, None, str(tmp_path / 'nowhere'))
    FO.write_png(os.path.join(raw, 'train', 'disparity_occlusions', 'left', '0000001.png'), np.zeros((3, 5, 3), np.uint8))
    with pytest.raises(ValueError, match='8-bit greyscale'):
        data.read_ft3d_raw_frame(os.path.join(raw, 'train'), '0000001')


def test_engine_raw_root_arguments(tmp_path, capsys):
    from hplflownet_amd import engine
    raw, calib = _kitti_tree(tmp_path)
    a = engine.parse_args(['--dataset', 'KITTI', '--raw-root', raw, '--kitti-calib', calib, '--evaluate'])
    assert a.raw_root == raw and a.data_root is None
    assert engine.parse_args(['--evaluate']).raw_root is None
    for argv in (['--dataset', 'KITTI', '--raw-root', raw, '--evaluate'],
                 ['--raw-root', raw, '--evaluate'],
                 ['--dataset', 'KITTI', '--raw-root', str(tmp_path / 'nowhere'), '--kitti-calib', calib, '--evaluate'],
                 ['--dataset', 'KITTI', '--raw-root', raw, '--data-root', raw, '--kitti-calib', calib, '--evaluate']):
        with pytest.raises(SystemExit):
            engine.parse_args(argv)
        assert '--raw-root' in capsys.readouterr().err


def test_wrappers_refuse_before_the_library():
    import torch
    from hplflownet_amd import flownet, ops
    z16, z3 = torch.zeros(6, dtype=torch.uint16), torch.zeros(6, 3, dtype=torch.uint16)
    with pytest.raises(_lib.HplError, match='device tensor'):
        ops.frames_from_kitti(z16, z16, z3, [P_OK], [2], [3])                 # host tensors: no CPU fallback
    with pytest.raises(_lib.HplError, match='device tensor'):
        ops.frames_from_ft3d(torch.zeros(6), torch.zeros(6), torch.zeros(6, 2), torch.zeros(6, dtype=torch.uint8),
                             torch.zeros(6, dtype=torch.uint8), [2], [3])
    for hw in (([2], [3, 4]), ([], []), ([-1], [3]), ([1] * 65, [1] * 65), (None, [3])):
        with pytest.raises(_lib.HplError, match='heights and widths'):
            ops.frames_from_kitti(z16, z16, z3, [P_OK], *hw)
    for frames in ([], 'x', [(np.zeros((2, 3), np.uint16),)], [(np.zeros(6, np.uint16),) * 4],
                   [(np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16), np.zeros((2, 3, 2), np.uint16), P_OK)],
                   [(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint16), np.zeros((2, 3, 3), np.uint16), P_OK)]):
        with pytest.raises(_lib.HplError, match='frames_from_kitti'):
            flownet.frames_from_kitti(frames)
