"""GPU: hpl_frames_from_kitti / hpl_frames_from_ft3d through ops, flownet, the raw readers, tools/preprocess.py and the engine
(DESIGN.md §25).  The device's outputs equal the reference's (tests/golden/frames.npz) and, on fuzzed frames, the numpy
restatement tests/frames_oracle.py: counts and pixel exactly, both clouds bit for bit (a NaN equals a NaN), the tails 0 / -1.
The arithmetic is float32 with one rounding per operation on both sides, so nothing here has a tolerance.  A workgroup takes
1024 pixels in quads that start at packed indices divisible by four: the shapes lie either side of a quad, a wave's 256 pixels
and a workgroup, and frames inside a batch start at every residue mod 4."""
import os
import sys

import numpy as np
import pytest
import torch

import frames_oracle as FO
from batch64 import counts64
from common import ROOT
from hplflownet_amd import _lib, data, flownet, ops

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))
P0 = FO.read_P('000000')
SHAPES = [(1, 1), (1, 3), (2, 63), (2, 65), (3, 131), (1, 1023), (1, 1024), (1, 1025), (37, 131), (3, 1300)]
KEYS = ('pc1', 'pc2', 'pixel', 'counts')


def dev(a, lead=0):
    """A host array on the device, flattened per pixel; lead > 0: behind `lead` elements of a wider buffer, so that it starts
    lead * itemsize bytes past an aligned address."""
    a = np.ascontiguousarray(a)
    if lead == 0:
        return torch.from_numpy(a).cuda()
    buf = np.zeros(a.size + lead, a.dtype)
    buf[lead:] = a.reshape(-1)
    return torch.from_numpy(buf).cuda()[lead:].view(a.shape)


def pack(frames, k, tail=()):
    return np.concatenate([np.ascontiguousarray(fr[k]).reshape((-1,) + tail) for fr in frames], axis=0)


def run_kitti(frames, lead=0, out=None):
    """frames: [(disp1, disp2, flow, P)] -> dict of host arrays of ONE ops.frames_from_kitti call."""
    hh, ww = [fr[0].shape[0] for fr in frames], [fr[0].shape[1] for fr in frames]
    res = ops.frames_from_kitti(dev(pack(frames, 0), lead), dev(pack(frames, 1), lead), dev(pack(frames, 2, (3,)), lead),
                                [fr[3] for fr in frames], hh, ww, out=out)
    return {k: x.cpu().numpy() for k, x in zip(KEYS, res)}


def run_ft3d(frames, near=None, lead=0, out=None):
    """frames: [(disp, dchange, flow, occ1, occ2)]."""
    hh, ww = [fr[0].shape[0] for fr in frames], [fr[0].shape[1] for fr in frames]
    res = ops.frames_from_ft3d(dev(pack(frames, 0), lead), dev(pack(frames, 1), lead), dev(pack(frames, 2, (2,)), lead),
                               dev(pack(frames, 3), lead), dev(pack(frames, 4), lead), hh, ww, near=near, out=out)
    return {k: x.cpu().numpy() for k, x in zip(KEYS, res)}


def want_kitti(frames):
    return dict(zip(KEYS, FO.packed([FO.kitti_frame(*fr) for fr in frames], [fr[0].size for fr in frames])))


def want_ft3d(frames, near=None):
    return dict(zip(KEYS, FO.packed([FO.ft3d_frame(*fr, near=near) for fr in frames], [fr[0].size for fr in frames])))


def check(got, want):
    assert np.array_equal(got['counts'], want['counts']), (got['counts'], want['counts'])
    assert got['pixel'].dtype == np.int32 and np.array_equal(got['pixel'], want['pixel'])
    assert FO.same_bits(got['pc1'], want['pc1']) and FO.same_bits(got['pc2'], want['pc2'])


# ----------------------------------------------------------------------------- the reference's outputs
def gold_kitti(k):
    return (GOLD['kitti%d_disp1' % k], GOLD['kitti%d_disp2' % k], GOLD['kitti%d_flow' % k], FO.read_P(str(GOLD['kitti%d_calib' % k])))


def gold_ft3d(k):
    return tuple(GOLD['ft3d%d_%s' % (k, key)] for key in ('disp', 'dchange', 'flow', 'occ1', 'occ2'))


def test_kitti_equals_the_reference():
    frames = [gold_kitti(k) for k in range(3)]
    batch = run_kitti(frames)
    p0 = 0
    for k, fr in enumerate(frames):
        w1, w2 = GOLD['kitti%d_pc1' % k], GOLD['kitti%d_pc2' % k]
        n = len(w1)
        alone = run_kitti([fr])
        for got, at in ((alone, 0), (batch, p0)):
            assert got['counts'][k if got is batch else 0] == n
            assert FO.same_bits(got['pc1'][:, at:at + n].T, w1) and FO.same_bits(got['pc2'][:, at:at + n].T, w2)
        p0 += fr[0].size
    check(batch, want_kitti(frames))


@pytest.mark.parametrize('tag,near', [('all', None), ('near', -35.0)])
def test_ft3d_equals_the_reference(tag, near):
    frames = [gold_ft3d(k) for k in range(2)]
    batch = run_ft3d(frames, near=near)
    p0 = 0
    for k, fr in enumerate(frames):
        w1, w2 = GOLD['ft3d%d_%s_pc1' % (k, tag)], GOLD['ft3d%d_%s_pc2' % (k, tag)]
        n = len(w1)
        alone = run_ft3d([fr], near=near)
        for got, at in ((alone, 0), (batch, p0)):
            assert got['counts'][k if got is batch else 0] == n
            assert FO.same_bits(got['pc1'][:, at:at + n].T, w1) and FO.same_bits(got['pc2'][:, at:at + n].T, w2)
        p0 += fr[0].size
    check(batch, want_ft3d(frames, near))


# ----------------------------------------------------------------------------- fuzzed frames against the restatement
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_shapes_alone(shape):
    rng = np.random.RandomState(shape[0] * 7919 + shape[1])
    fr = FO.kitti_raw(rng, *shape) + (P0,)
    check(run_kitti([fr]), want_kitti([fr]))
    ft = FO.ft3d_raw(rng, *shape)
    check(run_ft3d([ft]), want_ft3d([ft]))
    check(run_ft3d([ft], near=-35.0), want_ft3d([ft], -35.0))


def test_shapes_together_start_at_every_residue():
    rng = np.random.RandomState(77)
    order = [SHAPES[0], SHAPES[2], SHAPES[1]] + SHAPES[3:]
    frames = [FO.kitti_raw(rng, *s) + (FO.read_P(FO.CALIB_NAMES[i % 3]),) for i, s in enumerate(order)]
    starts = np.cumsum([0] + [fr[0].size for fr in frames])[:-1]
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    check(run_kitti(frames), want_kitti(frames))
    fts = [FO.ft3d_raw(rng, *s, extreme=i % 2 == 1) for i, s in enumerate(order)]
    check(run_ft3d(fts), want_ft3d(fts))
    check(run_ft3d(fts, near=-35.0), want_ft3d(fts, -35.0))


def test_the_scan_past_its_first_chunk():
    """A 3 x 5 frame, then frames that own 257 and 256 workgroups: the per-frame scan (k_frames_scan) takes
    a frame's workgroups 256 at a time, so the second frame's last workgroup gets its offset from the carry of the first chunk;
    both large frames start off a multiple of 4 and neither at workgroup 0.  A stretch of 1424 invalid pixels in the second
    frame covers its 256th workgroup and reaches into the 255th and the 257th."""
    def frame_blocks(p0, p1):                                 # csrc/frames.hip: quads start at the frame's start rounded down to 4
        return -(-(p1 - p0 // 4 * 4) // 1024) if p1 > p0 else 0

    shapes = [(3, 5), (2002, 131), (2000, 131)]
    starts = np.cumsum([0] + [h * w for h, w in shapes])
    assert [frame_blocks(int(a), int(b)) for a, b in zip(starts, starts[1:])] == [1, 257, 256] and starts[1] % 4 == 3 and starts[2] % 4 == 1
    lo, hi = 12 + 255 * 1024 - 300 - 15, 12 + 256 * 1024 + 100 - 15        # pixels of the second frame, from packed indices
    rng = np.random.RandomState(78)
    frames = [FO.kitti_raw(rng, *s) + (FO.read_P(FO.CALIB_NAMES[i]),) for i, s in enumerate(shapes)]
    frames[1][0].reshape(-1)[lo:hi] = 0                       # disp1 = 0: not valid
    want = want_kitti(frames)
    px = want['pixel'][15:15 + want['counts'][1]]
    assert not ((px >= lo) & (px < hi)).any() and (px < lo).any() and (px >= hi).any()
    check(run_kitti(frames), want)
    fts = [FO.ft3d_raw(rng, *s) for s in shapes]
    fts[1][3].reshape(-1)[lo:hi] = 255                        # occluded in the first view
    check(run_ft3d(fts, near=-35.0), want_ft3d(fts, -35.0))


def test_all_invalid_all_valid_and_an_empty_frame_between():
    rng = np.random.RandomState(5)
    d1, d2, fl = FO.kitti_raw(rng, 9, 131)
    none = (d1, np.zeros_like(d2), fl, P0)
    every = (np.maximum(d1, 1), np.maximum(d2, 1), np.concatenate([fl[..., :2], np.ones_like(fl[..., :1])], axis=-1), P0)
    empty = (np.zeros((0, 7), np.uint16), np.zeros((0, 7), np.uint16), np.zeros((0, 7, 3), np.uint16), P0)
    thin = (np.zeros((5, 0), np.uint16), np.zeros((5, 0), np.uint16), np.zeros((5, 0, 3), np.uint16), P0)
    for frames in ([none], [every], [every, empty, none], [empty, thin, every, thin], [none, every, empty]):
        got, want = run_kitti(frames), want_kitti(frames)
        check(got, want)
    got = run_kitti([every, empty, none])
    assert got['counts'].tolist() == [9 * 131, 0, 0] and np.array_equal(got['pixel'][:9 * 131], np.arange(9 * 131))
    assert not got['pc1'][:, 9 * 131:].any() and (got['pixel'][9 * 131:] == -1).all()
    disp, dchange, flow, occ1, occ2 = FO.ft3d_raw(rng, 9, 131)
    fnone, fevery = (disp, dchange, flow, occ1, np.full_like(occ2, 255)), (disp, dchange, flow, np.zeros_like(occ1), np.zeros_like(occ2))
    fempty = tuple(x[:0] for x in (disp, dchange, flow, occ1, occ2))
    for frames in ([fnone], [fevery], [fevery, fempty, fnone], [fempty, fevery]):
        check(run_ft3d(frames), want_ft3d(frames))
        check(run_ft3d(frames, near=-35.0), want_ft3d(frames, -35.0))
    far = (np.full_like(disp, -1.0), np.zeros_like(dchange), flow, np.zeros_like(occ1), np.zeros_like(occ2))     # z = -1050: all cut
    assert run_ft3d([far], near=-35.0)['counts'].tolist() == [0] and run_ft3d([far])['counts'].tolist() == [9 * 131]


def test_extreme_raw_values():
    rng = np.random.RandomState(6)
    frames = [FO.kitti_raw(rng, 6, 67, extreme=True) + (FO.read_P(nm),) for nm in FO.CALIB_NAMES]
    d1, d2, fl = frames[0][:3]
    assert {0, 1, 65535} <= set(d1.reshape(-1).tolist()) and {0, 65535} <= set(fl[..., 0].reshape(-1).tolist())
    assert {0, 1, 2} == set(fl[..., 2].reshape(-1).tolist())
    want = want_kitti(frames)
    assert 0 < want['counts'].min() and np.isfinite(want['pc1']).all() and np.isfinite(want['pc2']).all()
    check(run_kitti(frames), want)
    fts = [FO.ft3d_raw(rng, 6, 67, extreme=True) for _ in range(2)]
    assert (fts[0][0] == 0).any() and (fts[0][0] > 0).any() and np.isnan(fts[0][0]).any()
    for near in (None, -35.0):
        want = want_ft3d(fts, near)
        assert np.isinf(want['pc1']).any() and np.isnan(want['pc1']).any() == (near is None)
        check(run_ft3d(fts, near=near), want)


# ----------------------------------------------------------------------------- strides and alignment
def test_strided_output():
    rng = np.random.RandomState(8)
    frames = [FO.kitti_raw(rng, 5, 131) + (P0,), FO.kitti_raw(rng, 2, 65) + (P0,)]
    N = sum(fr[0].size for fr in frames)
    wide1, wide2 = torch.full((3, N + 37), 7.0, device='cuda'), torch.full((3, 2 * N), 7.0, device='cuda')
    got = run_kitti(frames, out=(wide1[:, 5:5 + N], wide2[:, N:]))
    check(got, want_kitti(frames))
    assert (wide1[:, :5] == 7).all() and (wide1[:, 5 + N:] == 7).all() and (wide2[:, :N] == 7).all()
    both = torch.empty((3, 2 * N), device='cuda')                    # the two clouds interleave row by row inside one buffer
    check(run_kitti(frames, out=(both[:, :N], both[:, N:])), want_kitti(frames))
    with pytest.raises(_lib.HplError, match='overlap'):
        run_kitti(frames, out=(both[:, :N], both[:, N - 1:2 * N - 1]))
    fts = [FO.ft3d_raw(rng, 5, 131), FO.ft3d_raw(rng, 2, 65)]
    wide1.fill_(7.0)
    wide2.fill_(7.0)
    check(run_ft3d(fts, near=-35.0, out=(wide1[:, 5:5 + N], wide2[:, N:])), want_ft3d(fts, -35.0))
    assert (wide1[:, :5] == 7).all() and (wide1[:, 5 + N:] == 7).all() and (wide2[:, :N] == 7).all()


@pytest.mark.parametrize('lead', [1, 2, 3])
def test_inputs_that_start_off_their_vector_alignment(lead):
    """lead = 1: the uint16 planes start 2-byte but not 4-byte aligned, the float32 planes 4-byte but not 16-byte aligned, the
    masks at an odd address: every quad takes the pixel-by-pixel path (lead 2 and 3: some planes are vector-aligned again)."""
    rng = np.random.RandomState(9 + lead)
    frames = [FO.kitti_raw(rng, 3, 131) + (P0,), FO.kitti_raw(rng, 9, 131) + (P0,)]
    t = dev(pack(frames, 0), lead)
    assert t.data_ptr() % 4 == (2 * lead) % 4 and t.is_contiguous()
    check(run_kitti(frames, lead=lead), want_kitti(frames))
    fts = [FO.ft3d_raw(rng, 3, 131), FO.ft3d_raw(rng, 9, 131)]
    check(run_ft3d(fts, near=-35.0, lead=lead), want_ft3d(fts, -35.0))


# ----------------------------------------------------------------------------- B = 64
def test_64_frames_each_as_alone():
    rng = np.random.RandomState(64)
    shapes = []
    for i, n in enumerate(counts64()):                        # 0, 1, 3, 37, 300, 2100 and 1025 pixels, empty frames at the ends
        w = 0 if n == 0 else (n if n < 37 else 37 if n == 37 else 25 if n in (300, 2100) else 41)
        shapes.append((0, 5) if n == 0 else (n // w, w))
    assert [h * w for h, w in shapes] == counts64()
    frames = [FO.kitti_raw(rng, h, w) + (FO.read_P(FO.CALIB_NAMES[i % 3]),) for i, (h, w) in enumerate(shapes)]
    fts = [FO.ft3d_raw(rng, h, w, extreme=i % 3 == 0) for i, (h, w) in enumerate(shapes)]
    bk, bf = run_kitti(frames), run_ft3d(fts, near=-35.0)
    check(bk, want_kitti(frames))
    check(bf, want_ft3d(fts, -35.0))
    p0 = 0
    for i, (h, w) in enumerate(shapes):
        n = h * w
        if n:                                                 # the device's own single-frame run
            for batch, alone in ((bk, run_kitti([frames[i]])), (bf, run_ft3d([fts[i]], near=-35.0))):
                assert batch['counts'][i] == alone['counts'][0] and np.array_equal(batch['pixel'][p0:p0 + n], alone['pixel'])
                assert FO.same_bits(batch['pc1'][:, p0:p0 + n], alone['pc1']) and FO.same_bits(batch['pc2'][:, p0:p0 + n], alone['pc2'])
        p0 += n


# ----------------------------------------------------------------------------- the list wrappers
def test_flownet_wrappers_return_views_per_frame():
    rng = np.random.RandomState(10)
    frames = [FO.kitti_raw(rng, 4, 33) + (P0,), FO.kitti_raw(rng, 7, 131) + (FO.read_P('000155'),)]
    pc1, pc2, pixel, counts = flownet.frames_from_kitti(frames)
    for b, fr in enumerate(frames):
        w1, w2, wp = FO.kitti_frame(*fr)
        assert counts[b] == len(wp) and tuple(pc1[b].shape) == (3, len(wp)) and np.array_equal(pixel[b].cpu().numpy(), wp)
        assert FO.same_bits(pc1[b].t().cpu().numpy(), w1) and FO.same_bits(pc2[b].t().cpu().numpy(), w2)
    fts = [FO.ft3d_raw(rng, 4, 33), tuple(torch.from_numpy(x) for x in FO.ft3d_raw(rng, 7, 131))]
    pc1, pc2, pixel, counts = flownet.frames_from_ft3d(fts, near=-35.0)
    for b, fr in enumerate(fts):
        w1, w2, wp = FO.ft3d_frame(*[np.asarray(x) for x in fr], near=-35.0)
        assert counts[b] == len(wp) and np.array_equal(pixel[b].cpu().numpy(), wp)
        assert FO.same_bits(pc1[b].t().cpu().numpy(), w1) and FO.same_bits(pc2[b].t().cpu().numpy(), w2)


# ----------------------------------------------------------------------------- raw tree -> tool -> readers -> engine
def test_raw_trees_through_the_tool_the_readers_and_the_engine(tmp_path):
    from hplflownet_amd import engine
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import preprocess
    rng = np.random.RandomState(11)
    # KITTI: disparities of 12.5 px and more keep the depths inside the readers' 35 m
    raw, calib, root = str(tmp_path / 'kraw'), str(tmp_path / 'calib'), tmp_path / 'kdata'
    kframes = [FO.kitti_raw(rng, 36 + k, 120 + 7 * k, p_valid=0.9, lo=3200) for k in range(3)]
    FO.write_kitti_tree(raw, calib, kframes, FO.CALIB_NAMES)
    assert preprocess.main([raw, str(root / 'KITTI_processed_occ_final'), '--dataset', 'KITTI', '--kitti-calib', calib, '--batch', '2']) == 3
    for kw in (dict(remove_ground=False), dict(), dict(remove_ground='plane'), dict(voxel=0.3)):
        old = data.KITTI(None, str(root), calib_dir=calib, **kw)
        new = data.KITTIRaw(None, raw, calib, **kw)
        assert len(old) == len(new) == 3
        for i in range(3):
            a, b = old.load(old.samples[i]), new.load(new.samples[i])
            assert a[0].dtype == b[0].dtype == np.float32 and a[0].shape == b[0].shape and len(a[0]) > 0
            assert FO.same_bits(a[0], b[0]) and FO.same_bits(a[1], b[1])
            so, sn = old[i], new[i]
            assert all(torch.equal(x, y) for x, y in zip(so, sn)) and so.camera == sn.camera and sn.camera is not None
    saved = np.load(str(root / 'KITTI_processed_occ_final' / '000155' / 'pc1.npy'))
    want = FO.kitti_frame(*kframes[1], FO.read_P('000155'))[0]
    assert saved.dtype == np.float32 and saved.ndim == 2 and saved.shape[1] == 3 and FO.same_bits(saved, want)
    # FlyingThings3D subset
    fraw, froot = str(tmp_path / 'fraw'), tmp_path / 'fdata'
    names = ['%07d' % k for k in range(5)]
    trees = {split: [FO.ft3d_raw(rng, 30 + k, 100 + 3 * k, p_valid=0.9) for k in range(5)] for split in ('train', 'val')}
    for split, frs in trees.items():
        FO.write_ft3d_tree(fraw, split, frs, names)
    assert preprocess.main([fraw, str(froot / 'FlyingThings3D_subset_processed_35m'), '--dataset', 'FlyingThings3DSubset', '--batch', '3']) == 10
    for train in (False, True):
        old = data.FlyingThings3DSubset(train, None, str(froot), full=True)
        new = data.FlyingThings3DRaw(train, None, fraw, full=True)
        assert len(old) == len(new) == 5
        for i in range(5):
            a, b = old.load(old.samples[i]), new.load(new.samples[i])
            assert a[0].shape == b[0].shape and len(a[0]) > 0 and FO.same_bits(a[0], b[0]) and FO.same_bits(a[1], b[1])
            assert (b[0][:, 2] > 0).all() and (b[0][:, 2] < 35).all()                      # x and z flipped, the near cut applied
        assert all(torch.equal(x, y) for x, y in zip(old[2], new[2])) and new[2].camera == data.FT3D_CAMERA
    w1 = FO.ft3d_frame(*trees['val'][4], near=-35.0)[0]
    assert FO.same_bits(np.load(str(froot / 'FlyingThings3D_subset_processed_35m' / 'val' / names[4] / 'pc1.npy')), w1)
    # the engine evaluates a random-weight model on the raw trees
    common = ['--evaluate', '--batch-size', '2', '--ragged', '--points', '8192', '--arch', 'HPLFlowNetShallow']
    res = engine.main(['--dataset', 'KITTI', '--raw-root', raw, '--kitti-calib', calib] + common)
    assert res and all(np.isfinite(v) for v in res.values()) and 'EPE2D' in res, res
    res = engine.main(['--dataset', 'FlyingThings3DSubset', '--raw-root', fraw] + common)
    assert res and all(np.isfinite(v) for v in res.values()), res
