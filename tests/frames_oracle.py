"""numpy restatement of hpl_frames_from_kitti / hpl_frames_from_ft3d (include/hpl_bcl.h): every operation on
float32 arrays, one rounding each, in the order the header states -- which is the order of the reference's kitti_utils.pixel2xyz /
disp_2_depth and flyingthings3d_utils.pixel2pc / next_pixel2pc (tests/golden/frames.npz holds THEIR outputs; test_frames_cpu.py
holds this file equal to them bit for bit).  Also generators of small synthetic raw frames and writers of the raw file formats
-- a PNG writer that can force each of the five row filters, PFM, .flo -- and of raw trees in the two datasets' layouts.
"""
import os
import struct
import zlib

import numpy as np

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CALIB_DIR = os.path.join(HERE, 'golden', 'kitti_calib')
CALIB_NAMES = ('000000', '000155', '000157')


# ------------------------------------------------------------------------------------------------ the restatement
def _grid(H, W):
    px = np.tile(np.arange(W, dtype=f32)[None, :], (H, 1))
    py = np.tile(np.arange(H, dtype=f32)[:, None], (1, W))
    return px, py


def kitti_frame(disp1, disp2, flow, P, baseline=0.54):
    """-> (pc1 [n, 3], pc2 [n, 3], pixel [n]) float32 / int32: the valid correspondences in ascending pixel index."""
    P = np.asarray(P, dtype=f32).reshape(3, 4)
    H, W = disp1.shape
    valid = (disp1 > 0) & (disp2 > 0) & (flow[..., 2] == 1)
    fb = P[0, 0] * f32(baseline)
    px1, py1 = _grid(H, W)
    px2 = px1 + (flow[..., 0].astype(f32) - f32(32768)) / f32(64)
    py2 = py1 + (flow[..., 1].astype(f32) - f32(32768)) / f32(64)

    def cloud(r, px, py):
        z = fb / (r.astype(f32) / f32(256) + f32(1e-5))
        x = -(((px * (z + P[2, 3])) - ((P[0, 2] * z) + P[0, 3])) / P[0, 0])
        y = -(((py * (z + P[2, 3])) - ((P[1, 2] * z) + P[1, 3])) / P[0, 0])
        return np.stack([x, y, z], axis=-1).astype(f32)

    with np.errstate(all='ignore'):
        pc1, pc2 = cloud(disp1, px1, py1), cloud(disp2, px2, py2)
    return pc1[valid], pc2[valid], np.flatnonzero(valid.reshape(-1)).astype(np.int32)


def ft3d_frame(disp, dchange, flow, occ1, occ2, near=None, f=-1050.0, cx=479.5, cy=269.5):
    """-> (pc1 [n, 3], pc2 [n, 3], pixel [n]); near: None or the near cut."""
    H, W = disp.shape
    nf, cx, cy = f32(-float(f)), f32(cx), f32(cy)
    px, py = _grid(H, W)
    with np.errstate(all='ignore'):
        d1 = disp.astype(f32)
        d2 = d1 + dchange.astype(f32)
        pxc, pyc = px - cx, py - cy
        pc1 = np.stack([(-pxc) / d1, pyc / d1, nf / d1], axis=-1).astype(f32)
        pc2 = np.stack([(-(pxc + flow[..., 0])) / d2, (pyc + flow[..., 1]) / d2, nf / d2], axis=-1).astype(f32)
        valid = (occ1 == 0) & (occ2 == 0)
        if near is not None:
            valid = valid & (pc1[..., 2] > f32(near)) & (pc2[..., 2] > f32(near))
    return pc1[valid], pc2[valid], np.flatnonzero(valid.reshape(-1)).astype(np.int32)


def packed(results, sizes):
    """The packed outputs of a batch: results = [(pc1, pc2, pixel)] per frame, sizes = [H * W] per frame
    -> (pc1 (3, N), pc2 (3, N), pixel (N,), counts (B,)) with the tails 0 / -1."""
    N = int(sum(sizes))
    o1, o2 = np.zeros((3, N), f32), np.zeros((3, N), f32)
    pixel = np.full(N, -1, np.int32)
    counts = np.zeros(len(sizes), np.int32)
    p0 = 0
    for b, ((a, c, px), n) in enumerate(zip(results, sizes)):
        k = len(px)
        o1[:, p0:p0 + k], o2[:, p0:p0 + k], pixel[p0:p0 + k], counts[b] = a.T, c.T, px, k
        p0 += n
    return o1, o2, pixel, counts


def same_bits(a, b):
    """Equal bit for bit, NaN where NaN (a NaN's payload is the processor's, not the definition's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    bits = a.view(np.uint32) == b.view(np.uint32)
    return bool(np.array_equal(na, nb) and np.all(bits | na))


# ------------------------------------------------------------------------------------------------ synthetic raw frames
def read_P(name):
    with open(os.path.join(CALIB_DIR, name + '.txt')) as fd:
        for line in fd:
            if line.startswith('P_rect_02'):
                return np.array([float(v) for v in line.split()[1:]], dtype=f32).reshape(3, 4)
    raise ValueError(name)


def kitti_raw(rng, H, W, p_valid=0.7, extreme=False, lo=256):
    """(disp1, disp2, flow) uint16 raw values, the valid disparities in lo .. 39999; extreme: disparities among 0 / 1 / 65535,
    flow among 0 / 65535, masks 0 / 1 / 2."""
    if extreme:
        d1 = rng.choice(np.array([0, 1, 65535, 300], np.uint16), size=(H, W))
        d2 = rng.choice(np.array([0, 1, 65535, 7000], np.uint16), size=(H, W))
        uv = rng.choice(np.array([0, 65535, 32768], np.uint16), size=(H, W, 2))
        m = rng.choice(np.array([0, 1, 1, 2], np.uint16), size=(H, W))
    else:
        d1 = rng.randint(lo, 40000, size=(H, W)).astype(np.uint16)
        d2 = rng.randint(lo, 40000, size=(H, W)).astype(np.uint16)
        d1[rng.rand(H, W) > p_valid ** 0.34] = 0
        d2[rng.rand(H, W) > p_valid ** 0.34] = 0
        uv = (32768 + rng.randint(-4000, 4000, size=(H, W, 2))).astype(np.uint16)
        m = (rng.rand(H, W) < p_valid ** 0.34).astype(np.uint16)
    return d1, d2, np.ascontiguousarray(np.concatenate([uv, m[..., None]], axis=-1))


def ft3d_raw(rng, H, W, p_valid=0.7, extreme=False):
    """(disp, dchange, flow, occ1, occ2): float32 maps and uint8 masks (0 visible, 255 occluded); extreme: disparities 0 and of
    both signs, so that depths are infinite, NaN (0 / 0 cannot occur, but d2 = d - d can be 0) and on both sides of the cut."""
    disp = -(5 + 295 * rng.rand(H, W)).astype(f32)
    dchange = rng.uniform(-3, 3, size=(H, W)).astype(f32)
    if extreme:
        pick = rng.rand(H, W)
        disp[pick < 0.15] = 0
        disp[(pick >= 0.15) & (pick < 0.3)] *= -1
        dchange[(pick >= 0.3) & (pick < 0.4)] = -disp[(pick >= 0.3) & (pick < 0.4)]
        disp[(pick >= 0.4) & (pick < 0.45)] = np.nan
    flow = rng.uniform(-30, 30, size=(H, W, 2)).astype(f32)
    occ1 = np.where(rng.rand(H, W) < p_valid ** 0.5, 0, 255).astype(np.uint8)
    occ2 = np.where(rng.rand(H, W) < p_valid ** 0.5, 0, 255).astype(np.uint8)
    return disp, dchange, flow, occ1, occ2


# ------------------------------------------------------------------------------------------------ file writers
def _chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)


def png_filter_rows(raw, bpp, filters):
    """raw (H, n) uint8 unfiltered rows -> (H, 1 + n) rows led by their filter byte.  Forward filtering looks at unfiltered
    bytes only, so it is elementwise."""
    H, n = raw.shape
    x = raw.astype(np.int32)
    left = np.zeros_like(x)
    left[:, bpp:] = x[:, :-bpp] if n > bpp else 0
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    upleft = np.zeros_like(x)
    upleft[1:, bpp:] = x[:-1, :-bpp] if n > bpp else 0
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = [np.zeros_like(x), left, up, (left + up) >> 1, paeth]
    out = np.zeros((H, 1 + n), np.uint8)
    for y in range(H):
        out[y, 0] = filters[y]
        out[y, 1:] = ((x[y] - preds[filters[y]][y]) & 0xff).astype(np.uint8)
    return out


def png_bytes(arr, filters=0, interlace=0, colour=None, depth=None, idat_split=0):
    """A PNG of arr -- uint8 / uint16, (H, W) or (H, W, 3) --; filters: one filter type for all rows or a list per row.
    interlace / colour / depth override the header (for the refusals); idat_split > 0 cuts the data into chunks of that size."""
    arr = np.ascontiguousarray(arr)
    H, W = arr.shape[:2]
    channels = 1 if arr.ndim == 2 else arr.shape[2]
    bits = 8 * arr.dtype.itemsize
    raw = (arr.astype('>u2') if bits == 16 else arr).reshape(H, -1).view(np.uint8).reshape(H, -1)
    fl = [filters] * H if isinstance(filters, int) else list(filters)
    data = zlib.compress(png_filter_rows(raw, channels * bits // 8, fl).tobytes(), 6)
    ihdr = struct.pack('>IIBBBBB', W, H, bits if depth is None else depth, ({1: 0, 3: 2}[channels]) if colour is None else colour,
                       0, 0, interlace)
    parts = [data] if idat_split <= 0 else [data[i:i + idat_split] for i in range(0, len(data), idat_split)]
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'tEXt', b'Comment\x00synthetic') + \
        b''.join(_chunk(b'IDAT', p) for p in parts) + _chunk(b'IEND', b'')


def write_png(path, arr, filters=0, **kw):
    with open(path, 'wb') as fd:
        fd.write(png_bytes(arr, filters, **kw))


def mixed_filters(H, start=0):
    return [(start + y) % 5 for y in range(H)]


def write_pfm(path, arr, little=True, scale=1.0):
    arr = np.asarray(arr, dtype=f32)
    with open(path, 'wb') as fd:
        fd.write(b'PF\n' if arr.ndim == 3 else b'Pf\n')
        fd.write(b'%d %d\n' % (arr.shape[1], arr.shape[0]))
        fd.write(b'%f\n' % (-scale if little else scale))
        fd.write(np.flipud(arr).astype('<f4' if little else '>f4').tobytes())


def write_flo(path, flow):
    flow = np.asarray(flow, dtype=f32)
    with open(path, 'wb') as fd:
        fd.write(b'PIEH' + struct.pack('<ii', flow.shape[1], flow.shape[0]) + flow.astype('<f4').tobytes())


def write_kitti_tree(raw_root, calib_dir, frames, names):
    """frames: [(disp1, disp2, flow)]; names: frame numbers among CALIB_NAMES (their calibrations are copied to calib_dir)."""
    import shutil
    os.makedirs(calib_dir, exist_ok=True)
    for sub in ('disp_occ_0', 'disp_occ_1', 'flow_occ'):
        os.makedirs(os.path.join(raw_root, 'training', sub), exist_ok=True)
    for k, ((d1, d2, fl), nm) in enumerate(zip(frames, names)):
        for sub, x in (('disp_occ_0', d1), ('disp_occ_1', d2), ('flow_occ', fl)):
            write_png(os.path.join(raw_root, 'training', sub, nm + '_10.png'), x, mixed_filters(x.shape[0], k))
        shutil.copy(os.path.join(CALIB_DIR, nm + '.txt'), os.path.join(calib_dir, nm + '.txt'))


FT3D_DIRS = (('disparity', 'left'), ('disparity_occlusions', 'left'), ('disparity_change', 'left', 'into_future'),
             ('flow', 'left', 'into_future'), ('flow_occlusions', 'left', 'into_future'))


def write_ft3d_tree(raw_root, split, frames, names):
    """frames: [(disp, dchange, flow, occ1, occ2)] below raw_root/split in the raw subset's layout."""
    dirs = [os.path.join(raw_root, split, *parts) for parts in FT3D_DIRS]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    for k, ((disp, dchange, flow, occ1, occ2), nm) in enumerate(zip(frames, names)):
        write_pfm(os.path.join(dirs[0], nm + '.pfm'), disp, little=k % 2 == 0)
        write_png(os.path.join(dirs[1], nm + '.png'), occ1, mixed_filters(occ1.shape[0], k))
        write_pfm(os.path.join(dirs[2], nm + '.pfm'), dchange, little=k % 2 == 1)
        write_flo(os.path.join(dirs[3], nm + '.flo'), flow)
        write_png(os.path.join(dirs[4], nm + '.png'), occ2, 4)
