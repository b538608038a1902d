"""Data path in front of the lattice build.

Own restatement of what feeds the hot path in the reference:

* `ProcessData` (/root/reference/transforms/transforms.py:494-548): scene flow `sf = pc2 - pc1`,
  depth cut (both clouds closer than DEPTH_THRESHOLD, :509-512), sampling of `num_points` indices
  without replacement -- the same indices for both clouds unless NO_CORR (:519-525) -- and the
  `allow_less_points` fallback (:526-532).  Differences: the RNG is an explicit, seedable
  `numpy.random.RandomState` instead of the global one, and failure returns `(None, None, None)`
  without printing.
* `Augmentation` (/root/reference/transforms/transforms.py:551-640), the training-time transform:
  both clouds get one random per-axis scale x rotation about y, one shift and a clipped per-point
  jitter (:565-590); cloud 2 then gets its own rotation about y and shift (:592-606), `sf` is
  taken BEFORE cloud 2's own jitter (:607-613); depth cut and sampling as in ProcessData.  The
  draws are made in the reference's order from the seedable RandomState, so `seed=s` reproduces
  the reference under `np.random.seed(s)` bit for bit (tests/golden/transforms.npz).  Unlike the
  reference the caller's arrays are not modified in place.
* `FlyingThings3DSubset` (/root/reference/datasets/flyingthings3d_subset.py:22-101): leaf
  directories below `<root>/FlyingThings3D_subset_processed_35m/{train,val}` holding `pc1.npy` /
  `pc2.npy`; x and z are negated on load (:96-99); every 4th sample unless `full` (:79-82).
* `KITTI` (/root/reference/datasets/kitti.py:22-107): leaf directories below
  `<root>/KITTI_processed_occ_final`; points with y < -1.4 in BOTH clouds are ground and removed
  (:100-105); frames whose line in the mapping file is empty are skipped (:76-83; the mapping file
  ships with the reference's dataset code, pass its path if you have it).

Cameras (the 2D metrics EPE2D / ACC2D, evaluation_utils.py:22-36, project the flow into the image): whether a reader has them
is a property of the reader (`has_cameras`), and every sample it returns carries the camera of the frame it actually came from
(`Sample.camera`, a fall-through to the next frame included).  FlyingThings3D has one fixed pinhole (the defaults of
utils/geometry.py:project_3d_to_2d); KITTI has `P_rect_02` of `calib_cam_to_cam/<frame>.txt` (utils/geometry.py:15-31), read
from `calib_dir` at construction -- without it the reader has no cameras.

* `KITTIRaw` / `FlyingThings3DRaw`: the same readers over the RAW downloads -- disparity, optical-flow and occlusion maps --
  which the reference turns into the processed trees offline (data_preprocess/process_kitti.py,
  process_flyingthings3d_subset.py).  Here the frames are back-projected on the device when they are read
  (flownet.frames_from_kitti / frames_from_ft3d), bit for bit what the scripts save; `read_png`, `read_pfm` and
  `read_flo` read the raw files (data_preprocess/IO.py, kitti_utils.py:29-36) without scipy or pypng.

The reference asserts the canonical sample counts (19 640 / 3 824 / 200) and exits; here a
mismatch is reported by `check_counts()` and left to the caller.  No dataset is available in the
build environment: the readers are exercised on synthetic directory trees of the same layout
(tests/test_data_cpu.py).  Samples are returned as device tensors `(3, N)` ready for
`GenerateDataUnsymmetric.build` -- the lattice itself is built on the GPU by the consumer
(engine.Trainer pipelines it on a second stream), not in DataLoader workers.
"""
import os

import numpy as np
import torch

__all__ = ['ProcessData', 'Augmentation', 'DeviceProcessData', 'DeviceAugmentation', 'FlyingThings3DSubset', 'KITTI', 'Sample',
           'read_kitti_camera', 'read_kitti_P', 'read_png', 'write_png', 'read_pfm', 'read_flo', 'KITTIRaw', 'FlyingThings3DRaw']

#: (f, cx, cy, constx, consty, constz) of every FlyingThings3D frame (utils/geometry.py:59 defaults)
FT3D_CAMERA = (-1050.0, 479.5, 269.5, 0.0, 0.0, 0.0)


class Sample(tuple):
    """(pc1, pc2, sf) of a reader, with `camera`: the (f, cx, cy, constx, consty, constz) of the frame it came from, or None;
    `frame`: that frame's name in its tree (KITTI: NNNNNN); `size`: the (H, W) of its raw maps where the reader saw them."""
    camera = None
    frame = None
    size = None


def read_kitti_camera(path):
    """The camera of a KITTI calib_cam_to_cam file as utils/geometry.py:15-31 reads it: the first line starting with P_rect_02
    as a float32 (3, 4) matrix P -> (f, cx, cy, constx, consty, constz) = (-P[0,0], P[0,2], P[1,2], P[0,3], P[1,3], P[2,3]),
    float32 values.  Only that line is parsed (other lines of KITTI's own files can be malformed)."""
    with open(path) as fd:
        for line in fd:
            if line.startswith('P_rect_02'):
                P = np.array([float(v) for v in line.split()[1:]], dtype=np.float32).reshape(3, 4)
                return tuple(float(v) for v in (-P[0, 0], P[0, 2], P[1, 2], P[0, 3], P[1, 3], P[2, 3]))
    raise ValueError('%s has no P_rect_02 line' % path)


def read_kitti_P(path):
    """P_rect_02 of a KITTI calib_cam_to_cam file as process_kitti.py:19-26 reads it: a float32 (3, 4) matrix (the first such
    line, as read_kitti_camera)."""
    with open(path) as fd:
        for line in fd:
            if line.startswith('P_rect_02'):
                return np.array([float(v) for v in line.split()[1:]], dtype=np.float32).reshape(3, 4)
    raise ValueError('%s has no P_rect_02 line' % path)


def read_png(path):
    """A PNG's raw sample values: uint8 or uint16 array (H, W) (greyscale) or (H, W, 3) (RGB) -- KITTI's disparity maps are
    16-bit grey, its flow maps 16-bit RGB, which Pillow cannot return.  Colour types 0 and 2 at depths 8 and 16, not
    interlaced; anything else is refused by name.  The chunks are parsed and inflated here; the row filters are undone by the
    library (hpl_png_unfilter, host only)."""
    import struct
    import zlib
    from . import ops
    with open(path, 'rb') as fd:
        blob = fd.read()
    if blob[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError('%s is not a PNG file' % path)
    at, header, idat, ended = 8, None, [], False
    while at + 12 <= len(blob) and not ended:
        n, kind = struct.unpack('>I4s', blob[at:at + 8])
        body = blob[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(blob):
            raise ValueError('%s: chunk %s is cut short' % (path, kind.decode('latin-1')))
        if zlib.crc32(kind + body) & 0xffffffff != struct.unpack('>I', blob[at + 8 + n:at + 12 + n])[0]:
            raise ValueError('%s: chunk %s fails its CRC' % (path, kind.decode('latin-1')))
        if kind == b'IHDR':
            if n != 13:
                raise ValueError('%s: IHDR of %d bytes' % (path, n))
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            ended = True
        at += 12 + n
    if header is None or not idat or not ended:
        raise ValueError('%s: no IHDR, IDAT or IEND chunk' % path)
    width, height, depth, colour, compression, filtering, interlace = header
    if colour not in (0, 2) or depth not in (8, 16):
        raise ValueError('%s: colour type %d at %d bits (read_png takes greyscale (0) and RGB (2) at 8 or 16 bits)' % (path, colour, depth))
    if interlace != 0 or compression != 0 or filtering != 0:
        raise ValueError('%s: interlace %d, compression %d, filter method %d (read_png takes non-interlaced PNGs of method 0)' % (
            path, interlace, compression, filtering))
    if width == 0 or height == 0:
        raise ValueError('%s: %d x %d pixels' % (path, width, height))
    channels = 3 if colour == 2 else 1
    bpp = channels * depth // 8
    stride = 1 + width * bpp
    raw = zlib.decompress(b''.join(idat))
    if len(raw) != height * stride:
        raise ValueError('%s: %d bytes of image data, %d x %d pixels of %d bytes need %d' % (path, len(raw), width, height, bpp, height * stride))
    rows = np.ascontiguousarray(ops.png_unfilter(raw, height, stride, bpp))
    px = rows if depth == 8 else rows.view('>u2').astype(np.uint16)
    return px.reshape(height, width) if channels == 1 else px.reshape(height, width, 3)


def write_png(path, arr):
    """Writes what read_png reads: a uint8 or uint16 array of shape (H, W) (greyscale) or (H, W, 3) (RGB) as a non-interlaced
    PNG of the same depth -- KITTI's disparity maps are 16-bit grey, its flow maps 16-bit RGB.  Every row goes out with filter
    type 0 (None), deflated with zlib; the chunks are IHDR, one IDAT and IEND."""
    import struct
    import zlib
    arr = np.asarray(arr)
    if arr.dtype not in (np.uint8, np.uint16) or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3) or \
            arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError('write_png takes uint8 or uint16 arrays of shape (H, W) or (H, W, 3) with H, W >= 1, got %s %s' % (
            arr.dtype, arr.shape))
    height, width = arr.shape[:2]
    samples = arr.astype('>u2') if arr.dtype == np.uint16 else arr           # (PNG samples are big-endian)
    rows = np.ascontiguousarray(samples).reshape(height, -1).view(np.uint8)
    raw = np.concatenate([np.zeros((height, 1), np.uint8), rows], axis=1).tobytes()      # a filter byte 0 leads every row

    def chunk(kind, body):
        return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xffffffff)

    header = struct.pack('>IIBBBBB', width, height, 8 * arr.dtype.itemsize, 2 if arr.ndim == 3 else 0, 0, 0, 0)
    with open(path, 'wb') as fd:
        fd.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', header) + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def read_pfm(path):
    """A PFM image as data_preprocess/IO.py:33-68 reads it: float32 (H, W) ('Pf') or (H, W, 3) ('PF'), the file's bottom-up rows
    turned top-down, little-endian when the scale is negative and big-endian otherwise."""
    import re
    with open(path, 'rb') as fd:
        kind = fd.readline().rstrip()
        if kind not in (b'PF', b'Pf'):
            raise ValueError('%s is not a PFM file' % path)
        dims = re.match(r'^(\d+)\s(\d+)\s$', fd.readline().decode('ascii', 'replace'))
        if not dims:
            raise ValueError('%s: malformed PFM header' % path)
        width, height = int(dims.group(1)), int(dims.group(2))
        try:
            scale = float(fd.readline().decode('ascii', 'replace').rstrip())
        except ValueError:
            raise ValueError('%s: malformed PFM header' % path)
        shape = (height, width, 3) if kind == b'PF' else (height, width)
        data = np.frombuffer(fd.read(), dtype='<f4' if scale < 0 else '>f4')
    if data.size != int(np.prod(shape)):
        raise ValueError('%s: %d values for %d x %d pixels' % (path, data.size, width, height))
    return np.ascontiguousarray(np.flipud(data.reshape(shape)), dtype=np.float32)


def read_flo(path):
    """A Middlebury .flo file as data_preprocess/IO.py:100-115 reads it: float32 (H, W, 2)."""
    with open(path, 'rb') as fd:
        blob = fd.read()
    if blob[:4] != b'PIEH':
        raise ValueError('%s: flow file header does not contain PIEH' % path)
    if len(blob) < 12:
        raise ValueError('%s is cut short' % path)
    width, height = (int(v) for v in np.frombuffer(blob, '<i4', 2, 4))
    if width < 0 or height < 0 or len(blob) - 12 < 8 * width * height:
        raise ValueError('%s: %d bytes for %d x %d pixels' % (path, len(blob) - 12, width, height))
    return np.frombuffer(blob, '<f4', 2 * width * height, 12).reshape(height, width, 2).astype(np.float32)


class ProcessData(object):
    def __init__(self, data_process_args, num_points, allow_less_points, seed=None):
        self.DEPTH_THRESHOLD = data_process_args['DEPTH_THRESHOLD']
        self.no_corr = data_process_args['NO_CORR']
        self.num_points = num_points
        self.allow_less_points = allow_less_points
        self.rng = np.random.RandomState(seed)

    def __call__(self, data):
        pc1, pc2 = data
        if pc1 is None:
            return None, None, None
        return self._select(pc1, pc2, pc2[:, :3] - pc1[:, :3])

    def _select(self, pc1, pc2, sf):
        """Depth cut + sampling; `sf` rows follow cloud 1's draw."""
        if self.DEPTH_THRESHOLD > 0:
            near = (pc1[:, 2] < self.DEPTH_THRESHOLD) & (pc2[:, 2] < self.DEPTH_THRESHOLD)
        else:
            near = np.ones(pc1.shape[0], dtype=bool)
        idx = np.nonzero(near)[0]
        if idx.size == 0:
            return None, None, None
        i1 = i2 = idx
        if self.num_points > 0:
            if idx.size >= self.num_points:
                i1 = self.rng.choice(idx, size=self.num_points, replace=False)
                i2 = self.rng.choice(idx, size=self.num_points, replace=False) if self.no_corr else i1
            elif not self.allow_less_points:
                return None, None, None
        return pc1[i1], pc2[i2], sf[i1]

    def __repr__(self):
        return ('%s\n(data_process_args: \n\tDEPTH_THRESHOLD: %s\n\tNO_CORR: %s\n\tallow_less_points: %s\n'
                '\tnum_points: %s\n)' % (self.__class__.__name__, self.DEPTH_THRESHOLD, self.no_corr,
                                         self.allow_less_points, self.num_points))


def _rot_y(angle, dtype):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=dtype)


class Augmentation(object):
    def __init__(self, aug_together_args, aug_pc2_args, data_process_args, num_points, allow_less_points=False,
                 seed=None):
        self.together_args = aug_together_args
        self.pc2_args = aug_pc2_args
        self.sampler = ProcessData(data_process_args, num_points, allow_less_points)
        self.rng = self.sampler.rng = np.random.RandomState(seed)
        self.no_corr = self.sampler.no_corr

    def _jitter(self, a, n):
        return np.clip(a['jitter_sigma'] * self.rng.randn(n, 3), -a['jitter_clip'], a['jitter_clip']).astype(np.float32)

    def __call__(self, data):
        pc1, pc2 = data
        if pc1 is None:
            return None, None, None
        tg, p2, rng = self.together_args, self.pc2_args, self.rng
        n = pc1.shape[0]
        # common motion of the scene: per-axis scale, rotation about y, shift, per-point jitter (in this draw order)
        scale = np.diag(rng.uniform(tg['scale_low'], tg['scale_high'], 3).astype(np.float32))
        m = scale.dot(_rot_y(rng.uniform(-tg['degree_range'], tg['degree_range']), np.float32).T)
        shift = rng.uniform(-tg['shift_range'], tg['shift_range'], (1, 3)).astype(np.float32)
        bias = shift + self._jitter(tg, n)
        a = pc1.copy()
        b = pc2.copy()
        a[:, :3] = pc1[:, :3].dot(m) + bias
        b[:, :3] = pc2[:, :3].dot(m) + bias
        # extra motion of cloud 2: rotation about y, shift; the flow is read off before its jitter
        m2 = _rot_y(rng.uniform(-p2['degree_range'], p2['degree_range']), pc1.dtype)
        shift2 = rng.uniform(-p2['shift_range'], p2['shift_range'], (1, 3)).astype(np.float32)
        b[:, :3] = b[:, :3].dot(m2.T) + shift2
        sf = b[:, :3] - a[:, :3]
        if not self.no_corr:
            b[:, :3] += self._jitter(p2, n)
        return self.sampler._select(a, b, sf)

    def __repr__(self):
        fmt = lambda d: ''.join('\t%-10s %s\n' % (k, d[k]) for k in sorted(d))      # noqa: E731
        return ('%s\n(together_args: \n%s\npc2_args: \n%s\ndata_process_args: \n\tDEPTH_THRESHOLD: %s\n'
                '\tNO_CORR: %s\n\tallow_less_points: %s\n\tnum_points: %s\n)' % (
                    self.__class__.__name__, fmt(self.together_args), fmt(self.pc2_args), self.sampler.DEPTH_THRESHOLD,
                    self.no_corr, self.sampler.allow_less_points, self.sampler.num_points))


class DeviceProcessData(object):
    """ProcessData on the device: the same arguments plus `device`; the raw numpy clouds go in, a Sample of
    (3, k) float32 device tensors -- or (None, None, None) on a rejection -- comes out (ops.TransformRunner over
    hpl_transform_pair, csrc/transforms.hip).  The sampling draws from a counter-based stream (Philox keyed by `seed`, one
    counter step per call): the same distribution as the host class, not the same sample; deterministic under a seed."""

    on_device = True
    augment = False

    def __init__(self, data_process_args, num_points, allow_less_points, seed=None, device='cuda'):
        from . import ops
        self.DEPTH_THRESHOLD = data_process_args['DEPTH_THRESHOLD']
        self.no_corr = data_process_args['NO_CORR']
        self.num_points = num_points
        self.allow_less_points = allow_less_points
        self.rng = np.random.RandomState(seed)
        self.seed = int(seed) & (2 ** 64 - 1) if seed is not None else int(self.rng.randint(0, 2 ** 63, dtype=np.int64))
        self.calls = 0
        self.runner = ops.TransformRunner(device)

    def params(self):
        """The hpl_transform_params of the next call (draws the host scalars of an augmentation)."""
        from ._lib import TransformParams
        p = TransformParams()
        p.depth_threshold = self.DEPTH_THRESHOLD        # (ctypes rounds it to float32, as numpy's comparison does)
        p.no_corr = int(bool(self.no_corr))
        p.num_points = int(self.num_points)
        p.allow_less_points = int(bool(self.allow_less_points))
        p.augment = int(self.augment)
        p.seed = self.seed
        p.counter = self.calls
        return p

    def __call__(self, data):
        pc1, pc2 = data
        if pc1 is None or pc1.shape[0] == 0:
            return None, None, None
        p = self.params()
        self.calls += 1
        out = self.runner.run(pc1, pc2, p)
        return Sample(out) if out[0] is not None else out

    def __repr__(self):
        return ('%s\n(data_process_args: \n\tDEPTH_THRESHOLD: %s\n\tNO_CORR: %s\n\tallow_less_points: %s\n'
                '\tnum_points: %s\n\tdevice: %s\n)' % (self.__class__.__name__, self.DEPTH_THRESHOLD, self.no_corr,
                                                       self.allow_less_points, self.num_points, self.runner.device))


class DeviceAugmentation(DeviceProcessData):
    """Augmentation on the device: per call the scalars are drawn on the host from RandomState(seed) in the reference's order
    without the jitter and the choice (scale x3, angle, shift x3, cloud 2's angle, shift2 x3); the per-point jitter and the
    sampling come from the device's counter-based stream (see DeviceProcessData)."""

    augment = True

    def __init__(self, aug_together_args, aug_pc2_args, data_process_args, num_points, allow_less_points=False, seed=None,
                 device='cuda'):
        super(DeviceAugmentation, self).__init__(data_process_args, num_points, allow_less_points, seed, device)
        self.together_args = aug_together_args
        self.pc2_args = aug_pc2_args

    def params(self):
        p = super(DeviceAugmentation, self).params()
        tg, p2, rng = self.together_args, self.pc2_args, self.rng
        scale = np.diag(rng.uniform(tg['scale_low'], tg['scale_high'], 3).astype(np.float32))
        m = scale.dot(_rot_y(rng.uniform(-tg['degree_range'], tg['degree_range']), np.float32).T)
        shift = rng.uniform(-tg['shift_range'], tg['shift_range'], (1, 3)).astype(np.float32)
        m2 = _rot_y(rng.uniform(-p2['degree_range'], p2['degree_range']), np.float32)
        shift2 = rng.uniform(-p2['shift_range'], p2['shift_range'], (1, 3)).astype(np.float32)
        p.m[:] = m.ravel().tolist()
        p.shift[:] = shift.ravel().tolist()
        p.m2[:] = m2.ravel().tolist()
        p.shift2[:] = shift2.ravel().tolist()
        p.jitter_sigma1, p.jitter_clip1 = float(tg['jitter_sigma']), float(tg['jitter_clip'])
        p.jitter_sigma2, p.jitter_clip2 = float(p2['jitter_sigma']), float(p2['jitter_clip'])
        return p

    def __repr__(self):
        fmt = lambda d: ''.join('\t%-10s %s\n' % (k, d[k]) for k in sorted(d))      # noqa: E731
        return ('%s\n(together_args: \n%s\npc2_args: \n%s\ndata_process_args: \n\tDEPTH_THRESHOLD: %s\n'
                '\tNO_CORR: %s\n\tallow_less_points: %s\n\tnum_points: %s\n\tdevice: %s\n)' % (
                    self.__class__.__name__, fmt(self.together_args), fmt(self.pc2_args), self.DEPTH_THRESHOLD,
                    self.no_corr, self.allow_less_points, self.num_points, self.runner.device))


def _leaf_dirs(root):
    """Sorted directories below `root` that contain no sub-directory (the reference's `useful_paths`)."""
    root = os.path.realpath(os.path.expanduser(root))
    return sorted(d for d, sub, _ in os.walk(root) if len(sub) == 0)


class _PairFolder(object):
    """Common part: list of sample directories, transform, tensors on `device`."""

    canonical = None        # expected number of leaf directories, for check_counts()
    has_cameras = False     # whether samples carry a camera (the 2D metrics need one)

    def __init__(self, transform, device='cuda'):
        self.transform = transform
        self.device = device
        self.samples = []

    def __len__(self):
        return len(self.samples)

    def point_counts(self, index):
        """(N1, N2) of a sample without loading it, when the transform fixes them (allow_less_points off: every sample it
        passes has num_points in each cloud -- the training protocol); else the shapes of the loaded sample."""
        t = self.transform
        t = getattr(t, 'sampler', t)
        if t is not None and not getattr(t, 'allow_less_points', True):
            return (t.num_points, t.num_points)
        s_ = self[index]
        return (int(s_[0].shape[-1]), int(s_[1].shape[-1]))

    def check_counts(self):
        """None if the tree has the canonical number of samples, else a message."""
        if self.canonical is not None and self._found != self.canonical:
            return '%s: found %d sample directories, the published split has %d' % (
                self.__class__.__name__, self._found, self.canonical)
        return None

    def load(self, path):
        raise NotImplementedError

    def _load_pair(self, path):
        """The frame's two [n, 3] float32 clouds as the processed tree stores them (the raw readers compute them instead)."""
        return np.load(os.path.join(path, 'pc1.npy')), np.load(os.path.join(path, 'pc2.npy'))

    def camera_of(self, path):
        """The camera of the frame in directory `path`, None if the reader has none."""
        return None

    def size_of(self, path):
        """The (H, W) of the raw maps of the frame in directory `path`, None if the reader never saw them."""
        return None

    def __getitem__(self, index):
        """-> (pc1, pc2, sf) float32 device tensors (3, N); falls on to the next sample if the
        transform rejects this one (the reference draws a random replacement, :44-47)."""
        on_device = getattr(self.transform, 'on_device', False)
        for k in range(len(self.samples)):
            path = self.samples[(index + k) % len(self.samples)]
            if on_device:           # a device transform returns the Sample itself, or (None, None, None) on a rejection
                out = self.transform(self.load(path))
                if out[0] is not None:
                    s_ = out if isinstance(out, Sample) else Sample(out)
                    s_.camera, s_.frame, s_.size = self.camera_of(path), os.path.basename(path), self.size_of(path)
                    return s_
                continue
            out = self.transform(self.load(path)) if self.transform is not None else None
            if out is None:
                pc1, pc2 = self.load(path)
                out = (pc1, pc2, pc2 - pc1)
            if out[0] is not None:
                s_ = Sample(torch.from_numpy(np.ascontiguousarray(a[:, :3].T, dtype=np.float32)).to(self.device) for a in out)
                s_.camera, s_.frame, s_.size = self.camera_of(path), os.path.basename(path), self.size_of(path)
                return s_
        raise RuntimeError('no usable sample under %s' % self.root)


class FlyingThings3DSubset(_PairFolder):
    has_cameras = True

    def __init__(self, train, transform, data_root, full=False, device='cuda'):
        super(FlyingThings3DSubset, self).__init__(transform, device)
        self.train = train
        self.canonical = 19640 if train else 3824
        dirs = self._sample_dirs(data_root)
        self._found = len(dirs)
        self.samples = dirs if full else dirs[::4]
        if not self.samples:
            raise RuntimeError('Found 0 files in subfolders of: ' + self.root)

    def _sample_dirs(self, data_root):
        self.root = os.path.join(data_root, 'FlyingThings3D_subset_processed_35m', 'train' if self.train else 'val')
        return _leaf_dirs(self.root)

    def load(self, path):
        pc1, pc2 = self._load_pair(path)
        for pc in (pc1, pc2):           # the subset stores x and z with the opposite sign
            pc[..., 0] *= -1
            pc[..., -1] *= -1
        return pc1, pc2

    def camera_of(self, path):
        return FT3D_CAMERA


class KITTI(_PairFolder):
    canonical = 200

    #: the keyword arguments of flownet.remove_ground that `ground` may hold
    GROUND_KEYS = ('up', 'max_tilt_deg', 'hyps', 'tau', 'refine', 'cut')
    #: the keys `outlier` may hold: the arguments of ops.outlier_filter, and flownet.remove_outliers' `by`
    OUTLIER_KEYS = ('mode', 'k', 'radius', 'std_ratio', 'min_neighbors', 'by')

    def __init__(self, transform, data_root, remove_ground=True, mapping_file=None, device='cuda', calib_dir=None, ground=None,
                 voxel=None, voxel_mode='centroid', fps=None, outlier=None):
        """remove_ground: True -- the reference's rule, a correspondence is dropped when y < -1.4 in both clouds --, False, or
        'plane': the same pair rule on a plane fitted to each cloud on the device (flownet.remove_ground(corr=True, seed=0,
        call=<frame number>, **ground), DESIGN.md §21: a frame's result does not depend on the order of reading).
        voxel (None: off): after the ground removal and before the transform samples its points, the pair is put on a voxel
        grid of that edge on the device (flownet.voxel_downsample(corr=True, voxel=voxel, mode=voxel_mode)):
        one correspondence per occupied cell of pc1.
        fps (None: off): after the ground removal and the voxel grid and before the transform, the pair is sampled to `fps`
        correspondences by farthest point sampling on the device (flownet.fps_sample(corr=True, num_points=fps));
        a frame of fewer distinct positions keeps that many.
        outlier (None: off; a dict of OUTLIER_KEYS): after the ground removal and before the voxel grid, the stray points are
        removed on the device (flownet.remove_outliers(corr=True, **outlier)): by default a correspondence is
        dropped when it is an outlier in either cloud."""
        from . import _lib, ops
        super(KITTI, self).__init__(transform, device)
        if outlier is not None:
            if torch.device(device).type != 'cuda':
                raise _lib.HplError('KITTI: outlier filters on the device, got device %s (there is no CPU fallback)' % (device,))
            if not isinstance(outlier, dict) or set(outlier) - set(self.OUTLIER_KEYS):
                raise _lib.HplError('KITTI: outlier holds %s, got %r' % (', '.join(self.OUTLIER_KEYS), outlier))
            if outlier.get('by', 'either') not in ('either', 'pc1'):
                raise _lib.HplError('KITTI: outlier[\'by\'] = %r (\'either\' or \'pc1\')' % (outlier['by'],))
            ops.outlier_args('KITTI: outlier', outlier.get('mode', 'statistical'), outlier.get('k', 16), outlier.get('radius', 1.0),
                             outlier.get('std_ratio', 2.0), outlier.get('min_neighbors'))
            outlier = dict(outlier)
        self.outlier = outlier
        if fps is not None:
            if torch.device(device).type != 'cuda':
                raise _lib.HplError('KITTI: fps samples on the device, got device %s (there is no CPU fallback)' % (device,))
            ops.fps_args('KITTI: fps', fps, 1)
        self.fps = fps
        if voxel is not None:
            if torch.device(device).type != 'cuda':
                raise _lib.HplError('KITTI: voxel downsamples on the device, got device %s (there is no CPU fallback)' % (device,))
            if voxel_mode not in ops.VOXEL_MODES:
                raise _lib.HplError('KITTI: voxel_mode = %r (%s)' % (voxel_mode, ' or '.join(repr(m) for m in ops.VOXEL_MODES)))
            ops.voxel_args('KITTI', voxel, (0, 0, 0), voxel_mode)
        elif voxel_mode != 'centroid':
            raise _lib.HplError('KITTI: voxel_mode applies to voxel=<edge>')
        self.voxel, self.voxel_mode = voxel, voxel_mode
        if remove_ground not in (True, False, 'plane'):
            raise _lib.HplError('KITTI: remove_ground = %r (True, False or \'plane\')' % (remove_ground,))
        self.ground = dict(ground or {})
        if remove_ground == 'plane':
            if torch.device(device).type != 'cuda':
                raise _lib.HplError('KITTI: remove_ground=\'plane\' fits on the device, got device %s (there is no CPU fallback)' % (device,))
            bad = sorted(set(self.ground) - set(self.GROUND_KEYS))
            if bad:
                raise _lib.HplError('KITTI: ground holds %s, got %s' % (', '.join(self.GROUND_KEYS), bad))
        elif self.ground:
            raise _lib.HplError('KITTI: ground applies to remove_ground=\'plane\'')
        self.remove_ground = remove_ground
        dirs = self._sample_dirs(data_root)
        self._found = len(dirs)
        if mapping_file is not None:
            with open(mapping_file) as fd:
                lines = [ln.strip() for ln in fd.readlines()]
            dirs = [d for d in dirs if lines[int(os.path.split(d)[-1])] != '']
        self.samples = dirs
        if not self.samples:
            raise RuntimeError('Found 0 files in subfolders of: ' + self.root)
        self.cameras = None
        if calib_dir is not None:
            names = [os.path.basename(d) for d in dirs]
            missing = [nm for nm in names if not os.path.isfile(os.path.join(calib_dir, nm + '.txt'))]
            if missing:
                raise FileNotFoundError('%s has no calibration for %d frame(s): %s' % (
                    calib_dir, len(missing), ', '.join(nm + '.txt' for nm in missing[:20]) + (' ...' if len(missing) > 20 else '')))
            self.cameras = {nm: read_kitti_camera(os.path.join(calib_dir, nm + '.txt')) for nm in names}
        self.has_cameras = self.cameras is not None

    def camera_of(self, path):
        return self.cameras[os.path.basename(path)] if self.cameras is not None else None

    def _sample_dirs(self, data_root):
        self.root = os.path.join(data_root, 'KITTI_processed_occ_final')
        return _leaf_dirs(self.root)

    def load(self, path):
        pc1, pc2 = self._load_pair(path)
        if self.remove_ground == 'plane':
            from .flownet import remove_ground
            name = os.path.basename(path)
            frame = int(name) if name.isdigit() else self.samples.index(path)
            t1, t2 = (torch.from_numpy(np.ascontiguousarray(p[:, :3].T, dtype=np.float32)).to(self.device) for p in (pc1, pc2))
            keep = remove_ground(t1, t2, corr=True, return_mask=True, seed=0, call=frame, **self.ground)[-1][0]
            pc1, pc2 = pc1[keep], pc2[keep]
        elif self.remove_ground:
            keep = ~((pc1[:, 1] < -1.4) & (pc2[:, 1] < -1.4))
            pc1, pc2 = pc1[keep], pc2[keep]
        if self.outlier is not None:
            from .flownet import remove_outliers
            t1, t2 = (torch.from_numpy(np.ascontiguousarray(p[:, :3].T, dtype=np.float32)).to(self.device) for p in (pc1, pc2))
            keep = remove_outliers(t1, t2, corr=True, return_mask=True, **self.outlier)[-1][0]
            pc1, pc2 = pc1[keep], pc2[keep]
        if self.voxel is not None:
            from .flownet import voxel_downsample
            t1, t2 = (torch.from_numpy(np.ascontiguousarray(p[:, :3].T, dtype=np.float32)).to(self.device) for p in (pc1, pc2))
            v1, v2 = voxel_downsample(t1, t2, voxel=self.voxel, mode=self.voxel_mode, corr=True)[:2]
            pc1, pc2 = (np.ascontiguousarray(v[0].t().cpu().numpy()) for v in (v1, v2))
        if self.fps is not None:
            from .flownet import fps_sample
            t1, t2 = (torch.from_numpy(np.ascontiguousarray(p[:, :3].T, dtype=np.float32)).to(self.device) for p in (pc1, pc2))
            f1, f2 = fps_sample(t1, t2, num_points=self.fps, corr=True)[:2]
            pc1, pc2 = (np.ascontiguousarray(f[0].t().cpu().numpy()) for f in (f1, f2))
        return pc1, pc2


def _saved(cloud):
    """A (3, n) device cloud as the [n, 3] float32 host array the reference's scripts save."""
    return np.ascontiguousarray(cloud.t().cpu().numpy())


def _need_device(who, device):
    if torch.device(device).type != 'cuda':
        from . import _lib
        raise _lib.HplError('%s back-projects its frames on the device, got device %s (there is no CPU fallback)' % (who, device))


#: the directories of a raw FlyingThings3D-subset split and their files' extensions, as process_flyingthings3d_subset.py:33-38
#: names them: disparity, its occlusions, disparity change, flow, its occlusions
FT3D_RAW_LAYOUT = ((('disparity', 'left'), '.pfm'), (('disparity_occlusions', 'left'), '.png'),
                   (('disparity_change', 'left', 'into_future'), '.pfm'), (('flow', 'left', 'into_future'), '.flo'),
                   (('flow_occlusions', 'left', 'into_future'), '.png'))


def read_ft3d_raw_frame(split_root, name):
    """(disparity, disparity change, flow, disparity occlusions, flow occlusions) of frame `name` below a raw split directory,
    in the order flownet.frames_from_ft3d takes them."""
    paths = [os.path.join(split_root, *parts) + os.sep + name + ext for parts, ext in FT3D_RAW_LAYOUT]
    disp, occ1, dchange, flow, occ2 = read_pfm(paths[0]), read_png(paths[1]), read_pfm(paths[2]), read_flo(paths[3]), read_png(paths[4])
    for p, o in ((paths[1], occ1), (paths[4], occ2)):
        if o.dtype != np.uint8 or o.ndim != 2:
            raise ValueError('%s: an occlusion mask is an 8-bit greyscale PNG, got %s %s' % (p, o.dtype, o.shape))
    return disp, dchange, flow, occ1, occ2


def read_kitti_raw_frame(raw_root, name):
    """(disp_occ_0, disp_occ_1, flow_occ) raw values of KITTI scene-flow frame `name` (NNNNNN) below `raw_root`/training."""
    out = []
    for sub, shape in (('disp_occ_0', 2), ('disp_occ_1', 2), ('flow_occ', 3)):
        p = os.path.join(raw_root, 'training', sub, name + '_10.png')
        x = read_png(p)
        if x.dtype != np.uint16 or x.ndim != shape:
            raise ValueError('%s: %s is a 16-bit %s PNG, got %s %s' % (p, sub, 'greyscale' if shape == 2 else 'RGB', x.dtype, x.shape))
        out.append(x)
    return tuple(out)


def _listed(directory, ext):
    if not os.path.isdir(directory):
        raise FileNotFoundError('%s is not a directory' % directory)
    return sorted(f[:-len(ext)] for f in os.listdir(directory) if f.endswith(ext))


def _missing(paths, what):
    gone = [p for p in paths if not os.path.isfile(p)]
    if gone:
        raise FileNotFoundError('%s: %d file(s) missing: %s' % (what, len(gone), ', '.join(gone[:8]) + (' ...' if len(gone) > 8 else '')))


class FlyingThings3DRaw(FlyingThings3DSubset):
    """FlyingThings3DSubset over the RAW subset: `raw_root`/{train,val}/ holding the five directories of FT3D_RAW_LAYOUT.  Every
    frame is back-projected on the device when it is read (flownet.frames_from_ft3d) and yields exactly what
    FlyingThings3DSubset yields for the tree process_flyingthings3d_subset.py would have written -- with --only_save_near_pts
    for near=-35. (the published FlyingThings3D_subset_processed_35m), without it for near=None."""

    def __init__(self, train, transform, raw_root, near=-35., full=False, device='cuda'):
        _need_device('FlyingThings3DRaw', device)
        self.near = near
        super(FlyingThings3DRaw, self).__init__(train, transform, raw_root, full=full, device=device)

    def _sample_dirs(self, raw_root):
        self.root = os.path.join(raw_root, 'train' if self.train else 'val')
        lead, ext = FT3D_RAW_LAYOUT[2]
        names = _listed(os.path.join(self.root, *lead), ext)           # (the reference lists disparity_change, :66-67)
        _missing([os.path.join(self.root, *parts) + os.sep + nm + e for nm in names for parts, e in FT3D_RAW_LAYOUT],
                 'FlyingThings3DRaw: ' + self.root)
        return [os.path.join(self.root, nm) for nm in names]       # (no directories: a sample's path only carries its name)

    def _load_pair(self, path):
        from .flownet import frames_from_ft3d
        pc1, pc2 = frames_from_ft3d([read_ft3d_raw_frame(self.root, os.path.basename(path))], near=self.near, device=self.device)[:2]
        return _saved(pc1[0]), _saved(pc2[0])


class KITTIRaw(KITTI):
    """KITTI over the RAW scene-flow download: `raw_root`/training/{disp_occ_0,disp_occ_1,flow_occ}/NNNNNN_10.png and the frames'
    calib_cam_to_cam files in `calib_dir` (NNNNNN.txt; they also give the cameras of the 2D metrics).  Every frame is
    back-projected on the device when it is read (flownet.frames_from_kitti) and yields exactly what KITTI yields
    for the tree process_kitti.py would have written; the keywords are KITTI's."""

    def __init__(self, transform, raw_root, calib_dir, remove_ground=True, mapping_file=None, device='cuda', ground=None,
                 voxel=None, voxel_mode='centroid', fps=None, outlier=None):
        _need_device('KITTIRaw', device)
        if calib_dir is None or not os.path.isdir(calib_dir):
            raise FileNotFoundError('KITTIRaw: calib_dir %r is not a directory (the back-projection needs every frame\'s P_rect_02)' % (calib_dir,))
        super(KITTIRaw, self).__init__(transform, raw_root, remove_ground=remove_ground, mapping_file=mapping_file, device=device,
                                       calib_dir=calib_dir, ground=ground, voxel=voxel, voxel_mode=voxel_mode, fps=fps,
                                       outlier=outlier)
        self.P = {nm: read_kitti_P(os.path.join(calib_dir, nm + '.txt')) for nm in (os.path.basename(d) for d in self.samples)}
        self.sizes = {}                              # (H, W) of every frame loaded so far

    def size_of(self, path):
        return self.sizes.get(os.path.basename(path))

    def _sample_dirs(self, raw_root):
        self.root = os.path.join(raw_root, 'training')
        names = [nm[:-3] for nm in _listed(os.path.join(self.root, 'disp_occ_0'), '.png') if nm.endswith('_10')]
        _missing([os.path.join(self.root, sub, nm + '_10.png') for nm in names for sub in ('disp_occ_1', 'flow_occ')],
                 'KITTIRaw: ' + self.root)
        return [os.path.join(self.root, nm) for nm in names]       # (no directories: a sample's path only carries its number)

    def _load_pair(self, path):
        from .flownet import frames_from_kitti
        name = os.path.basename(path)
        raw = read_kitti_raw_frame(os.path.dirname(self.root), name)
        self.sizes[name] = tuple(raw[0].shape)
        pc1, pc2 = frames_from_kitti([raw + (self.P[name],)], device=self.device)[:2]
        return _saved(pc1[0]), _saved(pc2[0])
