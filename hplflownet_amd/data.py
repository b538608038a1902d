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
           'read_kitti_camera']

#: (f, cx, cy, constx, consty, constz) of every FlyingThings3D frame (utils/geometry.py:59 defaults)
FT3D_CAMERA = (-1050.0, 479.5, 269.5, 0.0, 0.0, 0.0)


class Sample(tuple):
    """(pc1, pc2, sf) of a reader, with `camera`: the (f, cx, cy, constx, consty, constz) of the frame it came from, or None."""
    camera = None


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

    def camera_of(self, path):
        """The camera of the frame in directory `path`, None if the reader has none."""
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
                    s_.camera = self.camera_of(path)
                    return s_
                continue
            out = self.transform(self.load(path)) if self.transform is not None else None
            if out is None:
                pc1, pc2 = self.load(path)
                out = (pc1, pc2, pc2 - pc1)
            if out[0] is not None:
                s_ = Sample(torch.from_numpy(np.ascontiguousarray(a[:, :3].T, dtype=np.float32)).to(self.device) for a in out)
                s_.camera = self.camera_of(path)
                return s_
        raise RuntimeError('no usable sample under %s' % self.root)


class FlyingThings3DSubset(_PairFolder):
    has_cameras = True

    def __init__(self, train, transform, data_root, full=False, device='cuda'):
        super(FlyingThings3DSubset, self).__init__(transform, device)
        self.train = train
        self.root = os.path.join(data_root, 'FlyingThings3D_subset_processed_35m', 'train' if train else 'val')
        self.canonical = 19640 if train else 3824
        dirs = _leaf_dirs(self.root)
        self._found = len(dirs)
        self.samples = dirs if full else dirs[::4]
        if not self.samples:
            raise RuntimeError('Found 0 files in subfolders of: ' + self.root)

    def load(self, path):
        pc1 = np.load(os.path.join(path, 'pc1.npy'))
        pc2 = np.load(os.path.join(path, 'pc2.npy'))
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

    def __init__(self, transform, data_root, remove_ground=True, mapping_file=None, device='cuda', calib_dir=None, ground=None,
                 voxel=None, voxel_mode='centroid'):
        """remove_ground: True -- the reference's rule, a correspondence is dropped when y < -1.4 in both clouds --, False, or
        'plane': the same pair rule on a plane fitted to each cloud on the device (flownet.remove_ground(corr=True, seed=0,
        call=<frame number>, **ground), DESIGN.md §21: a frame's result does not depend on the order of reading).
        voxel (None: off): after the ground removal and before the transform samples its points, the pair is put on a voxel
        grid of that edge on the device (flownet.voxel_downsample(corr=True, voxel=voxel, mode=voxel_mode)):
        one correspondence per occupied cell of pc1."""
        from . import _lib, ops
        super(KITTI, self).__init__(transform, device)
        if voxel is not None:
            if torch.device(device).type != 'cuda':
                raise _lib.HplError('KITTI: voxel downsamples on the device, got device %s (there is no CPU fallback)' % (device,))
            if voxel_mode not in ops.VOXEL_MODES:
                raise _lib.HplError('KITTI: voxel_mode = %r (%s)' % (voxel_mode, ' or '.join(repr(m) for m in ops.VOXEL_MODES)))
            ops.voxel_args('KITTI', voxel, (0, 0, 0), voxel_mode)
        elif voxel_mode != 'centroid':
            raise _lib.HplError('KITTI: voxel_mode applies to voxel=<edge>')
        self.voxel, self.voxel_mode = voxel, voxel_mode
        self.root = os.path.join(data_root, 'KITTI_processed_occ_final')
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
        dirs = _leaf_dirs(self.root)
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

    def load(self, path):
        pc1 = np.load(os.path.join(path, 'pc1.npy'))
        pc2 = np.load(os.path.join(path, 'pc2.npy'))
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
        if self.voxel is not None:
            from .flownet import voxel_downsample
            t1, t2 = (torch.from_numpy(np.ascontiguousarray(p[:, :3].T, dtype=np.float32)).to(self.device) for p in (pc1, pc2))
            v1, v2 = voxel_downsample(t1, t2, voxel=self.voxel, mode=self.voxel_mode, corr=True)[:2]
            pc1, pc2 = (np.ascontiguousarray(v[0].t().cpu().numpy()) for v in (v1, v2))
        return pc1, pc2
