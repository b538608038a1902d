"""The refusals of the point-cloud wrappers (ops.* and their flownet.* callers) as one table.

Per op: the good calls -- keyword arguments at the smallest shapes the op takes (N = 10 points, M = 12 in a second cloud, Q = 5
queries, frames of 2 x 3 and 1 x 4 pixels; '' is B = 1, 'b2' two clouds, further variants where a rule needs one; a variant
named '~..' is no good call itself but one argument short of its row, where an earlier rule would otherwise fire first) -- and the bad
rows.  A row changes ONE argument of a good call and names it.  What a row must raise:

  wrapper  HplError whose text starts with the Python op's name (`says_op`) and not with 'hpl_' -- the wrapper refused, not
           the library -- and holds the words the text uses for the argument (`says`, by default the argument's name);
  lib      the C entry's to refuse on purpose (an output over an input, a non-finite viewpoint, the resident capacity of fps,
           and the values only the entry looks at): HplError whose text starts with 'hpl_';
  widened  wrapper, since the wrappers share one scalar rule; before that a bare ValueError / TypeError of float().

cpu=True: the rule fires before any tensor is looked at (or the caller touches no device at all), so the row also runs on
host tensors, without a GPU.

Not in the table: the negative answer of an hpl_*_workspace_bytes.  It needs B > 64 or N >= 2^31 / 3; _prefix refuses the first
with its own text before the room is asked for (every wrapper but knn_interpolate, which has no room), and the second needs a
2.1 G-point cloud.  The test_workspace_bytes tests of the ops hold the entries' answers.
Nor the two lib refusals of fps that need more than the smallest shapes (a cloud past the resident capacity, an output over the
wide buffer its input is a view of): tests/test_gpu_fps.py holds them.

`python tests/refusals.py` prints one line per row: op | row | exception type | text."""
import collections

import numpy as np
import torch

NAN, INF = float('nan'), float('inf')
BIG = (2 ** 31 + 2) // 3

Row = collections.namedtuple('Row', 'arg value label base says kind cpu')
Op = collections.namedtuple('Op', 'name fn says_op goods rows')


def R(arg, value, label=None, base='', says=None, kind='wrapper', cpu=False):
    return Row(arg, value, label or '%s=%r' % (arg, value), base, arg if says is None else says, kind, cpu)


class T(object):
    """A zero tensor made on the test's device when the call is built: host=True keeps it on the host, grad=True makes it
    require grad, view(t) takes a view of it."""

    def __init__(self, *shape, **kw):
        self.shape, self.kw = shape, kw

    def __call__(self, dev):
        kw = dict(self.kw)
        host, grad, view = kw.pop('host', False), kw.pop('grad', False), kw.pop('view', None)
        t = torch.zeros(*self.shape, device='cpu' if host else dev, **kw)
        if view is not None:
            t = view(t)
        return t.requires_grad_() if grad else t

    def __repr__(self):
        return 'T%r%s' % (self.shape, ''.join(' %s' % k for k in sorted(self.kw)))


class Same(object):
    """The good call's own tensor of another argument (an output laid over an input)."""

    def __init__(self, arg):
        self.arg = arg

    def __repr__(self):
        return 'the %s tensor' % self.arg


def resolve(v, dev):
    if isinstance(v, T):
        return v(dev)
    if isinstance(v, (list, tuple)) and any(isinstance(x, (T, list, tuple)) for x in v):
        return type(v)(resolve(x, dev) for x in v)
    return v


def build(op, row, dev, base=''):
    """(function, keyword arguments) of a row's call (row None: the good call `base`)."""
    import hplflownet_amd as H
    from hplflownet_amd import flownet, ops
    kw = {k: resolve(v, dev) for k, v in op.goods[row.base if row else base].items()}
    if row is not None:
        kw[row.arg] = kw[row.value.arg] if isinstance(row.value, Same) else resolve(row.value, dev)
    mod, name = op.fn.split('.')
    return getattr({'ops': ops, 'flownet': flownet, 'H': H}[mod], name), kw


F64, I32, U8, U16 = torch.float64, torch.int32, torch.uint8, torch.uint16
EYE = T(1, 3, 3, view=lambda t: t + torch.eye(3, device=t.device))
P_OK = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003]], np.float32)


def prefix_rows(arg, n, says=None, base=''):
    """The rows of one _prefix rule: too short, not from 0, decreasing, more than 65 entries."""
    return [R(arg, [0, 4], base=base, says=says), R(arg, [1, n], base=base, says=says),
            R(arg, [0, n + 2, n], base=base, says=says), R(arg, [0] * 65 + [n], '%s of 66 entries' % arg, base=base, says=says)]


def cloud_rows(arg, n=10, base=''):
    """The rows of one _soa3 operand."""
    return [R(arg, T(3, n, dtype=F64), base=base), R(arg, T(n, 3), base=base), R(arg, T(3, n, grad=True), base=base),
            R(arg, T(1, 3, n), base=base), R(arg, T(3, n, host=True), base=base), R(arg, None, base=base)]


def flow_rows(n=10):
    return [R('flow', T(n, 3, dtype=F64)), R('flow', T(n - 1, 3)), R('flow', T(n, 3, grad=True)), R('flow', T(n, 3, host=True)),
            R('flow', None)]


def vec_rows(arg, n=10, base=''):
    """The rows of an (N,) float32 vector on the cloud's device without grad."""
    return [R(arg, T(n - 1), base=base), R(arg, T(n, host=True), base=base), R(arg, T(n, dtype=F64), base=base),
            R(arg, T(n, grad=True), base=base), R(arg, 'x', base=base)]


def rows_out(n=10, base=''):
    """The rows of a contiguous [N, 3] out."""
    return [R('out', T(n, 3, host=True), base=base), R('out', T(3, n), base=base), R('out', T(n, 3, dtype=F64), base=base),
            R('out', T(n, 6, view=lambda t: t[:, :3]), 'out=a column slice', base=base), R('out', T(n, 3, grad=True), base=base)]


def soa_out_rows(n=10, arg='out', base=''):
    """The rows of a (3, n) out with unit stride along its points."""
    return [R(arg, T(3, n, host=True), base=base), R(arg, T(n, 3), base=base), R(arg, T(3, n, dtype=F64), base=base),
            R(arg, T(3, 2 * n, view=lambda t: t[:, ::2]), '%s=every second column' % arg, base=base),
            R(arg, T(3, n, grad=True), base=base), R(arg, 'x', base=base)]


def attrs_rows(n=10):
    return [R('attrs', T(n, 2)), R('attrs', T(2, n, dtype=F64)), R('attrs', T(2, n, host=True)), R('attrs', T(9, n)),
            R('attrs', T(0, n)), R('attrs', T(n)), R('attrs', 'x'), R('attrs', T(2, n, grad=True))]


def scalar_rows(arg, zero_ok=False, inf_ok=False, widened=True):
    rows = [R(arg, NAN, cpu=True), R(arg, -1.0, cpu=True)]
    rows.append(R(arg, -INF, cpu=True) if inf_ok else R(arg, INF, cpu=True))
    if not zero_ok:
        rows.append(R(arg, 0.0, cpu=True))
    kind = 'widened' if widened else 'wrapper'
    return rows + [R(arg, 'x', kind=kind, cpu=True), R(arg, None, kind=kind, cpu=True)]


def int_rows(arg, lo, hi):
    return [R(arg, lo - 1, cpu=True), R(arg, hi + 1, cpu=True), R(arg, float(lo), cpu=True), R(arg, True, cpu=True)]


PC, PC2 = T(3, 10), T(3, 12)
_pair_forms = [                         # the rows voxel_downsample and fps_sample share (host tensors do: no device is touched)
    R('pc2', T(3, 9), says='corr=True', cpu=True), R('sf', T(3, 9), cpu=True), R('pc2', [PC, PC], says='as many clouds', cpu=True),
    R('sf', T(3, 9), 'sf=T(3, 9) without pc2', base='alone', cpu=True), R('pc1', T(10, 3), cpu=True), R('pc1', [], cpu=True),
    R('pc1', T(3), cpu=True), R('pc1', [None], cpu=True), R('pc2', T(2, 10), cpu=True), R('sf', 'x', cpu=True),
    R('pc1', [PC] * 33, 'pc1=33 clouds, corr=False', base='~free33', says='1 .. 32', cpu=True),
    R('pc1', [PC] * 65, 'pc1=65 clouds', base='~joint65', says='1 .. 64', cpu=True),
    R('pc1', [PC] * 65, 'pc1=65 clouds alone', base='alone', says='1 .. 64', cpu=True)]
_pair_goods = {'': dict(pc1=PC, pc2=PC, sf=PC), 'alone': dict(pc1=PC), 'free': dict(pc1=PC, pc2=PC2, corr=False),
               '~free33': dict(pc1=[PC] * 32, pc2=[PC] * 33, corr=False), '~joint65': dict(pc1=[PC] * 64, pc2=[PC] * 65)}
_KITTI = dict(disp1=T(10, dtype=U16), disp2=T(10, dtype=U16), flow=T(10, 3, dtype=U16), P=[P_OK, P_OK], heights=[2, 1], widths=[3, 4])
_FT3D = dict(disp=T(10), dchange=T(10), flow=T(10, 2), occ1=T(10, dtype=U8), occ2=T(10, dtype=U8), heights=[2, 1], widths=[3, 4])
_sizes_rows = [R('widths', [3, 4, 5], says='heights and widths', cpu=True), R('heights', [], says='heights and widths', cpu=True),
               R('heights', [-1, 1], says='heights and widths', cpu=True), R('heights', None, says='heights and widths', cpu=True),
               R('heights', [1] * 65, 'heights=65 frames', says='heights and widths', cpu=True),
               R('widths', [3, 2 ** 31], says='heights and widths', cpu=True)]
_frame = (np.zeros((2, 3), np.uint16), np.zeros((2, 3), np.uint16), np.zeros((2, 3, 3), np.uint16), P_OK)


def _pair_out_rows():
    return [R('out', T(3, 10), says='out'), R('out', 'x'), R('out', (T(3, 10), T(3, 10, host=True))),
            R('out', (T(3, 10), T(3, 20, view=lambda t: t[:, ::2])), 'out=(.., every second column)'),
            R('out', (T(3, 10), T(3, 10, grad=True))), R('out', (T(3, 10), T(3, 9)))]


OPS = [
    Op('knn_interpolate', 'ops.knn_interpolate', 'knn_interpolate',
       {'': dict(ref=PC, values=T(10, 3), q=T(3, 5), k=3),
        'b2': dict(ref=PC, values=T(10, 3), q=T(3, 5), ref_prefix=[0, 5, 10], q_prefix=[0, 2, 5]),
        'blend': dict(ref=PC, values=T(10, 3), q=T(3, 5), out=T(5, 3), coverage=T(5))},
       [R('k', 0, cpu=True), R('k', 9, cpu=True), R('k', 3.0, cpu=True), R('k', True, cpu=True),
        R('eps', -1.0, kind='lib'), R('eps', NAN, kind='lib')] + cloud_rows('ref')[:5] + [R('q', T(3, 5, dtype=F64)), R('q', T(3, 5, grad=True))] + [
        R('values', T(10, 3, grad=True)), R('values', T(9, 3)), R('values', T(10, 3, dtype=F64)), R('values', T(10, 3, host=True)),
        R('values', T(10, 17), kind='lib'), R('ref_prefix', [0, 4, 10], says='prefixes'), R('q_prefix', [0, 4], base='b2', says='prefixes'),
        R('ref_prefix', [0, 5, 9], base='b2', says='prefixes'),
        R('ref_prefix', [0, 12, 10], base='b2', kind='lib'), R('ref_prefix', [0, 0, 10], base='b2', kind='lib'),
        R('out', T(5, 3), 'out without coverage'), R('coverage', T(5), 'coverage without out'), R('out', T(5, 4), base='blend'),
        R('out', T(5, 3, grad=True), base='blend'), R('coverage', T(4), base='blend'), R('coverage', T(5, host=True), base='blend')]),
    Op('rigid_fit', 'ops.rigid_fit', 'rigid_fit',
       {'': dict(pc=PC, flow=T(10, 3)), 'b2': dict(pc=PC, flow=T(10, 3), prefix=[0, 4, 10])},
       int_rows('iters', 0, 16) + scalar_rows('tau') + cloud_rows('pc') + flow_rows() + vec_rows('weight') + prefix_rows('prefix', 10) +
       [R('prefix', [0, 12, 10], base='b2')] + rows_out()),
    Op('icp', 'ops.icp', 'icp',
       {'': dict(src=PC, dst=PC2), 'b2': dict(src=PC, dst=PC2, src_prefix=[0, 5, 10], dst_prefix=[0, 6, 12]),
        'plane': dict(src=PC, dst=PC2, metric='plane', dst_normal=T(3, 12)),
        'init': dict(src=PC, dst=PC2, init=(EYE, T(1, 3)), iters=2)},
       [R('metric', 'line', cpu=True), R('metric', 'plane', 'metric=plane without dst_normal', says='dst_normal', cpu=True),
        R('dst_normal', T(3, 12), 'dst_normal with metric=point', cpu=True)] + int_rows('iters', 0, 64) + [R('iters', 1.0, cpu=True)] +
       scalar_rows('max_dist') + scalar_rows('tau') + scalar_rows('tol_rot', True) + scalar_rows('tol_trans', True) +
       cloud_rows('src') + cloud_rows('dst', 12)[:5] +
       [R('dst_normal', T(3, 11), base='plane'), R('dst_normal', T(3, 12, host=True), base='plane'),
        R('dst_normal', T(3, 12, dtype=F64), base='plane'),
        R('dst_normal', T(12, 3), base='plane'), R('dst_normal', T(3, 12, grad=True), base='plane'), R('iters', 65, base='plane')] +
       vec_rows('weight') + prefix_rows('src_prefix', 10, 'prefix of src') + prefix_rows('dst_prefix', 12, 'prefix of dst') +
       [R('src_prefix', [0, 12, 10], base='b2', says='prefix of src'), R('dst_prefix', [0, 13, 12], base='b2', says='prefix of dst'),
        R('dst_prefix', [0, 6, 12], says='prefixes'), R('src_prefix', [0, 5, 10], says='prefixes'),
        R('init', EYE), R('init', (EYE, T(1, 3, host=True))), R('init', (T(1, 3, 3, dtype=F64), T(1, 3))), R('init', (T(3, 3), T(3))),
        R('init', (EYE, T(1, 3)), base='b2'), R('init', (T(1, 3, 3, grad=True), T(1, 3))), R('init', (EYE, T(1, 3), T(1, 3))), R('init', 'x')] +
       rows_out()),
    Op('normals', 'ops.normals', 'normals',
       {'': dict(pc=PC, k=3), 'b2': dict(pc=PC, k=3, prefix=[0, 5, 10])},
       int_rows('k', 3, 32) + [R('k', 16.0, cpu=True)] + scalar_rows('radius') + cloud_rows('pc') + prefix_rows('prefix', 10) +
       [R('viewpoint', (0.0, 1.0)), R('viewpoint', [[0, 0, 0], [1, 1, 1]]), R('viewpoint', 'up'), R('viewpoint', [[0, 0, 0]] * 3, base='b2'),
        R('viewpoint', [[0, 0, 0], [0, NAN, 0]], base='b2', kind='lib')] + soa_out_rows() + [R('out', Same('pc'), kind='lib')]),
    Op('motion_segment', 'ops.motion_segment', 'motion_segment',
       {'': dict(pc=PC, flow=T(10, 3), residual=T(10)), 'b2': dict(pc=PC, flow=T(10, 3), residual=T(10), prefix=[0, 4, 10])},
       scalar_rows('tau', widened=False) + scalar_rows('eps', widened=False) + scalar_rows('dv', inf_ok=True, widened=False) +
       int_rows('min_points', 1, 2 ** 31 - 1) + [R('min_points', 2.0, cpu=True)] + int_rows('max_objects', 1, 4096) +
       cloud_rows('pc') + flow_rows() + vec_rows('residual')[:4] +
       [R('residual', None)] + prefix_rows('prefix', 10) + [R('prefix', [0, 12, 10], base='b2')] +
       [R('out', T(10, dtype=I32, host=True)), R('out', T(10)), R('out', T(9, dtype=I32)),
        R('out', T(20, dtype=I32, view=lambda t: t[::2]), 'out=every second entry'), R('out', 'x')]),
    Op('ground_min_cos', 'ops.ground_min_cos', 'ground_fit', {'': dict(max_tilt_deg=20.0)},
       [R('max_tilt_deg', 90.0, cpu=True), R('max_tilt_deg', -1.0, cpu=True), R('max_tilt_deg', NAN, cpu=True)]),
    Op('ground_fit', 'ops.ground_fit', 'ground_fit',
       {'': dict(pc=PC, hyps=4), 'b2': dict(pc=PC, hyps=4, prefix=[0, 4, 10])},
       int_rows('hyps', 1, 1024) + int_rows('refine', 0, 8) + scalar_rows('tau') + scalar_rows('cut', True) +
       [R('max_tilt_deg', 90.0, cpu=True), R('max_tilt_deg', -1.0, cpu=True), R('max_tilt_deg', NAN, cpu=True),
        R('up', (0, 0, 0), cpu=True), R('up', (0, 1), cpu=True), R('up', (0, NAN, 1), cpu=True), R('up', 1.0, cpu=True),
        R('seed', -1, cpu=True), R('seed', 1.0, cpu=True), R('call', 1 << 64, cpu=True)] + cloud_rows('pc') + prefix_rows('prefix', 10) +
       [R('prefix', [0, 12, 10], base='b2')]),
    Op('voxel_args', 'ops.voxel_args', 'who', {'': dict(who='who', voxel=0.1, origin=(0, 0, 0), mode='centroid')},
       [R('voxel', v, cpu=True) for v in (0.0, -1.0, NAN, INF, 1e39, 1e-50, 'x', True, None)] +
       [R('origin', v, cpu=True) for v in ((0, 0), (0, NAN, 0), (0, 0, INF), (1e39, 0, 0), None, (0, 'x', 0))] +
       [R('mode', v, cpu=True) for v in ('mean', 0, None)]),
    Op('voxel_downsample', 'ops.voxel_downsample', 'voxel_downsample',
       {'': dict(pc=PC, attrs=T(2, 10)), 'b2': dict(pc=PC, prefix=[0, 4, 10])},
       [R('voxel', 0.0, cpu=True), R('voxel', 'x', cpu=True), R('origin', (0, 0), cpu=True), R('mode', 'mean', cpu=True)] +
       cloud_rows('pc') + attrs_rows() + prefix_rows('prefix', 10) + [R('prefix', [0, 12, 10], base='b2')] + soa_out_rows() +
       [R('out', Same('pc'), kind='lib')]),
    Op('fps_args', 'ops.fps_args', 'who', {'': dict(who='who', m=4, batch=1, path='auto')},
       [R('m', v, says='samples', cpu=True) for v in (0, -3, True, 2.0, '4', None, BIG)] +
       [R('m', BIG // 64 + 1, base='b64', says='samples', cpu=True)] + [R('path', v, cpu=True) for v in ('fast', 1, None)]),
    Op('fps', 'ops.fps', 'fps',
       {'': dict(pc=PC, m=4, attrs=T(2, 10)), 'b2': dict(pc=PC, m=4, prefix=[0, 4, 10]), 'b2e': dict(pc=PC, m=4, prefix=[0, 0, 10])},
       cloud_rows('pc') + attrs_rows() + prefix_rows('prefix', 10) + [R('prefix', [0, 12, 10], base='b2')] +
       [R('m', 0, says='samples'), R('m', 2.0, says='samples'), R('m', BIG, says='samples'), R('path', 'fast'),
        R('start', [0, 0]), R('start', [10]), R('start', [-1]), R('start', [1.0]), R('start', [True]), R('start', 3), R('start', [0], base='b2'),
        R('start', [0, 6], base='b2'), R('start', [4, 0], base='b2'), R('start', [5, 10], base='b2e')] +
       soa_out_rows(4) + [R('out', T(3, 4), base='b2')]),
    Op('frames_from_kitti', 'ops.frames_from_kitti', 'frames_from_kitti', {'': _KITTI},
       _sizes_rows + [R('disp1', T(10, dtype=U16, host=True), cpu=True), R('disp1', T(9, dtype=U16)), R('disp2', T(10)),
                      R('disp2', T(10, dtype=U16, host=True)), R('flow', T(10, 2, dtype=U16)), R('flow', None),
                      R('P', [P_OK], 'P=one matrix'), R('P', 'x'), R('P', [P_OK[:2], P_OK[:2]], 'P=two (2, 4) matrices')] + _pair_out_rows() +
       [R('out', T(3, 21, view=lambda t: (t[:, :10], t[:, 9:19])), 'out=two views that overlap', kind='lib')]),
    Op('frames_from_ft3d', 'ops.frames_from_ft3d', 'frames_from_ft3d', {'': _FT3D},
       _sizes_rows + [R('disp', T(10, host=True), cpu=True), R('disp', T(10, dtype=F64)), R('dchange', T(9)), R('flow', T(10, 3)),
                      R('occ1', T(10)), R('occ2', T(10, dtype=U8, host=True)), R('dchange', T(10, grad=True)), R('near', NAN)] + _pair_out_rows()),
    Op('selfsup_loss', 'ops.selfsup_loss', 'selfsup_loss',
       {'': dict(pc1=PC, flow=T(10, 3), pc2=PC2), 'b2': dict(pc1=PC, flow=T(10, 3), pc2=PC2, prefix1=[0, 5, 10], prefix2=[0, 6, 12]),
        'nograd': dict(pc1=PC, flow=T(10, 3), pc2=PC2, need_grad=False)},
       [R('k', -1, cpu=True), R('k', 9, cpu=True), R('k', 2.0, cpu=True), R('k', True, cpu=True), R('k', 0, 'k=0 with w_smooth=1', cpu=True)] +
       [R('w_chamfer', v, says='weights', cpu=True) for v in (-1.0, INF, NAN, 'x', None)] +
       [R('w_smooth', v, says='weights', cpu=True) for v in (-1.0, INF, NAN, 'x')] +
       cloud_rows('pc1') + cloud_rows('pc2', 12)[:5] +
       [R('flow', T(10, 3, dtype=F64)), R('flow', T(9, 3)), R('flow', T(10, 3, host=True)),
        R('flow', T(10, 3, grad=True), says='flow requires grad')] + prefix_rows('prefix1', 10) + prefix_rows('prefix2', 12) +
       [R('prefix1', [0, 5, 10], says='prefix1 lists'), R('prefix2', [0, 13, 12], base='b2')] +
       rows_out() + [R('out', T(10, 3), 'out without need_grad', base='nograd')]),
    # ------------------------------------------------------------------------- the flownet callers
    Op('rigid_refine', 'flownet.rigid_refine', 'rigid_refine',
       {'': dict(pc1=PC, flow=PC), 'list': dict(pc1=[PC], flow=[PC]), 'batch': dict(pc1=T(2, 3, 10), flow=T(2, 3, 10))},
       [R('flow', [PC], says='flow are both lists', cpu=True), R('flow', [PC, PC], base='list', says='flow are both lists', cpu=True),
        R('pc1', [], base='list', says='pc1 and flow', cpu=True), R('lat_or_counts', [4, 5], base='list', says='counts', cpu=True),
        R('flow', T(3, 3, 10), base='batch', says='flow', cpu=True), R('flow', T(3, 20), base='batch', says='flow', cpu=True),
        R('lat_or_counts', [4, 5], says='counts', cpu=True), R('lat_or_counts', [11, -1], says='counts', cpu=True)]),
    Op('segment_motion', 'flownet.segment_motion', 'segment_motion', {'': dict(pc1=PC, flow=PC)},
       [R('flow', [PC], says='flow are both lists', cpu=True), R('rigid', (1, 2, 3, 4), cpu=True), R('rigid', 'x', cpu=True)]),
    Op('icp_register', 'flownet.icp_register', 'icp_register',
       {'': dict(pc1=PC, pc2=PC2), 'list': dict(pc1=[PC, PC], pc2=[PC2, PC2])},
       [R('pc1', [], cpu=True), R('pc1', [None], cpu=True), R('pc2', T(3), cpu=True), R('pc2', None, cpu=True),
        R('pc2', [PC2], base='list', cpu=True), R('lat_or_counts', [4, 5], says='counts', cpu=True),
        R('lat_or_counts', ([4, 6], [6, 7]), says='counts', cpu=True), R('lat_or_counts', [10, 10], base='list', says='counts', cpu=True),
        R('lat_or_counts', ([10, 10], [12, 11]), base='list', says='pc2', cpu=True),
        R('metric', 'line', cpu=True), R('normals', T(3, 12), says='metric', cpu=True)]),
    Op('estimate_normals', 'flownet.estimate_normals', 'estimate_normals',
       {'': dict(pc=PC, k=3), 'list': dict(pc=[PC, PC], k=3)},
       [R('lat_or_counts', [7, 2], says='counts', cpu=True), R('pc', T(10), cpu=True), R('pc', [], cpu=True),
        R('lat_or_counts', [10, 9], base='list', says='counts', cpu=True)]),
    Op('remove_ground', 'flownet.remove_ground', 'remove_ground',
       {'': dict(pc1=PC, pc2=PC, sf=PC, hyps=4), 'free': dict(pc1=PC, pc2=PC2, corr=False, hyps=4), '~pairs33': dict(pc1=[PC] * 32, pc2=[PC] * 33)},
       [R('pc2', T(3, 9), says='corr=True', cpu=True), R('sf', T(3, 9), cpu=True), R('pc2', [PC, PC], says='as many clouds', cpu=True),
        R('return_votes', True, says='optional outputs', cpu=True), R('return_height', True, says='optional outputs', cpu=True),
        R('return_mask', True, base='free', cpu=True), R('pc1', T(10, 3), cpu=True), R('pc1', [], cpu=True), R('pc2', None, cpu=True),
        R('pc1', [PC] * 33, 'pc1=33 clouds', base='~pairs33', says='1 .. 32', cpu=True)]),
    Op('voxel_downsample (flownet)', 'flownet.voxel_downsample', 'voxel_downsample', _pair_goods,
       _pair_forms + [R('voxel', 0.0, cpu=True), R('voxel', NAN, cpu=True), R('mode', 'median', cpu=True), R('origin', (0, 0), cpu=True)]),
    Op('fps_sample', 'flownet.fps_sample', 'fps_sample',
       {k: dict(v, num_points=4) for k, v in _pair_goods.items()},
       _pair_forms + [R('num_points', v, says='samples', cpu=True) for v in (0, 2.5, True, BIG)] +
       [R('seed', 1, 'seed with start', base='start', says='start and seed', cpu=True), R('seed', -1, cpu=True), R('seed', 1.5, cpu=True),
        R('seed', True, cpu=True)]),
    Op('frames_from_kitti (flownet)', 'flownet.frames_from_kitti', 'frames_from_kitti', {'': dict(frames=[_frame])},
       [R('frames', [], cpu=True), R('frames', 'x', cpu=True), R('frames', [(np.zeros((2, 3), np.uint16),)], 'frames=a tuple of one array', cpu=True),
        R('frames', [(np.zeros(6, np.uint16),) * 4], 'frames=flat arrays', says='frame', cpu=True),
        R('frames', [_frame[:2] + (np.zeros((2, 3, 2), np.uint16), P_OK)], 'frames=a (H, W, 2) flow', says='frame', cpu=True),
        R('frames', [(np.zeros((2, 3), np.float32),) + _frame[1:]], 'frames=a float32 disparity', says='frame', cpu=True)]),
    Op('selfsup_loss (flownet)', 'flownet.selfsup_loss', 'selfsup_loss',
       {'': dict(flow=PC, pc1=PC, pc2=PC2), 'list': dict(flow=[PC, PC], pc1=[PC, PC], pc2=[PC2, PC2]),
        'batch': dict(flow=T(2, 3, 10), pc1=T(2, 3, 10), pc2=T(2, 3, 12))},
       [R('pc2', [PC2], base='list', cpu=True), R('pc2', T(1, 3, 12), cpu=True), R('pc2', T(3, 3, 12), base='batch', cpu=True),
        R('pc2', T(3, 12), base='batch', cpu=True), R('pc2', None, cpu=True), R('flow', [PC], says='flow are both lists', cpu=True)]),
]
for _op in OPS:                     # the variants that only some rows need
    if _op.name == 'fps_args':
        _op.goods['b64'] = dict(_op.goods[''], batch=64)
    if _op.name == 'fps_sample':
        _op.goods['start'] = dict(_op.goods[''], start=[0])

ROWS = [(op, row) for op in OPS for row in op.rows]
CPU_ROWS = [(op, row) for op, row in ROWS if row.cpu]
WIDENED = [(op, row) for op, row in ROWS if row.kind == 'widened']


def row_id(op_row):
    return '%s-%s' % (op_row[0].name, op_row[1].label)


def run_good_calls(op, dev):
    """Every good call of an op, as it stands."""
    for base in op.goods:
        if not base.startswith('~'):
            fn, kw = build(op, None, dev, base)
            fn(**kw)


def outcome(op, row, dev):
    """(exception or None, its text) of a row's call."""
    fn, kw = build(op, row, dev)
    try:
        fn(**kw)
    except Exception as e:                                  # noqa: BLE001 (the table reports whatever comes)
        return e, str(e)
    return None, ''


def verdict(op, row, dev):
    """None when the row's call is refused as the table says, else what is wrong with it."""
    from hplflownet_amd import _lib
    e, text = outcome(op, row, dev)
    if not isinstance(e, _lib.HplError):
        return 'raised %r, not HplError' % (e,)
    if row.kind == 'lib':
        return None if text.startswith('hpl_') else 'the library is to refuse this, got: %s' % text
    if text.startswith('hpl_') or not text.startswith(op.says_op):
        return 'the text does not start with %r: %s' % (op.says_op, text)
    if str(row.says) not in text:
        return 'the text does not name %r: %s' % (row.says, text)
    return None


def dump():
    """One line per row -- op | row | exception type | text -- after the good calls have run (without a GPU: the cpu rows)."""
    device = 'cuda' if torch.cuda.is_available() else 'cpu'
    if device == 'cuda':
        for o in OPS:
            run_good_calls(o, device)
        torch.cuda.synchronize()
    for o, r in (ROWS if device == 'cuda' else CPU_ROWS):
        exc, msg = outcome(o, r, device)
        print('%s | %s | %s | %s' % (o.name, r.label, type(exc).__name__, msg.replace('\n', ' ')))


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump()
