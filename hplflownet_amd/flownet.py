"""Model assembly on top of the HIP bilateral layers: HPLFlowNet and HPLFlowNetShallow.

Own counterpart of the reference's callers of the hot path:
same module names, hence the same state_dict keys and shapes as
/root/reference/models/HPLFlowNet.py:11-236 and models/HPLFlowNet_shallow.py:11-169
(checked against tests/golden/state_dict.json), same forward signature
`model(pc1, pc2, generated_data) -> (1, 3, N)`.  The wiring is table driven instead of
spelled out layer by layer, runs channel-last end to end, and replaces every torch.cat of
the reference forward by writes into column slices of one buffer per layer input.

Level L (0-based) hosts bcn{L+1} (Down, shared by both clouds), bcn{L+1}_ (Up) and, for
L >= 2, corr{L-1}.
"""
import collections
import ctypes
import os
import weakref

import torch
import torch.nn as nn

from . import _lib, ops
from .bcl import (BilateralConvFlex, BilateralCorrelationFlex, Conv1dReLU, NbrTable, _ConvReLU, _conv_of, pointwise_conv,
                  to_channel_first, to_channel_last)

__all__ = ['HPLFlowNet', 'HPLFlowNetShallow', 'DeviceLattice', 'PairBlur', 'DenseFlow', 'rigid_refine', 'icp_register', 'estimate_normals', 'segment_motion']


# ----------------------------------------------------------------------------- lattice container
class _Level(object):
    # pair / emg_pair: both clouds as one (ops.PairTables, el_minus_gr [N0+N1, 4]); None when the
    # lattice came from the reference's per-cloud wire format
    __slots__ = ('clouds', 'blur', 'emg', 'corr1', 'corr2', 'H', 'pair', 'emg_pair')

    def __init__(self):
        self.pair = None
        self.emg_pair = None


class PairBlur(object):
    """Blur tables of the two clouds of a level as ONE int32 table [F, H0+H1]: columns [0,H0) are
    cloud 1's vertices, columns [H0,H0+H1) cloud 2's with neighbour ids shifted by H0 (so the table
    indexes the pair's stacked feature matrix).  Behaves like the list [blur1, blur2]:
    [0] is a zero-copy view, [1] (cloud 2's own numbering) is materialised on first use."""

    def __init__(self, table, H0):
        self.pair = NbrTable(table)
        self.H0 = H0
        self._own = [NbrTable(table[:, :H0]), None]

    def __len__(self):
        return 2

    def __getitem__(self, i):
        if i == 1 and self._own[1] is None:
            t = self.pair.t[:, self.H0:]
            self._own[1] = NbrTable(torch.where(t >= 0, t - self.H0, t).contiguous())
            self._own[1]._sym = self.pair._sym
        return self._own[i]

    def __iter__(self):
        return iter((self[0], self[1]))


class DeviceLattice(object):
    """`generated_data` resident on the device in kernel-ready form:
    int32 tables, CSR of each splat, channel-last el_minus_gr.  Built either from the
    reference's list of dicts (host or device tensors, with or without the B=1 dimension
    added by default_collate) or directly by hplflownet_amd.lattice on the GPU."""

    def __init__(self, levels, wide_up=None):
        self.levels = levels
        #: hint from the consumer (model.lattice_hint()), one entry per level (or one value for all): True = the Up
        #: conv of that level is wide enough to run as tap-group passes (the single-pass row order of its table is
        #: never used), False = it is not (the group orders are never used), None = unknown: prepare() builds both
        self.wide_up = wide_up

    def prepare(self, for_training=False):
        """Build every lazily constructed table (CSRs, tap orders, symmetry verdicts) now, on the
        current stream, so that a lattice built on a side stream is complete before it is handed to
        the forward.  for_training: the tables of the per-cloud path + the symmetry read-back."""
        self.prepare_tables(for_training)
        if for_training:
            self.resolve_symmetry()
        return self

    def prepare_tables(self, for_training=False):
        """The launches of prepare() without its read-back (lattice.LatticeBuild overlaps that one)."""
        for L, lv in enumerate(self.levels):
            if lv.pair is not None:
                lv.pair.csr()       # one build; the per-cloud CSRs are views / offset copies of it
            if lv.pair is not None and isinstance(lv.blur, PairBlur):
                # the Down layers run once per pair; cloud 1 alone is splatted only by the correlation
                # layers that take a previous correlation (levels >= 3) and sliced by the Up layers
                tables = [lv.blur.pair, lv.blur[0], lv.corr1]
                if for_training:
                    lv.clouds[0].csr()
            else:
                for c in lv.clouds:
                    c.csr()
                tables = list(lv.blur) + [lv.corr1]
            up = lv.blur[0] if isinstance(lv.blur, PairBlur) else None
            wide = self.wide_up[L] if isinstance(self.wide_up, (list, tuple)) else self.wide_up
            grouped = up is not None and wide is not False and up.groups() is not None   # multi-pass row orders
            if grouped:
                up.group_tiles()
            for tbl in tables:
                if tbl is not None and not (tbl is up and grouped and wide and tbl is not lv.corr1):
                    tbl.perm_tiles          # (builds the row order first)
        return self

    def symmetry_begin(self):
        """Launch the symmetry checks of every blur / corr1 table not decided yet and start the copy of
        their flags to pinned memory -> (todo, event or None); symmetry_finish(todo) after the event."""
        todo = []
        for lv in self.levels:
            tables = [lv.corr1]
            if isinstance(lv.blur, PairBlur):
                tables += [lv.blur.pair]
            else:
                tables += list(lv.blur)
            for t in tables:
                if t is not None and t._sym is None and t.t.shape[0] == 15 and all(t is not u for u, _ in todo):
                    todo.append((t, ops.table_symmetry_flag(t.t)))
        if not todo:
            return (todo, None), None
        flags = torch.cat([f for _, f in todo])
        host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
        host.copy_(flags, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record()
        return (todo, host), landed

    def symmetry_finish(self, begun):
        todo, host = begun
        if todo:
            for (t, _), v in zip(todo, host.tolist()):
                t._sym = bool(v)
        for lv in self.levels:
            if isinstance(lv.blur, PairBlur):            # the per-cloud views inherit the pair's verdict
                for i in (0, 1):
                    if lv.blur._own[i] is not None and lv.blur._own[i]._sym is None:
                        lv.blur._own[i]._sym = lv.blur.pair._sym
        return self

    def resolve_symmetry(self):
        """Decide `symmetric` of every blur / corr1 table that has not been checked yet with ONE host
        read-back (the backward picks the mirrored-gather or the atomic-scatter form from it)."""
        begun, landed = self.symmetry_begin()
        if landed is not None:
            landed.synchronize()
        return self.symmetry_finish(begun)

    @staticmethod
    def from_generated_data(gd, device):
        levels = []
        for d in gd:
            lv = _Level()

            def t(key):
                v = d[key]
                v = torch.as_tensor(v)
                return v.to(device, non_blocking=True)

            def cnt(key):
                v = d[key]
                return int(v.reshape(-1)[0].item()) if torch.is_tensor(v) else int(v)

            lv.H = (cnt('pc1_hash_cnt'), cnt('pc2_hash_cnt'))
            lv.clouds, lv.blur, lv.emg = [], [], []
            for ci, nm in enumerate(('pc1', 'pc2')):
                bary = t(nm + '_barycentric').reshape(4, -1).float()
                off = t(nm + '_lattice_offset').reshape(4, -1)
                lv.clouds.append(ops.CloudTables(bary, off, lv.H[ci]))
                bl = t(nm + '_blur_neighbors')
                lv.blur.append(NbrTable(ops.narrow(bl.reshape(-1, lv.H[ci]))) if bl.numel() > 1 else None)
                if lv.blur[-1] is not None:      # the same sparsity rule as a device-built lattice (tap groups only where most slots are empty)
                    lv.blur[-1].vertices_per_point = lv.H[ci] / float(max(1, bary.shape[1]))
                lv.emg.append(t(nm + '_el_minus_gr').reshape(4, -1).float().t().contiguous())
            c1 = t('pc1_corr_indices')
            if c1.numel() > 1:
                lv.corr1 = NbrTable(ops.narrow(c1.reshape(-1, lv.H[0])))
                c2 = t('pc2_corr_indices')
                c2 = c2.reshape(-1, lv.corr1.t.shape[0], lv.H[0])
                lv.corr2 = NbrTable(ops.corr2_permute(c2))
                lv.corr2._sym = False
            else:
                lv.corr1 = lv.corr2 = None
            levels.append(lv)
        return DeviceLattice(levels)


def _assemble(rows, parts, device):
    """Concatenate channel blocks into one [rows, sum C] matrix.  A part is (C, tensor) or
    (C, callable(out_view) -> tensor), or (4, 'ones'): the constant part 1, 0, 0, 0 of a folded bias (inference only).
    Without autograd the blocks are written in place (no cat copy for callables); with autograd this is a plain torch.cat."""
    if torch.is_grad_enabled():
        return torch.cat([src(None) if callable(src) else src for _, src in parts], dim=1)
    total = sum(c for c, _ in parts)
    buf = torch.empty((rows, total), dtype=torch.float32, device=device)
    col = 0
    for c, src in parts:
        view = buf[:, col:col + c]
        if callable(src):
            src(view)
        elif isinstance(src, str):
            view.zero_()
            view[:, 0].fill_(1.0)
        else:
            view.copy_(src)
        col += c
    return buf


# ----------------------------------------------------------------------------- the two models
_PLANS = weakref.WeakKeyDictionary()        # model -> plan.ForwardPlan (kept outside the module: deepcopy / state_dict safe)
_FOLDS = weakref.WeakKeyDictionary()        # model -> {L: ops.FoldedWeight of the consumer of bcn{L+1}_}: they go with the model


class _FlowNetBase(nn.Module):
    """Shared wiring.  Subclasses define SPEC."""

    NLEV = None          # number of lattice levels
    DOWN = None          # num_output of every Down BCL
    CORR = None          # (num_corr_output, num_output) of every CorrBCL
    UP = None            # per level L: num_output of bcn{L+1}_
    REFINE = False       # corr{j}_refine Conv1d stacks (shallow model)
    HEAD_IN = None
    #: on a device-built lattice the Down path runs once per PAIR (both clouds stacked), in inference and
    #: in training; False forces the per-cloud path (what reference-format lattices use)
    pair_batched = True
    #: inference on a device-built lattice runs as ONE native call (plan.ForwardPlan: the same launches issued by
    #: csrc/executor.hip instead of ~130 Python round trips); False forces the Python path below
    native_forward = not os.environ.get('HPL_NO_NATIVE')
    #: DenseFlow.forward: a list the pair-batched inference path appends bcn1_'s vertex activation to (None: off)
    _dense_keep = None

    def __init__(self, args):
        super(_FlowNetBase, self).__init__()
        self.scales_filter_map = args.scales_filter_map
        assert len(self.scales_filter_map) == self.NLEV
        sfm = self.scales_filter_map
        dim, leaky = args.dim, args.use_leaky
        self.use_leaky = leaky
        chunk = -1 if getattr(args, 'evaluate', False) else 1024 * 1024 * 25
        self.chunk_size = chunk

        def bcl(n_in, n_out, radius, splat, slice_):
            return BilateralConvFlex(dim, radius, n_in, n_out, args.DEVICE, use_bias=args.bcn_use_bias,
                                     use_leaky=leaky, use_norm=args.bcn_use_norm, do_splat=splat,
                                     do_slice=slice_, last_relu=args.last_relu, chunk_size=chunk)

        self.conv1 = nn.Sequential(Conv1dReLU(dim, 32, use_leaky=leaky), Conv1dReLU(32, 32, use_leaky=leaky),
                                   Conv1dReLU(32, 64, use_leaky=leaky))
        feat = 64
        corr_dim = {}                     # channels of the (refined) correlation living at level L
        for L in range(self.NLEV):
            setattr(self, 'bcn%d' % (L + 1), bcl(feat + dim + 1, self.DOWN, sfm[L][1], True, False))
            if L >= 2:
                j = L - 1
                setattr(self, 'corr%d' % j, BilateralCorrelationFlex(
                    dim, sfm[L][2], sfm[L][3], feat, self.CORR[0], self.CORR[1], args.DEVICE,
                    use_bias=args.bcn_use_bias, use_leaky=leaky, use_norm=args.bcn_use_norm,
                    prev_corr_dim=0 if L == 2 else corr_dim[L - 1], last_relu=args.last_relu,
                    chunk_size=chunk))
                corr_dim[L] = self.CORR[1][-1]
                if self.REFINE:
                    c_in = corr_dim[L] + (dim + 1 if L + 1 < self.NLEV else 0)
                    setattr(self, 'corr%d_refine' % j, nn.Sequential(
                        Conv1dReLU(c_in, 64, use_leaky=leaky), Conv1dReLU(64, 64, use_leaky=leaky),
                        Conv1dReLU(64, 64, use_leaky=leaky)))
                    corr_dim[L] = 64
        up_out = None
        for L in reversed(range(self.NLEV)):
            if L == self.NLEV - 1:
                n_in = corr_dim[L] + feat
            else:
                n_in = dim + 1 + up_out + (corr_dim[L] if L >= 2 else 0) + feat
            setattr(self, 'bcn%d_' % (L + 1), bcl(n_in, self.UP[L], sfm[L][1], False, True))
            up_out = self.UP[L][-1]
        self.conv2 = Conv1dReLU(self.HEAD_IN, 1024, use_leaky=leaky)
        self.conv3 = Conv1dReLU(1024, 512, use_leaky=leaky)
        self.conv4 = nn.Conv1d(512, 3, kernel_size=1)

    def lattice_hint(self):
        """What this model needs of a lattice's lazily built tables (DeviceLattice.wide_up): per level, whether the
        Up conv that gathers through the level's blur table is wide enough for the tap-group passes."""
        from .bcl import GROUPS_MIN_CHANNELS
        return [getattr(self, 'bcn%d_' % (L + 1)).num_input >= GROUPS_MIN_CHANNELS for L in range(self.NLEV)]

    def fold_up(self):
        """True when the inference forward on a device-built lattice runs folded: every Up stack ends in a
        bias-only 1x1 conv behind at least one other conv, and HPL_FOLD_UP is not 0."""
        if not ops.FOLD_UP:
            return False
        for L in range(self.NLEV):
            layer = getattr(self, 'bcn%d_' % (L + 1))
            mods = list(layer.blur_conv)
            if not layer.do_slice or len(mods) < 2 or isinstance(mods[-1], _ConvReLU):
                return False
            w = mods[-1].weight
            if w.shape[0] != w.shape[1]:          # (the `up` block keeps its width: the layers' num_input stay what they are)
                return False
        return True

    def up_fold(self, L, ensure=True):
        """The folded weight of the consumer of Up layer bcn{L+1}_ (ops.FoldedWeight, current): L >= 1: of the 15-tap conv of
        bcn{L}_ (its `up` block behind el_minus_gr and, with a bias to carry, the ones part); L == 0: of conv2, with its bias.
        One per consumer, kept with the model; ensure=False: allocated, not computed (a program is emitted without a device)."""
        prod = getattr(self, 'bcn%d_' % (L + 1))
        tail = prod.blur_conv[-1]
        lb = prod.bias if prod.use_bias else None
        up_w = tail.weight.shape[0]
        if L == 0:
            c2 = self.conv2.conv
            src, args = (c2.weight, tail.weight, tail.bias, lb, c2.bias), (1, 0, up_w, -1, True)
        else:
            cons = _conv_of(getattr(self, 'bcn%d_' % L).blur_conv[0])
            ones = 4 if (tail.bias is not None or lb is not None) else -1
            src, args = (cons.weight, tail.weight, tail.bias, lb, None), (cons.weight.shape[2], 4, up_w, ones, False)
        mine = _FOLDS.setdefault(self, {})
        ent = mine.get(L)
        if ent is None or not ent.made_of(src, args):          # first use, or a parameter was replaced: new tensors
            ent = mine[L] = ops.FoldedWeight(src[0], args[0], args[1], args[2], src[1], src[2], src[3], args[3], src[4], args[4])
        return ent.ensure() if ensure else ent

    def forward_plan(self):
        """The native plan of this model's inference forward (built on first use, rebuilt when a parameter was
        replaced by a new tensor; in-place parameter updates only refresh its weight images)."""
        from .plan import ForwardPlan
        plan = _PLANS.get(self)
        if plan is None or not plan.fresh():
            plan = _PLANS[self] = ForwardPlan(self)
        return plan

    # -- helpers ------------------------------------------------------------------------
    def _stack(self, x, seq, out=None):
        mods = list(seq)
        for i, m in enumerate(mods):
            x = pointwise_conv(x, m.conv, True, self.use_leaky, out=out if i == len(mods) - 1 else None)
        return x

    def _corr(self, L, lat, feats, prev, corrs, dev):
        lv = lat.levels[L]
        j = L - 1
        c = getattr(self, 'corr%d' % j).forward_cl(feats[0], feats[1], prev,
                                                  lv.clouds[0] if prev is not None else None,
                                                  lv.corr1, lv.corr2)
        if self.REFINE:
            if L + 1 < self.NLEV:
                c = _assemble(c.shape[0], [(4, lat.levels[L + 1].emg[0]), (c.shape[1], c)], dev)
            c = self._stack(c, getattr(self, 'corr%d_refine' % j))
        corrs[L] = c
        return c

    def forward(self, pc1, pc2, generated_data):
        B = batch_of(pc1, pc2, generated_data, torch.is_grad_enabled(), self.pair_batched)
        ragged = isinstance(pc1, (list, tuple))          # lists of (3, N_b) clouds -> a list of B (1, 3, N1_b) flows
        if ragged and B == 1:
            return [self.forward(pc1[0][None], pc2[0][None], generated_data)]
        dev = pc1[0].device if ragged else pc1.device
        if not (pc1[0] if ragged else pc1).is_cuda:
            raise _lib.HplError('the HIP path needs device tensors (no CPU fallback)')
        native_lat = getattr(generated_data, 'device_lattice', None)       # lattice.NativeLattice
        # a natively built lattice lives in one arena, usually allocated on the lattice stream: tell the allocator that this
        # stream reads it, so that dropping the lattice right after the call cannot hand the memory to the next build early
        arena = getattr(generated_data, 'arena', None)
        if arena is None:
            arena = getattr(generated_data, '_arena', None)
        if arena is not None:
            arena.record_stream(torch.cuda.current_stream(dev))
        if self.native_forward and self.pair_batched and not torch.is_grad_enabled() and self._dense_keep is None and \
                (native_lat is not None or isinstance(generated_data, DeviceLattice)):
            plan = self.forward_plan()
            if plan.accepts(generated_data):
                return plan(pc1, pc2, generated_data)
        if native_lat is not None:
            generated_data = native_lat()
        lat = generated_data if isinstance(generated_data, DeviceLattice) else \
            DeviceLattice.from_generated_data(generated_data[:self.NLEV], dev)
        nlev = self.NLEV
        if torch.is_grad_enabled():
            lat.resolve_symmetry()
            if ops.BANK is not None:
                ops.BANK.refresh()          # all weight images of this step in one launch
        pair = self.pair_batched and \
            all(lv.pair is not None and isinstance(lv.blur, PairBlur) for lv in lat.levels[:nlev])
        down = [[], []]
        corrs = {}
        prev = None
        if pair and torch.is_grad_enabled():
            # the same stacked Down path written with autograd-visible ops (cat instead of in-place columns)
            y = self._stack(torch.cat([to_channel_last(pc1), to_channel_last(pc2)], dim=0), self.conv1)
            for L in range(nlev):
                lv = lat.levels[L]
                layer = getattr(self, 'bcn%d' % (L + 1))
                if L == 0 and (lv.clouds[0].N != pc1.shape[2] or lv.clouds[1].N != pc2.shape[2]):
                    raise _lib.HplError('lattice was built for %d / %d points, got %d / %d'
                                        % (lv.clouds[0].N, lv.clouds[1].N, pc1.shape[2], pc2.shape[2]))
                y = layer.forward_cl(torch.cat([lv.emg_pair, y], dim=1), lv.pair, lv.blur.pair, None)
                feats = [y[:lv.H[0]], y[lv.H[0]:]]
                down[0].append(feats[0])
                down[1].append(feats[1])
                if L >= 2:
                    prev = self._corr(L, lat, feats, prev, corrs, dev)
        elif pair:
            # Both clouds go through conv1 and the Down BCLs as ONE stacked matrix (cloud 2's points and
            # vertices behind cloud 1's; pair CSR, pair blur table): half the launches, and the output
            # of level L is written straight into columns [4, 4+C) of level L+1's input.
            feat_c = self.conv1[-1].conv.out_channels
            n0 = lat.levels[0].pair.N
            xin = torch.empty((n0, 3), dtype=torch.float32, device=dev)
            if ragged:          # a ragged batch: pair-major rows as well, every pair with its own counts
                t1 = sum(p.shape[1] for p in pc1)
                if lat.levels[0].clouds[0].N != t1 or lat.levels[0].clouds[1].N != n0 - t1:
                    raise _lib.HplError('ragged lattice was built for %d / %d points, got %d / %d'
                                        % (lat.levels[0].clouds[0].N, lat.levels[0].clouds[1].N, t1,
                                           sum(p.shape[1] for p in pc2)))
                torch.cat([p.t() for p in pc1], out=xin[:t1])
                torch.cat([p.t() for p in pc2], out=xin[t1:])
            elif lat.levels[0].clouds[0].N != B * pc1.shape[2] or lat.levels[0].clouds[1].N != B * pc2.shape[2]:
                raise _lib.HplError('lattice was built for %d / %d points, got %d / %d'
                                    % (lat.levels[0].clouds[0].N, lat.levels[0].clouds[1].N, B * pc1.shape[2],
                                       B * pc2.shape[2]))
            elif B > 1:           # a batch: pair-major rows, cloud 1 of every pair, then cloud 2 of every pair
                h = pc1.shape[2]
                xin[:B * h].view(B, h, 3).copy_(pc1.transpose(1, 2))
                xin[B * h:].view(B, pc2.shape[2], 3).copy_(pc2.transpose(1, 2))
            else:
                h = pc1.shape[2]
                xin[:h].copy_(to_channel_last(pc1))
                xin[h:].copy_(to_channel_last(pc2))
            x = torch.empty((n0, 4 + feat_c), dtype=torch.float32, device=dev)
            self._stack(xin, self.conv1, out=x[:, 4:])
            for L in range(nlev):
                lv = lat.levels[L]
                layer = getattr(self, 'bcn%d' % (L + 1))
                x[:, :4].copy_(lv.emg_pair)
                c_out = layer.num_output[-1]
                H0, Hp = lv.H[0], lv.pair.H
                nxt = torch.empty((Hp, 4 + c_out), dtype=torch.float32, device=dev) if L + 1 < nlev else None
                y = layer.forward_cl(x, lv.pair, lv.blur.pair, None, out=nxt[:, 4:] if nxt is not None else None)
                feats = [y[:H0], y[H0:]]
                down[0].append(feats[0])
                down[1].append(feats[1])
                x = nxt
                if L >= 2:
                    prev = self._corr(L, lat, feats, prev, corrs, dev)
        elif ragged:
            raise _lib.HplError('ragged batches need the pair-batched forward')
        else:
            feats = [self._stack(to_channel_last(pc1), self.conv1), self._stack(to_channel_last(pc2), self.conv1)]
            for L in range(nlev):
                lv = lat.levels[L]
                layer = getattr(self, 'bcn%d' % (L + 1))
                for ci in (0, 1):
                    cloud = lv.clouds[ci]
                    x = _assemble(cloud.N, [(4, lv.emg[ci]), (feats[ci].shape[1], feats[ci])], dev)
                    feats[ci] = layer.forward_cl(x, cloud, lv.blur[ci], None)
                    down[ci].append(feats[ci])
                if L >= 2:
                    prev = self._corr(L, lat, feats, prev, corrs, dev)
        # the folded form (the launches of plan.build_program(fold=True)): an Up layer runs conv15 -> slice and hands its
        # pre-1x1 rows down; its 1x1 and biases are in the weights of the conv that reads them
        fold = pair and not torch.is_grad_enabled() and self.fold_up()
        up = None        # callable(out_view) producing the previous Up output, or None
        up_c = 0
        wf = None        # folded: the ops.FoldedWeight the layer's 15-tap conv runs on
        for L in reversed(range(nlev)):
            lv = lat.levels[L]
            layer = getattr(self, 'bcn%d_' % (L + 1))
            if L == nlev - 1:
                parts = [(corrs[L].shape[1], corrs[L]), (down[0][L].shape[1], down[0][L])]
            else:
                parts = [(4, lat.levels[L + 1].emg[0])]
                if wf is not None and wf.args[3] >= 0:
                    parts.append((4, 'ones'))
                parts.append((up_c, up))
                if L >= 2:
                    parts.append((corrs[L].shape[1], corrs[L]))
                parts.append((down[0][L].shape[1], down[0][L]))
            x = _assemble(lv.H[0], parts, dev)

            def produce(out, layer=layer, x=x, lv=lv, keep=self._dense_keep if L == 0 else None,
                        w0=wf.weight if wf is not None else None):
                return layer.forward_cl(x, None, lv.blur[0], lv.clouds[0], out=out, keep=keep, w0=w0, folded=fold)
            up, up_c = produce, layer.num_output[-1]
            if fold:
                up_c = layer.blur_conv[-1].weight.shape[1]
                wf = self.up_fold(L)
        y = up(None)                                           # [N, HEAD_IN]; folded: bcn1_'s pre-1x1 rows
        if fold:
            y = ops.gconv(y, wf.weight, wf.bias, None, y.shape[0], 1, act=ops.ACT_LEAKY, bwd_mode='dense',
                          slope=ops.LEAKY_RATE if self.use_leaky else 0.0)
        else:
            y = pointwise_conv(y, self.conv2.conv, True, self.use_leaky)
        y = pointwise_conv(y, self.conv3.conv, True, self.use_leaky)
        y = pointwise_conv(y, self.conv4, False, self.use_leaky)
        if ragged:
            return ragged_flows(y, [p.shape[1] for p in pc1])
        if B > 1:
            return y.view(B, -1, y.shape[1]).transpose(1, 2)              # (B, 3, N1)
        return to_channel_first(y)


def ragged_flows(y, n1):
    """[sum N1_b, 3] flow of a ragged batch -> pair b's (1, 3, N1_b) flow, a view of rows [off_b, off_b + N1_b)."""
    out, o = [], 0
    for n in n1:
        out.append(y[o:o + n].t().unsqueeze(0))
        o += n
    return out


def batch_of(pc1, pc2, lat, grad, pair_batched=True):
    """Pairs of a forward (no launch): (1, 3, N) / (3, N) inputs take a single-pair lattice; (B, 3, N) inputs a lattice of
    lattice.GenerateDataUnsymmetric.build_native_batch with the same B, inference only (no autograd).  Two lists of B
    (3, N_b) clouds take the ragged lattice build_native_batch made of them (a list of one pair: a single-pair lattice)."""
    lb = int(getattr(lat, 'batch', 1) or 1)
    ragged = bool(getattr(lat, 'ragged', False))
    if isinstance(pc1, (list, tuple)) or isinstance(pc2, (list, tuple)):
        if not isinstance(pc1, (list, tuple)) or not isinstance(pc2, (list, tuple)):
            raise _lib.HplError('pc1 and pc2 are both lists of (3, N) clouds or both tensors')
        b = len(pc1)
        if len(pc2) != b:
            raise _lib.HplError('pc1 lists %d clouds, pc2 %d' % (b, len(pc2)))
        if b != lb or (b > 1 and not ragged):
            raise _lib.HplError('%d pairs of clouds in lists, but the lattice was built for %d%s (build_native_batch of the lists '
                                'builds a ragged batch)' % (b, lb, '' if ragged else ' of equal counts'))
        if any(not torch.is_tensor(p) or p.dim() != 2 or p.shape[0] != 3 for p in list(pc1) + list(pc2)):
            raise _lib.HplError('every cloud of a ragged batch is a (3, N) tensor')
        if ragged and [(int(p.shape[1]), int(q.shape[1])) for p, q in zip(pc1, pc2)] != [tuple(c) for c in lat.point_counts]:
            raise _lib.HplError('the ragged lattice was built for the point counts %s, got other clouds' % (lat.point_counts,))
        if b > 1 and grad:
            raise _lib.HplError('ragged batches are for inference: run the forward under torch.no_grad()')
        if b > 1 and not pair_batched:
            raise _lib.HplError('batched inference needs the pair-batched forward')
        return b
    if ragged:
        raise _lib.HplError('a ragged lattice takes the two lists of (3, N) clouds it was built from')
    b1 = int(pc1.shape[0]) if pc1.dim() == 3 else 1
    b2 = int(pc2.shape[0]) if pc2.dim() == 3 else 1
    if b1 != b2:
        raise _lib.HplError('pc1 holds %d clouds, pc2 %d' % (b1, b2))
    if b1 != lb:
        raise _lib.HplError('%d pairs of clouds, but the lattice was built for %d (build_native_batch builds a batch)' % (b1, lb))
    if b1 > 1 and grad:
        raise _lib.HplError('batched lattices are for inference: run the forward under torch.no_grad() (training takes one pair)')
    if b1 > 1 and not pair_batched:
        raise _lib.HplError('batched inference needs the pair-batched forward')
    return b1


class HPLFlowNet(_FlowNetBase):
    """7-level model: /root/reference/models/HPLFlowNet.py:11-430."""
    NLEV = 7
    DOWN = [64, 64]
    CORR = ([32, 32], [64, 64])
    UP = {6: [128, 128], 5: [128, 128], 4: [128, 128], 3: [256, 256], 2: [256, 256], 1: [512, 512],
          0: [1024, 1024]}
    REFINE = False
    HEAD_IN = 1024


class HPLFlowNetShallow(_FlowNetBase):
    """5-level model: /root/reference/models/HPLFlowNet_shallow.py:11-311."""
    NLEV = 5
    DOWN = [64]
    CORR = ([32], [32])
    UP = {4: [64], 3: [64], 2: [64], 1: [64], 0: [128]}
    REFINE = True
    HEAD_IN = 128


def load_reference_checkpoint(model, checkpoint, strict=True):
    """Load a checkpoint written by the reference (`main_utils.save_checkpoint`, main_utils.py:54-64:
    dict with 'state_dict' of the DataParallel-wrapped model, keys prefixed 'module.', main.py:104,122)
    or a bare state_dict into one of the models above.  `checkpoint` is a path or the loaded object."""
    obj = torch.load(checkpoint, map_location='cpu') if isinstance(checkpoint, str) else checkpoint
    sd = obj.get('state_dict', obj) if isinstance(obj, dict) else obj
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}
    return model.load_state_dict(sd, strict=strict)


# ----------------------------------------------------------------------------- rigid refinement
def _prefix_of(counts):
    """[0, c0, c0 + c1, ...]: where each cloud of a packed tensor starts, and the total."""
    prefix = [0]
    for c in counts:
        prefix.append(prefix[-1] + int(c))
    return prefix


def _stated_counts(lat_or_counts, total=None, cloud=None):
    """The points per pair that lat_or_counts states -- a ragged lattice: its point_counts (of the second cloud for cloud=1); an
    equal batch's lattice: total / batch; a sequence of counts; with `cloud` given also a pair (counts of pc1, counts of pc2)
    -- or None where it states none: None itself, and an equal batch's lattice without a total."""
    if lat_or_counts is None:
        return None
    if getattr(lat_or_counts, 'ragged', False):
        return [int(c[cloud or 0]) for c in lat_or_counts.point_counts]
    if hasattr(lat_or_counts, 'levels') or hasattr(lat_or_counts, 'batch'):
        b = int(getattr(lat_or_counts, 'batch', 1) or 1)
        return None if total is None else [total // b] * b
    if cloud is not None and len(lat_or_counts) == 2 and all(isinstance(c, (list, tuple)) for c in lat_or_counts):
        lat_or_counts = lat_or_counts[cloud]
    return [int(c) for c in lat_or_counts]


def _pair_counts(lat_or_counts, total, who='rigid_refine', cloud=None, what=''):
    """Points per pair of a packed cloud of `total` points, as _stated_counts reads them (nothing stated: one pair); what:
    ' of pc1', where the refusal has to say which cloud."""
    counts = _stated_counts(lat_or_counts, total, cloud)
    if counts is None:
        return [total]
    if sum(counts) != total or any(c < 0 for c in counts):
        raise _lib.HplError('%s: the point counts %s%s do not add up to %d points' % (who, counts, what, total))
    return counts


def _cloud_forms(x, who, what, rows3=False):
    """One cloud operand in the forms rigid_refine takes -> (clouds, form): the (3, N_b) views of its clouds, and form None for
    a (B, 3, N) tensor, False for a (3, N) one -- one cloud, or a packed (3, sum N_b) one whose counts the caller knows --,
    else a list's per-cloud flags (True: the entry came as (1, 3, N_b)).  rows3: every cloud must hold 3 rows here, and there
    must be one (the callers that lay clouds side by side before an op sees them)."""
    listed = isinstance(x, (list, tuple))
    if listed:
        form = [torch.is_tensor(c) and c.dim() == 3 for c in x]
        clouds = [c[0] if lead else c for c, lead in zip(x, form)]
    elif torch.is_tensor(x) and x.dim() == 3:
        clouds, form = [x[b] for b in range(x.shape[0])], None
    else:
        clouds, form = [x], False
    if (not clouds and (listed or rows3)) or any(not torch.is_tensor(c) or c.dim() != 2 or (rows3 and c.shape[0] != 3) for c in clouds):
        raise _lib.HplError(('%s: %s is a tensor or a non-empty list of (3, N_b) tensors' if listed and not rows3 else
                             '%s: %s is a (3, N) or (B, 3, N) tensor or a list of (3, N_b) tensors') % (who, what))
    return clouds, form


def _packed(x, clouds, form):
    """The (3, sum N_b) cloud of an operand _cloud_forms read: the operand itself or a view where it holds one cloud, else one
    copy."""
    if form is None and len(clouds) != 1:
        return x.transpose(0, 1).reshape(3, x.shape[0] * x.shape[2])
    return clouds[0] if len(clouds) == 1 else torch.cat(clouds, dim=1)


def _rows_as(rows, form, prefix):
    """The [sum N_b, 3] rows of a per-point result in the form of an operand: (B, 3, N) (form None), (3, N) (False) or a list of
    (3, N_b) / (1, 3, N_b) views (the flags of _cloud_forms)."""
    if form is None:
        return rows.view(len(prefix) - 1, prefix[1], 3).transpose(1, 2)
    if form is False:
        return rows.t()
    return [rows[prefix[b]:prefix[b + 1]].t().unsqueeze(0) if lead else rows[prefix[b]:prefix[b + 1]].t() for b, lead in enumerate(form)]


def _packed_rows(fls):
    """The [sum N_b, 3] tensor whose consecutive row blocks the (3, N_b) views `fls` are -- the flows of a ragged forward
    (ragged_flows) --, or None where they are anything else."""
    f0, off = fls[0], fls[0].storage_offset()
    for f in fls:
        if f.dtype != f0.dtype or f.device != f0.device or tuple(f.stride()) != (1, 3) or f.storage_offset() != off or \
                f.untyped_storage().data_ptr() != f0.untyped_storage().data_ptr():
            return None
        off += 3 * int(f.shape[1])
    return f0.as_strided(((off - f0.storage_offset()) // 3, 3), (3, 1), f0.storage_offset())


def _packed_pairs(pc1, flow, lat_or_counts, who):
    """The packed operands of ops.rigid_fit / ops.motion_segment for the forms the models take and return (rigid_refine's
    docstring lists them).  -> (pc (3, sum N_b), flow, prefix, counts, form): the form of `flow` as _rows_as takes it -- None for a
    (B, 3, N) pair of tensors, False for a packed pair, else the flags of a list.  (It reads its lists itself, not through
    _cloud_forms: the flows are packed as rows, in place where they are a ragged forward's.)"""
    if isinstance(pc1, (list, tuple)) or isinstance(flow, (list, tuple)):
        if not isinstance(pc1, (list, tuple)) or not isinstance(flow, (list, tuple)) or len(pc1) != len(flow) or not pc1:
            raise _lib.HplError('%s: pc1 and flow are both lists of as many clouds, or both tensors' % who)
        lead = [f.dim() == 3 for f in flow]
        pcs = [p[0] if p.dim() == 3 else p for p in pc1]
        fls = [f[0] if f.dim() == 3 else f for f in flow]
        counts = [int(p.shape[1]) for p in pcs]
        if lat_or_counts is not None and _pair_counts(lat_or_counts, sum(counts)) != counts:
            raise _lib.HplError('%s: the clouds hold %s points, the lattice or counts say otherwise' % (who, counts))
        pc = pcs[0] if len(pcs) == 1 else torch.cat(pcs, dim=1)
        fl = fls[0] if len(fls) == 1 else _packed_rows(fls)
        if fl is None:
            fl = torch.cat([f.t() for f in fls], dim=0)
        shape = lead
    elif pc1.dim() == 3:
        B, _, n = pc1.shape
        if flow.dim() != 3 or flow.shape[0] != B:
            raise _lib.HplError('%s: a (B, 3, N) cloud takes a (B, 3, N) flow' % who)
        counts = [int(n)] * B
        pc = pc1[0] if B == 1 else pc1.transpose(0, 1).reshape(3, B * n)
        fl = flow[0] if B == 1 else flow.transpose(1, 2).reshape(B * n, 3)       # (the forward's rows: a view)
        shape = None
    else:
        counts = _pair_counts(lat_or_counts, int(pc1.shape[1]))
        pc, fl, shape = pc1, flow, False
    return pc, fl, _prefix_of(counts), counts, shape


def rigid_refine(pc1, flow, lat_or_counts=None, **kw):
    """The rigid refinement of a forward's flow in ONE ops.rigid_fit call: per pair the robust rigid fit of
    (pc1, flow) and the flow with its inliers replaced by the rigid flow.  pc1 / flow as the models take and return them: a
    (B, 3, N) tensor pair (or (3, N): one pair), or two lists of B (3, N_b) / (1, 3, N_b) tensors (a ragged batch); a packed
    (3, sum N_b) cloud with its flow takes the pairs' counts from lat_or_counts (the forward's lattice, or a sequence of
    counts).  kw: iters, tau, weight (packed, pair-major), return_residual (packed) of ops.rigid_fit.
    The flow a forward returned is read in place (a (B, 3, N) view of its [B N, 3] rows; the row-block views of a ragged
    forward); B > 1 clouds are packed into one (3, sum N_b) tensor first (one copy), any other list of flows likewise.
    -> (R (B, 3, 3), t (B, 3), stats (B, 4), refined[, residual]), refined in the form of `flow`: views of one [sum N_b, 3]
    tensor."""
    pc, fl, prefix, counts, shape = _packed_pairs(pc1, flow, lat_or_counts, 'rigid_refine')
    res = ops.rigid_fit(pc, fl, prefix=prefix, **kw)
    ref = res[3]
    if shape is not False or tuple(flow.shape) == (3, ref.shape[0]):         # (a packed [N, 3] flow gets its rows as they are)
        ref = _rows_as(ref, shape, prefix)
    return res[:3] + (ref,) + res[4:]


# ----------------------------------------------------------------------------- rigid registration
def icp_register(pc1, pc2, lat_or_counts=None, init=None, **kw):
    """The rigid registration of pc1 onto pc2 in ONE ops.icp call: per pair the motion (R, t) with
    R pc1 + t ~ pc2, from the clouds alone.  pc1 / pc2 in the forms rigid_refine takes, each on its own: a (B, 3, N) tensor
    (or (3, N): one pair), or a list of B (3, N_b) / (1, 3, N_b) tensors (a ragged batch; N_b of pc1 and of pc2 may differ);
    a packed (3, sum N_b) cloud takes its pairs' counts from lat_or_counts: a ragged forward's lattice (its point_counts),
    a sequence of counts for both clouds, or a pair (counts of pc1, counts of pc2).  B > 1 clouds are packed into one
    (3, sum N_b) tensor first (one copy each).  init: (R (B, 3, 3), t (B, 3)) -- the first entries of a rigid_refine result --
    or None (identity).  kw: weight (packed, pair-major), iters, max_dist, tau, tol_rot, tol_trans, return_matches of ops.icp;
    metric='plane'  with normals (the (3, sum M_b) normals of the packed pc2) or, with normals=None, ONE
    ops.normals call on pc2 in the same stream: normals_k (16) neighbours within normals_radius (default: max_dist), seen from
    the origin.
    -> (R (B, 3, 3), t (B, 3), stats (B, 6), flow[, match, dist2]), flow = R p + t - p in the form of pc1: views of one
    [sum N_b, 3] tensor; match and dist2 stay packed."""
    read = []
    for cloud, (pc, what) in enumerate(((pc1, 'pc1'), (pc2, 'pc2'))):
        clouds, form = _cloud_forms(pc, 'icp_register', what)
        n = _pair_counts(lat_or_counts, int(pc.shape[1]), 'icp_register', cloud, ' of %s' % what) if form is False else \
            [int(c.shape[1]) for c in clouds]
        read.append((_packed(pc, clouds, form), n, form))
    (src, n1, shape), (dst, n2, shape2) = read
    if len(n1) != len(n2):
        raise _lib.HplError('icp_register: pc1 holds %d clouds, pc2 %d' % (len(n1), len(n2)))
    for cloud, (what, n, form) in enumerate((('pc1', n1, shape), ('pc2', n2, shape2))):
        if form is not False and _stated_counts(lat_or_counts, None, cloud) not in (None, n):
            raise _lib.HplError('icp_register: the clouds of %s hold %s points, the lattice or counts say otherwise' % (what, n))
    sp, dp = _prefix_of(n1), _prefix_of(n2)
    metric, normals = kw.pop('metric', 'point'), kw.pop('normals', None)
    normals_k, normals_radius = kw.pop('normals_k', 16), kw.pop('normals_radius', None)
    if metric == 'plane':
        # metric='plane' (DESIGN.md §29): normals = the (3, sum M_b) normals of the packed pc2, or None: ops.normals of pc2 on the
        # same stream, k = normals_k, radius = normals_radius (default: max_dist), seen from the origin
        if normals is None:
            normals = ops.normals(dst, k=normals_k, radius=kw.get('max_dist', 1.0) if normals_radius is None else normals_radius,
                                  prefix=dp)[0]
        kw.update(metric='plane', dst_normal=normals)
    elif metric != 'point' or normals is not None:
        raise _lib.HplError('icp_register: metric = %r (\'point\', or \'plane\' with normals (3, M) or None)' % (metric,))
    res = ops.icp(src, dst, init=init, src_prefix=sp, dst_prefix=dp, **kw)
    return res[:3] + (_rows_as(res[3], shape, sp),) + res[4:]


# ----------------------------------------------------------------------------- surface normals
def estimate_normals(pc, lat_or_counts=None, k=16, radius=1.0, viewpoint=None):
    """The surface normals of the cloud(s) pc in ONE ops.normals call.  pc in the forms rigid_refine takes: a
    (B, 3, N) tensor (or (3, N): one cloud), or a list of B (3, N_b) / (1, 3, N_b) tensors (a ragged batch); a packed
    (3, sum N_b) cloud takes its clouds' counts from lat_or_counts (a forward's lattice -- a ragged one: the counts of its
    first clouds --, or a sequence of counts).  B > 1 clouds are packed into one (3, sum N_b) tensor first (one copy).
    k, radius, viewpoint: of ops.normals (viewpoint: three numbers for every cloud, or B triples; None: the origin).
    -> (normal, curvature, count): normal in the form of pc -- (B, 3, N), (3, N) or a list of views of one (3, sum N_b)
    tensor --, curvature and count (B, N) for a (B, 3, N) tensor, else packed (sum N_b,)."""
    who = 'estimate_normals'
    clouds, shape = _cloud_forms(pc, who, 'pc')
    counts = _pair_counts(lat_or_counts, int(pc.shape[1]), who) if shape is False else [int(c.shape[1]) for c in clouds]
    if shape and lat_or_counts is not None and _pair_counts(lat_or_counts, sum(counts), who) != counts:
        raise _lib.HplError('estimate_normals: the clouds hold %s points, the lattice or counts say otherwise' % (counts,))
    cloud, prefix = _packed(pc, clouds, shape), _prefix_of(counts)
    normal, curvature, count = ops.normals(cloud, k=k, radius=radius, viewpoint=viewpoint, prefix=prefix)
    B = len(counts)
    if shape is None:
        n = counts[0]
        return normal.view(3, B, n).transpose(0, 1), curvature.view(B, n), count.view(B, n)
    if shape is False:
        return normal, curvature, count
    return ([normal[:, prefix[b]:prefix[b + 1]].unsqueeze(0) if shape[b] else normal[:, prefix[b]:prefix[b + 1]]
             for b in range(B)], curvature, count)


# ----------------------------------------------------------------------------- moving objects
def segment_motion(pc1, flow, lat_or_counts=None, rigid=None, object_fits=False, iters=4, tau=0.1, weight=None, **kw):
    """The moving objects of a forward's flow: ops.rigid_fit(return_residual=True) over the pairs -- unless
    `rigid` hands in what an earlier rigid_refine(..., return_residual=True) or ops.rigid_fit(..., return_residual=True) of the
    same operands returned --, then ONE ops.motion_segment call with that fit's residuals and tau.  pc1 / flow / lat_or_counts:
    the forms rigid_refine takes, read in place the same way.  iters, tau, weight: of the fit; kw: eps, dv, min_points,
    max_objects of ops.motion_segment.
    -> (labels (sum N_b,) int32, packed pair-major; obj_info (B, max_objects, 2); obj_motion (B, max_objects, 6); stats (B, 4)):
    no read-back, no host synchronisation.
    object_fits=True, and only then, READS BACK stats and obj_info once (a host synchronisation: this is for interactive use,
    not for an evaluation loop), gathers each listed object's points in object order and fits every object's own rigid
    motion with ops.rigid_fit, the objects as its segments, 64 a call.  The result gains a fifth entry: per pair a tuple
    (R (K_b, 3, 3), t (K_b, 3), stats (K_b, 4)) over the pair's first K_b = min(objects, max_objects) objects (an object of fewer
    than 3 points has status 0, R = I, t = 0, as that op defines).
    object_fits='device' is the form without a read-back: ONE ops.object_fit call on the labels just computed,
    with the fit's iters and tau and, as object_fits=True, no weight.  The fifth entry is then (obj_Rt (B, max_objects, 12),
    obj_stats (B, max_objects, 4)): the rows of a pair's first min(objects, max_objects) objects hold the bits object_fits=True
    returns, the rows behind them R = I, t = 0, stats 0."""
    pc, fl, prefix, counts, _ = _packed_pairs(pc1, flow, lat_or_counts, 'segment_motion')
    if rigid is None:
        residual = ops.rigid_fit(pc, fl, weight=weight, iters=iters, tau=tau, prefix=prefix, return_residual=True)[4]
    else:
        residual = rigid[-1] if isinstance(rigid, (list, tuple)) and len(rigid) == 5 else None
        if not torch.is_tensor(residual) or tuple(residual.shape) != (pc.shape[1],):
            raise _lib.HplError('segment_motion: rigid is the result of a fit of the same operands with return_residual=True')
    labels, info, motion, stats = ops.motion_segment(pc, fl, residual, tau=tau, prefix=prefix, **kw)
    if not object_fits:
        return labels, info, motion, stats
    if object_fits == 'device':
        return labels, info, motion, stats, ops.object_fit(pc, fl, labels, max_objects=info.shape[1], iters=iters, tau=tau,
                                                           prefix=prefix)
    host = info.cpu().numpy()                                # the one read-back (it follows the launches on this stream)
    dev = pc.device
    fits = []
    flt = fl if tuple(fl.shape) == (3, pc.shape[1]) else fl.t()          # (3, N) view, any strides
    for b in range(len(counts)):
        sizes = [int(c) for r, c in host[b] if r >= 0]
        K = len(sizes)
        if K == 0:
            fits.append((torch.zeros((0, 3, 3), device=dev), torch.zeros((0, 3), device=dev), torch.zeros((0, 4), device=dev)))
            continue
        lab = labels[prefix[b]:prefix[b + 1]]
        order = torch.argsort(torch.where((lab >= 0) & (lab < K), lab, K), stable=True)[:sum(sizes)] + prefix[b]
        opc, ofl = pc[:, order].contiguous(), flt[:, order].contiguous()
        Rs, ts, sts = [], [], []
        for c in range(0, K, 64):
            pre = _prefix_of(sizes[c:c + 64])
            lo = sum(sizes[:c])
            R, t, st, _ = ops.rigid_fit(opc[:, lo:lo + pre[-1]], ofl[:, lo:lo + pre[-1]], iters=iters, tau=tau, prefix=pre)
            Rs.append(R)
            ts.append(t)
            sts.append(st)
        fits.append((torch.cat(Rs), torch.cat(ts), torch.cat(sts)))
    return labels, info, motion, stats, fits


def piecewise_rigid(pc1, flow, lat_or_counts=None, iters=4, tau=0.1, obj_iters=None, obj_tau=None, weight=None, **segment_kw):
    """The piecewise-rigid flow of a forward's flow in three stream-ordered calls without a read-back:
    ops.rigid_fit(return_residual=True) for the ego-motion, ops.motion_segment on its residuals for the objects, and
    ops.object_fit on the fit's refined flow and residual for each object's own motion.  pc1 / flow / lat_or_counts: the forms
    rigid_refine takes, read in place the same way.  iters, tau, weight: of the ego fit (tau is the movers' threshold too);
    obj_iters, obj_tau: of the object fits (None: iters and tau; the object fits take the same weight); segment_kw: eps, dv,
    min_points, max_objects of ops.motion_segment.
    -> (R (B, 3, 3), t (B, 3), stats (B, 4), labels (sum N_b,), obj_info, obj_Rt (B, max_objects, 12), obj_stats
    (B, max_objects, 4), refined): refined in the form of `flow`, as rigid_refine returns it -- the ego-motion's rigid flow at
    its inliers, an object's at the inliers of its fit, the input flow's bits at every other point."""
    w = _piecewise(pc1, flow, lat_or_counts, iters, tau, obj_iters, obj_tau, weight, segment_kw)
    return w.fit[:3] + (w.seg[0], w.seg[1], w.obj_Rt, w.obj_stats, w.refined)


_Piecewise = collections.namedtuple('_Piecewise', 'fit seg obj_Rt obj_stats refined replaced')


def _piecewise(pc1, flow, lat_or_counts, iters, tau, obj_iters, obj_tau, weight, segment_kw, keep_ego=False):
    """piecewise_rigid's three calls -> _Piecewise: fit = ops.rigid_fit's five results and seg = ops.motion_segment's four, of the
    packed operands; refined in the form of `flow`.  By default the object fits update the ego fit's refined rows where they
    lie (fit[3] is then the piecewise-rigid flow too).  keep_ego (validate(objects=...), which reports both flows): the object
    fits write into rows of their own, fit[3] -- in the form of `flow` -- stays the ego fit's, and replaced (B,) int64 counts
    each pair's rows that an object fit wrote, on the device."""
    pc, fl, prefix, counts, shape = _packed_pairs(pc1, flow, lat_or_counts, 'piecewise_rigid')
    fit = ops.rigid_fit(pc, fl, weight=weight, iters=iters, tau=tau, prefix=prefix, return_residual=True)
    seg = ops.motion_segment(pc, fl, fit[4], tau=tau, prefix=prefix, **segment_kw)
    # (a row an object fit writes is finite -- an inlier has a finite residual --, so NaN marks the rows it left alone)
    rows = torch.full_like(fit[3], float('nan')) if keep_ego else fit[3]
    obj_Rt, obj_stats = ops.object_fit(pc, fl, seg[0], weight=weight, max_objects=seg[1].shape[1],
                                       iters=iters if obj_iters is None else obj_iters, tau=tau if obj_tau is None else obj_tau,
                                       prefix=prefix, residual=None if keep_ego else fit[4], refined=rows)[:2]
    replaced = None
    if keep_ego:
        wrote = rows[:, 0] == rows[:, 0]
        rows = torch.where(wrote[:, None], rows, fit[3])
        replaced = torch.stack([wrote[a:b].sum() for a, b in zip(prefix[:-1], prefix[1:])])
    as_flow = shape is not False or tuple(flow.shape) == (3, rows.shape[0])    # (a packed [N, 3] flow gets its rows as they are)
    if keep_ego and as_flow:
        fit = fit[:3] + (_rows_as(fit[3], shape, prefix),) + fit[4:]
    return _Piecewise(fit, seg, obj_Rt, obj_stats, _rows_as(rows, shape, prefix) if as_flow else rows, replaced)


# ----------------------------------------------------------------------------- ground removal
_Pairs = collections.namedtuple('_Pairs', 'c1 c2 fl joint clouds prefix')


def _clouds(x, who, what):
    return _cloud_forms(x, who, what, True)[0]


def _pairs_in(who, pc1, pc2, sf, corr):
    """The operands of voxel_downsample and fps_sample, in the forms remove_ground takes (pc2 and sf may be None) -> _Pairs: the
    clouds c1, c2, fl of each; joint: the pairs stay pairs (corr, or no pc2; at most 64), else the op runs over the 2 B clouds
    c1 + c2 (at most 32 pairs); clouds: those it runs over, and their prefix."""
    c1 = _clouds(pc1, who, 'pc1')
    c2 = _clouds(pc2, who, 'pc2') if pc2 is not None else None
    fl = _clouds(sf, who, 'sf') if sf is not None else None
    B = len(c1)
    if (c2 is not None and len(c2) != B) or (fl is not None and (len(fl) != B or any(f.shape[1] != c.shape[1] for f, c in zip(fl, c1)))):
        raise _lib.HplError('%s: pc1, pc2 and sf hold as many clouds, and sf as many points as pc1' % who)
    joint = corr or c2 is None
    if corr and c2 is not None and any(a.shape[1] != b.shape[1] for a, b in zip(c1, c2)):
        raise _lib.HplError('%s: corr=True takes clouds that correspond point to point (as many points in pc1 and pc2)' % who)
    if not 1 <= (B if joint else 2 * B) <= 64:
        raise _lib.HplError('%s: %d pairs (1 .. %d a call)' % (who, B, 64 if joint else 32))
    clouds = c1 if joint else c1 + c2
    return _Pairs(c1, c2, fl, joint, clouds, _prefix_of(c.shape[1] for c in clouds))


def _pairs_packed(p):
    """(the packed cloud, attrs) of _pairs_in's operands: what rides with pc1's points -- pc2 when the pairs stay pairs, and sf
    (zero over the pc2 clouds where those are clouds of their own) -- as attribute channels, or None."""
    pc = torch.cat(p.clouds, dim=1)
    riders = []
    if p.joint and p.c2 is not None:
        riders.append(torch.cat(p.c2, dim=1))
    if p.fl is not None:
        f = torch.cat(p.fl, dim=1)
        riders.append(f if p.joint else torch.cat([f, f.new_zeros((3, p.prefix[-1] - p.prefix[len(p.c1)]))], dim=1))
    return pc, torch.cat(riders, dim=0) if riders else None


def _pairs_out(p, out_pc, out_attrs, stats, spans):
    """(pc1 list, pc2 list or None, sf list or None, stats) of the op's outputs: spans[i] = the columns (first, end) that hold
    the results of p.clouds[i]."""
    B = len(p.c1)
    cols = [out_pc[:, a:b] for a, b in spans]
    o2 = None if p.c2 is None else cols[B:] if not p.joint else [out_attrs[:3, a:b] for a, b in spans[:B]]
    of = None if p.fl is None else [out_attrs[out_attrs.shape[0] - 3:, a:b] for a, b in spans[:B]]
    return cols[:B], o2, of, stats if p.joint else stats.view(2, B, 4)


def remove_ground(pc1, pc2, sf=None, corr=True, return_mask=False, **kw):
    """The pair(s) without their ground, by ONE ops.ground_fit call over the 2 B clouds -- the pc1 clouds first, then the pc2
    clouds -- (DESIGN.md §21): every cloud gets its own fitted plane.  pc1 / pc2 / sf in the forms rigid_refine takes: (3, N)
    tensors (one pair), (B, 3, N) tensors, or lists of B (3, N_b) tensors.  kw: up, max_tilt_deg, hyps, tau, refine, cut, seed,
    call of ops.ground_fit.
    corr=True (the clouds of a pair correspond point to point, so they hold as many points): the reference's pair rule on the
    fitted planes -- index i is dropped when it is ground in BOTH clouds; pc1, pc2 and sf are indexed together.
    corr=False: each cloud is compacted on its own through keep_idx and the kept counts; sf follows pc1.
    One read-back (corr=True: the pair masks; corr=False: the kept counts), as the device transforms make one.
    -> (pc1 list of (3, K_b), pc2 list, sf list or None, planes (2, B, 4), stats (2, B, 4) int32[, masks]): return_mask (with
    corr=True) appends the pairs' keep masks as host numpy bool arrays."""
    who = 'remove_ground'
    if 'return_votes' in kw or 'return_height' in kw:
        raise _lib.HplError('%s takes the fitting arguments of ops.ground_fit, not its optional outputs' % who)
    c1, c2 = _clouds(pc1, who, 'pc1'), _clouds(pc2, who, 'pc2')
    fl = _clouds(sf, who, 'sf') if sf is not None else None
    B = len(c1)
    if len(c2) != B or (fl is not None and (len(fl) != B or any(f.shape[1] != c.shape[1] for f, c in zip(fl, c1)))):
        raise _lib.HplError('%s: pc1, pc2 and sf hold as many clouds, and sf as many points as pc1' % who)
    if corr and any(a.shape[1] != b.shape[1] for a, b in zip(c1, c2)):
        raise _lib.HplError('%s: corr=True takes clouds that correspond point to point (as many points in pc1 and pc2)' % who)
    if return_mask and not corr:
        raise _lib.HplError('%s: return_mask comes with corr=True' % who)
    if not 1 <= 2 * B <= 64:
        raise _lib.HplError('%s: %d pairs (1 .. 32 a call)' % (who, B))
    prefix = _prefix_of(c.shape[1] for c in c1 + c2)
    pc = torch.cat(c1 + c2, dim=1)
    plane, stats, ground, keep = ops.ground_fit(pc, prefix=prefix, **kw)
    n1 = prefix[B]
    o1, o2, of, masks = [], [], ([] if fl is not None else None), []
    if corr:
        host = (~(ground[:n1].bool() & ground[n1:].bool())).cpu().numpy()       # the one read-back
        for b in range(B):
            m = host[prefix[b]:prefix[b + 1]]
            masks.append(m)
            idx = torch.from_numpy(m.nonzero()[0]).to(pc.device)
            o1.append(c1[b].index_select(1, idx))
            o2.append(c2[b].index_select(1, idx))
            if fl is not None:
                of.append(fl[b].index_select(1, idx))
    else:
        kept = stats[:, 3].cpu().tolist()                                       # the one read-back
        for b in range(B):
            i1 = keep[prefix[b]:prefix[b] + kept[b]].long() - prefix[b]
            i2 = keep[prefix[B + b]:prefix[B + b] + kept[B + b]].long() - prefix[B + b]
            o1.append(c1[b].index_select(1, i1))
            o2.append(c2[b].index_select(1, i2))
            if fl is not None:
                of.append(fl[b].index_select(1, i1))
    res = (o1, o2, of, plane.view(2, B, 4), stats.view(2, B, 4))
    return res + (masks,) if return_mask else res


# ----------------------------------------------------------------------------- outlier removal
OUTLIER_BY = ('either', 'pc1')


def remove_outliers(pc1, pc2=None, sf=None, corr=True, by='either', return_mask=False, **kw):
    """The pair(s) without their stray points, by ONE ops.outlier_filter call.  pc1 / pc2 / sf in the forms
    voxel_downsample takes: (3, N) tensors (one pair), (B, 3, N) tensors, or lists of B (3, N_b) tensors; pc2 and sf may be
    None.  kw: mode, k, radius, std_ratio, min_neighbors of ops.outlier_filter.
    corr=True (the clouds of a pair correspond point to point, so they hold as many points), by='either': the op runs over the
    2 B clouds -- the pc1 clouds first, then the pc2 clouds -- and a correspondence is dropped when it is an outlier in either
    cloud; pc1, pc2 and sf are indexed together, so pc2' - pc1' keeps sf' exactly.  At most 32 pairs a call.  (Without pc2:
    as by='pc1'.)
    corr=True, by='pc1': pc1's clouds decide; pc2 and sf follow through keep_idx.  At most 64 pairs a call.
    corr=False: each of the 2 B clouds is filtered on its own; sf follows pc1.  At most 32 pairs a call.
    One read-back: the pair masks (by='either', or return_mask) or the kept counts.
    -> (pc1 list of (3, K_b), pc2 list or None, sf list or None, thresh (B, 4) float32, stats (B, 4) int32 -- (2, B, 4) both
    where the op ran over 2 B clouds --[, masks]): return_mask (with corr=True) appends the pairs' keep masks as host numpy
    bool arrays."""
    who = 'remove_outliers'
    if set(kw) - {'mode', 'k', 'radius', 'std_ratio', 'min_neighbors'}:
        raise _lib.HplError('%s takes mode, k, radius, std_ratio and min_neighbors of ops.outlier_filter, got %s' % (
            who, sorted(set(kw) - {'mode', 'k', 'radius', 'std_ratio', 'min_neighbors'})))
    if by not in OUTLIER_BY:
        raise _lib.HplError('%s: by = %r (%s)' % (who, by, ' or '.join(repr(x) for x in OUTLIER_BY)))
    if return_mask and not corr:
        raise _lib.HplError('%s: return_mask comes with corr=True' % who)
    ops.outlier_args(who, kw.get('mode', 'statistical'), kw.get('k', 16), kw.get('radius', 1.0), kw.get('std_ratio', 2.0),
                     kw.get('min_neighbors'))
    p = _pairs_in(who, pc1, pc2, sf, corr)
    c1, c2, fl = p.c1, p.c2, p.fl
    B = len(c1)
    both = c2 is not None and not (corr and by == 'pc1')         # the op runs over the 2 B clouds
    if both and 2 * B > 64:
        raise _lib.HplError('%s: %d pairs (1 .. 32 a call)' % (who, B))
    clouds = c1 + c2 if both else c1
    prefix = _prefix_of(c.shape[1] for c in clouds)
    keep, keep_idx, _, _, thresh, stats = ops.outlier_filter(torch.cat(clouds, dim=1), prefix=prefix, **kw)
    n1 = prefix[B]
    o1, o2, of, masks = [], ([] if c2 is not None else None), ([] if fl is not None else None), []
    if corr and (both or return_mask):
        host = ((keep[:n1] & keep[n1:]) if both else keep).bool().cpu().numpy()        # the one read-back
        for b in range(B):
            m = host[prefix[b]:prefix[b + 1]]
            masks.append(m)
            idx = torch.from_numpy(m.nonzero()[0]).to(keep.device)
            o1.append(c1[b].index_select(1, idx))
            if c2 is not None:
                o2.append(c2[b].index_select(1, idx))
            if fl is not None:
                of.append(fl[b].index_select(1, idx))
    else:
        kept = stats[:, 1].cpu().tolist()                                               # the one read-back
        for b in range(B):
            i1 = keep_idx[prefix[b]:prefix[b] + kept[b]].long() - prefix[b]
            o1.append(c1[b].index_select(1, i1))
            if c2 is not None:
                o2.append(c2[b].index_select(1, i1 if corr else
                                             keep_idx[prefix[B + b]:prefix[B + b] + kept[B + b]].long() - prefix[B + b]))
            if fl is not None:
                of.append(fl[b].index_select(1, i1))
    res = (o1, o2, of, thresh.view(2, B, 4) if both else thresh, stats.view(2, B, 4) if both else stats)
    return res + (masks,) if return_mask else res


# ----------------------------------------------------------------------------- voxel-grid downsampling
def voxel_downsample(pc1, pc2=None, sf=None, voxel=0.1, mode='centroid', corr=True, origin=(0, 0, 0), return_index=False):
    """The pair(s) on a voxel grid of edge `voxel`, one point per occupied cell, by ONE ops.voxel_downsample call (DESIGN.md
    §24).  pc1 / pc2 / sf in the forms remove_ground takes: (3, N) tensors (one pair), (B, 3, N) tensors, or lists of B
    (3, N_b) tensors; pc2 and sf may be None.  mode 'centroid' (the cell's mean) or 'nearest' (the member nearest to it: the
    output is a subset of the input).
    corr=True (the clouds of a pair correspond point to point, so they hold as many points): pc1's cells decide; pc2 and sf
    ride as attribute channels, so a pair stays a pair and pc2' - pc1' equals sf' up to the rounding of the means -- exactly
    in mode 'nearest'.  At most 64 pairs a call.
    corr=False: the 2 B clouds -- the pc1 clouds first, then the pc2 clouds -- are each voxelised on their own; sf follows pc1.
    At most 32 pairs a call.
    One read-back: the voxel counts.
    -> (pc1 list of (3, V_b), pc2 list or None, sf list or None, stats (B, 4) int32 -- corr=False with pc2: (2, B, 4) --
    [, voxel_of list, rep list]): return_index appends, per voxelised cloud (corr=False: the pc1 clouds, then the pc2 clouds),
    voxel_of (n_b,) int64 -- every input point's column in the cloud's output, -1 for a point of no voxel -- and rep (V_b,)
    int64, the member nearest to the mean as an index into the cloud."""
    who = 'voxel_downsample'
    ops.voxel_args(who, voxel, origin, mode)
    p = _pairs_in(who, pc1, pc2, sf, corr)
    pc, attrs = _pairs_packed(p)
    prefix = p.prefix
    out_pc, out_attrs, _, rep, voxel_of, stats = ops.voxel_downsample(pc, attrs, voxel=voxel, origin=origin, mode=mode, prefix=prefix)
    V = stats[:, 0].cpu().tolist()                                              # the one read-back
    res = _pairs_out(p, out_pc, out_attrs, stats, [(prefix[b], prefix[b] + V[b]) for b in range(len(p.clouds))])
    if return_index:
        vo, rp = [], []
        for b in range(len(p.clouds)):
            w = voxel_of[prefix[b]:prefix[b + 1]].long()
            vo.append(torch.where(w >= 0, w - prefix[b], w))
            rp.append(rep[prefix[b]:prefix[b] + V[b]].long() - prefix[b])
        res += (vo, rp)
    return res


# ----------------------------------------------------------------------------- farthest point sampling
def fps_sample(pc1, pc2=None, sf=None, num_points=8192, corr=True, start=None, seed=None, return_index=False):
    """The pair(s) sampled to num_points points a cloud by farthest point sampling, by ONE ops.fps call.  pc1 /
    pc2 / sf in the forms voxel_downsample takes: (3, N) tensors (one pair), (B, 3, N) tensors, or lists of B (3, N_b) tensors;
    pc2 and sf may be None.  A cloud of fewer distinct finite positions than num_points yields that many points.
    corr=True (the clouds of a pair correspond point to point, so they hold as many points): pc1 decides; pc2 and sf ride as
    attribute channels, so a pair stays a pair and pc2' - pc1' keeps sf' exactly.  At most 64 pairs a call.
    corr=False: the 2 B clouds -- the pc1 clouds first, then the pc2 clouds -- are each sampled on their own; sf follows pc1.
    At most 32 pairs a call.
    start: one index per sampled cloud (its first sample); seed: every sampled cloud's start is drawn on the host from
    numpy.random.RandomState(seed), in cloud order; neither: every cloud starts at its first finite point.
    One read-back: the counts.
    -> (pc1 list of (3, count_b), pc2 list or None, sf list or None, stats (B, 4) int32 -- corr=False with pc2: (2, B, 4) --
    [, idx list]): return_index appends, per sampled cloud, idx (count_b,) int64 into the cloud, in selection order."""
    who = 'fps_sample'
    p = _pairs_in(who, pc1, pc2, sf, corr)
    clouds = p.clouds
    ops.fps_args(who, num_points, len(clouds))
    if start is not None and seed is not None:
        raise _lib.HplError('%s: start and seed together (give one)' % who)
    sizes = [int(c.shape[1]) for c in clouds]
    if seed is not None:
        import numpy as np
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
            raise _lib.HplError('%s: seed = %r (an int in 0 .. 2^32 - 1)' % (who, seed))
        rs = np.random.RandomState(seed)
        start = [int(rs.randint(0, n)) if n > 0 else 0 for n in sizes]
    pc, attrs = _pairs_packed(p)
    out_pc, out_attrs, idx, _, _, stats = ops.fps(pc, num_points, attrs, start=start, prefix=p.prefix)
    K = stats[:, 0].cpu().tolist()                                              # the one read-back
    m = num_points
    res = _pairs_out(p, out_pc, out_attrs, stats, [(b * m, b * m + K[b]) for b in range(len(clouds))])
    if return_index:
        res += ([idx[b, :K[b]].long() for b in range(len(clouds))],)
    return res


# ----------------------------------------------------------------------------- frames from raw maps
def _pack_planes(who, frames, specs, device):
    """frames: a list of tuples of per-frame arrays (numpy or tensors), plane k of shape (H, W) + specs[k][1] and a dtype in
    specs[k][0] -> (packed device tensors, one per plane, heights, widths)."""
    import numpy as np
    if not isinstance(frames, (list, tuple)) or not 1 <= len(frames) <= 64 or any(
            not isinstance(fr, (list, tuple)) or len(fr) < len(specs) for fr in frames):
        raise _lib.HplError('%s: a list of 1 .. 64 frames, each a tuple of %d arrays' % (who, len(specs)))
    hh, ww = [], []
    for fr in frames:
        shp = tuple(fr[0].shape)
        if len(shp) != 2:
            raise _lib.HplError('%s: a frame\'s first array is (H, W), got %s' % (who, shp))
        hh.append(shp[0])
        ww.append(shp[1])
    packed = []
    for k, (dtypes, tail) in enumerate(specs):
        parts = []
        for b, fr in enumerate(frames):
            x = fr[k]
            if not torch.is_tensor(x):
                x = torch.from_numpy(np.ascontiguousarray(x))
            if x.dtype not in dtypes or tuple(x.shape) != (hh[b], ww[b]) + tail:
                raise _lib.HplError('%s: array %d of frame %d must be %s of shape %s, got %s %s' % (
                    who, k, b, ' / '.join(str(d) for d in dtypes), (hh[b], ww[b]) + tail, x.dtype, tuple(x.shape)))
            parts.append(x.reshape((-1,) + tail))
        packed.append(parts)
    return [torch.cat(parts, dim=0).to(device) for parts in packed], hh, ww


def _frame_views(pc1, pc2, pixel, counts, hh, ww):
    n = counts.cpu().tolist()                                                       # the one read-back
    o1, o2, px, p0 = [], [], [], 0
    for b in range(len(hh)):
        o1.append(pc1[:, p0:p0 + n[b]])
        o2.append(pc2[:, p0:p0 + n[b]])
        px.append(pixel[p0:p0 + n[b]])
        p0 += hh[b] * ww[b]
    return o1, o2, px, n


def frames_from_kitti(frames, baseline=0.54, device='cuda'):
    """The corresponding clouds of KITTI scene-flow frames from their raw maps by ONE ops.frames_from_kitti call (DESIGN.md
    §25).  frames: a list of 1 .. 64 tuples (disp1 (H, W) uint16, disp2 (H, W) uint16, flow (H, W, 3) uint16, P (3, 4)) -- the
    raw values of disp_occ_0, disp_occ_1 and flow_occ as data.read_png returns them and the frame's P_rect_02 --, numpy arrays
    or tensors; the frames may differ in size.  One read-back: the counts.
    -> (pc1 list of (3, n_b) float32 views, pc2 list, pixel list of (n_b,) int32 -- i * W + j of every correspondence, in
    ascending order --, counts list): pc1[b].T is the pc1.npy the reference's process_kitti.py saves for the frame, bit for bit."""
    who = 'frames_from_kitti'
    (d1, d2, fl), hh, ww = _pack_planes(who, frames, [(ops._U16, ()), (ops._U16, ()), (ops._U16, (3,))], device)
    pc1, pc2, pixel, counts = ops.frames_from_kitti(d1, d2, fl, [fr[3] for fr in frames], hh, ww, baseline=baseline)
    return _frame_views(pc1, pc2, pixel, counts, hh, ww)


def frames_from_ft3d(frames, near=None, f=-1050.0, cx=479.5, cy=269.5, device='cuda'):
    """The corresponding clouds of FlyingThings3D-subset frames from their raw maps by ONE ops.frames_from_ft3d call (DESIGN.md
    §25).  frames: a list of 1 .. 64 tuples (disparity (H, W) float32, disparity change (H, W) float32, flow (H, W, 2) float32,
    disparity occlusions (H, W) uint8, flow occlusions (H, W) uint8).  near: None or the near cut (-35.).  One read-back.
    -> as frames_from_kitti: pc1[b].T is the pc1.npy the reference's process_flyingthings3d_subset.py saves (x and z with the
    sign it saves; data.FlyingThings3DRaw flips them as the reference's reader does)."""
    who = 'frames_from_ft3d'
    f32, u8 = (torch.float32,), (torch.uint8,)
    (d, dc, fl, o1, o2), hh, ww = _pack_planes(who, frames, [(f32, ()), (f32, ()), (f32, (2,)), (u8, ()), (u8, ())], device)
    pc1, pc2, pixel, counts = ops.frames_from_ft3d(d, dc, fl, o1, o2, hh, ww, f=f, cx=cx, cy=cy, near=near)
    return _frame_views(pc1, pc2, pixel, counts, hh, ww)


# ----------------------------------------------------------------------------- maps from clouds
def _per_frame(who, name, x, B, width):
    """B host rows of `width` numbers from one row for all frames or a sequence of B rows."""
    try:
        rows = [x] * B if len(x) == width and not hasattr(x[0], '__len__') else list(x)
        rows = [tuple(r) for r in rows]
    except TypeError:
        rows = []
    if len(rows) != B or any(len(r) != width for r in rows):
        raise _lib.HplError('%s: %s is one row of %d numbers or one for each of the %d clouds' % (who, name, width, B))
    return rows


def _render_in(who, pc, camera, size):
    """(clouds, form, packed cloud, prefix, cameras, heights, widths) of the operands render_maps and visibility take."""
    clouds, form = _cloud_forms(pc, who, 'pc', rows3=True)
    B = len(clouds)
    sizes = [(int(h), int(w)) for h, w in _per_frame(who, 'size', size, B, 2)]
    prefix = _prefix_of([int(c.shape[1]) for c in clouds])
    return clouds, form, _packed(pc, clouds, form), prefix, _per_frame(who, 'camera', camera, B, 6), [s[0] for s in sizes], [s[1] for s in sizes]


def _per_cloud(x, form, prefix):
    """A packed (sum N_b,) per-point result in the form of the operand: (B, N), (N,) or a list of (N_b,) views."""
    if form is None:
        return x.view(len(prefix) - 1, -1)
    if form is False:
        return x
    return [x[prefix[b]:prefix[b + 1]] for b in range(len(prefix) - 1)]


def visibility(pc, camera, size, footprint=1, rel_tol=0.02, abs_tol=0.0, near=1e-3):
    """Which points of the cloud(s) pc a camera sees, by ONE ops.render_maps call: a point is visible when its
    pixel lies in the image and no point that covers that pixel is nearer than it by more than the tolerance -- zc <= zmin *
    (1 + rel_tol) + abs_tol.  pc: a (3, N) cloud, a (B, 3, N) batch or a list of (3, N_b) tensors; camera: one (f, cx, cy,
    constx, consty, constz) or one per cloud; size: one (H, W) or one per cloud.  For "is pc1 + flow hidden in frame 2" pass the
    warped cloud together with the second frame's cloud and read the mask of the former.  footprint: every point covers the
    (2 footprint + 1)^2 pixels around its own -- with 0 a sparse cloud leaks: far points show through the gaps between near
    ones.  The defaults footprint=1, rel_tol=0.02 are starting values; they are not measured on real frames.
    -> a boolean mask in the form of pc: (N,), (B, N) or a list of (N_b,).  No read-back."""
    who = 'visibility'
    _, form, cloud, prefix, cams, hh, ww = _render_in(who, pc, camera, size)
    res = ops.render_maps(cloud, cams, hh, ww, footprint=footprint, rel_tol=rel_tol, abs_tol=abs_tol, near=near, prefix=prefix)
    return _per_cloud(res[4].bool(), form, prefix)


def render_maps(pc, camera, size, attrs=None, footprint=0, rel_tol=0.0, abs_tol=0.0, near=1e-3):
    """The cloud(s) pc splatted into one image each by ONE ops.render_maps call and one read-back, the stats.
    pc, camera, size: as visibility takes them; attrs: None, or channels that ride with the points -- a (C, N) tensor for one
    cloud, (B, C, N) for a batch, a list of (C, N_b) -- with C <= 8.  The renderer is a point splat, no surface reconstruction:
    the footprint is in pixels and is not scaled by depth.
    -> (winner: list of (H_b, W_b) int32 views, the cloud-local index of each pixel's nearest point or -1; depth: list of
    (H_b, W_b) float32, its zc or 0; attr_map: list of (C, H_b, W_b) float32 or None; visible: boolean mask(s) in the form of pc;
    pixel_of: int32 i * W + j of every point's pixel or -1, in the form of pc; stats: B host rows (points inside, pixels
    covered, points visible, points not projectable))."""
    who = 'render_maps'
    clouds, form, cloud, prefix, cams, hh, ww = _render_in(who, pc, camera, size)
    B = len(clouds)
    packed_attrs = None
    if attrs is not None:
        al = list(attrs) if isinstance(attrs, (list, tuple)) else ([attrs[b] for b in range(attrs.shape[0])] if torch.is_tensor(attrs) and attrs.dim() == 3 else [attrs])
        if len(al) != B or any(not torch.is_tensor(a) or a.dim() != 2 or a.shape[1] != c.shape[1] or a.shape[0] != al[0].shape[0] for a, c in zip(al, clouds)):
            raise _lib.HplError('%s: attrs holds (C, N_b) channels for each of the %d clouds' % (who, B))
        packed_attrs = al[0] if B == 1 else torch.cat(al, dim=1)
    pixel_of, winner, depth, attr_map, visible, stats = ops.render_maps(
        cloud, cams, hh, ww, attrs=packed_attrs, footprint=footprint, rel_tol=rel_tol, abs_tol=abs_tol, near=near, prefix=prefix)
    qq = _prefix_of([h * w for h, w in zip(hh, ww)])
    frame = lambda x, b: x[..., qq[b]:qq[b + 1]].view(x.shape[:-1] + (hh[b], ww[b]))
    return ([frame(winner, b) for b in range(B)], [frame(depth, b) for b in range(B)],
            None if attr_map is None else [frame(attr_map, b) for b in range(B)],
            _per_cloud(visible.bool(), form, prefix), _per_cloud(pixel_of, form, prefix), stats.cpu().tolist())    # the one read-back


def flow_to_kitti_maps(pc1s, flows, Ps, sizes, baseline=0.54, footprint=0):
    """A scene-flow result in KITTI's own form by ONE ops.maps_to_kitti call.  pc1s: a list of B <= 64 (3, n_b)
    device clouds (or one); flows: their (3, n_b) or (n_b, 3) flows; Ps: each frame's (3, 4) P_rect_02; sizes: each frame's
    (H, W); baseline in metres.  Every pixel takes the nearest pc1 point whose footprint covers it.
    -> a list of (disp_0 (H, W) uint16, disp_1 (H, W) uint16, flow (H, W, 3) uint16) numpy arrays: the raw values of
    disp_0/NNNNNN_10.png, disp_1/NNNNNN_10.png -- the disparity of pc1 + flow at the pixel of pc1 -- and flow/NNNNNN_10.png
    (u, v, valid), which data.write_png writes as KITTI's devkit reads them; 0 where no point falls.  Only the maps are read
    back."""
    who = 'flow_to_kitti_maps'
    if torch.is_tensor(pc1s):
        pc1s, flows, Ps, sizes = [pc1s], [flows], [Ps], [sizes]
    clouds, _ = _cloud_forms(list(pc1s), who, 'pc1s', rows3=True)
    B = len(clouds)
    if len(flows) != B or len(Ps) != B or len(sizes) != B:
        raise _lib.HplError('%s: %d clouds need as many flows, P matrices and sizes' % (who, B))
    fls = [ops._flow_view(f, int(c.shape[1]), c.device, who) for f, c in zip(flows, clouds)]
    pc1 = clouds[0].contiguous() if B == 1 else torch.cat(clouds, dim=1)
    pc2 = pc1 + (fls[0] if B == 1 else torch.cat(fls, dim=1))
    hh, ww = [int(s[0]) for s in sizes], [int(s[1]) for s in sizes]
    d1, d2, fl = ops.maps_to_kitti(pc1, pc2, Ps, hh, ww, baseline=baseline, footprint=footprint,
                                   prefix=_prefix_of([int(c.shape[1]) for c in clouds]))
    d1, d2, fl = d1.cpu().numpy(), d2.cpu().numpy(), fl.cpu().numpy()
    qq = _prefix_of([h * w for h, w in zip(hh, ww)])
    return [(d1[qq[b]:qq[b + 1]].reshape(hh[b], ww[b]), d2[qq[b]:qq[b + 1]].reshape(hh[b], ww[b]),
             fl[qq[b]:qq[b + 1]].reshape(hh[b], ww[b], 3)) for b in range(B)]


# ----------------------------------------------------------------------------- self-supervised loss
def selfsup_loss(flow, pc1, pc2, k=8, w_chamfer=1.0, w_smooth=1.0):
    """The self-supervised loss of a forward's flow in ONE ops.selfsup_loss call: Chamfer distance between
    pc1 + flow and pc2 plus the smoothness of the flow over pc1's k-nearest-neighbour graph, per pair; no flow label.  flow /
    pc1 / pc2 as the models return and take them, in the forms rigid_refine takes: (B, 3, N) tensors (or (3, N): one pair),
    or lists of B (3, N_b) / (1, 3, N_b) tensors (a ragged batch).  The flow is read in place the same way.
    -> (the mean of L over the pairs, a scalar that back-propagates into `flow` alone -- pc1 and pc2 get no gradient --,
    components (B, 4) = (L, C12, C21, S) per pair, detached)."""
    pc, fl, prefix1, counts, _ = _packed_pairs(pc1, flow, None, 'selfsup_loss')
    B = len(counts)
    if isinstance(pc2, (list, tuple)):
        if len(pc2) != B:
            raise _lib.HplError('selfsup_loss: pc1 lists %d clouds, pc2 %d' % (B, len(pc2)))
        qs = [p[0] if p.dim() == 3 else p for p in pc2]
        counts2 = [int(p.shape[1]) for p in qs]
        q = qs[0] if B == 1 else torch.cat(qs, dim=1)
    elif not torch.is_tensor(pc2) or pc2.dim() != (3 if torch.is_tensor(pc1) and pc1.dim() == 3 else 2) or \
            (pc2.dim() == 3 and pc2.shape[0] != B):
        raise _lib.HplError('selfsup_loss: pc2 comes in the form of pc1 (%d pairs)' % B)
    elif pc2.dim() == 3:
        counts2 = [int(pc2.shape[2])] * B
        q = pc2[0] if B == 1 else pc2.transpose(0, 1).reshape(3, B * counts2[0])
    else:
        counts2, q = [int(pc2.shape[1])], pc2
    L, comps = ops.SelfSupLossFn.apply(fl, pc, q, k, w_chamfer, w_smooth, prefix1, _prefix_of(counts2))
    return L.mean(), comps


# ----------------------------------------------------------------------------- dense flow
class DenseState(object):
    """What DenseFlow.forward keeps for later queries: the lattice (its arena holds the level-0 table of cloud 1), the vertex
    activation Z the last Up layer slices ([H0, C] float32, all pairs) and the number of pairs.

    Zw: HPLFlowNet only, made by the first query call with more rows than H0 and kept for later ones -- bcn1_'s trailing 1x1
    applied to Z on the vertices ([H0, 1024] float32, a second ~106 MB per pair at N = 8 192).  Which side of the slice that
    1x1 runs on is decided per query call from its total row count, so a point's flow can differ in its last bits with the
    number of queries it is asked with (both orders are the same function, within the rounding of the GEMM)."""

    def __init__(self, lat, Z, batch, pc1=None, flow=None):
        self.lat, self.Z, self.batch = lat, Z, batch
        self.Zw = None
        self._pc1, self._flow = pc1, flow          # the forward's own pc1 argument and result, as given (no launch, no copy)
        self._fill = None

    def fill_inputs(self):
        """What query(fill='knn') interpolates from, made by the first filled query and kept: the packed sampled pc1
        (3, sum N_b), the forward's flow rows [sum N_b, 3] (both copies of the state's own: later edits of the tensors the
        forward took and returned do not reach them) and the pairs' point prefix (B + 1 host ints)."""
        if self._fill is None:
            pc1, flow, B = self._pc1, self._flow, self.batch
            if pc1 is None or flow is None:
                raise _lib.HplError('fill=\'knn\' needs a state that kept the sampled cloud and its flow')
            if isinstance(pc1, (list, tuple)):       # the forward's own row order: pair-major
                counts = [int(p.shape[1]) for p in pc1]
                packed = torch.cat(list(pc1), dim=1)
                rows = torch.cat([f[0].t() for f in flow], dim=0)
            else:
                n = int(pc1.shape[-1])
                counts = [n] * B
                packed = (pc1.reshape(1, 3, n) if B == 1 else pc1).transpose(0, 1).reshape(3, B * n).clone()
                rows = flow.transpose(1, 2).reshape(B * n, 3).clone()
            self._fill = (packed.contiguous(), rows.contiguous(), _prefix_of(counts))
            self._pc1 = self._flow = None
        return self._fill


class DenseFlow(object):
    """Scene flow at any query points from one sampled forward.

    The output at a pc1 point depends on that point only through its level-0 barycentric slice of bcn1_ (the last Up layer)
    and the per-point head conv2 -> conv3 -> conv4.  `forward` runs the model's pair-batched inference path (the native
    plan's launches) and also keeps bcn1_'s vertex activation Z (bcn1_'s stack minus its trailing bias-only 1x1 in
    HPLFlowNet, C = 1024, ~106 MB per pair at N = 8 192; the whole stack in HPLFlowNetShallow, C = 128).  `query` locates points in pc1's level-0 lattice (hpl_lattice_query: no
    insertion), slices Z there and runs the head:

        df = DenseFlow(model)                       # eval-mode model, under torch.no_grad()
        flow, state = df.forward(pc1, pc2, lat)     # flow == model(pc1, pc2, lat), bit for bit
        qflow, cov = df.query(state, q)             # (3, Q) query flow, (Q,) coverage

    A query whose simplex vertices are not all vertices of pc1's lattice gets the found ones only (renormalize: rescaled to sum
    to 1); coverage 0 leaves the head's bias-only output, which the caller masks.  Batches (lattices of build_native_batch)
    take lists of B query clouds and return lists.  Lattices without a native level-0 table (the reference wire format),
    training lattices, autograd and mismatched shapes raise HplError before any launch."""

    #: rows per pass of the query head: a 1024-wide fp32 matrix reaches the 2 GiB limit of the 32-bit offsets near 524 k rows
    CHUNK = 65536
    MAX_CHUNK = (1 << 31) // (4 * 1024) - 1

    def __init__(self, model):
        if not isinstance(model, _FlowNetBase):
            raise _lib.HplError('DenseFlow wraps an HPLFlowNet or HPLFlowNetShallow')
        self.model = model

    def _refuse(self):
        if torch.is_grad_enabled():
            raise _lib.HplError('DenseFlow is inference only: run it under torch.no_grad()')
        if self.model.training:
            raise _lib.HplError('DenseFlow needs the model in eval mode')

    def forward(self, pc1, pc2, lat):
        """-> (flow as model(pc1, pc2, lat) returns it, DenseState).  lat: a NativeLattice of build_native /
        build_native_batch."""
        self._refuse()
        info = getattr(lat, 'query_info', None)
        if info is None or getattr(lat, 'tables', None) is None:
            raise _lib.HplError('DenseFlow needs a natively built lattice (build_native / build_native_batch): this one has no '
                                'level-0 table to query')
        B = batch_of(pc1, pc2, lat, False, True)
        dev = pc1[0].device if isinstance(pc1, (list, tuple)) else pc1.device
        if not dev.type == 'cuda':
            raise _lib.HplError('the HIP path needs device tensors (no CPU fallback)')
        keep = []
        self.model._dense_keep = keep            # the pair-batched Python path: the native plan's launches, bcn1_'s Z kept
        try:
            flow = self.model(pc1, pc2, lat)
        finally:
            self.model._dense_keep = None
        if len(keep) != 1 or keep[0].shape[0] != int(lat.tables[0].H0):
            raise _lib.HplError('DenseFlow: the forward did not run the pair-batched path')
        return flow, DenseState(lat, keep[0], B, pc1, flow)

    def query(self, state, q, renormalize=True, chunk=None, fill=None, k=3):
        """q: (3, Q) float32 device tensor (single pair), or a list of B (3, Q_b) tensors (batch) -> (qflow (3, Q), coverage
        (Q,)), or two lists.  fill='knn' (DESIGN.md §17): a query of coverage c < 1 gets c * (the lattice answer) + (1 - c) *
        (the forward's flow interpolated from its pair's k nearest sampled points, ops.knn_interpolate); coverage is returned
        as the lattice gave it."""
        self._refuse()
        if not isinstance(state, DenseState):
            raise _lib.HplError('query takes the state DenseFlow.forward returned')
        if fill is not None:
            if fill != 'knn':
                raise _lib.HplError('fill = %r (None or \'knn\')' % (fill,))
            if not renormalize:
                raise _lib.HplError('fill=\'knn\' blends with the renormalised lattice answer: renormalize=False is refused')
            if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 8:
                raise _lib.HplError('fill=\'knn\' takes k in 1 .. 8, got %r' % (k,))
        chunk = self.CHUNK if chunk is None else int(chunk)
        if chunk < 1 or chunk > self.MAX_CHUNK:
            raise _lib.HplError('chunk of %d rows (1 .. %d)' % (chunk, self.MAX_CHUNK))
        listed = isinstance(q, (list, tuple))
        qs = list(q) if listed else [q]
        if state.batch > 1 and (not listed or len(qs) != state.batch):
            raise _lib.HplError('a lattice of %d pairs takes a list of %d query clouds' % (state.batch, state.batch))
        if state.batch == 1 and listed and len(qs) != 1:
            raise _lib.HplError('a single-pair lattice takes one query cloud, got %d' % len(qs))
        dev = state.Z.device
        for t in qs:
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != 3 or t.dtype != torch.float32 or t.device != dev:
                raise _lib.HplError('every query cloud is a (3, Q) float32 tensor on %s' % dev)
        counts = [int(t.shape[1]) for t in qs]
        Q = sum(counts)
        prefix = _prefix_of(counts)
        qcat = (qs[0] if len(qs) == 1 else torch.cat(qs, dim=1)).contiguous()
        qflow = torch.empty((Q, 3), dtype=torch.float32, device=dev)
        cov = torch.empty((Q,), dtype=torch.float32, device=dev)
        if Q:
            bary, off = self.locate(state, qcat, prefix, renormalize, cov)
            for s in range(0, Q, chunk):
                e = min(Q, s + chunk)
                self.head(state, bary[:, s:e].contiguous(), off[:, s:e].contiguous(), qflow[s:e], Q)
            if fill is not None:      # one launch over the whole batch: pair b's queries see pair b's sample only
                packed, rows, rp = state.fill_inputs()
                ops.knn_interpolate(packed, rows, qcat, k=k, ref_prefix=rp, q_prefix=prefix, out=qflow, coverage=cov)
        if not listed:
            return qflow.t(), cov
        return [qflow[a:b].t() for a, b in zip(prefix[:-1], prefix[1:])], [cov[a:b] for a, b in zip(prefix[:-1], prefix[1:])]

    def locate(self, state, q, prefix, renormalize, cov):
        """hpl_lattice_query of (3, Q) queries -> bary (4, Q), off (4, Q); coverage into `cov`."""
        L = _lib.load()
        Q = q.shape[1]
        bary = torch.empty((4, Q), dtype=torch.float32, device=q.device)
        off = torch.empty((4, Q), dtype=torch.int32, device=q.device)
        pre = (ctypes.c_int64 * len(prefix))(*prefix)
        _lib.check(L.hpl_lattice_query(ctypes.byref(state.lat.query_info), q.data_ptr(), Q, pre if state.batch > 1 else None,
                                       1 if renormalize else 0, bary.data_ptr(), off.data_ptr(), cov.data_ptr(), _lib.stream()),
                   'hpl_lattice_query')
        return bary, off

    def head(self, state, bary, off, out, q_total):
        """Slice Z at (bary, off) [n queries], bcn1_'s trailing 1x1 + bias (HPLFlowNet), conv2, conv3, conv4 -> out [n, 3]."""
        m = self.model
        layer = m.bcn1_
        n = bary.shape[1]
        bias = layer.bias if layer.use_bias else None
        mods = list(layer.blur_conv)
        reorder = len(mods) >= 2 and not isinstance(mods[-1], _ConvReLU)
        if not reorder:
            y = ops.slice_raw(state.Z, bary, off, n, bias=bias)
        else:
            conv = _conv_of(mods[-1])
            H0 = state.Z.shape[0]
            # both biases after the slice on either side, so that a query of partial or no coverage gets the same head input
            b = conv.bias if bias is None else (bias if conv.bias is None else (conv.bias + bias))
            if q_total > H0:          # more queries than vertices: the 1x1 on the vertices once (HPL_COND_SHRINK's other side)
                W = state.Zw
                if W is None:
                    W = state.Zw = ops.gconv(state.Z, conv.weight, None, None, H0, 1, act=ops.ACT_NONE, bwd_mode='dense')
                y = ops.slice_raw(W, bary, off, n, bias=b)
            else:
                z = ops.slice_raw(state.Z, bary, off, n)
                y = ops.gconv(z, conv.weight, b, None, n, 1, act=ops.ACT_NONE, bwd_mode='dense')
        y = pointwise_conv(y, m.conv2.conv, True, m.use_leaky)
        y = pointwise_conv(y, m.conv3.conv, True, m.use_leaky)
        pointwise_conv(y, m.conv4, False, m.use_leaky, out=out)
        return out
