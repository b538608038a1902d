"""Train / evaluate driver for the HIP hot path.

Own counterpart of the reference's loops (/root/reference/main.py:95-286) and checkpoint helpers
(/root/reference/main_utils.py:54-64), reduced to what drives the bilateral layers:

* loss `EPE3DLoss` = mean_n ||flow_n - sf_n||_2 (main.py:213, models/epe3d_loss.py:9-10);
* Adam(lr=1e-4, weight_decay=0) over all parameters (main.py:138-140).  The reference's
  `adjust_learning_rate` computes a decayed rate and then resets every group to `args.lr`
  (main_utils.py:14-30), i.e. the rate is constant; so it is here;
* checkpoint dict {'epoch' (next start epoch), 'arch', 'state_dict', 'min_loss', 'optimizer'}
  written as checkpoint.pth.tar, copied to checkpoint_<epoch>.pth.tar when epoch % 10 == 1 and to
  model_best.pth.tar when best (main.py:183-189, main_utils.py:54-64).  The reference saves the
  state_dict of a DataParallel wrapper, so keys carry a 'module.' prefix; it is written (and
  accepted on load, see flownet.load_reference_checkpoint) so files are interchangeable;
* metrics EPE3D / Acc3D strict / Acc3D relax / outliers (evaluation_utils.py:4-19) and, when the reader has cameras,
  EPE2D / Acc2D (:22-36), on the device (ops.flow_metrics_pairs).

What is new relative to the reference: the permutohedral lattice of pair i+1 is built on the GPU
on a second HIP stream while pair i trains (the reference builds it in DataLoader worker
processes on the CPU), and with world_size > 1 every rank trains its own pair and the gradients
are averaged with one bucketed all-reduce over RCCL (parallel.GradAllReducer) -- mean loss over
the global batch, as `.mean()` over a batch would give.

On real data (`--dataset FlyingThings3DSubset|KITTI --data-root DIR`) the training set goes through
`data.Augmentation` with the published settings (configs/train_ours.yaml:40-57, main.py:56-63) and is
visited in a fresh random order every epoch (DataLoader shuffle=True, main.py:67); validation goes
through `data.ProcessData` in order (main.py:76-90).  `--init xavier` gives the reference's start
(xavier-normal weights, zero biases: main_utils.py:33-47, main.py:100-101).
`--device-transforms` runs both transforms on the device instead (data.DeviceAugmentation / DeviceProcessData: the same
protocol from a counter-based random stream).  `--evaluate --dense` on real data also reports the metrics of
the flow at every valid point of each frame, answered from the sampled forward (flownet.DenseFlow): an
interpolation of the sampled forward, not the paper's protocol.

    python -m hplflownet_amd.engine --arch HPLFlowNet --points 8192 --pairs 8 --epochs 1 --ckpt-dir /tmp/ck
    python -m hplflownet_amd.engine --evaluate --resume /tmp/ck/model_best.pth.tar --pairs 4
"""
import argparse
import collections
import os
import shutil
from types import SimpleNamespace

import numpy as np
import torch

from . import data as data_mod
from . import ops, parallel
from ._lib import HplError
from .flownet import HPLFlowNet, HPLFlowNetShallow, load_reference_checkpoint, selfsup_loss
from .lattice import GenerateDataUnsymmetric, LatticePipeline, NativeLatticeBuild
from .synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair

ARCHS = {'HPLFlowNet': (HPLFlowNet, 7), 'HPLFlowNetShallow': (HPLFlowNetShallow, 5)}


def epe3d_loss(flow, sf):
    """flow, sf: (B, 3, N) -> scalar mean end-point error."""
    return torch.norm(flow - sf, p=2, dim=1).mean()


def flow_metrics(pred, gt):
    """pred, gt: (N, 3) tensors -> dict(EPE3D, Acc3DS, Acc3DR, Outliers) (evaluation_utils.py:4-19)."""
    err = torch.norm(gt - pred, dim=-1)
    rel = err / (torch.norm(gt, dim=-1) + 1e-4)
    return {'EPE3D': float(err.mean()),
            'Acc3DS': float(((err < 0.05) | (rel < 0.05)).float().mean()),
            'Acc3DR': float(((err < 0.1) | (rel < 0.1)).float().mean()),
            'Outliers': float(((err > 0.3) | (rel > 0.1)).float().mean())}


# configs/train_ours.yaml:40-57
DATA_PROCESS = {'DEPTH_THRESHOLD': 35., 'NO_CORR': True}
AUG_TOGETHER = {'degree_range': 0.1745329252, 'shift_range': 1., 'scale_low': 0.95, 'scale_high': 1.05,
                'jitter_sigma': 0.01, 'jitter_clip': 0.00}
AUG_PC2 = {'degree_range': 0., 'shift_range': 0.3, 'jitter_sigma': 0.01, 'jitter_clip': 0.00}


def init_weights_(model, init_type='xavier', gain=1.0):
    """Every Conv*/Linear weight drawn as the reference does, biases zeroed (main_utils.py:33-47)."""
    fn = {'normal': lambda w: torch.nn.init.normal_(w, 0.0, gain),
          'xavier': lambda w: torch.nn.init.xavier_normal_(w, gain=gain),
          'kaiming': lambda w: torch.nn.init.kaiming_normal_(w, a=0, mode='fan_in'),
          'orthogonal': lambda w: torch.nn.init.orthogonal_(w, gain=gain)}
    if init_type not in fn:
        raise NotImplementedError('initialization method [%s] is not implemented' % init_type)
    with torch.no_grad():        # in-place through the parameter itself: bumps its version, which the cached
        for m in model.modules():    # weight images of the inference path key on (ops.invalidate_weight_cache)
            name = m.__class__.__name__
            if hasattr(m, 'weight') and ('Conv' in name or 'Linear' in name):
                fn[init_type](m.weight)
                if getattr(m, 'bias', None) is not None:
                    m.bias.zero_()
    ops.invalidate_weight_cache()
    return model


def model_args(nscales, device='cuda', evaluate=False):
    """The reference's config keys the layers read (configs/train_ours.yaml)."""
    return SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:nscales], use_leaky=True, bcn_use_bias=True,
                           bcn_use_norm=True, last_relu=False, DEVICE=device, evaluate=evaluate)


class SyntheticPairs(object):
    """`count` seeded FT3D-like pairs (synthetic.synthetic_pair), resident on the device as (3, N)."""

    def __init__(self, count, num_points, device, first_seed=0):
        self.items = []
        for s in range(first_seed, first_seed + count):
            pc1, pc2, sf = synthetic_pair(num_points, s)
            self.items.append(tuple(torch.from_numpy(np.ascontiguousarray(a.T)).to(device) for a in (pc1, pc2, sf)))

    has_cameras = False        # (no 2D metrics)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]

    def point_counts(self, i):
        return self.items[i][0].shape[-1], self.items[i][1].shape[-1]


class Trainer(object):
    def __init__(self, arch='HPLFlowNet', device='cuda', lr=1e-4, seed=0, distributed=False, rank=0, init='hash',
                 native_step=None, loss='epe3d', selfsup=None):
        self.loss, self.selfsup = loss, selfsup_options(loss, selfsup)
        cls, nsc = ARCHS[arch]
        self.rank = rank
        self.arch, self.device = arch, torch.device(device)
        self.args = model_args(nsc, evaluate=False)
        torch.manual_seed(seed)
        self.model = cls(self.args)
        if init == 'hash':
            fill_module_(self.model, 1.0, 'hash')       # deterministic He-uniform start (no dataset, no RNG state)
        else:
            init_weights_(self.model, init)
        self.shuffle = np.random.RandomState(seed + 7919 * rank)
        self.model.to(self.device)
        self.gen = GenerateDataUnsymmetric(self.args, device=self.device, wide_up=self.model.lattice_hint())
        if self.device.type == 'cuda':
            ops.enable_weight_bank()          # one batched weight re-layout per training step
        # (fused: the same update, two launches instead of sixteen)
        self.opt = torch.optim.Adam([p for p in self.model.parameters() if p.requires_grad], lr=lr, weight_decay=0,
                                    fused=self.device.type == 'cuda')
        self.reducer = None
        if distributed:
            parallel.broadcast_parameters(self.model)
            self.reducer = parallel.GradAllReducer(self.model.parameters())
        self.epoch = 0
        self.min_loss = None
        self._side = torch.cuda.Stream(device=self.device, priority=-1) if self.device.type == 'cuda' else None
        # the training step as one native program (train_plan.TrainPlan: forward + loss + backward enqueued by a handful of C calls,
        # gradients in one flat arena the all-reduce runs on); HPL_NATIVE_TRAIN=0 / native_step=False keep the autograd path
        # loss='selfsup' runs on the autograd path unless native_step is an explicit True: the native program then takes the
        # pairs' losses and gradients from hpl_selfsup_loss between its forward and its backward
        asked = native_step is True
        if native_step is None:
            native_step = os.environ.get('HPL_NATIVE_TRAIN', '1') != '0'
        self.native_step = bool(native_step) and self.device.type == 'cuda' and (loss == 'epe3d' or asked)
        self.tplan = None
        self.native_steps = 0

    def _pair_loss(self, flow, pc1, pc2, sf):
        """The loss of one pair's forward: EPE3D against sf, or (loss='selfsup') the self-supervised loss, which never reads sf."""
        if self.loss == 'selfsup':
            return selfsup_loss(flow, pc1[None], pc2[None], **self.selfsup)[0]
        return epe3d_loss(flow, sf[None])

    def train_step(self, pc1, pc2, sf, lat):
        """One optimiser step on one pair (main.py:203-217) -> the loss (device tensor, not synchronised)."""
        if getattr(lat, 'batch', 1) > 1 or getattr(lat, 'ragged', False):
            raise HplError('train_step takes one pair: a lattice of %d pairs is for batched inference (validate)' % lat.batch)
        self._native_plan()
        if self.tplan is not None:
            if self.loss == 'selfsup':               # (a batch of one pair: pair_losses[0] is its L)
                r = self.tplan.step_batch(pc1[None], pc2[None], None, lat, 'selfsup', self.selfsup)
                r = None if r is None else (r[0], r[2])
            else:
                r = self.tplan.step(pc1, pc2, sf, lat)
            if r is not None:
                self._step_tail(native=True)
                self.native_steps += 1
                return r[1][0].clone()
            self.tplan.gflat.zero_()                 # a lattice the native backward refuses: autograd adds into the same arena
        flow = self.model(pc1[None], pc2[None], lat)
        loss = self._pair_loss(flow, pc1, pc2, sf)
        if self.tplan is None:
            self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self._step_tail(native=False)
        return loss.detach()

    def _step_tail(self, native):
        """The end of every optimiser step, behind its backward: the gradients' all-reduce, then the update.  native: the native
        program ran the backward and reduces in its own bucket order (finish); else autograd did, and with a native plan the
        fallback reduces in that same order -- ranks that ran the native program post the same collectives -- (reduce_fallback),
        without one through the reducer.  The update is one launch over the plan's flat arrays (hpl_adam_flat) where it has
        them, else the optimiser's."""
        if native:
            self.tplan.finish()
        elif self.tplan is not None:
            self.tplan.reduce_fallback()
        elif self.reducer is not None:
            self.reducer()
        if self.tplan is None or not self.tplan.adam_step(self.opt):
            self.opt.step()

    def train_step_batch(self, pc1, pc2, sf, lat):
        """One optimiser step over B pairs: pc1, sf (B, 3, N1), pc2 (B, 3, N2) and their lattice of
        build_native_batch(..., for_training=True) -> the B per-pair losses (device tensor, not synchronised).  The gradient is
        the mean over the pairs (what W ranks of one pair each average); one Adam step per batch.  B = 1 is train_step."""
        from .train_plan import check_batch_step
        B = check_batch_step(pc1, pc2, sf, lat)
        if B == 1:
            return self.train_step(pc1[0], pc2[0], sf[0], lat).reshape(1)
        self._native_plan()
        if self.tplan is not None:
            r = self.tplan.step_batch(pc1, pc2, sf, lat, self.loss, self.selfsup)
            if r is not None:
                self._step_tail(native=True)
                self.native_steps += 1
                return r[2]
            self.tplan.gflat.zero_()                 # the native program refuses the batch: autograd adds into the same arena
        else:
            self.opt.zero_grad(set_to_none=True)
        return self._per_pair_fallback(pc1, pc2, sf, B)

    def _native_plan(self):
        """The native training program, made at the first step that wants it."""
        if self.native_step and self.tplan is None:
            from .train_plan import TrainPlan
            if self.reducer is None:
                self.reducer = parallel.GradAllReducer(self.model.parameters(), overlap=False)
            self.tplan = TrainPlan(self.model, reducer=self.reducer)

    def _per_pair_fallback(self, pc1, pc2, sf, B):
        """The autograd path of a batch: pair by pair on single-pair training lattices, each loss scaled by 1 / B -- the same
        mean-over-pairs gradient --, then ONE all-reduce (in the native program's bucket order) and ONE optimiser step: ranks
        keep posting the same collectives."""
        losses = []
        for b in range(B):
            lb = self._single_lattice(pc1[b], pc2[b])
            flow = self.model(pc1[b][None], pc2[b][None], lb)
            loss = self._pair_loss(flow, pc1[b], pc2[b], sf[b])
            (loss / B).backward()
            losses.append(loss.detach())
        self._step_tail(native=False)
        return torch.stack(losses)

    def _single_lattice(self, pc1, pc2):
        """One pair's training lattice (tables of the backward included), built on the current stream."""
        if self.gen.native_supported():
            return NativeLatticeBuild(self.gen, pc1, pc2, for_training=True).finish()
        return self.gen.build(pc1.contiguous(), pc2.contiguous()).prepare(True)

    # ------------------------------------------------------------------ lattice pipeline
    def _lattices(self, data, order, training, depth=2, batch_size=1):
        """Yield (sample, lattice) for `order`.  Each sample is fetched once (readers may sample randomly);
        the lattices of the next `depth` samples are under construction on the side stream while the
        current one is consumed, and the host never blocks on their vertex-count read-backs.  batch_size = B > 1
        (native builder): consecutive samples of `order` with equal point counts (batch_groups) come as one stacked
        sample ((B, 3, N) each) with one batched lattice."""
        main = torch.cuda.current_stream(self.device)
        native = self.gen.native_supported()
        # the native (fused) builder drives both; in training it also adds the tables of the backward (tap lists, symmetry
        # verdicts) -- on a producer thread, off the thread that issues the step's launches
        groups = None
        if batch_size > 1:
            if not native:
                raise HplError('batches of %d pairs need the native lattice builder' % batch_size)
            groups = batch_groups([point_counts(data, k) for k in order], batch_size)
        pipe = LatticePipeline(self.gen, lambda k: data[order[k]], 0, len(order), depth=depth, stream=self._side,
                               for_training=training, native=native, threaded=training and native,
                               batch=batch_size, groups=groups)
        keep = collections.deque()
        try:
            for _ in range(len(order) if groups is None else len(groups)):
                (_, sample), lat, ev = pipe.get()
                main.wait_event(ev)
                yield sample, lat
                fin = torch.cuda.Event()
                fin.record(main)
                keep.append((lat, sample, fin))         # side-stream memory stays alive until its consumer is done
                while len(keep) > 2:
                    keep.popleft()[2].synchronize()
        finally:
            pipe.close()                                # (a consumer that stops early must not leave the producer thread behind)
            for _, _, fin in keep:
                fin.synchronize()

    # ------------------------------------------------------------------ loops
    def train_epoch(self, data, order=None, batch_size=1):
        """One pass over `order`; batch_size = B > 1: one step per group of <= B consecutive samples with equal point counts
        (train_step_batch).  -> the mean loss over the pairs of all ranks."""
        self.model.train()
        order = list(range(len(data))) if order is None else list(order)
        total = torch.zeros((), device=self.device)
        if batch_size > 1:
            for (pc1, pc2, sf), lat in self._lattices(data, order, True, batch_size=batch_size):
                total += self.train_step_batch(pc1, pc2, sf, lat).sum()
        else:
            for (pc1, pc2, sf), lat in self._lattices(data, order, True):
                total += self.train_step(pc1, pc2, sf, lat)
        self.epoch += 1
        tot = parallel.sum_over_ranks([float(total), float(len(order))], device=self.device)
        return tot[0] / max(1.0, tot[1])             # mean loss over the global batch stream (all ranks)

    @torch.no_grad()
    def validate(self, data, batch_size=1, ragged=False, dense=False, dense_fill=None, dense_k=3, rigid=None, segment=None,
                 icp=None, objects=None, write=None):
        """Metrics of `data` (means over its pairs, all ranks).  batch_size = B > 1: runs of consecutive pairs with the same
        point counts are evaluated B at a time (one batched lattice build and one batched forward); a pair whose counts
        differ from its neighbours' forms a batch of its own.  ragged=True: consecutive pairs are batched whatever their
        counts (ragged_groups: <= B pairs and <= RAGGED_POINT_BUDGET points per cloud side a batch).  `val_batches`: the
        forwards this rank ran.

        The keys are EPE3D / Acc3DS / Acc3DR / Outliers, plus EPE2D / Acc2D when the reader has cameras (`has_cameras`): the
        reader decides, not the samples, so every rank issues the same collective.  Each forward is followed on its stream by
        one hpl_flow_metrics launch over its pairs, into a (len(data), 8) device array at the pairs' sample indices; that array
        is read back once.  `val_pairs`: this rank's [(index into data, {metric: value})] in sample order.

        dense=True (a DenseFrames reader): every forward also answers the flow at all valid points of its frames
        (DenseFlow.query); those flows go through the same metrics into a second array, and the keys gain dense_<metric> plus
        dense_coverage (the mean query coverage) and dense_full (the fraction of queries whose vertices were all found), all
        means over pairs.  dense_fill='knn' (with dense_k neighbours): the part of a query the lattice does not
        cover is filled from the sampled flow (DenseFlow.query(fill='knn')); the same keys, then of the filled flow.

        rigid={'iters': T, 'tau': tau}: behind each forward's metrics launch one ops.rigid_fit over that forward's
        pairs -- the robust rigid fit of (pc1, sampled flow) per pair; the flow is read in place, the clouds of a forward of
        B > 1 pairs are packed with one copy first -- and one more metrics launch of the refined flow into a third array; the
        forwards' fit statistics stay on the device and come back, joined by one concatenation, with the read-back.  The keys gain
        rigid_<metric> plus rigid_inliers (the inlier share), rigid_angle_deg and rigid_trans (the fitted rotation angle and
        |t|), means over pairs.  With dense=True the refinement is still of the sampled flow.

        segment={'eps': e, 'dv': v, 'min_points': m} (with rigid): the fit also returns its residuals and one
        ops.motion_segment call per forward groups the points above the fit's tau into moving objects.  Its integer counts stay
        on the device and come back with the read-back.  The keys gain seg_objects (objects per pair), seg_moving (the share
        of a pair's points in objects) and seg_noise (the share labelled -2: movers in no object), means over pairs.

        icp={'iters': T, 'max_dist': d, 'tau': tau, 'init': 'identity' | 'rigid'}: behind each forward one
        ops.icp over that forward's pairs registers pc1 onto pc2 from the clouds alone -- the ICP baseline of the scene-flow
        papers, independent of the model's output -- or, with init='rigid' (which takes rigid), starting from that forward's
        rigid fit: network + ICP.  The flow R p + t - p goes through one more metrics launch into an array of its own; the
        (B, 6) statistics stay on the device and come back with the read-back.  The keys gain icp_<metric> plus icp_matched,
        icp_rmse, icp_angle_deg, icp_trans and icp_rounds, means over pairs.

        objects={'iters': T, 'tau': tau} (with rigid and segment; {}: the fit's values): one ops.object_fit call
        per forward fits every listed object's own rigid motion on the labels just computed -- no read-back -- and the
        piecewise-rigid flow (the ego-motion's rigid flow at its inliers, an object's at the inliers of its fit, the sampled flow
        elsewhere) goes through one more metrics launch into an array of its own.  Behind every other key, and changing none,
        the keys gain piecewise_<metric> plus piecewise_object_inliers: the share of a pair's points whose flow an object fit
        replaced, from integer counts that stay on the device until the read-back.

        write=callable(samples, pc1s, flows) (KittiWriter): called behind every forward with the flow that is
        evaluated -- the dense flow at all valid points with dense=True, else the sampled one -- and the clouds it belongs to.
        It changes no key and no value."""
        if dense_fill is not None and not dense:
            raise HplError('validate: dense_fill applies to dense=True')
        if rigid is not None:
            rigid = _options('rigid', rigid)
        if segment is not None:
            if rigid is None:
                raise HplError('validate: segment applies to rigid')
            segment = segment_options(segment)
        if objects is not None:
            if rigid is None or segment is None:
                raise HplError('validate: objects applies to rigid with segment')
            objects = object_options(objects, rigid)
        if icp is not None:
            _known_keys('icp', icp)
            if icp.get('metric') != 'plane' and ('normals_k' in icp or 'normals_radius' in icp):
                raise HplError(_GROUPS['icp'].takes % (icp,))
            if icp.get('init') == 'rigid' and rigid is None:
                raise HplError('validate: icp init \'rigid\' starts from the rigid fit: it takes rigid')
            icp = _GROUPS['icp'].filled(icp, None)
            icp_init = icp.pop('init')
            if icp.get('metric') != 'plane':     # (point-to-plane, DESIGN.md §29: icp_register runs ops.normals on pc2)
                icp.pop('metric', None)
        self.model.eval()
        cams = bool(getattr(data, 'has_cameras', False))
        keys = metric_keys(data)
        dkeys = ['dense_' + k for k in keys] + ['dense_coverage', 'dense_full'] if dense else []
        rkeys = ['rigid_' + k for k in keys] + list(RIGID_STATS) if rigid is not None else []
        rkeys = rkeys + list(SEGMENT_STATS) if segment is not None else rkeys
        rkeys = rkeys + ['icp_' + k for k in keys] + list(ICP_STATS) if icp is not None else rkeys
        rkeys = rkeys + ['piecewise_' + k for k in keys] + list(OBJECT_STATS) if objects is not None else rkeys
        self.val_batches = 0
        self.val_pairs = []
        forward = lambda p1, p2, lat, samples: self.model(p1, p2, lat)       # noqa: E731
        n = len(data)
        if n > 0:
            nxt = [0]                                    # sample index of the next pair (groups are runs of consecutive samples)
            rows = _Rows(n, self.device, cams, nxt)
            if dense:
                from .flownet import DenseFlow
                drows, dflow = _Rows(n, self.device, cams, nxt, 'dense_'), DenseFlow(self.model)
                dcov = torch.zeros((n, 2), dtype=torch.float64, device=self.device)
            if rigid is not None:
                rrows, rstats = _Rows(n, self.device, cams, nxt, 'rigid_'), []      # every forward's (B, 4) fit statistics, on the device
                sstats, scounts = [], []                 # segment: every forward's (B, 4) integer counts, on the device
            if objects is not None:
                orows, ocounts = _Rows(n, self.device, cams, nxt, 'piecewise_'), []  # every forward's (B,) counts of the replaced rows
            if icp is not None:
                irows, istats = _Rows(n, self.device, cams, nxt, 'icp_'), []        # every forward's (B, 6) registration statistics

            def add(preds, samples, batched=None):
                rows.add(preds, samples, samples)
                if write is not None and not dense:
                    write(samples, [s_[0] for s_ in samples], list(preds))
                fitted = None
                if rigid is not None:
                    from .flownet import rigid_refine
                    # an equal batch goes as the forward's own (B, 3, N) tensors: its flow rows are read in place
                    pc1, flow = batched if batched is not None else ([s_[0] for s_ in samples], list(preds))
                    if segment is None:
                        fit = rigid_refine(pc1, flow, **rigid)
                    elif objects is not None:
                        from .flownet import _piecewise
                        whole = _piecewise(pc1, flow, None, rigid['iters'], rigid['tau'], objects['iters'], objects['tau'], None,
                                           segment, keep_ego=True)
                        fit = whole.fit
                        sstats.append(whole.seg[3])
                        scounts.extend(int(s_[0].shape[1]) for s_ in samples)
                        ocounts.append(whole.replaced)
                    else:
                        from .flownet import segment_motion
                        fit = rigid_refine(pc1, flow, return_residual=True, **rigid)
                        sstats.append(segment_motion(pc1, flow, rigid=fit, tau=rigid['tau'], **segment)[3])
                        scounts.extend(int(s_[0].shape[1]) for s_ in samples)
                    fitted = (fit[0], fit[1])
                    rstats.append(fit[2])        # (sample order: the groups are runs of consecutive samples)
                    rrows.add(list(fit[3]), samples, samples)
                    if objects is not None:
                        orows.add(list(whole.refined), samples, samples)
                if icp is not None:
                    from .flownet import icp_register
                    res = icp_register([s_[0] for s_ in samples], [s_[1] for s_ in samples],
                                       init=fitted if icp_init == 'rigid' else None, **icp)
                    istats.append(res[2])
                    irows.add(list(res[3]), samples, samples)
                nxt[0] += len(samples)

            def dense_forward(p1, p2, lat, samples):
                """The forward through DenseFlow, the frames' full clouds queried behind it (their metrics are added before the
                sampled ones': both write the rows from the same sample index)."""
                flow, state = dflow.forward(p1, p2, lat)
                fulls = [s_.dense for s_ in samples]
                qs = [f[0] for f in fulls]
                qf, cov = dflow.query(state, qs if state.batch > 1 else qs[0], fill=dense_fill, k=dense_k)
                if state.batch == 1:
                    qf, cov = [qf], [cov]
                drows.add(qf, fulls, samples)
                if write is not None:
                    write(samples, qs, list(qf))
                for b, c in enumerate(cov):
                    dcov[nxt[0] + b, 0] = c.double().mean()
                    dcov[nxt[0] + b, 1] = (c == 1).double().mean()
                return flow
            try:
                self._validate_forwards(data, batch_size, ragged, add, dense_forward if dense else forward)
                rows.read()                              # the one read-back (it follows every launch on this stream)
                if dense:
                    drows.read()
                    dcv = dcov.cpu().numpy()
                if rigid is not None:
                    rrows.read()
                    rst = torch.cat(rstats).cpu().numpy()
                    if segment is not None:
                        sst = torch.cat(sstats).cpu().numpy()
                    if objects is not None:
                        orows.read()
                        oct_ = torch.cat(ocounts).cpu().numpy()
                if icp is not None:
                    irows.read()
                    ist = torch.cat(istats).cpu().numpy()
            finally:
                torch.cuda.current_stream(self.device).synchronize()     # the stage's copies have run before it is released
            self.val_pairs = [(i, rows.fold(i)) for i in range(n)]
            for i, v in self.val_pairs:
                if dense:
                    v.update(drows.fold(i))
                    v['dense_coverage'], v['dense_full'] = float(dcv[i, 0]), float(dcv[i, 1])
                if rigid is not None:
                    v.update(rrows.fold(i))
                    v.update(zip(RIGID_STATS, (float(x) for x in rst[i, 1:])))
                    if segment is not None:
                        v.update(zip(SEGMENT_STATS, segment_fold(sst[i], scounts[i])))
                if icp is not None:
                    v.update(irows.fold(i))
                    v.update(zip(ICP_STATS, (float(x) for x in ist[i, 1:])))
                if objects is not None:
                    v.update(orows.fold(i))
                    v['piecewise_object_inliers'] = int(oct_[i]) / max(1, scounts[i])
        keys = keys + dkeys + rkeys
        agg = [sum(v[k] for _, v in self.val_pairs) for k in keys]      # (in sample order)
        # every rank evaluated its own shard (shards may differ in length by one): sums and the sample count are
        # added over the ranks, so all ranks return the metrics of the WHOLE split (and agree on `best` in fit())
        tot = parallel.sum_over_ranks(agg + [float(n)], device=self.device)
        self.val_samples = int(tot[-1])         # over all ranks: 0 = no rank had a validation sample
        return {k: v / max(1.0, tot[-1]) for k, v in zip(keys, tot[:-1])}

    def _validate_forwards(self, data, batch_size, ragged, add, forward):
        """The forwards of validate(): flow = forward(p1, p2, lat, samples) -- the model's, or the dense rider's around it --, then
        add(preds, samples), preds[b] the (3, N_b) flow view of samples[b]; an equal batch adds its own (pc1, flow) tensors, both
        (B, 3, N), as a third argument."""
        if batch_size > 1 and ragged:
            for group in self._ragged_batches(data, batch_size):
                p1, p2 = [g[0] for g in group], [g[1] for g in group]
                flows = forward(p1, p2, self.gen.build_native_batch(p1, p2), group)      # (a list of one pair: build_native)
                self.val_batches += 1
                add([f[0] for f in flows], group)
        elif batch_size > 1:
            for group in self._batches(data, batch_size):
                p1 = torch.stack([g[0] for g in group])
                p2 = torch.stack([g[1] for g in group])
                lat = self.gen.build_native_batch(p1, p2) if len(group) > 1 else self.gen.build_native(p1[0], p2[0])
                flow = forward(p1, p2, lat, group)
                self.val_batches += 1
                add(list(flow), group, (p1, flow))
        else:
            for s_, lat in self._lattices(data, list(range(len(data))), False):
                flow = forward(s_[0][None], s_[1][None], lat, [s_])
                self.val_batches += 1
                add([flow[0]], [s_])

    @staticmethod
    def _batches(data, batch_size):
        """Consecutive samples of `data` (each fetched once) in groups of <= batch_size with equal point counts."""
        return _grouped((data[i] for i in range(len(data))), _sample_counts, _equal_rule(batch_size))

    @staticmethod
    def _ragged_batches(data, batch_size, budget=None):
        """Consecutive samples of `data` (each fetched once, in order) in the groups of ragged_groups."""
        return _grouped((data[i] for i in range(len(data))), _sample_counts,
                        _ragged_rule(batch_size, RAGGED_POINT_BUDGET if budget is None else budget))

    # ------------------------------------------------------------------ checkpoints
    def state(self):
        # (the native training step keeps parameters and Adam moments as views of flat arrays -- train_plan.TrainPlan --: a
        # checkpoint holds tensors of their own, as the reference's does)
        sd = collections.OrderedDict(('module.' + k, v.detach().clone()) for k, v in self.model.state_dict().items())
        osd = self.opt.state_dict()
        osd['state'] = {i: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in osd['state'].items()}
        return {'epoch': self.epoch, 'arch': self.arch, 'state_dict': sd, 'min_loss': self.min_loss,
                'optimizer': osd}

    def save_checkpoint(self, ckpt_dir, is_best, filename='checkpoint.pth.tar'):
        os.makedirs(ckpt_dir, exist_ok=True)
        path = os.path.join(ckpt_dir, filename)
        st = self.state()
        torch.save(st, path)
        if st['epoch'] % 10 == 1:
            shutil.copyfile(path, os.path.join(ckpt_dir, 'checkpoint_%d.pth.tar' % st['epoch']))
        if is_best:
            shutil.copyfile(path, os.path.join(ckpt_dir, 'model_best.pth.tar'))
        return path

    def resume(self, path, load_optimizer=True):
        ck = torch.load(path, map_location='cpu')
        load_reference_checkpoint(self.model, ck, strict=True)
        if isinstance(ck, dict):
            self.epoch = int(ck.get('epoch', 0))
            self.min_loss = ck.get('min_loss')
            if load_optimizer and 'optimizer' in ck:
                self.opt.load_state_dict(ck['optimizer'])
        return ck

    def fit(self, train_data, val_data, epochs, ckpt_dir=None, log=print, shuffle=False, batch_size=1):
        for _ in range(self.epoch, epochs):
            tr = self.train_epoch(train_data, self.shuffle.permutation(len(train_data)) if shuffle else None, batch_size)
            # validate() ends in a collective: every rank calls it whenever the split exists, also with an empty shard
            # (fewer validation samples than ranks); the decision to fall back to the train loss is taken on the
            # globally reduced sample count so that all ranks agree
            val, metrics = tr, ''
            if val_data is not None:
                res = self.validate(val_data)
                if self.val_samples > 0:
                    val = res['EPE3D']
                    metrics = '  (val %s)' % ' '.join('%s %.4f' % kv for kv in res.items())
            best = self.min_loss is None or val < self.min_loss
            if best:
                self.min_loss = val
            log('epoch %d  train EPE3D %.5f  val EPE3D %.5f%s%s' % (self.epoch, tr, val, '  (best)' if best else '', metrics))
            if ckpt_dir and self.rank == 0:
                self.save_checkpoint(ckpt_dir, best)
        return self.min_loss


class _Rows(object):
    """validate()'s metric rows under a key prefix: the (n, 8) float64 sums of one flow per pair on the device, written at the
    pairs' sample indices (`nxt`) by one hpl_flow_metrics launch per forward, and their pinned descriptor rows (one per sample:
    no row is refilled in a call)."""

    def __init__(self, n, device, cams, nxt, prefix=''):
        self.cams, self.nxt, self.prefix = cams, nxt, prefix
        self.sums = torch.zeros((n, 8), dtype=torch.float64, device=device)
        self.stage = ops.MetricsStage(n, device)

    def add(self, flows, clouds, samples):
        """A forward's pairs: flows[b] measured on clouds[b] = (pc1, pc2, sf), with the camera of samples[b]."""
        cameras = [getattr(s_, 'camera', None) if self.cams else None for s_ in samples]
        missing = [b for b, cam in enumerate(cameras) if self.cams and cam is None]
        if missing:
            raise HplError('validate: the reader has cameras, but sample %d came without one' % (self.nxt[0] + missing[0]))
        ops.flow_metrics_pairs(flows, [c[2] for c in clouds], [c[0] for c in clouds], cameras, self.sums, self.nxt[0], self.stage)

    def read(self):
        self.words = self.sums.cpu().numpy()

    def fold(self, i):
        return {self.prefix + k: x for k, x in ops.flow_metrics_fold(self.words[i], self.cams).items()}


def selfsup_options(loss, selfsup):
    """Trainer's loss / selfsup arguments, checked: None for 'epe3d', else {'k': 8, 'w_chamfer': 1.0, 'w_smooth': 1.0} with the
    given entries in place."""
    if loss not in ('epe3d', 'selfsup'):
        raise HplError('Trainer: loss is \'epe3d\' or \'selfsup\', got %r' % (loss,))
    if loss == 'epe3d':
        if selfsup is not None:
            raise HplError('Trainer: selfsup options apply to loss=\'selfsup\'')
        return None
    o = _options('selfsup', {} if selfsup is None else selfsup)
    # (wider than the command line: k = 0 switches the smoothness term off, and k is taken as the int it is, never cast)
    if isinstance(o['k'], bool) or not isinstance(o['k'], int) or not 0 <= o['k'] <= 8 or \
            not 0 <= o['w_chamfer'] < float('inf') or not 0 <= o['w_smooth'] < float('inf') or (o['k'] == 0 and o['w_smooth'] != 0):
        raise HplError(_GROUPS['selfsup'].needs_text % (selfsup,))
    return o


#: validate(segment=...): the per-pair keys from hpl_motion_segment's integer counts
SEGMENT_STATS = ('seg_objects', 'seg_moving', 'seg_noise')


def segment_options(segment):
    """validate's segment argument, checked and with its defaults: {'eps': 0.5, 'dv': inf, 'min_points': 5}."""
    return _options('segment', segment, ranges=True)


#: validate(objects=...): the per-pair key beside the piecewise_<metric> keys
OBJECT_STATS = ('piecewise_object_inliers',)


def object_options(objects, rigid):
    """validate's objects argument, checked and with its defaults: the rigid fit's iters and tau."""
    return _options('objects', objects, {'rigid': rigid}, ranges=True)


def segment_fold(row, points):
    """(seg_objects, seg_moving, seg_noise) of one pair of `points` points from its (movers, objects, points in objects, out of
    range) counts."""
    movers, objects, inside, _ = (int(x) for x in row)
    return float(objects), inside / max(1, points), (movers - inside) / max(1, points)


#: validate(rigid=...): the per-pair fit statistics beside the rigid_<metric> keys (stats[1:] of ops.rigid_fit)
RIGID_STATS = ('rigid_inliers', 'rigid_angle_deg', 'rigid_trans')
#: validate(icp=...): the per-pair registration statistics beside the icp_<metric> keys (stats[1:] of ops.icp)
ICP_STATS = ('icp_matched', 'icp_rmse', 'icp_angle_deg', 'icp_trans', 'icp_rounds')


def metric_keys(data):
    """The keys validate() reports for a reader: the four 3D metrics, and EPE2D / Acc2D when it has cameras (`has_cameras`).  Decided
    from the reader alone, never from its samples: a rank with an empty shard reports (and reduces) the same keys."""
    return list(ops.METRICS_3D) + (list(ops.METRICS_2D) if getattr(data, 'has_cameras', False) else [])


# ---------------------------------------------------------------------- batches: two grouping rules, each stated once
def _sample_counts(s_):
    """(N1, N2) of a sample (pc1, pc2, sf), (3, N) each."""
    return (int(s_[0].shape[-1]), int(s_[1].shape[-1]))


def same_counts(a, b):
    """True if samples a and b ((pc1, pc2, sf), (3, N) each) have the same point counts: they can share a batch."""
    return _sample_counts(a) == _sample_counts(b)


def point_counts(data, i):
    """(N1, N2) of sample i of a reader: its point_counts(i) if it has one (no fetch), else the shapes of data[i]."""
    f = getattr(data, 'point_counts', None)
    return tuple(f(i)) if f is not None else _sample_counts(data[i])


def _grouped(items, counts, closes):
    """Consecutive `items` in groups, each item drawn once and in order (a reader may sample randomly): closes(held, c) -- held
    the counts of the open group's members, c = counts(item) those of the next item -- ends the group before that item."""
    group, held = [], []
    for x in items:
        c = counts(x)
        if group and closes(held, c):
            yield group
            group, held = [], []
        group.append(x)
        held.append(c)
    if group:
        yield group


def _equal_rule(batch_size):
    """Equal counts, at most batch_size."""
    return lambda held, c: len(held) >= batch_size or held[0] != c


def _ragged_rule(batch_size, budget):
    """At most batch_size pairs and the point budget (ragged_closes)."""
    return lambda held, c: ragged_closes(len(held), (sum(h[0] for h in held), sum(h[1] for h in held)), c, batch_size, budget)


def batch_groups(counts, batch_size):
    """Index groups validate(batch_size=...) forms from per-sample point counts [(n1, n2), ...]: consecutive, equal
    counts, at most batch_size each."""
    return list(_grouped(range(len(counts)), counts.__getitem__, _equal_rule(batch_size)))


#: points per cloud side of a ragged evaluation batch: at most the largest batch DESIGN.md §11 ran (B = 16 x N = 8 192), well
#: inside the forward's 32-bit limits (lattice.MAX_RAGGED_POINTS)
RAGGED_POINT_BUDGET = 131072


def ragged_closes(n, tot, c, batch_size, budget):
    """True if a group of n pairs holding tot = (points of cloud 1, of cloud 2) closes before a pair of counts c."""
    return n >= batch_size or tot[0] + c[0] > budget or tot[1] + c[1] > budget


def ragged_groups(counts, batch_size, budget=RAGGED_POINT_BUDGET):
    """Index groups validate(batch_size=..., ragged=True) forms from per-sample point counts [(n1, n2), ...]: consecutive,
    whatever the counts, at most batch_size each and at most `budget` points per cloud side (a pair above it alone)."""
    return list(_grouped(range(len(counts)), counts.__getitem__, _ragged_rule(batch_size, budget)))


# ---------------------------------------------------------------------- the options, declared once
_INF = float('inf')
_OMIT = object()                 # an option's value when it is not given: its key is left out of the group's dict
_POS = (lambda v: 0 < v < _INF, 'a finite value > 0')
_NONNEG = (lambda v: 0 <= v < _INF, 'a finite value >= 0')
_Check = collections.namedtuple('Check', 'group bad text')       # a check of parse_args whose sentence has no regular form


def _within(lo, hi):
    return (lambda v: lo <= v <= hi, '%d .. %d' % (lo, hi))


def _as_is(v):
    return v


class _Flag(object):
    """One flag of the command line; _FLAGS holds them in the order of --help, a _Check at its place among its group's options.
    With a group the flag is one of its options: `key` its name in the group's dict and in the programmatic argument, `unset`
    its value when not given (a value, _OMIT, or a function of the groups built so far: another option's value), `takes` =
    (range predicate, its words), `on` = (switch, its words) where the option's switch is narrower than its group's, `cast`
    what the programmatic side applies to a value (default: the flag's type).  The keywords are add_argument's."""

    def __init__(self, flag, group=None, key=None, unset=None, takes=None, on=None, cast=None, **kw):
        self.flag, self.dest, self.group, self.key, self.unset, self.on, self.kw = \
            flag, flag[2:].replace('-', '_'), group, key, unset, on, kw
        self.ok, self.takes = takes or ((lambda v: True), None)
        self.cast = cast or kw.get('type') or _as_is


class _Group(object):
    """A group of options; _GROUPS holds them in the order parse_args checks them.  `flag` [`value`] names the switch in the
    options' "applies to ..." and `on` reads it; `needs` = (what the switch itself requires, its words).  as_dict: parse_args
    leaves a.<name> = {key: value}, None with the switch off, and the programmatic side takes the same dict: `takes` is its
    refusal of an unknown key or of a value outside an option's choices, `needs_text` that of a range, where it checks one."""

    def __init__(self, name, flag, on, needs, value=None, as_dict=True, takes=None, needs_text=None):
        self.name, self.flag, self.on, self.needs, self.as_dict, self.takes, self.needs_text = \
            name, flag, on, needs, as_dict, takes, needs_text
        self.applies = flag if value is None else '%s %s' % (flag, value)

    def rows(self):
        return [r for r in _FLAGS if r.group == self.name]

    def options(self):
        return [r for r in self.rows() if getattr(r, 'key', None) is not None]

    def filled(self, given, built, rows=None):
        """{key: value}: given[key] where it is given, else the option's value when unset."""
        o = {}
        for r in self.options() if rows is None else rows:
            v = given[r.key] if r.key in given else r.unset(built) if callable(r.unset) else r.unset
            if v is not _OMIT:
                o[r.key] = r.cast(v)
        return o


def _known_keys(name, given):
    g = _GROUPS[name]
    if not isinstance(given, dict) or set(given) - {r.key for r in g.options()} or \
            any(r.key in given and given[r.key] not in r.kw['choices'] for r in g.options() if 'choices' in r.kw):
        raise HplError(g.takes % (given,))


def _options(name, given, built=None, ranges=False):
    """The programmatic side of a group: `given` checked against the declared keys, then filled and cast; ranges=True: the
    options' ranges checked too (validate's rigid and icp leave theirs to the op wrappers)."""
    _known_keys(name, given)
    o = _GROUPS[name].filled(given, built)
    if ranges and not all(r.ok(o[r.key]) for r in _GROUPS[name].options()):
        raise HplError(_GROUPS[name].needs_text % (given,))
    return o


_ON_KITTI = (lambda a: a.dataset == 'KITTI', '--dataset KITTI')
_GROUPS = collections.OrderedDict((g.name, g) for g in (
    _Group('write', '--write-kitti', lambda a: a.write_kitti is not None, as_dict=False,
          needs=(lambda a: a.evaluate and a.dataset == 'KITTI' and a.kitti_calib is not None,
                 '--evaluate --dataset KITTI with --kitti-calib DIR')),
    _Group('run', None, lambda a: False, None, as_dict=False),
    _Group('dense', '--dense', lambda a: a.dense, as_dict=False,
          needs=(lambda a: a.evaluate and a.dataset != 'synthetic', '--evaluate with --dataset FlyingThings3DSubset|KITTI')),
    _Group('rigid', '--rigid-refine', lambda a: a.rigid_refine, needs=(lambda a: a.evaluate, '--evaluate'),
          takes='validate: rigid takes {\'iters\': T, \'tau\': tau}, got %r'),
    _Group('segment', '--segment', lambda a: a.segment, needs=(lambda a: a.evaluate and a.rigid_refine, '--evaluate --rigid-refine'),
          takes='validate: segment takes {\'eps\': e, \'dv\': v, \'min_points\': m}, got %r',
          needs_text='validate: segment needs eps finite and > 0, dv > 0 and min_points >= 1, got %r'),
    _Group('objects', '--object-refine', lambda a: a.object_refine,
          needs=(lambda a: a.evaluate and a.rigid_refine and a.segment, '--evaluate --rigid-refine --segment'),
          takes='validate: objects takes {\'iters\': T, \'tau\': tau}, got %r',
          needs_text='validate: objects needs iters in 0 .. 16 and tau finite and > 0, got %r'),
    _Group('icp', '--baseline', lambda a: a.baseline == 'icp', value='icp', needs=(lambda a: a.evaluate, '--evaluate'),
          takes='validate: icp takes {\'iters\': T, \'max_dist\': d, \'tau\': tau, \'init\': \'identity\' | \'rigid\', \'metric\': '
                '\'point\' | \'plane\'[, \'normals_k\': K, \'normals_radius\': R with \'plane\']}, got %r'),
    _Group('selfsup', '--loss', lambda a: a.loss == 'selfsup', value='selfsup',
          needs=(lambda a: not a.evaluate, 'training (--evaluate reports the supervised metrics)'),
          takes='Trainer: selfsup takes {\'k\': k, \'w_chamfer\': w, \'w_smooth\': w}, got %r',
          needs_text='Trainer: selfsup needs k in 1 .. 8 (0 with w_smooth = 0) and finite weights >= 0, got %r'),
    _Group('ground_fit', '--ground', lambda a: a.ground == 'plane', value='plane', needs=_ON_KITTI),
    _Group('voxel', '--voxel', lambda a: a.voxel is not None, needs=_ON_KITTI, as_dict=False),
    _Group('outlier_filter', '--outlier', lambda a: a.outlier is not None, needs=_ON_KITTI),
    _Group('fps', '--fps', lambda a: a.fps is not None, needs=_ON_KITTI, as_dict=False)))
_PLANE = (lambda a: a.icp_metric == 'plane', '--icp-metric plane')
_STATISTICAL = (lambda a: a.outlier == 'statistical', '--outlier statistical')

_FLAGS = [
    _Flag('--arch', default='HPLFlowNet', choices=sorted(ARCHS)),
    _Flag('--points', type=int, default=8192),
    _Flag('--pairs', type=int, default=None,
         help='pairs per epoch and rank: synthetic data default 8; real datasets default 0 = the whole '
              'split (a positive value caps the shard and is logged)'),
    _Flag('--val-pairs', type=int, default=None,
         help='validation pairs per rank while training: synthetic default 2, real datasets default 0 = all'),
    _Flag('--epochs', type=int, default=1),
    _Flag('--lr', type=float, default=1e-4),
    _Flag('--ckpt-dir', default=None),
    _Flag('--resume', default=None),
    _Flag('--evaluate', action='store_true'),
    _Flag('--batch-size', type=int, default=1,
         help='--evaluate: pairs per batched lattice build and forward (1 .. 64); consecutive pairs with equal point '
              'counts are batched (default 1: one pair at a time)'),
    _Flag('--ragged', action='store_true',
         help='--evaluate --batch-size B: batch consecutive pairs whatever their point counts (<= B pairs and <= %d '
              'points per cloud side a batch) instead of runs of equal counts' % RAGGED_POINT_BUDGET),
    _Flag('--train-batch-size', type=int, default=None,
         help='training: pairs per native step (1 .. 64, default 1); consecutive pairs with equal point counts share '
              'one batched lattice build and one step, whose gradient is the mean over them.  With W ranks the global '
              'batch is W x B pairs'),
    _Flag('--selfsup-native', action='store_true',
         help='--loss selfsup: run the step as the native training program (its loss and gradient from '
              'hpl_selfsup_loss between the forward and the backward) instead of the autograd path'),
    _Flag('--dataset', default='synthetic', choices=['synthetic', 'FlyingThings3DSubset', 'KITTI']),
    _Flag('--data-root', default=None),
    _Flag('--raw-root', default=None, metavar='DIR',
         help='--dataset KITTI|FlyingThings3DSubset: read the RAW download below DIR (disparity, optical-flow and '
              'occlusion maps) instead of a processed tree below --data-root, back-projecting every frame on the '
              'device as it is read (data.KITTIRaw / FlyingThings3DRaw, DESIGN.md §25); KITTI needs --kitti-calib'),
    _Flag('--kitti-calib', default=None, metavar='DIR',
         help='--dataset KITTI: directory of KITTI\'s calib_cam_to_cam/<frame>.txt files; the camera (P_rect_02) of each '
              'frame gives the 2D metrics EPE2D / Acc2D (without it KITTI evaluation reports the four 3D metrics)'),
    _Flag('--device-transforms', action='store_true',
         help='--dataset FlyingThings3DSubset|KITTI: run the data transforms on the device (data.DeviceAugmentation for '
              'training, data.DeviceProcessData for validation and --evaluate): the same protocol from a counter-based '
              'random stream, so a different random sample than the host transforms (DESIGN.md §15)'),
    _Check('run', lambda a: not 1 <= a.batch_size <= 64 or (a.batch_size > 1 and not a.evaluate),
          '--batch-size takes 1 .. 64 and applies to --evaluate (training takes one pair per step)'),
    _Check('run', lambda a: a.train_batch_size is not None and (a.evaluate or not 1 <= a.train_batch_size <= 64),
          '--train-batch-size takes 1 .. 64 and applies to training (--evaluate batches with --batch-size)'),
    _Check('run', lambda a: a.ragged and (not a.evaluate or a.batch_size < 2), '--ragged applies to --evaluate with --batch-size >= 2'),
    _Check('run', lambda a: a.kitti_calib is not None and (a.dataset != 'KITTI' or not os.path.isdir(a.kitti_calib)),
          '--kitti-calib takes an existing directory and applies to --dataset KITTI'),
    _Check('run', lambda a: a.raw_root is not None and (a.dataset == 'synthetic' or not os.path.isdir(a.raw_root)),
          '--raw-root takes an existing directory and applies to --dataset FlyingThings3DSubset|KITTI'),
    _Check('run', lambda a: a.raw_root is not None and a.data_root is not None, '--raw-root and --data-root exclude each other'),
    _Check('run', lambda a: a.raw_root is not None and a.dataset == 'KITTI' and a.kitti_calib is None,
          '--raw-root with --dataset KITTI needs --kitti-calib DIR (every frame\'s P_rect_02)'),
    _Check('run', lambda a: a.device_transforms and a.dataset == 'synthetic',
          '--device-transforms applies to --dataset FlyingThings3DSubset|KITTI (synthetic pairs have no transform)'),
    _Flag('--dense', action='store_true',
         help='with --evaluate on FlyingThings3DSubset / KITTI: also the metrics of the flow at every valid point of each '
              'frame, answered from the sampled forward (DenseFlow, DESIGN.md §16; not the paper\'s protocol)'),
    _Flag('--dense-fill', 'dense', choices=['knn'],
         help='with --dense: fill the part of each query that the sampled lattice does not cover by inverse-distance '
              'interpolation of the sampled flow from the --dense-k nearest sampled points (DESIGN.md §17)'),
    _Flag('--dense-k', 'dense', unset=3, takes=_within(1, 8), on=(lambda a: a.dense_fill is not None, '--dense-fill knn'), type=int,
         metavar='K',
         help='neighbours of --dense-fill knn (1 .. 8, default 3)'),
    _Flag('--rigid-refine', action='store_true',
         help='with --evaluate: behind each forward fit the rigid motion that explains most of its sampled flow (per '
              'pair, on the device) and also report the metrics of the flow whose inliers are replaced by the rigid '
              'flow, as rigid_<metric>, with rigid_inliers / rigid_angle_deg / rigid_trans (DESIGN.md §18; with --dense '
              'the sampled flow only)'),
    _Flag('--rigid-iters', 'rigid', 'iters', unset=4, takes=_within(0, 16), type=int, metavar='T',
         help='reweighted solves of --rigid-refine after the least-squares one (0 .. 16, default 4)'),
    _Flag('--rigid-tau', 'rigid', 'tau', unset=0.1, takes=_POS, type=float, metavar='TAU',
         help='--rigid-refine: inlier threshold and scale of the Geman-McClure weights in metres (> 0, default 0.1)'),
    _Flag('--segment', action='store_true',
         help='with --evaluate --rigid-refine: group the points the rigid fit leaves unexplained (residual above '
              '--rigid-tau) into moving objects on the device and report seg_objects / seg_moving / seg_noise '
              '(DESIGN.md §19)'),
    _Flag('--object-refine', action='store_true',
         help='with --evaluate --rigid-refine --segment: fit every listed object\'s own rigid motion on the device and '
              'also report the metrics of the piecewise-rigid flow -- ego-motion on the static points, each '
              'object\'s motion on its points -- as piecewise_<metric>, with piecewise_object_inliers (DESIGN.md §32)'),
    _Flag('--object-iters', 'objects', 'iters', unset=lambda built: built['rigid']['iters'], takes=_within(0, 16), type=int, metavar='T',
         help='reweighted solves of --object-refine after the least-squares one (0 .. 16, default: --rigid-iters)'),
    _Flag('--object-tau', 'objects', 'tau', unset=lambda built: built['rigid']['tau'], takes=_POS, type=float, metavar='TAU',
         help='--object-refine: inlier threshold and weight scale of the object fits in metres (> 0, default: '
              '--rigid-tau)'),
    _Flag('--segment-eps', 'segment', 'eps', unset=0.5, takes=_POS, type=float, metavar='E',
         help='--segment: link radius in metres (finite and > 0, default 0.5)'),
    _Flag('--segment-dv', 'segment', 'dv', unset=_INF, takes=(lambda v: v > 0, 'a value > 0'), type=float, metavar='V',
         help='--segment: largest flow difference of two linked points in metres (> 0, default inf: positions alone)'),
    _Flag('--segment-min-points', 'segment', 'min_points', unset=5, takes=(lambda v: v >= 1, 'a value >= 1'), type=int, metavar='M',
         help='--segment: points of the smallest object (>= 1, default 5)'),
    _Flag('--baseline', default=None, choices=['icp'],
         help='with --evaluate: behind each forward also register pc1 onto pc2 from the clouds alone by robust '
              'point-to-point ICP on the device and report the metrics of its flow as icp_<metric>, with icp_matched / '
              'icp_rmse / icp_angle_deg / icp_trans / icp_rounds (DESIGN.md §27)'),
    _Flag('--icp-iters', 'icp', 'iters', unset=30, takes=_within(0, 64), type=int, metavar='T',
         help='--baseline icp: rounds at most (0 .. 64, default 30)'),
    _Flag('--icp-max-dist', 'icp', 'max_dist', unset=1.0, takes=_POS, type=float, metavar='D',
         help='--baseline icp: a match is accepted within D metres (finite and > 0, default 1.0)'),
    _Flag('--icp-tau', 'icp', 'tau', unset=0.3, takes=_POS, type=float, metavar='TAU',
         help='--baseline icp: scale of the Geman-McClure weights in metres (finite and > 0, default 0.3)'),
    _Flag('--icp-init', 'icp', 'init', unset='identity', choices=['identity', 'rigid'],
         help='--baseline icp: start from identity (the papers\' baseline, independent of the model; default) or from '
              'the fit of --rigid-refine (network + ICP)'),
    _Check('icp', lambda a: a.icp_init == 'rigid' and not a.rigid_refine, '--icp-init rigid starts from the fit of --rigid-refine'),
    _Flag('--icp-metric', 'icp', 'metric', unset=_OMIT, choices=['point', 'plane'],
         help='--baseline icp: the residual of a round: point-to-point (default) or point-to-plane on the normals of '
              'pc2, estimated on the device behind each forward (DESIGN.md §29)'),
    _Flag('--icp-normals-k', 'icp', 'normals_k', unset=_OMIT, takes=_within(3, 32), on=_PLANE, cast=_as_is, type=int, metavar='K',
         help='--icp-metric plane: neighbours of a normal (3 .. 32, default 16)'),
    _Flag('--icp-normals-radius', 'icp', 'normals_radius', unset=_OMIT, takes=_POS, on=_PLANE, cast=_as_is, type=float, metavar='R',
         help='--icp-metric plane: radius of a normal\'s neighbourhood in metres (finite and > 0, default --icp-max-dist)'),
    _Flag('--loss', default='epe3d', choices=['epe3d', 'selfsup'],
         help='training loss: epe3d against the ground-truth flow (default), or selfsup: Chamfer distance between the '
              'warped cloud and pc2 plus the smoothness of the flow over the k nearest neighbours -- no flow label is '
              'read; it runs on the autograd path (DESIGN.md §20) unless --selfsup-native is given'),
    _Flag('--selfsup-k', 'selfsup', 'k', unset=8, takes=_within(1, 8), cast=_as_is, type=int, metavar='K',
         help='--loss selfsup: neighbours of the smoothness graph (1 .. 8, default 8)'),
    _Flag('--selfsup-chamfer-weight', 'selfsup', 'w_chamfer', unset=1.0, takes=_NONNEG, type=float, metavar='W',
         help='--loss selfsup: weight of the Chamfer term (finite and >= 0, default 1)'),
    _Flag('--selfsup-smooth-weight', 'selfsup', 'w_smooth', unset=1.0, takes=_NONNEG, type=float, metavar='W',
         help='--loss selfsup: weight of the smoothness term (finite and >= 0, default 1)'),
    _Check('selfsup', lambda a: a.selfsup_native and a.loss != 'selfsup', '--selfsup-native applies to --loss selfsup'),
    _Flag('--ground', default='threshold', choices=['threshold', 'plane'],
         help='--dataset KITTI: how the reader removes the ground: threshold -- the reference\'s rule, a correspondence '
              'with y < -1.4 in both clouds is dropped (default) --, or plane: the same pair rule on a plane fitted to '
              'each cloud on the device (DESIGN.md §21)'),
    _Flag('--voxel', type=float, default=None, metavar='V',
         help='--dataset KITTI: put every frame on a voxel grid of edge V metres (finite and > 0) on the device after '
              'the ground removal and before the sampling of --points: one correspondence per occupied cell '
              '(flownet.voxel_downsample, DESIGN.md §24); default off'),
    _Check('voxel', lambda a: a.voxel is not None and not 0 < a.voxel < _INF, '--voxel takes a finite value > 0'),
    _Flag('--voxel-mode', 'voxel', choices=['centroid', 'nearest'],
         help='--voxel: a cell becomes the mean of its points (centroid, the default) or the point nearest to it'),
    _Flag('--outlier', 'outlier_filter', 'mode', choices=['statistical', 'radius'],
         help='--dataset KITTI: remove every frame\'s stray points on the device after the ground removal and before '
              '--voxel: a correspondence is dropped when it is an outlier in either cloud (flownet.remove_outliers, '
              'DESIGN.md §33); default off'),
    _Flag('--outlier-k', 'outlier_filter', 'k', unset=16, takes=_within(1, 32), on=_STATISTICAL, type=int, metavar='K',
         help='--outlier statistical: the nearest neighbours of the mean distance, 1 .. 32 (default 16)'),
    _Flag('--outlier-radius', 'outlier_filter', 'radius', unset=1.0, takes=_POS, type=float, metavar='R',
         help='--outlier: the search radius in metres, finite and > 0 (default 1.0)'),
    _Flag('--outlier-std-ratio', 'outlier_filter', 'std_ratio', unset=2.0, takes=_NONNEG, on=_STATISTICAL, type=float, metavar='S',
         help='--outlier statistical: kept up to mu + S sigma of the mean distances, finite and >= 0 (default 2.0)'),
    _Flag('--outlier-min-neighbors', 'outlier_filter', 'min_neighbors', unset=2, takes=(lambda v: 1 <= v <= 2 ** 31 - 1, 'an int >= 1'),
         on=(lambda a: a.outlier == 'radius', '--outlier radius'), type=int, metavar='M',
         help='--outlier radius: kept with at least M neighbours within the radius, >= 1 (default 2)'),
    _Flag('--fps', type=int, default=None, metavar='K',
         help='--dataset KITTI: sample every frame to K correspondences (an int >= 1) by farthest point sampling on the '
              'device, after the ground removal and --voxel and before the sampling of --points '
              '(flownet.fps_sample, DESIGN.md §30); default off'),
    _Check('fps', lambda a: a.fps is not None and a.fps < 1, '--fps takes an int >= 1'),
    _Flag('--ground-tau', 'ground_fit', 'tau', unset=0.1, takes=_POS, type=float, metavar='TAU',
         help='--ground plane: inlier distance of the fit in metres (finite and > 0, default 0.1)'),
    _Flag('--ground-cut', 'ground_fit', 'cut', unset=0.3, takes=_NONNEG, type=float, metavar='C',
         help='--ground plane: a point at most C metres above the plane is ground (finite and >= 0, default 0.3)'),
    _Flag('--ground-hyps', 'ground_fit', 'hyps', unset=256, takes=_within(1, 1024), type=int, metavar='H',
         help='--ground plane: three-point hypotheses per cloud (1 .. 1024, default 256)'),
    _Flag('--ground-tilt', 'ground_fit', 'max_tilt_deg', unset=20.0, takes=(lambda v: 0 <= v < 90, '0 <= DEG < 90'), type=float,
         metavar='DEG',
         help='--ground plane: largest tilt of the plane\'s normal from --ground-up in degrees (0 <= DEG < 90, default 20)'),
    _Flag('--ground-up', 'ground_fit', 'up', unset=(0.0, 1.0, 0.0),
         takes=(lambda v: all(abs(x) < _INF for x in v) and any(v), 'three finite numbers, not all zero,'), cast=tuple, type=float, nargs=3,
         metavar=('X', 'Y', 'Z'),
         help='--ground plane: the up direction (finite, not zero; default 0 1 0, KITTI\'s camera frame as the reader stores it)'),
    _Flag('--write-kitti', default=None, metavar='DIR',
         help='--evaluate --dataset KITTI: write every evaluated frame\'s flow -- the dense one with --dense, else the '
              'sampled one -- as KITTI\'s three 16-bit PNGs DIR/disp_0|disp_1|flow/NNNNNN_10.png (DESIGN.md §34); the '
              'camera is the frame\'s of --kitti-calib, the size the raw frame\'s with --raw-root, else --write-size'),
    _Flag('--write-footprint', 'write', takes=_within(0, 4), type=int, metavar='R',
         help='--write-kitti: every point covers the (2 R + 1)^2 pixels around its own (0 .. 4, default 0)'),
    _Flag('--write-size', 'write', takes=(lambda v: min(v) >= 1, 'two sizes >= 1'),
         on=(lambda a: a.write_kitti is not None and a.raw_root is None, '--write-kitti without --raw-root'), type=int, nargs=2,
         metavar=('H', 'W'),
         help='--write-kitti without --raw-root: the size of the maps'),
    _Check('write', lambda a: a.write_kitti is not None and a.raw_root is None and a.write_size is None,
          '--write-kitti without --raw-root needs --write-size H W'),
    _Flag('--init', default='hash', choices=['hash', 'xavier', 'normal', 'kaiming', 'orthogonal']),
]


def parse_args(argv=None):
    """The command line of main(), checked (argparse exits with a message on a bad combination): the flags of _FLAGS, then
    the _GROUPS in their order -- the switch's own requirement, then each option and each hand-written check in turn --, each
    group that becomes a dict left as a.<group>."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for r in _FLAGS:
        if isinstance(r, _Flag):
            ap.add_argument(r.flag, **r.kw)
    a = ap.parse_args(argv)
    built = {}
    for g in _GROUPS.values():
        on = g.on(a)
        if on and not g.needs[0](a):
            ap.error('%s applies to %s' % (g.flag, g.needs[1]))
        for r in g.rows():
            if isinstance(r, _Check):
                if r.bad(a):
                    ap.error(r.text)
                continue
            v = getattr(a, r.dest)
            r_on, words = (on, g.applies) if r.on is None else (r.on[0](a), r.on[1])
            if v is not None and not (r_on and r.ok(v)):
                ap.error('%s takes %s and applies to %s' % (r.flag, r.takes, words) if r.takes else '%s applies to %s' % (r.flag, words))
            if not g.as_dict and v is None:
                setattr(a, r.dest, r.unset)
        if g.as_dict:       # (an option whose own switch is off is no key of the dict: --outlier-k under --outlier radius)
            given = {r.key: getattr(a, r.dest) for r in g.options() if getattr(a, r.dest) is not None}
            built[g.name] = g.filled(given, built, [r for r in g.options() if r.on is None or r.on[0](a)]) if on else None
            setattr(a, g.name, built[g.name])
    if a.outlier_filter:                # (the run's report lists the filter's values in this order)
        a.outlier_filter = {k: a.outlier_filter[k] for k in ('mode', 'radius', 'k', 'std_ratio', 'min_neighbors') if k in a.outlier_filter}
    a.train_batch_size = a.train_batch_size or 1
    if a.pairs is None:
        a.pairs = 8 if a.dataset == 'synthetic' else 0
    if a.val_pairs is None:
        a.val_pairs = 2 if a.dataset == 'synthetic' else 0
    return a


def main(argv=None):
    a = parse_args(argv)
    rank, world, local_rank = parallel.init_distributed()
    dev = torch.device('cuda', local_rank)
    torch.cuda.set_device(dev)
    tr = Trainer(a.arch, dev, lr=a.lr, distributed=world > 1, rank=rank, init=a.init, loss=a.loss, selfsup=a.selfsup,
                 native_step=True if a.selfsup_native else None)
    if a.resume:
        tr.resume(a.resume, load_optimizer=not a.evaluate)
    if a.dataset != 'synthetic':
        return _real_data(a, tr, dev, rank, world)
    if a.evaluate:
        res = tr.validate(SyntheticPairs(a.pairs, a.points, dev, first_seed=1000 + rank * a.pairs), a.batch_size, a.ragged,
                          rigid=a.rigid, segment=a.segment, icp=a.icp, objects=a.objects)
        if rank == 0:
            print(' '.join('%s %.4f' % kv for kv in res.items()))
        return res
    train = SyntheticPairs(a.pairs, a.points, dev, first_seed=rank * a.pairs)
    val = SyntheticPairs(a.val_pairs, a.points, dev, first_seed=1000)
    return tr.fit(train, val, a.epochs, a.ckpt_dir, log=print if rank == 0 else (lambda *_: None), batch_size=a.train_batch_size)


class _Shard(object):
    """Every world-th sample of a reader, starting at rank (independent pairs per GPU).

    equal=True (training): every rank gets ceil(len / world) samples, the short ranks wrapping around to the
    start of the reader (what torch's DistributedSampler does) -- train_epoch issues one gradient all-reduce per
    step, so ranks with different step counts would leave each other blocked in a collective.  equal=False
    (validation: no per-step collective, sums are reduced at the end): the plain strided split, no duplicates."""

    def __init__(self, reader, rank, world, limit=0, equal=False):
        self.reader = reader
        n = len(reader)
        if equal and n > 0:
            per = (n + world - 1) // world
            self.ids = [(rank + i * world) % n for i in range(per)]
        else:
            self.ids = list(range(rank, n, world))
        if limit > 0:
            self.ids = self.ids[:limit]
        self.has_cameras = bool(getattr(reader, 'has_cameras', False))     # the reader's answer, whatever this shard holds

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        return self.reader[self.ids[i]]

    def point_counts(self, i):
        return point_counts(self.reader, self.ids[i])


class _Both(object):
    """A reader's transform that also runs `full` on the same loaded frame (DenseFrames)."""

    def __init__(self, sampled, full, keep):
        self.sampled, self.full, self.keep = sampled, full, keep
        self.on_device = getattr(sampled, 'on_device', False)
        self.sampler = getattr(sampled, 'sampler', sampled)      # (what _PairFolder.point_counts reads)

    def __call__(self, data):
        self.keep[0] = self.full(data)
        return self.sampled(data)


class KittiWriter(object):
    """validate(write=...): the evaluated flow of every frame as KITTI's three 16-bit PNGs below `directory` --
    disp_0/NNNNNN_10.png, disp_1/NNNNNN_10.png, flow/NNNNNN_10.png -- by one flownet.flow_to_kitti_maps call per forward
    (DESIGN.md §34).  The camera is the sample's, the one the 2D metrics use; the size is the sample's raw frame's, else `size`.
    Each call reads its maps back: it is off unless asked for."""

    def __init__(self, directory, footprint=0, size=None, baseline=0.54):
        self.directory, self.footprint, self.size, self.baseline = directory, int(footprint), size, baseline
        self.written = []
        for sub in ('disp_0', 'disp_1', 'flow'):
            os.makedirs(os.path.join(directory, sub), exist_ok=True)

    def __call__(self, samples, pc1s, flows):
        from .flownet import flow_to_kitti_maps
        Ps, sizes = [], []
        for s_ in samples:
            cam, size, frame = getattr(s_, 'camera', None), getattr(s_, 'size', None) or self.size, getattr(s_, 'frame', None)
            if cam is None or size is None or frame is None:
                raise HplError('KittiWriter: a sample needs its camera, its frame\'s name and a size (frame %r, camera %r, size %r)' % (
                    frame, cam, size))
            f, cx, cy, kx, ky, kz = cam          # (read_kitti_camera: f = -P00; the float32 values come back exactly)
            Ps.append([-f, 0.0, cx, kx, 0.0, -f, cy, ky, 0.0, 0.0, 1.0, kz])
            sizes.append(tuple(size))
        maps = flow_to_kitti_maps(list(pc1s), list(flows), Ps, sizes, baseline=self.baseline, footprint=self.footprint)
        for s_, planes in zip(samples, maps):
            for sub, x in zip(('disp_0', 'disp_1', 'flow'), planes):
                data_mod.write_png(os.path.join(self.directory, sub, s_.frame + '_10.png'), x)
            self.written.append(s_.frame)


class DenseFrames(object):
    """A reader whose samples also carry `.dense` = (pc1, pc2, sf) of every valid point of their frame, (3, M) float32 device
    tensors in index order with sf = pc2 - pc1: `full` is a ProcessData / DeviceProcessData with num_points = 0 and
    allow_less_points, applied to the same loaded frame as the reader's own transform (which gives the sampled pair)."""

    def __init__(self, reader, full):
        self.reader = reader
        self._last = [None]
        reader.transform = _Both(reader.transform, full, self._last)
        self.has_cameras = bool(getattr(reader, 'has_cameras', False))
        self.device = reader.device

    def __len__(self):
        return len(self.reader)

    def check_counts(self):
        return self.reader.check_counts()

    def point_counts(self, i):
        return point_counts(self.reader, i)

    def __getitem__(self, i):
        s_ = self.reader[i]
        out = self._last[0]                   # the full transform of the frame the sample came from (the last one loaded)
        if out is None or out[0] is None:
            raise HplError('DenseFrames: the frame of sample %d has no valid point' % i)
        if not all(torch.is_tensor(t) for t in out):
            out = tuple(torch.from_numpy(np.ascontiguousarray(t[:, :3].T, dtype=np.float32)).to(self.device) for t in out)
        s_.dense = tuple(out)
        return s_


def _real_data(a, tr, dev, rank, world):
    log = print if rank == 0 else (lambda *_: None)
    # the published evaluation protocol (configs/test_ours_KITTI.yaml:9,36-37, test_ours_FlyingThings3D.yaml:9,35-36):
    # NO_CORR True (the two clouds are sampled independently) and allow_less_points True -- a frame with fewer than
    # num_points valid points is evaluated on what it has, not replaced by another frame; training
    # (configs/train_ours.yaml:6) rejects such frames
    if a.device_transforms:             # the same protocol on the device, from its own random stream
        process = lambda less: data_mod.DeviceProcessData(DATA_PROCESS, a.points, less, seed=0, device=dev)     # noqa: E731
        augment = lambda: data_mod.DeviceAugmentation(AUG_TOGETHER, AUG_PC2, DATA_PROCESS, a.points, False,     # noqa: E731
                                                      seed=1 + rank, device=dev)
    else:
        process = lambda less: data_mod.ProcessData(DATA_PROCESS, a.points, less, seed=0)                       # noqa: E731
        augment = lambda: data_mod.Augmentation(AUG_TOGETHER, AUG_PC2, DATA_PROCESS, a.points, False, seed=1 + rank)  # noqa: E731
    if a.dataset == 'KITTI':                        # evaluation only in the reference
        kitti = data_mod.KITTIRaw if a.raw_root is not None else data_mod.KITTI
        val = kitti(process(True), a.raw_root if a.raw_root is not None else a.data_root, device=dev, calib_dir=a.kitti_calib,
                    remove_ground='plane' if a.ground_fit else True, ground=a.ground_fit, voxel=a.voxel,
                    voxel_mode=a.voxel_mode or 'centroid', fps=a.fps, outlier=a.outlier_filter)
        train = None
        if a.kitti_calib is None:
            log('note: 2D metrics (EPE2D, Acc2D) need the frames\' cameras: pass --kitti-calib DIR (calib_cam_to_cam)')
    elif a.raw_root is not None:
        val = data_mod.FlyingThings3DRaw(False, process(bool(a.evaluate)), a.raw_root, device=dev)
        train = None if a.evaluate else data_mod.FlyingThings3DRaw(True, augment(), a.raw_root, device=dev)
    else:
        val = data_mod.FlyingThings3DSubset(False, process(bool(a.evaluate)), a.data_root, device=dev)
        train = None if a.evaluate else data_mod.FlyingThings3DSubset(True, augment(), a.data_root, device=dev)
    for ds in (train, val):
        msg = ds.check_counts() if ds is not None else None
        if msg:
            log('warning: ' + msg)
    cap = a.val_pairs if train is not None else a.pairs
    if cap > 0:
        log('note: evaluating the first %d samples of each rank\'s shard only (--%s)' % (cap, 'val-pairs' if train is not None else 'pairs'))
    if train is not None and a.pairs > 0:
        log('note: training on the first %d samples of each rank\'s shard only (--pairs)' % a.pairs)
    if a.dense:       # every valid point of each frame, in index order, beside the sampled pair (loaded once)
        full = data_mod.DeviceProcessData(DATA_PROCESS, 0, True, seed=0, device=dev) if a.device_transforms else \
            data_mod.ProcessData(DATA_PROCESS, 0, True, seed=0)
        val = DenseFrames(val, full)
    val = _Shard(val, rank, world, cap)
    if train is None:
        write = KittiWriter(a.write_kitti, a.write_footprint or 0, a.write_size) if a.write_kitti is not None else None
        res = tr.validate(val, a.batch_size, a.ragged, dense=a.dense, dense_fill=a.dense_fill, dense_k=a.dense_k, rigid=a.rigid,
                          segment=a.segment, icp=a.icp, objects=a.objects, write=write)
        if a.outlier_filter:                # the run's report carries the filter it ran with (the mode as OUTLIER_MODES' number)
            res['outlier_mode'] = float(ops.OUTLIER_MODES[a.outlier_filter['mode']])
            res.update(('outlier_' + k, float(v)) for k, v in a.outlier_filter.items() if k != 'mode')
        log(' '.join('%s %.4f' % kv for kv in res.items()))
        return res
    return tr.fit(_Shard(train, rank, world, a.pairs, equal=True), val, a.epochs, a.ckpt_dir, log=log, shuffle=True,
                  batch_size=a.train_batch_size)


if __name__ == '__main__':
    main()
