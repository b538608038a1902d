"""Tensor-level wrappers and autograd glue over the C ABI (include/hpl_bcl.h).

Everything here is host-side plumbing: shapes are checked, outputs are allocated as
torch tensors, and the HIP library does the work on the current stream.  Activations
are channel-last 2-D float32 tensors `[rows, channels]` with unit channel stride (the
row stride may exceed the channel count: column slices of wider buffers are fine).
"""
import collections
import ctypes
import math
import operator
import os
import struct

import torch

from . import _lib
from ._lib import GConvDesc, RelayoutJob, check, ptr, stream

ACT_NONE, ACT_LEAKY = 0, 1
LEAKY_RATE = 0.1   # reference: models/module_utils.py:6


def _cl(x, what='activation'):
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise _lib.HplError('%s must be a channel-last 2-D float32 device tensor with unit channel stride, '
                            'got shape %s strides %s dtype %s device %s'
                            % (what, tuple(x.shape), x.stride(), x.dtype, x.device))
    return x


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else max(x.shape[1], x.stride(0))


# --------------------------------------------------------------------------- tables
def narrow(t):
    """int64 device table (reference wire format) -> contiguous int32."""
    if t.dtype == torch.int32:
        return t.contiguous()
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    check(_lib.load().hpl_index_narrow(ptr(t), ptr(out), t.numel(), stream()), 'hpl_index_narrow')
    return out


def corr2_permute(t):
    """pc2_corr_indices [F, K, H] (int64 or int32) -> int32 [K, F*H]."""
    t = t.contiguous()
    F, K, H = t.shape
    out = torch.empty((K, F * H), dtype=torch.int32, device=t.device)
    fn = _lib.load().hpl_corr2_permute if t.dtype == torch.int64 else _lib.load().hpl_corr2_permute32
    check(fn(ptr(t), ptr(out), F, K, H, stream()), 'hpl_corr2_permute')
    return out


class CloudTables(object):
    """Device-resident tables of one cloud at one lattice level.

    bary [4, N] f32, off [4, N] i32 (vertex of each (remainder, point)), H vertices,
    CSR of the splat (csr_ptr/csr_pt/csr_w) and the density normaliser `norm` [H]."""

    def __init__(self, bary, off, H, blur=None):
        self.bary = bary.contiguous().float()
        self.off = narrow(off)
        self.N = int(self.bary.shape[1])
        self.H = int(H)
        self.blur = narrow(blur) if blur is not None else None
        self._csr = None
        self._sym = {}

    def csr(self):
        if self._csr is None and getattr(self, '_csr_src', None) is not None:
            pair_csr, n0, h0 = self._csr_src           # (the pair's ARRAYS, not the pair: no reference cycle cloud <-> pair)
            p_ptr, p_pt, p_w, p_norm = pair_csr
            self._csr = (p_ptr[h0:] - 4 * n0, p_pt[4 * n0:] - n0, p_w[4 * n0:], p_norm[h0:])
        if self._csr is None:
            dev = self.bary.device
            csr_ptr = torch.empty(self.H + 1, dtype=torch.int32, device=dev)
            csr_pt = torch.empty(4 * self.N, dtype=torch.int32, device=dev)
            csr_w = torch.empty(4 * self.N, dtype=torch.float32, device=dev)
            norm = torch.empty(self.H, dtype=torch.float32, device=dev)
            scratch = torch.empty(self.H + 1 + 4 * self.N + 1026, dtype=torch.int32, device=dev)
            check(_lib.load().hpl_csr_build(ptr(self.off), ptr(self.bary), 4 * self.N, self.N, self.H, ptr(csr_ptr),
                                            ptr(csr_pt), ptr(csr_w), ptr(norm), ptr(scratch), stream()),
                  'hpl_csr_build')
            self._csr = (csr_ptr, csr_pt, csr_w, norm)
        return self._csr

    def slice_back(self, g, use_norm):
        """Backward of the splat: g [H, C] -> [N, C] = sum_r bary[r, n] * norm[v] * g[v = off[r, n]]."""
        return slice_raw(g, self.bary, self.off, self.N, vscale=self.csr()[3] if use_norm else None)


class PairTables(object):
    """Both clouds of one lattice level treated as one cloud: points [0,N0) + [N0,N0+N1), vertices
    [0,H0) + [H0,H0+H1).  Only what the splat needs (the pair CSR); a vertex belongs to one cloud,
    so every segment equals the per-cloud CSR and the result rows equal the per-cloud results."""

    def __init__(self, c0, c1):
        self.c0, self.c1 = c0, c1
        self.N = c0.N + c1.N
        self.H = c0.H + c1.H
        self._csr = None

    def csr(self):
        if self._csr is None:
            c0, c1 = self.c0, self.c1
            dev = c0.bary.device
            csr_ptr = torch.empty(self.H + 1, dtype=torch.int32, device=dev)
            csr_pt = torch.empty(4 * self.N, dtype=torch.int32, device=dev)
            csr_w = torch.empty(4 * self.N, dtype=torch.float32, device=dev)
            norm = torch.empty(self.H, dtype=torch.float32, device=dev)
            scratch = torch.empty(self.H + 1 + 4 * self.N + 1026, dtype=torch.int32, device=dev)
            check(_lib.load().hpl_csr_build_pair(ptr(c0.off), ptr(c0.bary), c0.N, c0.H, ptr(c1.off), ptr(c1.bary),
                                                 c1.N, c1.H, ptr(csr_ptr), ptr(csr_pt), ptr(csr_w), ptr(norm),
                                                 ptr(scratch), stream()), 'hpl_csr_build_pair')
            self._csr = (csr_ptr, csr_pt, csr_w, norm)
            # the pair CSR is the two per-cloud CSRs laid end to end: cloud 1's is a set of views
            # (no launch), cloud 2's needs its offsets removed (built on first use)
            if c0._csr is None:
                c0._csr = (csr_ptr[:c0.H + 1], csr_pt[:4 * c0.N], csr_w[:4 * c0.N], norm[:c0.H])
            if c1._csr is None:
                c1._csr_src = (self._csr, c0.N, c0.H)
        return self._csr

    def slice_back(self, g, use_norm):
        """Backward of the pair splat: each cloud's rows from its own vertices (one launch per cloud
        into the two halves of one [N0+N1, C] matrix)."""
        c0, c1 = self.c0, self.c1
        norm = self.csr()[3] if use_norm else None
        out = torch.empty((self.N, g.shape[1]), dtype=torch.float32, device=g.device)
        slice_raw(g[:c0.H], c0.bary, c0.off, c0.N, vscale=norm[:c0.H] if use_norm else None, out=out[:c0.N])
        slice_raw(g[c0.H:], c1.bary, c1.off, c1.N, vscale=norm[c0.H:] if use_norm else None, out=out[c0.N:])
        return out


def tap_order(nbr):
    """int32 [F<=15, M] neighbour table -> int32 [M] permutation sorting the rows by tap-presence mask
    (deterministic: ties by row id)."""
    F, M = nbr.shape
    L = _lib.load()
    perm = torch.empty(M, dtype=torch.int32, device=nbr.device)
    scratch = torch.empty((int(L.hpl_tap_order_scratch_ints(M)) + 1) // 2, dtype=torch.int64, device=nbr.device)
    check(L.hpl_tap_order(ptr(nbr), nbr.stride(0), F, M, ptr(perm), ptr(scratch), stream()), 'hpl_tap_order')
    return perm


TILE_BM = 64        # tile height of the gather-GEMM classes that take a row order (csrc/gconv.hip: 64x128, 64x64)
#: HPL_MATH=f32 keeps every gather-GEMM on the fp32 MFMA; default (f16x2): the wide launches run on the fp16 MFMA with every
#: fp32 operand carried as a scaled fp16 pair, HPL_MATH=bf16x3: on the bf16 MFMA with exact bf16 triples (csrc/gconv3.hip: both
#: fp32-class accuracy; tiles 128 rows high)
MATH = os.environ.get('HPL_MATH', 'f16x2')
SPLIT3 = MATH != 'f32'
SPLIT_PLANES = 3 if MATH == 'bf16x3' else 2
GROUP_TILE_BM = 128 if SPLIT3 else 64
#: weight images narrower than this stay fp32-only (the split kernel takes launches with N >= 256, C >= 32)
SPLIT3_MIN_N, SPLIT3_MIN_C = 256, 32


def split3_maybe(M, C, F, N):
    """csrc/gconv_common.h split3_maybe: can this launch run on the split-operand kernel at all?  (Launches that cannot
    skip the reduction of their operand's magnitude and run on the fp32 MFMA.)"""
    if not (C >= SPLIT3_MIN_C and N >= SPLIT3_MIN_N and M >= 1024 and F <= 15):
        return False
    tiles = -(-M // 128) * -(-N // 256)
    if tiles >= 128:
        return True
    if F == 1:
        return M >= 8192
    if M >= 16384:
        return True
    return N % 256 == 0 and min(256 // tiles, -(-F * C // 32) // 16) >= 2


def tile_index(nbr, perm, BM=TILE_BM):
    """int32 [F<=15, M] table + row order (or None) -> (tile_idx int32 [tiles, F, BM], tile_mask int32 [tiles, 8]):
    the gather indices and tap masks of every BM-row tile, precomputed once per lattice (hpl_tile_index)."""
    F, M = nbr.shape
    tiles = (M + BM - 1) // BM
    idx = torch.empty((tiles, F, BM), dtype=torch.int32, device=nbr.device)
    mask = torch.empty((tiles, 8), dtype=torch.int32, device=nbr.device)
    check(_lib.load().hpl_tile_index(ptr(nbr), nbr.stride(0), F, M, ptr(perm), BM, ptr(idx), ptr(mask), stream()),
          'hpl_tile_index')
    return idx, mask


def tap_lists(nbr):
    """int32 [F, M] table -> (list_m, list_row int32 [F*M], tap_ptr int32 [F+1]): the present vertices of
    every tap and their source rows."""
    F, M = nbr.shape
    lm = torch.empty(F * M, dtype=torch.int32, device=nbr.device)
    lr = torch.empty(F * M, dtype=torch.int32, device=nbr.device)
    tp = torch.empty(F + 1, dtype=torch.int32, device=nbr.device)
    scratch = torch.empty(2 * F * ((M + 1023) // 1024) + 1100, dtype=torch.int32, device=nbr.device)
    check(_lib.load().hpl_tap_lists(ptr(nbr), nbr.stride(0), F, M, ptr(lm), ptr(lr), ptr(tp), ptr(scratch),
                                    stream()), 'hpl_tap_lists')
    return lm, lr, tp


def table_symmetry_flag(nbr):
    """Launch the symmetry check of an int32 [F, M] table; -> int32 device tensor [1] (1 = symmetric).
    No host sync: read several flags back together (DeviceLattice.resolve_symmetry)."""
    F, M = nbr.shape
    flag = torch.ones(1, dtype=torch.int32, device=nbr.device)
    check(_lib.load().hpl_table_symmetric(ptr(nbr), nbr.stride(0), F, M, ptr(flag), stream()), 'hpl_table_symmetric')
    return flag


def table_is_symmetric(nbr):
    """nbr[f, h] = g  =>  nbr[(F - f) % F, g] = h  (SURVEY.md fact 7).  One host sync."""
    F, H = nbr.shape
    if F != 15:
        return False
    if nbr.is_cuda and nbr.dtype == torch.int32 and nbr.stride(1) == 1:
        return bool(table_symmetry_flag(nbr).item())
    f = torch.arange(1, F, device=nbr.device)
    g = nbr[f].long()
    valid = g >= 0
    back = nbr[(F - f)].long().gather(1, g.clamp(min=0))
    hh = torch.arange(H, device=nbr.device)[None, :].expand_as(g)
    ok = ((back == hh) | ~valid).all() & (nbr[0].long() == torch.arange(H, device=nbr.device)).all()
    return bool(ok.item())


# --------------------------------------------------------------------------- raw ops
def splat_raw(feat, csr, H, use_norm=True, out=None):
    feat = _cl(feat)
    csr_ptr, csr_pt, csr_w, norm = csr
    C = feat.shape[1]
    if out is None:
        out = torch.empty((H, C), dtype=torch.float32, device=feat.device)
    _cl(out, 'out')
    check(_lib.load().hpl_splat(ptr(feat), _ld(feat), C, ptr(csr_ptr), ptr(csr_pt), ptr(csr_w),
                                ptr(norm) if use_norm else None, H, ptr(out), _ld(out), stream()), 'hpl_splat')
    return out


def slice_raw(Y, bary, off, N, vscale=None, bias=None, out=None):
    Y = _cl(Y)
    C = Y.shape[1]
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=Y.device)
    _cl(out, 'out')
    check(_lib.load().hpl_slice(ptr(Y), _ld(Y), C, ptr(bary), ptr(off), N, ptr(vscale), ptr(bias), ptr(out),
                                _ld(out), stream()), 'hpl_slice')
    return out


def gather_sum_raw(Z, nbr, M, K, N, col_step, bias=None, res=None, res_mod=0, act=ACT_NONE, slope=LEAKY_RATE, out=None):
    """Y[m, n] = act(bias[n] + res[m % res_mod, n] + sum_k Z[nbr[k, m], k*col_step + n])  (hpl_gather_sum)."""
    Z = _cl(Z)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=Z.device)
    check(_lib.load().hpl_gather_sum(ptr(Z), _ld(Z), ptr(nbr), nbr.stride(0), M, K, N, col_step, ptr(bias), ptr(res),
                                     _ld(res) if res is not None else 0, res_mod, act, slope, ptr(out), _ld(out), stream()),
          'hpl_gather_sum')
    return out


def table_invert(tbl, H0, F, H1):
    """int32 [K, F*H0] table with values in [0, H1) -> int32 [F, K*H1] inverse (hpl_table_invert)."""
    K = tbl.shape[0]
    inv = torch.empty((F, K * H1), dtype=torch.int32, device=tbl.device)
    check(_lib.load().hpl_table_invert(ptr(tbl), tbl.stride(0), K, H0, F, H1, ptr(inv), stream()), 'hpl_table_invert')
    return inv


def ragged_stage(pc1s, pc2s, sfs=None):
    """A ragged batch's per-pair clouds -> its pair-major matrices in ONE launch (hpl_ragged_stage): pc1s[b], sfs[b] (3, N1_b),
    pc2s[b] (3, N2_b) float32 device tensors (row slices of a padded (B, 3, Nmax) tensor are read in place) -> (3, sum N1_b),
    (3, sum N2_b) and, with sfs, (3, sum N1_b) tensors on the current stream."""
    B = len(pc1s)
    sides = [pc1s, pc2s] + ([sfs] if sfs is not None else [])
    keep, descs, outs = [], [], []
    for ts in sides:
        # rows of unit stride and a row stride >= the count; anything else is copied first
        ts = [t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous() for t in ts]
        keep.append(ts)
        descs.append(((ctypes.c_void_p * B)(*[ptr(t) for t in ts]), (ctypes.c_int64 * B)(*[int(t.shape[1]) for t in ts]),
                      (ctypes.c_int64 * B)(*[int(t.stride(0)) for t in ts])))
        outs.append(torch.empty((3, sum(int(t.shape[1]) for t in ts)), dtype=torch.float32, device=ts[0].device))
    d1, d2 = descs[0], descs[1]
    d3 = descs[2] if sfs is not None else (None, None, None)
    check(_lib.load().hpl_ragged_stage(B, d1[0], d1[1], d1[2], d2[0], d2[1], d2[2], d3[0], d3[2], ptr(outs[0]), ptr(outs[1]),
                                       ptr(outs[2]) if sfs is not None else None, stream()), 'hpl_ragged_stage')
    return tuple(outs)


# --------------------------------------------------------------------------- evaluation metrics
#: the keys of the 3D metrics (evaluation_utils.py:4-19) and of the 2D pair that needs a camera (:22-36)
METRICS_3D = ('EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers')
METRICS_2D = ('EPE2D', 'Acc2D')


class MetricsStage(object):
    """Room for `count` hpl_metrics_pair descriptors: pinned host memory (the source of the asynchronous copy) and its device
    twin.  Row r belongs to one launch; a row must not be refilled before the copy that read it has run on its stream."""

    SIZE = ctypes.sizeof(_lib.MetricsPair)

    def __init__(self, count, device):
        self.count = count
        self.host = torch.empty(count * self.SIZE, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.empty(count * self.SIZE, dtype=torch.uint8, device=device)


_metrics_inflight = collections.deque()      # (event, stage) of calls that brought no stage: alive until their copy has run


def _metrics_desc(pred, gt, pc1, camera):
    n = int(gt.shape[-1])
    for t, what in ((pred, 'pred'), (gt, 'gt'), (pc1, 'pc1')):
        if t.dim() != 2 or t.shape[0] != 3 or int(t.shape[1]) != n or t.dtype != torch.float32 or not t.is_cuda:
            raise _lib.HplError('flow_metrics_pairs: %s must be a (3, %d) float32 device view, got shape %s dtype %s device %s'
                                % (what, n, tuple(t.shape), t.dtype, t.device))
    d = _lib.MetricsPair(ptr(pred), ptr(gt), ptr(pc1), n, pred.stride(0), pred.stride(1), gt.stride(0), gt.stride(1),
                         pc1.stride(0), pc1.stride(1))
    if camera is not None:
        if len(camera) != 6:
            raise _lib.HplError('flow_metrics_pairs: a camera is (f, cx, cy, constx, consty, constz), got %r' % (camera,))
        d.camera[:] = [float(c) for c in camera]        # (ctypes rounds each to float32)
        d.has_camera = 1
    return d


def flow_metrics_pairs(preds, gts, pc1s, cameras, out, row=0, stage=None):
    """The per-pair metric sums of B <= 64 pairs in ONE launch (hpl_flow_metrics) on the current stream.  preds[b], gts[b],
    pc1s[b]: (3, N_b) float32 device views of any strides (the forward's point-major flow as it comes); cameras[b]: a
    (f, cx, cy, constx, consty, constz) tuple or None (no 2D metrics).  out: (R, 8) float64 device tensor; pair b's sums go to
    row `row + b` (flow_metrics_fold turns a row into metric values; slots 5 and 6 stay untouched without a camera).  stage: a
    MetricsStage whose rows row .. row + B - 1 hold the descriptors; without one the call brings its own."""
    B = len(preds)
    if not (len(gts) == len(pc1s) == len(cameras) == B):
        raise _lib.HplError('flow_metrics_pairs: %d preds, %d gts, %d clouds, %d cameras' % (B, len(gts), len(pc1s), len(cameras)))
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != 8 or not out.is_contiguous() or not out.is_cuda \
            or not 0 <= row or row + B > out.shape[0]:
        raise _lib.HplError('flow_metrics_pairs: out must be a contiguous (>= %d, 8) float64 device tensor, got %s %s'
                            % (row + B, tuple(out.shape), out.dtype))
    descs = (_lib.MetricsPair * max(B, 1))(*[_metrics_desc(p, g, c, cam) for p, g, c, cam in zip(preds, gts, pc1s, cameras)])
    own = stage is None
    if own:
        while _metrics_inflight and _metrics_inflight[0][0].query():
            _metrics_inflight.popleft()
        stage, srow = MetricsStage(max(B, 1), out.device), 0
    else:
        srow = row
        if srow + B > stage.count:
            raise _lib.HplError('flow_metrics_pairs: rows %d .. %d outside a stage of %d' % (srow, srow + B - 1, stage.count))
    off = srow * MetricsStage.SIZE
    ctypes.memmove(stage.host.data_ptr() + off, descs, B * MetricsStage.SIZE)
    check(_lib.load().hpl_flow_metrics(stage.host.data_ptr() + off, B, stage.dev.data_ptr() + off, out[row].data_ptr() if B else
                                       out.data_ptr(), stream()), 'hpl_flow_metrics')
    if own:
        ev = torch.cuda.Event()
        ev.record()
        _metrics_inflight.append((ev, stage))
    return out


def flow_metrics_fold(words, camera=True):
    """One pair's 8 words of hpl_flow_metrics (a host sequence) -> {metric: value}: each sum over the pair's point count, the
    2D pair only when the pair had a camera."""
    n = float(words[0])
    r = dict(zip(METRICS_3D, (float(words[k]) / n for k in (1, 2, 3, 4))))
    if camera:
        r.update(zip(METRICS_2D, (float(words[5]) / n, float(words[6]) / n)))
    return r


# --------------------------------------------------------------------------- nearest neighbours
def _soa3(x, what, op='knn_interpolate'):
    """A (3, n) float32 device cloud with unit stride along its points (rows may be views of a wider buffer)."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise _lib.HplError('%s: %s must be a (3, n) float32 device tensor, got %s' % (
            op, what, (tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x)))
    if x.requires_grad:
        raise _lib.HplError('%s has no autograd: %s requires grad' % (op, what))
    n = x.shape[1]
    if x.stride(0) < max(n, 1) or (n > 1 and x.stride(1) != 1):
        x = x.contiguous()           # (after which a row starts max(n, 1) elements behind the previous one)
    return x, _soa_ld(x, n)


def _int_in(who, name, v, lo, hi):
    """v when it is an int (no bool) in lo .. hi."""
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise _lib.HplError('%s: %s = %r (an int in %d .. %d)' % (who, name, v, lo, hi))
    return v


def _prefix(prefix, n, who, what='the prefix'):
    """The host list of B + 1 <= 65 non-decreasing ints from 0 to n (None: one pair)."""
    pp = [0, n] if prefix is None else [int(x) for x in prefix]
    if len(pp) < 2 or len(pp) > 65 or pp[0] != 0 or pp[-1] != n or pp != sorted(pp):
        raise _lib.HplError('%s: %s holds B + 1 <= 65 non-decreasing entries from 0 to %d, got %s' % (who, what, n, pp))
    return pp


def _flow_view(flow, N, dev, who, raw_op_hint=None):
    """A (3, N) or [N, 3] float32 flow on dev as a (3, N) view of any strides that keep its elements apart (the models' flow
    views and DenseFlow.query's answers are read in place; anything else is copied).  raw_op_hint: what to tell a caller
    whose flow requires grad."""
    if not torch.is_tensor(flow) or flow.dim() != 2 or flow.dtype != torch.float32 or flow.device != dev or \
            (tuple(flow.shape) != (3, N) and tuple(flow.shape) != (N, 3)):
        raise _lib.HplError('%s: flow must be a (3, %d) or (%d, 3) float32 tensor on %s, got %s' % (
            who, N, N, dev, (tuple(flow.shape), flow.dtype, flow.device) if torch.is_tensor(flow) else type(flow)))
    if flow.requires_grad:
        raise _lib.HplError(raw_op_hint or '%s has no autograd: flow requires grad' % who)
    if tuple(flow.shape) != (3, N):
        flow = flow.t()
    if N > 0 and (min(flow.stride()) < 1 or (flow.stride(1) == 1 and flow.stride(0) < N) or
                  (flow.stride(0) == 1 and flow.stride(1) < 3 and N > 1)):
        flow = flow.contiguous()
    return flow


_WORKSPACES = {}


def _room(who, dev, nbytes, limits, *counts):
    """(workspace, stream) of a launch on the current stream; nbytes: the answer of the op's hpl_*_workspace_bytes, negative
    when the counts are outside the limits -- `limits % counts` says which.  The scratch is per (op, device, stream), one
    buffer per size class (the next power of two): a call on another stream never shares the partial sums of one in flight."""
    if nbytes < 0:
        raise _lib.HplError('%s: %s' % (who, limits % counts))
    st = stream()
    size = 1 << max(12, (nbytes - 1).bit_length())
    key = (who, dev, st, size)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = torch.empty(size, dtype=torch.uint8, device=dev)
    return ws, st


_INF = float('inf')


def _scalar(who, name, v, zero_ok=False, inf_ok=False):
    """v as a float when it is finite and > 0 (zero_ok: >= 0; inf_ok: any value > 0, +inf too); what is no number counts as NaN."""
    try:
        v = float(v)
    except (TypeError, ValueError):
        v = float('nan')
    if not ((v >= 0 if zero_ok else v > 0) and (inf_ok or v < _INF)):
        raise _lib.HplError('%s: %s = %r (%s %s 0)' % (who, name, v, 'any value' if inf_ok else 'finite and', '>=' if zero_ok else '>'))
    return v


def _vector(who, name, t, n, dev):
    """An (n,) float32 tensor on dev without grad, contiguous."""
    if not torch.is_tensor(t) or tuple(t.shape) != (n,) or t.dtype != torch.float32 or t.device != dev or t.requires_grad:
        raise _lib.HplError('%s: %s must be a (%d,) float32 tensor on %s without grad' % (who, name, n, dev))
    return t.contiguous()


def _attrs(who, attrs, n, dev):
    """(attrs, C, row stride) of the (C, n) float32 channels, 1 <= C <= 8, that ride with a cloud's points (rows may be views
    of a wider buffer); None: (None, 0, 0)."""
    if attrs is None:
        return None, 0, 0
    if not torch.is_tensor(attrs) or attrs.dim() != 2 or attrs.shape[1] != n or attrs.dtype != torch.float32 or \
            attrs.device != dev or not 1 <= attrs.shape[0] <= 8:
        raise _lib.HplError('%s: attrs must be a (C, %d) float32 tensor on %s with 1 <= C <= 8, got %s' % (
            who, n, dev, (tuple(attrs.shape), attrs.dtype, attrs.device) if torch.is_tensor(attrs) else type(attrs)))
    if attrs.requires_grad:
        raise _lib.HplError('%s has no autograd: attrs requires grad' % who)
    C = attrs.shape[0]
    if (C > 1 and attrs.stride(0) < max(n, 1)) or (n > 1 and attrs.stride(1) != 1):
        attrs = attrs.contiguous()
    return attrs, C, max(n, 1) if C == 1 or attrs.is_contiguous() else attrs.stride(0)


def _rows_out(who, out, n, dev):
    """`out` as the contiguous [n, 3] float32 tensor on dev that takes a per-point result (None: a new one)."""
    if out is None:
        return torch.empty((n, 3), dtype=torch.float32, device=dev)
    if not torch.is_tensor(out) or tuple(out.shape) != (n, 3) or out.dtype != torch.float32 or out.device != dev or \
            not out.is_contiguous() or out.requires_grad:
        raise _lib.HplError('%s: out must be a contiguous (%d, 3) float32 tensor on %s' % (who, n, dev))
    return out


def _soa_ok(o, n, dev):
    return torch.is_tensor(o) and tuple(o.shape) == (3, n) and o.dtype == torch.float32 and o.device == dev and \
        not o.requires_grad and o.stride(0) >= max(n, 1) and (n <= 1 or o.stride(1) == 1)


def _soa_ld(x, n):
    """The row stride of a (3, n) tensor that _soa3 or _soa_ok passed: max(n, 1) for a contiguous one, else its stride(0) --
    which is a contiguous one's stride(0) too whenever n >= 1."""
    return max(n, 1) if x.is_contiguous() else x.stride(0)


def _soa_out(who, out, n, dev, along):
    """(out, row stride): `out` as a (3, n) float32 tensor on dev with unit stride along `along` (rows may be views of a wider
    buffer; None: a new one)."""
    if out is None:
        return torch.empty((3, n), dtype=torch.float32, device=dev), max(n, 1)
    if not _soa_ok(out, n, dev):
        raise _lib.HplError('%s: out must be a (3, %d) float32 tensor on %s with unit stride along %s' % (who, n, dev, along))
    return out, _soa_ld(out, n)


_PAIR_LIMITS = '%d pairs of %d points together are outside the limits (64 pairs, N < 2^31 / 3)'
_CLOUD_LIMITS = '%d clouds of %d points together are outside the limits (64 clouds, N < 2^31 / 3)'


_I64_ARRAYS = {}


def _c_prefix(pp):
    """A host prefix as the int64 array the library takes (the array types are made once a length)."""
    t = _I64_ARRAYS.get(len(pp))
    if t is None:
        t = _I64_ARRAYS[len(pp)] = ctypes.c_int64 * len(pp)
    return t(*pp)


def _identity_rt(B, dev):
    """The (B, 12) rows (R | t) of B identities: what a fit of empty pairs returns."""
    Rt = torch.zeros((B, 12), dtype=torch.float32, device=dev)
    Rt[:, 0:9:4] = 1.0
    return Rt


def knn_interpolate(ref, values, q, k=3, eps=1e-8, ref_prefix=None, q_prefix=None, return_neighbors=False, out=None,
                    coverage=None):
    """hpl_knn_interp on the current stream: for every query of q (3, Q) its k nearest points of ref (3, N),
    exact, and the inverse-distance interpolation sum w_i v_i / sum w_i, w_i = 1 / (d2_i + eps), of values [N, C] (C <= 16)
    -> [Q, C]; a query equal to a reference point gets that point's row bit for bit.  ref_prefix / q_prefix (host sequences of
    B + 1 ints from 0 to N / Q): B pairs, every query searching its own pair's points.  return_neighbors: -> (out, idx (k, Q)
    int32 into ref, dist2 (k, Q) float32), ascending; a pair of fewer than k points leaves idx = -1, dist2 = +inf.
    out + coverage (Q,): the blend form -- `out` [Q, C] holds a base value per query and is updated in place to
    coverage * base + (1 - coverage) * interpolation; rows of coverage 1 are neither searched nor written (their neighbour
    columns keep idx = -1, dist2 = +inf).  No autograd: a tensor that requires grad raises HplError."""
    _int_in('knn_interpolate', 'k', k, 1, 8)
    ref, ref_ld = _soa3(ref, 'ref')
    q, q_ld = _soa3(q, 'q')
    N, Q = ref.shape[1], q.shape[1]
    dev = ref.device
    if not torch.is_tensor(values) or values.dim() != 2 or values.shape[0] != N or values.dtype != torch.float32 or \
            values.device != dev or q.device != dev:
        raise _lib.HplError('knn_interpolate: values must be a (%d, C) float32 tensor on %s, and q on the same device' % (N, dev))
    if values.requires_grad:
        raise _lib.HplError('knn_interpolate has no autograd: values requires grad')
    values = values.contiguous()
    C = values.shape[1]
    rp = [0, N] if ref_prefix is None else [int(x) for x in ref_prefix]
    qp = [0, Q] if q_prefix is None else [int(x) for x in q_prefix]
    if len(rp) != len(qp) or len(rp) < 2 or rp[-1] != N or qp[-1] != Q:
        raise _lib.HplError('knn_interpolate: the prefixes hold B + 1 entries each and end at N = %d and Q = %d, got %s and %s'
                            % (N, Q, rp, qp))
    B = len(rp) - 1
    if (out is None) != (coverage is None):
        raise _lib.HplError('knn_interpolate: out (the base values) and coverage come together')
    if out is not None:
        for t, shape, what in ((out, (Q, C), 'out'), (coverage, (Q,), 'coverage')):
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != dev or \
                    not t.is_contiguous() or t.requires_grad:
                raise _lib.HplError('knn_interpolate: %s must be a contiguous %s float32 tensor on %s' % (what, shape, dev))
    else:
        out = torch.empty((Q, C), dtype=torch.float32, device=dev)
    idx = dist2 = None
    if return_neighbors:
        if coverage is None:
            idx = torch.empty((k, Q), dtype=torch.int32, device=dev)
            dist2 = torch.empty((k, Q), dtype=torch.float32, device=dev)
        else:
            idx = torch.full((k, Q), -1, dtype=torch.int32, device=dev)
            dist2 = torch.full((k, Q), float('inf'), dtype=torch.float32, device=dev)
    if Q == 0:
        return (out, idx, dist2) if return_neighbors else out
    check(_lib.load().hpl_knn_interp(ref.data_ptr(), ref_ld, values.data_ptr(), C, q.data_ptr(), q_ld, k, float(eps), B,
                                     _c_prefix(rp), _c_prefix(qp), ptr(idx), ptr(dist2),
                                     out.data_ptr(), ptr(coverage), stream()), 'hpl_knn_interp')
    return (out, idx, dist2) if return_neighbors else out


# --------------------------------------------------------------------------- rigid motion from flow
def rigid_fit(pc, flow, weight=None, iters=4, tau=0.1, prefix=None, return_residual=False, out=None):
    """hpl_rigid_fit on the current stream: the rigid motion q = R p + t that explains most of the flow of
    each pair, fitted by iteratively reweighted least squares (Geman-McClure weights of scale tau, iters reweighted solves
    after the plain one; float64 sums in a fixed order), and the flow refined by it.  pc (3, N) float32; flow (3, N) or
    [N, 3] float32 of any strides (the models' flow views and DenseFlow.query's answers are read in place; a (3, 3) tensor is
    (3, N)); weight (N,) float32 or None -- for a dense flow, its coverage --: a weight that is not > 0 (NaN included) and a
    non-finite point count as 0.  prefix (host sequence of B + 1 ints from 0 to N): B <= 64 pairs, each with its own fit.
    -> (R (B, 3, 3), t (B, 3), stats (B, 4) = (status, inlier share, rotation angle in degrees, |t|), refined [N, 3]
    [, residual (N,)]): an inlier (residual <= tau, weight > 0) gets the rigid flow R p + t - p, any other point its input
    flow bit for bit.  status 0 (fewer than 3 points, or no weight): R = I, t = 0, refined = flow.  out: a contiguous [N, 3]
    float32 tensor that takes the refined flow (it must not overlap flow).  No autograd, no host synchronisation."""
    _int_in('rigid_fit', 'iters', iters, 0, 16)
    tau = _scalar('rigid_fit', 'tau', tau)
    pc, pc_ld = _soa3(pc, 'pc', 'rigid_fit')
    N, dev = pc.shape[1], pc.device
    flow = _flow_view(flow, N, dev, 'rigid_fit')
    if weight is not None:
        weight = _vector('rigid_fit', 'weight', weight, N, dev)
    pp = _prefix(prefix, N, 'rigid_fit')
    B = len(pp) - 1
    out = _rows_out('rigid_fit', out, N, dev)
    residual = torch.empty(N, dtype=torch.float32, device=dev) if return_residual else None
    lib = _lib.load()
    if N == 0:                                   # nothing to launch: every pair is empty
        Rt = _identity_rt(B, dev)
        stats = torch.zeros((B, 4), dtype=torch.float32, device=dev)
    else:
        Rt = torch.empty((B, 12), dtype=torch.float32, device=dev)
        stats = torch.empty((B, 4), dtype=torch.float32, device=dev)
        ws, st = _room('rigid_fit', dev, lib.hpl_rigid_fit_workspace_bytes(B, N), _PAIR_LIMITS, B, N)
        check(lib.hpl_rigid_fit(pc.data_ptr(), pc_ld, flow.data_ptr(), flow.stride(0), flow.stride(1), ptr(weight), B,
                                _c_prefix(pp), iters, tau, Rt.data_ptr(), stats.data_ptr(), ptr(residual),
                                out.data_ptr(), ws.data_ptr(), ws.numel(), st), 'hpl_rigid_fit')
    res = (Rt[:, :9].view(B, 3, 3), Rt[:, 9:], stats, out)
    return res + (residual,) if return_residual else res


# --------------------------------------------------------------------------- rigid registration of a cloud pair
def icp(src, dst, weight=None, init=None, iters=30, max_dist=1.0, tau=0.3, tol_rot=0.0, tol_trans=0.0, src_prefix=None,
        dst_prefix=None, return_matches=False, out=None, metric='point', dst_normal=None):
    """hpl_icp on the current stream: per pair the rigid motion q = R p + t that lays src (3, N) onto dst (3, M)
    by robust point-to-point ICP -- each round matches every moved src point to its exact nearest dst point within max_dist
    (a sorted grid over dst, built once a call), weighs the matches by Geman-McClure of scale tau and solves as ops.rigid_fit
    does; the motion a round hands on is rounded to float32.  weight (N,) float32 or None: a weight that is not in (0, inf)
    and a non-finite point count as 0.  init: a pair (R (B, 3, 3), t (B, 3)) of float32 device tensors -- an ops.rigid_fit
    result passes straight in -- or None (identity).  iters 0 .. 64 rounds at most; a pair stops once a round changes no R
    entry by more than tol_rot and no t entry by more than tol_trans (0: at a bitwise fixpoint).  src_prefix / dst_prefix (host
    sequences of B + 1 ints from 0 to N / M): B <= 64 pairs, N_b != M_b allowed.
    -> (R (B, 3, 3), t (B, 3), stats (B, 6) = (status, matched share, RMSE of the matches, rotation angle in degrees, |t|,
    rounds run), flow [N, 3] = R p + t - p [, match (N,) int32 into the packed dst or -1, dist2 (N,) float32 or +inf]).
    status 0 (fewer than 3 src points, no dst point, or a round without any match): the motion is the one the failed round
    started from.  out: a contiguous [N, 3] float32 tensor that takes the flow.  No autograd, no host synchronisation.
    metric='plane' (hpl_icp_plane) takes dst_normal (3, M) float32 -- ops.normals(dst)[0] --: the round minimises
    the residuals along the matched points' normals (a match on a zero or non-finite normal takes no part) by a minimum-norm
    Gauss-Newton step; match, stop, failure, finish and the outputs are the same."""
    if metric not in ('point', 'plane'):
        raise _lib.HplError('icp: metric = %r (\'point\' or \'plane\')' % (metric,))
    if (metric == 'plane') != (dst_normal is not None):
        raise _lib.HplError('icp: metric \'plane\' takes dst_normal (3, M), metric \'point\' takes none')
    _int_in('icp', 'iters', iters, 0, 64)
    max_dist, tau = _scalar('icp', 'max_dist', max_dist), _scalar('icp', 'tau', tau)
    tol_rot, tol_trans = _scalar('icp', 'tol_rot', tol_rot, True), _scalar('icp', 'tol_trans', tol_trans, True)
    src, src_ld = _soa3(src, 'src', 'icp')
    dst, dst_ld = _soa3(dst, 'dst', 'icp')
    N, M, dev = src.shape[1], dst.shape[1], src.device
    if dst.device != dev:
        raise _lib.HplError('icp: src is on %s, dst on %s' % (dev, dst.device))
    if dst_normal is not None:
        dst_normal, dn_ld = _soa3(dst_normal, 'dst_normal', 'icp')
        if dst_normal.shape[1] != M or dst_normal.device != dev:
            raise _lib.HplError('icp: dst_normal must be a (3, %d) float32 tensor on %s' % (M, dev))
    if weight is not None:
        weight = _vector('icp', 'weight', weight, N, dev)
    sp = _prefix(src_prefix, N, 'icp', 'the prefix of src')
    dp = _prefix(dst_prefix, M, 'icp', 'the prefix of dst')
    if len(sp) != len(dp):
        raise _lib.HplError('icp: the prefixes hold B + 1 entries each, got %d and %d' % (len(sp), len(dp)))
    B = len(sp) - 1
    if init is not None:
        if not isinstance(init, (list, tuple)) or len(init) != 2:
            raise _lib.HplError('icp: init is a pair (R (%d, 3, 3), t (%d, 3)) of float32 tensors on %s' % (B, B, dev))
        for t_, shape in zip(init, ((B, 3, 3), (B, 3))):
            if not torch.is_tensor(t_) or tuple(t_.shape) != shape or t_.dtype != torch.float32 or t_.device != dev or \
                    t_.requires_grad:
                raise _lib.HplError('icp: init is a pair (R (%d, 3, 3), t (%d, 3)) of float32 tensors on %s without grad' % (B, B, dev))
        init = torch.cat([init[0].reshape(B, 9), init[1]], dim=1).contiguous()
    out = _rows_out('icp', out, N, dev)
    match = torch.empty(N, dtype=torch.int32, device=dev) if return_matches else None
    dist2 = torch.empty(N, dtype=torch.float32, device=dev) if return_matches else None
    lib = _lib.load()
    if N == 0:                                   # nothing to launch: every src cloud is empty
        Rt = _identity_rt(B, dev) if init is None else init
        stats = torch.zeros((B, 6), dtype=torch.float32, device=dev)
    else:
        Rt = torch.empty((B, 12), dtype=torch.float32, device=dev)
        stats = torch.empty((B, 6), dtype=torch.float32, device=dev)
        nbytes = (lib.hpl_icp_plane_workspace_bytes if metric == 'plane' else lib.hpl_icp_workspace_bytes)(B, N, M)
        ws, st = _room('icp', dev, nbytes, '%d pairs of %d and %d points together are outside the limits (64 pairs, N, M < 2^31 / 3)',
                       B, N, M)
        tail = (ptr(weight), ptr(init), B, _c_prefix(sp), _c_prefix(dp), iters, max_dist, tau,
                tol_rot, tol_trans, Rt.data_ptr(), stats.data_ptr(), ptr(match), ptr(dist2), out.data_ptr(), ws.data_ptr(),
                ws.numel(), st)
        if metric == 'plane':
            check(lib.hpl_icp_plane(src.data_ptr(), src_ld, dst.data_ptr(), dst_ld, dst_normal.data_ptr(), dn_ld, *tail),
                  'hpl_icp_plane')
        else:
            check(lib.hpl_icp(src.data_ptr(), src_ld, dst.data_ptr(), dst_ld, *tail), 'hpl_icp')
    res = (Rt[:, :9].view(B, 3, 3), Rt[:, 9:], stats, out)
    return res + (match, dist2) if return_matches else res


# --------------------------------------------------------------------------- surface normals
def normals(pc, k=16, radius=1.0, viewpoint=None, prefix=None, return_neighbors=False, out=None):
    """hpl_normals on the current stream: per point of pc (3, N) its k (3 .. 32) nearest points of the same cloud
    within radius, itself included, exact and ordered by (d2, index) -- a sorted grid over the cloud, built once a call --, and
    the unit eigenvector of the smallest eigenvalue of their float64 scatter matrix, turned towards the cloud's viewpoint.
    viewpoint: three numbers for every cloud, B triples, or None (the origin); host values.  prefix (host sequence of B + 1 ints
    from 0 to N): B <= 64 clouds, every point searching its own cloud.
    -> (normal (3, N) float32, curvature (N,) float32 = lambda_min / sum lambda, count (N,) int32 <= k [, nbr (N, k) int32 into
    the packed cloud, then -1, nbr_d2 (N, k) float32, then +inf]).  A point with fewer than 3 neighbours, a degenerate
    neighbourhood or a non-finite or out-of-range position has the normal (0, 0, 0) and the curvature 0.  out: a (3, N) float32
    tensor with unit stride along its points (rows may be views of a wider buffer) that takes the normal.  No autograd, no host
    synchronisation."""
    _int_in('normals', 'k', k, 3, 32)
    radius = _scalar('normals', 'radius', radius)
    pc, pc_ld = _soa3(pc, 'pc', 'normals')
    N, dev = pc.shape[1], pc.device
    pp = _prefix(prefix, N, 'normals')
    B = len(pp) - 1
    view = None
    if viewpoint is not None:
        try:
            v = torch.as_tensor(viewpoint, dtype=torch.float32, device='cpu').reshape(-1).tolist()
        except (TypeError, ValueError, RuntimeError):
            v = []
        if len(v) == 3:
            v = v * B
        if len(v) != 3 * B:
            raise _lib.HplError('normals: viewpoint holds three numbers or %d triples, got %r' % (B, viewpoint))
        view = (ctypes.c_float * (3 * B))(*v)
    out, out_ld = _soa_out('normals', out, N, dev, 'its points')
    curvature = torch.empty(N, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    nbr = torch.empty((N, k), dtype=torch.int32, device=dev) if return_neighbors else None
    nbr_d2 = torch.empty((N, k), dtype=torch.float32, device=dev) if return_neighbors else None
    if N > 0:
        lib = _lib.load()
        ws, st = _room('normals', dev, lib.hpl_normals_workspace_bytes(B, N), _CLOUD_LIMITS, B, N)
        check(lib.hpl_normals(pc.data_ptr(), pc_ld, B, _c_prefix(pp), k, radius, view, out.data_ptr(),
                              out_ld, ptr(curvature), ptr(count), ptr(nbr), ptr(nbr_d2), ws.data_ptr(), ws.numel(), st),
              'hpl_normals')
    res = (out, curvature, count)
    return res + (nbr, nbr_d2) if return_neighbors else res


# --------------------------------------------------------------------------- outlier removal
OUTLIER_MODES = {'statistical': 0, 'radius': 1}


def outlier_args(who, mode, k, radius, std_ratio, min_neighbors):
    """(the mode's number, k, radius, std_ratio, min_neighbors as the library takes them) or an HplError: k 1 .. 32 and std_ratio
    finite and >= 0 in mode 'statistical', which refuses min_neighbors; min_neighbors 1 .. 2^31 - 1 required in mode 'radius'."""
    if mode not in OUTLIER_MODES:
        raise _lib.HplError('%s: mode = %r (%s)' % (who, mode, ' or '.join(repr(m) for m in OUTLIER_MODES)))
    radius = _scalar(who, 'radius', radius)
    if mode == 'statistical':
        _int_in(who, 'k', k, 1, 32)
        std_ratio = _scalar(who, 'std_ratio', std_ratio, True)
        if min_neighbors is not None:
            raise _lib.HplError('%s: min_neighbors applies to mode \'radius\', got %r in mode \'statistical\'' % (who, min_neighbors))
        min_neighbors = 0
    else:
        if min_neighbors is None:
            raise _lib.HplError('%s: mode \'radius\' needs min_neighbors (an int in 1 .. %d)' % (who, 2 ** 31 - 1))
        _int_in(who, 'min_neighbors', min_neighbors, 1, 2 ** 31 - 1)
        k, std_ratio = 0, 0.0
    return OUTLIER_MODES[mode], k, radius, std_ratio, min_neighbors


def outlier_filter(pc, mode='statistical', k=16, radius=1.0, std_ratio=2.0, min_neighbors=None, prefix=None,
                   return_neighbors=False, out=None):
    """hpl_outlier_filter on the current stream: the stray points of pc (3, N), exact over all pairs of a cloud
    (a sorted grid over the cloud, built once a call, finds the candidates).  A point's neighbours are the OTHER points of its
    cloud within radius.  mode 'statistical': mean_dist = the mean distance to the k (1 .. 32) nearest neighbours, a missing one
    counted at the radius; per cloud mu and the sample sigma of mean_dist; kept iff mean_dist <= T = mu + std_ratio sigma (the
    float32 values as returned).  mode 'radius': kept iff the point has at least min_neighbors neighbours.  A point that is not
    finite or out of the grid's range is removed and takes no part.  prefix (host sequence of B + 1 ints from 0 to N): B <= 64
    clouds, each filtered on its own.
    -> (keep (N,) uint8, keep_idx (N,) int32: per cloud from prefix[b] on the packed indices of its kept points, ascending,
    then -1, mean_dist (N,) float32 (None in mode 'radius'), count (N,) int32: min(k, neighbours), or all neighbours in mode
    'radius', thresh (B, 4) float32 = (mu, sigma, T, 0), zeros in mode 'radius', stats (B, 4) int32 = (taking part, kept, removed
    though taking part, not taking part)[, nbr_d2 (N, k) float32: the squared distances ascending, then +inf; mode
    'statistical' only]).  out: a contiguous (N,) uint8 tensor that takes keep.  The same bits for a cloud alone and in any
    batch.  No autograd, no host synchronisation, no read-back."""
    who = 'outlier_filter'
    m, k, radius, std_ratio, min_neighbors = outlier_args(who, mode, k, radius, std_ratio, min_neighbors)
    if return_neighbors and m != 0:
        raise _lib.HplError('outlier_filter: return_neighbors applies to mode \'statistical\'')
    pc, pc_ld = _soa3(pc, 'pc', who)
    N, dev = pc.shape[1], pc.device
    pp = _prefix(prefix, N, who)
    B = len(pp) - 1
    if out is None:
        keep = torch.empty(N, dtype=torch.uint8, device=dev)
    elif not torch.is_tensor(out) or tuple(out.shape) != (N,) or out.dtype != torch.uint8 or out.device != dev or \
            not out.is_contiguous():
        raise _lib.HplError('outlier_filter: out must be a contiguous (%d,) uint8 tensor on %s' % (N, dev))
    else:
        keep = out
    keep_idx = torch.empty(N, dtype=torch.int32, device=dev)
    mean_dist = torch.empty(N, dtype=torch.float32, device=dev) if m == 0 else None
    count = torch.empty(N, dtype=torch.int32, device=dev)
    nbr_d2 = torch.empty((N, k), dtype=torch.float32, device=dev) if return_neighbors else None
    if N == 0:                                   # nothing to launch: every cloud is empty
        thresh = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    else:
        thresh = torch.empty((B, 4), dtype=torch.float32, device=dev)
        stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
        lib = _lib.load()
        ws, st = _room(who, dev, lib.hpl_outlier_filter_workspace_bytes(B, N), _CLOUD_LIMITS, B, N)
        check(lib.hpl_outlier_filter(pc.data_ptr(), pc_ld, B, _c_prefix(pp), m, k, radius, std_ratio, min_neighbors,
                                     keep.data_ptr(), keep_idx.data_ptr(), ptr(mean_dist), count.data_ptr(), ptr(nbr_d2),
                                     thresh.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), st), 'hpl_outlier_filter')
    res = (keep, keep_idx, mean_dist, count, thresh, stats)
    return res + (nbr_d2,) if return_neighbors else res


# --------------------------------------------------------------------------- moving objects from flow
def motion_segment(pc, flow, residual, tau=0.1, eps=0.5, dv=float('inf'), min_points=5, max_objects=256, prefix=None, out=None):
    """hpl_motion_segment on the current stream: the points whose residual against a rigid fit exceeds tau
    (the movers), grouped into the connected components of the graph that links two movers of a pair within eps metres of
    each other whose flows differ by at most dv (+inf: positions alone); a component of at least min_points movers is an
    object, numbered per pair in the order of its smallest point index.  pc (3, N) float32, flow (3, N) or [N, 3] float32 of
    any strides, prefix: exactly as ops.rigid_fit takes them (read in place); residual (N,) float32 as rigid_fit returns it.
    -> (labels (N,) int32: object number, -1 no mover, -2 noise, -3 out of the grid's range; obj_info (B, max_objects, 2) int32:
    root index within the pair and point count, unused rows -1, 0; obj_motion (B, max_objects, 6) float32: centroid and mean
    flow, unused rows 0; stats (B, 4) int32: movers, objects -- the true count, also past max_objects --, points in objects,
    points out of range).  out: a contiguous (N,) int32 tensor that takes the labels.  The same bits for a pair alone and in
    any batch.  No autograd, no host synchronisation, no read-back."""
    tau, eps = _scalar('motion_segment', 'tau', tau), _scalar('motion_segment', 'eps', eps)
    dv = _scalar('motion_segment', 'dv', dv, inf_ok=True)
    _int_in('motion_segment', 'min_points', min_points, 1, 2 ** 31 - 1)
    _int_in('motion_segment', 'max_objects', max_objects, 1, 4096)
    pc, pc_ld = _soa3(pc, 'pc', 'motion_segment')
    N, dev = pc.shape[1], pc.device
    flow = _flow_view(flow, N, dev, 'motion_segment')
    residual = _vector('motion_segment', 'residual', residual, N, dev)
    pp = _prefix(prefix, N, 'motion_segment')
    B = len(pp) - 1
    if out is not None:
        if not torch.is_tensor(out) or tuple(out.shape) != (N,) or out.dtype != torch.int32 or out.device != dev or \
                not out.is_contiguous():
            raise _lib.HplError('motion_segment: out must be a contiguous (%d,) int32 tensor on %s' % (N, dev))
        labels = out
    else:
        labels = torch.empty(N, dtype=torch.int32, device=dev)
    lib = _lib.load()
    if N == 0:                                   # nothing to launch: every pair is empty
        info = torch.zeros((B, max_objects, 2), dtype=torch.int32, device=dev)
        info[:, :, 0] = -1
        return (labels, info, torch.zeros((B, max_objects, 6), dtype=torch.float32, device=dev),
                torch.zeros((B, 4), dtype=torch.int32, device=dev))
    info = torch.empty((B, max_objects, 2), dtype=torch.int32, device=dev)
    motion = torch.empty((B, max_objects, 6), dtype=torch.float32, device=dev)
    stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws, st = _room('motion_segment', dev, lib.hpl_motion_segment_workspace_bytes(B, N), _PAIR_LIMITS, B, N)
    check(lib.hpl_motion_segment(pc.data_ptr(), pc_ld, flow.data_ptr(), flow.stride(0), flow.stride(1), residual.data_ptr(), B,
                                 _c_prefix(pp), tau, eps, dv, min_points, max_objects, labels.data_ptr(),
                                 info.data_ptr(), motion.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), st),
          'hpl_motion_segment')
    return labels, info, motion, stats


# --------------------------------------------------------------------------- object motions from flow
def _inplace(who, name, t, shape, dtype, dev):
    """t as the contiguous tensor of that shape and dtype on dev that a kernel reads or updates where it lies."""
    if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous() or \
            t.requires_grad:
        raise _lib.HplError('%s: %s must be a contiguous %s %s tensor on %s without grad' % (
            who, name, shape, str(dtype).replace('torch.', ''), dev))
    return t


def object_fit(pc, flow, labels, weight=None, max_objects=256, iters=4, tau=0.1, prefix=None, residual=None, refined=None,
               out=None):
    """hpl_object_fit on the current stream: ops.rigid_fit per labelled object.  pc (3, N) float32, flow (3, N)
    or [N, 3] float32 of any strides, weight, iters, tau, prefix: exactly as ops.rigid_fit takes them (read in place); labels
    (N,) int32 as ops.motion_segment returns them, or any other labelling: object o of a pair is its points of label o, in
    ascending index, and a label outside 0 .. max_objects - 1 belongs to no object.
    -> (obj_Rt (B, max_objects, 12): R row-major, then t; obj_stats (B, max_objects, 4): status, the inlier share of the
    object's members, the rotation angle in degrees, |t| [, residual][, refined]): every row is what ops.rigid_fit returns for
    the object's members gathered as one pair, bit for bit; a row without members holds R = I, t = 0, stats 0.
    residual (N,) and refined [N, 3] (contiguous float32) are UPDATED IN PLACE and returned when given: residual at every
    member of a listed object, refined at the inliers of a fitted object (R_o p + t_o - p); every other row keeps its bits.
    Handed what ops.rigid_fit(return_residual=True) returned, they become the piecewise-rigid flow and its residual.
    out: a pair of contiguous float32 tensors (B, max_objects, 12) and (B, max_objects, 4) that take obj_Rt and obj_stats.
    No autograd, no host synchronisation, no read-back."""
    _int_in('object_fit', 'max_objects', max_objects, 1, 4096)
    _int_in('object_fit', 'iters', iters, 0, 16)
    tau = _scalar('object_fit', 'tau', tau)
    pc, pc_ld = _soa3(pc, 'pc', 'object_fit')
    N, dev = pc.shape[1], pc.device
    flow = _flow_view(flow, N, dev, 'object_fit')
    labels = _inplace('object_fit', 'labels', labels, (N,), torch.int32, dev)
    if weight is not None:
        weight = _vector('object_fit', 'weight', weight, N, dev)
    pp = _prefix(prefix, N, 'object_fit')
    B = len(pp) - 1
    if residual is not None:
        residual = _inplace('object_fit', 'residual', residual, (N,), torch.float32, dev)
    if refined is not None:
        refined = _inplace('object_fit', 'refined', refined, (N, 3), torch.float32, dev)
    if out is not None:
        if not isinstance(out, (list, tuple)) or len(out) != 2:
            raise _lib.HplError('object_fit: out is a pair of tensors (obj_Rt, obj_stats)')
        Rt = _inplace('object_fit', 'out[0]', out[0], (B, max_objects, 12), torch.float32, dev)
        stats = _inplace('object_fit', 'out[1]', out[1], (B, max_objects, 4), torch.float32, dev)
    else:
        Rt = torch.empty((B, max_objects, 12), dtype=torch.float32, device=dev)
        stats = torch.empty((B, max_objects, 4), dtype=torch.float32, device=dev)
    if N == 0:                                   # nothing to launch: every object is empty
        Rt.copy_(_identity_rt(B * max_objects, dev).view(B, max_objects, 12))
        stats.zero_()
    else:
        lib = _lib.load()
        ws, st = _room('object_fit', dev, lib.hpl_object_fit_workspace_bytes(B, N, max_objects), _PAIR_LIMITS, B, N)
        check(lib.hpl_object_fit(pc.data_ptr(), pc_ld, flow.data_ptr(), flow.stride(0), flow.stride(1), ptr(weight),
                                 labels.data_ptr(), B, _c_prefix(pp), max_objects, iters, tau, Rt.data_ptr(), stats.data_ptr(),
                                 ptr(residual), ptr(refined), ws.data_ptr(), ws.numel(), st), 'hpl_object_fit')
    res = (Rt, stats)
    if residual is not None:
        res += (residual,)
    if refined is not None:
        res += (refined,)
    return res


# --------------------------------------------------------------------------- ground removal
def ground_min_cos(max_tilt_deg):
    """The float32 cosine hpl_ground_fit takes for a largest tilt in degrees (0 <= tilt < 90)."""
    t = float(max_tilt_deg)
    if not 0 <= t < 90:
        raise _lib.HplError('ground_fit: max_tilt_deg = %r (0 <= tilt < 90 degrees)' % (max_tilt_deg,))
    return struct.unpack('f', struct.pack('f', math.cos(math.radians(t))))[0]


def ground_fit(pc, prefix=None, up=(0, 1, 0), max_tilt_deg=20.0, hyps=256, tau=0.1, refine=2, cut=0.3, seed=0, call=0,
               return_votes=False, return_height=False):
    """hpl_ground_fit on the current stream: per cloud the ground plane n . x + d = 0 by RANSAC (hyps
    three-point hypotheses from the counter-based stream (seed, call); a hypothesis whose normal tilts more than max_tilt_deg
    from `up` is no candidate; a point votes within tau of the plane), refined by `refine` least-squares rounds on its inliers,
    and every point classified by its signed height: ground when it is finite and at most `cut` above the plane.  pc (3, N)
    float32 (rows may be views of a wider buffer); prefix (host sequence of B + 1 ints from 0 to N): B <= 64 clouds, each with
    its own plane.
    -> (plane (B, 4) float32 = (n, d), stats (B, 4) int32 = (status, winning hypothesis, its votes, kept count), ground (N,)
    uint8, keep_idx (N,) int32: per cloud from prefix[b] on the packed indices of its kept points, ascending, then -1
    [, votes (B, hyps) int32, -1 an invalid hypothesis][, height (N,) float32, NaN at a non-finite point]).  status 0 (no valid
    hypothesis, fewer than 3 points): plane 0, nothing ground, every index kept.  No autograd, no host synchronisation."""
    _int_in('ground_fit', 'hyps', hyps, 1, 1024)
    _int_in('ground_fit', 'refine', refine, 0, 8)
    tau, cut = _scalar('ground_fit', 'tau', tau), _scalar('ground_fit', 'cut', cut, True)
    min_cos = ground_min_cos(max_tilt_deg)
    try:
        upv = [float(x) for x in up]
    except TypeError:
        upv = []
    if len(upv) != 3 or not all(abs(x) < float('inf') for x in upv) or not any(upv):
        raise _lib.HplError('ground_fit: up = %r (three finite numbers, not all zero)' % (up,))
    _int_in('ground_fit', 'seed', seed, 0, 2 ** 64 - 1)
    _int_in('ground_fit', 'call', call, 0, 2 ** 64 - 1)
    pc, pc_ld = _soa3(pc, 'pc', 'ground_fit')
    N, dev = pc.shape[1], pc.device
    pp = _prefix(prefix, N, 'ground_fit')
    B = len(pp) - 1
    lib = _lib.load()
    votes = height = None
    if N == 0:                                   # nothing to launch: every cloud is empty
        plane = torch.zeros((B, 4), dtype=torch.float32, device=dev)
        stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        stats[:, 1] = -1
        ground = torch.zeros(0, dtype=torch.uint8, device=dev)
        keep = torch.zeros(0, dtype=torch.int32, device=dev)
        if return_votes:
            votes = torch.full((B, hyps), -1, dtype=torch.int32, device=dev)
        if return_height:
            height = torch.zeros(0, dtype=torch.float32, device=dev)
    else:
        plane = torch.empty((B, 4), dtype=torch.float32, device=dev)
        stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
        ground = torch.empty(N, dtype=torch.uint8, device=dev)
        keep = torch.empty(N, dtype=torch.int32, device=dev)
        if return_votes:
            votes = torch.empty((B, hyps), dtype=torch.int32, device=dev)
        if return_height:
            height = torch.empty(N, dtype=torch.float32, device=dev)
        ws, st = _room('ground_fit', dev, lib.hpl_ground_fit_workspace_bytes(B, N, hyps), _CLOUD_LIMITS, B, N)
        check(lib.hpl_ground_fit(pc.data_ptr(), pc_ld, B, _c_prefix(pp), (ctypes.c_float * 3)(*upv), min_cos,
                                 hyps, tau, refine, cut, seed, call, plane.data_ptr(), stats.data_ptr(), ptr(votes), ptr(height),
                                 ground.data_ptr(), keep.data_ptr(), ws.data_ptr(), ws.numel(), st), 'hpl_ground_fit')
    res = (plane, stats, ground, keep)
    if return_votes:
        res += (votes,)
    if return_height:
        res += (height,)
    return res


# --------------------------------------------------------------------------- voxel-grid downsampling
VOXEL_MODES = {'centroid': 0, 'nearest': 1}


def voxel_args(who, voxel, origin, mode):
    """(voxel as the float32 the library takes, origin as three floats, the mode's number) or an HplError."""
    try:
        v = struct.unpack('f', struct.pack('f', float(voxel)))[0]
    except (TypeError, ValueError, OverflowError):
        v = float('nan')
    if isinstance(voxel, bool) or not (v > 0 and v < float('inf')):
        raise _lib.HplError('%s: voxel = %r (finite and > 0 as a float32)' % (who, voxel))
    try:
        org = [float(x) for x in origin]
    except (TypeError, ValueError):
        org = []
    if len(org) != 3 or not all(abs(x) <= 3.4028234663852886e38 for x in org):
        raise _lib.HplError('%s: origin = %r (three finite numbers)' % (who, origin))
    if mode not in VOXEL_MODES:
        raise _lib.HplError('%s: mode = %r (%s)' % (who, mode, ' or '.join(repr(m) for m in VOXEL_MODES)))
    return v, org, VOXEL_MODES[mode]


def voxel_downsample(pc, attrs=None, voxel=0.1, origin=(0, 0, 0), mode='centroid', prefix=None, out=None):
    """hpl_voxel_downsample on the current stream: one point per occupied cell of the grid of edge `voxel`
    anchored at `origin` -- mode 'centroid': the mean of the cell's points; 'nearest': the member nearest to that mean, bit for
    bit, so the output is a subset of the input.  pc (3, N) float32 (rows may be views of a wider buffer); attrs (C, N) float32,
    C <= 8, or None: channels that are averaged (or picked) with their points; prefix (host sequence of B + 1 ints from 0 to
    N): B <= 64 clouds, each voxelised on its own.  A cloud's voxels are numbered in ascending (cell_x, cell_y, cell_z) order;
    voxel v of cloud b is column prefix[b] + v of every per-voxel output, and the columns behind a cloud's V_b voxels hold 0
    (rep: -1).  A point that is not finite, or whose cell lies outside +-(2^18 - 2), belongs to no voxel.
    -> (out_pc (3, N) float32, out_attrs (C, N) float32 or None, count (N,) int32, rep (N,) int32: the packed index of the member
    nearest to the mean, voxel_of (N,) int32: every point's voxel column or -1 -- a per-voxel result goes back to the points
    as values[:, voxel_of] --, stats (B, 4) int32 = (V_b, valid, non-finite, out-of-range points)).  out: a (3, N) float32
    tensor with unit stride along the points that takes out_pc; it must not overlap pc or attrs.  The same bits for a cloud
    alone and in any batch.  No autograd, no host synchronisation, no read-back: V_b stays on the device."""
    who = 'voxel_downsample'
    v, org, m = voxel_args(who, voxel, origin, mode)
    pc, pc_ld = _soa3(pc, 'pc', who)
    N, dev = pc.shape[1], pc.device
    attrs, C, attr_ld = _attrs(who, attrs, N, dev)
    pp = _prefix(prefix, N, who)
    B = len(pp) - 1
    out_pc, out_ld = _soa_out(who, out, N, dev, 'the points')
    out_attrs = torch.empty((C, N), dtype=torch.float32, device=dev) if C else None
    count = torch.empty(N, dtype=torch.int32, device=dev)
    rep = torch.empty(N, dtype=torch.int32, device=dev)
    voxel_of = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:                                   # nothing to launch: every cloud is empty
        return out_pc, out_attrs, count, rep, voxel_of, torch.zeros((B, 4), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws, st = _room(who, dev, lib.hpl_voxel_downsample_workspace_bytes(B, N, C), _CLOUD_LIMITS, B, N)
    check(lib.hpl_voxel_downsample(pc.data_ptr(), pc_ld, ptr(attrs), attr_ld, C, B, _c_prefix(pp), v,
                                   (ctypes.c_float * 3)(*org), m, out_pc.data_ptr(), out_ld, ptr(out_attrs), max(N, 1),
                                   count.data_ptr(), rep.data_ptr(), voxel_of.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                   ws.numel(), st), 'hpl_voxel_downsample')
    return out_pc, out_attrs, count, rep, voxel_of, stats


# --------------------------------------------------------------------------- farthest point sampling
FPS_PATHS = {'auto': 0, 'resident': 1, 'rounds': 2}


def fps_resident_capacity():
    """The most points a cloud may hold on fps's resident path."""
    return int(_lib.load().hpl_fps_resident_capacity())


def fps_args(who, m, batch, path='auto'):
    """(m, the path's number) or an HplError: m a non-bool int >= 1 with batch * m inside the 32-bit limit."""
    if isinstance(m, bool) or not isinstance(m, int) or m < 1 or batch * m >= (2 ** 31 + 2) // 3:
        raise _lib.HplError('%s: %r samples for each of %d clouds (an int >= 1, together below 2^31 / 3)' % (who, m, batch))
    if not isinstance(path, str) or path not in FPS_PATHS:
        raise _lib.HplError('%s: path = %r (%s)' % (who, path, ', '.join(repr(p) for p in FPS_PATHS)))
    return m, FPS_PATHS[path]


def fps(pc, m, attrs=None, start=None, prefix=None, path='auto', return_cover=False, out=None):
    """hpl_fps on the current stream: farthest point sampling, m points per cloud in selection order -- sample 0
    is the cloud's start (start[b], a cloud-local index; None, or a start whose point is not finite: the smallest finite
    index), every further sample the finite point farthest (float32 d2, ties to the smaller index) from all samples before it;
    a cloud stops early when every remaining point coincides with a sample.  pc (3, N) float32 (rows may be views of a wider
    buffer); attrs (C, N) float32, C <= 8, or None: channels gathered with their points; prefix (host sequence of B + 1 ints
    from 0 to N): B <= 64 clouds, each sampled on its own; start: None or a host sequence of B ints; path: 'auto', 'resident'
    (one launch, clouds of at most fps_resident_capacity() points) or 'rounds' (one launch a round, any size) -- the same bits.
    -> (out_pc (3, B m) float32: column b m + j is sample j of cloud b, 0 past the cloud's count; out_attrs (C, B m) or None;
    idx (B, m) int32, cloud-local, -1 past the count; dist (B, m) float32: each sample's distance to the samples before it
    when it was chosen, +inf for sample 0, 0 past the count; cover (N,) float32 with return_cover, else None: every point's
    squared distance to its nearest sample; stats (B, 4) int32 = (count, finite points, others, the path taken: 1 or 2)).
    out: a (3, B m) float32 tensor with unit stride along the samples that takes out_pc; it must not overlap pc or attrs.  The
    same bits for a cloud alone and in any batch.  No autograd, no host synchronisation, no read-back."""
    who = 'fps'
    pc, pc_ld = _soa3(pc, 'pc', who)
    N, dev = pc.shape[1], pc.device
    attrs, C, attr_ld = _attrs(who, attrs, N, dev)
    pp = _prefix(prefix, N, who)
    B = len(pp) - 1
    m, pnum = fps_args(who, m, B, path)
    M = B * m
    st = None
    if start is not None:
        try:
            st = [None if isinstance(x, bool) else operator.index(x) for x in start]
        except TypeError:
            st = None
        if st is None or len(st) != B or None in st or any(pp[b + 1] > pp[b] and not 0 <= st[b] < pp[b + 1] - pp[b] for b in range(B)):
            raise _lib.HplError('%s: start holds %d ints, each an index into its cloud, got %r' % (who, B, start))
        st = (ctypes.c_int32 * B)(*[x if pp[b + 1] > pp[b] else 0 for b, x in enumerate(st)])
    out_pc, out_ld = _soa_out(who, out, M, dev, 'the samples')
    if N == 0:                                   # nothing to launch: every cloud is empty
        out_pc.zero_()
        return (out_pc, torch.zeros((C, M), dtype=torch.float32, device=dev) if C else None,
                torch.full((B, m), -1, dtype=torch.int32, device=dev), torch.zeros((B, m), dtype=torch.float32, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev) if return_cover else None,
                torch.zeros((B, 4), dtype=torch.int32, device=dev))
    out_attrs = torch.empty((C, M), dtype=torch.float32, device=dev) if C else None
    idx = torch.empty((B, m), dtype=torch.int32, device=dev)
    dist = torch.empty((B, m), dtype=torch.float32, device=dev)
    cover = torch.empty(N, dtype=torch.float32, device=dev) if return_cover else None
    stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws, s = _room(who, dev, lib.hpl_fps_workspace_bytes(B, N, m, C), _CLOUD_LIMITS, B, N)
    check(lib.hpl_fps(pc.data_ptr(), pc_ld, ptr(attrs), attr_ld, C, B, _c_prefix(pp), st, m, pnum,
                      idx.data_ptr(), dist.data_ptr(), out_pc.data_ptr(), out_ld, ptr(out_attrs), M, ptr(cover),
                      stats.data_ptr(), ws.data_ptr(), ws.numel(), s), 'hpl_fps')
    return out_pc, out_attrs, idx, dist, cover, stats


# --------------------------------------------------------------------------- frames from raw maps
def _frames_plane(who, name, t, dtypes, shape, dev):
    """A packed per-pixel device tensor of the given shape and one of the dtypes, contiguous (a view that starts anywhere in a
    wider buffer is taken as it is)."""
    if not torch.is_tensor(t) or t.dtype not in dtypes or tuple(t.shape) != shape or not t.is_cuda or (dev is not None and t.device != dev):
        raise _lib.HplError('%s: %s must be a %s %s device tensor%s, got %s' % (
            who, name, shape, ' / '.join(str(d) for d in dtypes), '' if dev is None else ' on %s' % dev,
            (tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t)))
    if t.requires_grad:
        raise _lib.HplError('%s has no autograd: %s requires grad' % (who, name))
    return t if t.is_contiguous() else t.contiguous()


def _frames_sizes(who, heights, widths):
    """(heights, widths, prefix) as host lists of a batch of 1 .. 64 frames, or an HplError."""
    try:
        hh, ww = [int(h) for h in heights], [int(w) for w in widths]
    except (TypeError, ValueError):
        hh, ww = [], [0]
    if len(hh) != len(ww) or not 1 <= len(hh) <= 64 or any(not 0 <= v < 2 ** 31 for v in hh + ww):
        raise _lib.HplError('%s: heights and widths hold the sizes (>= 0) of the same 1 .. 64 frames, got %r and %r' % (who, heights, widths))
    pp = [0]
    for h, w in zip(hh, ww):
        pp.append(pp[-1] + h * w)
    return hh, ww, pp


def _frames_outputs(who, out, N, B, dev):
    """(out_pc1, ld, out_pc2, ld, pixel, counts) of a frames call; out: None or a pair of (3, N) float32 tensors with unit stride
    along the pixels (rows may be views of a wider buffer)."""
    if out is None:
        out = (torch.empty((3, N), dtype=torch.float32, device=dev), torch.empty((3, N), dtype=torch.float32, device=dev))
    if not isinstance(out, (list, tuple)) or len(out) != 2 or not (_soa_ok(out[0], N, dev) and _soa_ok(out[1], N, dev)):
        raise _lib.HplError('%s: out must be a pair of (3, %d) float32 tensors on %s with unit stride along the pixels' % (who, N, dev))
    pixel = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev) if N == 0 else torch.empty(B, dtype=torch.int32, device=dev)
    return out[0], _soa_ld(out[0], N), out[1], _soa_ld(out[1], N), pixel, counts


def _frames_room(who, lib, B, N, dev):
    return _room(who, dev, lib.hpl_frames_workspace_bytes(B, N),
                 '%d frames of %d pixels together are outside the limits (64 frames, N < 2^31 / 3)', B, N)


_U16 = (torch.uint16, torch.int16)          # (the same bits: a PNG's raw values)


def frames_from_kitti(disp1, disp2, flow, P, heights, widths, baseline=0.54, out=None):
    """hpl_frames_from_kitti on the current stream: the corresponding clouds of a batch of KITTI scene-flow
    frames from their raw PNG values, as the reference's process_kitti.py computes them, bit for bit.  disp1, disp2 (N,) uint16
    (or int16 of the same bits) device tensors: the packed disp_occ_0 / disp_occ_1 values of B <= 64 frames of heights[b] x
    widths[b] pixels, row-major, one frame behind the other; flow (N, 3) uint16: the flow_occ values (u, v, mask); P: B (3, 4)
    or (12,) P_rect_02 matrices (host, float32 values); baseline in metres.
    -> (pc1 (3, N) float32, pc2 (3, N), pixel (N,) int32, counts (B,) int32): frame b's valid correspondences are columns
    prefix[b] .. prefix[b] + counts[b] (prefix = the running sum of heights * widths) in ascending pixel index, pixel their
    i * width + j; the rest of a frame's range is 0 (pixel: -1).  out: a pair of (3, N) float32 tensors with unit stride along
    the pixels that take pc1 and pc2; they must not overlap the inputs.  No autograd, no host synchronisation, no read-back."""
    import numpy as np
    who = 'frames_from_kitti'
    hh, ww, pp = _frames_sizes(who, heights, widths)
    B, N = len(hh), pp[-1]
    disp1 = _frames_plane(who, 'disp1', disp1, _U16, (N,), None)
    dev = disp1.device
    disp2 = _frames_plane(who, 'disp2', disp2, _U16, (N,), dev)
    flow = _frames_plane(who, 'flow', flow, _U16, (N, 3), dev)
    try:
        Pm = np.ascontiguousarray(np.asarray([np.asarray(p, dtype=np.float32).reshape(12) for p in P], dtype=np.float32))
    except (TypeError, ValueError):
        Pm = np.zeros((0, 12), np.float32)
    if Pm.shape != (B, 12):
        raise _lib.HplError('%s: P holds the (3, 4) P_rect_02 of each of the %d frames' % (who, B))
    o1, ld1, o2, ld2, pixel, counts = _frames_outputs(who, out, N, B, dev)
    lib = _lib.load()
    ws, st = _frames_room(who, lib, B, N, dev)
    check(lib.hpl_frames_from_kitti(disp1.data_ptr(), disp2.data_ptr(), flow.data_ptr(), B, (ctypes.c_int32 * B)(*hh),
                                    (ctypes.c_int32 * B)(*ww), _c_prefix(pp),
                                    Pm.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(baseline), o1.data_ptr(), ld1,
                                    o2.data_ptr(), ld2, pixel.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), st),
          'hpl_frames_from_kitti')
    return o1, o2, pixel, counts


def frames_from_ft3d(disp, dchange, flow, occ1, occ2, heights, widths, f=-1050.0, cx=479.5, cy=269.5, near=None, out=None):
    """hpl_frames_from_ft3d on the current stream: the corresponding clouds of a batch of FlyingThings3D-subset
    frames as the reference's process_flyingthings3d_subset.py computes them, bit for bit (x and z keep the sign the reference
    SAVES; its dataset reader flips them on load, and so does data.FlyingThings3DRaw).  disp, dchange (N,) float32 packed device
    tensors: disparity and disparity change of B <= 64 frames of heights[b] x widths[b] pixels; flow (N, 2) float32; occ1, occ2
    (N,) uint8: the disparity and flow occlusion masks (0 = visible).  near: None, or the near cut of --only_save_near_pts
    (-35.): a correspondence is kept only when z1 > near and z2 > near.
    -> (pc1, pc2, pixel, counts) and out as frames_from_kitti."""
    who = 'frames_from_ft3d'
    hh, ww, pp = _frames_sizes(who, heights, widths)
    B, N = len(hh), pp[-1]
    disp = _frames_plane(who, 'disp', disp, (torch.float32,), (N,), None)
    dev = disp.device
    dchange = _frames_plane(who, 'dchange', dchange, (torch.float32,), (N,), dev)
    flow = _frames_plane(who, 'flow', flow, (torch.float32,), (N, 2), dev)
    occ1 = _frames_plane(who, 'occ1', occ1, (torch.uint8,), (N,), dev)
    occ2 = _frames_plane(who, 'occ2', occ2, (torch.uint8,), (N,), dev)
    if near is not None and not float(near) == float(near):
        raise _lib.HplError('%s: near = %r (None or a number)' % (who, near))
    o1, ld1, o2, ld2, pixel, counts = _frames_outputs(who, out, N, B, dev)
    lib = _lib.load()
    ws, st = _frames_room(who, lib, B, N, dev)
    check(lib.hpl_frames_from_ft3d(disp.data_ptr(), dchange.data_ptr(), flow.data_ptr(), occ1.data_ptr(), occ2.data_ptr(), B,
                                   (ctypes.c_int32 * B)(*hh), (ctypes.c_int32 * B)(*ww), _c_prefix(pp), float(f),
                                   float(cx), float(cy), 0 if near is None else 1, 0.0 if near is None else float(near),
                                   o1.data_ptr(), ld1, o2.data_ptr(), ld2, pixel.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                   ws.numel(), st), 'hpl_frames_from_ft3d')
    return o1, o2, pixel, counts


def png_unfilter(raw, height, stride, bpp):
    """hpl_png_unfilter (host only): `raw`, the inflated IDAT stream of a non-interlaced PNG -- height rows of a filter byte and
    stride - 1 data bytes --, with the row filters undone -> numpy uint8 (height, stride - 1)."""
    import numpy as np
    if len(raw) != height * stride:
        raise _lib.HplError('png_unfilter: %d bytes for %d rows of %d' % (len(raw), height, stride))
    rows = np.frombuffer(raw, dtype=np.uint8).copy().reshape(height, stride)
    check(_lib.load().hpl_png_unfilter(rows.ctypes.data, height, stride, bpp), 'hpl_png_unfilter')
    return rows[:, 1:]


# --------------------------------------------------------------------------- maps from clouds
_RENDER_LIMITS = '%d frames of %d pixels together are outside the limits (64 frames, M < 2^31 / 3)'


def _render_shapes(who, n, prefix, heights, widths, footprint):
    """(point prefix, heights, widths, pixel prefix) of B clouds with one frame each, and the footprint checked."""
    pp = _prefix(prefix, n, who)
    hh, ww, qq = _frames_sizes(who, heights, widths)
    if len(hh) != len(pp) - 1:
        raise _lib.HplError('%s: %d clouds but %d frame sizes' % (who, len(pp) - 1, len(hh)))
    _int_in(who, 'footprint', footprint, 0, 4)
    return pp, hh, ww, qq


def _host_rows(who, name, rows, B, width, what):
    """B host rows of `width` float32 values as a contiguous numpy array."""
    import numpy as np
    try:
        m = np.ascontiguousarray(np.asarray([np.asarray(r, dtype=np.float32).reshape(width) for r in rows], dtype=np.float32))
    except (TypeError, ValueError):
        m = np.zeros((0, width), np.float32)
    if m.shape != (B, width):
        raise _lib.HplError('%s: %s holds %s of each of the %d frames' % (who, name, what, B))
    return m


def render_maps(pc, camera, heights, widths, attrs=None, footprint=0, rel_tol=0.0, abs_tol=0.0, near=1e-3, prefix=None, out=None):
    """hpl_render_maps on the current stream: the clouds of a ragged batch splatted into one image each through a
    z-buffer.  pc (3, N) float32 (rows may be views of a wider buffer); prefix (host sequence of B + 1 ints from 0 to N): B <= 64
    clouds; camera: B host rows (f, cx, cy, constx, consty, constz), the cameras of the 2D metrics; heights, widths: the B image
    sizes, image b owning pixels qprefix[b] .. qprefix[b + 1] (the running sum of heights * widths, M in all) of every per-pixel
    output, row-major; attrs (C, N) float32, C <= 8, or None: channels that ride with the points.  A point is projectable when
    it is finite with zc = Z + constz >= near, inside when its pixel (rintf of the projection, ties to even) lies in the image;
    every inside point offers (zc, local index) to the (2 footprint + 1)^2 pixels around its own and a pixel keeps the nearest,
    ties to the smaller index.
    -> (pixel_of (N,) int32: i * width + j or -1, winner (M,) int32: the local index of the pixel's point or -1, depth (M,)
    float32: its zc or 0, attr_map (C, M) float32 or None: its channels or 0, visible (N,) uint8: 1 when the point is inside and
    zc <= zmin * (1 + rel_tol) + abs_tol with zmin the depth at its own pixel, stats (B, 4) int32 = (points inside, pixels
    covered, points visible, points not projectable)).  out: a (C, M) float32 tensor with unit stride along the pixels that takes
    attr_map; it must not overlap pc or attrs.  The same bits for a cloud alone and in any batch.  No autograd, no host
    synchronisation, no read-back."""
    who = 'render_maps'
    pc, pc_ld = _soa3(pc, 'pc', who)
    N, dev = pc.shape[1], pc.device
    attrs, C, attr_ld = _attrs(who, attrs, N, dev)
    pp, hh, ww, qq = _render_shapes(who, N, prefix, heights, widths, footprint)
    B, M = len(hh), qq[-1]
    cam = _host_rows(who, 'camera', camera, B, 6, 'the (f, cx, cy, constx, consty, constz)')
    rel_tol, abs_tol = _scalar(who, 'rel_tol', rel_tol, zero_ok=True), _scalar(who, 'abs_tol', abs_tol, zero_ok=True)
    near = _scalar(who, 'near', near)
    attr_map, map_ld = None, max(M, 1)
    if C:
        attr_map = torch.empty((C, M), dtype=torch.float32, device=dev) if out is None else out
        if not torch.is_tensor(attr_map) or tuple(attr_map.shape) != (C, M) or attr_map.dtype != torch.float32 or \
                attr_map.device != dev or attr_map.requires_grad or (M > 1 and attr_map.stride(1) != 1) or \
                (C > 1 and attr_map.stride(0) < max(M, 1)):
            raise _lib.HplError('%s: out must be a (%d, %d) float32 tensor on %s with unit stride along the pixels' % (who, C, M, dev))
        map_ld = max(M, 1) if C == 1 or attr_map.is_contiguous() else attr_map.stride(0)
    elif out is not None:
        raise _lib.HplError('%s: out takes the attribute map, and there are no attrs' % who)
    pixel_of = torch.empty(N, dtype=torch.int32, device=dev)
    winner = torch.empty(M, dtype=torch.int32, device=dev)
    depth = torch.empty(M, dtype=torch.float32, device=dev)
    visible = torch.empty(N, dtype=torch.uint8, device=dev)
    if N == 0 and M == 0:                        # nothing to launch
        return pixel_of, winner, depth, attr_map, visible, torch.zeros((B, 4), dtype=torch.int32, device=dev)
    stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
    lib = _lib.load()
    ws, st = _room(who, dev, lib.hpl_render_workspace_bytes(B, M), _RENDER_LIMITS, B, M)
    check(lib.hpl_render_maps(pc.data_ptr(), pc_ld, ptr(attrs), attr_ld, C, B, _c_prefix(pp),
                              cam.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int32 * B)(*hh),
                              (ctypes.c_int32 * B)(*ww), _c_prefix(qq), footprint, rel_tol, abs_tol, near, pixel_of.data_ptr(),
                              winner.data_ptr(), depth.data_ptr(), ptr(attr_map), map_ld, visible.data_ptr(), stats.data_ptr(),
                              ws.data_ptr(), ws.numel(), st), 'hpl_render_maps')
    return pixel_of, winner, depth, attr_map, visible, stats


def maps_to_kitti(pc1, pc2, P, heights, widths, baseline=0.54, footprint=0, prefix=None, out=None):
    """hpl_maps_to_kitti on the current stream: the raw values of KITTI's three scene-flow PNGs from the two
    clouds of a ragged batch of frames -- the inverse of frames_from_kitti.  pc1 (3, N) float32: the clouds of frame 1; pc2
    (3, N): their partners pc1 + flow, point for point; prefix (host sequence of B + 1 ints from 0 to N); P: B (3, 4) or (12,)
    P_rect_02 matrices (host); heights, widths: the B image sizes (M pixels in all); baseline in metres.  The z-buffer of
    render_maps over pc1 (camera (-P00, P02, P12, P03, P13, P23), near 1e-3) picks every pixel's point.
    -> (disp1 (M,) uint16: disparity of frame 1, disp2 (M,) uint16: disparity of the partner, flow (M, 3) uint16: (u, v, 1)), 0
    where a pixel has no point.  With footprint 0 a batch from frames_from_kitti comes back as its raw maps at every valid
    pixel.  out: a triple of contiguous uint16 tensors of those shapes.  No autograd, no host synchronisation, no read-back."""
    who = 'maps_to_kitti'
    pc1, ld1 = _soa3(pc1, 'pc1', who)
    N, dev = pc1.shape[1], pc1.device
    pc2, ld2 = _soa3(pc2, 'pc2', who)
    if pc2.shape[1] != N or pc2.device != dev:
        raise _lib.HplError('%s: pc2 must be a (3, %d) tensor on %s like pc1' % (who, N, dev))
    pp, hh, ww, qq = _render_shapes(who, N, prefix, heights, widths, footprint)
    B, M = len(hh), qq[-1]
    Pm = _host_rows(who, 'P', P, B, 12, 'the (3, 4) P_rect_02')
    if out is None:
        out = (torch.empty(M, dtype=torch.uint16, device=dev), torch.empty(M, dtype=torch.uint16, device=dev),
               torch.empty((M, 3), dtype=torch.uint16, device=dev))
    if not isinstance(out, (list, tuple)) or len(out) != 3 or any(
            not torch.is_tensor(o) or o.dtype not in _U16 or o.device != dev or not o.is_contiguous() or tuple(o.shape) != s
            for o, s in zip(out, ((M,), (M,), (M, 3)))):
        raise _lib.HplError('%s: out must be contiguous uint16 tensors of shapes (%d,), (%d,), (%d, 3) on %s' % (who, M, M, M, dev))
    lib = _lib.load()
    ws, st = _room(who, dev, lib.hpl_render_workspace_bytes(B, M), _RENDER_LIMITS, B, M)
    check(lib.hpl_maps_to_kitti(pc1.data_ptr(), ld1, pc2.data_ptr(), ld2, B, _c_prefix(pp), (ctypes.c_int32 * B)(*hh),
                                (ctypes.c_int32 * B)(*ww), _c_prefix(qq), Pm.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                float(baseline), footprint, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                ws.data_ptr(), ws.numel(), st), 'hpl_maps_to_kitti')
    return tuple(out)


# --------------------------------------------------------------------------- self-supervised loss
def selfsup_loss(pc1, flow, pc2, k=8, w_chamfer=1.0, w_smooth=1.0, prefix1=None, prefix2=None, need_grad=True,
                 return_neighbors=False, out=None):
    """hpl_selfsup_loss on the current stream: per pair the Chamfer distance between the warped cloud
    pc1 + flow and pc2 (both directions, squared distances to the nearest point, means over the points) plus the smoothness
    of the flow over pc1's k-nearest-neighbour graph (mean over the points of the mean |f_i - f_n|^2 over a point's k nearest
    other points), L = w_chamfer (C12 + C21) + w_smooth S, and dL/dflow with the neighbour assignments held constant.  pc1
    (3, N1), pc2 (3, N2) float32; flow (3, N1) or [N1, 3] float32 of any strides (read in place, as ops.rigid_fit reads it).
    k 1 .. 8, or 0 with w_smooth = 0 (no graph search); the weights finite and >= 0.  prefix1 / prefix2 (host sequences of B + 1
    ints from 0 to N1 / N2): B <= 64 pairs, each with its own loss.
    -> (loss (B, 4) = (L, C12, C21, S), dflow [N1, 3] or None with need_grad=False[, nn12 (N1,), nn21 (N2,), nbr (k, N1) int32
    into the packed clouds, -1 where absent]).  out: a contiguous [N1, 3] float32 tensor that takes dflow (it must not overlap an
    input).  Float64 sums in a fixed order: the same bits for a pair alone and in any batch.  This is the raw op (a tensor that
    requires grad raises HplError; SelfSupLossFn is the autograd form); no host synchronisation, no read-back."""
    who = 'selfsup_loss'
    _int_in(who, 'k', k, 0, 8)
    try:
        w_chamfer, w_smooth = float(w_chamfer), float(w_smooth)
    except (TypeError, ValueError):
        w_chamfer = w_smooth = float('nan')
    if not (0 <= w_chamfer < float('inf')) or not (0 <= w_smooth < float('inf')):
        raise _lib.HplError('%s: the weights must be finite and >= 0, got %r / %r' % (who, w_chamfer, w_smooth))
    if k == 0 and w_smooth != 0:
        raise _lib.HplError('%s: k = 0 goes with w_smooth = 0' % who)
    pc1, ld1 = _soa3(pc1, 'pc1', who)
    pc2, ld2 = _soa3(pc2, 'pc2', who)
    N1, N2, dev = pc1.shape[1], pc2.shape[1], pc1.device
    if pc2.device != dev:
        raise _lib.HplError('%s: pc1 on %s, pc2 on %s' % (who, dev, pc2.device))
    flow = _flow_view(flow, N1, dev, who, '%s is the raw op: flow requires grad (SelfSupLossFn is the autograd form)' % who)
    p1, p2 = _prefix(prefix1, N1, who, 'prefix1'), _prefix(prefix2, N2, who, 'prefix2')
    if len(p1) != len(p2):
        raise _lib.HplError('%s: prefix1 lists %d pairs, prefix2 %d' % (who, len(p1) - 1, len(p2) - 1))
    B = len(p1) - 1
    dflow = None
    if out is not None:
        if not need_grad or not torch.is_tensor(out) or tuple(out.shape) != (N1, 3) or out.dtype != torch.float32 or \
                out.device != dev or not out.is_contiguous() or out.requires_grad:
            raise _lib.HplError('%s: out (with need_grad) must be a contiguous (%d, 3) float32 tensor on %s' % (who, N1, dev))
        dflow = out
    elif need_grad:
        dflow = torch.empty((N1, 3), dtype=torch.float32, device=dev)
    nn12 = nn21 = nbr = None
    if return_neighbors:
        nn12 = torch.full((N1,), -1, dtype=torch.int32, device=dev)
        nn21 = torch.full((N2,), -1, dtype=torch.int32, device=dev)
        nbr = torch.full((k, N1), -1, dtype=torch.int32, device=dev)
    if N1 == 0:                                  # nothing to launch: every component of every pair is 0
        loss = torch.zeros((B, 4), dtype=torch.float32, device=dev)
    else:
        lib = _lib.load()
        loss = torch.empty((B, 4), dtype=torch.float32, device=dev)
        ws, st = _room(who, dev, lib.hpl_selfsup_loss_workspace_bytes(B, N1, N2, k), '%d pairs of %d / %d points together, k = %d are '
                       'outside the limits (64 pairs, counts < 2^31 / 3, k N1 < 2^31)', B, N1, N2, k)
        check(lib.hpl_selfsup_loss(pc1.data_ptr(), ld1, flow.data_ptr(), flow.stride(0), flow.stride(1), pc2.data_ptr(), ld2, B,
                                   _c_prefix(p1), _c_prefix(p2), k, w_chamfer, w_smooth,
                                   loss.data_ptr(), ptr(dflow), ptr(nn12), ptr(nn21), ptr(nbr) if k > 0 else None, ws.data_ptr(),
                                   ws.numel(), st), 'hpl_selfsup_loss')
    return (loss, dflow, nn12, nn21, nbr) if return_neighbors else (loss, dflow)


class SelfSupLossFn(torch.autograd.Function):
    """ops.selfsup_loss with autograd: forward computes the loss and dL/dflow in ONE call; backward hands back that gradient
    scaled by each pair's upstream gradient.  (flow (3, N1) or [N1, 3], pc1, pc2, k, w_chamfer, w_smooth, prefix1, prefix2) ->
    (L (B,), components (B, 4), not differentiable).  pc1 and pc2 get no gradient: the neighbour assignments are constants."""

    @staticmethod
    def forward(ctx, flow, pc1, pc2, k, w_chamfer, w_smooth, prefix1, prefix2):
        loss, dflow = selfsup_loss(pc1.detach(), flow.detach(), pc2.detach(), k, w_chamfer, w_smooth, prefix1, prefix2)
        N1 = dflow.shape[0]
        B = loss.shape[0]
        pair = None
        if B > 1:                                # the pair of every point (host numbers: no read-back)
            counts = [b - a for a, b in zip(prefix1, prefix1[1:])]
            pair = torch.repeat_interleave(torch.arange(B, device=dflow.device),
                                           torch.tensor(counts, device=dflow.device), output_size=N1)
        ctx.rows = tuple(flow.shape) != (3, N1)  # flow came point-major
        ctx.pair = pair
        ctx.save_for_backward(dflow)
        comps = loss.clone()
        ctx.mark_non_differentiable(comps)
        return loss[:, 0].clone(), comps

    @staticmethod
    def backward(ctx, gL, _):
        dflow, = ctx.saved_tensors
        g = dflow * (gL[0] if ctx.pair is None else gL[ctx.pair][:, None])
        return (g if ctx.rows else g.t()), None, None, None, None, None, None, None


# --------------------------------------------------------------------------- data transforms
def transform_capacity(M, num_points):
    """The most rows hpl_transform_pair emits for M points: min(num_points, M), or M when num_points <= 0."""
    cap = ctypes.c_int64()
    check(_lib.load().hpl_transform_capacity(int(M), int(num_points), ctypes.byref(cap)), 'hpl_transform_capacity')
    return cap.value


class TransformRunner(object):
    """hpl_transform_pair for one transform object (data.DeviceAugmentation / DeviceProcessData).

    The work runs on a stream of its own: the count read-back then waits for this transform's copies and launches only, not
    for whatever the caller's stream holds (LatticePipeline calls its source under the lattice stream).  The caller's
    current stream waits on the transform's event, and the outputs are record_stream-ed to it.  Raw numpy clouds reach the
    device through a grow-only, double-buffered pinned stage (a slot is refilled only after the event of the copy that read
    it); the parameters through a pinned stage of their own; the device copy of the clouds and the workspace are grow-only
    and stream-ordered.  `last_counts` = (valid points, emitted rows) of the last call."""

    PSIZE = ctypes.sizeof(_lib.TransformParams)

    def __init__(self, device='cuda'):
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.stream = torch.cuda.Stream(self.device)
        self._host = [None, None]
        self._pstage = [torch.empty(self.PSIZE, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._ev = [None, None]
        self._slot = 0
        self._dev_in = None
        self._ws = None
        self._counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._counts_host = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        self.last_counts = None

    @staticmethod
    def _grow(buf, n, make):
        if buf is None or buf.numel() < n:
            return make(max(n, int(1.25 * buf.numel()) if buf is not None else n))
        return buf

    def _stage_numpy(self, pc1, pc2, M, slot):
        ev = self._ev[slot]
        if ev is not None:
            ev.synchronize()                     # the copy that last read this slot has run
        self._host[slot] = self._grow(self._host[slot], 6 * M,
                                      lambda n: torch.empty(n, dtype=torch.float32, pin_memory=True))
        h = self._host[slot][:6 * M].numpy()
        h[:3 * M].reshape(M, 3)[:] = pc1[:, :3]
        h[3 * M:].reshape(M, 3)[:] = pc2[:, :3]
        self._dev_in = self._grow(self._dev_in, 6 * M,
                                  lambda n: torch.empty(n, dtype=torch.float32, device=self.device))
        self._dev_in[:6 * M].copy_(self._host[slot][:6 * M], non_blocking=True)
        if self._ev[slot] is None:
            self._ev[slot] = torch.cuda.Event()
        self._ev[slot].record(self.stream)
        return self._dev_in[:3 * M], self._dev_in[3 * M:6 * M]

    def run(self, pc1, pc2, params, jitter1=None, jitter2=None, sel1=None, sel2=None):
        """pc1, pc2: the raw clouds, numpy (M, >= 3) arrays or (M, 3) contiguous float32 device tensors; params: a
        _lib.TransformParams.  jitter1 / jitter2 / sel1 / sel2: the test hook of hpl_transform_pair (device tensors: (M, 3)
        float32, int32 indices).  -> (pc1, pc2, sf) contiguous (3, k) float32 device tensors, or (None, None, None) when
        the pair is rejected."""
        M = int(pc1.shape[0])
        if int(pc2.shape[0]) != M:
            raise _lib.HplError('transform: the clouds have %d and %d points (the reference pairs them point by point)'
                                % (M, int(pc2.shape[0])))
        lib = _lib.load()
        caller = torch.cuda.current_stream(self.device)
        s = self.stream
        cap = transform_capacity(M, params.num_points)
        hooks = (jitter1, jitter2, sel1, sel2)
        for t, dt in zip(hooks, (torch.float32, torch.float32, torch.int32, torch.int32)):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != self.device):
                raise _lib.HplError('transform: hook arrays are contiguous %s tensors on %s' % (dt, self.device))
        for t in (jitter1, jitter2):
            if t is not None and t.numel() != 3 * M:
                raise _lib.HplError('transform: a jitter hook holds (M, 3) = %d values, got %d' % (3 * M, t.numel()))
        if sel1 is not None and (not 1 <= sel1.numel() <= cap or (sel2 is not None and sel2.numel() != sel1.numel())):
            raise _lib.HplError('transform: selection hooks hold 1 .. %d indices each, got %d and %s'
                                % (cap, sel1.numel(), None if sel2 is None else sel2.numel()))
        with torch.cuda.stream(s):
            if isinstance(pc1, torch.Tensor):
                for t in (pc1, pc2):
                    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous() or t.device != self.device:
                        raise _lib.HplError('transform: device clouds are contiguous (M, 3) float32 tensors on %s' % self.device)
                s.wait_stream(caller)            # the caller may have produced them
                d1, d2 = pc1, pc2
            else:
                if pc1.ndim != 2 or pc1.shape[1] < 3 or pc2.ndim != 2 or pc2.shape[1] < 3:
                    raise _lib.HplError('transform: numpy clouds are (M, >= 3), got %s and %s' % (pc1.shape, pc2.shape))
                if any(t is not None for t in hooks):
                    s.wait_stream(caller)
                self._slot ^= 1
                d1, d2 = self._stage_numpy(pc1, pc2, M, self._slot)
            wsb = lib.hpl_transform_workspace_bytes(M)
            self._ws = self._grow(self._ws, wsb, lambda n: torch.empty(n, dtype=torch.uint8, device=self.device))
            out = torch.empty(9 * cap, dtype=torch.float32, device=self.device)
            pstage = self._pstage[self._slot]
            ctypes.memmove(pstage.data_ptr(), ctypes.byref(params), self.PSIZE)
            n_sel = int(sel1.numel()) if sel1 is not None else 0
            check(lib.hpl_transform_pair(ptr(d1), ptr(d2), M, pstage.data_ptr(), ptr(jitter1), ptr(jitter2), ptr(sel1),
                                         ptr(sel2), n_sel, ptr(out), ptr(out[3 * cap:]), ptr(out[6 * cap:]), cap,
                                         ptr(self._counts), ptr(self._ws), wsb, s.cuda_stream), 'hpl_transform_pair')
            self._counts_host.copy_(self._counts, non_blocking=True)
            done = torch.cuda.Event()
            done.record(s)
        done.synchronize()                       # the one read-back: (valid, emitted)
        V, k = self._counts_host.tolist()
        self.last_counts = (V, k)
        caller.wait_event(done)
        out.record_stream(caller)
        if k <= 0:
            return None, None, None
        return tuple(out[o * cap:o * cap + 3 * k].view(3, k) for o in (0, 3, 6))


def round_up(x, m):
    return (x + m - 1) // m * m


def weight_relayout(W, R, Q, F, sr, sq, sf, base=0, fmap=None):
    """-> Wt [roundup(F*R, 32), roundup(Q, 4)] with Wt[(fmap[f]*R + r), q] = W.flat[base + r*sr + q*sq + f*sf]."""
    k_rows = round_up(F * R, 32)
    ldw = round_up(Q, 4)
    Wt = torch.empty((k_rows, ldw), dtype=torch.float32, device=W.device)
    check(_lib.load().hpl_weight_relayout(ptr(W), base, R, Q, F, sr, sq, sf, ptr(fmap), ptr(Wt), k_rows, ldw,
                                          stream()), 'hpl_weight_relayout')
    return Wt


#: HPL_FOLD_UP=0: the inference forward keeps the Up layers' trailing bias-only 1x1 convs as launches of their own (the
#: program and the Python path of before the fold); read once, for A/B runs
FOLD_UP = os.environ.get('HPL_FOLD_UP', '1') != '0'


def weight_fold(W, F, up0, up_w, Wb, bias_a=None, bias_b=None, ones_col=-1, own_bias=None, dense_bias=False, out=None,
                out_bias=None):
    """hpl_weight_fold: the consumer weight W ((O, C, F, 1) or (O, C, 1), the parameter's own layout) with its columns
    [up0, up0 + up_w) multiplied by the producer's bias-only 1x1 Wb ((up_w, Cb, 1[, 1])), the producer's bias bias_a + bias_b
    carried by a four-column ones part inserted at column ones_col (>= 0) or, dense_bias (F == 1), by the folded bias
    own_bias + W[:, up] b.  Sums in double, rounded once; deterministic.  -> (folded weight, folded bias or None)."""
    O = W.shape[0]
    C = W.numel() // (O * F)
    Cb = Wb.numel() // up_w
    if Wb.shape[0] != up_w or W.dtype is not torch.float32 or Wb.dtype is not torch.float32 or not (W.is_contiguous() and Wb.is_contiguous()):
        raise _lib.HplError('weight_fold: contiguous float32 weights, the 1x1 with %d output channels; got %s / %s'
                            % (up_w, tuple(W.shape), tuple(Wb.shape)))
    for b in (bias_a, bias_b):
        if b is not None and (b.numel() != up_w or not b.is_contiguous()):
            raise _lib.HplError('weight_fold: a bias of %d entries, got %s' % (up_w, tuple(b.shape)))
    if own_bias is not None and (own_bias.numel() != O or not own_bias.is_contiguous()):
        raise _lib.HplError('weight_fold: the consumer\'s bias has %d entries, got %s' % (O, tuple(own_bias.shape)))
    Cout = C - up_w + Cb + (4 if ones_col >= 0 else 0)
    shape = (O, Cout) + tuple(W.shape[2:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=W.device)
    if dense_bias and out_bias is None:
        out_bias = torch.empty((O,), dtype=torch.float32, device=W.device)
    if tuple(out.shape) != shape or not out.is_contiguous() or (out_bias is not None and out_bias.numel() != O):
        raise _lib.HplError('weight_fold: the folded weight is %s, got %s' % (shape, tuple(out.shape)))
    check(_lib.load().hpl_weight_fold(ptr(W), O, C, F, up0, up_w, ptr(Wb), Cb, ptr(bias_a), ptr(bias_b), ones_col, ptr(out),
                                      out.numel(), ptr(own_bias), ptr(out_bias), stream()), 'hpl_weight_fold')
    return out, out_bias


class FoldedWeight(object):
    """A consumer's weight with the producer's bias-only 1x1 folded in (weight_fold), kept current: `weight` (and `bias` of a
    folded dense layer) are allocated once and rewritten IN PLACE whenever one of the parameters they are made of has a new
    version (or invalidate_weight_cache() ran), so the images made of them -- the native plan's bank, _cached_relayout of the
    Python path -- refresh the way they do for a parameter.  The native plan and the Python path share one of these per
    consumer (flownet._FlowNetBase.up_fold keeps them with the model): the same tensor, hence the same launches on the same bits."""

    def __init__(self, W, F, up0, up_w, Wb, bias_a, bias_b, ones_col, own_bias, dense_bias):
        self.src = (W, Wb, bias_a, bias_b, own_bias)
        self.args = (F, up0, up_w, ones_col, dense_bias)
        self.ptrs = self._ptrs()
        self._keep = [None if p is None else p.detach() for p in self.src]      # the storages stay: their addresses are not reused
        O = W.shape[0]
        Cout = W.numel() // (O * F) - up_w + Wb.numel() // up_w + (4 if ones_col >= 0 else 0)
        self.weight = torch.empty((O, Cout) + tuple(W.shape[2:]), dtype=torch.float32, device=W.device)
        self.bias = torch.empty((O,), dtype=torch.float32, device=W.device) if dense_bias else None
        self._sig = None
        self._ev = self._stream = None

    def _ptrs(self):
        return tuple(None if p is None else p.data_ptr() for p in self.src)

    def made_of(self, src, args):
        return args == self.args and all(a is b for a, b in zip(src, self.src)) and self._ptrs() == self.ptrs

    def ensure(self):
        """Current values on the current stream -> self."""
        sig = (weight_epoch(),) + tuple(None if p is None else p._version for p in self.src)
        if sig != self._sig:
            F, up0, up_w, ones_col, dense_bias = self.args
            W, Wb, ba, bb, own = [None if p is None else p.detach() for p in self.src]
            with torch.no_grad():
                self.weight, self.bias = weight_fold(W, F, up0, up_w, Wb, ba, bb, ones_col, own, dense_bias, out=self.weight,
                                                     out_bias=self.bias)
            if self._sig is not None:                 # rewritten through its pointer: tell the caches keyed on the version
                torch.autograd.graph.increment_version(self.weight)
                if self.bias is not None:
                    torch.autograd.graph.increment_version(self.bias)
            self._sig = sig
            self._ev = torch.cuda.Event()
            self._ev.record()
            self._stream = stream()
        elif self._ev is not None and stream() != self._stream:
            if self._ev.query():
                self._ev = None
            else:
                torch.cuda.current_stream().wait_event(self._ev)
        return self


class SplitW(object):
    """Split image of a weight image: `planes` uint8 [P, k_rows/8 * ldw * 16] in MFMA B-fragment order -- P = 3: bf16 planes
    hi / mid / lo with Wt == hi + mid + lo exactly (hpl_weight_split3); P = 2: fp16 planes hi / lo of Wt * s, s the power of
    two that puts the image's largest magnitude `amax` (float32 [1], device) into [2^14, 2^15) (hpl_weight_split2h)."""
    __slots__ = ('planes', 'amax', 'P')

    def __init__(self, planes, amax, P):
        self.planes, self.amax, self.P = planes, amax, P

    def rows_from(self, k0, ldw):
        """The same image from row k0 (a multiple of 8) on: k-blocks of 8 rows, 16 bytes per column."""
        return SplitW(self.planes[:, (k0 // 8) * ldw * 16:], self.amax, self.P)


def weight_split3(Wt, out=None, planes=None):
    """fp32 weight image [k_rows (multiple of 8), ldw] -> SplitW: the operand of the split-operand gather-GEMM (gconv_raw
    Wt3=...); planes = 2 / 3 (default: SPLIT_PLANES, i.e. HPL_MATH); out: a SplitW of the same image to refresh."""
    k_rows, ldw = Wt.shape
    if k_rows % 8 or not Wt.is_contiguous():
        raise _lib.HplError('weight_split3: image must be contiguous with a multiple of 8 rows, got %s' % (tuple(Wt.shape),))
    P = out.P if out is not None else (planes or SPLIT_PLANES)
    if out is None:
        out = SplitW(torch.empty((P, k_rows // 8 * ldw * 16), dtype=torch.uint8, device=Wt.device),
                     torch.zeros(1, dtype=torch.float32, device=Wt.device) if P == 2 else None, P)
    if P == 2:
        check(_lib.load().hpl_weight_split2h(ptr(Wt), k_rows, ldw, ptr(out.planes), out.planes.stride(0), ptr(out.amax), stream()),
              'hpl_weight_split2h')
    else:
        check(_lib.load().hpl_weight_split3(ptr(Wt), k_rows, ldw, ptr(out.planes), out.planes.stride(0), stream()), 'hpl_weight_split3')
    return out


def amax(X, rows=None, cols=None):
    """float32 [1] on the device: the largest magnitude of X[:rows, :cols] (hpl_amax; the scale of a gather-GEMM's fp16-pair
    operands)."""
    p_, ld, r, c = _mat(X, 'amax input')
    out = torch.empty(1, dtype=torch.float32, device=X.device)
    check(_lib.load().hpl_amax(p_, ld, r if rows is None else rows, c if cols is None else cols, ptr(out), stream()), 'hpl_amax')
    return out


def amax_rows(X, rows=None, cols=None):
    """(float32 [1], int32 [1]) on the device: the largest magnitude of X[:rows, :cols] and its range-guard word -- ~bits of the
    smallest non-zero ROW maximum, 0 for an all-zero block (hpl_amax_rows; hpl_gconv_desc.a_guard)."""
    p_, ld, r, c = _mat(X, 'amax input')
    out = torch.empty(1, dtype=torch.float32, device=X.device)
    guard = torch.empty(1, dtype=torch.int32, device=X.device)
    check(_lib.load().hpl_amax_rows(p_, ld, r if rows is None else rows, c if cols is None else cols, ptr(out), ptr(guard), stream()),
          'hpl_amax_rows')
    return out, guard


def _mat(x, what, dev=True):
    """(data_ptr, leading dimension, rows, cols) of a channel-last 2-D float32 device matrix, validated with one
    stride() / shape read (this sits on the host's critical path: ~100 calls per forward).  dev=False (launch queries): any device."""
    st, sh = x.stride(), x.shape
    if len(st) != 2 or x.dtype is not torch.float32 or (dev and not x.is_cuda) or (st[1] != 1 and sh[1] > 1):
        raise _lib.HplError('%s must be a channel-last 2-D float32 device tensor with unit channel stride, '
                            'got shape %s strides %s dtype %s device %s' % (what, tuple(sh), st, x.dtype, x.device))
    return x.data_ptr(), (st[0] if sh[0] > 1 else max(sh[1], st[0])), sh[0], sh[1]


def _gconv_desc(A, nbr, M, C, F, Wt, N, bias, act, res, res_mod, out, scat, scat_c, slope, row_perm, split_k, reg_stride, tiles,
                out2, rows2, Wt3, y_amax, guard, y_guard, guard_trips, query=False):
    """-> (hpl_gconv_desc, out, stream, tensors the descriptor points to) of a gconv_raw call: the one place the descriptor is
    built, for the launch (gconv_raw) and for the query of the instance it takes (gconv_launch_info).  query: the tensors may live on any device -- the selection
    looks at a pointer's null-ness and alignment only --, nothing is launched and no device memory is allocated."""
    dev = not query
    ptr = _addr if query else _lib.ptr
    keep = None           # device scalars made here: they must outlive the launch
    d = GConvDesc()
    d.A, d.lda, d.rows_a, a_cols = _mat(A, 'activation', dev)
    if nbr is not None:
        nst, nsh = nbr.stride(), nbr.shape
        if nbr.dtype is not torch.int32 or len(nsh) != 2 or nsh[0] != F or nsh[1] != M or nst[1] != 1:
            raise _lib.HplError('neighbour table must be int32 [F=%d, M=%d] with unit column stride, got %s %s'
                                % (F, M, tuple(nsh), nbr.dtype))
        d.nbr, d.nbr_stride = ptr(nbr), nst[0]
    elif F != 1:
        if reg_stride <= 0 or (F - 1) * reg_stride + M > d.rows_a:
            raise _lib.HplError('F > 1 needs a neighbour table or a regular stride inside A (F=%d stride=%d M=%d '
                                'rows=%d)' % (F, reg_stride, M, d.rows_a))
        d.reg_stride = reg_stride
    d.M, d.C, d.F = M, C, F
    if C > a_cols:
        raise _lib.HplError('C=%d exceeds the %d channels of A' % (C, a_cols))
    wsh = Wt.shape
    if wsh[0] < F * C or wsh[1] < N or not Wt.is_contiguous():
        raise _lib.HplError('Wt %s too small for K=%d N=%d' % (tuple(wsh), F * C, N))
    d.Wt, d.ldw, d.N = ptr(Wt), wsh[1], N
    d.w_rows = min(wsh[0], round_up(F * C, 32))     # rows past the image read as zero
    d.act, d.slope = act, slope
    if Wt3 is not None:           # weight_split3 of the image Wt is a row range of (same first row)
        if Wt3.P == 3:
            d.Wt3, d.wt3_plane_stride, d.wt3_planes = ptr(Wt3.planes), Wt3.planes.stride(0), 3
        elif scat is None and split3_maybe(M, C, F, N):
            # fp16 pairs: the launch scales A by its largest magnitude (csrc/gconv_common.h split3_maybe: launches that cannot
            # qualify skip the reduction and run on the fp32 MFMA)
            if query:             # (the reductions are launches: a query stands a non-null scalar in for their results)
                d.a_amax = _QUERY_PTR
                if guard:
                    d.a_guard = _QUERY_PTR
            elif guard:
                keep = amax_rows(A, cols=C)
                d.a_amax, d.a_guard = ptr(keep[0]), ptr(keep[1])
                if guard_trips is not None:
                    d.guard_trips = ptr(guard_trips)
            else:
                keep = amax(A, cols=C)
                d.a_amax = ptr(keep)
            d.Wt3, d.wt3_plane_stride, d.wt3_planes = ptr(Wt3.planes), Wt3.planes.stride(0), 2
            d.w_amax = ptr(Wt3.amax)
    if bias is not None:
        d.bias = ptr(bias)
    if res is not None:
        d.res, d.ldres, rrows, _ = _mat(res, 'res', dev)
        d.res_mod = res_mod or rrows
    if scat is not None:
        if out is None:
            raise _lib.HplError('scatter epilogue needs a zero-initialised `out`')
        d.scat, d.scat_stride, d.scat_c = ptr(scat), scat.stride(0), scat_c
    elif out is None and not query:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if out is None:               # (a query: the result gconv_raw would allocate -- contiguous and aligned)
        d.Y, d.ldy = _QUERY_PTR, N
    else:
        d.Y, d.ldy, _, _ = _mat(out, 'out', dev)
    if out2 is not None:
        d.Y2, d.ldy2, r2, c2 = _mat(out2, 'out2', dev)
        if scat is not None or rows2 > r2 or c2 < N:
            raise _lib.HplError('second destination: %d rows x %d columns for rows2=%d N=%d' % (r2, c2, rows2, N))
        d.rows2 = rows2
    if y_amax is not None:
        d.y_amax = ptr(y_amax)
        if y_guard is not None:
            d.y_guard = ptr(y_guard)
    if row_perm is not None:
        if row_perm.dtype is not torch.int32 or row_perm.numel() != M or not row_perm.is_contiguous():
            raise _lib.HplError('row_perm must be a contiguous int32 tensor of M=%d entries' % M)
        d.row_perm = ptr(row_perm)
        if tiles is not None:         # (tile_idx, tile_mask) of THIS table and row order (tile_index)
            d.tile_idx, d.tile_mask, d.tile_bm = ptr(tiles[0]), ptr(tiles[1]), tiles[0].shape[2]
        if CLOCK_PROBE is not None and N > 64 and M >= 16384:
            d.clock_probe = CLOCK_PROBE.data_ptr()
    st = None if query else stream()
    if split_k and scat is None and M * N <= _SPLITK_MAX_ELEMS:
        if query:
            d.ws, d.ws_bytes = _QUERY_PTR, _SPLITK_WS_FLOATS * 4
        else:
            ws = _splitk_workspace(A.device, st)
            d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    return d, out, st, keep


def gconv_raw(A, nbr, M, C, F, Wt, N, bias=None, act=ACT_NONE, res=None, res_mod=0, out=None,
              scat=None, scat_c=0, naive=False, slope=LEAKY_RATE, row_perm=None, split_k=True, reg_stride=0, tiles=None,
              out2=None, rows2=0, Wt3=None, y_amax=None, guard=True, y_guard=None, guard_trips=None):
    """Y[m, n] = act(bias[n] + res[m % res_mod, n] + sum_{f,c} A[nbr[f, m], c] * Wt[f*C + c, n]).
    row_perm (int32 [M], from tap_order): processing order of the output rows; results are unchanged.
    nbr None and reg_stride > 0: tap f of row m reads row f*reg_stride + m (no table: the displacement
    filter of the correlation layer, whose taps are the F blocks of H1 virtual vertices).
    out2 / rows2: rows m < rows2 of the result are also stored to the matrix (view) `out2`.
    y_amax (float32 [1], device, cleared by the caller): max(y_amax, largest |Y|) is left there; y_guard (int32 [1], cleared by the
    caller): the range-guard word of Y beside it.  guard: fp16-pair launches take the range guard of A with its largest magnitude
    (one pass: hpl_amax_rows) -- a second pass over the residuals when A has a row 2^18 below its largest entry; guard_trips
    (int32 [1], device): += 1 when this launch took it."""
    d, out, st, _keep = _gconv_desc(A, nbr, M, C, F, Wt, N, bias, act, res, res_mod, out, scat, scat_c, slope, row_perm, split_k,
                                    reg_stride, tiles, out2, rows2, Wt3, y_amax, guard, y_guard, guard_trips)
    lib = _lib.load()
    rc = (lib.hpl_gconv_forward_naive if naive else lib.hpl_gconv_forward)(ctypes.byref(d), st)
    if rc != 0:
        check(rc, 'hpl_gconv_forward')
    return out


def _info_dict(info):
    return {name: getattr(info, name) for name, _ in info._fields_ if name != 'pad_'}


def gconv_launch_info(A, nbr, M, C, F, Wt, N, bias=None, act=ACT_NONE, res=None, res_mod=0, out=None,
                      scat=None, scat_c=0, slope=LEAKY_RATE, row_perm=None, split_k=True, reg_stride=0, tiles=None,
                      out2=None, rows2=0, Wt3=None, y_amax=None, guard=True, y_guard=None, guard_trips=None):
    """The kernel instance gconv_raw takes for the same arguments, as a dict of hpl_gconv_info's fields (include/hpl_bcl.h).
    Host code only: it launches nothing and the tensors may be host tensors of the same shapes, strides and alignment."""
    d = _gconv_desc(A, nbr, M, C, F, Wt, N, bias, act, res, res_mod, out, scat, scat_c, slope, row_perm, split_k,
                    reg_stride, tiles, out2, rows2, Wt3, y_amax, guard, y_guard, guard_trips, query=True)[0]
    info = _lib.GConvInfo()
    check(_lib.load().hpl_gconv_launch_info(ctypes.byref(d), ctypes.byref(info)), 'hpl_gconv_launch_info')
    return _info_dict(info)


def _addr(t):
    """Address of a tensor on any device (or None): for the launch queries."""
    return None if t is None else t.data_ptr()


_QUERY_PTR = 256      # a non-null, aligned stand-in for device memory a query would otherwise have to allocate

#: diagnostic (bench.py): a zeroed int64 device tensor (>= 2 entries); sampled workgroups of the wide row-ordered
#: launches add their residence in shader cycles to [0] and in 100 MHz wall ticks to [1] -- the clock the chip
#: sustains under that kernel
CLOCK_PROBE = None

_SPLITK_MAX_ELEMS = 8 << 20          # split-K is offered for outputs of <= 8 M elements (the launch picks the count)
_SPLITK_WS = {}
_SPLITK_WS_FLOATS = 16 << 20


def _splitk_workspace(device, st):
    """Per-(device, stream) scratch for split-K partial tiles: 16 M floats = 64 MB (csrc/executor.hip: same size, so that both
    issue paths pick the same split counts: a launch fits its splits to the scratch)."""
    key = (device, st)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = _SPLITK_WS[key] = torch.empty(_SPLITK_WS_FLOATS, dtype=torch.float32, device=device)
    return ws


def _wgrad_args(A, nbr, M, C, F, dY, N, taps, want_bias, reg_stride, query=False, scales=True):
    """-> (arguments of hpl_gconv_wgrad_scaled up to the stream, dWt, bias gradient or None, device scalars the arguments point
    to): built in one place for the launch
    (wgrad_raw) and for the query of its instance (wgrad_launch_info; query: as _gconv_desc).
    scales: True: the largest magnitudes of A and dY are measured where the launch can use them; False: none are passed; a pair
    of float32 [1] device tensors: the caller's own (upper bounds of the magnitudes of A and dY)."""
    ptr = _addr if query else _lib.ptr
    if not query:
        A, dY = _cl(A), _cl(dY, 'dY')
    kp, ldw = round_up(F * C, 32), round_up(N, 4)
    if query:                     # (nothing is allocated: aligned stand-ins for the gradient and the bias gradient behind it)
        dWt, gb = None, None
        p_dWt, p_gb = _QUERY_PTR, (_QUERY_PTR + kp * ldw * 4 if want_bias else None)
    else:
        buf = torch.zeros(kp * ldw + (ldw if want_bias else 0), dtype=torch.float32, device=A.device)
        dWt = buf[:kp * ldw].view(kp, ldw)
        gb = buf[kp * ldw:kp * ldw + N] if want_bias else None
        p_dWt, p_gb = ptr(dWt), ptr(gb)
    tl, tr, tp = taps if (taps is not None and nbr is not None) else (None, None, None)
    # wide layers (csrc/wgrad3.hip's test): fp16-pair operands need the largest magnitudes of both
    sa = sd = keep = None
    if scales is not True and scales is not False:
        keep = tuple(scales)
        if len(keep) != 2 or any(s.dtype != torch.float32 or s.numel() != 1 for s in keep):
            raise _lib.HplError('wgrad: scales must be True, False or a pair of float32 [1] tensors')
        sa, sd = ptr(keep[0]), ptr(keep[1])
    elif scales and SPLIT_PLANES == 2 and SPLIT3 and N >= 256 and C >= 128 and M >= 8192 and \
            (tl is not None or (F == 1 and nbr is None)):
        if query:
            sa = sd = _QUERY_PTR
        else:
            keep = (amax(A, cols=C), amax(dY, rows=M, cols=N))       # (both alive until the launch is enqueued)
            sa, sd = ptr(keep[0]), ptr(keep[1])
    return (ptr(A), _ld(A), A.shape[0], ptr(nbr), nbr.stride(0) if nbr is not None else 0,
            reg_stride if nbr is None else 0, M, C, F, ptr(dY), _ld(dY), N, p_dWt, ldw,
            ptr(tl), ptr(tr), ptr(tp), M if tl is not None else 0, p_gb, sa, sd), dWt, gb, keep


def wgrad_raw(A, nbr, M, C, F, dY, N, taps=None, want_bias=False, reg_stride=0, scales=True):
    """-> dWt [roundup(F*C,32), roundup(N,4)] = sum_m A[nbr[f,m], c] * dY[m, n]  (and, with want_bias,
    the bias gradient sum_m dY[m, :] from the same launch).
    taps = tap_lists(nbr): sum over the present vertices of each tap only (wide layers).
    scales: the operand magnitudes of the wide layers' fp16-pair form (csrc/wgrad3.hip).  True: measured here; False: none, so
    the split-operand kernel takes bf16 triples; (a, d): float32 [1] device tensors >= the largest |A| and |dY|."""
    args, dWt, gb, _keep = _wgrad_args(A, nbr, M, C, F, dY, N, taps, want_bias, reg_stride, scales=scales)
    check(_lib.load().hpl_gconv_wgrad_scaled(*(args + (stream(),))), 'hpl_gconv_wgrad')
    return (dWt, gb) if want_bias else dWt


def wgrad_launch_info(A, nbr, M, C, F, dY, N, taps=None, want_bias=False, reg_stride=0, scales=True):
    """The kernel instance wgrad_raw takes for the same arguments, as a dict of hpl_wgrad_info's fields (include/hpl_bcl.h).
    Host code only, as gconv_launch_info."""
    args = _wgrad_args(A, nbr, M, C, F, dY, N, taps, want_bias, reg_stride, query=True, scales=scales)[0]
    info = _lib.WGradInfo()
    check(_lib.load().hpl_wgrad_launch_info(*(args + (ctypes.byref(info),))), 'hpl_wgrad_launch_info')
    return _info_dict(info)


def colsum(X):
    X = _cl(X)
    out = torch.empty(X.shape[1], dtype=torch.float32, device=X.device)
    check(_lib.load().hpl_colsum(ptr(X), _ld(X), X.shape[0], X.shape[1], ptr(out), stream()), 'hpl_colsum')
    return out


def leaky_bwd(dY, Y, slope=LEAKY_RATE, amax=None):
    """dX = dY * (Y > 0 ? 1 : slope); amax (float32 [1], cleared by the caller): max(amax, largest |dX|) is left there."""
    dY, Y = _cl(dY, 'dY'), _cl(Y, 'Y')
    dX = torch.empty(tuple(Y.shape), dtype=torch.float32, device=Y.device)
    check(_lib.load().hpl_leaky_bwd_amax(ptr(dY), _ld(dY), ptr(Y), _ld(Y), slope, ptr(dX), _ld(dX), Y.shape[0],
                                         Y.shape[1], ptr(amax), stream()), 'hpl_leaky_bwd')
    return dX


# --------------------------------------------------------------------------- autograd
class SplatFn(torch.autograd.Function):
    """splat + density normalisation (models/bilateralNN.py:151-186); backward is a slice
    weighted by the normaliser (SparseSum.backward, bilateralNN.py:33-40)."""

    @staticmethod
    def forward(ctx, feat, cloud, use_norm):
        ctx.cloud, ctx.use_norm = cloud, use_norm
        return splat_raw(feat, cloud.csr(), cloud.H, use_norm)

    @staticmethod
    def backward(ctx, g):
        g = g if g.stride(1) == 1 else g.contiguous()
        return ctx.cloud.slice_back(g, ctx.use_norm), None, None


class SliceFn(torch.autograd.Function):
    """slice + bias (models/bilateralNN.py:223-238); backward w.r.t. Y is an un-normalised splat."""

    @staticmethod
    def forward(ctx, Y, cloud, bias):
        ctx.cloud = cloud
        ctx.has_bias = bias is not None
        return slice_raw(Y, cloud.bary, cloud.off, cloud.N, bias=bias)

    @staticmethod
    def backward(ctx, g):
        c = ctx.cloud
        g = g if g.stride(1) == 1 else g.contiguous()
        gY = splat_raw(g, c.csr(), c.H, use_norm=False)
        gb = colsum(g) if ctx.has_bias else None
        return gY, None, gb


_MIRROR = {}


def _mirror_map(F, device):
    # tap f of the forward table is tap (F - f) % F seen from the neighbour
    key = (F, str(device))
    if key not in _MIRROR:
        _MIRROR[key] = ((F - torch.arange(F, device=device)) % F).to(torch.int32)
    return _MIRROR[key]


class WeightBank(object):
    """Training re-lays every conv weight after each optimiser step, once for the forward and once for
    the data gradient: ~160 small launches per step.  The bank records those requests during the
    first step and from then on refreshes ALL images with one launch (`hpl_weight_relayout_batch`)
    at the start of a step; a lookup is served from the bank while the parameter's version still is
    the one the refresh saw, otherwise the caller re-lays that weight on its own."""

    def __init__(self):
        self.jobs = collections.OrderedDict()     # key -> [weight, args, offset, elems, version]
        self.buf = None
        self.dev_jobs = self.dev_prefix = None
        self.total = 0
        self.dirty = False                        # jobs added since the device tables were built

    @staticmethod
    def _key(weight, R, Q, F, sr, sq, sf, base, mirror):
        return (weight.data_ptr(), tuple(weight.shape), R, Q, F, sr, sq, sf, base, mirror)

    def get(self, weight, R, Q, F, sr, sq, sf, base=0, mirror=False):
        """The [roundup(F*R,32), roundup(Q,4)] image of `weight`, from the bank when fresh."""
        key = self._key(weight, R, Q, F, sr, sq, sf, base, mirror)
        job = self.jobs.get(key)
        k_rows, ldw = round_up(F * R, 32), round_up(Q, 4)
        if job is not None and not self.dirty and job[4] == weight._version and job[0] is weight:
            img = self.buf[job[2]:job[2] + job[3]].view(k_rows, ldw)
            img._hpl_bank_job = job             # split3_of keeps the image's split planes with the job
            return img
        if job is None:
            self.register(weight, R, Q, F, sr, sq, sf, base, mirror)
        fmap = _mirror_map(F, weight.device) if mirror else None
        return weight_relayout(weight, R, Q, F, sr, sq, sf, base=base, fmap=fmap)

    def register(self, weight, R, Q, F, sr, sq, sf, base=0, mirror=0):
        """Record an image without producing it (the native plans: every image exists after the next refresh()).
        mirror 0 / 1: Wt[(f*R + r), q] (taps as stored / in the order (F - f) % F); mirror 2: taps as column blocks,
        Wt[r, f*Q + q] (hpl_relayout_job).  -> the job (offset in job[2] after refresh, image shape (job[6], job[7]))."""
        key = self._key(weight, R, Q, F, sr, sq, sf, base, mirror)
        job = self.jobs.get(key)
        if job is None:
            k_rows, ldw = (round_up(R, 32), round_up(F * Q, 4)) if mirror == 2 else (round_up(F * R, 32), round_up(Q, 4))
            job = self.jobs[key] = [weight, (R, Q, F, sr, sq, sf, base, mirror), None, k_rows * ldw, -1, None, k_rows, ldw]
            self.dirty = True
        return job

    def refresh(self, lo=0, hi=None):
        """One launch: every recorded image (or the images of jobs [lo, hi) in registration order) from the current parameter values."""
        if not self.jobs:
            return
        dev = next(iter(self.jobs.values()))[0].device
        if self.dirty or self.buf is None:
            arr = (RelayoutJob * len(self.jobs))()
            prefix = [0]
            for i, job in enumerate(self.jobs.values()):
                w, (R, Q, F, sr, sq, sf, base, mirror) = job[0], job[1]
                arr[i].W, arr[i].base, arr[i].sr, arr[i].sq, arr[i].sf = w.data_ptr(), base, sr, sq, sf
                arr[i].R, arr[i].Q, arr[i].F, arr[i].mirror = R, Q, F, int(mirror)
                arr[i].ldw = round_up(F * Q, 4) if int(mirror) == 2 else round_up(Q, 4)
                job[2] = prefix[-1]
                prefix.append(prefix[-1] + job[3])
            self.total = prefix[-1]
            self.prefix_host = prefix
            raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.dev_jobs = raw.to(dev)
            self.dev_prefix = torch.tensor(prefix, dtype=torch.int64, device=dev)
            self.buf = torch.empty(self.total, dtype=torch.float32, device=dev)
            self.dirty = False
        hi = len(self.jobs) if hi is None else hi
        if hi <= lo:
            return
        check(_lib.load().hpl_weight_relayout_batch(self.dev_jobs.data_ptr() + lo * ctypes.sizeof(RelayoutJob), hi - lo,
                                                    self.dev_prefix.data_ptr() + 8 * lo, self.prefix_host[hi] - self.prefix_host[lo],
                                                    ptr(self.buf), stream()), 'hpl_weight_relayout_batch')
        for job in list(self.jobs.values())[lo:hi]:
            job[4] = job[0]._version


#: bank used by the autograd path when a training loop calls BANK.refresh() at the start of its steps
BANK = None


def enable_weight_bank(on=True):
    """Switch the batched weight re-layout of the training path on / off (off: one launch per use)."""
    global BANK
    BANK = WeightBank() if on else None
    return BANK


def _train_relayout(weight, R, Q, F, sr, sq, sf, base=0, mirror=False):
    if BANK is not None:
        return BANK.get(weight, R, Q, F, sr, sq, sf, base, mirror)
    fmap = _mirror_map(F, weight.device) if mirror else None
    return weight_relayout(weight, R, Q, F, sr, sq, sf, base=base, fmap=fmap)


MAX_TAPS_PER_PASS = 15      # hpl_gconv_forward: F <= 15 (LDS-staged index table of a tile)


def gconv_passes(A, nbr, M, C, F, Wt, N, groups=None, bias=None, act=ACT_NONE, res=None, res_mod=0, out=None,
                 slope=LEAKY_RATE, row_perm=None, reg_stride=0, tiles=None, guard=True):
    """gconv_raw, run as one pass per tap group when `groups` = [(f0, f1, perm), ...] is given: pass i
    contracts taps [f0, f1) (rows f0*C.. of Wt, rows f0.. of the table) in its own row order and adds
    to the output of the passes before it; bias / residual enter the first pass, the activation the last."""
    regular = nbr is None and reg_stride > 0
    if not groups and (nbr is not None or regular) and F > MAX_TAPS_PER_PASS:
        # radius-2 stencils (65 taps): the kernel stages the indices of at most 15 taps per tile, so the
        # contraction runs as ceil(F / 15) accumulating passes over consecutive tap ranges
        groups = [(f0, min(F, f0 + MAX_TAPS_PER_PASS), None) for f0 in range(0, F, MAX_TAPS_PER_PASS)]
    # wide stencil layers also carry the split image of their weights: the kernel takes the launch when it is big enough
    W3 = split3_of(Wt) if (SPLIT3 and (nbr is not None or F == 1) and N >= SPLIT3_MIN_N and C >= SPLIT3_MIN_C) else None
    if not groups or not (nbr is not None or regular) or len(groups) < 2:
        return gconv_raw(A, nbr, M, C, F, Wt, N, bias=bias, act=act, res=res, res_mod=res_mod, out=out, slope=slope,
                         row_perm=row_perm, reg_stride=reg_stride, tiles=tiles if not isinstance(tiles, list) else None,
                         Wt3=W3, guard=guard)
    y = out
    gt = tiles if isinstance(tiles, list) and len(tiles) == len(groups) else [None] * len(groups)
    for i, (f0, f1, perm) in enumerate(groups):
        first, last = i == 0, i == len(groups) - 1
        # the same rows of the split image (k-blocks of 8 rows, 16 bytes per column)
        w3 = W3.rows_from(f0 * C, Wt.shape[1]) if (W3 is not None and (f0 * C) % 8 == 0) else None
        # a tap range of a regular pattern is the same pattern over the rows from f0*reg_stride on
        y = gconv_raw(A[f0 * reg_stride:] if regular else A, None if regular else nbr[f0:f1], M, C, f1 - f0,
                      Wt[f0 * C:], N, bias=bias if first else None,
                      act=act if last else ACT_NONE, res=res if first else y, res_mod=res_mod if first else 0,
                      out=y, slope=slope, row_perm=perm, reg_stride=reg_stride, tiles=gt[i] if perm is not None else None,
                      Wt3=w3, guard=guard)
    return y


def _split3_entry(Wt, version):
    ev = torch.cuda.Event()
    w3 = weight_split3(Wt)
    ev.record()                       # behind k_weight_split3: a consumer on another stream waits for THIS, not for the re-layout
    return [w3, version, ev, stream()]


def _split3_wait(entry):
    ev = entry[2]
    if ev is not None and stream() != entry[3]:
        if ev.query():
            entry[2] = None           # seen complete once: visible to every later launch on any stream
        else:
            torch.cuda.current_stream().wait_event(ev)
    return entry[0]


def split3_of(Wt):
    """The split image of a weight image, made once per image: images handed out by a WeightBank keep it with the bank's
    job (the bank returns a fresh view of its buffer on every lookup, so an attribute on the view would never be found
    again; valid while the job's parameter version is the one its last refresh saw), other images carry it as an
    attribute keyed on their version.  Either way the entry holds the event recorded behind the split kernel: a forward
    on another stream that finds the entry waits for the split, not just for the re-layout (_cached_relayout's event)."""
    job = getattr(Wt, '_hpl_bank_job', None)
    if job is not None:
        ent = job[5]
        if ent is None or ent[1] != job[4]:
            ent = job[5] = _split3_entry(Wt, job[4])
        return _split3_wait(ent)
    ent = getattr(Wt, '_hpl_split3', None)
    if ent is None or ent[1] != Wt._version:
        ent = Wt._hpl_split3 = _split3_entry(Wt, Wt._version)
    return _split3_wait(ent)


class GConvFn(torch.autograd.Function):
    """Gathered convolution Y = act(b + sum_f W_f . A[nbr[f]]) with the conv weight in its torch
    layout `weight.view(O, Ctot, F)`; channels [c0, c0+C) of the weight are used.

    bwd_mode: 'mirror' (symmetric table over the same vertex set: gather with mirrored taps),
              'scatter' (any table: fp32 atomics), 'dense' (no table)."""

    @staticmethod
    def forward(ctx, A, weight, bias, nbr, M, c0, C, F, act, res, res_mod, bwd_mode, slope, row_perm=None,
                taps=None, groups=None, reg_stride=0, tiles=None):
        O = weight.shape[0]
        Ctot = weight.numel() // (O * F)
        Wt = _train_relayout(weight, C, O, F, F, Ctot * F, 1, base=c0 * F)
        Y = gconv_passes(A, nbr, M, C, F, Wt, O, groups, bias=bias, act=act, res=res, res_mod=res_mod, slope=slope,
                         row_perm=row_perm, reg_stride=reg_stride, tiles=tiles)
        ctx.reg_stride = reg_stride
        ctx.tiles = tiles            # the mirror backward gathers through the same table in the same row orders
        ctx.groups = groups          # the mirror backward gathers through the same table: same groups
        ctx.slope = slope
        ctx.row_perm = row_perm      # same table in the mirror backward -> same tap masks -> same order
        ctx.taps = taps
        ctx.save_for_backward(A, weight, nbr, Y if act != ACT_NONE else None)
        ctx.cfg = (M, c0, C, F, act, res is not None, res_mod, bwd_mode, bias is not None, Ctot)
        return Y

    @staticmethod
    def backward(ctx, g):
        A, weight, nbr, Y = ctx.saved_tensors
        M, c0, C, F, act, has_res, res_mod, bwd_mode, has_bias, Ctot = ctx.cfg
        O = weight.shape[0]
        g = g if (g.dim() == 2 and g.stride(1) == 1) else g.contiguous()
        if act == ACT_LEAKY:
            g = leaky_bwd(g, Y, ctx.slope)
        gA = gW = gb = gres = None
        if ctx.needs_input_grad[0]:
            rows = A.shape[0]
            if bwd_mode == 'dense':
                WtT = _train_relayout(weight, O, C, 1, Ctot * F, F, 1, base=c0 * F)
                # wide 1x1 layers: the data gradient is a dense GEMM of the same class as their forward (split operands)
                W3 = split3_of(WtT) if (SPLIT3 and C >= SPLIT3_MIN_N and O >= SPLIT3_MIN_C) else None
                gA_c = gconv_raw(g, None, M, O, 1, WtT, C, Wt3=W3, guard=False)       # (gradients run unguarded: HPL_FLAG_NOGUARD)
            elif bwd_mode == 'mirror':
                if rows != M:
                    raise _lib.HplError('mirror backward needs a table over the same vertex set')
                WtT = _train_relayout(weight, O, C, F, Ctot * F, F, 1, base=c0 * F, mirror=True)
                gA_c = gconv_passes(g, nbr, M, O, F, WtT, C, ctx.groups, row_perm=ctx.row_perm, tiles=ctx.tiles, guard=False)
            else:   # scatter: G[m, (f, c)] = g[m] . W[:, c, f], added into row nbr[f, m]
                # columns ordered (f, c): source element (o, f*C + c) = W[o, c0 + c, f]
                Wcols = weight.view(O, Ctot, F)[:, c0:c0 + C, :].permute(0, 2, 1).reshape(O, F * C).contiguous()
                WtS = weight_relayout(Wcols, O, F * C, 1, F * C, 1, 1)
                if bwd_mode == 'regular':
                    # source rows f*stride + m are all distinct: block f of G IS the gradient of rows
                    # [f*stride, f*stride + M) -- a plain GEMM and one strided copy, no atomics
                    G = gconv_raw(g, None, M, O, 1, WtS, F * C)
                    rs = ctx.reg_stride
                    if rs == M and rows == F * M:
                        gA_c = G.view(M, F, C).transpose(0, 1).reshape(F * M, C)
                    else:
                        gA_c = torch.zeros((rows, C), dtype=torch.float32, device=A.device)
                        for f in range(F):
                            gA_c[f * rs:f * rs + M] = G[:, f * C:(f + 1) * C]
                else:
                    gA_c = torch.zeros((rows, C), dtype=torch.float32, device=A.device)
                    gconv_raw(g, None, M, O, 1, WtS, F * C, out=gA_c, scat=nbr, scat_c=C)
            if C == A.shape[1]:
                gA = gA_c
            else:
                gA = torch.zeros_like(A)
                gA[:, :C] = gA_c
        want_gb = has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dWt = wgrad_raw(A, nbr, M, C, F, g, O, taps=ctx.taps, want_bias=want_gb, reg_stride=ctx.reg_stride)
            if want_gb:
                dWt, gb = dWt
            # the un-layout writes every element of the channel range: zeros only for partial ranges
            gW = torch.empty_like(weight) if (c0 == 0 and C == Ctot) else torch.zeros_like(weight)
            check(_lib.load().hpl_weight_unlayout(ptr(dWt), dWt.shape[1], C, O, F, ptr(gW), c0 * F, F, Ctot * F, 1,
                                                  0, stream()), 'hpl_weight_unlayout')
        elif want_gb:
            gb = colsum(g)
        if has_res and ctx.needs_input_grad[9]:
            if res_mod and res_mod != M:
                gres = g.view(M // res_mod, res_mod, O).sum(dim=0)
            else:
                gres = g
        return gA, gW, gb, None, None, None, None, None, None, gres, None, None, None, None, None, None, None, None


def _cols_image(weight, C, O, F, Ctot, c0):
    """[roundup(C, 32), roundup(F*O, 4)] image with element (c, f*O + o) = weight[o, c0 + c, f] ("taps as column blocks",
    hpl_relayout_job.mirror == 2): from the training bank when it holds a fresh one, else made here."""
    if BANK is not None:
        job = BANK.register(weight, C, O, F, F, Ctot * F, 1, c0 * F, 2)
        if not BANK.dirty and job[4] == weight._version and job[0] is weight:
            return BANK.buf[job[2]:job[2] + job[3]].view(job[6], job[7])
    img = torch.zeros((round_up(C, 32), round_up(F * O, 4)), dtype=torch.float32, device=weight.device)
    img[:C, :F * O] = weight.detach().reshape(O, Ctot, F)[:, c0:c0 + C, :].permute(1, 2, 0).reshape(C, F * O)
    return img


class CorrPc2Fn(torch.autograd.Function):
    """The pc2 half of the patch correlation (models/bnn_flow.py:195-202) over the F*H0 virtual vertices:
    P[f*H0 + h] = act(bias + res[h] + sum_k W_k . f2[corr2[k][f*H0 + h]]), computed as a projection of every pc2 vertex per tap
    (one dense GEMM) and a gather-sum (hpl_gather_sum); the backward gathers through the inverse table (no atomics)."""

    @staticmethod
    def forward(ctx, f2, weight, bias, res, table, H0, F, K, c0, C, slope):
        O = weight.shape[0]
        Ctot = weight.numel() // (O * K)
        Hv = f2.shape[0]
        Z = gconv_raw(f2, None, Hv, C, 1, _cols_image(weight, C, O, K, Ctot, c0), K * O)
        Y = gather_sum_raw(Z, table.t, F * H0, K, O, O, bias=bias, res=res, res_mod=H0, act=ACT_LEAKY, slope=slope)
        ctx.table, ctx.cfg = table, (H0, F, K, c0, C, O, Ctot, Hv, slope)
        ctx.save_for_backward(f2, weight, Y)
        return Y

    @staticmethod
    def backward(ctx, g):
        f2, weight, Y = ctx.saved_tensors
        H0, F, K, c0, C, O, Ctot, Hv, slope = ctx.cfg
        g = g if (g.dim() == 2 and g.stride(1) == 1) else g.contiguous()
        g = leaky_bwd(g, Y, slope)
        gres = g.view(F, H0, O).sum(dim=0) if ctx.needs_input_grad[3] else None
        gb = colsum(g) if ctx.needs_input_grad[2] else None
        gf2 = gW = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            inv = ctx.table.inverse(H0, F, Hv)
            dZ = gather_sum_raw(g, inv, K * Hv, F, O, 0).view(Hv, K * O)
            if ctx.needs_input_grad[0]:
                WzT = _train_relayout(weight, O, C, K, Ctot * K, K, 1, base=c0 * K)          # [(k*O + o), c]
                gf2 = gconv_raw(dZ, None, Hv, K * O, 1, WzT, C)
            if ctx.needs_input_grad[1]:
                dWz = wgrad_raw(f2, None, Hv, C, 1, dZ, K * O)
                gW = torch.zeros_like(weight)
                gW.view(O, Ctot, K)[:, c0:c0 + C, :] = dWz[:C, :K * O].view(C, K, O).permute(2, 0, 1)
        return gf2, gW, gb, gres, None, None, None, None, None, None, None


def corr_pc2(f2, weight, bias, res, table, H0, F, K, c0, C, slope):
    """-> [F*H0, O]; `table`: bcl.NbrTable of the permuted pc2_corr_indices [K, F*H0]."""
    if torch.is_grad_enabled() and (f2.requires_grad or weight.requires_grad or (res is not None and res.requires_grad)):
        return CorrPc2Fn.apply(f2, weight, bias, res, table, H0, F, K, c0, C, slope)
    O = weight.shape[0]
    Ctot = weight.numel() // (O * K)
    key = (id(weight), c0, C, 'cols')
    hit = _WT_CACHE.get(key)
    if hit is None or hit[2] != weight._version or hit[1] is not weight or hit[3] != weight.data_ptr():
        img = _cols_image(weight, C, O, K, Ctot, c0)
        ev = torch.cuda.Event()
        ev.record()
        hit = _WT_CACHE[key] = [img, weight, weight._version, weight.data_ptr(), ev, stream()]
    elif hit[4] is not None and stream() != hit[5]:
        if hit[4].query():
            hit[4] = None
        else:
            torch.cuda.current_stream().wait_event(hit[4])
    Z = gconv_raw(f2, None, f2.shape[0], C, 1, hit[0], K * O)
    return gather_sum_raw(Z, table.t, F * H0, K, O, O, bias=bias, res=res, res_mod=H0, act=ACT_LEAKY, slope=slope)


def gconv(A, weight, bias, nbr, M, F, act=ACT_NONE, c0=0, C=None, res=None, res_mod=0, bwd_mode='scatter',
          out=None, slope=LEAKY_RATE, row_perm=None, taps=None, tap_groups=None, reg_stride=0, tiles=None):
    """Autograd-aware gathered convolution; with grad disabled it can write into `out`.

    tap_groups: [(f0, f1, perm), ...] -- the contraction is run as one pass per group of
    consecutive taps, each with the rows sorted by the group's own (short) tap mask, the passes
    accumulating into the output (bias in the first, activation in the last).  A 5-bit mask leaves
    ~32 row classes, so 64-row tiles are nearly pure and absent taps are skipped almost exactly
    (43 % instead of 59 % of the slices executed on bcn1_, 72 % instead of 83 % on bcn2_)."""
    O = weight.shape[0]
    Ctot = weight.numel() // (O * F)
    C = Ctot if C is None else C
    if torch.is_grad_enabled() and (A.requires_grad or weight.requires_grad or
                                    (res is not None and res.requires_grad)):
        y = GConvFn.apply(A, weight, bias, nbr, M, c0, C, F, act, res, res_mod, bwd_mode, slope, row_perm,
                          taps() if callable(taps) else taps,
                          tap_groups() if callable(tap_groups) else tap_groups, reg_stride,
                          tiles() if callable(tiles) else tiles)
        if out is not None:
            out.copy_(y)
            return out
        return y
    Wt = _cached_relayout(weight, C, O, F, Ctot, c0)
    groups = tap_groups() if callable(tap_groups) else tap_groups
    return gconv_passes(A, nbr, M, C, F, Wt, O, groups, bias=bias, act=act, res=res, res_mod=res_mod, out=out,
                        slope=slope, row_perm=row_perm, reg_stride=reg_stride, tiles=tiles() if callable(tiles) else tiles)


_WT_CACHE = collections.OrderedDict()
_WT_CACHE_MAX = 512


def invalidate_weight_cache():
    """Drop every cached weight image of the inference path.  The cache keys on the parameter's identity,
    version counter and data pointer, which writes through `param.data` (`p.data.copy_(...)`, reference-style
    `model.apply(init)` with `m.weight.data`) do NOT change: call this after editing weights that way.
    (In-place writes through the parameter under torch.no_grad(), load_state_dict and optimiser steps bump the
    version and need nothing.)  The native forward plans (plan.ForwardPlan) key on the epoch bumped here as well: they
    refresh their weight images and combined biases at their next use."""
    global _WEIGHT_EPOCH
    _WT_CACHE.clear()
    _WEIGHT_EPOCH += 1


_WEIGHT_EPOCH = 0


def weight_epoch():
    return _WEIGHT_EPOCH


def _cached_relayout(weight, C, O, F, Ctot, c0):
    """Inference path: the k-major weight image only changes when the parameter does (tensor identity +
    version counter); the entry keeps the parameter alive, so its id cannot be recycled while cached.
    An image is produced on one stream and may be consumed on others (bench.py alternates forwards over
    several): the entry carries the event recorded behind its re-layout kernel, and a consumer on another
    stream waits for it until it has been seen complete once."""
    key = (id(weight), c0, C)
    hit = _WT_CACHE.get(key)
    if hit is not None and hit[2] == weight._version and hit[1] is weight and hit[3] == weight.data_ptr():
        ev = hit[4]
        if ev is not None:
            st = stream()
            if st != hit[5]:
                if ev.query():
                    hit[4] = None
                else:
                    torch.cuda.current_stream().wait_event(ev)
        return hit[0]
    Wt = weight_relayout(weight.detach(), C, O, F, F, Ctot * F, 1, base=c0 * F)
    ev = torch.cuda.Event()
    ev.record()
    _WT_CACHE[key] = [Wt, weight, weight._version, weight.data_ptr(), ev, stream()]     # (.data swaps keep id and version)
    _WT_CACHE.move_to_end(key)
    if len(_WT_CACHE) > _WT_CACHE_MAX:
        _WT_CACHE.popitem(last=False)
    return Wt
