"""GPU: the self-supervised loss in the native training step.  hpl_pair_grad is pinned bit for bit against numpy;
the native step under loss='selfsup' (train_plan.TrainPlan.step_batch) matches autograd through ops.selfsup_loss for one pair
and for an equal batch; engine.Trainer takes it only when asked, and engine.main trains with --selfsup-native."""
import math

import numpy as np
import pytest
import torch

from hplflownet_amd.synthetic import surface_pair, synthetic_pair
from test_gpu_train_batch import KINK_BAR, _dev, _model, _single_lat

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ----------------------------------------------------------------------------- hpl_pair_grad
@pytest.mark.parametrize('rows', [1, 5, 1024, 1027])
def test_pair_grad_is_numpy(rows):
    from hplflownet_amd import _lib
    from hplflownet_amd._lib import check
    lib = _lib.load()
    g = torch.Generator(device='cpu').manual_seed(rows)
    total = rows * 3
    for B, stride in ((3, 1), (5, 4), (64, 4), (1, 1)):
        losses = torch.randn(B, stride, generator=g).to(DEV)
        s = np.float32(0)
        for v in losses[:, 0].cpu().numpy():
            s = np.float32(s + v)
        want_loss = np.float32(s / np.float32(B))
        w = np.float32(1.0) / np.float32(B)
        for off_src, off_dst in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (2, 3), (3, 0)):        # floats past a 16-byte boundary
            src = torch.randn(total + 8, generator=g).to(DEV)
            dst = torch.full((total + 12,), float('nan'), device=DEV)
            loss = torch.full((2,), float('nan'), device=DEV)
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            d = dst[4 + off_dst:]
            check(lib.hpl_pair_grad(src[off_src:].data_ptr(), rows, B, losses.data_ptr(), stride, d.data_ptr(), loss.data_ptr(),
                                    _lib.stream()), 'hpl_pair_grad')
            torch.cuda.synchronize()
            want = src[off_src:off_src + total].cpu().numpy() * w
            got = d[:total].cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rows, B, off_src, off_dst)
            assert bool(torch.isnan(dst[:4 + off_dst]).all()) and bool(torch.isnan(d[total:]).all())      # nothing outside
            assert loss[:1].cpu().numpy().view(np.int32)[0] == want_loss.view(np.int32) and math.isnan(float(loss[1]))


def test_pair_grad_loss_alone_and_gradient_alone():
    from hplflownet_amd import _lib
    from hplflownet_amd._lib import check
    lib = _lib.load()
    g = torch.Generator(device='cpu').manual_seed(7)
    rows, B, stride = 333, 6, 4
    losses = torch.randn(B, stride, generator=g).to(DEV)
    src = torch.randn(rows * 3, generator=g).to(DEV)
    s = np.float32(0)
    for v in losses[:, 0].cpu().numpy():
        s = np.float32(s + v)
    want_loss = np.float32(s / np.float32(B))
    loss = torch.full((2,), float('nan'), device=DEV)
    dst = torch.full((rows * 3 + 4,), float('nan'), device=DEV)
    check(lib.hpl_pair_grad(None, rows, B, losses.data_ptr(), stride, None, loss.data_ptr(), _lib.stream()), 'hpl_pair_grad')
    check(lib.hpl_pair_grad(src.data_ptr(), rows, B, None, 1, dst.data_ptr(), None, _lib.stream()), 'hpl_pair_grad')
    torch.cuda.synchronize()
    assert loss[:1].cpu().numpy().view(np.int32)[0] == want_loss.view(np.int32) and math.isnan(float(loss[1]))
    want = src.cpu().numpy() * (np.float32(1.0) / np.float32(B))
    assert np.array_equal(dst[:rows * 3].cpu().numpy().view(np.int32), want.view(np.int32)) and bool(torch.isnan(dst[rows * 3:]).all())


def _pairs(kinds, counts, seed, sf_nan=False):
    """lists of (3, N1_b) pc1, (3, N2_b) pc2, (3, N1_b) sf: pair b drawn by kinds[b] ('frustum' or 'surface')"""
    out = [[], [], []]
    for b, (kind, (n1, n2)) in enumerate(zip(kinds, counts)):
        trio = (synthetic_pair if kind == 'frustum' else surface_pair)(max(n1, n2), seed + 7 * b)
        for j, n in enumerate((n1, n2, n1)):
            out[j].append(_dev(trio[j][:n]))
    if sf_nan:
        out[2] = [torch.full_like(s, float('nan')) for s in out[2]]
    return tuple(out)


# ----------------------------------------------------------------------------- the self-supervised loss in the native step
SELFSUP = {'k': 4, 'w_chamfer': 1.0, 'w_smooth': 0.5}


@pytest.mark.parametrize('activation', ['smooth', 'leaky'])
@pytest.mark.parametrize('form,counts', [('single', [(256, 256)]), ('single', [(301, 257)]), ('equal', [(256, 256), (256, 256)]),
                                         ('equal', [(200, 230)] * 3)])
def test_native_selfsup_step_matches_autograd(form, counts, activation, monkeypatch):
    from hplflownet_amd import bcl, ops
    from hplflownet_amd.train_plan import TrainPlan
    if activation == 'smooth':
        monkeypatch.setattr(bcl, 'LEAKY_RATE', 1.0)
    model, gen = _model('HPLFlowNetShallow')
    B = len(counts)
    p1, p2, nan_sf = _pairs(('frustum', 'surface', 'frustum')[:B], counts, 90 + B, sf_nan=True)
    # reference: autograd through a second model of the same weights, dL_b/dflow / B fed into each pair's forward
    ref, _ = _model('HPLFlowNetShallow')
    ref_losses = []
    for b in range(B):
        flow = ref(p1[b][None], p2[b][None], _single_lat(gen, p1[b], p2[b]))
        loss4, dflow = ops.selfsup_loss(p1[b], flow.detach()[0], p2[b], SELFSUP['k'], SELFSUP['w_chamfer'], SELFSUP['w_smooth'])
        flow.backward(dflow.t()[None] / B)
        ref_losses.append(float(loss4[0, 0]))
    torch.cuda.synchronize()
    plan = TrainPlan(model)
    t1, t2 = torch.stack(p1), torch.stack(p2)
    # (the label is never read: NaN for the equal batch, None for the single pair)
    r = plan.step_batch(t1, t2, torch.stack(nan_sf) if form == 'equal' else None, gen.build_native_batch(t1, t2, for_training=True),
                        loss='selfsup', selfsup=SELFSUP)
    assert r is not None                      # the native path was taken
    plan.finish()
    torch.cuda.synchronize()
    pair_losses, loss = r[2].tolist(), float(r[1])
    for x, y in zip(pair_losses, ref_losses):
        assert abs(x - y) <= 1e-5 * abs(y), (x, y)
    mean = sum(ref_losses) / B
    assert abs(loss - mean) <= 1e-5 * abs(mean), (loss, mean)
    worst = ('', 0.0)
    for (k, p), q in zip(model.named_parameters(), ref.parameters()):
        qg = q.grad if q.grad is not None else torch.zeros_like(q)
        err = float((p.grad - qg).abs().max()) / max(float(qg.abs().max()), 1e-20)
        worst = max(worst, (k, err), key=lambda kv: kv[1])
    print('selfsup %s %s %s: loss %.3g, worst gradient %s %.3g' % (form, counts, activation, abs(loss - mean) / abs(mean), worst[0], worst[1]))
    assert worst[1] < (2e-4 if activation == 'smooth' else KINK_BAR), worst


def test_trainer_selfsup_native_is_opt_in():
    from hplflownet_amd import engine
    p1, p2, nan_sf = _pairs(('frustum', 'surface'), [(256, 256), (256, 256)], 95, sf_nan=True)
    tr = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup', selfsup=SELFSUP, native_step=True)
    assert tr.native_step
    l1 = tr.train_step(p1[0], p2[0], nan_sf[0], tr._single_lattice(p1[0], p2[0]))
    assert tr.native_steps == 1 and bool(torch.isfinite(l1))
    e1, e2 = torch.stack(p1), torch.stack(p2)
    l2 = tr.train_step_batch(e1, e2, torch.stack(nan_sf), tr.gen.build_native_batch(e1, e2, for_training=True))
    assert tr.native_steps == 2 and tuple(l2.shape) == (2,) and bool(torch.isfinite(l2).all())
    l3 = tr.train_step_batch(e1[:1], e2[:1], torch.stack(nan_sf[:1]), tr.gen.build_native_batch(e1[:1], e2[:1], for_training=True))
    assert tr.native_steps == 3 and tuple(l3.shape) == (1,) and bool(torch.isfinite(l3).all())
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
    # the native step reports what the autograd step of the same weights reports
    a = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup', selfsup=SELFSUP)
    assert not a.native_step                      # the default keeps the self-supervised loss on the autograd path
    la = a.train_step(p1[0], p2[0], nan_sf[0], a._single_lattice(p1[0], p2[0]))
    a.train_step_batch(e1, e2, torch.stack(nan_sf), a.gen.build_native_batch(e1, e2, for_training=True))
    assert a.native_steps == 0 and a.tplan is None
    assert abs(float(la) - float(l1)) <= 1e-5 * abs(float(la)), (float(la), float(l1))


def test_refused_selfsup_batch_takes_the_per_pair_fallback(monkeypatch):
    from hplflownet_amd import engine
    from hplflownet_amd.train_plan import TrainPlan
    p1, p2, nan_sf = _pairs(('frustum', 'surface'), [(256, 256), (256, 256)], 97, sf_nan=True)
    e1, e2, esf = torch.stack(p1), torch.stack(p2), torch.stack(nan_sf)
    nat = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup', selfsup=SELFSUP, native_step=True)
    l_nat = nat.train_step_batch(e1, e2, esf, nat.gen.build_native_batch(e1, e2, for_training=True))
    fb = engine.Trainer('HPLFlowNetShallow', DEV, init='hash', loss='selfsup', selfsup=SELFSUP, native_step=True)
    monkeypatch.setattr(TrainPlan, 'tables', lambda self, lat: False)
    adam = []
    real_adam = TrainPlan.adam_step
    monkeypatch.setattr(TrainPlan, 'adam_step', lambda self, opt: adam.append(1) or real_adam(self, opt))
    l_fb = fb.train_step_batch(e1, e2, esf, fb.gen.build_native_batch(e1, e2, for_training=True))
    torch.cuda.synchronize()
    assert nat.native_steps == 1 and fb.native_steps == 0 and len(adam) == 1
    for x, y in zip(l_fb.tolist(), l_nat.tolist()):
        assert abs(x - y) <= 1e-5 * abs(y), (x, y)
    # the fallback's all-reduce: the plan's bucket order, what ranks on the native program issue, then finish
    seen = []
    fb.tplan.reducer.launch_flat = lambda b: seen.append(b)
    fb.tplan.reducer.finish_flat = lambda: seen.append('finish')
    fb.train_step_batch(e1, e2, esf, fb.gen.build_native_batch(e1, e2, for_training=True))
    assert seen == list(fb.tplan.bucket_order) + ['finish'] and len(adam) == 2


@pytest.mark.parametrize('batch', [1, 2])
def test_engine_trains_with_the_native_selfsup_step(batch, monkeypatch):
    from hplflownet_amd import engine
    epochs = []
    real_epoch = engine.Trainer.train_epoch

    def epoch(self, *a, **k):
        r = real_epoch(self, *a, **k)
        epochs.append((r, self.native_steps))
        return r
    monkeypatch.setattr(engine.Trainer, 'train_epoch', epoch)
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '256', '--pairs', '4', '--epochs', '1', '--val-pairs', '0',
                       '--loss', 'selfsup', '--selfsup-native', '--selfsup-k', '4', '--train-batch-size', str(batch)])
    (mean, steps), = epochs
    assert steps == 4 // batch and np.isfinite(mean) and np.isfinite(res)
