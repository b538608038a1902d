"""GPU: batched training -- B pairs per native training step (train_plan.TrainPlan.step_batch, engine.Trainer.train_step_batch).
The batch is one fused lattice with pair-major rows and no cross-pair edges; the unchanged training program runs on it.  Its
loss is the mean of the pairs' EPE3D and its gradient the mean of their gradients: what the single-pair step gives pair by pair,
averaged (and what W ranks of one pair each average).  The staging launch (hpl_batch_stage) and the per-pair losses
(hpl_epe3d_pairs) are pinned bit for bit."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, surface_pair, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(arch):
    import hplflownet_amd as H
    nl = 7 if arch == 'HPLFlowNet' else 5
    a = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:nl], evaluate=False, use_leaky=True, bcn_use_bias=True,
                              bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    model = getattr(H, arch)(a)
    fill_module_(model, 1.0, 'hash')
    model = model.to(DEV).train()
    gen = H.GenerateDataUnsymmetric(a, device=DEV, wide_up=model.lattice_hint())
    return model, gen


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)


def _batch(kinds, n, seed):
    """(B, 3, n) pc1, pc2, sf: pair b drawn by kinds[b] ('frustum' or 'surface')."""
    out = [[], [], []]
    for b, kind in enumerate(kinds):
        trio = (synthetic_pair if kind == 'frustum' else surface_pair)(n, seed + 7 * b)
        for j in range(3):
            out[j].append(_dev(trio[j]))
    return tuple(torch.stack(x) for x in out)


def _single_lat(gen, p1, p2):
    return gen.build_native(p1, p2).device_lattice().prepare(True)


def _run_single(plan, p1, p2, sf, lat):
    r = plan.step(p1, p2, sf, lat)
    assert r is not None
    plan.finish()
    torch.cuda.synchronize()
    return r[0][0].clone(), float(r[1]), plan.gflat.clone()


def _run_batch(plan, p1, p2, sf, lat):
    r = plan.step_batch(p1, p2, sf, lat)
    assert r is not None
    plan.finish()
    torch.cuda.synchronize()
    return r[0].clone(), float(r[1]), r[2].clone(), plan.gflat.clone()


def _grad_err(plan, model, g, ref):
    """worst (parameter, max |d| / max |ref|) over the parameters' gradients, read from two flat arenas of the plan's layout"""
    worst = ('', 0.0)
    for k, p in model.named_parameters():
        o = plan._goff[id(p)]
        a, b = g[o:o + p.numel()], ref[o:o + p.numel()]
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-20)
        if err > worst[1]:
            worst = (k, err)
    return worst


CASES = [('HPLFlowNetShallow', 512, ('frustum', 'frustum')), ('HPLFlowNetShallow', 512, ('frustum', 'surface', 'frustum', 'surface')),
         ('HPLFlowNet', 1024, ('surface', 'frustum')), ('HPLFlowNet', 1024, ('frustum',) * 4)]

#: Gradient bar of the models as they are (LeakyReLU slope 0.1).  A LeakyReLU input within fp32 rounding of 0 takes the
#: other branch when its sum is formed in another order -- and a batch of B pairs runs its GEMMs with other tiles and
#: split counts than one pair does.  One such entry moves a weight-gradient column by ~|g| / N: measured worst 6.4e-4 (default
#: mode) / 9.9e-4 (HPL_MATH=f32) of max |g| over CASES, 1.2e-3 for a batch of one pair twice.  With every activation the identity
#: (no kink; test_batched_step_is_the_mean_of_single_steps[smooth]) the same comparison stays below 1.3e-6 in both modes, so the
#: 2e-4 bar of test_native_step_matches_autograd holds there, and this one only absorbs branch flips.
KINK_BAR = 5e-3


@pytest.mark.parametrize('activation', ['smooth', 'leaky'])
@pytest.mark.parametrize('arch,n,kinds', CASES)
def test_batched_step_is_the_mean_of_single_steps(arch, n, kinds, activation, monkeypatch):
    from hplflownet_amd import bcl
    from hplflownet_amd.train_plan import TrainPlan
    if activation == 'smooth':
        monkeypatch.setattr(bcl, 'LEAKY_RATE', 1.0)          # every LeakyReLU the identity: a network without kinks
    model, gen = _model(arch)
    B = len(kinds)
    p1, p2, sf = _batch(kinds, n, 5 + B)
    plan = TrainPlan(model)
    singles = [_run_single(plan, p1[b], p2[b], sf[b], _single_lat(gen, p1[b], p2[b])) for b in range(B)]
    g_mean = sum(s[2] for s in singles) / B
    lat = gen.build_native_batch(p1, p2, for_training=True)
    assert lat.batch == B
    flow, loss, pair_losses, g = _run_batch(plan, p1, p2, sf, lat)
    assert flow.shape == (B, 3, n) and pair_losses.shape == (B,)
    flow_err = 0.0
    for b, s in enumerate(singles):
        bar = 2e-4 * max(1.0, float(s[0].abs().max()))
        err = float((flow[b] - s[0]).abs().max())
        flow_err = max(flow_err, err / max(1.0, float(s[0].abs().max())))
        assert err < bar, ('flow of pair %d' % b, err, bar)
        assert abs(float(pair_losses[b]) - s[1]) <= 1e-5 * abs(s[1]), (b, float(pair_losses[b]), s[1])
    mean_loss = sum(s[1] for s in singles) / B
    assert abs(loss - mean_loss) <= 1e-5 * abs(mean_loss), (loss, mean_loss)
    worst = _grad_err(plan, model, g, g_mean)
    print('HPL_MATH=%s %s %s n=%d B=%d: flow %.3g, loss %.3g, worst gradient %s %.3g' % (
        os.environ.get('HPL_MATH', 'default'), activation, arch, n, B, flow_err, abs(loss - mean_loss) / abs(mean_loss), worst[0],
        worst[1]))
    assert worst[1] < (2e-4 if activation == 'smooth' else KINK_BAR), worst


@pytest.mark.skipif(os.environ.get('HPL_MATH') == 'f32', reason='this test starts the f32 run itself')
def test_batched_step_is_the_mean_of_single_steps_under_f32():
    env = dict(os.environ, HPL_MATH='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-s', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_train_batch.py'), '-k', 'mean_of_single_steps and not f32'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print('\n'.join(l[l.index('HPL_MATH='):] for l in r.stdout.splitlines() if 'HPL_MATH=' in l))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '%d passed' % (2 * len(CASES)) in r.stdout, r.stdout[-2000:]


def test_epe3d_pairs_is_epe3d_of_each_pair():
    from hplflownet_amd import _lib
    from hplflownet_amd._lib import check, ptr
    lib = _lib.load()
    g = torch.Generator(device='cpu').manual_seed(3)
    for B, n in ((3, 1000), (4, 2500), (1, 1024)):
        pred = torch.randn(B * n, 3, generator=g).to(DEV)
        sf = torch.randn(3, B * n, generator=g).to(DEV)
        sf[:, 5] = pred[5]                                   # a zero-length error (the 0 / 0 branch)
        out = torch.full((B,), float('nan'), device=DEV)
        check(lib.hpl_epe3d_pairs(ptr(pred), ptr(sf), B, n, ptr(out), _lib.stream()), 'hpl_epe3d_pairs')
        for b in range(B):
            pb = pred[b * n:(b + 1) * n].contiguous()
            sb = sf[:, b * n:(b + 1) * n].contiguous()
            one = torch.full((1,), float('nan'), device=DEV)
            check(lib.hpl_epe3d(ptr(pb), ptr(sb), n, None, ptr(one), _lib.stream()), 'hpl_epe3d')
            torch.cuda.synchronize()
            assert out[b].view(torch.int32).item() == one[0].view(torch.int32).item(), (B, n, b, float(out[b]), float(one[0]))
            ref = float(torch.norm(pb.double() - sb.t().double(), dim=1).mean())
            assert abs(float(out[b]) - ref) <= 1e-6 * ref, (float(out[b]), ref)


@pytest.mark.parametrize('n1,n2', [(1001, 999), (1024, 512), (6, 10)])
def test_batch_stage_is_a_permute(n1, n2):
    from hplflownet_amd import _lib
    from hplflownet_amd._lib import check, ptr
    lib = _lib.load()
    B = 3
    g = torch.Generator(device='cpu').manual_seed(n1)
    pc1, sf = torch.randn(B, 3, n1, generator=g).to(DEV), torch.randn(B, 3, n1, generator=g).to(DEV)
    pc2 = torch.randn(B, 3, n2, generator=g).to(DEV)
    for with_sf in (True, False):
        d1, d2, ds = (torch.full((3, B * m), float('nan'), device=DEV) for m in (n1, n2, n1))
        check(lib.hpl_batch_stage(B, n1, n2, ptr(pc1), ptr(pc2), ptr(sf) if with_sf else None, ptr(d1), ptr(d2),
                                  ptr(ds) if with_sf else None, _lib.stream()), 'hpl_batch_stage')
        torch.cuda.synchronize()
        assert torch.equal(d1, torch.cat(list(pc1), dim=1)) and torch.equal(d2, pc2.permute(1, 0, 2).reshape(3, B * n2))
        if with_sf:
            assert torch.equal(ds, sf.permute(1, 0, 2).reshape(3, B * n1))
        else:
            assert bool(torch.isnan(ds).all())                 # (no sf: its destination is not touched)


def test_stale_workspace_and_staging_do_not_matter():
    """Workspace and staging buffers full of NaN give the same results; a B = 2 -> 4 -> 1 -> 2 sequence on one plan matches a
    fresh plan per batch (flow, loss and per-pair losses bit for bit, gradients as close as two clean runs are)."""
    from hplflownet_amd.train_plan import TrainPlan
    model, gen = _model('HPLFlowNetShallow')
    n = 512
    p1, p2, sf = _batch(('frustum', 'surface', 'frustum', 'frustum'), n, 40)
    lats = {B: gen.build_native_batch(p1[:B], p2[:B], for_training=True) for B in (1, 2, 4)}
    plan = TrainPlan(model)

    def run(B, fill=None):
        if fill is not None:
            torch.cuda.synchronize()
            ws = plan._ws['train']
            ws[:ws.numel() // 16 * 16].view(torch.float32).fill_(fill)
            for t in plan._stage[1]:
                t.fill_(fill)
        return _run_batch(plan, p1[:B], p2[:B], sf[:B], lats[B])

    a = run(2)
    b = run(2, float('nan'))
    c = run(2)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2]) and bool(torch.isfinite(b[3]).all())
    noise = float((c[3] - a[3]).abs().max())
    assert float((b[3] - a[3]).abs().max()) <= max(2.0 * noise, 1e-6 * float(a[3].abs().max()))
    seq = [(B, run(B)) for B in (2, 4, 1, 2)]
    del plan
    for B, r in seq:
        fresh = TrainPlan(model)
        f = _run_batch(fresh, p1[:B], p2[:B], sf[:B], lats[B])
        assert torch.equal(r[0], f[0]) and r[1] == f[1] and torch.equal(r[2], f[2]), B
        worst = _grad_err(fresh, model, r[3], f[3])
        assert worst[1] < 2e-4, (B, worst)
        del fresh


def test_batch_of_one_is_the_single_step():
    from hplflownet_amd.train_plan import TrainPlan
    model, gen = _model('HPLFlowNet')
    p1, p2, sf = _batch(('frustum',), 1024, 60)
    lat1 = gen.build_native_batch(p1, p2, for_training=True)
    assert lat1.batch == 1
    plan = TrainPlan(model)
    flow_s, loss_s, g_s = _run_single(plan, p1[0], p2[0], sf[0], lat1)
    g_s2 = _run_single(plan, p1[0], p2[0], sf[0], lat1)[2]
    flow_b, loss_b, pl, g_b = _run_batch(plan, p1, p2, sf, lat1)
    assert torch.equal(flow_b[0], flow_s) and loss_b == loss_s and float(pl[0]) == loss_s
    # (the weight-gradient slabs are summed with atomics: the arena is as close to step()'s as two step() runs are)
    assert float((g_b - g_s).abs().max()) <= max(2.0 * float((g_s2 - g_s).abs().max()), 1e-6 * float(g_s.abs().max()))


def _pairs(n, B, seed):
    p1, p2, sf = _batch(('frustum', 'surface') * (B // 2), n, seed)
    return p1, p2, sf


def test_trainer_batched_steps_match_the_autograd_loop():
    """Three Adam steps of train_step_batch on B = 2 pairs end where the autograd loop that averages the pairs' losses and steps
    once per batch ends."""
    from hplflownet_amd import engine
    p1, p2, sf = _pairs(512, 2, 70)
    tr = engine.Trainer('HPLFlowNetShallow', DEV, lr=1e-4, init='hash')
    lat = tr.gen.build_native_batch(p1, p2, for_training=True)
    native = [tr.train_step_batch(p1, p2, sf, lat).clone() for _ in range(3)]
    assert tr.native_steps == 3
    ref = engine.Trainer('HPLFlowNetShallow', DEV, lr=1e-4, init='hash', native_step=False)
    lats = [ref.gen.build(p1[b], p2[b]).prepare(True) for b in range(2)]
    auto = []
    for _ in range(3):
        ref.opt.zero_grad(set_to_none=True)
        losses = [engine.epe3d_loss(ref.model(p1[b][None], p2[b][None], lats[b]), sf[b][None]) for b in range(2)]
        (sum(losses) / 2).backward()
        ref.opt.step()
        auto.append([float(x) for x in losses])
    for a, b in zip(native, auto):
        for x, y in zip(a.tolist(), b):
            assert abs(x - y) < 2e-3 * abs(y), (x, y)
    worst = 0.0
    for (k, p), q in zip(tr.model.named_parameters(), ref.model.parameters()):
        worst = max(worst, float((p.detach() - q.detach()).abs().max()))
    print('worst weight difference after 3 steps: %.3g' % worst)
    assert worst <= 2e-4, worst


def test_refused_batch_takes_the_per_pair_fallback(monkeypatch):
    from hplflownet_amd import bcl, engine
    from hplflownet_amd.train_plan import TrainPlan
    monkeypatch.setattr(bcl, 'LEAKY_RATE', 1.0)          # (no LeakyReLU kink: the 2e-4 bar measures the semantics, see KINK_BAR)
    p1, p2, sf = _pairs(512, 2, 80)
    nat = engine.Trainer('HPLFlowNetShallow', DEV, lr=1e-4, init='hash')
    lat = nat.gen.build_native_batch(p1, p2, for_training=True)
    l_nat = nat.train_step_batch(p1, p2, sf, lat)
    torch.cuda.synchronize()
    g_nat = nat.tplan.gflat.clone()
    fb = engine.Trainer('HPLFlowNetShallow', DEV, lr=1e-4, init='hash')
    monkeypatch.setattr(TrainPlan, 'tables', lambda self, lat: False)
    seen, adam = [], []
    real_adam = TrainPlan.adam_step
    monkeypatch.setattr(TrainPlan, 'adam_step', lambda self, opt: adam.append(1) or real_adam(self, opt))
    l_fb = fb.train_step_batch(p1, p2, sf, fb.gen.build_native_batch(p1, p2, for_training=True))
    torch.cuda.synchronize()
    assert fb.native_steps == 0 and len(adam) == 1
    assert all(float(s['step']) == 1.0 for s in fb.opt.state.values())
    for a, b in zip(l_fb.tolist(), l_nat.tolist()):
        assert abs(a - b) <= 1e-5 * abs(b), (a, b)
    worst = _grad_err(fb.tplan, fb.model, fb.tplan.gflat, g_nat)
    assert worst[1] < 2e-4, worst
    # the fallback's all-reduce: the plan's bucket order, what ranks on the native program issue
    fb.tplan.reducer.launch_flat = lambda b: seen.append(b)
    fb.tplan.reducer.finish_flat = lambda: seen.append('finish')
    fb.train_step_batch(p1, p2, sf, fb.gen.build_native_batch(p1, p2, for_training=True))
    assert seen == list(fb.tplan.bucket_order) + ['finish']


def test_engine_trains_in_batches(monkeypatch, capsys):
    from hplflownet_amd import engine
    pair_losses, epochs = [], []
    real_step, real_epoch = engine.Trainer.train_step_batch, engine.Trainer.train_epoch

    def step(self, *a):
        r = real_step(self, *a)
        pair_losses.extend(r.tolist())
        return r

    def epoch(self, *a, **k):
        r = real_epoch(self, *a, **k)
        epochs.append((r, self.native_steps))
        return r
    monkeypatch.setattr(engine.Trainer, 'train_step_batch', step)
    monkeypatch.setattr(engine.Trainer, 'train_epoch', epoch)
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--pairs', '4', '--train-batch-size', '2', '--epochs', '1',
                       '--val-pairs', '0'])
    assert len(pair_losses) == 4 and all(np.isfinite(pair_losses))
    (mean, steps), = epochs
    assert steps == 2                                   # two native steps of two pairs
    assert abs(mean - sum(pair_losses) / 4) <= 1e-6 * abs(mean)
    assert np.isfinite(res) and abs(res - mean) <= 1e-12 + 1e-9 * abs(mean)
