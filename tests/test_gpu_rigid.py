"""GPU: hpl_rigid_fit / ops.rigid_fit, flownet.rigid_refine and engine --evaluate --rigid-refine.

The kernel takes the rotation from Horn's quaternion by Jacobi sweeps; tests/rigid_oracle.py takes it from a float64 SVD.  R, t
and the residuals are held within the larger of (a) what the restatement's own float32 mode loses against its float64 mode on
that input and (b) a float32 output floor: 8 * 2^-24 for entries of R, 8 * 2^-24 * max(|p| + |f|) for t and lengths.  Inlier
masks are compared exactly: tests/test_rigid_cpu.py shows that no residual of these scenes lies within 1e-4 of tau."""
import os

import numpy as np
import pytest
import torch

from batch64 import counts64, prefix_of
from rigid_oracle import base_weights, fit, rotation, scene, weights
from test_rigid_cpu import CASES, mirror_scene

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TAU = 0.1
EPS = 8 * 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run(p, f, w=None, iters=4, tau=TAU, prefix=None):
    from hplflownet_amd import ops
    out = ops.rigid_fit(dev(p), dev(f), None if w is None else dev(w), iters=iters, tau=tau, prefix=prefix, return_residual=True)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def proper(R):
    R = R.double().cpu().numpy()
    return np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0


_ORACLE = {}


def oracle(n, seed, weighted, iters):
    """The scene, its weights and the restatement's two modes, computed once per case."""
    key = (n, seed, weighted, iters)
    if key not in _ORACLE:
        p, f, _ = scene(n, seed)
        w = weights(n, seed) if weighted else None
        _ORACLE[key] = (p, f, w, fit(p, f, w, iters, TAU, np.float64), fit(p, f, w, iters, TAU, np.float32))
    return _ORACLE[key]


def compare(got, p, f, w, o64, o32, what):
    R, t, stats, refined, residual = [x.cpu().numpy() for x in got]
    scale = float((np.abs(p) + np.abs(f)).max())
    bar_R = max(float(np.abs(o32['R'] - o64['R']).max()), EPS)
    bar_t = max(float(np.abs(o32['t'] - o64['t']).max()), EPS * scale)
    bar_r = max(float(np.abs(o32['residual'] - o64['residual']).max()), EPS * scale)
    eR, et = float(np.abs(R[0] - o64['R']).max()), float(np.abs(t[0] - o64['t']).max())
    er = float(np.abs(residual - o64['residual']).max())
    print('%s: |R - oracle| %.3g (bar %.3g, float32 mode %.3g)  |t - oracle| %.3g (bar %.3g, float32 mode %.3g)  '
          '|residual - oracle| %.3g (bar %.3g)' % (what, eR, bar_R, float(np.abs(o32['R'] - o64['R']).max()), et, bar_t,
                                                   float(np.abs(o32['t'] - o64['t']).max()), er, bar_r))
    assert stats[0, 0] == o64['status'] == 1
    assert eR <= bar_R and et <= bar_t and er <= bar_r, what
    assert proper(got[0][0])
    mask = o64['inlier']
    assert np.array_equal((residual <= np.float32(TAU)) & (base_weights(p, f, w) > 0), mask)
    assert abs(stats[0, 1] - o64['share']) <= 2.0 ** -23
    assert abs(stats[0, 2] - o64['angle_deg']) <= max(np.degrees(2 * bar_R), 1e-5) and abs(stats[0, 3] - o64['trans']) <= 2 * bar_t
    # refined: the rigid flow on the inliers within the bar, the input flow's bits everywhere else
    assert float(np.abs(refined[mask] - o64['refined'][mask]).max(initial=0)) <= bar_r
    assert np.array_equal(refined[~mask].view(np.int32), f.T[~mask].view(np.int32))
    assert mask.any() and (refined[mask] != f.T[mask]).any()


@pytest.mark.parametrize('n,seed', CASES)
@pytest.mark.parametrize('iters', [0, 4])
@pytest.mark.parametrize('weighted', [False, True])
def test_against_the_restatement(n, seed, iters, weighted):
    p, f, w, o64, o32 = oracle(n, seed, weighted, iters)
    got = run(p, f, w, iters)
    if iters == 0 and not o64['inlier'].any():                          # a least-squares fit of a scene with movers: no inlier
        R, t, stats, refined, residual = [x.cpu().numpy() for x in got]
        assert stats[0, 1] == 0 and np.array_equal(refined.view(np.int32), f.T.copy().view(np.int32))
        scale = float((np.abs(p) + np.abs(f)).max())
        assert np.abs(R[0] - o64['R']).max() <= max(float(np.abs(o32['R'] - o64['R']).max()), EPS)
        assert np.abs(t[0] - o64['t']).max() <= max(float(np.abs(o32['t'] - o64['t']).max()), EPS * scale)
        assert np.abs(residual - o64['residual']).max() <= max(float(np.abs(o32['residual'] - o64['residual']).max()), EPS * scale)
        assert proper(got[0][0]) and stats[0, 0] == 1
        return
    compare(got, p, f, w, o64, o32, 'N = %d iters %d weighted %s' % (n, iters, weighted))


def test_reflection_and_collinear_clouds_give_rotations():
    p, f = mirror_scene()
    got = run(p, f, None, 0)
    o = fit(p, f, None, 0, TAU)
    assert proper(got[0][0]) and float(got[2][0, 0]) == 1
    assert np.abs(got[0][0].cpu().numpy() - o['R']).max() <= 1e-6       # (a 180 degree turn about the in-plane axis)
    assert abs(float(got[2][0, 2]) - 180.0) <= 0.1
    # a collinear cloud under an exact motion: the turn about the line is free; any proper R that maps the line fits every point
    s = np.linspace(-10, 10, 300)
    p = (np.array([[1.0], [0.5], [20.0]]) + np.array([[0.6], [0.1], [0.79]]) * s).astype(np.float32)
    q = rotation((0.1, 1.0, 0.05), 0.03) @ p.astype(np.float64) + np.array([[0.05], [-0.02], [-0.9]])
    f = (q - p).astype(np.float32)
    for iters in (0, 4):
        R, t, stats, refined, residual = run(p, f, None, iters)
        assert proper(R[0]) and bool(torch.isfinite(t).all())
        # the inputs are float32 roundings of an exact motion (<= 2^-24 * 36 m each): the fit's residuals stay at that scale
        assert float(residual.max()) <= 1e-4 and float(stats[0, 1]) == 1.0


COUNTS = (37, 1000, 3, 4099, 256)


def ragged_inputs():
    parts = [scene(n, 70 + i) for i, n in enumerate(COUNTS)]
    p = np.concatenate([x[0] for x in parts], 1)
    f = np.concatenate([x[1] for x in parts], 1)
    w = np.concatenate([weights(n, 70 + i) for i, n in enumerate(COUNTS)])
    prefix = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
    return parts, p, f, w, prefix


@pytest.mark.parametrize('weighted', [False, True])
def test_ragged_batches_equal_their_pairs(weighted):
    parts, p, f, w, prefix = ragged_inputs()
    w = w if weighted else None
    R, t, stats, refined, residual = run(p, f, w, 4, prefix=prefix)
    for b, n in enumerate(COUNTS):
        sl = slice(prefix[b], prefix[b + 1])
        one = run(p[:, sl], f[:, sl], None if w is None else w[sl], 4)
        assert same(one, (R[b:b + 1], t[b:b + 1], stats[b:b + 1], refined[sl], residual[sl])), b
        assert same(one, run(p[:, sl], f[:, sl], None if w is None else w[sl], 4, prefix=[0, n])), b      # B = 1 with a prefix
        o = fit(p[:, sl], f[:, sl], None if w is None else w[sl], 4, TAU)
        assert np.abs(R[b].cpu().numpy() - o['R']).max() <= 1e-6 and float(stats[b, 0]) == 1
        assert abs(float(stats[b, 1]) - o['share']) <= 2.0 ** -23
    # pairs in another order and with an empty pair between them: every pair keeps its bits
    order = [3, 0, 4]
    q = np.concatenate([p[:, prefix[b]:prefix[b + 1]] for b in order], 1)
    g = np.concatenate([f[:, prefix[b]:prefix[b + 1]] for b in order], 1)
    pre = [0, COUNTS[3], COUNTS[3], COUNTS[3] + COUNTS[0], COUNTS[3] + COUNTS[0] + COUNTS[4]]
    R2, t2, stats2, refined2, residual2 = run(q, g, None, 4, prefix=pre)
    if w is None:
        for j, b in zip((0, 2, 3), order):
            assert same((R[b], t[b], stats[b]), (R2[j], t2[j], stats2[j]))
            assert same((refined[prefix[b]:prefix[b + 1]],), (refined2[pre[j]:pre[j + 1]],))
    assert stats2[1].tolist() == [0, 0, 0, 0] and torch.equal(R2[1].cpu(), torch.eye(3)) and not bool(t2[1].any())


def test_a_batch_of_64_pairs_equals_its_pairs():
    """B = 64 (tests/batch64.py): every pair's outputs are the bits of that pair run alone with prefix = [0, n], and its fit
    is the restatement's within the bars of the ragged test above; a pair of fewer than 3 points has status 0."""
    counts = counts64()
    prefix = prefix_of(counts)
    parts = [scene(n, 200 + i) for i, n in enumerate(counts)]
    p, f = np.concatenate([x[0] for x in parts], 1), np.concatenate([x[1] for x in parts], 1)
    R, t, stats, refined, residual = run(p, f, None, 4, prefix=prefix)
    for b, n in enumerate(counts):
        sl = slice(prefix[b], prefix[b + 1])
        one = run(p[:, sl], f[:, sl], None, 4, prefix=[0, n])
        assert same(one, (R[b:b + 1], t[b:b + 1], stats[b:b + 1], refined[sl], residual[sl])), b
        o = fit(p[:, sl], f[:, sl], None, 4, TAU)
        assert float(stats[b, 0]) == o['status'] == (1 if n >= 3 else 0), b
        assert np.abs(R[b].cpu().numpy() - o['R']).max() <= 1e-6 and abs(float(stats[b, 1]) - o['share']) <= 2.0 ** -23, b
        if n < 3:
            assert torch.equal(R[b].cpu(), torch.eye(3)) and not bool(t[b].any())
            assert same((refined[sl],), (dev(f[:, sl].T),)), b


def test_strided_inputs_are_read_in_place():
    from hplflownet_amd import ops
    n, B, nmax = 1000, 3, 1500
    p, f, _ = scene(n, 5)
    want = ops.rigid_fit(dev(p), dev(f), return_residual=True)
    rows = dev(f.T.copy())                                              # the forward's point-major [N, 3] rows
    assert same(want, ops.rigid_fit(dev(p), rows, return_residual=True))
    assert same(want, ops.rigid_fit(dev(p), rows.t(), return_residual=True))          # its (3, N) view, strides (1, 3)
    wide_p = torch.full((B, 3, nmax), float('nan'), device=DEV)
    wide_f = torch.full((B, 3, nmax), float('nan'), device=DEV)
    wide_p[1, :, 7:7 + n] = dev(p)
    wide_f[1, :, 7:7 + n] = dev(f)
    a, b = wide_p[1][:, 7:7 + n], wide_f[1][:, 7:7 + n]
    assert not a.is_contiguous() and a.stride(0) == nmax
    assert same(want, ops.rigid_fit(a, b, return_residual=True))
    out = torch.empty((n, 3), device=DEV)
    res = ops.rigid_fit(a, b, out=out)
    assert res[3] is out and torch.equal(out, want[3])
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide_p[1][:, :7]).all()) and bool(torch.isnan(wide_f[1][:, 7 + n:]).all())
    # a padded batch through the convenience call: one fit per pair, pair 1 the one above
    import hplflownet_amd as H
    for i in (0, 2):
        pi, fi, _ = scene(nmax, 20 + i)
        wide_p[i], wide_f[i] = dev(pi), dev(fi)
    R, t, stats, refined = H.rigid_refine(wide_p[:, :, 7:7 + n], wide_f[:, :, 7:7 + n])
    assert refined.shape == (B, 3, n) and same((R[1], t[1], stats[1], refined[1].t()), (want[0][0], want[1][0], want[2][0], want[3]))
    lists = H.rigid_refine([wide_p[i][:, 7:7 + n] for i in range(B)], [wide_f[i][None, :, 7:7 + n] for i in range(B)])
    assert same((R, t, stats), lists[:3]) and all(x.shape == (1, 3, n) and torch.equal(x[0], refined[i]) for i, x in enumerate(lists[3]))


def test_degenerate_inputs():
    from hplflownet_amd import ops
    p, f, _ = scene(500, 9)
    eye = torch.eye(3)

    def failed(R, t, stats, refined, residual, ff):
        assert torch.equal(R.cpu(), eye) and not bool(t.any()) and stats.tolist() == [0, 0, 0, 0]
        assert torch.equal(bits(refined).cpu(), bits(dev(ff.T.copy())).cpu())
        assert bool(torch.isfinite(residual).all())
        assert np.abs(residual.cpu().numpy() - np.linalg.norm(ff.astype(np.float64), axis=0)).max() <= EPS * 2
    for w in (np.zeros(500, np.float32), np.full(500, np.nan, np.float32), np.full(500, -1.0, np.float32),
              np.full(500, np.inf, np.float32)):
        for iters in (0, 4):
            R, t, stats, refined, residual = run(p, f, w, iters)
            failed(R[0], t[0], stats[0], refined, residual, f)
    for n in (1, 2):                                                    # fewer than three points carry no rigid fit
        R, t, stats, refined, residual = run(p[:, :n], f[:, :n], None, 4)
        failed(R[0], t[0], stats[0], refined, residual, f[:, :n])
    # inside a batch: the failed pairs do not touch their neighbours
    pre = [0, 1, 200, 200, 500]
    wz = np.ones(500, np.float32)
    R, t, stats, refined, residual = run(p, f, wz, 4, prefix=pre)
    failed(R[0], t[0], stats[0], refined[:1], residual[:1], f[:, :1])
    assert stats[2].tolist() == [0, 0, 0, 0] and torch.equal(R[2].cpu(), eye)
    assert same((R[1], t[1], stats[1], refined[1:200]), [x[0] if i < 3 else x for i, x in enumerate(run(p[:, 1:200], f[:, 1:200], None, 4)[:4])])
    assert stats[:, 0].tolist() == [0, 1, 0, 1]
    assert ops.rigid_fit(dev(p[:, :0]), dev(f[:, :0]), prefix=[0, 0, 0])[2].tolist() == [[0, 0, 0, 0]] * 2      # N = 0: no launch


def test_points_with_nan_flow_take_no_part():
    p, f, static = scene(1000, 12)
    bad = np.array([0, 17, 500, 998, 999])
    fb, pb = f.copy(), p.copy()
    fb[0, bad[:2]] = np.nan
    fb[2, bad[2]] = np.inf
    pb[1, bad[3:]] = np.nan
    keep = np.ones(1000, bool)
    keep[bad] = False
    R, t, stats, refined, residual = run(pb, fb, None, 4)
    o = fit(p[:, keep], f[:, keep], None, 4, TAU)
    o32 = fit(p[:, keep], f[:, keep], None, 4, TAU, np.float32)
    scale = float((np.abs(p) + np.abs(f)).max())
    assert np.abs(R[0].cpu().numpy() - o['R']).max() <= max(float(np.abs(o32['R'] - o['R']).max()), EPS)
    assert np.abs(t[0].cpu().numpy() - o['t']).max() <= max(float(np.abs(o32['t'] - o['t']).max()), EPS * scale)
    got = refined.cpu().numpy()
    assert np.array_equal(got[bad].view(np.int32), fb.T[bad].view(np.int32))                 # their rows: the input bits
    assert np.array_equal(residual.cpu().numpy()[keep] <= np.float32(TAU), o['inlier'])
    assert abs(float(stats[0, 1]) - o['inlier'].sum() / 1000.0) <= 2.0 ** -23
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all()) and bool(torch.isfinite(stats).all())
    assert same((R, t), run(pb, fb, np.ones(1000, np.float32), 4)[:2])                       # unit weights: the NULL path's bits


def test_same_bits_twice_and_beside_a_busy_stream():
    parts, p, f, w, prefix = ragged_inputs()
    big = scene(300000, 2)                                              # ~ 290 workgroups a pair: their partials in a fixed order
    first = run(p, f, w, 4, prefix=prefix)
    bfirst = run(big[0], big[1], None, 4)
    again = run(p, f, w, 4, prefix=prefix)
    assert same(first, again)
    from hplflownet_amd import ops
    tp, tf, tw, bp, bf = dev(p), dev(f), dev(w), dev(big[0]), dev(big[1])
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            a = torch.tanh(a @ a * 1e-3)
    busy = ops.rigid_fit(tp, tf, tw, iters=4, tau=TAU, prefix=prefix, return_residual=True)       # (no synchronisation between)
    bbusy = ops.rigid_fit(bp, bf, iters=4, tau=TAU, return_residual=True)
    torch.cuda.synchronize()
    assert same(first, busy) and same(bfirst, bbusy)
    o = fit(big[0], big[1], None, 4, TAU)
    assert np.abs(bfirst[0][0].cpu().numpy() - o['R']).max() <= EPS and np.array_equal(
        bfirst[4].cpu().numpy() <= np.float32(TAU), o['inlier'])


# ----------------------------------------------------------------------------- engine --evaluate --rigid-refine
ARGS = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate']
RIGID = ['rigid_inliers', 'rigid_angle_deg', 'rigid_trans']


def rigid_tree(root, counts, kitti=False):
    """Frames whose ground-truth flow is ONE rigid motion: FlyingThings3D-style (the reader takes every fourth directory and
    stores x and z with the opposite sign) or KITTI-style (every directory, as stored)."""
    R = rotation((0.1, 1.0, 0.05), 0.03)
    for i, n in enumerate(counts):
        d = os.path.join(root, 'KITTI_processed_occ_final', '%06d' % i) if kitti else \
            os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        rng = np.random.RandomState(300 + i)
        pc = np.stack([rng.uniform(-5, 5, n), rng.uniform(-1, 1, n), rng.uniform(3, 30, n)], 1)
        flip = np.array([1, 1, 1] if kitti else [-1, 1, -1], np.float64)
        np.save(os.path.join(d, 'pc1.npy'), (pc * flip).astype(np.float32))
        np.save(os.path.join(d, 'pc2.npy'), ((pc @ R.T + np.array([0.05, -0.02, -0.4])) * flip).astype(np.float32))


def close(a, b, keys):
    for k in keys:
        assert abs(a[k] - b[k]) <= 2e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])


def test_engine_rigid_refine_single_batched_and_by_hand(tmp_path):
    from hplflownet_amd import data as data_mod
    from hplflownet_amd import engine, ops
    root = str(tmp_path)
    rigid_tree(root, [700] * 13)                                        # 4 samples, more than --points: equal sampled counts
    args = ARGS + ['--dataset', 'FlyingThings3DSubset', '--data-root', root]
    plain = engine.main(args)
    one = engine.main(args + ['--rigid-refine'])
    four = engine.main(args + ['--rigid-refine', '--batch-size', '4'])
    assert list(one) == list(plain) + ['rigid_' + k for k in plain] + RIGID and list(four) == list(one)
    assert all(one[k] == plain[k] for k in plain)                       # the keys of before: exactly the run without the flag
    close(one, four, list(one))
    assert all(np.isfinite(v) for v in one.values()) and 0 <= one['rigid_inliers'] <= 1
    other = engine.main(args + ['--rigid-refine', '--rigid-iters', '0', '--rigid-tau', '0.5'])
    assert all(other[k] == plain[k] for k in plain) and other['rigid_trans'] != one['rigid_trans']
    # by hand: the engine's own reader and model, then ops.rigid_fit and the metrics op
    tr = engine.Trainer('HPLFlowNetShallow', torch.device('cuda', torch.cuda.current_device()))
    tr.model.eval()
    reader = data_mod.FlyingThings3DSubset(False, data_mod.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root, device=tr.device)
    sums = torch.zeros((len(reader), 8), dtype=torch.float64, device=DEV)
    stats = []
    with torch.no_grad():
        for i in range(len(reader)):
            s_ = reader[i]
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))
            _, _, st, refined = ops.rigid_fit(s_[0], flow[0], iters=4, tau=0.1)
            stats.append(st[0].cpu().numpy())
            ops.flow_metrics_pairs([refined.t()], [s_[2]], [s_[0]], [getattr(s_, 'camera', None)], sums, i)
        words = sums.cpu().numpy()
    folds = [ops.flow_metrics_fold(w, bool(getattr(reader, 'has_cameras', False))) for w in words]
    for k in plain:
        assert one['rigid_' + k] == sum(x[k] for x in folds) / len(folds), k
    for j, k in enumerate(RIGID):
        assert one[k] == sum(float(s[1 + j]) for s in stats) / len(stats), k


def test_engine_rigid_refine_ragged_kitti(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    rigid_tree(root, [300, 450, 380, 500], kitti=True)                  # short frames: every pair keeps its own count
    args = ARGS + ['--dataset', 'KITTI', '--data-root', root, '--rigid-refine']
    one = engine.main(args)
    ragged = engine.main(args + ['--batch-size', '4', '--ragged'])
    assert list(one) == list(ragged) and 'rigid_EPE3D' in one and 'rigid_trans' in one
    close(one, ragged, list(one))


class _Truth(torch.nn.Module):
    """A stand-in model: the ground-truth flow plus noise, with a block of movers."""

    def __init__(self, samples, movers):
        super().__init__()
        self.samples, self.movers, self.i = samples, movers, 0

    def forward(self, p1, p2, lat):
        s_ = self.samples[self.i]
        self.i += 1
        g = torch.Generator(device='cpu').manual_seed(self.i)
        flow = s_[2] + (0.01 * torch.randn(s_[2].shape, generator=g)).to(DEV)
        flow[:, :self.movers] += torch.tensor([[1.0], [0.0], [0.5]], device=DEV)
        return flow.t().contiguous().t()[None]                          # (1, 3, N) with point-major rows, as the models return


class _Rigid(list):
    has_cameras = False


def test_validate_refines_a_noisy_rigid_flow():
    from hplflownet_amd import engine
    R = torch.from_numpy(rotation((0.1, 1.0, 0.05), 0.03)).float()
    data = _Rigid()
    for i in range(3):
        p, _, _ = scene(1024, 40 + i, movers=0)
        p1 = dev(p)
        sf = (R.to(DEV) @ p1 + torch.tensor([[0.05], [-0.02], [-0.9]], device=DEV)) - p1
        data.append((p1, p1 + sf, sf))
    tr = engine.Trainer('HPLFlowNetShallow', torch.device('cuda', torch.cuda.current_device()))
    tr.model = _Truth(data, 256)
    tr._lattices = lambda d, order, train, **kw: ((d[i], None) for i in order)          # no lattice: the stand-in takes none
    res = tr.validate(data, rigid={'iters': 4, 'tau': 0.1})
    print(res)
    assert res['rigid_inliers'] == 0.75                                 # the static share: 768 of 1024 in every pair
    assert res['rigid_EPE3D'] < res['EPE3D']
    # the inliers' error is the fit's, far below the noise; the movers keep theirs: 0.25 * |(1, 0, 0.5)| and a little noise
    assert abs(res['rigid_EPE3D'] - 0.25 * np.hypot(1.0, 0.5)) <= 0.01
    assert abs(res['rigid_angle_deg'] - np.degrees(0.03)) <= 0.02 and abs(res['rigid_trans'] - np.linalg.norm([0.05, -0.02, -0.9])) <= 0.01
