"""GPU: hpl_icp_plane / ops.icp(metric='plane') / icp_register(metric='plane') against the numpy restatement
tests/icp_plane_oracle.py on pairs whose src and dst are drawn INDEPENDENTLY from the same surfaces.  The bars are those of
tests/test_gpu_icp.py: the larger of the restatement's own float32-mode loss and 8 x 2^-24 (x scale for t and lengths), taken
from the restatement, never from the device.  The normals of the round tests come from the restatement of hpl_normals, so an
error of the normals cannot hide here."""
import numpy as np
import pytest
import torch

import icp_oracle as P
import icp_plane_oracle as O
import normals_oracle as NO
from batch64 import counts64, prefix_of

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 8 * 2.0 ** -24
MD, TAU = 1.0, 0.3
DRIFT = 6 * 2.0 ** -24                            # per round and entry of R^T R - I: the bound include/hpl_bcl.h states


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def init_of(motion, B=1):
    if motion is None:
        return None
    ms = motion if isinstance(motion, list) else [motion] * B
    return dev(np.stack([m[0] for m in ms])), dev(np.stack([m[1] for m in ms]))


def run(src, dst, nrm, w=None, init=None, iters=0, sp=None, dp=None, metric='plane', **kw):
    from hplflownet_amd import ops
    B = 1 if sp is None else len(sp) - 1
    extra = dict(metric='plane', dst_normal=nrm if torch.is_tensor(nrm) else dev(nrm)) if metric == 'plane' else {}
    out = ops.icp(dev(src), dev(dst), None if w is None else dev(w), init_of(init, B), iters=iters, max_dist=kw.pop('max_dist', MD),
                  tau=kw.pop('tau', TAU), src_prefix=sp, dst_prefix=dp, return_matches=True, **extra, **kw)
    torch.cuda.synchronize()
    return out                                   # R, t, stats, flow, match, dist2


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def motion_of(got, b=0):
    return got[0][b].cpu().numpy(), got[1][b].cpu().numpy()


_PAIRS = {}


def pair(n, radius=1.0, seed=None):
    """(src, dst, the restatement's normals of dst at k = 16), once per size."""
    key = (n, radius, seed)
    if key not in _PAIRS:
        src, dst = O.pair(n, n if seed is None else seed)
        _PAIRS[key] = (src, dst, NO.normals(dst, 16, radius)['normal'])
    return _PAIRS[key]


# ----------------------------------------------------------------------------- 1. one round
def bars(src, dst, nrm, w, R0, t0, matched=None, md=MD):
    matched = P.match(src, dst, R0, t0, md) if matched is None else matched
    o64 = O.round_(src, dst, nrm, R0, t0, w, md, TAU, np.float64, matched)
    o32 = O.round_(src, dst, nrm, R0, t0, w, md, TAU, np.float32, matched)
    scale = float(max(np.abs(src[np.isfinite(src)]).max(), np.abs(dst[np.isfinite(dst)]).max()))
    dR, dt = float(np.abs(o32['R'] - o64['R']).max()), float(np.abs(o32['t'] - o64['t']).max())
    return o64, max(dR, EPS), max(dt, EPS * scale), scale, (dR, dt)


def check_round(got, src, dst, nrm, w, R0, t0, what, matched=None, md=MD):
    """One device round from (R0, t0) against the restatement; the finish (every point-to-point match) against icp_oracle's."""
    o64, bar_R, bar_t, scale, (dR, dt) = bars(src, dst, nrm, w, R0, t0, matched, md)
    R, t = motion_of(got)
    stats = got[2][0].cpu().numpy()
    eR, et = float(np.abs(R - o64['R']).max()), float(np.abs(t - o64['t']).max())
    print('%s: |R - oracle| %.3g (bar %.3g, float32 mode %.3g)  |t - oracle| %.3g (bar %.3g, float32 mode %.3g)' % (
        what, eR, bar_R, dR, et, bar_t, dt))
    assert o64['ok'] and stats[0] == 1 and stats[5] == 1
    assert eR <= bar_R and et <= bar_t, what
    fm = P.match(src, dst, R, t, md)
    f64 = P.finish(src, dst, R, t, w, md, np.float64, fm)
    f32 = P.finish(src, dst, R, t, w, md, np.float32, fm)
    assert np.array_equal(got[4].cpu().numpy(), f64['match'])
    assert np.array_equal(got[5].cpu().numpy().view(np.int32), f64['dist2'].view(np.int32))
    assert abs(stats[1] - f64['share']) <= 2.0 ** -23
    assert abs(stats[2] - f64['rmse']) <= max(abs(f32['rmse'] - f64['rmse']), EPS * scale)
    return fm


@pytest.mark.parametrize('n,radius', [(300, 2.0), (1025, 1.0), (3000, 1.0)])
@pytest.mark.parametrize('weighted', [False, True])
def test_one_round_against_the_restatement(n, radius, weighted):
    src, dst, nrm = pair(n, radius)
    w = P.weights(n, n) if weighted else None
    for name, motion in (('identity', P.IDENTITY), ('truth', (P.TRUE_R.astype(np.float32), P.TRUE_T.astype(np.float32)))):
        got = run(src, dst, nrm, w, motion, iters=1)
        check_round(got, src, dst, nrm, w, motion[0], motion[1], 'N = %d weighted %s from %s' % (n, weighted, name))


# ----------------------------------------------------------------------------- 2. chaining and lockstep
@pytest.mark.parametrize('weighted', [False, True])
def test_three_rounds_equal_three_chained_calls(weighted):
    src, dst, nrm = pair(1025)
    w = P.weights(1025, 5) if weighted else None
    whole = run(src, dst, nrm, w, None, iters=3)
    step, motion = None, None
    for _ in range(3):
        step = run(src, dst, nrm, w, motion, iters=1)
        motion = motion_of(step)
    assert whole[2][0, 5] == 3 and step[2][0, 5] == 1
    assert same(whole[:2] + (whole[2][:, :5],) + whole[3:], step[:2] + (step[2][:, :5],) + step[3:])
    assert not np.array_equal(motion[0], np.eye(3, dtype=np.float32))


def test_eight_rounds_in_lockstep_with_the_restatement():
    src, dst, nrm = pair(1025)
    motion = P.IDENTITY
    matched = P.match(src, dst, *motion, MD)
    assert np.array_equal(run(src, dst, nrm, iters=0)[4].cpu().numpy(), matched[0])
    for k in range(8):
        got = run(src, dst, nrm, None, motion, iters=1)
        matched = check_round(got, src, dst, nrm, None, motion[0], motion[1], 'round %d' % k, matched)
        motion = motion_of(got)


# ----------------------------------------------------------------------------- 3. convergence
def off_truth(R, t):
    return float(np.abs(np.asarray(R, np.float64) - P.TRUE_R).max()), float(np.abs(np.asarray(t, np.float64) - P.TRUE_T).max())


@pytest.mark.parametrize('n', [1025, 3000])
def test_convergence_from_identity_on_the_independently_sampled_scene(n):
    src, dst, nrm = pair(n)
    ref = O.chain(src, dst, nrm, iters=30)
    refR, reft = off_truth(ref['R32'], ref['t32'])
    point = P.chain(src, dst, iters=30)
    ptR, ptt = off_truth(point['R32'], point['t32'])
    assert ref['status'] == 1 and ref['rounds'] < 30
    # the restatement: point-to-plane ends nearer the true translation -- the error the issue's table gives, in mm -- than 30
    # point-to-point rounds do.  (The rotation's error is printed: at n = 1 025 both are about 1e-3 and either may be the larger.)
    assert reft < ptt
    _, bar_R, bar_t, _, _ = bars(src, dst, nrm, None, ref['R32'], ref['t32'])
    got = run(src, dst, nrm, iters=30)
    rounds = int(got[2][0, 5])
    eR, et = off_truth(*motion_of(got))
    dpt = run(src, dst, None, iters=30, metric='point')
    dR, dt_ = off_truth(*motion_of(dpt))
    print('N = %d: plane %d rounds (restatement %d), R off truth by %.3g (restatement %.3g), t by %.3g (%.3g); point %d rounds, '
          'R off by %.3g (restatement %.3g), t by %.3g (%.3g)' % (n, rounds, ref['rounds'], eR, refR, et, reft, int(dpt[2][0, 5]),
                                                                   dR, ptR, dt_, ptt))
    assert got[2][0, 0] == 1 and rounds == ref['rounds']
    assert eR <= 2 * refR + bar_R and et <= 2 * reft + bar_t
    assert et < dt_                              # the same inequality on the device
    assert same(run(src, dst, nrm, None, motion_of(got), iters=1)[:2], got[:2])       # a fixpoint


# ----------------------------------------------------------------------------- 4. degenerate and special cases
def test_a_single_plane_leaves_the_unobserved_directions_alone():
    """Both clouds on the plane y = const, normals (0, 1, 0): the columns of J for the rotation about y and the slides along x
    and z are exactly zero, so are their eigenvalues, and the step has no such component."""
    rng = np.random.RandomState(4)
    src = np.stack([rng.uniform(-4, 4, 900), np.full(900, -1.5), rng.uniform(4, 12, 900)]).astype(np.float32)
    dst = np.stack([rng.uniform(-4, 4, 900), np.full(900, -1.25), rng.uniform(4, 12, 900)]).astype(np.float32)
    nrm = np.tile(np.array([[0.0], [1.0], [0.0]], np.float32), (1, 900))
    o = O.round_(src, dst, nrm, *P.IDENTITY)
    assert o['ok'] and np.abs(o['x'][[1, 3, 5]]).max() <= 1e-12 and (np.abs(o['lam'][:3]) <= O.RANK * o['lam'][-1]).all()
    got = run(src, dst, nrm, None, None, iters=1)
    check_round(got, src, dst, nrm, None, *P.IDENTITY, 'single plane')
    end = run(src, dst, nrm, iters=30)
    R, t = motion_of(end)
    assert end[2][0, 0] == 1 and np.isfinite(R).all() and np.isfinite(t).all()
    # every residual is t_y - 0.25 exactly, so (I, (0, 0.25, 0)) solves the round exactly: nothing slides, nothing turns
    assert np.abs(t - np.array([0, 0.25, 0])).max() <= EPS * 12 and np.abs(R - np.eye(3)).max() <= EPS


def test_invalid_normals_take_no_part():
    src, dst, nrm = pair(1025)
    bad = nrm.copy()
    bad[:, 0::3] = 0
    bad[1, 1::7] = np.nan
    bad[0, 2::11] = np.inf
    got = run(src, dst, bad, None, None, iters=1)
    check_round(got, src, dst, bad, None, *P.IDENTITY, 'a third of the normals invalid')
    m = got[4].cpu().numpy()                     # (equal to the point-to-point finish: check_round)
    assert (~O.valid_normals(bad))[m[m >= 0]].sum() > 100           # the finish reports the matches on invalid normals too
    init = (P.TRUE_R.astype(np.float32), P.TRUE_T.astype(np.float32))
    for none in (np.zeros_like(nrm), np.full_like(nrm, np.nan)):
        dead = run(src, dst, none, None, init, iters=5)
        assert dead[2][0, 0] == 0 and dead[2][0, 5] == 1
        assert np.array_equal(motion_of(dead)[0], init[0]) and np.array_equal(motion_of(dead)[1], init[1])
        assert not O.chain(src, dst, none, init=init, iters=5)['status']


def test_the_rotation_stays_proper_within_the_stated_drift():
    src, dst, nrm = pair(3000)
    got = run(src, dst, nrm, P.weights(3000, 9), None, iters=30)
    R = motion_of(got)[0].astype(np.float64)
    rounds = int(got[2][0, 5])
    drift = np.abs(R.T @ R - np.eye(3)).max()
    print('%d rounds: |R^T R - I| %.3g (bound %.3g)' % (rounds, drift, 30 * DRIFT))
    assert got[2][0, 0] == 1 and drift <= 30 * DRIFT and np.linalg.det(R) > 0


# ----------------------------------------------------------------------------- 5. bits and wrappers
def batch_equals_pairs(ns, ms, iters=4):
    from hplflownet_amd import ops
    parts = [O.pair(max(n, m, 1), 40 + i) for i, (n, m) in enumerate(zip(ns, ms))]
    srcs, dsts = [p[0][:, :n] for p, n in zip(parts, ns)], [p[1][:, :m] for p, m in zip(parts, ms)]
    sp, dp = prefix_of(list(ns)), prefix_of(list(ms))
    src, dst = np.concatenate(srcs, 1), np.concatenate(dsts, 1)
    nrm = ops.normals(dev(dst), k=8, radius=2.0, prefix=dp)[0]
    got = run(src, dst, nrm, None, None, iters=iters, sp=sp, dp=dp)
    for b, (n, m) in enumerate(zip(ns, ms)):
        one = run(srcs[b], dsts[b], nrm[:, dp[b]:dp[b + 1]], None, None, iters=iters)
        s = slice(sp[b], sp[b + 1])
        assert same((got[0][b], got[1][b], got[2][b], got[3][s], got[5][s]), (one[0][0], one[1][0], one[2][0], one[3], one[5])), b
        assert torch.equal(got[4][s], torch.where(one[4] >= 0, one[4] + dp[b], one[4])), b
    return got


def test_ragged_batches_and_empty_pairs_equal_their_pairs():
    got = batch_equals_pairs((37, 1000, 0, 3, 2100, 256, 5), (50, 800, 10, 10, 1500, 300, 0))
    status = got[2][:, 0].cpu().tolist()
    assert status[2] == 0 and status[6] == 0 and status[1] == 1 and status[4] == 1


def test_a_batch_of_64_pairs_equals_its_pairs():
    batch_equals_pairs(counts64(), counts64(), iters=2)


def test_op_refusals():
    from hplflownet_amd import _lib, ops
    a, b = torch.zeros(3, 10, device=DEV), torch.zeros(3, 12, device=DEV)
    nb = torch.zeros(3, 12, device=DEV)
    for kw in (dict(metric='plane'), dict(dst_normal=nb), dict(metric='line', dst_normal=nb), dict(metric='point', dst_normal=nb),
               dict(metric='plane', dst_normal=nb[:, :11]), dict(metric='plane', dst_normal=nb.cpu()),
               dict(metric='plane', dst_normal=nb.double()), dict(metric='plane', dst_normal=nb.t()),
               dict(metric='plane', dst_normal=nb.clone().requires_grad_()), dict(metric='plane', dst_normal=nb, iters=65)):
        with pytest.raises(_lib.HplError):
            ops.icp(a, b, **kw)
    got = ops.icp(a, b, metric='plane', dst_normal=nb, iters=2)
    assert got[2].shape == (1, 6) and float(got[2][0, 0]) == 0           # zero normals: the first round fails


def test_icp_register_plane_equals_the_two_ops_by_hand():
    import hplflownet_amd as H
    from hplflownet_amd import _lib, ops
    n, B = 700, 3
    pairs = [O.pair(n, 60 + i) for i in range(B)]
    p1, p2 = torch.stack([dev(x[0]) for x in pairs]), torch.stack([dev(x[1]) for x in pairs])
    k1, k2 = p1.transpose(0, 1).reshape(3, B * n), p2.transpose(0, 1).reshape(3, B * n)
    pre = prefix_of([n] * B)
    nrm = ops.normals(k2, k=16, radius=1.0, prefix=pre)[0]
    want = ops.icp(k1, k2, iters=5, src_prefix=pre, dst_prefix=pre, metric='plane', dst_normal=nrm)
    got = H.icp_register(p1, p2, iters=5, metric='plane')
    assert same(want[:3], got[:3]) and all(torch.equal(got[3][b].t(), want[3][pre[b]:pre[b + 1]]) for b in range(B))
    nrm2 = ops.normals(k2, k=8, radius=1.5, prefix=pre)[0]
    want2 = ops.icp(k1, k2, iters=5, max_dist=0.8, src_prefix=pre, dst_prefix=pre, metric='plane', dst_normal=nrm2)
    assert same(want2[:3], H.icp_register(p1, p2, iters=5, max_dist=0.8, metric='plane', normals_k=8, normals_radius=1.5)[:3])
    assert same(want2[:3], H.icp_register(p1, p2, iters=5, max_dist=0.8, metric='plane', normals=nrm2)[:3])
    assert not same(want[:2], ops.icp(k1, k2, iters=5, src_prefix=pre, dst_prefix=pre)[:2])
    for bad in (dict(metric='line'), dict(normals=nrm), dict(metric='point', normals=nrm)):
        with pytest.raises(_lib.HplError):
            H.icp_register(p1, p2, **bad)


# ----------------------------------------------------------------------------- 6. engine --baseline icp --icp-metric plane
ARGS = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate']
ICP = ['icp_matched', 'icp_rmse', 'icp_angle_deg', 'icp_trans', 'icp_rounds']


def surface_tree(root, counts, kitti=False):
    """Frames of the surface scene whose pc2 is the scene's rigid motion of pc1, fewer points than --points so that the reader
    keeps every correspondence (the layouts of tests/test_gpu_icp.py's rigid_tree)."""
    import os
    for i, n in enumerate(counts):
        d = os.path.join(root, 'KITTI_processed_occ_final', '%06d' % i) if kitti else \
            os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        pc = NO.scene(n, 300 + i).astype(np.float64).T
        flip = np.array([1, 1, 1] if kitti else [-1, 1, -1], np.float64)
        np.save(os.path.join(d, 'pc1.npy'), (pc * flip).astype(np.float32))
        np.save(os.path.join(d, 'pc2.npy'), ((pc @ P.TRUE_R.T + P.TRUE_T) * flip).astype(np.float32))


def close(a, b, keys):
    for k in keys:
        assert abs(a[k] - b[k]) <= 2e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])


def test_engine_icp_metric_plane_single_batched_and_by_hand(tmp_path):
    from hplflownet_amd import data as data_mod
    from hplflownet_amd import engine, ops
    root = str(tmp_path)
    surface_tree(root, [400] * 13)                                      # 4 samples of equal counts
    args = ARGS + ['--dataset', 'FlyingThings3DSubset', '--data-root', root, '--baseline', 'icp']
    point = engine.main(args)
    flags = ['--icp-metric', 'plane', '--icp-normals-k', '8', '--icp-normals-radius', '2.0']
    one = engine.main(args + flags)
    four = engine.main(args + flags + ['--batch-size', '4'])
    assert list(one) == list(point) and list(four) == list(point)       # the report keys are unchanged
    assert all(one[k] == point[k] for k in point if not k.startswith('icp_'))
    assert engine.main(args + ['--icp-metric', 'point']) == point
    assert one['icp_trans'] != point['icp_trans'] and all(np.isfinite(v) for v in one.values())
    close(one, four, list(one))
    dev_ = torch.device('cuda', torch.cuda.current_device())
    reader = data_mod.FlyingThings3DSubset(False, data_mod.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root, device=dev_)
    cams = bool(getattr(reader, 'has_cameras', False))
    sums = torch.zeros((len(reader), 8), dtype=torch.float64, device=DEV)
    stats = []
    for i in range(len(reader)):
        s_ = reader[i]
        nrm = ops.normals(s_[1], k=8, radius=2.0)[0]
        _, _, st, flow = ops.icp(s_[0], s_[1], iters=30, max_dist=1.0, tau=0.3, metric='plane', dst_normal=nrm)
        stats.append(st[0].cpu().numpy())
        ops.flow_metrics_pairs([flow.t()], [s_[2]], [s_[0]], [getattr(s_, 'camera', None)], sums, i)
    folds = [ops.flow_metrics_fold(w, cams) for w in sums.cpu().numpy()]
    for k in folds[0]:
        assert one['icp_' + k] == sum(x[k] for x in folds) / len(folds), k
    for j, k in enumerate(ICP):
        assert one[k] == sum(float(s[1 + j]) for s in stats) / len(stats), k
    print('plane: icp_EPE3D %.4g in %.1f rounds; point: %.4g in %.1f rounds' % (one['icp_EPE3D'], one['icp_rounds'],
                                                                                point['icp_EPE3D'], point['icp_rounds']))
    assert one['icp_EPE3D'] * 10 <= one['icp_trans']                    # (zero flow is off by about |t| and the turn)


def test_engine_icp_metric_plane_ragged_kitti(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    surface_tree(root, [300, 450, 380, 500], kitti=True)
    args = ARGS + ['--dataset', 'KITTI', '--data-root', root, '--baseline', 'icp', '--icp-metric', 'plane', '--icp-normals-radius', '2']
    one = engine.main(args)
    ragged = engine.main(args + ['--batch-size', '4', '--ragged'])
    assert list(one) == list(ragged) and 'icp_EPE3D' in one and 'icp_rounds' in one
    assert all(one[k] == ragged[k] for k in ICP)                        # the registration's bits do not depend on the batch
    close(one, ragged, list(one))
