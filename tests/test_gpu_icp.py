"""GPU: hpl_icp / ops.icp, flownet.icp_register and engine --evaluate --baseline icp.

The matches are compared exactly: tests/icp_oracle.py restates the all-pairs match in the interface's float32 arithmetic, by
brute force.  The round's solve is the kernel's Horn quaternion against the restatement's float64 SVD; R, t and lengths are held
within the larger of (a) what the restatement's own float32 mode loses against its float64 mode on that input and (b) a float32
output floor: 8 * 2^-24 for entries of R, 8 * 2^-24 * scale for t and lengths, scale the largest coordinate.  Every bar comes
from the restatement, never from the device."""
import os

import numpy as np
import pytest
import torch

import icp_oracle as O
from batch64 import counts64, prefix_of
from rigid_oracle import rotation

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 8 * 2.0 ** -24
MD, TAU = 1.0, 0.3
#: a motion near the scene's (0.01 rad about (0.1, 1, 0.05), t = (0.03, -0.01, -0.25)) and not equal to it
NEAR = (rotation((0.0, 1.0, 0.1), 0.008).astype(np.float32), np.array([0.0, 0.02, -0.2], np.float32))
TRUE = (O.TRUE_R.astype(np.float32), O.TRUE_T.astype(np.float32))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def init_of(motion, B=1):
    """A float32 motion (R (3, 3), t (3,)), or a list of B of them -> the (R (B, 3, 3), t (B, 3)) device pair of ops.icp."""
    if motion is None:
        return None
    ms = motion if isinstance(motion, list) else [motion] * B
    return dev(np.stack([m[0] for m in ms])), dev(np.stack([m[1] for m in ms]))


def run(src, dst, w=None, init=None, iters=0, sp=None, dp=None, **kw):
    from hplflownet_amd import ops
    B = 1 if sp is None else len(sp) - 1
    out = ops.icp(dev(src), dev(dst), None if w is None else dev(w), init_of(init, B), iters=iters, max_dist=kw.pop('max_dist', MD),
                  tau=kw.pop('tau', TAU), src_prefix=sp, dst_prefix=dp, return_matches=True, **kw)
    torch.cuda.synchronize()
    return out                                   # R, t, stats, flow, match, dist2


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def motion_of(got, b=0):
    return got[0][b].cpu().numpy(), got[1][b].cpu().numpy()


def proper(R):
    R = np.asarray(R, np.float64)
    return np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0


_SCENES = {}


def scene(n, seed=None, m=None):
    key = (n, seed, m)
    if key not in _SCENES:
        _SCENES[key] = O.scene(n, n if seed is None else seed, m)
    return _SCENES[key]


# ----------------------------------------------------------------------------- 1. match only
def doctored(n, m, seed):
    """The scene with what a grid can get wrong: duplicated dst points, a dst point exactly max_dist from a query, queries on
    cell borders with dst points on either side, non-finite points in both clouds and points at 1e7 m."""
    src, dst = (x.copy() for x in scene(n, seed, m))
    if n < 200 or m < 200:
        return src, dst
    rng = np.random.RandomState(seed + 1)
    dup = rng.permutation(m)[:40]
    dst[:, dup[:20]] = dst[:, dup[20:]]                       # duplicates: the tie goes to the smaller index
    edge = np.float32(1.001 * MD)
    for j in range(16):                                       # queries on cell borders, dst points just inside both cells
        c = np.array([(j - 8) * edge, ((j % 3) - 1) * edge, (3 + j) * edge], np.float32)
        src[:, 100 + j] = c
        dst[:, 100 + 2 * j] = c + np.array([0.25, 0.0, -0.125], np.float32)
        dst[:, 101 + 2 * j] = c - np.array([0.25, 0.0, -0.125], np.float32)      # the same d2: a tie across two cells
    src[:, 0] = (40.0, 0.0, 5.0)                              # (alone out there under either motion)
    dst[:, 0] = (41.0, 0.0, 5.0)                              # exactly max_dist away under identity
    dst[:, 1] = (39.0, 0.0, 5.0)                              # and so is this one: the tie goes to index 0
    src[0, 1], src[2, 2], src[1, 3] = np.nan, np.inf, -np.inf
    dst[0, 2], dst[2, 3], dst[1, 4] = np.nan, np.inf, -np.inf
    src[:, 4] = (1e7, 0.0, 5.0)
    src[:, 5] = (0.0, -1e7, 5.0)
    dst[:, 5] = (1e7, 0.0, 5.0)                               # beside src 4, and outside the cell range: no part
    dst[:, 6] = (0.0, 0.0, -1e7)
    return src, dst


@pytest.mark.parametrize('n,m', [(1, 1), (3, 5), (255, 257), (1025, 300), (3000, 3000)])
@pytest.mark.parametrize('motion', ['identity', 'moved'])
def test_match_only_equals_the_restatement(n, m, motion):
    src, dst = doctored(n, m, 11 * n + m)
    R, t = O.IDENTITY if motion == 'identity' else TRUE
    got = run(src, dst, None, None if motion == 'identity' else (R, t), iters=0)
    want = O.finish(src, dst, R, t, None, MD)
    match, dist2, flow = got[4].cpu().numpy(), got[5].cpu().numpy(), got[3].cpu().numpy()
    assert np.array_equal(match, want['match'])
    assert np.array_equal(dist2.view(np.int32), want['dist2'].view(np.int32))
    assert np.array_equal(got[0][0].cpu().numpy(), R) and np.array_equal(got[1][0].cpu().numpy(), t)      # iters = 0: the init
    ok = np.isfinite(src).all(0)
    scale = np.abs(src[:, ok]).max(0) + 1.0
    assert (np.abs(flow[ok] - want['flow'][ok]).max(1) <= EPS * scale).all()
    stats = got[2][0].cpu().numpy()
    assert stats[0] == (1 if n >= 3 else 0) and stats[5] == 0 and abs(stats[1] - want['share']) <= 2.0 ** -23
    if n >= 200 and m >= 200:
        assert (match[1:6] == -1).all() and np.isinf(dist2[1:6]).all() and (match >= 0).sum() > min(n, m) // 2
        assert not np.isin(match, [2, 3, 4, 5, 6]).any()
        if motion == 'identity':
            assert match[0] == 0 and dist2[0] == np.float32(1.0)         # exactly at max_dist, the smaller index of the tie
            assert (match[100:116] >= 0).all()                           # the queries on cell borders


def test_a_point_just_past_max_dist_is_no_match():
    src = np.array([[40.0], [0.0], [5.0]], np.float32)
    dst = np.array([[41.0, np.nextafter(np.float32(39.0), np.float32(0))], [0.0, 0.0], [5.0, 5.0]], np.float32)
    got = run(src, dst)
    assert got[4].tolist() == [0] and got[5].tolist() == [1.0]
    got = run(src, dst[:, 1:])
    assert got[4].tolist() == [-1] and got[5].tolist() == [float('inf')] and got[2][0].tolist() == [0, 0, 0, 0, 0, 0]


def test_the_last_cells_of_the_key_and_the_ones_past_them():
    """tests/grid_edge.py: queries and dst points in the cells +-(2^18 - 2) of each axis match among themselves; those one cell
    further out, within max_dist of them, take no part on either side (tests/test_grid_edge.py checks the cloud on the CPU)."""
    import grid_edge as E
    dst, inside, cluster = E.cloud()
    src = dst + np.float32(0.0625)
    E.check_cells(dst, inside, cluster)
    E.check_cells(src, inside, cluster)
    want = O.finish(src, dst, *O.IDENTITY, None, MD)
    got = run(src, dst, iters=0)
    match, dist2 = got[4].cpu().numpy(), got[5].cpu().numpy()
    assert np.array_equal(match, want['match']) and np.array_equal(dist2.view(np.int32), want['dist2'].view(np.int32))
    assert (match[~inside] == -1).all() and np.isposinf(dist2[~inside]).all()
    assert (match[inside] >= 0).all() and (cluster[match[inside]] == cluster[inside]).all()    # no other edge, nothing from outside


# ----------------------------------------------------------------------------- 2. one round
def bars(src, dst, w, R0, t0, matched=None, what=''):
    """The restatement's round from the float32 motion (R0, t0) in both modes -> (o64, bar_R, bar_t, scale)."""
    matched = O.match(src, dst, R0, t0, MD) if matched is None else matched
    o64 = O.round_(src, dst, R0, t0, w, MD, TAU, np.float64, matched)
    o32 = O.round_(src, dst, R0, t0, w, MD, TAU, np.float32, matched)
    scale = float(max(np.abs(src[np.isfinite(src)]).max(), np.abs(dst[np.isfinite(dst)]).max()))
    dR, dt = float(np.abs(o32['R'] - o64['R']).max()), float(np.abs(o32['t'] - o64['t']).max())
    return o64, max(dR, EPS), max(dt, EPS * scale), scale, (dR, dt)


def check_round(got, src, dst, w, R0, t0, what, matched=None):
    """One device round from (R0, t0) against the restatement; the finish against the restatement under the device's own Rt."""
    o64, bar_R, bar_t, scale, (dR, dt) = bars(src, dst, w, R0, t0, matched)
    R, t = motion_of(got)
    stats = got[2][0].cpu().numpy()
    eR, et = float(np.abs(R - o64['R']).max()), float(np.abs(t - o64['t']).max())
    print('%s: |R - oracle| %.3g (bar %.3g, float32 mode %.3g)  |t - oracle| %.3g (bar %.3g, float32 mode %.3g)' % (
        what, eR, bar_R, dR, et, bar_t, dt))
    assert o64['ok'] and stats[0] == 1 and stats[5] == 1
    assert eR <= bar_R and et <= bar_t, what
    assert proper(R)
    fm = O.match(src, dst, R, t, MD)
    f64 = O.finish(src, dst, R, t, w, MD, np.float64, fm)
    f32 = O.finish(src, dst, R, t, w, MD, np.float32, fm)
    bar_rmse = max(abs(f32['rmse'] - f64['rmse']), EPS * scale)
    print('%s: |rmse - oracle| %.3g (bar %.3g)  |angle - oracle| %.3g  ||t| - oracle| %.3g  share %.6f / %.6f' % (
        what, abs(stats[2] - f64['rmse']), bar_rmse, abs(stats[3] - f64['angle_deg']), abs(stats[4] - f64['trans']), stats[1],
        f64['share']))
    assert np.array_equal(got[4].cpu().numpy(), f64['match'])
    assert np.array_equal(got[5].cpu().numpy().view(np.int32), f64['dist2'].view(np.int32))
    assert abs(stats[1] - f64['share']) <= 2.0 ** -23
    assert abs(stats[2] - f64['rmse']) <= bar_rmse
    assert abs(stats[3] - f64['angle_deg']) <= max(np.degrees(2 * EPS), 1e-5) and abs(stats[4] - f64['trans']) <= 2 * EPS * scale
    return fm


@pytest.mark.parametrize('n', [300, 1025, 3000])
@pytest.mark.parametrize('weighted', [False, True])
def test_one_round_against_the_restatement(n, weighted):
    src, dst = scene(n)
    w = O.weights(n, n) if weighted else None
    got = run(src, dst, w, NEAR, iters=1)
    check_round(got, src, dst, w, NEAR[0], NEAR[1], 'N = %d weighted %s' % (n, weighted))


# ----------------------------------------------------------------------------- 3. chain
@pytest.mark.parametrize('weighted', [False, True])
def test_three_rounds_equal_three_chained_calls(weighted):
    src, dst = scene(1025)
    w = O.weights(1025, 5) if weighted else None
    whole = run(src, dst, w, None, iters=3)
    step, motion = None, None
    for _ in range(3):
        step = run(src, dst, w, motion, iters=1)
        motion = motion_of(step)
    assert whole[2][0, 5] == 3 and step[2][0, 5] == 1
    assert same(whole[:2] + (whole[2][:, :5],) + whole[3:], step[:2] + (step[2][:, :5],) + step[3:])
    assert not np.array_equal(motion[0], np.eye(3, dtype=np.float32))


# ----------------------------------------------------------------------------- 4. lockstep
def test_eight_rounds_in_lockstep_with_the_restatement():
    n = 1025
    src, dst = scene(n)
    motion = O.IDENTITY
    matched = O.match(src, dst, *motion, MD)
    start = run(src, dst, iters=0)
    assert np.array_equal(start[4].cpu().numpy(), matched[0])
    for k in range(8):
        got = run(src, dst, None, motion, iters=1)
        # (the finish's match under the new motion, checked against the restatement there, is the next round's)
        matched = check_round(got, src, dst, None, motion[0], motion[1], 'round %d' % k, matched)
        motion = motion_of(got)
    assert np.abs(motion[0] - O.TRUE_R).max() <= 1e-3 and np.abs(motion[1] - O.TRUE_T).max() <= 1e-2


# ----------------------------------------------------------------------------- 5. convergence
@pytest.mark.parametrize('n', [300, 1025, 3000])
def test_convergence_on_the_scene(n):
    src, dst = scene(n)
    ref = O.chain(src, dst, iters=30)
    refR, reft = float(np.abs(ref['R32'] - O.TRUE_R).max()), float(np.abs(ref['t32'] - O.TRUE_T).max())
    idR, idt = float(np.abs(np.eye(3) - O.TRUE_R).max()), float(np.abs(O.TRUE_T).max())
    assert ref['status'] == 1 and ref['rounds'] < 30 and refR <= 0.1 * idR and reft <= 0.1 * idt
    _, bar_R, bar_t, _, _ = bars(src, dst, None, ref['R32'], ref['t32'])         # the bars of a round at the restatement's end
    got = run(src, dst, iters=30)
    rounds = int(got[2][0, 5])
    R, t = motion_of(got)
    eR, et = float(np.abs(R - O.TRUE_R).max()), float(np.abs(t - O.TRUE_T).max())
    print('N = %d: %d rounds (restatement %d); R off truth by %.3g (restatement %.3g, bar %.3g), t by %.3g (restatement %.3g, bar '
          '%.3g)' % (n, rounds, ref['rounds'], eR, refR, bar_R, et, reft, bar_t))
    assert got[2][0, 0] == 1 and 0 < rounds < 30
    assert same(got, run(src, dst, iters=rounds))
    assert eR <= 2 * refR + bar_R and et <= 2 * reft + bar_t
    # a fixpoint: one more round from it hands the same bits on
    assert same(run(src, dst, None, (R, t), iters=1)[:2], got[:2])
    # with tolerances it stops no later, at the motion of the last round it ran
    tol = run(src, dst, iters=30, tol_rot=1e-4, tol_trans=1e-4)
    early = int(tol[2][0, 5])
    assert 0 < early <= rounds
    motion = None
    for _ in range(early):
        motion = motion_of(run(src, dst, None, motion, iters=1))
    assert np.array_equal(motion[0], tol[0][0].cpu().numpy()) and np.array_equal(motion[1], tol[1][0].cpu().numpy())
    if early > 1:
        assert same(run(src, dst, iters=early)[:2], tol[:2])


# ----------------------------------------------------------------------------- 6. ragged
NS = (37, 1000, 3, 2100, 256)
MS = (50, 800, 10, 1500, 300)


def ragged_inputs(ns=NS, ms=MS, seed=70):
    parts = [scene(n, seed + i, m) for i, (n, m) in enumerate(zip(ns, ms))]
    src = np.concatenate([x[0] for x in parts], 1)
    dst = np.concatenate([x[1] for x in parts], 1)
    w = np.concatenate([O.weights(n, seed + i) for i, n in enumerate(ns)])
    return parts, src, dst, w, prefix_of(list(ns)), prefix_of(list(ms))


def pair_of(got, b, sp, dp):
    """Pair b's outputs of a batched call in the form of a call of the pair alone (its matches from 0)."""
    sl = slice(sp[b], sp[b + 1])
    match = got[4][sl]
    return (got[0][b:b + 1], got[1][b:b + 1], got[2][b:b + 1], got[3][sl], torch.where(match >= 0, match - dp[b], match), got[5][sl])


@pytest.mark.parametrize('weighted', [False, True])
def test_ragged_batches_equal_their_pairs(weighted):
    parts, src, dst, w, sp, dp = ragged_inputs()
    w = w if weighted else None
    inits = [NEAR, TRUE, O.IDENTITY, NEAR, TRUE]
    got = run(src, dst, w, inits, iters=4, sp=sp, dp=dp)
    for b in range(len(NS)):
        ws = None if w is None else w[sp[b]:sp[b + 1]]
        one = run(parts[b][0], parts[b][1], ws, inits[b], iters=4)
        assert same(one, pair_of(got, b, sp, dp)), b
        assert same(one, run(parts[b][0], parts[b][1], ws, inits[b], iters=4, sp=[0, NS[b]], dp=[0, MS[b]])), b
        assert float(got[2][b, 0]) == 1 and float(got[2][b, 5]) >= 1, b
    assert int((got[4] >= 0).sum()) > sum(NS) // 2


def test_empty_pairs_inside_a_batch():
    parts, src, dst, w, sp, dp = ragged_inputs()
    # pair 1 without src, pair 3 without dst: (37, 50), (0, 800), (3, 10), (2100, 0), (256, 300)
    s2 = np.concatenate([parts[b][0] for b in (0, 2, 3, 4)], 1)
    d2 = np.concatenate([parts[b][1] for b in (0, 1, 2, 4)], 1)
    sp2, dp2 = prefix_of([37, 0, 3, 2100, 256]), prefix_of([50, 800, 10, 0, 300])
    inits = [NEAR, TRUE, NEAR, TRUE, NEAR]
    got = run(s2, d2, None, inits, iters=4, sp=sp2, dp=dp2)
    for b in (0, 2, 4):
        assert same(run(parts[b][0], parts[b][1], None, inits[b], iters=4), pair_of(got, b, sp2, dp2)), b
    for b in (1, 3):
        assert np.array_equal(motion_of(got, b)[0], inits[b][0]) and np.array_equal(motion_of(got, b)[1], inits[b][1])
        st = got[2][b].tolist()
        assert st[:3] == [0, 0, 0] and st[5] == 0
        assert abs(st[3] - O.angle_deg(inits[b][0])) <= 1e-5 and abs(st[4] - float(np.linalg.norm(inits[b][1].astype(np.float64)))) <= 1e-6
    sl = slice(sp2[3], sp2[4])
    assert bool((got[4][sl] == -1).all()) and bool(torch.isinf(got[5][sl]).all())
    want = O.finish(parts[3][0], parts[3][1][:, :0], *TRUE)['flow']
    assert np.abs(got[3][sl].cpu().numpy() - want).max() <= EPS * 40


def test_a_batch_of_64_pairs_equals_its_pairs():
    """B = 64 (tests/batch64.py), N_b != M_b: the dst counts are the src counts one pair on."""
    ns = counts64()
    ms = ns[1:] + ns[:1]
    ms[40], ms[50] = 1800, 1100
    parts, src, dst, w, sp, dp = ragged_inputs(ns, ms, 200)
    got = run(src, dst, None, None, iters=3, sp=sp, dp=dp)
    for b, (n, m) in enumerate(zip(ns, ms)):
        if n > 0:
            assert same(run(parts[b][0], parts[b][1], None, None, iters=3, sp=[0, n], dp=[0, m]), pair_of(got, b, sp, dp)), b
        if n < 3 or m == 0:
            assert torch.equal(got[0][b].cpu(), torch.eye(3)) and not bool(got[1][b].any())
            assert float(got[2][b, 0]) == 0 and float(got[2][b, 5]) == 0, (b, got[2][b].tolist())
    assert float(got[2][40, 0]) == 1 and float(got[2][50, 0]) == 1 and float(got[2][40, 5]) == 3


# ----------------------------------------------------------------------------- 7. strided views
def test_strided_views_are_read_in_place_and_nothing_else_is_written():
    from hplflownet_amd import ops
    n, m, wide = 1000, 900, 1500
    src, dst = scene(n, 5, m)
    want = ops.icp(dev(src), dev(dst), iters=3, return_matches=True)
    ws = torch.full((3, 3, wide), float('nan'), device=DEV)
    wd = torch.full((3, 3, wide), float('nan'), device=DEV)
    ws[1, :, 7:7 + n] = dev(src)
    wd[1, :, 11:11 + m] = dev(dst)
    a, b = ws[1][:, 7:7 + n], wd[1][:, 11:11 + m]
    assert not a.is_contiguous() and a.stride(0) == wide and not b.is_contiguous()
    guard = torch.full((n + 2, 3), float('nan'), device=DEV)
    got = ops.icp(a, b, iters=3, return_matches=True, out=guard[1:n + 1])
    torch.cuda.synchronize()
    assert got[3].data_ptr() == guard[1].data_ptr() and same(want, got)
    assert bool(torch.isnan(guard[0]).all()) and bool(torch.isnan(guard[n + 1]).all())
    assert bool(torch.isnan(ws[1][:, :7]).all()) and bool(torch.isnan(ws[1][:, 7 + n:]).all()) and bool(torch.isnan(ws[0]).all())
    assert bool(torch.isnan(wd[1][:, :11]).all()) and bool(torch.isnan(wd[1][:, 11 + m:]).all()) and bool(torch.isnan(wd[2]).all())
    assert torch.equal(ws[1][:, 7:7 + n], dev(src)) and torch.equal(wd[1][:, 11:11 + m], dev(dst))


# ----------------------------------------------------------------------------- 8. degenerate inputs
def failed(got, init, rounds, b=0):
    R, t = motion_of(got, b)
    assert np.array_equal(R, init[0]) and np.array_equal(t, init[1])
    st = got[2][b].tolist()
    assert st[0] == 0 and st[5] == rounds and all(np.isfinite(st))


def test_degenerate_inputs():
    src, dst = scene(1024, 9)
    # all dst in one cell: every query within reach compares with all 1 024 of them
    rng = np.random.RandomState(3)
    d1 = (np.array([[3.2], [0.2], [10.2]]) + rng.uniform(0, 0.6, (3, 1024))).astype(np.float32)
    s1 = (np.array([[3.5], [0.5], [10.5]]) + rng.uniform(-1.5, 1.5, (3, 1024))).astype(np.float32)
    assert len(np.unique(np.floor(d1.astype(np.float64) / (1.001 * MD)), axis=1).T) == 1
    got = run(s1, d1, iters=2)
    assert got[2][0, 0] == 1 and proper(motion_of(got)[0]) and bool(torch.isfinite(got[2]).all())
    fin = O.finish(s1, d1, *motion_of(got))
    assert np.array_equal(got[4].cpu().numpy(), fin['match']) and np.array_equal(got[5].cpu().numpy().view(np.int32), fin['dist2'].view(np.int32))
    assert 0 < (fin['match'] >= 0).sum() < 1024
    # all src points identical: no rotation can be told, the quaternion of a zero matrix is the identity's; t moves the point
    k = int(np.nonzero(O.match(src, dst, NEAR[0], NEAR[1], MD)[0] >= 0)[0][0])          # (a point with a match under NEAR)
    s2 = np.repeat(src[:, k:k + 1], 1024, 1)
    got = run(s2, dst, None, NEAR, iters=3)
    R, t = motion_of(got)
    assert got[2][0, 0] == 1 and np.array_equal(R, np.eye(3, dtype=np.float32)) and np.isfinite(t).all()
    assert bool(torch.isfinite(got[2]).all()) and bool(torch.isfinite(got[3]).all())
    # fewer than three src points, no dst, no dst within max_dist, all weights off: status 0, the motion stays the init
    for k in (1, 2):
        failed(run(src[:, :k], dst, None, NEAR, iters=4), NEAR, 0)
    failed(run(src, dst[:, :0], None, NEAR, iters=4), NEAR, 0)
    far = run(src, dst + np.float32(100), None, NEAR, iters=4)
    failed(far, NEAR, 1)
    assert bool((far[4] == -1).all()) and bool(torch.isinf(far[5]).all()) and far[2][0].tolist()[1:3] == [0, 0]
    for w in (np.zeros(1024, np.float32), np.full(1024, np.nan, np.float32), np.full(1024, -1.0, np.float32),
              np.full(1024, np.inf, np.float32)):
        off = run(src, dst, w, NEAR, iters=4)
        failed(off, NEAR, 1)
        assert off[2][0].tolist()[1:3] == [0, 0] and int((off[4] >= 0).sum()) > 512      # matched, but nothing with a weight
    failed(run(src, dst, None, None, iters=4, max_dist=1e-4), O.IDENTITY, 1)
    # N = 0: no launch; the outputs are pre-filled
    from hplflownet_amd import ops
    e = ops.icp(dev(src[:, :0]), dev(dst), src_prefix=[0, 0, 0], dst_prefix=[0, 1000, 1024], return_matches=True)
    assert e[2].tolist() == [[0] * 6] * 2 and torch.equal(e[0].cpu(), torch.eye(3).expand(2, 3, 3)) and e[3].shape == (0, 3)


def test_non_finite_src_points_take_no_part():
    n = 1000
    src, dst = scene(n, 12)
    bad = np.array([0, 17, 500, 998, 999])
    sb = src.copy()
    sb[0, bad[:2]] = np.nan
    sb[2, bad[2]] = np.inf
    sb[1, bad[3:]] = -np.inf
    keep = np.ones(n, bool)
    keep[bad] = False
    got = run(sb, dst, None, NEAR, iters=1)
    w = keep.astype(np.float32)
    o64, bar_R, bar_t, _, _ = bars(src, dst, w, NEAR[0], NEAR[1])
    R, t = motion_of(got)
    assert np.abs(R - o64['R']).max() <= bar_R and np.abs(t - o64['t']).max() <= bar_t
    assert bool((got[4][dev(bad, np.int64)] == -1).all()) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())
    assert same(got[:3], run(sb, dst, np.ones(n, np.float32), NEAR, iters=1)[:3])          # unit weights: the NULL path's bits


# ----------------------------------------------------------------------------- 9. repeatability
def test_same_bits_twice_and_beside_a_busy_stream():
    from hplflownet_amd import ops
    parts, src, dst, w, sp, dp = ragged_inputs()
    first = run(src, dst, w, None, iters=6, sp=sp, dp=dp)
    assert same(first, run(src, dst, w, None, iters=6, sp=sp, dp=dp))
    ts, td, tw = dev(src), dev(dst), dev(w)
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            a = torch.tanh(a @ a * 1e-3)
    busy = ops.icp(ts, td, tw, iters=6, max_dist=MD, tau=TAU, src_prefix=sp, dst_prefix=dp, return_matches=True)
    torch.cuda.synchronize()
    assert same(first, busy)


# ----------------------------------------------------------------------------- 11. icp_register
def test_icp_register_takes_the_three_forms():
    import hplflownet_amd as H
    from hplflownet_amd import ops
    n, B = 700, 3
    pairs = [scene(n, 30 + i) for i in range(B)]
    p1 = torch.stack([dev(x[0]) for x in pairs])
    p2 = torch.stack([dev(x[1]) for x in pairs])
    packed1, packed2 = p1.transpose(0, 1).reshape(3, B * n), p2.transpose(0, 1).reshape(3, B * n)
    pre = prefix_of([n] * B)
    want = ops.icp(packed1, packed2, iters=5, src_prefix=pre, dst_prefix=pre, return_matches=True)
    got = H.icp_register(p1, p2, iters=5, return_matches=True)                       # (B, 3, N)
    assert got[3].shape == (B, 3, n) and same(want[:3] + want[4:], got[:3] + got[4:])
    assert all(torch.equal(got[3][b].t(), want[3][pre[b]:pre[b + 1]]) for b in range(B))
    one = H.icp_register(p1[0], p2[0], iters=5)                                      # (3, N): one pair
    assert one[3].shape == (3, n) and same((want[0][:1], want[1][:1], want[2][:1], want[3][:n]), (one[0], one[1], one[2], one[3].t()))
    assert same(one, H.icp_register(p1[:1], p2[:1], iters=5)[:3] + (H.icp_register(p1[:1], p2[:1], iters=5)[3][0],))
    # lists of ragged clouds, (3, N_b) and (1, 3, N_b) entries; N_b of pc1 and of pc2 differ
    ns, ms = (700, 300, 512), (650, 300, 700)
    l1 = [p1[b][:, :ns[b]] for b in range(B)]
    l2 = [p2[b][:, :ms[b]] for b in range(B)]
    sp, dp = prefix_of(list(ns)), prefix_of(list(ms))
    wantl = ops.icp(torch.cat(l1, 1), torch.cat(l2, 1), iters=5, src_prefix=sp, dst_prefix=dp)
    gotl = H.icp_register([l1[0], l1[1][None], l1[2]], l2, iters=5)
    assert same(wantl[:3], gotl[:3]) and [tuple(f.shape) for f in gotl[3]] == [(3, 700), (1, 3, 300), (3, 512)]
    assert all(torch.equal(f.reshape(3, -1).t(), wantl[3][sp[b]:sp[b + 1]]) for b, f in enumerate(gotl[3]))
    # a packed cloud with its counts, and an init from a rigid fit's form
    init = (wantl[0].clone(), wantl[1].clone())
    gotp = H.icp_register(torch.cat(l1, 1), torch.cat(l2, 1), (list(ns), list(ms)), init=init, iters=2)
    assert gotp[3].shape == (3, sum(ns))
    assert same(ops.icp(torch.cat(l1, 1), torch.cat(l2, 1), init=init, iters=2, src_prefix=sp, dst_prefix=dp)[:3], gotp[:3])
    from hplflownet_amd import _lib
    for bad in ((p1, p2[:2]), (l1, l2[:2]), (torch.cat(l1, 1), torch.cat(l2, 1), [700, 300]), (p1[0][0], p2[0])):
        with pytest.raises(_lib.HplError):
            H.icp_register(*bad)


# ----------------------------------------------------------------------------- 12. engine --evaluate --baseline icp
ARGS = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate']
ICP = ['icp_matched', 'icp_rmse', 'icp_angle_deg', 'icp_trans', 'icp_rounds']


def rigid_tree(root, counts, kitti=False):
    """Frames whose pc2 is ONE rigid motion of pc1 -- the scene's: 0.01 rad about (0.1, 1, 0.05), t = (0.03, -0.01, -0.25) --,
    fewer points than --points so that the reader keeps every correspondence: FlyingThings3D-style (the reader takes every
    fourth directory and stores x and z with the opposite sign) or KITTI-style (every directory, as stored)."""
    for i, n in enumerate(counts):
        d = os.path.join(root, 'KITTI_processed_occ_final', '%06d' % i) if kitti else \
            os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        rng = np.random.RandomState(300 + i)
        pc = np.stack([rng.uniform(-15, 15, n), rng.uniform(-2, 2, n), rng.uniform(3, 33, n)], 1)
        flip = np.array([1, 1, 1] if kitti else [-1, 1, -1], np.float64)
        np.save(os.path.join(d, 'pc1.npy'), (pc * flip).astype(np.float32))
        np.save(os.path.join(d, 'pc2.npy'), ((pc @ O.TRUE_R.T + O.TRUE_T) * flip).astype(np.float32))


def close(a, b, keys):
    for k in keys:
        assert abs(a[k] - b[k]) <= 2e-4 * max(1.0, abs(a[k])), (k, a[k], b[k])


def test_engine_baseline_icp_single_batched_and_by_hand(tmp_path):
    from hplflownet_amd import data as data_mod
    from hplflownet_amd import engine, ops
    root = str(tmp_path)
    rigid_tree(root, [400] * 13)                                        # 4 samples of equal counts
    args = ARGS + ['--dataset', 'FlyingThings3DSubset', '--data-root', root]
    plain = engine.main(args)
    one = engine.main(args + ['--baseline', 'icp'])
    four = engine.main(args + ['--baseline', 'icp', '--batch-size', '4'])
    assert list(one) == list(plain) + ['icp_' + k for k in plain] + ICP and list(four) == list(one)
    assert all(one[k] == plain[k] for k in plain)                       # the keys of before: exactly the run without the flag
    close(one, four, list(one))
    assert all(np.isfinite(v) for v in one.values()) and 0 < one['icp_matched'] <= 1 and 0 < one['icp_rounds'] < 30
    other = engine.main(args + ['--baseline', 'icp', '--icp-iters', '1', '--icp-max-dist', '0.7', '--icp-tau', '0.2'])
    assert all(other[k] == plain[k] for k in plain) and other['icp_rounds'] == 1 and other['icp_trans'] != one['icp_trans']
    # by hand: the engine's own reader, then ops.icp and the metrics op; identity does not look at the model
    dev_ = torch.device('cuda', torch.cuda.current_device())
    reader = data_mod.FlyingThings3DSubset(False, data_mod.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root, device=dev_)
    cams = bool(getattr(reader, 'has_cameras', False))
    sums = torch.zeros((len(reader), 8), dtype=torch.float64, device=DEV)
    zsums = torch.zeros((len(reader), 8), dtype=torch.float64, device=DEV)
    stats = []
    for i in range(len(reader)):
        s_ = reader[i]
        _, _, st, flow = ops.icp(s_[0], s_[1], iters=30, max_dist=1.0, tau=0.3)
        stats.append(st[0].cpu().numpy())
        ops.flow_metrics_pairs([flow.t()], [s_[2]], [s_[0]], [getattr(s_, 'camera', None)], sums, i)
        ops.flow_metrics_pairs([torch.zeros_like(flow).t()], [s_[2]], [s_[0]], [getattr(s_, 'camera', None)], zsums, i)
    folds = [ops.flow_metrics_fold(w, cams) for w in sums.cpu().numpy()]
    zero = [ops.flow_metrics_fold(w, cams) for w in zsums.cpu().numpy()]
    for k in plain:
        assert one['icp_' + k] == sum(x[k] for x in folds) / len(folds), k
    for j, k in enumerate(ICP):
        assert one[k] == sum(float(s[1 + j]) for s in stats) / len(stats), k
    zero_epe = sum(x['EPE3D'] for x in zero) / len(zero)
    print('icp_EPE3D %.4g against %.4g of zero flow' % (one['icp_EPE3D'], zero_epe))
    assert one['icp_EPE3D'] * 10 <= zero_epe
    # network + ICP: the init is the rigid fit's
    both = engine.main(args + ['--rigid-refine', '--baseline', 'icp', '--icp-init', 'rigid', '--icp-iters', '2'])
    assert list(both) == list(plain) + ['rigid_' + k for k in plain] + ['rigid_inliers', 'rigid_angle_deg', 'rigid_trans'] + \
        ['icp_' + k for k in plain] + ICP
    tr = engine.Trainer('HPLFlowNetShallow', dev_)
    tr.model.eval()
    isums = torch.zeros((len(reader), 8), dtype=torch.float64, device=DEV)
    istats = []
    with torch.no_grad():
        for i in range(len(reader)):
            s_ = reader[i]
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))
            R, t, _, _ = ops.rigid_fit(s_[0], flow[0], iters=4, tau=0.1)
            _, _, st, iflow = ops.icp(s_[0], s_[1], init=(R, t), iters=2, max_dist=1.0, tau=0.3)
            istats.append(st[0].cpu().numpy())
            ops.flow_metrics_pairs([iflow.t()], [s_[2]], [s_[0]], [getattr(s_, 'camera', None)], isums, i)
    folds = [ops.flow_metrics_fold(w, cams) for w in isums.cpu().numpy()]
    for k in plain:
        assert both['icp_' + k] == sum(x[k] for x in folds) / len(folds), k
    for j, k in enumerate(ICP):
        assert both[k] == sum(float(s[1 + j]) for s in istats) / len(istats), k


def test_engine_baseline_icp_ragged_kitti(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    rigid_tree(root, [300, 450, 380, 500], kitti=True)                  # short frames: every pair keeps its own count
    args = ARGS + ['--dataset', 'KITTI', '--data-root', root, '--baseline', 'icp']
    one = engine.main(args)
    ragged = engine.main(args + ['--batch-size', '4', '--ragged'])
    assert list(one) == list(ragged) and 'icp_EPE3D' in one and 'icp_rounds' in one
    assert all(one[k] == ragged[k] for k in ICP)                        # the registration's bits do not depend on the batch
    close(one, ragged, list(one))
    assert one['icp_EPE3D'] * 10 <= one['icp_trans']                    # (zero flow is off by about |t| and the turn)
