"""GPU: hpl_motion_segment / ops.motion_segment, flownet.segment_motion and validate(segment=...).

labels, obj_info and stats must EQUAL tests/segment_oracle.py (the all-pairs float32 predicate, no grid): no tolerance.
obj_motion: the inputs are float32 and the kernel's sums float64; n * 2^-53 at n <= 450 000 is far below a float32 half-ulp,
so every entry lies within 1 float32 ulp of the oracle's float64 mean rounded to float32 (derived, not measured)."""
import numpy as np
import pytest
import torch

import rigid_oracle
from batch64 import counts64, prefix_of
from segment_oracle import SCENE_KW, scene, segment, segment_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(p, f, r, prefix=None, **kw):
    from hplflownet_amd import ops
    out = ops.motion_segment(dev(p), dev(f), dev(r), prefix=prefix, **kw)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def ulps(got, want):
    """Distance in float32 steps between two finite float32 arrays."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(got) - key(want))


def check(got, p, f, r, prefix=None, what='', **kw):
    """Every output against the oracle; -> the oracle's stats."""
    prefix = [0, p.shape[1]] if prefix is None else prefix
    labels, info, motion, stats = [x.cpu().numpy() for x in got]
    want = segment_batch(p, f, r, prefix, **kw)
    print('%s: stats %s (oracle %s), largest obj_motion distance %d ulp' % (
        what, stats.tolist(), want[3].tolist(), int(ulps(motion, want[2]).max())))
    assert np.array_equal(stats, want[3]), what
    assert np.array_equal(labels, want[0]), what
    assert np.array_equal(info, want[1]), what
    assert np.isfinite(motion).all() and int(ulps(motion, want[2]).max()) <= 1, what
    assert labels.dtype == np.int32 and info.dtype == np.int32 and stats.dtype == np.int32
    return want[3]


_SCENE = {}


def the_scene(n):
    if n not in _SCENE:
        _SCENE[n] = scene(n)
    return _SCENE[n]


@pytest.mark.parametrize('n', [300, 1000, 4099])
@pytest.mark.parametrize('min_points', [1, 5])
def test_scene_equals_the_oracle(n, min_points):
    p, f, r, per = the_scene(n)
    st = check(run(p, f, r, min_points=min_points, **SCENE_KW), p, f, r, min_points=min_points, what='scene N = %d' % n, **SCENE_KW)
    assert st[0, 0] == 6 * per and st[0, 1] >= 6


def test_dense_load_every_point_a_mover():
    p, f, _, _ = the_scene(4099)
    r = np.ones(4099, np.float32)
    st = check(run(p, f, r, **SCENE_KW), p, f, r, what='all movers', **SCENE_KW)
    assert st[0, 0] == 4099 and st[0, 1] > 6 and st[0, 2] < 4099          # background components and noise


def test_shuffled_chains():
    """Two chains of 2 000 points at spacing 0.9 eps, 3 eps apart, their points interleaved in index and each in random order
    along its line: deep trees, many racing hooks, two components whose roots are the smallest indices."""
    eps, m = 0.5, 2000
    rng = np.random.RandomState(5)
    p = np.zeros((3, 2 * m), np.float32)
    p[0, 0::2] = (0.9 * eps) * rng.permutation(m)
    p[0, 1::2] = (0.9 * eps) * rng.permutation(m)
    p[1, 1::2] = 3 * eps
    f, r = np.zeros_like(p), np.ones(2 * m, np.float32)
    got = run(p, f, r, eps=eps)
    st = check(got, p, f, r, what='chains', eps=eps)
    assert st.tolist() == [[2 * m, 2, 2 * m, 0]]
    assert got[1][0, :3].tolist() == [[0, m], [1, m], [-1, 0]]
    assert torch.equal(got[0].cpu(), torch.arange(2 * m, dtype=torch.int32) % 2)


def test_cell_edges_and_the_closed_bound():
    """Points on exact multiples of eps on both sides of 0 in every axis (floor, not truncation; neighbours across cell
    faces), and pairs at distance exactly eps (linked: <=) and one float above it (not linked)."""
    eps = 0.5
    up = np.nextafter(np.float32(eps), np.float32(1))
    g = np.arange(-3, 4) * eps
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij')).reshape(3, -1)
    pairs = [lattice, [[0, eps], [0, 0], [0, 0]], [[0, up], [0, 0], [0, 0]], [[-eps, 0], [0, 0], [0, 0]], [[-up, 0], [0, 0], [0, 0]],
             [[0, 0], [0, -eps], [0, 0]], [[7, 7], [3, 3], [-up, 0]], [[-eps, -2 * eps], [0, 0], [0, 0]]]
    pairs = [np.asarray(x, np.float32) for x in pairs]
    p = np.concatenate(pairs, 1)
    prefix = np.concatenate([[0], np.cumsum([x.shape[1] for x in pairs])]).tolist()
    f, r = np.zeros_like(p), np.ones(p.shape[1], np.float32)
    st = check(run(p, f, r, prefix=prefix, eps=eps, min_points=1), p, f, r, prefix, eps=eps, min_points=1, what='cell edges')
    assert st[:, 1].tolist() == [1, 1, 2, 1, 2, 1, 2, 1] and st[0].tolist() == [343, 1, 343, 0]


def test_heavy_cell():
    rng = np.random.RandomState(6)
    p = np.concatenate([np.tile([[1.3], [-0.2], [9.0]], (1, 600)), np.array([[1.3], [-0.2], [9.0]]) + rng.uniform(-0.14, 0.14, (3, 40))], 1)
    p = p[:, rng.permutation(640)].astype(np.float32)
    f, r = np.zeros_like(p), np.ones(640, np.float32)
    st = check(run(p, f, r, eps=0.5), p, f, r, eps=0.5, what='heavy cell')
    assert st.tolist() == [[640, 1, 640, 0]]


def test_flow_criterion():
    rng = np.random.RandomState(7)
    p = rng.uniform(0, 1, (3, 300)).astype(np.float32) + np.array([[2.0], [0.0], [10.0]], np.float32)
    f = (0.01 * rng.normal(size=(3, 300))).astype(np.float32)
    f[0, 1::2] += 1.0                                                      # the odd points: a second cloud, 1 m/s apart
    r = np.ones(300, np.float32)
    two = run(p, f, r, eps=0.5, dv=0.3)
    st = check(two, p, f, r, eps=0.5, dv=0.3, what='dv = 0.3')
    assert st.tolist() == [[300, 2, 300, 0]] and torch.equal(two[0].cpu(), torch.arange(300, dtype=torch.int32) % 2)
    st = check(run(p, f, r, eps=0.5), p, f, r, eps=0.5, what='dv = inf')
    assert st.tolist() == [[300, 1, 300, 0]]


def test_more_objects_than_table_rows():
    p = np.zeros((3, 100), np.float32)
    p[0] = 2.0 * np.random.RandomState(8).permutation(100)
    f, r = np.zeros_like(p), np.ones(100, np.float32)
    got = run(p, f, r, eps=0.5, min_points=1, max_objects=16)
    st = check(got, p, f, r, eps=0.5, min_points=1, max_objects=16, what='overflow')
    assert st.tolist() == [[100, 100, 100, 0]] and got[1].shape == (1, 16, 2) and got[2].shape == (1, 16, 6)
    assert torch.equal(got[0].cpu(), torch.arange(100, dtype=torch.int32))
    assert got[1][0].cpu().tolist() == [[i, 1] for i in range(16)]


COUNTS = (37, 1000, 3, 4099, 256)


def test_ragged_batch_equals_its_pairs():
    """Every pair's scene fills the same space: nothing links across pairs, and each pair has its bits alone and in the batch."""
    parts = [scene(n, 1 + (i % 2)) if n >= 300 else [x[..., -n:] for x in scene(300, 1 + (i % 2))[:3]]      # (a short pair: the
             for i, n in enumerate(COUNTS)]                                                                  # tail of a scene)
    p, f = np.concatenate([x[0] for x in parts], 1), np.concatenate([x[1] for x in parts], 1)
    r = np.concatenate([x[2] for x in parts])
    prefix = np.concatenate([[0], np.cumsum(COUNTS)]).tolist()
    kw = dict(min_points=3, **SCENE_KW)
    labels, info, motion, stats = got = run(p, f, r, prefix=prefix, **kw)
    check(got, p, f, r, prefix, what='ragged', **kw)
    for b, n in enumerate(COUNTS):
        sl = slice(prefix[b], prefix[b + 1])
        one = run(p[:, sl], f[:, sl], r[sl], **kw)
        assert same(one, (labels[sl], info[b:b + 1], motion[b:b + 1], stats[b:b + 1])), b
        assert same(one, run(p[:, sl], f[:, sl], r[sl], prefix=[0, n], **kw)), b
    # another order, an empty pair between: every pair keeps its bits
    order = [3, 0, 4]
    q = np.concatenate([p[:, prefix[b]:prefix[b + 1]] for b in order], 1)
    g = np.concatenate([f[:, prefix[b]:prefix[b + 1]] for b in order], 1)
    rr = np.concatenate([r[prefix[b]:prefix[b + 1]] for b in order])
    pre = [0, COUNTS[3], COUNTS[3], COUNTS[3] + COUNTS[0], COUNTS[3] + COUNTS[0] + COUNTS[4]]
    l2, i2, m2, s2 = run(q, g, rr, prefix=pre, **kw)
    for j, b in zip((0, 2, 3), order):
        assert same((labels[prefix[b]:prefix[b + 1]], info[b], motion[b], stats[b]), (l2[pre[j]:pre[j + 1]], i2[j], m2[j], s2[j]))
    assert s2[1].tolist() == [0, 0, 0, 0] and i2[1, 0].tolist() == [-1, 0] and not bool(m2[1].any())


def test_a_batch_of_64_pairs_equals_its_pairs():
    """B = 64 (tests/batch64.py): the oracle's outputs, and every pair's are the bits of that pair run alone with
    prefix = [0, n]."""
    counts = counts64()
    prefix = prefix_of(counts)
    parts = [scene(n, 1 + (i % 2)) if n >= 300 else [x[..., 300 - n:] for x in scene(300, 1 + (i % 2))[:3]]     # (a short pair:
             for i, n in enumerate(counts)]                                                                   # the tail of a scene)
    p, f = np.concatenate([x[0] for x in parts], 1), np.concatenate([x[1] for x in parts], 1)
    r = np.concatenate([x[2] for x in parts])
    kw = dict(min_points=3, max_objects=64, **SCENE_KW)
    labels, info, motion, stats = got = run(p, f, r, prefix=prefix, **kw)
    check(got, p, f, r, prefix, what='B = 64', **kw)
    for b, n in enumerate(counts):
        sl = slice(prefix[b], prefix[b + 1])
        one = run(p[:, sl], f[:, sl], r[sl], prefix=[0, n], **kw)
        assert same(one, (labels[sl], info[b:b + 1], motion[b:b + 1], stats[b:b + 1])), b
    assert int(stats[40, 1]) > 0 and int(stats[50, 1]) > 0 and int(stats[34, 1]) > 0      # objects on both sides of the step


def test_degenerate_inputs():
    from hplflownet_amd import ops
    one = np.array([[1.0], [2.0], [3.0]], np.float32)
    for res, lab, stats in ((1.0, 0, [1, 1, 1, 0]), (0.05, -1, [0, 0, 0, 0]), (np.nan, -1, [0, 0, 0, 0])):
        got = run(one, np.zeros_like(one), np.array([res], np.float32), min_points=1)
        check(got, one, np.zeros_like(one), np.array([res], np.float32), min_points=1, what='N = 1')
        assert got[0].tolist() == [lab] and got[3].tolist() == [stats]
    p, f, r, per = [np.copy(x) if isinstance(x, np.ndarray) else x for x in the_scene(1000)]
    got = run(p, f, np.zeros_like(r), **SCENE_KW)                          # no movers at all
    assert got[3].tolist() == [[0, 0, 0, 0]] and bool((got[0] == -1).all()) and not bool(got[2].any())
    assert bool((got[1][0, :, 0] == -1).all()) and not bool(got[1][0, :, 1].any())
    box = 1000 - 6 * per
    p[0, box + 1], p[1, box + 2], f[2, box + 3], f[0, box + 4] = np.nan, np.inf, np.nan, -np.inf
    r[box + 5], r[box + 6], r[3] = np.nan, np.inf, np.inf
    p[2, box + 7], p[0, 5], r[5] = 1e30, -1e30, 1.0
    p[1, 6], r[6] = np.nan, np.nan
    got = run(p, f, r, **SCENE_KW)
    st = check(got, p, f, r, what='non-finite', **SCENE_KW)
    lab = got[0].cpu().numpy()
    assert lab[[box + 1, box + 2, box + 3, box + 4, box + 5, 6]].tolist() == [-1] * 6 and lab[[box + 7, 5]].tolist() == [-3, -3]
    assert lab[box + 6] >= 0 and lab[3] == -2 and st[0, 3] == 2
    assert bool(torch.isfinite(got[2]).all())
    assert [x.shape for x in ops.motion_segment(dev(p[:, :0]), dev(f[:, :0]), dev(r[:0]), prefix=[0, 0, 0], max_objects=4)] == \
        [(0,), (2, 4, 2), (2, 4, 6), (2, 4)]                              # N = 0: no launch


def test_operand_forms_are_read_in_place():
    from hplflownet_amd import ops
    n, B, nmax = 1000, 3, 1500
    p, f, r, _ = the_scene(n)
    want = ops.motion_segment(dev(p), dev(f), dev(r), **SCENE_KW)
    rows = dev(f.T.copy())                                                 # the forward's point-major [N, 3] rows
    assert same(want, ops.motion_segment(dev(p), rows, dev(r), **SCENE_KW))
    assert same(want, ops.motion_segment(dev(p), rows.t(), dev(r), **SCENE_KW))
    wide_p = torch.full((B, 3, nmax), float('nan'), device=DEV)
    wide_f = torch.full((B, 3, nmax), float('nan'), device=DEV)
    wide_p[1, :, 7:7 + n], wide_f[1, :, 7:7 + n] = dev(p), dev(f)
    a, b = wide_p[1][:, 7:7 + n], wide_f[1][:, 7:7 + n]
    assert not a.is_contiguous() and a.stride(0) == nmax
    out = torch.empty(n, dtype=torch.int32, device=DEV)
    got = ops.motion_segment(a, b, dev(r), out=out, **SCENE_KW)
    assert got[0] is out and same(want, got)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide_p[1][:, :7]).all()) and bool(torch.isnan(wide_f[1][:, 7 + n:]).all())


def test_same_bits_twice_and_beside_a_busy_stream():
    from hplflownet_amd import ops
    p, f, _, _ = the_scene(4099)
    tp, tf, tr = dev(p), dev(f), torch.ones(4099, device=DEV)
    first = ops.motion_segment(tp, tf, tr, **SCENE_KW)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    busy = ops.motion_segment(tp, tf, tr, **SCENE_KW)
    torch.cuda.synchronize()
    assert same(first, busy)


# ----------------------------------------------------------------------------- flownet.segment_motion
def test_segment_motion_and_object_fits():
    import hplflownet_amd as H
    from hplflownet_amd import ops
    p, f, _, per = the_scene(4099)
    tp, tf = dev(p), dev(f)
    fit = ops.rigid_fit(tp, tf, iters=4, tau=0.1, return_residual=True)
    want = ops.motion_segment(tp, tf, fit[4], **SCENE_KW)
    got = H.segment_motion(tp, tf, **SCENE_KW)
    assert len(got) == 4 and same(want, got)
    assert same(want, H.segment_motion(tp, tf, rigid=fit, **SCENE_KW))
    assert same(want, H.segment_motion(tp[None], tf[None], **SCENE_KW))
    assert same(want, H.segment_motion([tp], [tf.t().contiguous().t()[None]], **SCENE_KW))
    # the fitted ego-motion leaves the boxes as the movers: the six objects of the scene
    res = fit[4].cpu().numpy()
    o = segment(p, f, res, **SCENE_KW)
    assert o['stats'].tolist() == [6 * per, 6, 6 * per, 0] and np.array_equal(got[0].cpu().numpy(), o['labels'])
    labels, info, motion, stats, fits = H.segment_motion(tp, tf, object_fits=True, **SCENE_KW)
    assert same(want, (labels, info, motion, stats)) and len(fits) == 1
    R, t, st = [x.cpu().numpy() for x in fits[0]]
    assert R.shape == (6, 3, 3) and t.shape == (6, 3) and st.shape == (6, 4)
    eps = 8 * 2.0 ** -24
    for k in range(6):
        member = o['labels'] == k
        pk, fk = p[:, member], f[:, member]
        o64, o32 = rigid_oracle.fit(pk, fk, None, 4, 0.1, np.float64), rigid_oracle.fit(pk, fk, None, 4, 0.1, np.float32)
        scale = float((np.abs(pk) + np.abs(fk)).max())
        bar_R = max(float(np.abs(o32['R'] - o64['R']).max()), eps)
        bar_t = max(float(np.abs(o32['t'] - o64['t']).max()), eps * scale)
        eR, et = float(np.abs(R[k] - o64['R']).max()), float(np.abs(t[k] - o64['t']).max())
        print('object %d: |R - oracle| %.3g (bar %.3g)  |t - oracle| %.3g (bar %.3g)' % (k, eR, bar_R, et, bar_t))
        assert st[k, 0] == o64['status'] == 1 and eR <= bar_R and et <= bar_t


# ----------------------------------------------------------------------------- validate(segment=...)
class _Pairs(list):
    has_cameras = False


def test_validate_segment_keys_on_a_whole_model():
    from hplflownet_amd import engine, ops
    from hplflownet_amd.flownet import rigid_refine
    tr = engine.Trainer('HPLFlowNetShallow', torch.device('cuda', torch.cuda.current_device()))
    data = _Pairs()
    for i, n in enumerate((512, 512, 400)):
        p, f, _, _ = scene(n, 50 + i)
        data.append((dev(p), dev(p + f), dev(f)))
    rigid, seg = {'iters': 2, 'tau': 0.1}, {'eps': 1.0, 'dv': 0.5, 'min_points': 3}
    plain = tr.validate(data, rigid=rigid)
    res = tr.validate(data, rigid=rigid, segment=seg)
    assert list(res) == list(plain) + ['seg_objects', 'seg_moving', 'seg_noise']
    assert all(res[k] == plain[k] for k in plain)
    batched = tr.validate(data, batch_size=4, ragged=True, rigid=rigid, segment=seg)
    assert list(batched) == list(res)
    # by hand: the same forwards, then the fit and ops.motion_segment per pair
    tr.model.eval()
    rows = []
    with torch.no_grad():
        for s_ in data:
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))
            fit = rigid_refine(s_[0], flow[0], return_residual=True, **rigid)
            st = ops.motion_segment(s_[0], flow[0], fit[4], tau=0.1, **seg)[3][0].tolist()
            n = s_[0].shape[1]
            rows.append((float(st[1]), st[2] / n, (st[0] - st[2]) / n))
    for j, k in enumerate(('seg_objects', 'seg_moving', 'seg_noise')):
        assert res[k] == sum(r[j] for r in rows) / len(rows), k
    print(res)
    with pytest.raises(engine.HplError):
        tr.validate(data, segment=seg)
