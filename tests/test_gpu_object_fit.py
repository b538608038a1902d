"""GPU: hpl_object_fit / ops.object_fit, flownet.segment_motion(object_fits='device'), flownet.piecewise_rigid and
validate(objects=...).

The op promises hpl_rigid_fit's bits per object, so its first oracle is ops.rigid_fit on the members gathered with torch: no
tolerance anywhere in that comparison.  The second is tests/object_fit_oracle.py (numpy, an SVD in place of the quaternion),
with the bars tests/test_gpu_segment.py uses for the object fits: what a float32 fit of the same input loses against the
float64 one, and no less than 8 float32 steps.  The scene's margin at tau (tests/test_object_fit_cpu.py) makes the comparison
of the inlier masks free of ties."""
import numpy as np
import pytest
import torch

import object_fit_oracle as oracle
import rigid_oracle
import segment_oracle
from batch64 import counts64, prefix_of
from object_fit_oracle import MAX_OBJECTS, N, SEED, SIZES, TAU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAYLOAD = 0x7fc12000             # a quiet NaN whose low bits number the row: no kernel writes such a value


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def payload(*shape):
    """A float32 tensor of NaNs, every element with its own payload."""
    n = int(np.prod(shape))
    return (PAYLOAD + torch.arange(n, dtype=torch.int32, device=DEV) % 4096).view(torch.float32).reshape(shape)


_CACHE = {}


def the_scene(variant='clean', other=MAX_OBJECTS):
    """The scene on the host and on the device, made once: dict(p, f, labels, w, out, tp, tf, tl, tw)."""
    key = (variant, other)
    if key not in _CACHE:
        p, f, labels, out = oracle.scene(SEED, other)
        w = rigid_oracle.weights(N, SEED)
        if variant == 'nonfinite':
            p, f, w = oracle.with_non_finite(p, f, labels, w)
        _CACHE[key] = dict(p=p, f=f, labels=labels, w=w, out=out, tp=dev(p), tf=dev(f), tl=dev(labels, np.int32), tw=dev(w))
    return _CACHE[key]


def run(s, weighted=False, iters=4, max_objects=MAX_OBJECTS, fill='payload', prefix=None, **kw):
    """ops.object_fit on a scene dict with fresh in-place arrays -> (obj_Rt, obj_stats, residual, refined)."""
    from hplflownet_amd import ops
    n = s['tp'].shape[1]
    residual = payload(n) if fill == 'payload' else torch.zeros(n, device=DEV)
    refined = payload(n, 3) if fill == 'payload' else torch.zeros(n, 3, device=DEV) if fill == 'zero' else \
        s['tf'].t().contiguous()
    got = ops.object_fit(kw.pop('pc', s['tp']), kw.pop('flow', s['tf']), s['tl'], weight=s['tw'] if weighted else None,
                         max_objects=max_objects, iters=iters, tau=TAU, prefix=prefix, residual=residual, refined=refined, **kw)
    torch.cuda.synchronize()
    assert got[2] is residual and got[3] is refined
    return got


def test_scene_has_the_sizes_labels_and_interleaving_it_states():
    s = the_scene()
    assert N == 24001 and [int((s['labels'] == k).sum()) for k in range(len(SIZES))] == list(SIZES)
    assert sorted(set(s['labels'].tolist()) - set(range(len(SIZES)))) == [-3, -2, -1, MAX_OBJECTS + 7]
    big = np.flatnonzero(s['labels'] == 11)
    assert not np.array_equal(big, np.arange(big[0], big[0] + len(big)))          # interleaved: the gather is no identity


# ----------------------------------------------------------------------------- 1 + 6: the bits of ops.rigid_fit
@pytest.mark.parametrize('iters', [0, 1, 4])
@pytest.mark.parametrize('variant,weighted', [('clean', False), ('clean', True), ('nonfinite', True)])
def test_every_object_has_the_bits_of_rigid_fit_on_its_gathered_members(variant, weighted, iters):
    from hplflownet_amd import ops
    s = the_scene(variant)
    Rt, st, res, ref = run(s, weighted, iters, fill='zero')
    _, _, res2, ref2 = run(s, weighted, iters, fill='flow')
    live = torch.from_numpy(rigid_oracle.base_weights(s['p'], s['f'], s['w'] if weighted else None) > 0).to(DEV)
    for k, n in enumerate(SIZES):
        idx = torch.nonzero(s['tl'] == k)[:, 0]                # ascending
        assert idx.numel() == n
        R, t, stats, rows, r = ops.rigid_fit(s['tp'][:, idx].contiguous(), s['tf'][:, idx].contiguous(),
                                             weight=s['tw'][idx] if weighted else None, iters=iters, tau=TAU, return_residual=True)
        what = 'object %d of %d members' % (k, n)
        assert same(Rt[0, k, :9], R.reshape(9)) and same(Rt[0, k, 9:], t[0]), what
        assert same(st[0, k], stats[0]), what
        assert same(res[idx], r) and same(res2[idx], r), what
        assert same(ref2[idx], rows), what                     # on the input flow's rows: rigid_fit's refined, every row
        inlier = (stats[0, 0] != 0) & live[idx] & (r <= TAU)
        assert same(ref[idx], torch.where(inlier[:, None], rows, torch.zeros_like(rows))), what
    if variant == 'nonfinite':
        assert st[0, :, 0].tolist() == [0, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1] + [0] * 4          # object 6: no weight at all
        assert int((~torch.isfinite(res)).sum()) == 5          # a non-finite member's residual: as rigid_fit leaves it
    else:
        assert st[0, :, 0].tolist() == [0, 0] + [1] * 10 + [0] * 4


# ----------------------------------------------------------------------------- 2: what is not touched
@pytest.mark.parametrize('weighted', [False, True])
def test_rows_outside_the_objects_and_of_non_inliers_keep_their_bits(weighted):
    s = the_scene()
    Rt, st, res, ref = run(s, weighted)
    listed = (s['tl'] >= 0) & (s['tl'] < MAX_OBJECTS)
    assert int(listed.sum()) == sum(SIZES)
    assert same(res[~listed], payload(N)[~listed]) and same(ref[~listed], payload(N, 3)[~listed])
    assert not bool(torch.isnan(res[listed]).any())
    status = torch.cat([st[0, :, 0], torch.zeros(1, device=DEV)])[torch.where(listed, s['tl'], MAX_OBJECTS).long()]
    live = torch.from_numpy(rigid_oracle.base_weights(s['p'], s['f'], s['w'] if weighted else None) > 0).to(DEV)
    inlier = listed & (status != 0) & live & (res <= TAU)
    assert same(ref[~inlier], payload(N, 3)[~inlier]) and not bool(torch.isnan(ref[inlier]).any())
    want = torch.from_numpy(~s['out']).to(DEV) & listed & live & (status != 0)
    assert torch.equal(inlier[s['tl'] >= 4], want[s['tl'] >= 4])          # (the scene's undisplaced members, in every large object)
    eye = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=DEV)
    for k in range(len(SIZES), MAX_OBJECTS):                   # rows of empty objects
        assert same(Rt[0, k], eye) and same(st[0, k], torch.zeros(4, device=DEV))
    share = [float((inlier & (s['tl'] == k)).sum()) / n for k, n in enumerate(SIZES)]
    assert st[0, :len(SIZES), 1].tolist() == [float(np.float32(x)) for x in share]


# ----------------------------------------------------------------------------- 3: against numpy
@pytest.mark.parametrize('weighted', [False, True])
def test_against_the_numpy_restatement(weighted):
    s = the_scene()
    Rt, st, res, ref = [x.cpu().numpy() for x in run(s, weighted)]
    w = s['w'] if weighted else None
    f64 = oracle.fit_objects(s['p'], s['f'], s['labels'], w)[0][0]
    f32 = oracle.fit_objects(s['p'], s['f'], s['labels'], w, dtype=np.float32)[0][0]
    eps = 8 * 2.0 ** -24
    touched = ref.view(np.int32)[:, 0] != payload(N, 3).cpu().numpy().view(np.int32)[:, 0]
    for k, (o64, o32) in enumerate(zip(f64, f32)):
        if o64 is None:
            assert k >= len(SIZES) and st[0, k, 0] == 0
            continue
        idx = o64['members']
        scale = float((np.abs(s['p'][:, idx]) + np.abs(s['f'][:, idx])).max())
        bar_R = max(float(np.abs(o32['R'] - o64['R']).max()), eps)
        bar_t = max(float(np.abs(o32['t'] - o64['t']).max()), eps * scale)
        eR = float(np.abs(Rt[0, k, :9].reshape(3, 3) - o64['R']).max())
        et = float(np.abs(Rt[0, k, 9:] - o64['t']).max())
        print('object %2d (%5d members): status %d  |R - oracle| %.3g (bar %.3g)  |t - oracle| %.3g (bar %.3g)' % (
            k, len(idx), st[0, k, 0], eR, bar_R, et, bar_t))
        assert st[0, k, 0] == o64['status'] and eR <= bar_R and et <= bar_t, k
        assert np.array_equal(touched[idx], o64['inlier']), k


# ----------------------------------------------------------------------------- 4: batch and placement
def _batch_with_the_scene_at(j):
    """The B = 64 batch of tests/batch64.py with the scene as pair j (an empty pair there), pair 1 without a labelled point,
    every other pair random points with labels in -1 .. 3."""
    s = the_scene()
    counts = counts64()
    assert counts[j] == 0
    counts[j] = N
    rng = np.random.RandomState(77)
    p, f, lab = [], [], []
    for b, n in enumerate(counts):
        if b == j:
            p.append(s['p']), f.append(s['f']), lab.append(s['labels'])
            continue
        p.append(rng.uniform(-5, 5, (3, n)).astype(np.float32)), f.append(rng.normal(0, 0.2, (3, n)).astype(np.float32))
        lab.append(np.full(n, -1, np.int32) if b == 1 else rng.randint(-1, 4, n).astype(np.int32))
    p, f, lab = np.concatenate(p, 1), np.concatenate(f, 1), np.concatenate(lab)
    return dict(tp=dev(p), tf=dev(f), tl=dev(lab, np.int32), tw=None), prefix_of(counts)


@pytest.mark.parametrize('j', [0, 31, 63])
def test_same_bits_alone_and_anywhere_in_a_ragged_batch_of_64(j):
    alone = run(the_scene(), iters=2)
    batch, prefix = _batch_with_the_scene_at(j)
    Rt, st, res, ref = run(batch, iters=2, prefix=prefix)
    sl = slice(prefix[j], prefix[j + 1])
    assert same(Rt[j], alone[0][0]) and same(st[j], alone[1][0])
    listed = (the_scene()['tl'] >= 0) & (the_scene()['tl'] < MAX_OBJECTS)
    wrote = ~torch.isnan(alone[3][:, 0])                                      # the inliers of the fitted objects
    assert int(wrote.sum()) > 15000 and not bool((wrote & ~listed).any())
    assert same(res[sl][listed], alone[2][listed]) and same(ref[sl][wrote], alone[3][wrote])
    assert same(res[sl][~listed], payload(prefix[-1])[sl][~listed])           # (a row's payload goes by its place in the batch)
    assert same(ref[sl][~wrote], payload(prefix[-1], 3)[sl][~wrote])
    empty = [b for b in range(64) if prefix[b] == prefix[b + 1]] + [1 if j != 1 else 2]       # no point; no labelled point
    assert len(empty) >= 5
    for b in empty:
        assert st[b].abs().sum().item() == 0 and Rt[b, :, 0::4][:, :3].eq(1).all() and Rt[b].sum().item() == 3 * MAX_OBJECTS
    n1 = slice(prefix[1], prefix[2])
    assert same(res[n1], payload(prefix[-1])[n1])
    assert st[40, :4, 0].tolist() == [1, 1, 1, 1] and st[40, 4:].abs().sum().item() == 0     # the other pairs fit their own


def test_same_bits_beside_a_busy_stream():
    s = the_scene()
    first = run(s, True)
    side = torch.cuda.Stream()
    a = torch.randn(1024, 1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    busy = run(s, True)
    assert all(same(x, y) for x, y in zip(first, busy))


def test_operand_forms_are_read_in_place():
    s = the_scene()
    want = run(s, True)
    wide = torch.full((3, 3, N + 500), float('nan'), device=DEV)
    wide[1, :, 7:7 + N] = s['tp']
    view = wide[1][:, 7:7 + N]
    assert not view.is_contiguous() and view.stride(0) == N + 500
    rows = s['tf'].t().contiguous()                            # the forward's point-major [N, 3] rows
    for kw in (dict(pc=view), dict(flow=rows), dict(flow=rows.t()), dict(pc=view, flow=rows)):
        assert all(same(x, y) for x, y in zip(want, run(s, True, **kw))), list(kw)
    from hplflownet_amd import ops
    out = (torch.empty(1, MAX_OBJECTS, 12, device=DEV), torch.empty(1, MAX_OBJECTS, 4, device=DEV))
    got = ops.object_fit(s['tp'], s['tf'], s['tl'], weight=s['tw'], max_objects=MAX_OBJECTS, tau=TAU, out=out)
    assert len(got) == 2 and got[0] is out[0] and got[1] is out[1] and same(got[0], want[0]) and same(got[1], want[1])
    none = ops.object_fit(s['tp'][:, :0], s['tf'][:, :0], s['tl'][:0], max_objects=4, prefix=[0, 0, 0])     # N = 0: no launch
    assert none[0].shape == (2, 4, 12) and none[0].sum().item() == 24 and none[1].shape == (2, 4, 4) and not bool(none[1].any())


# ----------------------------------------------------------------------------- 5: max_objects
def test_max_objects_bounds_the_table_and_changes_no_row():
    s = the_scene(other=4096)                                  # (its fourth background label, 4103, is outside every table)
    want = run(s, True, max_objects=MAX_OBJECTS)
    for m in (1, 12, 4096):
        Rt, st, res, ref = run(s, True, max_objects=m)
        k = min(m, len(SIZES))
        assert Rt.shape == (1, m, 12) and st.shape == (1, m, 4)
        assert same(Rt[0, :k], want[0][0, :k]) and same(st[0, :k], want[1][0, :k])
        inside = (s['tl'] >= 0) & (s['tl'] < m)
        assert same(res[inside], want[2][inside]) and same(ref[inside], want[3][inside])
        assert same(res[~inside], payload(N)[~inside]) and same(ref[~inside], payload(N, 3)[~inside])     # left alone
        assert st[0, k:].abs().sum().item() == 0 and Rt[0, k:].sum().item() == 3 * (m - k)


# ----------------------------------------------------------------------------- 7: the chain
def test_segment_motion_device_fits_equal_the_read_back_form():
    import hplflownet_amd as H
    p, f, _, per = segment_oracle.scene(4099)
    tp, tf = dev(p), dev(f)
    kw = segment_oracle.SCENE_KW
    labels, info, motion, stats, fits = H.segment_motion(tp, tf, object_fits=True, **kw)
    got = H.segment_motion(tp, tf, object_fits='device', **kw)
    assert len(got) == 5 and all(same(x, y) for x, y in zip(got[:4], (labels, info, motion, stats)))
    Rt, st = got[4]
    R, t, s = fits[0]
    assert R.shape[0] == 6 and Rt.shape == (1, 256, 12) and st.shape == (1, 256, 4)
    assert same(Rt[0, :6, :9], R.reshape(6, 9)) and same(Rt[0, :6, 9:], t) and same(st[0, :6], s)
    assert st[0, :6, 0].tolist() == [1] * 6 and st[0, 6:].abs().sum().item() == 0
    assert len(H.segment_motion(tp, tf, **kw)) == 4


def test_piecewise_rigid_rows_and_input_forms():
    import hplflownet_amd as H
    from hplflownet_amd import ops
    kw = segment_oracle.SCENE_KW
    p, f, _, per = segment_oracle.scene(4099)
    tp, tf = dev(p), dev(f)
    R, t, stats, labels, info, oRt, ost, refined = H.piecewise_rigid(tp, tf, **kw)
    ego = ops.rigid_fit(tp, tf, iters=4, tau=kw['tau'], return_residual=True)
    seg = ops.motion_segment(tp, tf, ego[4], **kw)
    marks = payload(4099, 3)
    obj = ops.object_fit(tp, tf, seg[0], iters=4, tau=kw['tau'], refined=marks)
    assert same(R, ego[0]) and same(t, ego[1]) and same(stats, ego[2]) and same(labels, seg[0]) and same(info, seg[1])
    assert same(oRt, obj[0]) and same(ost, obj[1]) and ost[0, :6, 0].tolist() == [1] * 6
    by_object = bits(marks)[:, 0] != bits(payload(4099, 3))[:, 0]
    by_ego = (ego[4] <= kw['tau']) & (ego[2][0, 0] != 0)
    assert int(by_object.sum()) > 5 * per and int(by_ego.sum()) > 2500 and not bool((by_object & by_ego).any())
    want = torch.where(by_object[:, None], marks, torch.where(by_ego[:, None], ego[3], tf.t()))
    assert refined.shape == (3, 4099) and same(refined.t(), want)
    # every input form: two pairs of 1000 points
    parts = [segment_oracle.scene(1000, 1 + b) for b in range(2)]
    a, b = [dev(x[0]) for x in parts], [dev(x[1]) for x in parts]
    base = H.piecewise_rigid(torch.stack(a), torch.stack(b), **kw)
    assert base[7].shape == (2, 3, 1000) and base[5].shape == (2, 256, 12)
    listed = H.piecewise_rigid(a, [x[None] for x in b], **kw)
    packed = H.piecewise_rigid(torch.cat(a, 1), torch.cat(b, 1), [1000, 1000], **kw)
    for other in (listed, packed):
        assert all(same(x, y) for x, y in zip(base[:7], other[:7]))
    assert same(listed[7][0], base[7][0][None]) and same(listed[7][1], base[7][1][None])
    assert same(packed[7], torch.cat(list(base[7]), 1))
    for i in range(2):
        one = H.piecewise_rigid(a[i], b[i], **kw)
        assert one[7].shape == (3, 1000) and same(one[7], base[7][i]) and same(one[5][0], base[5][i])
        assert same(one[3], base[3][1000 * i:1000 * (i + 1)])
        assert same(H.piecewise_rigid(a[i][None], b[i][None], **kw)[7][0], one[7])
    tight = H.piecewise_rigid(a[0], b[0], obj_iters=0, obj_tau=0.05, **kw)
    by_hand = ops.object_fit(a[0], b[0], tight[3], iters=0, tau=0.05)
    assert same(tight[5], by_hand[0]) and same(tight[6], by_hand[1]) and not same(tight[6], H.piecewise_rigid(a[0], b[0], **kw)[6])


# ----------------------------------------------------------------------------- 8: validate(objects=...)
class _Pairs(list):
    has_cameras = False


def test_validate_objects_keys_on_a_whole_model():
    from hplflownet_amd import engine, ops
    from hplflownet_amd.flownet import piecewise_rigid
    tr = engine.Trainer('HPLFlowNetShallow', torch.device('cuda', torch.cuda.current_device()))
    data = _Pairs()
    for i, n in enumerate((512, 512, 400)):
        p, f, _, _ = segment_oracle.scene(n, 50 + i)
        data.append((dev(p), dev(p + f), dev(f)))
    rigid, seg, objects = {'iters': 2, 'tau': 0.1}, {'eps': 1.0, 'dv': 0.5, 'min_points': 3}, {'iters': 1, 'tau': 0.2}
    before = tr.validate(data, rigid=rigid, segment=seg)
    res = tr.validate(data, rigid=rigid, segment=seg, objects=objects)
    metrics = [k[len('rigid_'):] for k in before if k.startswith('rigid_') and k[len('rigid_'):] in before]
    assert metrics == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers']
    assert list(res) == list(before) + ['piecewise_' + k for k in metrics] + ['piecewise_object_inliers']
    assert all(res[k] == before[k] for k in before)
    batched = tr.validate(data, batch_size=4, ragged=True, rigid=rigid, segment=seg, objects=objects)
    assert list(batched) == list(res) and all(np.isfinite(v) for v in batched.values())
    defaults = tr.validate(data, rigid=rigid, segment=seg, objects={})
    assert defaults == tr.validate(data, rigid=rigid, segment=seg, objects=dict(rigid))
    # by hand: the same forwards, then the chain and the metrics per pair
    tr.model.eval()
    rows = []
    with torch.no_grad():
        for s_ in data:
            flow = tr.model(s_[0][None], s_[1][None], tr.gen.build_native(s_[0], s_[1]))
            out = piecewise_rigid(s_[0], flow[0], obj_iters=1, obj_tau=0.2, **rigid, **seg)
            marks = payload(s_[0].shape[1], 3)
            ops.object_fit(s_[0], flow[0], out[3], iters=1, tau=0.2, refined=marks)
            share = float((bits(marks)[:, 0] != bits(payload(s_[0].shape[1], 3))[:, 0]).sum()) / s_[0].shape[1]
            sums = torch.zeros((1, 8), dtype=torch.float64, device=DEV)
            ops.flow_metrics_pairs([out[7]], [s_[2]], [s_[0]], [None], sums)
            rows.append(dict(ops.flow_metrics_fold(sums[0].cpu().tolist(), False), object_inliers=share))
    for k in metrics + ['object_inliers']:
        assert res['piecewise_' + k] == sum(r[k] for r in rows) / len(rows), k
    print({k: res[k] for k in res if k.startswith('piecewise_')})
    for kw in (dict(rigid=rigid, objects=objects), dict(segment=seg, objects=objects), dict(objects=objects)):
        with pytest.raises(engine.HplError):
            tr.validate(data, **kw)
