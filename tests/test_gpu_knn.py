"""GPU: hpl_knn_interp / ops.knn_interpolate and DenseFlow.query(fill='knn').

The search is exact and its operations and their order are fixed (include/hpl_bcl.h), so idx and dist2 are compared with
torch.equal against the numpy restatement tests/knn_oracle.py.  The interpolation is held within 2e-6 * max(1, max|values|)
of the float64 evaluation of the same weights from the float32 d2: (k + 4) roundings on a convex combination."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from batch64 import counts64, prefix_of
from hplflownet_amd._lib import HplError
from knn_oracle import interpolate64, knn_search
from test_gpu_dense_flow import GOLD, dev, ft3d_tree, make, pair, random_queries

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-8


def bar(values):
    return 2e-6 * max(1.0, float(np.abs(np.asarray(values)).max()))


def cloud(rng, n, lo=-10.0, hi=10.0):
    return rng.uniform(lo, hi, (3, n)).astype(np.float32)


def check_neighbours(ref, val, q, k, idx, d2, out, rp=None, qp=None, what=''):
    """idx / dist2 / out of the device (tensors) against the restatement at k and, by its prefix property, at any smaller k."""
    oi, od = knn_search(ref, q, k, rp, qp)
    assert torch.equal(idx.cpu(), torch.from_numpy(oi)), what
    assert torch.equal(d2.cpu(), torch.from_numpy(od)), what
    want = interpolate64(val, oi, od, EPS)
    got = out.cpu().numpy()
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print('%s k = %d: max |out - float64| = %.3g (bar %.3g)' % (what, k, err, bar(val)))
    assert err <= bar(val), what
    hit = od[0] == 0
    assert np.array_equal(got[hit], np.asarray(val)[oi[0][hit]]), what          # exact hits: the row's bits
    return oi, od


@pytest.mark.parametrize('N', [1, 2, 8192])
@pytest.mark.parametrize('Q', [1, 1000, 300000])
def test_search_and_interpolation_against_the_restatement(N, Q):
    from hplflownet_amd import ops
    rng = np.random.RandomState(N + Q)
    ref, q = cloud(rng, N), cloud(rng, Q, -12, 12)
    val = rng.uniform(-3, 3, (N, 3)).astype(np.float32)
    if N > 2:
        ref[:, 100] = ref[:, 17]                           # duplicate reference points
        ref[:, 4000] = ref[:, 17]
    m = min(Q, N) // 2
    q[:, :m] = ref[:, :m]                                  # queries equal to reference points
    tr, tv, tq = dev(ref), dev(val), dev(q)
    oi, od = knn_search(ref, q, 8)                         # the first k rows of the k = 8 answer are the answer at k
    for k in (1, 3, 8):
        out, idx, d2 = ops.knn_interpolate(tr, tv, tq, k=k, eps=EPS, return_neighbors=True)
        torch.cuda.synchronize()
        assert out.shape == (Q, 3) and idx.shape == (k, Q) and d2.shape == (k, Q)
        assert torch.equal(idx.cpu(), torch.from_numpy(oi[:k])), k
        assert torch.equal(d2.cpu(), torch.from_numpy(od[:k])), k
        want = interpolate64(val, oi[:k], od[:k], EPS)
        got = out.cpu().numpy()
        err = float(np.abs(got - want).max())
        print('N = %d Q = %d k = %d: max |out - float64| = %.3g (bar %.3g)' % (N, Q, k, err, bar(val)))
        assert err <= bar(val)
        hit = od[0] == 0
        assert hit[:m].all()
        assert np.array_equal(got[hit].view(np.int32), val[oi[0][hit]].view(np.int32))
        if N < k:                                          # a pair with fewer than k points
            assert (idx[N:] == -1).all() and torch.isinf(d2[N:]).all()
        assert torch.equal(ops.knn_interpolate(tr, tv, tq, k=k, eps=EPS), out)


def test_strided_inputs_and_wide_values():
    from hplflownet_amd import ops
    rng = np.random.RandomState(5)
    ref, q = cloud(rng, 700), cloud(rng, 1300)
    val = rng.uniform(-100, 100, (700, 16)).astype(np.float32)
    wide_r = torch.full((3, 1000), float('nan'), device=DEV)
    wide_q = torch.full((3, 2000), float('nan'), device=DEV)
    wide_r[:, 100:800] = dev(ref)
    wide_q[:, 3:1303] = dev(q)
    out, idx, d2 = ops.knn_interpolate(wide_r[:, 100:800], dev(val), wide_q[:, 3:1303], k=5, eps=EPS, return_neighbors=True)
    torch.cuda.synchronize()
    check_neighbours(ref, val, q, 5, idx, d2, out, what='row-strided')
    # a transposed (n, 3) buffer: no unit stride along the points, the wrapper packs it
    out2 = ops.knn_interpolate(dev(ref.T.copy()).t(), dev(val), dev(q.T.copy()).t(), k=5, eps=EPS)
    assert torch.equal(out2, out)


def test_single_column_views_of_wider_buffers():
    """A one-point reference cloud and a one-point query set passed as column slices of NaN-filled wide buffers: their rows lie
    a buffer row apart, and the answer is the packed call's."""
    from hplflownet_amd import ops
    rng = np.random.RandomState(11)
    ref, q = cloud(rng, 500), cloud(rng, 700)
    val = dev(rng.uniform(-3, 3, (500, 3)).astype(np.float32))
    wide_r = torch.full((3, 1000), float('nan'), device=DEV)
    wide_q = torch.full((3, 2000), float('nan'), device=DEV)
    wide_r[:, 100:600] = dev(ref)
    wide_q[:, 3:703] = dev(q)
    for i in (3, 400):
        one = wide_q[:, i:i + 1]
        assert not one.is_contiguous()
        got = ops.knn_interpolate(wide_r[:, 100:600], val, one, k=3, eps=EPS, return_neighbors=True)
        want = ops.knn_interpolate(dev(ref), val, dev(q[:, i - 3:i - 2]), k=3, eps=EPS, return_neighbors=True)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(got[1].cpu(), torch.from_numpy(knn_search(ref, q[:, i - 3:i - 2], 3)[0]))
    for j in (100, 350):
        one = wide_r[:, j:j + 1]
        got = ops.knn_interpolate(one, val[j - 100:j - 99], wide_q[:, 3:703], k=3, eps=EPS, return_neighbors=True)
        want = ops.knn_interpolate(dev(ref[:, j - 100:j - 99]), val[j - 100:j - 99], dev(q), k=3, eps=EPS, return_neighbors=True)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert bool((got[1][0] == 0).all()) and bool(torch.isfinite(got[0]).all())
        assert torch.equal(got[2].cpu(), torch.from_numpy(knn_search(ref[:, j - 100:j - 99], q, 3)[1]))


def test_a_query_without_any_neighbour_is_nan():
    """Finite coordinates so far apart that every d2 overflows: no candidate enters, idx = -1, the interpolation is NaN."""
    from hplflownet_amd import ops
    ref = np.array([[1e19, -1e19], [0, 0], [0, 0]], np.float32)
    q = np.array([[-3e19, 1e19], [0, 0], [0, 0]], np.float32)              # the second query sits on the first point
    val = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    out, idx, d2 = ops.knn_interpolate(dev(ref), dev(val), dev(q), k=2, eps=EPS, return_neighbors=True)
    oi, od = knn_search(ref, q, 2)
    assert torch.equal(idx.cpu(), torch.from_numpy(oi)) and torch.equal(d2.cpu(), torch.from_numpy(od))
    assert idx[:, 0].tolist() == [-1, -1] and bool(torch.isnan(out[0]).all())
    assert idx[:, 1].tolist() == [0, -1] and torch.equal(out[1].cpu(), torch.from_numpy(val[0]))
    assert np.isnan(interpolate64(val, oi, od, EPS)[0]).all()


def ragged_case(B, seed):
    rng = np.random.RandomState(seed)
    ns = [int(x) for x in rng.randint(1, 900, B)]
    qs = [int(x) for x in rng.randint(1, 3000, B)]
    ns[-1] = 2                                             # a pair with fewer than k = 3 points
    if B > 2:
        qs[2] = 0                                          # a pair without queries
    refs = [cloud(rng, n, -5, 5) for n in ns]
    qrs = [cloud(rng, n, -5, 5) for n in qs]
    # planted: a point of pair 0 that sits ON pair 1's first queries, nearer than anything pair 1 holds
    qrs[1][:, :20] = refs[0][:, :1] + rng.normal(0, 1e-4, (3, 20)).astype(np.float32)
    vals = [rng.uniform(-2, 2, (n, 3)).astype(np.float32) for n in ns]
    return refs, vals, qrs


@pytest.mark.parametrize('B', [2, 5])
def test_ragged_batches_equal_their_pairs(B):
    from hplflownet_amd import ops
    refs, vals, qrs = ragged_case(B, B)
    rp = np.concatenate([[0], np.cumsum([r.shape[1] for r in refs])]).tolist()
    qp = np.concatenate([[0], np.cumsum([x.shape[1] for x in qrs])]).tolist()
    ref, val, q = np.concatenate(refs, 1), np.concatenate(vals, 0), np.concatenate(qrs, 1)
    out, idx, d2 = ops.knn_interpolate(dev(ref), dev(val), dev(q), k=3, eps=EPS, ref_prefix=rp, q_prefix=qp,
                                       return_neighbors=True)
    torch.cuda.synchronize()
    check_neighbours(ref, val, q, 3, idx, d2, out, rp, qp, what='B = %d' % B)
    for b in range(B):
        sl = slice(qp[b], qp[b + 1])
        own = idx[:, sl]
        assert bool(((own == -1) | ((own >= rp[b]) & (own < rp[b + 1]))).all())        # pair b's queries see pair b's points only
        if qp[b + 1] == qp[b]:
            continue
        o1, i1, s1 = ops.knn_interpolate(dev(refs[b]), dev(vals[b]), dev(qrs[b]), k=3, eps=EPS, return_neighbors=True)
        assert torch.equal(o1, out[sl]) and torch.equal(s1, d2[:, sl])
        assert torch.equal(torch.where(i1 >= 0, i1 + rp[b], i1), own)
    assert int((idx[:, qp[1]:qp[1] + 20] == 0).sum()) == 0                             # the planted point is never returned
    assert bool((idx[2, qp[B - 1]:] == -1).all()) and bool(torch.isinf(d2[2, qp[B - 1]:]).all())


def test_a_batch_of_64_pairs_equals_its_pairs():
    """B = 64 (tests/batch64.py): every pair's outputs are the bits of that pair run alone with its own prefixes, and the
    restatement's.  An empty pair has no queries and no points (queries without points are refused)."""
    from hplflownet_amd import ops
    qs = counts64()
    ns = [0 if n == 0 else 1 + (7 * i) % 500 for i, n in enumerate(qs)]
    ns[1] = 2                                              # a pair with fewer than k = 3 points
    rng = np.random.RandomState(64)
    refs = [cloud(rng, n, -5, 5) for n in ns]
    qrs = [cloud(rng, n, -5, 5) for n in qs]
    vals = [rng.uniform(-2, 2, (n, 3)).astype(np.float32) for n in ns]
    rp, qp = prefix_of(ns), prefix_of(qs)
    ref, val, q = np.concatenate(refs, 1), np.concatenate(vals, 0), np.concatenate(qrs, 1)
    out, idx, d2 = ops.knn_interpolate(dev(ref), dev(val), dev(q), k=3, eps=EPS, ref_prefix=rp, q_prefix=qp,
                                       return_neighbors=True)
    torch.cuda.synchronize()
    check_neighbours(ref, val, q, 3, idx, d2, out, rp, qp, what='B = 64')
    for b in range(64):
        if qs[b] == 0:
            continue
        sl = slice(qp[b], qp[b + 1])
        o1, i1, s1 = ops.knn_interpolate(dev(refs[b]), dev(vals[b]), dev(qrs[b]), k=3, eps=EPS, ref_prefix=[0, ns[b]],
                                         q_prefix=[0, qs[b]], return_neighbors=True)
        assert torch.equal(o1.view(torch.int32), out[sl].view(torch.int32)) and torch.equal(s1, d2[:, sl]), b
        assert torch.equal(torch.where(i1 >= 0, i1 + rp[b], i1), idx[:, sl]), b
    assert bool((idx[2, qp[1]:qp[2]] == -1).all())


def test_coverage_form():
    from hplflownet_amd import ops
    rng = np.random.RandomState(9)
    ref, q = cloud(rng, 3000), cloud(rng, 20000, -12, 12)
    val = rng.uniform(-3, 3, (3000, 3)).astype(np.float32)
    cov = rng.uniform(0, 1, 20000).astype(np.float32)
    cov[rng.rand(20000) < 0.3] = 1.0
    cov[rng.rand(20000) < 0.2] = 0.0
    cov[5000:5600] = 1.0                                   # whole workgroups and waves without work
    base = rng.uniform(-3, 3, (20000, 3)).astype(np.float32)
    out = dev(base)
    res, idx, d2 = ops.knn_interpolate(dev(ref), dev(val), dev(q), k=3, eps=EPS, out=out, coverage=dev(cov),
                                       return_neighbors=True)
    torch.cuda.synchronize()
    assert res is out
    got = out.cpu().numpy()
    full = cov == 1
    assert np.array_equal(got[full].view(np.int32), base[full].view(np.int32))         # their bits stay
    assert bool((idx[:, torch.from_numpy(full).to(DEV)] == -1).all())
    oi, od = knn_search(ref, q, 3)
    assert np.array_equal(idx.cpu().numpy()[:, ~full], oi[:, ~full])
    assert np.array_equal(d2.cpu().numpy()[:, ~full], od[:, ~full])
    c = cov.astype(np.float64)[:, None]
    want = c * base.astype(np.float64) + (1 - c) * interpolate64(val, oi, od, EPS)
    err = float(np.abs(got - want)[~full].max())
    print('coverage form: max |out - float64 blend| = %.3g (bar %.3g)' % (err, bar(val)))
    assert err <= bar(val)
    plain = ops.knn_interpolate(dev(ref), dev(val), dev(q), k=3, eps=EPS)
    zero = torch.from_numpy(cov == 0).to(DEV)
    assert torch.equal(out[zero], plain[zero])             # coverage 0: the interpolation itself
    with pytest.raises(HplError):
        ops.knn_interpolate(dev(ref), dev(val), dev(q), out=out)                        # out without coverage


def test_same_bits_beside_a_busy_stream():
    from hplflownet_amd import ops
    rng = np.random.RandomState(3)
    ref, q = dev(cloud(rng, 8192)), dev(cloud(rng, 100000))
    val = dev(rng.uniform(-3, 3, (8192, 3)).astype(np.float32))
    alone = ops.knn_interpolate(ref, val, q, k=3, return_neighbors=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(40):
            a = torch.tanh(a @ a * 1e-3)
    busy = ops.knn_interpolate(ref, val, q, k=3, return_neighbors=True)
    torch.cuda.synchronize()
    for x, y in zip(alone, busy):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- DenseFlow.query(fill='knn')
def fill_queries(p1, p2, n, seed):
    """pc1 itself (coverage 1), jittered pc1 and pc2 points (partial coverage), points far outside the box (coverage 0)."""
    rng = np.random.RandomState(seed)
    far = (p1.max(1, keepdims=True) + 50 + rng.uniform(0, 5, (3, 64))).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([p1, random_queries(p1, p2, n, seed), far], 1))


@pytest.mark.parametrize('nsc', [7, 5])
def test_dense_fill_single_pair(nsc, monkeypatch):
    import hplflownet_amd as H
    from hplflownet_amd import ops
    m, gen = make(nsc, monkeypatch)
    p1, p2 = pair(2048, 3)
    t1, t2 = dev(p1), dev(p2)
    q = dev(fill_queries(p1, p2, 1500, 2))
    lat = gen.build_native(t1, t2)
    df = H.DenseFlow(m)
    with torch.no_grad():
        ref = m(t1[None], t2[None], lat)
        flow, state = df.forward(t1[None], t2[None], lat)
        assert torch.equal(flow, ref)                                   # the forward is unchanged
        plain, cov = df.query(state, q)
        again, cov2 = df.query(state, q, fill=None)
        assert torch.equal(plain, again) and torch.equal(cov, cov2)     # fill=None: the path without the argument
        for k in (3, 1):
            filled, fcov = df.query(state, q, fill='knn', k=k)
            interp = ops.knn_interpolate(t1, ref[0].t().contiguous(), q, k=k)
            torch.cuda.synchronize()
            assert torch.equal(fcov, cov)                               # coverage as the lattice gave it
            n1 = p1.shape[1]
            assert bool((cov[:n1] == 1).all()) and bool((cov[-64:] == 0).all())
            one, zero = cov == 1, cov == 0
            part = ~one & ~zero
            assert int(part.sum()) > 100
            assert torch.equal(filled[:, one], plain[:, one])           # queries equal to pc1 (every covered one): fill=None's bits
            assert torch.equal(filled[:, zero], interp.t()[:, zero])    # coverage 0: the interpolation of the forward's flow
            c = cov.double()
            want = c * plain.double() + (1 - c) * interp.t().double()
            err = float((filled.double() - want)[:, part].abs().max())
            # the blend's two inputs are the forward's flow rows (the values) AND the lattice answer (the base row): both scale it
            lim = 2e-6 * max(1.0, float(ref.abs().max()), float(plain.abs().max()))
            print('nsc %d k %d: blend error %.3g (bar %.3g), %d partial' % (nsc, k, err, lim, int(part.sum())))
            assert err <= lim
        first, _ = df.query(state, q, fill='knn')
        flow.zero_()                                                    # the state keeps rows of its own once it has filled
        again, _ = df.query(state, q, fill='knn')
        assert torch.equal(first, again)
        with pytest.raises(HplError):
            df.query(state, q, fill='knn', renormalize=False)
        with pytest.raises(HplError):
            df.query(state, q, fill='nearest')
        for k in (0, 9, 2.0):
            with pytest.raises(HplError):
                df.query(state, q, fill='knn', k=k)


@pytest.mark.skipif(os.environ.get('HPL_MATH') == 'f32', reason='this test starts the f32 run itself')
def test_dense_fill_f32():
    env = dict(os.environ, HPL_MATH='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_knn.py') + '::test_dense_fill_single_pair'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize('ragged', [False, True])
def test_dense_fill_batches_match_single_pairs(ragged, monkeypatch):
    import hplflownet_amd as H
    m, gen = make(7, monkeypatch)
    n = [(1024, 1024), (1024, 1024)] if not ragged else [(900, 1000), (1200, 800)]
    pairs = [pair(max(a, b), 11 + i) for i, (a, b) in enumerate(n)]
    pcs1 = [dev(p[0][:, :a]) for p, (a, b) in zip(pairs, n)]
    pcs2 = [dev(p[1][:, :b]) for p, (a, b) in zip(pairs, n)]
    qs = [dev(fill_queries(p[0][:, :a], p[1][:, :b], 600, 3 + i)) for i, (p, (a, b)) in enumerate(zip(pairs, n))]
    qs[0] = torch.cat([qs[0], pcs1[1]], 1)        # pair 1's sample as queries of pair 0: they may only see pair 0's sample
    df = H.DenseFlow(m)
    with torch.no_grad():
        if ragged:
            lat = gen.build_native_batch(pcs1, pcs2)
            flow, state = df.forward(pcs1, pcs2, lat)
            assert all(torch.equal(a, b) for a, b in zip(flow, m(pcs1, pcs2, lat)))
        else:
            lat = gen.build_native_batch(torch.stack(pcs1), torch.stack(pcs2))
            flow, state = df.forward(torch.stack(pcs1), torch.stack(pcs2), lat)
            assert torch.equal(flow, m(torch.stack(pcs1), torch.stack(pcs2), lat))
        plain, pc = df.query(state, qs)
        filled, fc = df.query(state, qs, fill='knn')
        for b in range(2):
            single = gen.build_native(pcs1[b], pcs2[b])
            sflow, st1 = df.forward(pcs1[b][None], pcs2[b][None], single)
            sp, sc = df.query(st1, qs[b])
            sf, sc2 = df.query(st1, qs[b], fill='knn')
            torch.cuda.synchronize()
            assert torch.equal(sc, fc[b]) and torch.equal(sc, pc[b]) and torch.equal(sc, sc2)
            # the batch's lattice answer is within the dense-flow bar of the pair's; the fill adds (1 - c) * interpolation of the
            # forwards' flows, which agree within the same bar: so do the filled answers
            lim = 2e-4 * max(1.0, float(sf.abs().max()))
            assert float((plain[b] - sp).abs().max()) <= lim
            assert float((filled[b] - sf).abs().max()) <= lim
            fb = flow[b][0] if ragged else flow[b]
            same = torch.equal(fb, sflow[0]) and torch.equal(plain[b], sp)
            print('ragged %s pair %d: the batch gave its pair\'s forward and lattice bits: %s (then the filled bits are compared '
                  'exactly)' % (ragged, b, same))
            if same:
                assert torch.equal(filled[b], sf)                       # the same inputs: the same bits
            zero = sc == 0
            assert int(zero.sum()) >= 64
            from hplflownet_amd import ops
            own = ops.knn_interpolate(pcs1[b], fb.t().contiguous(), qs[b], k=3)
            assert torch.equal(filled[b][:, zero], own.t()[:, zero])    # pair b's uncovered queries: pair b's sample only


# ----------------------------------------------------------------------------- engine --evaluate --dense --dense-fill knn
BASE = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'FlyingThings3DSubset']


def test_engine_fill_on_frames_the_sample_covers(tmp_path):
    """Frames smaller than --points: every coverage is 1, nothing is filled, the dense values are bit-equal."""
    from hplflownet_amd import engine
    root = str(tmp_path)
    ft3d_tree(root, 3, [400, 450, 380])
    plain = engine.main(BASE + ['--data-root', root, '--dense'])
    res = engine.main(BASE + ['--data-root', root, '--dense', '--dense-fill', 'knn'])
    assert list(res) == list(plain)
    assert res == plain and res['dense_full'] == 1.0


def test_engine_fill_on_larger_frames_equals_a_query_by_hand(tmp_path):
    import hplflownet_amd as H
    from hplflownet_amd import data as data_mod
    from hplflownet_amd import engine, ops
    root = str(tmp_path)
    ft3d_tree(root, 2, 3000)
    args = BASE + ['--data-root', root, '--dense']
    plain = engine.main(args)
    res = engine.main(args + ['--dense-fill', 'knn', '--dense-k', '4'])
    assert list(res) == list(plain)
    keys = [k for k in res if not k.startswith('dense_')]
    assert all(res[k] == plain[k] for k in keys)                        # the sampled metrics do not move
    assert res['dense_coverage'] == plain['dense_coverage'] and res['dense_full'] == plain['dense_full'] < 1
    assert any(res['dense_' + k] != plain['dense_' + k] for k in keys)
    # by hand: the engine's own reader and model, then query(fill='knn') and the metrics op
    tr = engine.Trainer('HPLFlowNetShallow', torch.device('cuda', torch.cuda.current_device()))
    tr.model.eval()
    reader = data_mod.FlyingThings3DSubset(False, data_mod.ProcessData(engine.DATA_PROCESS, 512, True, seed=0), root,
                                           device=tr.device)
    val = engine.DenseFrames(reader, data_mod.ProcessData(engine.DATA_PROCESS, 0, True, seed=0))
    sums = torch.zeros((len(val), 8), dtype=torch.float64, device=DEV)
    df = H.DenseFlow(tr.model)
    with torch.no_grad():
        for i in range(len(val)):
            s_ = val[i]
            lat = tr.gen.build_native(s_[0], s_[1])
            _, state = df.forward(s_[0][None], s_[1][None], lat)
            qf, _ = df.query(state, s_.dense[0], fill='knn', k=4)
            ops.flow_metrics_pairs([qf], [s_.dense[2]], [s_.dense[0]], [getattr(s_, 'camera', None)], sums, i)
        words = sums.cpu().numpy()
    cams = bool(getattr(val, 'has_cameras', False))
    folds = [ops.flow_metrics_fold(w, cams) for w in words]
    for k in keys:
        assert res['dense_' + k] == sum(f[k] for f in folds) / len(folds), k


def test_engine_fill_kitti_ragged(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    frames = [str(f) for f in np.load(os.path.join(GOLD, 'metrics2d.npz'))['kitti_frames']]
    for fr in frames:
        d = os.path.join(root, 'KITTI_processed_occ_final', fr)
        os.makedirs(d)
        rng = np.random.RandomState(int(fr))
        m = 900 + 150 * int(fr) % 400
        pc = np.stack([rng.uniform(-5, 5, m), rng.uniform(-1, 1, m), rng.uniform(3, 30, m)], 1).astype(np.float32)
        np.save(os.path.join(d, 'pc1.npy'), pc)
        np.save(os.path.join(d, 'pc2.npy'), pc + rng.normal(0, 0.1, pc.shape).astype(np.float32))
    args = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'KITTI', '--data-root', root,
            '--kitti-calib', os.path.join(GOLD, 'kitti_calib'), '--dense', '--batch-size', '2', '--ragged']
    plain = engine.main(args)
    res = engine.main(args + ['--dense-fill', 'knn'])
    assert list(res) == list(plain)
    for k in res:
        assert np.isfinite(res[k]), k
    assert res['dense_coverage'] == plain['dense_coverage'] and res['EPE3D'] == plain['EPE3D']
    assert res['dense_EPE3D'] != plain['dense_EPE3D']


def test_engine_argument_errors():
    from hplflownet_amd import engine
    for extra in (['--dense-fill', 'knn'], ['--dense', '--dense-k', '3'], ['--dense', '--dense-fill', 'knn', '--dense-k', '9'],
                  ['--dense', '--dense-fill', 'nearest']):
        with pytest.raises(SystemExit):
            engine.parse_args(BASE + ['--data-root', '/nonexistent'] + extra)
