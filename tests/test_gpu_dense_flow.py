"""GPU: dense scene flow (flownet.DenseFlow) -- flow at any query points from one sampled forward.

hpl_lattice_query locates queries in level 0 of cloud 1 of a finished lattice; the head slices the activation the last Up
layer slices there.  Checked: queries equal to pc1 give pc1's own lattice rows and the forward's flow; random queries match a
numpy restatement over the C oracle's keys (exact ids / weights / coverage, range check included, aliasing keys refused); the
query head against a float64 torch head; chunks and both sides of the trailing 1x1; equal and ragged batches against their
pairs' single-pair runs; the staged fallback; the forward unchanged; refusals before any launch."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from dense_oracle import NpQuery, np_pack
from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(nsc, monkeypatch, fused=True):
    import hplflownet_amd as H
    monkeypatch.setenv('HPL_LATTICE_FUSED', '1' if fused else '0')
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:nsc], evaluate=True, use_leaky=True,
                                 bcn_use_bias=True, bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = (H.HPLFlowNet if nsc == 7 else H.HPLFlowNetShallow)(args)
    fill_module_(m, 1.0, 'hash')
    m = m.to(DEV).eval()
    gen = H.GenerateDataUnsymmetric(args, device=DEV, wide_up=m.lattice_hint())
    assert gen.native_builder().fused == fused
    return m, gen


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def bar(ref):
    return 2e-4 * max(1.0, float(ref.abs().max()))


def locate(df, state, q, renorm=True):
    cov = torch.empty(q.shape[1], dtype=torch.float32, device=DEV)
    bary, off = df.locate(state, q.contiguous(), [0, q.shape[1]], renorm, cov)
    return off.cpu().numpy(), bary.cpu().numpy(), cov.cpu().numpy()


def head64(m, Z, bary, off):
    """float64 torch restatement of the query head over Z read back."""
    Z = Z.double()
    layer = m.bcn1_
    mods = list(layer.blur_conv)
    from hplflownet_amd.bcl import _ConvReLU, _conv_of
    w = bary.double()
    z = sum(w[r][:, None] * Z[off[r].long()] for r in range(4))
    bias = layer.bias.double().reshape(-1) if layer.use_bias else 0
    if len(mods) >= 2 and not isinstance(mods[-1], _ConvReLU):
        c = _conv_of(mods[-1])
        z = z @ c.weight.double().reshape(c.weight.shape[0], -1).t() + c.bias.double() + bias
    else:
        z = z + bias

    def conv(x, c, act):
        y = x @ c.weight.double().reshape(c.weight.shape[0], -1).t() + c.bias.double()
        return torch.where(y > 0, y, 0.1 * y) if act else y
    y = conv(z, m.conv2.conv, True)
    y = conv(y, m.conv3.conv, True)
    return conv(y, m.conv4, False).t()


def pair(n, seed):
    a, b, _ = synthetic_pair(n, seed)
    return a.T.copy(), b.T.copy()


@pytest.mark.parametrize('nsc', [7, 5])
def test_queries_equal_to_pc1(nsc, monkeypatch):
    import hplflownet_amd as H
    m, gen = make(nsc, monkeypatch)
    p1, p2 = pair(2048, 3)
    t1, t2 = dev(p1), dev(p2)
    lat = gen.build_native(t1, t2)
    df = H.DenseFlow(m)
    with torch.no_grad():
        ref = m(t1[None], t2[None], lat)
        flow, state = df.forward(t1[None], t2[None], lat)
        assert torch.equal(flow, ref)                       # the forward is unchanged
        off, bary, cov = locate(df, state, t1)
        c0 = lat.levels[0].clouds[0]
        assert np.array_equal(off, c0.off.cpu().numpy())
        assert np.array_equal(bary.view(np.int32), c0.bary.cpu().numpy().view(np.int32))
        assert (cov == 1).all()
        qf, qc = df.query(state, t1)
        torch.cuda.synchronize()
    assert qf.shape == (3, 2048) and qc.shape == (2048,)
    assert float((qf - ref[0]).abs().max()) <= bar(ref)


@pytest.mark.skipif(os.environ.get('HPL_MATH') == 'f32', reason='this test starts the f32 run itself')
def test_queries_equal_to_pc1_f32():
    env = dict(os.environ, HPL_MATH='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_dense_flow.py') + '::test_queries_equal_to_pc1'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def random_queries(p1, p2, n, seed):
    rng = np.random.RandomState(seed)
    jit = p1[:, rng.randint(0, p1.shape[1], n)] + rng.normal(0, 0.05, (3, n)).astype(np.float32)
    on2 = p2[:, rng.randint(0, p2.shape[1], n // 2)]
    lo, hi = p1.min(1, keepdims=True), p1.max(1, keepdims=True)
    out = lo + (hi - lo) * rng.uniform(-0.5, 1.5, (3, n // 2)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([jit, on2, out], 1).astype(np.float32))


@pytest.mark.parametrize('fused', [True, False])
def test_random_queries_against_numpy(fused, monkeypatch):
    import hplflownet_amd as H
    m, gen = make(7, monkeypatch, fused)
    p1, p2 = pair(1024, 5)
    lat = gen.build_native(dev(p1), dev(p2))
    df = H.DenseFlow(m)
    npq = NpQuery(p1, p2)
    q = random_queries(p1, p2, 1500, 1)
    with torch.no_grad():
        _, state = df.forward(dev(p1)[None], dev(p2)[None], lat)
        for renorm in (False, True):
            off, bary, cov = locate(df, state, dev(q), renorm)
            o2, b2, c2, _ = npq(q, renorm)
            assert np.array_equal(off, o2) and np.array_equal(bary, b2) and np.array_equal(cov, c2)
        assert 0 < (cov == 0).sum() < q.shape[1] and 0 < (cov == 1).sum() < q.shape[1]
        qf, qc = df.query(state, dev(q))
        ref = head64(m, state.Z, torch.from_numpy(bary).to(DEV), torch.from_numpy(off).to(DEV))
        torch.cuda.synchronize()
    assert float((qf.double() - ref).abs().max()) <= bar(ref)


def alias_queries(npq, count=8):
    """Points at lattice vertices k' outside the key range whose packed key equals that of a real vertex k of pc1: k' - k = d with
    sum(d) = 0, all d_i of one residue mod 4 (k' is a lattice point) and d3 + r3 (d2 + r2 (d1 + r1 d0)) = 0 (key2int's value)."""
    from oracle import lattice_oracle as LO
    mm = npq.mm
    r = [int(mm[4 + i] - mm[i] + 1) for i in range(4)]
    E = LO.elevate_matrix().astype(np.float64)
    stdf = 4 * np.sqrt(2 / 3)
    a = np.arange(-4 * max(r) ** 2, 4 * max(r) ** 2 + 1)
    d1, d2 = np.meshgrid(a, a, indexing='ij')
    out = []
    for d0 in range(-8, 9):
        d3 = -r[3] * (d2 + r[2] * (d1 + r[1] * d0))
        ok = (d0 + d1 + d2 + d3 == 0) & ((d1 - d0) % 4 == 0) & ((d2 - d0) % 4 == 0) & ((d3 - d0) % 4 == 0) & \
            ((d0 != 0) | (d1 != 0) | (d2 != 0))
        for i, j in zip(*np.nonzero(ok)):
            d = np.array([d0, d1[i, j], d2[i, j], d3[i, j]])
            for k in npq.ids:
                kp = np.array(k) + d
                if all(mm[x] <= kp[x] <= mm[4 + x] for x in range(4)):
                    continue
                assert np_pack(kp, mm) == np_pack(k, mm)
                out.append(np.linalg.lstsq(E, kp.astype(np.float64), rcond=None)[0] / (stdf * npq.scale))
                if len(out) >= count:
                    return np.ascontiguousarray(np.array(out, np.float32).T)
    return np.ascontiguousarray(np.array(out, np.float32).T)


def test_aliasing_keys_are_missing(monkeypatch):
    """Queries whose simplex vertices lie outside the key range but pack onto real vertices of pc1: without the range check
    they would find those vertices; they must be missing, coverage 0."""
    import hplflownet_amd as H
    m, gen = make(5, monkeypatch)
    rng = np.random.RandomState(2)
    p1 = (rng.uniform(-0.05, 0.05, (3, 6)) + np.array([[0.], [0.], [1.]])).astype(np.float32)
    p2 = (p1 + 0.01).astype(np.float32)
    lat = gen.build_native(dev(p1), dev(p2))
    df = H.DenseFlow(m)
    npq = NpQuery(p1, p2)
    q = alias_queries(npq)
    o2, b2, c2, aliased = npq(q, True)
    assert q.shape[1] == 8 and aliased.all() and (c2 == 0).all()
    q = np.ascontiguousarray(np.concatenate([q, p1, random_queries(p1, p2, 200, 3)], 1))
    o2, b2, c2, aliased = npq(q, True)
    with torch.no_grad():
        _, state = df.forward(dev(p1)[None], dev(p2)[None], lat)
        off, bary, cov = locate(df, state, dev(q), True)
    assert np.array_equal(off, o2) and np.array_equal(bary, b2) and np.array_equal(cov, c2)
    assert (cov[:8] == 0).all() and (cov[8:14] == 1).all()


def test_chunks_and_both_sides_of_the_trailing_1x1(monkeypatch):
    import hplflownet_amd as H
    m, gen = make(7, monkeypatch)
    p1, p2 = pair(1024, 7)
    lat = gen.build_native(dev(p1), dev(p2))
    df = H.DenseFlow(m)
    H0 = lat.H[0][0]
    with torch.no_grad():
        _, state = df.forward(dev(p1)[None], dev(p2)[None], lat)
        for n in (H0 // 2, 2 * H0):          # after the slice / on the vertices
            q = dev(random_queries(p1, p2, n // 2, n)[:, :n])
            a, ca = df.query(state, q, chunk=q.shape[1])
            b, cb = df.query(state, q, chunk=1000)
            off, bary, cov = locate(df, state, q)
            ref = head64(m, state.Z, torch.from_numpy(bary).to(DEV), torch.from_numpy(off).to(DEV))
            torch.cuda.synchronize()
            assert torch.equal(ca, cb)
            assert float((a.double() - ref).abs().max()) <= bar(ref)
            assert float((b.double() - ref).abs().max()) <= bar(ref)


@pytest.mark.parametrize('ragged', [False, True])
def test_batches_match_single_pairs(ragged, monkeypatch):
    import hplflownet_amd as H
    m, gen = make(7, monkeypatch)
    n = [(1024, 1024), (1024, 1024)] if not ragged else [(900, 1000), (1200, 800)]
    pairs = [pair(max(a, b), 11 + i) for i, (a, b) in enumerate(n)]
    pcs1 = [dev(p[0][:, :a]) for p, (a, b) in zip(pairs, n)]
    pcs2 = [dev(p[1][:, :b]) for p, (a, b) in zip(pairs, n)]
    qs = [dev(random_queries(p[0][:, :a], p[1][:, :b], 600, 3 + i)) for i, (p, (a, b)) in enumerate(zip(pairs, n))]
    # pair 0's queries also hold pair 1's points: as queries of pair 0 they may only find pair 0's vertices
    qs[0] = torch.cat([qs[0], pcs1[1]], 1)
    df = H.DenseFlow(m)
    with torch.no_grad():
        if ragged:
            lat = gen.build_native_batch(pcs1, pcs2)
            flow, state = df.forward(pcs1, pcs2, lat)
            ref = m(pcs1, pcs2, lat)
            assert all(torch.equal(a, b) for a, b in zip(flow, ref))
        else:
            lat = gen.build_native_batch(torch.stack(pcs1), torch.stack(pcs2))
            flow, state = df.forward(torch.stack(pcs1), torch.stack(pcs2), lat)
            assert torch.equal(flow, m(torch.stack(pcs1), torch.stack(pcs2), lat))
        qf, qc = df.query(state, qs)
        cov = torch.empty(sum(q.shape[1] for q in qs), dtype=torch.float32, device=DEV)
        pre = [0, qs[0].shape[1], qs[0].shape[1] + qs[1].shape[1]]
        bary, off = df.locate(state, torch.cat(qs, 1).contiguous(), pre, True, cov)
        H00 = int(lat.pair_counts[0, 0, 0])
        assert int(off[:, :pre[1]].max()) < H00                 # pair 0 never reaches a vertex of pair 1
        assert int(off[:, pre[1]:][bary[:, pre[1]:] > 0].min()) >= H00
        for b in range(2):
            single = gen.build_native(pcs1[b], pcs2[b])
            _, st1 = df.forward(pcs1[b][None], pcs2[b][None], single)
            sf, sc = df.query(st1, qs[b])
            torch.cuda.synchronize()
            assert torch.equal(sc, qc[b])
            assert float((qf[b] - sf).abs().max()) <= bar(sf)


def test_staged_fallback(monkeypatch):
    """A pair that outgrew a level-0 bound is rebuilt by the staged driver: its own level-0 table answers the queries."""
    import hplflownet_amd as H
    m, gen = make(7, monkeypatch)
    nb = gen.native_builder()
    p1, p2 = pair(1024, 9)
    q = random_queries(p1, p2, 800, 4)
    npq = NpQuery(p1, p2)
    df = H.DenseFlow(m)
    nb.bounds = [0] * 8
    nb.seen = [0] * 8
    nb.bounds[0] = 16
    before = nb.fallbacks
    lat = gen.build_native(dev(p1), dev(p2))
    with torch.no_grad():
        torch.cuda.synchronize()
        assert nb.fallbacks == before + 1 and lat.query_info.keys is not None
        _, state = df.forward(dev(p1)[None], dev(p2)[None], lat)
        off, bary, cov = locate(df, state, dev(q), True)
    o2, b2, c2, _ = npq(q, True)
    assert np.array_equal(off, o2) and np.array_equal(bary, b2) and np.array_equal(cov, c2)


def test_refusals(monkeypatch):
    import hplflownet_amd as H
    from hplflownet_amd import _lib
    from oracle import lattice_oracle as LO
    m, gen = make(5, monkeypatch)
    p1, p2 = pair(512, 1)
    t1, t2 = dev(p1), dev(p2)
    lat = gen.build_native(t1, t2)
    df = H.DenseFlow(m)
    with pytest.raises(_lib.HplError):
        df.forward(t1[None], t2[None], lat)                     # grad mode
    with torch.no_grad():
        ref_lat = H.DeviceLattice.from_generated_data(LO.generate_data(p1.T, p2.T, SCALES_FILTER_MAP[:5]), DEV)
        with pytest.raises(_lib.HplError):
            df.forward(t1[None], t2[None], ref_lat)
        with pytest.raises(_lib.HplError):
            df.forward(t1[None, :, :100], t2[None], lat)
        _, state = df.forward(t1[None], t2[None], lat)
        for bad in (t1[:2], t1.double(), [t1, t1], t1.cpu()):
            with pytest.raises(_lib.HplError):
                df.query(state, bad)
        with pytest.raises(_lib.HplError):
            df.query(state, t1, chunk=0)
    with pytest.raises(_lib.HplError):
        df.query(state, t1)                                     # grad mode
    m.train()
    with torch.no_grad(), pytest.raises(_lib.HplError):
        df.forward(t1[None], t2[None], lat)


# ----------------------------------------------------------------------------- engine --evaluate --dense
GOLD = os.path.join(ROOT, 'tests', 'golden')
DENSE_KEYS = ['dense_EPE3D', 'dense_Acc3DS', 'dense_Acc3DR', 'dense_Outliers']


def ft3d_tree(root, count, n):
    for i in range(count):
        d = os.path.join(root, 'FlyingThings3D_subset_processed_35m', 'val', '%07d' % i)
        os.makedirs(d)
        p1, p2, _ = synthetic_pair(n[i] if isinstance(n, list) else n, 60 + i)
        flip = np.array([-1, 1, -1], np.float32)
        np.save(os.path.join(d, 'pc1.npy'), p1 * flip)
        np.save(os.path.join(d, 'pc2.npy'), p2 * flip)


def test_engine_dense_on_frames_the_sample_covers(tmp_path):
    """Frames smaller than --points: the sample is every valid point, so the dense metrics are the sampled ones."""
    from hplflownet_amd import engine
    root = str(tmp_path)
    ft3d_tree(root, 3, [400, 450, 380])
    base = ['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'FlyingThings3DSubset', '--data-root', root]
    plain = engine.main(base)
    res = engine.main(base + ['--dense'])
    assert list(plain) == ['EPE3D', 'Acc3DS', 'Acc3DR', 'Outliers', 'EPE2D', 'Acc2D']
    assert list(res) == list(plain) + ['dense_' + k for k in plain] + ['dense_coverage', 'dense_full']
    for k in plain:
        assert res[k] == plain[k]                                   # the sampled metrics are unchanged
        assert abs(res['dense_' + k] - res[k]) <= 2e-4 * max(1.0, abs(res[k])), k
    assert res['dense_coverage'] == 1.0 and res['dense_full'] == 1.0


def test_engine_dense_on_larger_frames(tmp_path):
    from hplflownet_amd import engine
    root = str(tmp_path)
    ft3d_tree(root, 3, 3000)
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'FlyingThings3DSubset',
                       '--data-root', root, '--dense', '--batch-size', '2'])
    for k in DENSE_KEYS + ['dense_EPE2D', 'dense_Acc2D', 'dense_coverage', 'dense_full']:
        assert k in res and np.isfinite(res[k]), k
    assert 0 < res['dense_coverage'] <= 1 and 0 < res['dense_full'] <= res['dense_coverage']


def test_engine_dense_kitti_ragged(tmp_path):
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
    res = engine.main(['--arch', 'HPLFlowNetShallow', '--points', '512', '--evaluate', '--dataset', 'KITTI', '--data-root', root,
                       '--kitti-calib', os.path.join(GOLD, 'kitti_calib'), '--dense', '--batch-size', '2', '--ragged'])
    for k in DENSE_KEYS + ['dense_EPE2D', 'dense_Acc2D', 'EPE2D', 'Acc2D']:
        assert k in res and np.isfinite(res[k]), k
    assert 0 < res['dense_coverage'] <= 1
