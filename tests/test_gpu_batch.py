"""GPU: batched inference -- B pairs in one fused lattice build (hpl_lattice_begin_batch) and one forward
(hpl_plan_run_batch).  Pair b's slice of every table of a batch is its single-pair build's plus the vertex / point offsets,
no table links two pairs, B = 1 is the single-pair path bit for bit, and every pair's flow meets the parity bar of
test_gpu_bench_size.py against its own single-pair forward (default math mode and HPL_MATH=f32)."""
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


def make_model(nsc):
    import hplflownet_amd as H
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP[:nsc], evaluate=True, use_leaky=True,
                                 bcn_use_bias=True, bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = (H.HPLFlowNet if nsc == 7 else H.HPLFlowNetShallow)(args)
    fill_module_(m, 1.0, 'hash')
    return m.to(DEV).eval(), args


def make_gen(nsc, monkeypatch):
    import hplflownet_amd as H
    monkeypatch.setenv('HPL_LATTICE_FUSED', '1')
    m, args = make_model(nsc)
    gen = H.GenerateDataUnsymmetric(args, device=DEV, wide_up=m.lattice_hint())
    assert gen.native_builder().fused
    return gen, m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV)


def clouds(kind, B, n1, n2, seed, mul=None):
    p1, p2 = [], []
    for b in range(B):
        a, c, _ = (synthetic_pair if kind == 'frustum' else surface_pair)(max(n1, n2), seed + 7 * b)
        f = mul[b] if mul is not None else 1.0
        p1.append(dev(a[:n1] * f))
        p2.append(dev(c[:n2] * f))
    return torch.stack(p1), torch.stack(p2)


def check_pair_slices(lat, singles):
    """every table of pair b of the batched lattice `lat` == singles[b] after the offsets; no index leaves pair b's ranges"""
    B = len(singles)
    assert lat.batch == B and lat.pair_counts.shape == (lat.n_levels, 2, B)
    for L in range(lat.n_levels):
        lv = lat.levels[L]
        H0, H1 = lv.H
        pc = lat.pair_counts[L]
        assert pc[0].sum() == H0 and pc[1].sum() == H1
        voff = [np.concatenate([[0], np.cumsum(pc[c])]) for c in (0, 1)]
        if L == 0:
            npair = [np.full(B, singles[0].tables[0].n0), np.full(B, singles[0].tables[0].n1)]
        else:
            npair = [lat.pair_counts[L - 1][c] for c in (0, 1)]
        noff = [np.concatenate([[0], np.cumsum(npair[c])]) for c in (0, 1)]
        n0 = int(noff[0][-1])
        blur = lv.blur.pair.t.cpu().numpy()
        emg = lv.emg_pair.cpu().numpy()
        ptr, pt, w, norm = [x.cpu() for x in lv.pair._csr]
        ptr, pt = ptr.numpy(), pt.numpy()
        corr2 = lv.corr2.t.cpu().numpy().reshape(225, H0) if lv.corr2 is not None else None
        for b, s in enumerate(singles):
            what = 'level %d pair %d' % (L, b)
            sv = s.levels[L]
            h0, h1 = sv.H
            assert (pc[0][b], pc[1][b]) == (h0, h1), what
            v0, v1 = int(voff[0][b]), int(voff[1][b])
            p0, p1 = int(noff[0][b]), int(noff[1][b])
            m0, m1 = int(npair[0][b]), int(npair[1][b])
            for c, (vo, po, m) in enumerate(((v0, p0, m0), (v1, p1, m1))):
                cl, scl = lv.clouds[c], sv.clouds[c]
                assert torch.equal(cl.bary[:, po:po + m], scl.bary), what
                assert torch.equal(cl.off[:, po:po + m] - vo, scl.off), what
            assert np.array_equal(emg[p0:p0 + m0], sv.emg_pair[:m0].cpu().numpy()), what
            assert np.array_equal(emg[n0 + p1:n0 + p1 + m1], sv.emg_pair[m0:].cpu().numpy()), what
            # blur: cloud-1 columns take cloud-1 ids, cloud-2 columns cloud-2 ids shifted by H0 (the pair's, or the batch's)
            sb = s.levels[L].blur.pair.t.cpu().numpy()
            for cols, scols, lo, hi, shift, sshift in (((v0, v0 + h0), (0, h0), 0, H0, v0, 0),
                                                       ((H0 + v1, H0 + v1 + h1), (h0, h0 + h1), H0, H0 + H1, H0 + v1, h0)):
                x = blur[:, cols[0]:cols[1]]
                ok = x[x >= 0]
                assert ((ok >= shift) & (ok < shift + (cols[1] - cols[0]))).all(), 'blur edge between pairs, ' + what
                assert np.array_equal(np.where(x >= 0, x - shift + sshift, -1), sb[:, scols[0]:scols[1]]), what
            if corr2 is not None:
                x = corr2[:, v0:v0 + h0]
                ok = x[x >= 0]
                assert ((ok >= v1) & (ok < v1 + h1)).all(), 'corr2 edge between pairs, ' + what
                sc = sv.corr2.t.cpu().numpy().reshape(225, h0)
                assert np.array_equal(np.where(x >= 0, x - v1, -1), sc), what
            # splat CSR: rows = cloud-1 vertices, then cloud-2 vertices; points = cloud-1 rows, then cloud-2 rows
            sptr, spt, sw, snorm = [x.cpu() for x in sv.pair._csr]
            sptr, spt = sptr.numpy(), spt.numpy()
            for rows, srows, pbase, spbase, m in (((v0, v0 + h0), (0, h0), p0, 0, m0),
                                                  ((H0 + v1, H0 + v1 + h1), (h0, h0 + h1), n0 + p1, m0, m1)):
                a0, a1 = int(ptr[rows[0]]), int(ptr[rows[1]])
                b0, b1 = int(sptr[srows[0]]), int(sptr[srows[1]])
                assert np.array_equal(ptr[rows[0]:rows[1] + 1] - a0, sptr[srows[0]:srows[1] + 1] - b0), what
                seg = pt[a0:a1]
                assert ((seg >= pbase) & (seg < pbase + m)).all(), 'CSR edge between pairs, ' + what
                assert np.array_equal(seg - pbase + spbase, spt[b0:b1]), what
                assert torch.equal(w[a0:a1], sw[b0:b1]), what
                assert torch.equal(norm[rows[0]:rows[1]], snorm[srows[0]:srows[1]]), what


@pytest.mark.parametrize('kind,nsc', [('frustum', 7), ('surface', 5)])
def test_batched_lattice_is_the_per_pair_lattices(kind, nsc, monkeypatch):
    gen, _ = make_gen(nsc, monkeypatch)
    p1, p2 = clouds(kind, 3, 1024, 777, 3)
    lat = gen.build_native_batch(p1, p2)
    singles = [gen.build_native(p1[b], p2[b]) for b in range(3)]
    torch.cuda.synchronize()
    check_pair_slices(lat, singles)


def test_batch_of_one_is_the_single_pair_path(monkeypatch):
    import hplflownet_amd as H
    gen, m = make_gen(7, monkeypatch)
    p1, p2 = clouds('frustum', 1, 1024, 1024, 5)
    a = gen.build_native_batch(p1, p2)
    b = gen.build_native(p1[0], p2[0])
    assert a.batch == 1 and a.H == b.H
    for x, y in zip(H.to_reference_format(a), H.to_reference_format(b)):
        for k in y:
            assert (torch.equal(x[k], y[k]) if torch.is_tensor(y[k]) else x[k] == y[k]), k
    with torch.no_grad():
        assert torch.equal(m(p1, p2, a), m(p1[0][None], p2[0][None], b))


def _flows_match(batched, singles, what):
    for b, s in enumerate(singles):
        ref = s[0]
        bar = 2e-4 * max(1.0, float(ref.abs().max()))
        err = float((batched[b] - ref).abs().max())
        assert err < bar, '%s pair %d: max|d| %.3g >= %.3g' % (what, b, err, bar)


@pytest.mark.parametrize('B,n', [(2, 1024), (4, 1024), (8, 1024), (2, 8192)])
def test_batched_forward_matches_per_pair_forwards(B, n, monkeypatch):
    gen, m = make_gen(7, monkeypatch)
    p1, p2 = clouds('frustum', B, n, n, 11 + B)
    lat = gen.build_native_batch(p1, p2)
    with torch.no_grad():
        flow = m(p1, p2, lat)
        assert flow.shape == (B, 3, n)
        singles = [m(p1[b][None], p2[b][None], gen.build_native(p1[b], p2[b])) for b in range(B)]
        _flows_match(flow, singles, 'native plan')
        m.native_forward = False                   # the Python no-grad pair path on the same batch
        try:
            flow_py = m(p1, p2, lat)
        finally:
            del m.native_forward
    torch.cuda.synchronize()
    assert flow_py.shape == (B, 3, n)
    bar = 2e-4 * max(1.0, float(flow.abs().max()))
    assert float((flow_py - flow).abs().max()) < bar


@pytest.mark.skipif(os.environ.get('HPL_MATH') == 'f32', reason='this test starts the f32 run itself')
def test_batched_forward_matches_under_f32():
    env = dict(os.environ, HPL_MATH='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_batch.py'), '-k', 'batched_forward_matches_per_pair or loud'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '5 passed' in r.stdout, r.stdout[-2000:]


def test_one_loud_pair_does_not_spoil_the_quiet_ones(monkeypatch):
    gen, m = make_gen(7, monkeypatch)
    B = 4
    p1, p2 = clouds('frustum', B, 1024, 1024, 31, mul=[1.0, 100.0, 1.0, 1.0])
    lat = gen.build_native_batch(p1, p2)
    plan = m.forward_plan()
    trips0 = plan.guard_trips()
    with torch.no_grad():
        flow = m(p1, p2, lat)
        singles = [m(p1[b][None], p2[b][None], gen.build_native(p1[b], p2[b])) for b in range(B)]
    torch.cuda.synchronize()
    _flows_match(flow, singles, 'loud batch')
    print('guard trips of the loud batch and its single pairs: %d' % (plan.guard_trips() - trips0))


def test_overflowing_bounds_rebuild_the_batch(monkeypatch):
    gen, _ = make_gen(7, monkeypatch)
    nb = gen.native_builder()
    p1, p2 = clouds('frustum', 3, 1024, 777, 41)
    singles = [gen.build_native(p1[b], p2[b]) for b in range(3)]
    for bad_level in (0, 2, 6):
        nb.bounds = [0] * 8
        nb.seen = [0] * 8
        nb.bounds[bad_level] = 16                      # far below the real vertex count of that level
        before = nb.fallbacks
        lat = gen.build_native_batch(p1, p2)
        torch.cuda.synchronize()
        assert nb.fallbacks == before + 1
        check_pair_slices(lat, singles)
        lat = gen.build_native_batch(p1, p2)           # the bounds observed from the batch fit
        torch.cuda.synchronize()
        assert nb.fallbacks == before + 1
        check_pair_slices(lat, singles)


def test_batch_errors_launch_nothing(monkeypatch):
    import hplflownet_amd as H
    from hplflownet_amd._lib import HplError
    from hplflownet_amd.engine import Trainer
    gen, m = make_gen(5, monkeypatch)
    p1, p2 = clouds('frustum', 2, 512, 512, 51)
    lat = gen.build_native_batch(p1, p2)
    single = gen.build_native(p1[0], p2[0])
    torch.cuda.synchronize()
    bad = [lambda: gen.build_native_batch(p1, p2[:1]),
           lambda: gen.build_native_batch(p1[:0], p2[:0]),
           lambda: gen.build_native_batch(p1[:1].expand(65, 3, 512).contiguous(), p2[:1].expand(65, 3, 512).contiguous()),
           lambda: m(p1, p2, single),
           lambda: m(p1[:1], p2[:1], lat),
           lambda: H.to_reference_format(lat)]
    for f in bad:
        with torch.no_grad():
            with pytest.raises(HplError):
                f()
    tr = Trainer('HPLFlowNetShallow', torch.device(DEV), init='hash')
    with pytest.raises(HplError):
        tr.train_step(p1[0], p2[0], p2[0] - p1[0], lat)
    with pytest.raises(HplError):
        m.train()
        m(p1, p2, lat)                                  # autograd forward of a batch


def test_engine_batched_evaluation_matches_one_pair_at_a_time():
    from hplflownet_amd.engine import Trainer

    class Frames(object):          # a reader with one short frame (allow_less_points) in the middle
        def __init__(self):
            self.n = [2048, 2048, 2048, 1500, 2048, 2048, 2048, 2048, 2048]

        def __len__(self):
            return len(self.n)

        def __getitem__(self, i):
            a, c, f = synthetic_pair(self.n[i], 200 + i)
            return dev(a), dev(c), dev(f)
    tr = Trainer('HPLFlowNetShallow', torch.device(DEV), init='hash')
    one = tr.validate(Frames(), 1)
    four = tr.validate(Frames(), 4)
    assert set(one) == set(four)
    assert abs(one['EPE3D'] - four['EPE3D']) < 1e-4, (one, four)
    for k in one:
        assert abs(one[k] - four[k]) < 1e-3, (k, one, four)
