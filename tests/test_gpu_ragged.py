"""GPU: ragged batched inference -- B pairs with their own point counts in one fused lattice build (hpl_ragged_stage +
hpl_lattice_begin_ragged) and one forward.  Pair b's slice of every table is its single-pair build's plus the vertex / point
offsets and no table links two pairs; equal counts give the equal-count batch's tables and flow bits; the staging launch is
torch.cat; every pair's flow meets the parity bar of test_gpu_batch.py against its own single-pair forward (default math
mode and HPL_MATH=f32, native plan and Python pair path); the engine evaluates a KITTI tree of short frames in ragged
batches with the metrics of one pair at a time."""
import ctypes
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
COUNTS = [(1024, 1024), (700, 913), (1536, 1536), (37, 37), (333, 250)]


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


def ragged_clouds(kind, counts, seed):
    p1, p2 = [], []
    for b, (n1, n2) in enumerate(counts):
        a, c, _ = (synthetic_pair if kind == 'frustum' else surface_pair)(max(n1, n2), seed + 7 * b)
        p1.append(dev(a[:n1]))
        p2.append(dev(c[:n2]))
    return p1, p2


def check_ragged_slices(lat, singles, counts):
    """every table of pair b of the ragged lattice `lat` == singles[b] after the offsets; no index leaves pair b's ranges"""
    B = len(singles)
    assert lat.batch == B and lat.ragged and lat.point_counts == [tuple(c) for c in counts]
    assert lat.pair_counts.shape == (lat.n_levels, 2, B)
    for L in range(lat.n_levels):
        lv = lat.levels[L]
        H0, H1 = lv.H
        pc = lat.pair_counts[L]
        assert pc[0].sum() == H0 and pc[1].sum() == H1
        voff = [np.concatenate([[0], np.cumsum(pc[c])]) for c in (0, 1)]
        if L == 0:
            npair = [np.array([c[0] for c in counts]), np.array([c[1] for c in counts])]
        else:
            npair = [lat.pair_counts[L - 1][c] for c in (0, 1)]
        noff = [np.concatenate([[0], np.cumsum(npair[c])]) for c in (0, 1)]
        n0 = int(noff[0][-1])
        assert (lv.clouds[0].N, lv.clouds[1].N) == (n0, int(noff[1][-1]))
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
            sb = sv.blur.pair.t.cpu().numpy()
            for cols, scols, shift, sshift in (((v0, v0 + h0), (0, h0), v0, 0), ((H0 + v1, H0 + v1 + h1), (h0, h0 + h1), H0 + v1, h0)):
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


def _tables_equal(a, b):
    """every table of two lattices over the same points, bit for bit"""
    for L in range(a.n_levels):
        x, y = a.levels[L], b.levels[L]
        assert x.H == y.H, L
        assert torch.equal(x.emg_pair, y.emg_pair), L
        for c in (0, 1):
            assert torch.equal(x.clouds[c].bary, y.clouds[c].bary) and torch.equal(x.clouds[c].off, y.clouds[c].off), L
        assert torch.equal(x.blur.pair.t, y.blur.pair.t), L
        for u, v in zip(x.pair._csr, y.pair._csr):
            assert torch.equal(u, v), L
        if x.corr2 is not None:
            assert torch.equal(x.corr2.t, y.corr2.t), L
    assert np.array_equal(a.pair_counts, b.pair_counts)


@pytest.mark.parametrize('kind,nsc', [('frustum', 7), ('surface', 7), ('frustum', 5), ('surface', 5)])
def test_ragged_lattice_is_the_per_pair_lattices(kind, nsc, monkeypatch):
    gen, _ = make_gen(nsc, monkeypatch)
    p1, p2 = ragged_clouds(kind, COUNTS, 3)
    lat = gen.build_native_batch(p1, p2)
    singles = [gen.build_native(a, b) for a, b in zip(p1, p2)]
    torch.cuda.synchronize()
    check_ragged_slices(lat, singles, COUNTS)
    for L in range(lat.n_levels):
        assert [tuple(lat.pair_counts[L, :, b]) for b in range(len(COUNTS))] == [s.H[L] for s in singles]


def test_ragged_batch_of_equal_counts_is_the_equal_batch(monkeypatch):
    gen, m = make_gen(7, monkeypatch)
    B, n1, n2 = 4, 1024, 900
    p1, p2 = ragged_clouds('frustum', [(n1, n2)] * B, 17)
    lat_r = gen.build_native_batch(p1, p2)
    lat_e = gen.build_native_batch(torch.stack(p1), torch.stack(p2))
    torch.cuda.synchronize()
    assert lat_r.ragged and not lat_e.ragged
    _tables_equal(lat_r, lat_e)
    with torch.no_grad():
        fr = m(p1, p2, lat_r)
        fe = m(torch.stack(p1), torch.stack(p2), lat_e)
    torch.cuda.synchronize()
    assert len(fr) == B
    for b in range(B):
        assert fr[b].shape == (1, 3, n1)
        assert torch.equal(fr[b][0], fe[b]), b


def test_ragged_stage_is_torch_cat():
    from hplflownet_amd import ops
    g = torch.Generator(device='cpu').manual_seed(5)
    for counts, offset in (([(5, 7), (1, 3), (64, 33), (17, 17)], 0),     # odd counts: the scalar path
                           ([(8, 4), (16, 12), (4, 4)], 0),                  # multiples of 4, aligned: the float4 path
                           ([(8, 4), (16, 12), (4, 4)], 1)):                 # the same behind a storage offset of one float
        B = len(counts)
        nmax = max(max(c) for c in counts) + 5
        pad = [torch.randn(offset + B * 3 * nmax, generator=g).to(DEV)[offset:].view(B, 3, nmax) for _ in range(3)]
        pc1 = [pad[0][b, :, :n1] for b, (n1, _) in enumerate(counts)]        # strided slices of padded (B, 3, Nmax) tensors
        pc2 = [pad[1][b, :, :n2] for b, (_, n2) in enumerate(counts)]
        sf = [pad[2][b, :, :n1] for b, (n1, _) in enumerate(counts)]
        a, b_, s = ops.ragged_stage(pc1, pc2, sf)
        torch.cuda.synchronize()
        assert torch.equal(a, torch.cat(pc1, 1)) and torch.equal(b_, torch.cat(pc2, 1)) and torch.equal(s, torch.cat(sf, 1))
        a, b_ = ops.ragged_stage([p.contiguous() for p in pc1], pc2)
        torch.cuda.synchronize()
        assert torch.equal(a, torch.cat(pc1, 1)) and torch.equal(b_, torch.cat(pc2, 1))
    # the whole budget of 64 pairs, one side 16-byte aligned and the other not
    counts = [(4 + 4 * (b % 5), 3 + b) for b in range(64)]
    p1 = [torch.randn(3, n1, generator=g).to(DEV) for n1, _ in counts]
    p2 = [torch.randn(3, n2 + 1, generator=g).to(DEV)[:, 1:] for _, n2 in counts]
    a, b_ = ops.ragged_stage(p1, p2)
    torch.cuda.synchronize()
    assert torch.equal(a, torch.cat(p1, 1)) and torch.equal(b_, torch.cat(p2, 1))


def _flows_match(flows, singles, what):
    for b, (f, s) in enumerate(zip(flows, singles)):
        assert f.shape == s.shape, (what, b, f.shape, s.shape)
        bar = 2e-4 * max(1.0, float(s.abs().max()))
        err = float((f - s).abs().max())
        assert err < bar, '%s pair %d: max|d| %.3g >= %.3g' % (what, b, err, bar)


@pytest.mark.parametrize('B,nmax', [(2, 1024), (5, 1024), (8, 2048), (2, 8192), (5, 8192)])
def test_ragged_forward_matches_per_pair_forwards(B, nmax, monkeypatch):
    gen, m = make_gen(7, monkeypatch)
    rng = np.random.RandomState(B * 1000 + nmax)
    counts = [(int(rng.randint(nmax // 2, nmax + 1)), int(rng.randint(nmax // 2, nmax + 1))) for _ in range(B)]
    counts[0] = (nmax, nmax)
    p1, p2 = ragged_clouds('frustum', counts, 11 + B)
    lat = gen.build_native_batch(p1, p2)
    with torch.no_grad():
        flows = m(p1, p2, lat)
        assert isinstance(flows, list) and len(flows) == B
        assert len({f.untyped_storage().data_ptr() for f in flows}) == 1          # views of one output matrix
        singles = [m(a[None], b[None], gen.build_native(a, b)) for a, b in zip(p1, p2)]
        _flows_match(flows, singles, 'native plan')
        m.native_forward = False                   # the Python no-grad pair path on the same ragged batch
        try:
            flows_py = m(p1, p2, lat)
        finally:
            del m.native_forward
    torch.cuda.synchronize()
    _flows_match(flows_py, flows, 'Python pair path')


@pytest.mark.skipif(os.environ.get('HPL_MATH') == 'f32', reason='this test starts the f32 run itself')
def test_ragged_forward_matches_under_f32():
    env = dict(os.environ, HPL_MATH='f32')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider',
                        os.path.join(ROOT, 'tests', 'test_gpu_ragged.py'), '-k', 'ragged_forward_matches_per_pair'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '5 passed' in r.stdout, r.stdout[-2000:]


def test_overflowing_bounds_rebuild_the_ragged_batch(monkeypatch):
    gen, m = make_gen(7, monkeypatch)
    nb = gen.native_builder()
    p1, p2 = ragged_clouds('frustum', COUNTS, 41)
    singles = [gen.build_native(a, b) for a, b in zip(p1, p2)]
    for bad_level in (0, 2, 6):
        nb.bounds = [0] * 8
        nb.seen = [0] * 8
        nb.bounds[bad_level] = 16                      # far below the real vertex count of that level
        before = nb.fallbacks
        lat = gen.build_native_batch(p1, p2)
        torch.cuda.synchronize()
        assert nb.fallbacks == before + 1
        check_ragged_slices(lat, singles, COUNTS)
        lat = gen.build_native_batch(p1, p2)           # the bounds observed from the batch fit
        torch.cuda.synchronize()
        assert nb.fallbacks == before + 1
        check_ragged_slices(lat, singles, COUNTS)
    with torch.no_grad():
        _flows_match(m(p1, p2, lat), [m(a[None], b[None], s) for a, b, s in zip(p1, p2, singles)], 'after a rebuild')


def test_ragged_errors_launch_nothing(monkeypatch):
    import hplflownet_amd as H
    from hplflownet_amd import _lib
    from hplflownet_amd._lib import HplError
    from hplflownet_amd.engine import Trainer
    gen, m = make_gen(5, monkeypatch)
    p1, p2 = ragged_clouds('frustum', [(512, 400), (300, 300)], 51)
    lat = gen.build_native_batch(p1, p2)
    eq = gen.build_native_batch(torch.stack([p1[1], p1[1]]), torch.stack([p2[1], p2[1]]))
    torch.cuda.synchronize()
    bad = [lambda: gen.build_native_batch(p1, p2[:1]),
           lambda: gen.build_native_batch(p1, p2, for_training=True),
           lambda: m(p1[::-1], p2[::-1], lat),                       # other counts than the lattice's
           lambda: m(torch.stack([p1[1], p1[1]]), torch.stack([p2[1], p2[1]]), lat),
           lambda: m([p1[1], p1[1]], [p2[1], p2[1]], eq),            # lists with an equal-count batch
           lambda: H.to_reference_format(lat)]
    for f in bad:
        with torch.no_grad():
            with pytest.raises(HplError):
                f()
    tr = Trainer('HPLFlowNetShallow', torch.device(DEV), init='hash')
    with pytest.raises(HplError):
        tr.train_step(p1[0], p2[0], p1[0], lat)
    with pytest.raises(HplError):
        tr.train_step_batch(torch.stack([p1[1], p1[1]]), torch.stack([p2[1], p2[1]]), torch.stack([p1[1], p1[1]]), lat)
    with pytest.raises(HplError):
        m.train()
        m(p1, p2, lat)                                  # autograd forward of a ragged batch
    # the C entry points refuse before any launch
    L = _lib.load()
    h = gen.native_builder().acquire()
    arena = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for B, n0, n1 in ((0, [1], [1]), (65, [8] * 65, [8] * 65), (2, [8, 0], [8, 8]), (2, [100000, 100000], [8, 8])):
        a0, a1 = (ctypes.c_int64 * max(1, B))(*n0), (ctypes.c_int64 * max(1, B))(*n1)
        assert L.hpl_lattice_arena_bytes_ragged(h, B, a0, a1) == -1
        assert L.hpl_lattice_begin_ragged(h, p1[0].data_ptr(), p2[0].data_ptr(), B, a0, a1, arena.data_ptr(), arena.numel(),
                                          None) == -1                    # HPL_EINVAL
    gen.native_builder().release(h)


def test_ragged_pipeline_hands_out_lists(monkeypatch):
    from hplflownet_amd.engine import ragged_groups
    from hplflownet_amd.lattice import LatticePipeline
    gen, m = make_gen(5, monkeypatch)
    counts = [(600, 600), (333, 250), (1024, 700), (37, 37), (512, 512)]
    p1, p2 = ragged_clouds('surface', counts, 61)
    groups = ragged_groups(counts, 2)
    pipe = LatticePipeline(gen, lambda k: (p1[k], p2[k]), 0, len(counts), native=True, batch=2, groups=groups, ragged=True)
    seen = []
    with torch.no_grad():
        for g in groups:
            (i, (a, b)), lat, ev = pipe.get()
            torch.cuda.current_stream().wait_event(ev)
            assert i == g[0] and isinstance(a, list) and len(a) == len(g)
            flows = m(a, b, lat)
            for k, f in zip(g, flows):
                seen.append(k)
                _flows_match([f], [m(p1[k][None], p2[k][None], gen.build_native(p1[k], p2[k]))], 'pipeline')
    assert seen == list(range(len(counts)))


def test_engine_ragged_kitti_evaluation(tmp_path, monkeypatch):
    """A KITTI-layout tree whose frames are short of --points (allow_less_points keeps every point of each) through
    data.KITTI and engine --evaluate --ragged: per-pair metrics as at --batch-size 1, in fewer batches."""
    from hplflownet_amd import engine
    base = tmp_path / 'KITTI_processed_occ_final'
    sizes = [2600, 1800, 3100, 2200, 900, 2900, 2500, 1500, 2000]
    for i, n in enumerate(sizes):
        a, c, _ = synthetic_pair(n, 300 + i)
        d = base / ('%06d' % i)
        d.mkdir(parents=True)
        np.save(str(d / 'pc1.npy'), a)
        np.save(str(d / 'pc2.npy'), c)
    runs = {}
    orig = engine.Trainer.validate

    def spy(self, data, *a, **k):
        r = orig(self, data, *a, **k)
        runs.setdefault('batches', []).append(self.val_batches)
        runs.setdefault('counts', []).append([engine.point_counts(data, i) for i in range(len(data))])
        return r
    monkeypatch.setattr(engine.Trainer, 'validate', spy)
    common = ['--evaluate', '--dataset', 'KITTI', '--data-root', str(tmp_path), '--points', '8192', '--arch', 'HPLFlowNetShallow']
    one = engine.main(common + ['--batch-size', '1'])
    four = engine.main(common + ['--batch-size', '4', '--ragged'])
    counts = runs['counts'][0]
    assert runs['counts'][1] == counts and len(set(counts)) == len(sizes)       # every frame its own counts, all below --points
    assert all(n1 < 8192 and n2 < 8192 for n1, n2 in counts)
    assert runs['batches'] == [len(sizes), 3]
    assert set(one) == set(four)
    assert abs(one['EPE3D'] - four['EPE3D']) < 2e-4 * max(1.0, one['EPE3D']), (one, four)
    for k in one:
        assert abs(one[k] - four[k]) < 1e-3, (k, one, four)
