"""GPU: the lattice builds production uses -- the fused single-pair build, the equal-count batch, the ragged batch
(csrc/lattice_fused.hip) and the native staged fallback (csrc/lattice_builder.hip) -- against the C oracle on the hard
clouds of tests/lattice_fuzz.py: exact rank ties, clouds inside one simplex, sparse clouds whose vertex counts grow from
level to level, key ranges of 2^56 .. 2^60; the rebuild after an overflow; the refusal of a batch whose pair does not
fit below the pair digit; and whole forwards over lattices of a handful of vertices.  All 7 scales, <= 300 points a cloud.
What the inputs are assumed to be (bands of the key ranges, ties, vertex counts) is asserted on the CPU by
tests/test_lattice_fuzz_cpu.py; every expectation about a batch is decided from the oracle's own key range."""
import types

import numpy as np
import pytest
import torch

import lattice_fuzz as F
from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_
from test_gpu_batch import check_pair_slices
from test_gpu_lattice_fused import assert_same_lattice, dev, make_gen
from test_gpu_ragged import check_ragged_slices

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def gens():
    """(fused, staged) GenerateDataUnsymmetric over all 7 scales, with the model's row-order hint"""
    mp = pytest.MonkeyPatch()
    try:
        yield make_gen(7, True, mp), make_gen(7, False, mp)
    finally:
        mp.undo()


def first_build(nb):
    """the builder as it is before it has seen a pair: the default bounds"""
    nb.bounds = [0] * 8
    nb.seen = [0] * 8


def counts(gd):
    return [(d['pc1_hash_cnt'], d['pc2_hash_cnt']) for d in gd]


def single(gen, case):
    """case = (kind, n1, n2, seed) -> (device clouds, fused single-pair lattice == the oracle, oracle tables)"""
    nb = gen.native_builder()
    pc1, pc2, gd = F.oracle_pair(*case)
    t1, t2 = dev(pc1), dev(pc2)
    first_build(nb)
    before = nb.fallbacks
    lat = gen.build_native(t1, t2)
    torch.cuda.synchronize()
    assert nb.fallbacks == before, case
    F.assert_equals_oracle(lat, pc1, pc2, case, gd=gd)
    return (t1, t2), lat, gd


def fitting(cases, B):
    """the cases whose key range fits below the pair digit of a batch of B; none may sit on the threshold"""
    bits, out = F.pair_bits(B), []
    for case in cases:
        rb = max(F.range_bits(*F.oracle_pair(*case)[:2]))
        assert abs(rb - bits) > 0.05, (case, rb, bits)
        if rb < bits:
            out.append(case)
    return out


def assert_pair_counts(lat, gds):
    for b, gd in enumerate(gds):
        assert [tuple(lat.pair_counts[L, :, b]) for L in range(lat.n_levels)] == counts(gd), b


@pytest.mark.parametrize('kind', F.KINDS)
def test_single_pair_builds_equal_the_oracle(kind, gens):
    gen_f, gen_s = gens
    nb = gen_f.native_builder()
    for n1, n2 in F.SIZES:
        for seed in (0, 1):
            what = (kind, n1, n2, seed)
            pc1, pc2, gd = F.oracle_pair(*what)
            t1, t2 = dev(pc1), dev(pc2)
            first_build(nb)
            before = nb.fallbacks
            a = gen_f.build_native(t1, t2)
            b = gen_s.build_native(t1, t2)
            torch.cuda.synchronize()
            assert nb.fallbacks == before, what                  # the fused build itself, not its staged rebuild
            F.assert_equals_oracle(a, pc1, pc2, ('fused',) + what, gd=gd)
            F.assert_equals_oracle(b, pc1, pc2, ('staged',) + what, gd=gd)
            assert_same_lattice(a, b, what)


def test_tight_bounds_after_a_degenerate_pair(gens):
    """one fused builder sees tiny, cloud, far32, same: the bounds follow the counts seen, so the second and the third pair
    outgrow them (the staged rebuild in the fused build's arena); the fourth is far below them"""
    gen = gens[0]
    nb = gen.native_builder()
    first_build(nb)
    n1, n2, seed = F.TIGHT_CASE
    rose = []
    for kind in F.TIGHT_KINDS:
        pc1, pc2, gd = F.oracle_pair(kind, n1, n2, seed)
        bounds, before = list(nb.bounds), nb.fallbacks
        lat = gen.build_native(dev(pc1), dev(pc2))
        torch.cuda.synchronize()
        F.assert_equals_oracle(lat, pc1, pc2, kind, gd=gd)
        over = F.overflowing_levels(bounds, counts(gd), n1, n2)
        assert nb.fallbacks == before + (1 if over else 0), (kind, over, bounds, counts(gd))
        rose.append(bool(over))
    assert rose == [False, True, True, False]


@pytest.mark.parametrize('B,n', [(5, 96), (64, 24)])
def test_batches_of_mixed_kinds_equal_the_oracle(B, n, gens):
    """equal-count batches holding one pair of every kind that fits B's bits ('lopsided' has a count of its own: it is in
    the ragged batches), filled up with plain clouds"""
    gen = gens[0]
    nb = gen.native_builder()
    kinds = fitting([(k, n, n, 10 + i) for i, k in enumerate(F.KINDS) if k != 'lopsided'], B)
    assert {'far', 'far32', 'axis', 'same', 'tiny'} <= {c[0] for c in kinds}
    assert ('far64' in {c[0] for c in kinds}) == (B == 5)          # 2^59.9 keys: under the 60 bits of B = 5, over the 57 of B = 64
    fill = iter([('cloud', n, n, 100 + i) for i in range(B)])
    batches = [kinds[i:i + B] for i in range(0, len(kinds), B)]
    for cases in batches:
        cases = cases + [next(fill) for _ in range(B - len(cases))]
        built = [single(gen, c) for c in cases]
        p1 = torch.stack([t[0][0] for t in built])
        p2 = torch.stack([t[0][1] for t in built])
        first_build(nb)
        for which in ('default bounds', 'observed bounds')[:2 if B == 5 else 1]:
            before = nb.fallbacks
            lat = gen.build_native_batch(p1, p2)
            torch.cuda.synchronize()
            assert nb.fallbacks == before, (which, cases)
            check_pair_slices(lat, [t[1] for t in built])
            assert_pair_counts(lat, [t[2] for t in built])


def test_ragged_batches_of_mixed_kinds_equal_the_oracle(gens):
    gen = gens[0]
    nb = gen.native_builder()
    rng = np.random.RandomState(5)
    cases = [('cloud', 1, 1, 40), ('lopsided', 300, 1, 41), ('cloud', 1, 300, 42)]
    cases += [(k, int(rng.randint(1, 301)), int(rng.randint(1, 301)), 50 + i) for i, k in enumerate(F.KINDS)]
    assert F.pair_bits(9) == F.pair_bits(len(cases)) == 59
    cases = fitting(cases, len(cases))
    assert 9 <= len(cases) <= 16 and {'far32', 'far', 'lopsided', 'same', 'axis', 'tiny'} <= {c[0] for c in cases}
    built = {c: single(gen, c) for c in cases}
    for order in (cases, cases[::-1]):
        p1 = [built[c][0][0] for c in order]
        p2 = [built[c][0][1] for c in order]
        cnt = [(int(a.shape[1]), int(b.shape[1])) for a, b in zip(p1, p2)]
        assert {(1, 1), (300, 1), (1, 300)} <= set(cnt)
        first_build(nb)
        before = nb.fallbacks
        lat = gen.build_native_batch(p1, p2)
        torch.cuda.synchronize()
        assert nb.fallbacks == before
        check_ragged_slices(lat, [built[c][1] for c in order], cnt)
        assert_pair_counts(lat, [built[c][2] for c in order])


def test_key_range_refusal(gens):
    """a pair of 2^59.9 (far64) or 2^60.2 (outlier) keys builds alone and in a batch of 4 (61 bits a pair); a batch of 16
    (59 bits) that holds it is refused, wherever the pair stands and in both forms of a batch, and the builder goes on"""
    from hplflownet_amd._lib import HplError
    gen = gens[0]
    nb = gen.native_builder()
    n = 128

    def fits(rb, B):
        assert abs(rb - F.pair_bits(B)) >= 0.5, (rb, B)            # half a bit from the threshold it straddles
        return rb < F.pair_bits(B)

    def bits(case):
        return max(F.range_bits(*F.oracle_pair(*case)[:2]))

    def stack(built):
        return torch.stack([t[0][0] for t in built]), torch.stack([t[0][1] for t in built])

    def lists(built):
        return [t[0][0] for t in built], [t[0][1] for t in built]

    clouds = [single(gen, ('cloud', n, n, 200 + i)) for i in range(15)]
    ragged = [single(gen, ('cloud', 100 + i, 90 + 2 * i, 300 + i)) for i in range(15)]
    after = [single(gen, ('far32' if i % 2 else 'cloud', n, n, 400 + i)) for i in range(16)]
    assert all(fits(bits(('far32', n, n, 400 + i)), 16) for i in range(1, 16, 2))
    for kind in ('far64', 'outlier'):
        wide = single(gen, (kind, n, n, 3))                         # alone: equals the oracle
        rb = bits((kind, n, n, 3))
        assert fits(rb, 4) and not fits(rb, 16)
        four = clouds[:2] + [wide] + clouds[2:3]
        first_build(nb)
        lat = gen.build_native_batch(*stack(four))
        torch.cuda.synchronize()
        check_pair_slices(lat, [t[1] for t in four])
        assert_pair_counts(lat, [t[2] for t in four])
        for form, others in ((stack, clouds), (lists, ragged)):
            for sixteen in ([wide] + others, others + [wide]):
                first_build(nb)
                with pytest.raises(HplError, match='key range'):
                    gen.build_native_batch(*form(sixteen))
                lat = gen.build_native_batch(*stack(after))         # the next call on the same builder
                torch.cuda.synchronize()
                assert_pair_counts(lat, [t[2] for t in after])
        check_pair_slices(lat, [t[1] for t in after])
    # 2^56.4 keys a pair under the 57 bits of a batch of 64
    many = [single(gen, ('far32', 24, 24, 500 + i)) for i in range(64)]
    assert all(fits(bits(('far32', 24, 24, 500 + i)), 64) for i in range(64))
    first_build(nb)
    before = nb.fallbacks
    lat = gen.build_native_batch(*stack(many))
    torch.cuda.synchronize()
    assert nb.fallbacks == before
    check_pair_slices(lat, [t[1] for t in many])
    assert_pair_counts(lat, [t[2] for t in many])


FORWARD_KINDS = ('tiny', 'same', 'axis', 'line', 'lopsided', 'far32')


@pytest.fixture(scope='module')
def flownet():
    import hplflownet_amd as H
    args = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True, bcn_use_bias=True,
                                 bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    m = H.HPLFlowNet(args)
    fill_module_(m, 1.0, 'hash')
    sd = {k: v.numpy().copy() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


@pytest.mark.parametrize('kind', FORWARD_KINDS)
def test_forward_over_degenerate_lattices(kind, gens, flownet):
    """HPLFlowNet over the fused lattice of a degenerate pair (n = 256; levels of 4 .. 16 vertices for tiny and same, a
    cloud of one point for lopsided) against oracle.bcl_oracle.hplflownet_forward over the oracle's tables, at the bar of
    test_config2_shallow_n4096_vs_oracle; finite; the native plan bit-equal to the launch-by-launch path.
    Measured max|got - ref| / max(1, max|ref|), bar 2e-4:
      tiny 2.3e-6   same 4.5e-6   axis 2.0e-6 (max|ref| 4.1)   line 2.8e-6 (21)   lopsided 9.0e-7 (26)   far32 1.6e-6 (1240)"""
    from oracle import bcl_oracle as BO
    gen = gens[0]
    m, sd = flownet
    (t1, t2), lat, gd = single(gen, (kind, 256, 256, 7))
    pc1, pc2, _ = F.oracle_pair(kind, 256, 256, 7)
    if kind in ('tiny', 'same'):
        assert max(max(c) for c in counts(gd)) <= 16, counts(gd)
    with torch.no_grad():
        y = m(t1[None], t2[None], lat).clone()
        m.native_forward = False
        try:
            y_py = m(t1[None], t2[None], lat).clone()
        finally:
            del m.native_forward
    torch.cuda.synchronize()
    assert tuple(y.shape) == (1, 3, 256) and torch.isfinite(y).all()
    assert torch.equal(y, y_py)
    ref = BO.hplflownet_forward(sd, pc1.T, pc2.T, gd)
    got = y[0].cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print('forward over %s: max|got - ref| = %.3g, max|ref| = %.3g, relative to the bar\'s scale %.3g'
          % (kind, err, float(np.abs(ref).max()), err / scale))
    assert err < 2e-4 * scale
