"""CPU: the inputs of the lattice fuzz (tests/lattice_fuzz.py) stay inside what the reference defines and inside what each
test of tests/test_gpu_lattice_fuzz.py assumes of them, so that no GPU test has to skip a case.  Every figure is a condition
on the INPUTS, taken from the C oracle's own keys; none is a tolerance on the code under test.

Measured over SIZES x seeds 0..3, log2 of the number of packed keys of a pair at level 0 (the widest level of the kinds that spread; inside one simplex
the deeper levels have up to 2^12.8 keys):
  cloud 19.9 .. 31.9   dup 8.0 .. 31.7   line 18.6 .. 29.6   plane 16.9 .. 31.0   far 40.0 .. 53.1   tiny 8.0 .. 11.0
  axis 9.8 .. 24.0     same 8.0           lopsided 19.9 .. 31.8
  far32 56.40 .. 56.40 far64 59.90 .. 59.90   outlier 60.20 .. 60.22
The int64 packing of the reference wraps past 2^63; everything here stays below 2^62.  Vertices per cloud: tiny <= 14 at
every level, same <= 14; the sparse kinds (far, far32, far64) GROW from level to level, up to 16.8 vertices per point at
n = 300 and 27 for a cloud of one point."""
import types

import pytest

import lattice_fuzz as F

SEEDS = range(4)


@pytest.fixture(scope='module')
def surveys():
    cache = {}

    def get(kind, n1, n2, seed):
        key = (kind, n1, n2, seed)
        if key not in cache:
            cache[key] = F.survey(*F.fuzz_pair(kind, n1, n2, seed))
        return cache[key]
    return get


def test_bits_per_pair_of_a_batch():
    """the table of DESIGN.md: what the pair digit leaves a pair"""
    want = {2: 62, 3: 61, 4: 61, 5: 60, 8: 60, 9: 59, 16: 59, 17: 58, 32: 58, 33: 57, 64: 57}
    assert {B: F.pair_bits(B) for B in want} == want


@pytest.mark.parametrize('kind', F.KINDS)
def test_fuzz_inputs_stay_inside_their_bands(kind, surveys):
    for n1, n2 in F.SIZES:
        for seed in SEEDS:
            p1, p2 = F.fuzz_pair(kind, n1, n2, seed)
            q1, q2 = F.fuzz_pair(kind, n1, n2, seed)
            assert p1.shape == (n1, 3) and p2.shape == (1 if kind == 'lopsided' else n2, 3)
            assert p1.dtype == p2.dtype == 'float32' and (p1 == q1).all() and (p2 == q2).all()
            s = surveys(kind, n1, n2, seed)
            what = (kind, n1, n2, seed, s['bits'])
            assert max(s['bits']) < 62, what                    # the reference's own packing is defined
            if kind in ('cloud', 'far', 'far32', 'far64', 'outlier'):
                assert s['bits'][0] == max(s['bits']), what     # level 0 is the widest (not so inside one simplex)
            if kind == 'far32':                                  # fits a batch of 64 (57 bits), by half a bit and no more than one
                assert 56.0 <= s['bits'][0] < 56.5, what
            if kind in ('far64', 'outlier'):                     # refused at B = 16 (59 bits), accepted at B = 4 (61 bits)
                assert 59.5 <= s['bits'][0] < 60.5, what
            if kind in ('axis', 'same'):
                assert s['ties'], what
            if kind == 'tiny':
                assert max(max(v) for v in s['verts']) <= 16, what
            # a first fused build takes it without a rebuild
            assert max(max(v) for v in s['verts']) <= F.default_bound(n1, p2.shape[0]), what


def test_the_tight_bounds_sequence_outgrows_its_bounds_twice():
    """test_tight_bounds_after_a_degenerate_pair: under the bounds that follow the counts seen (NativeBuilder.observe), the
    second and the third pair of tiny, cloud, far32, same outgrow them, at levels of their own"""
    from hplflownet_amd.lattice import NativeBuilder
    n1, n2, seed = F.TIGHT_CASE
    st = types.SimpleNamespace(seen=[0] * 8, bounds=[0] * 8)
    over = []
    for kind in F.TIGHT_KINDS:
        verts = F.survey(*F.fuzz_pair(kind, n1, n2, seed))['verts']
        over.append(F.overflowing_levels(st.bounds, verts, n1, n2))
        NativeBuilder.observe(st, verts)
    assert over[0] == [] and over[3] == [] and over[1] and over[2], over
    assert set(over[1]) != set(over[2]), over
