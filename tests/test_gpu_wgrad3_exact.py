"""GPU: the split-operand weight gradient (csrc/wgrad3.hip) bit for bit, in every launch form of the WGRAD3 table of
tests/gconv_forms.py (whose instances tests/test_gconv_forms_cpu.py pins) and in both operand families.

The operands are integers whose arithmetic is exact (gconv_forms.exact_wgrad_operands): a power-of-two scale is exact, an
integer below 2^22 is exactly an fp16 pair and a bf16 triple, the products the kernel drops are zero when one operand needs its
first plane alone, and fp32 sums of integers below 2^24 are exact in any order.  So a result has ONE right value, whatever the
slab order, the atomic order or the family, and every comparison here is torch.equal against float64 on the device
(index_select + matmul).  Each test first asserts the precondition itself, (|X|^T |dY|).max() < 2^24 in the common unit.

Both families run in the default process: with operand magnitudes (scales=True) the launch takes fp16 pairs, without
(scales=False) bf16 triples.  The expectation is chosen by HPL_MATH (gconv_forms.wgrad3_expect), so the file passes unchanged
under HPL_MATH=bf16x3 (always triples) and HPL_MATH=f32 (the fp32 kernel, where integer products are exact as well)."""
import os

import pytest
import torch

import gconv_forms as G

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MATH = os.environ.get('HPL_MATH', '')
CASES = {c['name']: c for c in G.WGRAD3}
FLOORS = ('w3x_dense_floor', 'w3x_tap_floor')


@pytest.fixture(scope='module')
def ops():
    from hplflownet_amd import ops as o
    return o


def _assert_equal(got, want, what):
    """got (float32) == want (float64), element for element."""
    g = got.double()
    if torch.equal(g, want):
        return
    bad = g != want
    i = int((g - want).abs().nan_to_num(float('inf')).reshape(-1).argmax())
    r, c = divmod(i, got.shape[-1]) if got.dim() == 2 else (0, i)
    raise AssertionError('%s: %d of %d elements differ; worst at (%d, %d): got %r want %r'
                         % (what, int(bad.sum()), bad.numel(), r, c, float(g.reshape(-1)[i]), float(want.reshape(-1)[i])))


def _check_info(ops, name, args, kw, scales):
    """The launch takes the instance the table names for this mode and selection; -> its family."""
    info = ops.wgrad_launch_info(*args, scales=scales, **kw)
    want = G.wgrad3_expect(name, MATH, scales is not False)
    if want is None:
        assert info['family'] == G.FP32 and info['bn'] == 128, info
    else:
        assert info == want
    return info['family']


def _reference(args):
    """-> float64 result, after the precondition that makes it the one right value."""
    want, S = G.wgrad_ref64(*args)
    assert float(S.max()) < G.EXACT_LIMIT
    return want


def _check_result(out, want, args, what, bias=True):
    A, nbr, M, C, F, dY, N = args
    dWt, gb = out
    K = F * C
    _assert_equal(dWt[:K, :N], want, what)
    assert not bool(dWt[K:].any()) and not bool(dWt[:, N:].any()), what + ': the image outside [F*C, N) is not zero'
    if bias:
        _assert_equal(gb, dY.double().sum(0), what + ' bias gradient')


@pytest.mark.parametrize('cls', G.CLASSES)
@pytest.mark.parametrize('name', list(CASES))
def test_exact(ops, name, cls):
    """Every case x class, with and without operand magnitudes: the pinned instance, the exact weight gradient, zeros outside
    [F*C, N), and the exact bias gradient (where its own sums stay below 2^24: not with a full-width dY)."""
    args, kw = G.exact_wgrad_operands(CASES[name], cls, DEV)
    want = _reference(args)
    families = set()
    for scales in (True, False):
        families.add(_check_info(ops, name, args, kw, scales))
        out = ops.wgrad_raw(*args, scales=scales, **kw)
        _check_result(out, want, args, '%s %s scales=%s' % (name, cls, scales), bias=cls != 'planes_dy')
    if MATH == '' and G.EXPECT_WGRAD3[name]['family'] != G.FP32:
        assert families == {G.PAIRS, G.TRIPLES}


@pytest.mark.parametrize('a,b', [(-80, -30), (60, -40), (15, 5), (-10, -10)])
@pytest.mark.parametrize('name', FLOORS)
def test_power_of_two_invariance(ops, name, a, b):
    """A * 2^a and dY * 2^b give the base result times 2^(a+b), bit for bit, in both families: the scale of each operand
    (split_scale), its inverse (split_unscale) and the order of acc * u_a * u_d in the epilogue lose nothing at magnitudes far
    from 1."""
    args, kw = G.exact_wgrad_operands(CASES[name], 'planes_a', DEV)
    A, nbr, M, C, F, dY, N = args
    want = _reference(args) * 2.0 ** (a + b)
    scaled = (A * 2.0 ** a, nbr, M, C, F, dY * 2.0 ** b, N)
    assert torch.equal(scaled[0].double(), A.double() * 2.0 ** a) and torch.equal(scaled[5].double(), dY.double() * 2.0 ** b)
    for scales in (True, False):
        _check_info(ops, name, scaled, kw, scales)
        base = ops.wgrad_raw(*args, scales=scales, **kw)
        out = ops.wgrad_raw(*scaled, scales=scales, **kw)
        assert torch.equal(out[0], base[0] * 2.0 ** (a + b))
        _check_result(out, want, scaled, '%s 2^%d 2^%d scales=%s' % (name, a, b, scales), bias=False)


@pytest.mark.parametrize('cls', ['planes_a', 'planes_dy'])
@pytest.mark.parametrize('name', FLOORS)
def test_callers_magnitudes_that_are_upper_bounds(ops, name, cls):
    """Magnitudes 4x the true maxima, values below 2^20: two bits of the pair's 22 go unused, and the result is still exact."""
    args, kw = G.exact_wgrad_operands(CASES[name], cls, DEV, bits=20)
    A, nbr, M, C, F, dY, N = args
    want = _reference(args)
    scales = (4 * A.abs().max().reshape(1), 4 * dY.abs().max().reshape(1))
    family = _check_info(ops, name, args, kw, scales)
    assert MATH != '' or family == G.PAIRS
    out = ops.wgrad_raw(*args, scales=scales, **kw)
    _check_result(out, want, args, '%s %s bounds' % (name, cls), bias=False)


@pytest.mark.parametrize('name', FLOORS)
def test_all_zero_gradient(ops, name):
    """dY = 0: its magnitude is 0, its scale 1; the weight gradient is exactly zero (no NaN from a scale of a zero)."""
    args, kw = G.exact_wgrad_operands(CASES[name], 'planes_a', DEV)
    A, nbr, M, C, F, dY, N = args
    args = (A, nbr, M, C, F, torch.zeros_like(dY), N)
    _check_info(ops, name, args, kw, True)
    dWt, gb = ops.wgrad_raw(*args, **kw)
    assert not bool(dWt.any()) and not bool(gb.any())          # (a NaN is non-zero)


@pytest.mark.parametrize('scales', [True, False], ids=['scales', 'noscales'])
@pytest.mark.parametrize('name', FLOORS)
def test_second_launch_accumulates(ops, name, scales):
    """The C ABI adds to the image it is given: a second launch onto the first one's result gives exactly twice the values
    (bias gradient included), and the rows past F*C are still zero."""
    from hplflownet_amd import _lib
    args, kw = G.exact_wgrad_operands(CASES[name], 'small', DEV)
    want = _reference(args)
    cargs, dWt, gb, _keep = ops._wgrad_args(*args, taps=kw.get('taps'), want_bias=True, reg_stride=0, scales=scales)
    lib = _lib.load()
    for n in (1, 2):
        assert lib.hpl_gconv_wgrad_scaled(*(cargs + (_lib.stream(),))) == 0
        _check_result((dWt, gb * (1.0 / n)), n * want, args, '%s launch %d' % (name, n))


@pytest.mark.parametrize('cls', ['small', 'planes_a'])
@pytest.mark.parametrize('name', ['w3x_tap_floor', 'w3x_tap_lists'])
def test_table_column_order(ops, name, cls):
    """Tap mode: permuting the vertices (the table's columns with their dY rows) moves every list entry to another slab and
    stage, and gives the same bits."""
    args, kw = G.exact_wgrad_operands(CASES[name], cls, DEV)
    A, nbr, M, C, F, dY, N = args
    want = _reference(args)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(7)).to(DEV)
    nbr_p = nbr[:, perm].contiguous()
    args_p = (A, nbr_p, M, C, F, dY[perm].contiguous(), N)
    kw_p = dict(kw, taps=ops.tap_lists(nbr_p))
    for scales in (True, False):
        _check_info(ops, name, args_p, kw_p, scales)
        base = ops.wgrad_raw(*args, scales=scales, **kw)
        out = ops.wgrad_raw(*args_p, scales=scales, **kw_p)
        assert torch.equal(out[0], base[0])
        _check_result(out, want, args_p, '%s %s permuted scales=%s' % (name, cls, scales), bias=cls != 'planes_dy')
