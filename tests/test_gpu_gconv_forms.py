"""GPU: every launch form of the fp32 gather-GEMM and of the fp32 weight gradient (the table of tests/gconv_forms.py, whose
instances tests/test_gconv_forms_cpu.py pins) against a float64 restatement computed with torch on the device (index_select +
matmul: nothing of the project's kernels), element by element.

The bar is derived, not measured.  fp32 products accumulated in fp32 in any order, u = 2^-24:
  forward   |y - ref| <= (K + 36) u S + 1e-30,  S = sum_k |a w| + |bias| + |res| in float64 for that element (36: up to 16 splits
            times 2 partial sets, bias, residual, activation; LeakyReLU's slope <= 1 keeps the bound valid)
  scatter   an output element is the atomic sum of T scattered GEMM elements: (K + 36 + T) u (sum of their S)
  wgrad     |dW - ref| <= (M_t + 260) u sum_m |a dy|,  M_t = vertices summed for that entry (260: up to 256 atomic slabs); the bias
            gradient likewise with M_t = M
No Wt3 is passed, so a case runs the same fp32 instance in every HPL_MATH mode.  Weight-gradient cases that hand off to wgrad3
are no cases of this file in the modes where they do (tests/test_gconv_forms_cpu.py pins them, tests/test_gpu_wgrad3.py holds
their bar): they are chosen at collection time, and run here on the fp32 kernel under HPL_MATH=f32."""
import ctypes
import os

import pytest
import torch

import gconv_forms as G

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
SLOPE = 0.1


@pytest.fixture(scope='module')
def ops():
    from hplflownet_amd import ops as o
    return o


def _gather_index(nbr, reg_stride, F, M):
    """[F, M] int64 source rows (-1: absent)."""
    if nbr is not None:
        return nbr.long()
    m = torch.arange(M, device=DEV)
    return torch.stack([f * reg_stride + m for f in range(F)])


def _gathered(A64z, idx, m0, m1):
    """[m1 - m0, F * C] float64: the gathered rows of output rows [m0, m1) (A64z: A in float64 with a zero row appended)."""
    F = idx.shape[0]
    sel = idx[:, m0:m1]
    sel = torch.where(sel < 0, torch.full_like(sel, A64z.shape[0] - 1), sel)
    X = A64z.index_select(0, sel.reshape(-1)).view(F, m1 - m0, -1)
    return X.permute(1, 0, 2).reshape(m1 - m0, -1)


def ref_forward(A, nbr, M, C, F, Wt, N, reg_stride=0, bias=None, res=None, res_mod=0, act=0):
    """-> (y, S) float64 [M, N]: the result and the sum of the magnitudes of its terms."""
    K = F * C
    A64z = torch.cat([A.double(), torch.zeros((1, C), dtype=torch.float64, device=DEV)])
    W = Wt[:K, :N].double()
    idx = _gather_index(nbr, reg_stride, F, M)
    y = torch.empty((M, N), dtype=torch.float64, device=DEV)
    S = torch.empty_like(y)
    chunk = max(1, (1 << 24) // K)
    for m0 in range(0, M, chunk):
        m1 = min(M, m0 + chunk)
        X = _gathered(A64z, idx, m0, m1)
        y[m0:m1] = X @ W
        S[m0:m1] = X.abs() @ W.abs()
    if bias is not None:
        y += bias.double()[None]
        S += bias.double().abs()[None]
    if res is not None:
        r = res.double()[torch.arange(M, device=DEV) % res_mod]
        y += r
        S += r.abs()
    if act:
        y = torch.where(y > 0, y, SLOPE * y)
    return y, S


def _assert_within(got, want, bound, what):
    err = (got.double() - want).abs()
    bad = ~(err <= bound)                 # (a NaN in the result is past every bound)
    if bool(bad.any()):
        i = int((err - bound).argmax())
        r, c = divmod(i, got.shape[1]) if got.dim() == 2 else (i, 0)
        raise AssertionError('%s: %d of %d elements past the bound; worst at (%d, %d): got %r want %r err %.3g bound %.3g'
                             % (what, int(bad.sum()), bad.numel(), r, c, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]),
                                float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])))


@pytest.mark.parametrize('case', G.FORWARD, ids=[c['name'] for c in G.FORWARD])
def test_forward_form(ops, case):
    args, kw, ex = G.forward_operands(case, DEV)
    A, nbr, M, C, F, Wt, N = args
    K = F * C
    info = ops.gconv_launch_info(*args, **kw)
    assert info == G.EXPECT_FORWARD[case['name']]           # device operands take the form the table names
    ref_kw = {k: kw[k] for k in ('reg_stride', 'bias', 'res', 'res_mod') if k in kw}
    if case['scat_c']:
        sc, Fs, srows = case['scat_c'], N // case['scat_c'], case['srows']
        g, s = ref_forward(A, None, M, C, 1, Wt, N, **ref_kw)
        ops.gconv_raw(*args, **kw)
        want = torch.zeros((srows, sc), dtype=torch.float64, device=DEV)
        S = torch.zeros_like(want)
        T = torch.zeros((srows, 1), dtype=torch.float64, device=DEV)
        for f in range(Fs):
            ok = kw['scat'][f] >= 0
            rows = kw['scat'][f][ok].long()
            want.index_add_(0, rows, g[ok, f * sc:(f + 1) * sc])
            S.index_add_(0, rows, s[ok, f * sc:(f + 1) * sc])
            T.index_add_(0, rows, torch.ones((rows.numel(), 1), dtype=torch.float64, device=DEV))
        _assert_within(kw['out'], want, (K + 36 + T) * U * S + 1e-30, case['name'])
        return
    want, S = ref_forward(A, nbr, M, C, F, Wt, N, act=kw['act'], **ref_kw)
    y = ops.gconv_raw(*args, **kw)
    assert y.shape == (M, N)
    _assert_within(y, want, (K + 36) * U * S + 1e-30, case['name'])
    if 'out_buf' in ex:                                     # sentinel columns on both sides of the view stay untouched
        left, right = case['out_pad']
        buf = ex['out_buf']
        assert bool((buf[:, :left] == G.SENTINEL).all())
        assert bool((buf[:, left + N:left + N + max(right, 8)] == G.SENTINEL).all())
    if 'out2_buf' in ex:
        r2, buf2 = case['rows2'], ex['out2_buf']
        assert torch.equal(buf2[:r2, :N], y[:r2])
        assert bool((buf2[r2:] == G.SENTINEL).all()) and bool((buf2[:, N:] == G.SENTINEL).all())
    # no atomics in this form: a second launch is bit-identical
    first = y.clone()
    y2 = ops.gconv_raw(*args, **kw)
    assert torch.equal(first, y2)


# the fp32 kernel's cases in this math mode: HPL_MATH=f32 keeps the wgrad3 hand-offs on it as well
WGRAD_FP32 = [c for c in G.WGRAD if G.EXPECT_WGRAD[c['name']]['family'] == G.FP32 or os.environ.get('HPL_MATH', '') == 'f32']


@pytest.mark.parametrize('case', WGRAD_FP32, ids=[c['name'] for c in WGRAD_FP32])
def test_wgrad_form(ops, case):
    args, kw = G.wgrad_operands(case, DEV)
    A, nbr, M, C, F, dY, N = args
    info = ops.wgrad_launch_info(*args, **kw)
    assert info['family'] == G.FP32                         # (an unexpected hand-off fails here)
    if G.EXPECT_WGRAD[case['name']]['family'] == G.FP32:
        assert info == G.EXPECT_WGRAD[case['name']]
    out = ops.wgrad_raw(*args, **kw)
    dWt, gb = out if case['bias'] else (out, None)
    K = F * C
    idx = _gather_index(nbr, kw.get('reg_stride', 0), F, M)
    A64z = torch.cat([A.double(), torch.zeros((1, C), dtype=torch.float64, device=DEV)])
    d64 = dY.double()
    want = torch.zeros((K, N), dtype=torch.float64, device=DEV)
    S = torch.zeros_like(want)
    chunk = max(1, (1 << 24) // K)
    for m0 in range(0, M, chunk):
        m1 = min(M, m0 + chunk)
        X = _gathered(A64z, idx, m0, m1)                     # [m, F*C]
        want += X.t() @ d64[m0:m1]
        S += X.abs().t() @ d64[m0:m1].abs()
    Mt = (idx >= 0).sum(1).double().repeat_interleave(C)[:, None]          # vertices summed for row k = f*C + c
    _assert_within(dWt[:K, :N], want, (Mt + 260) * U * S + 1e-30, case['name'])
    assert not bool(dWt[K:].any()) and not bool(dWt[:, N:].any())           # rows / columns outside [F*C, N): exactly zero
    if gb is not None:
        _assert_within(gb[None], d64.sum(0)[None], (M + 260) * U * d64.abs().sum(0)[None] + 1e-30, case['name'] + ' bias')


def test_regular_pattern_through_tap_group_passes(ops):
    """gconv_passes cuts a regular pattern into tap groups by slicing A from f0 * reg_stride: two passes, the second adds to the first."""
    case = dict(G.FORWARD[0], name='regular_passes', M=97, rows=15 * 97, C=32, F=15, N=64, table='reg', bias=True, act=True)
    args, kw, _ = G.forward_operands(case, DEV)
    A, _, M, C, F, Wt, N = args
    want, S = ref_forward(A, None, M, C, F, Wt, N, reg_stride=M, bias=kw['bias'], act=1)
    y = ops.gconv_passes(A, None, M, C, F, Wt, N, groups=[(0, 8, None), (8, 15, None)], bias=kw['bias'], act=1, reg_stride=M)
    _assert_within(y, want, (F * C + 72) * U * S + 1e-30, 'two passes')       # (each pass its own 36)
    one = ops.gconv_raw(A, None, M, C, F, Wt, N, bias=kw['bias'], act=1, reg_stride=M)
    _assert_within(one, want, (F * C + 36) * U * S + 1e-30, 'one pass')


def test_contraction_past_the_limit_is_refused_and_writes_nothing(ops):
    from hplflownet_amd import _lib
    M, C, N = 65, 32772, 32
    A = torch.ones((M, C), device=DEV)
    Wt = torch.ones((C + 28, N), device=DEV)
    out = torch.full((M, N), G.SENTINEL, device=DEV)
    with pytest.raises(_lib.HplError, match=r'contraction length F\*C = 32772 > 32768'):
        ops.gconv_raw(A, None, M, C, 1, Wt, N, out=out)
    torch.cuda.synchronize()
    assert bool((out == G.SENTINEL).all())


def test_empty_launch_writes_nothing(ops):
    """M = 0 returns OK and writes nothing (through the C ABI: torch gives an empty tensor a null address)."""
    from hplflownet_amd import _lib
    lib = _lib.load()
    A = torch.ones((4, 8), device=DEV)
    Wt = torch.ones((32, 32), device=DEV)
    Y = torch.full((4, 32), G.SENTINEL, device=DEV)
    d = _lib.GConvDesc()
    d.A, d.lda, d.rows_a, d.M, d.C, d.F = A.data_ptr(), 8, 4, 0, 8, 1
    d.Wt, d.ldw, d.N, d.Y, d.ldy = Wt.data_ptr(), 32, 30, Y.data_ptr(), 32
    assert lib.hpl_gconv_forward(ctypes.byref(d), _lib.stream()) == 0
    dW = torch.full((32, 32), G.SENTINEL, device=DEV)
    gb = torch.full((32,), G.SENTINEL, device=DEV)
    assert lib.hpl_gconv_wgrad_scaled(A.data_ptr(), 8, 4, None, 0, 0, 0, 8, 1, Y.data_ptr(), 32, 30, dW.data_ptr(), 32, None, None, None,
                                      0, gb.data_ptr(), None, None, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((Y == G.SENTINEL).all()) and bool((dW == G.SENTINEL).all()) and bool((gb == G.SENTINEL).all())
