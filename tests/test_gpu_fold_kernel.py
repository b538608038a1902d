"""GPU: hpl_weight_fold (csrc/gconv.hip) against float64 numpy, and one folded layer pair -- a bias-only 1x1
behind a 15-tap conv through a table with absent taps -- against the unfolded pair and against float64.

The kernel accumulates in double in a fixed order and rounds once: every element within 1 ulp (fp32) of the float64 product,
two calls the same bits.  The layer pair meets the err / sum|a||w| bars tests/test_gpu_split3.py holds these kernels to."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _fold64(W, up0, up_w, Wb, b_tot, ones_col, own_bias=None):
    """float64 numpy: W [O, C, F], Wb [up_w, Cb], b_tot [up_w] or None -> (folded [O, Cout, F], folded bias [O] or None)"""
    W, Wb = W.astype(np.float64), Wb.astype(np.float64)
    up = W[:, up0:up0 + up_w, :]                                     # [O, up_w, F]
    prod = np.einsum('okf,kj->ojf', up, Wb)
    out = np.concatenate([W[:, :up0], prod, W[:, up0 + up_w:]], axis=1)
    if ones_col >= 0:
        ones = np.zeros((W.shape[0], 4, W.shape[2]))
        ones[:, 0, :] = np.einsum('okf,k->of', up, b_tot.astype(np.float64))
        out = np.concatenate([out[:, :ones_col], ones, out[:, ones_col:]], axis=1)
    fb = None
    if own_bias is not None:
        fb = own_bias.astype(np.float64) + (up[:, :, 0] @ b_tot.astype(np.float64) if b_tot is not None else 0.0)
    return out, fb


def _within_one_ulp(got, ref64):
    r32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(r32)).astype(np.float64)
    d = np.abs(got.astype(np.float64) - ref64)
    assert np.all(d <= ulp), 'largest error %.3g ulp' % float((d / ulp).max())


def _rand(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


@pytest.mark.parametrize('case', ['bias', 'no_bias', 'up_not_first'])
def test_fold_of_a_15_tap_consumer(case):
    from hplflownet_amd import ops
    O, F, up_w = 12, 15, 8
    C = 4 + 8 + 4
    up0 = 8 if case == 'up_not_first' else 4             # emg | up | other,  or  emg | other | up
    W = _rand((O, C, F, 1), 1)
    Wb = _rand((up_w, up_w, 1, 1), 2)
    ba, bb = (None, None) if case == 'no_bias' else (_rand((up_w,), 3), _rand((up_w,), 4))
    ones_col = -1 if case == 'no_bias' else 4
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)      # noqa: E731
    got, gb = ops.weight_fold(t(W), F, up0, up_w, t(Wb), t(ba), t(bb), ones_col)
    again, _ = ops.weight_fold(t(W), F, up0, up_w, t(Wb), t(ba), t(bb), ones_col)
    assert gb is None and tuple(got.shape) == (O, C + (4 if ones_col >= 0 else 0), F, 1)
    assert torch.equal(got, again)
    b_tot = None if ba is None else (ba + bb)            # the fp32 sum the unfolded forward adds (plan.bias_sum)
    ref, _ = _fold64(W[..., 0], up0, up_w, Wb[:, :, 0, 0], b_tot, ones_col)
    g = got.cpu().numpy()[..., 0]
    _within_one_ulp(g, ref)
    if ones_col >= 0:                                     # the constant part: one weight column and three of zeros
        assert np.all(g[:, 5:8, :] == 0.0) and np.any(g[:, 4, :] != 0.0)
    # one bias alone is taken as it is
    if case == 'bias':
        got1, _ = ops.weight_fold(t(W), F, up0, up_w, t(Wb), None, t(bb), ones_col)
        _within_one_ulp(got1.cpu().numpy()[..., 0], _fold64(W[..., 0], up0, up_w, Wb[:, :, 0, 0], bb, ones_col)[0])


def test_fold_of_a_dense_head_with_its_bias():
    from hplflownet_amd import ops
    O, C = 16, 8
    W, Wb = _rand((O, C, 1), 5), _rand((C, C, 1, 1), 6)
    ba, bb, own = _rand((C,), 7), _rand((C,), 8), _rand((O,), 9)
    t = lambda a: torch.from_numpy(a).to(DEV)             # noqa: E731
    got, gb = ops.weight_fold(t(W), 1, 0, C, t(Wb), t(ba), t(bb), -1, t(own), True)
    again, gb2 = ops.weight_fold(t(W), 1, 0, C, t(Wb), t(ba), t(bb), -1, t(own), True)
    assert tuple(got.shape) == (O, C, 1) and tuple(gb.shape) == (O,)
    assert torch.equal(got, again) and torch.equal(gb, gb2)
    ref, rb = _fold64(W, 0, C, Wb[:, :, 0, 0], ba + bb, -1, own)
    _within_one_ulp(got.cpu().numpy(), ref)
    _within_one_ulp(gb.cpu().numpy(), rb)


def test_fold_refuses_what_it_cannot_carry():
    from hplflownet_amd import _lib, ops
    t = lambda a: torch.from_numpy(a).to(DEV)             # noqa: E731
    W, Wb, b = t(_rand((12, 16, 15, 1), 1)), t(_rand((8, 8, 1, 1), 2)), t(_rand((8,), 3))
    with pytest.raises(_lib.HplError):                    # a bias with neither a ones part nor a folded bias
        ops.weight_fold(W, 15, 4, 8, Wb, b, None, -1)
    with pytest.raises(_lib.HplError):                    # a ones part behind the folded columns
        ops.weight_fold(W, 15, 4, 8, Wb, b, None, 12)
    with pytest.raises(_lib.HplError):                    # columns outside the weight
        ops.weight_fold(W, 15, 12, 8, Wb, b, None, 4)
    with pytest.raises(_lib.HplError):                    # a folded bias of a 15-tap conv
        ops.weight_fold(W, 15, 4, 8, Wb, b, None, 4, None, True)


# ----------------------------------------------------------------------------- one layer pair
def _table(M, F, seed):
    """int32 [F, M], ~40 % of the taps absent; every 7th row has no present tap at all, every 5th only its own (tap 0)"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    nbr = torch.randint(0, M, (F, M), generator=g, dtype=torch.int32)
    nbr[torch.rand((F, M), generator=g) < 0.4] = -1
    rows = torch.arange(M)
    nbr[:, rows % 5 == 0] = -1
    nbr[0, rows % 5 == 0] = rows[rows % 5 == 0].to(torch.int32)
    nbr[:, rows % 7 == 0] = -1
    return nbr.to(DEV)


def _gather_sum64(A64, nbr, W64):
    """sum_f A[nbr[f]] @ W[:, :, f].T in float64 (absent taps contribute nothing): A64 [M, C], W64 [O, C, F]"""
    y = torch.zeros((nbr.shape[1], W64.shape[0]), dtype=torch.float64, device=A64.device)
    for f in range(nbr.shape[0]):
        idx = nbr[f].long()
        rows = torch.where((idx >= 0)[:, None], A64[idx.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=A64.device))
        y += rows @ W64[:, :, f].t()
    return y


@pytest.mark.parametrize('M,c_up,c_other,O,groups', [(200, 64, 0, 64, False),         # the fp32 kernel
                                                      (1100, 256, 64, 512, True)])      # the pair form: M >= 1024, N >= 256, two tap-group passes
def test_folded_layer_pair_against_the_unfolded_pair_and_float64(M, c_up, c_other, O, groups):
    from hplflownet_amd import ops
    F = 15
    torch.manual_seed(M)
    u = torch.randn(M, c_up, device=DEV) * torch.exp(0.5 * torch.randn(M, 1, device=DEV))
    u = torch.where(u > 0, u, 0.1 * u)                    # what a LeakyReLU leaves
    emg = torch.randn(M, 4, device=DEV)
    other = torch.randn(M, c_other, device=DEV)
    Wb = torch.randn(c_up, c_up, 1, 1, device=DEV) / c_up ** 0.5
    ba, bb = torch.randn(c_up, device=DEV), torch.randn(c_up, device=DEV)
    C = 4 + c_up + c_other
    W = torch.randn(O, C, F, 1, device=DEV) / (F * C) ** 0.5
    bias = torch.randn(O, device=DEV)
    nbr = _table(M, F, 3)
    assert int((nbr >= 0).sum(0).min()) == 0              # rows without any present tap: no bias term there
    kw = {}
    if groups and ops.SPLIT3:         # this case is the pair-form (split-operand) kernel's: both passes qualify, folded (C + 4) and unfolded
        assert all(ops.split3_maybe(M, c, f, O) for c in (C + 4, C) for f in (8, 7))
        assert O >= ops.SPLIT3_MIN_N and C >= ops.SPLIT3_MIN_C
    if groups:
        kw = dict(tap_groups=[(f0, f1, ops.tap_order(nbr[f0:f1].contiguous())) for f0, f1 in ((0, 8), (8, 15))])
    # unfolded: 1x1 + bias, then the 15-tap conv over emg | W_b u + b | other
    b_tot = ba + bb
    y_up = ops.gconv(u, Wb, b_tot, None, M, 1, act=ops.ACT_NONE)
    A = torch.cat([emg, y_up, other], dim=1).contiguous()
    unf = ops.gconv(A, W, bias, nbr, M, F, act=ops.ACT_LEAKY, **kw)
    # folded: the 15-tap conv over emg | 1, 0, 0, 0 | u | other with the folded weight
    Wf, _ = ops.weight_fold(W, F, 4, c_up, Wb, ba, bb, 4)
    ones = torch.zeros(M, 4, device=DEV)
    ones[:, 0] = 1.0
    Af = torch.cat([emg, ones, u, other], dim=1).contiguous()
    fol = ops.gconv(Af, Wf, bias, nbr, M, F, act=ops.ACT_LEAKY, **kw)
    # float64, from the two factors
    W64 = W.double()[..., 0]
    y64 = u.double() @ Wb.double()[:, :, 0, 0].t() + b_tot.double()
    A64 = torch.cat([emg.double(), y64, other.double()], dim=1)
    pre = _gather_sum64(A64, nbr, W64) + bias.double()
    ref = torch.where(pre > 0, pre, ops.LEAKY_RATE * pre)
    # magnitude sums: of the folded contraction, and of the two unfolded ones composed (the first one's error reaches the
    # result through |W15|, so the pair is held to twice the bars)
    mag_f = _gather_sum64(Af.double().abs(), nbr, Wf.double()[..., 0].abs()) + bias.double().abs()
    m64 = u.double().abs() @ Wb.double()[:, :, 0, 0].abs().t() + b_tot.double().abs()
    mag_u = _gather_sum64(torch.cat([emg.double().abs(), m64, other.double().abs()], dim=1), nbr, W64.abs()) + bias.double().abs()
    ef, eu = (fol.double() - ref).abs(), (unf.double() - ref).abs()
    rf, ru = ef / mag_f, eu / mag_u
    print('M=%d C=%d O=%d: max|err| folded %.3g unfolded %.3g (scale %.3g); err / sum|a||w|: folded max %.3g mean %.3g, '
          'unfolded max %.3g mean %.3g' % (M, C + 4, O, float(ef.max()), float(eu.max()), float(ref.abs().max()),
                                           float(rf.max()), float(rf.mean()), float(ru.max()), float(ru.mean())))
    assert float(rf.max()) < 1.5e-6 and float(rf.mean()) < 5e-8
    assert float(ru.max()) < 2 * 1.5e-6 and float(ru.mean()) < 2 * 5e-8
    # rows without a present tap: the bias alone, in both forms (no bias term of the 1x1 leaks in through the ones part)
    dead = (nbr >= 0).sum(0) == 0
    lone = torch.where(bias > 0, bias, ops.LEAKY_RATE * bias)
    tol = 2.0 ** -22 * float(bias.abs().max())
    assert float((fol[dead] - lone).abs().max()) <= tol and float((unf[dead] - lone).abs().max()) <= tol
