"""CPU: which kernel instance every case of tests/gconv_forms.py takes.  hpl_gconv_launch_info / hpl_wgrad_launch_info run the
selection of hpl_gconv_forward / hpl_gconv_wgrad_scaled itself (the launch path launches from the struct they fill) without a
device, so this test pins the dispatch: a threshold that moves, or a case that leaves the table, fails here -- and the GPU test
(tests/test_gpu_gconv_forms.py) checks the results of the very instances named here."""
import ctypes
import os

import pytest

import gconv_forms as G
from hplflownet_amd import _lib, ops

MATH = os.environ.get('HPL_MATH', '')


def _fwd_info(case):
    args, kw, _ = G.forward_operands(case, 'cpu', fill=False)
    return ops.gconv_launch_info(*args, **kw)


def _wgrad_info(case):
    args, kw = G.wgrad_operands(case, 'cpu', fill=False)
    return ops.wgrad_launch_info(*args, **kw)


def test_tables_are_consistent():
    for cases, expect in ((G.FORWARD, G.EXPECT_FORWARD), (G.WGRAD, G.EXPECT_WGRAD), (G.WGRAD3, G.EXPECT_WGRAD3)):
        names = [c['name'] for c in cases]
        assert len(set(names)) == len(names)
        assert set(names) == set(expect)


@pytest.mark.parametrize('case', G.FORWARD, ids=[c['name'] for c in G.FORWARD])
def test_forward_case_takes_its_form(case):
    assert _fwd_info(case) == G.EXPECT_FORWARD[case['name']]


@pytest.mark.parametrize('case', G.WGRAD, ids=[c['name'] for c in G.WGRAD])
def test_wgrad_case_takes_its_form(case):
    want = G.EXPECT_WGRAD[case['name']]
    got = _wgrad_info(case)
    if want['family'] != G.FP32 and MATH == 'f32':
        assert got['family'] == G.FP32 and got['bn'] == 128       # HPL_MATH=f32 keeps the wide layers on the fp32 kernel
        return
    if want['family'] != G.FP32 and MATH == 'bf16x3':
        want = dict(want, family=G.TRIPLES)
    assert got == want


def _fwd(**kw):
    return dict(family=G.FP32, **kw)


# The forms the table must reach, written out (not computed from the library): every entry is a set of hpl_gconv_info fields
# that at least one FORWARD case must report.
REQUIRED_FORWARD = (
    # each tile configuration, vector and scalar A loads, F_LDS 1 and 15
    [_fwd(bm=bm, bn=bn, threads=th, avec=av, f_lds=fl, compact=0)
     for bm, bn, th in ((64, 32, 128), (128, 32, 256), (64, 64, 256), (64, 128, 512)) for av in (0, 1) for fl in (1, 15)] +
    # the COMPACT instance
    [_fwd(bm=64, bn=128, threads=512, avec=1, f_lds=8, compact=1, splits=1)] +
    # small split-K (<= 128 tiles) and mid split-K (more), each with both finish kernels
    [_fwd(small=True, finish=G.FINISH_SCALAR), _fwd(small=True, finish=G.FINISH_VEC4),
     _fwd(small=False, finish=G.FINISH_SCALAR), _fwd(small=False, finish=G.FINISH_VEC4)] +
    # XCD column order under a row permutation
    [_fwd(col_share=s) for s in (1, 2, 4, 8)] +
    # tile tables used (64- and 128-row tiles) and ignored
    [_fwd(tile_tables=1, bm=64), _fwd(tile_tables=1, bm=128), _fwd(tile_tables=0, given_tiles=True)] +
    # scatter epilogue on a 64-row and a 128-row tile
    [_fwd(scatter=True, bm=64), _fwd(scatter=True, bm=128)] +
    # 64-bit epilogue addressing reached by shape (not by a scatter)
    [_fwd(epi_fast=0, scatter=False)] +
    # the contraction limit: 1024 slices, and 16 splits
    [_fwd(nk=1024, splits=1), _fwd(nk=1024, splits=16), _fwd(nk=512, compact=1), _fwd(nk=513, compact=0, bn=128)]
)


def _fwd_features(case, info):
    f = dict(info)
    f['small'] = info['splits'] > 1 and info['tiles_m'] * info['tiles_n'] <= 128
    if info['splits'] == 1:
        f.pop('small')
    f['given_tiles'] = case['tiles_bm'] is not None
    f['scatter'] = case['scat_c'] > 0
    f['nk'] = (case['F'] * case['C'] + 31) // 32
    return f


def test_every_required_forward_form_is_reached():
    feats = [_fwd_features(c, _fwd_info(c)) for c in G.FORWARD]
    for form in REQUIRED_FORWARD:
        assert any(all(k in f and f[k] == v for k, v in form.items()) for f in feats), 'no FORWARD case reaches %r' % (form,)


def _wg(**kw):
    return dict(family=G.FP32, **kw)


REQUIRED_WGRAD = (
    # BN 32 / 64 / 128, each scalar, vector and tap; BN = 128 with vectors is the 512-thread deep form
    [_wg(bn=32, vec=0, tap=0, threads=256, deep=0), _wg(bn=32, vec=1, tap=0, threads=256, deep=0), _wg(bn=32, vec=1, tap=1, threads=256, deep=0),
     _wg(bn=64, vec=0, tap=0, threads=256, deep=0), _wg(bn=64, vec=1, tap=0, threads=256, deep=0), _wg(bn=64, vec=1, tap=1, threads=256, deep=0),
     _wg(bn=128, vec=0, tap=0, threads=256, deep=0), _wg(bn=128, vec=1, tap=0, threads=512, deep=1),
     _wg(bn=128, vec=1, tap=1, threads=512, deep=1)] +
    # the bias gradient: in the kernel, by column sum (tap mode), none
    [_wg(bias=G.WBIAS_KERNEL), _wg(bias=G.WBIAS_COLSUM, tap=1), _wg(bias=G.WBIAS_NONE)] +
    # scalar loads through a table with F > 1; the regular pattern with vector and scalar loads; N = 3
    [_wg(vec=0, table='rand', F=15), _wg(vec=1, table='reg'), _wg(vec=0, table='reg'), _wg(N=3, vec=0, C=32)] +
    # the tap rule c_tiles * 128 * 4 <= 5 * C with lists given
    [_wg(C=100, taps=True, tap=0), _wg(C=104, taps=True, tap=1), _wg(C=132, taps=True, tap=0), _wg(C=260, taps=True, tap=0),
     _wg(C=256, taps=True, tap=1)] +
    # each side of every threshold of the hand-off to wgrad3, dense and tap
    [dict(wgrad3=True, tap=0, N=256, C=128, M=8192), dict(wgrad3=True, tap=1, N=256, C=128, M=8192),
     _wg(N=252, C=128, M=8192, tap=0, table='dense'), _wg(N=256, C=124, M=8192, table='dense'), _wg(N=256, C=128, M=8191, tap=0, table='dense'),
     _wg(N=258, C=128, M=8192, vec=1, table='dense'), _wg(N=252, C=128, M=8192, tap=1), _wg(N=256, C=128, M=8191, tap=1),
     _wg(N=256, C=128, M=8192, F=15, tap=0, vec=1)]
)


def test_every_required_wgrad_form_is_reached():
    feats = []
    for c in G.WGRAD:
        f = dict(_wgrad_info(c))
        # (the hand-off itself depends on the math mode; the table's entry is the default mode's)
        f['wgrad3'] = G.EXPECT_WGRAD[c['name']]['family'] != G.FP32
        if f['wgrad3']:
            f.pop('family')
        f.update(M=c['M'], C=c['C'], F=c['F'], N=c['N'], table=c['table'], taps=c['taps'])
        feats.append(f)
    for form in REQUIRED_WGRAD:
        assert any(all(k in f and f[k] == v for k, v in form.items()) for f in feats), 'no WGRAD case reaches %r' % (form,)


def _wgrad3_info(case, scales):
    args, kw = G.wgrad_operands(case, 'cpu', fill=False)
    return ops.wgrad_launch_info(*args, scales=scales, **kw)


@pytest.mark.parametrize('scales', [True, False], ids=['scales', 'noscales'])
@pytest.mark.parametrize('case', G.WGRAD3, ids=[c['name'] for c in G.WGRAD3])
def test_wgrad3_case_takes_its_form(case, scales):
    """The pinned entry with magnitudes in the default mode; bf16 triples without them or under HPL_MATH=bf16x3; the fp32
    kernel under HPL_MATH=f32, and in every mode for the two cases that must stay on it."""
    want = G.wgrad3_expect(case['name'], MATH, scales)
    got = _wgrad3_info(case, scales)
    if want is None:
        assert MATH == 'f32' and got['family'] == G.FP32 and got['bn'] == 128
        return
    assert got == want
    if MATH == '' and scales:
        assert got == G.EXPECT_WGRAD3[case['name']]
    if MATH == '' and G.EXPECT_WGRAD3[case['name']]['family'] != G.FP32:
        assert got['family'] == (G.PAIRS if scales else G.TRIPLES)


def test_wgrad3_query_with_the_callers_magnitudes():
    """A pair of float32 [1] tensors selects as measured magnitudes do; anything else is refused."""
    import torch
    case = G.WGRAD3[0]
    args, kw = G.wgrad_operands(case, 'cpu', fill=False)
    one = torch.ones(1)
    assert ops.wgrad_launch_info(*args, scales=(one, one), **kw) == ops.wgrad_launch_info(*args, **kw)
    with pytest.raises(_lib.HplError, match='scales'):
        ops.wgrad_launch_info(*args, scales=(one, torch.ones(1, dtype=torch.float64)), **kw)


# The forms of the split-operand weight gradient the table must reach, written out.  Features (_w3_features): tap, F, the
# vertices of the last dense slab (M - (splits - 1) * m_per_split), the widths of the last channel and column blocks
# (c_tail = C % 128, n_tail = N % 256; 0: full), tiles_k / tiles_n, view (operands as column views), more_rows (rows of A past
# M), lists ('eng': the engineered lists), wgrad3 (the default mode hands off).
REQUIRED_WGRAD3 = (
    # dense: the floor, and a last slab of 1 / 16 / 17 / 33 vertices = 1 / 1 / 2 / 3 steps
    [dict(wgrad3=True, tap=0, M=8192, C=128, N=256, tiles=1, splits=32, m_per_split=256, last_slab=256, view=False)] +
    [dict(wgrad3=True, tap=0, tiles=1, m_per_split=256, splits=33, last_slab=n) for n in (1, 16, 17, 33)] +
    # dense: 4 channels / 4 columns in the second blocks; 3 x 3 tiles; column views with rows of A past M
    [dict(wgrad3=True, tap=0, c_tail=4, n_tail=4, tiles_k=2, tiles_n=2), dict(wgrad3=True, tap=0, tiles_k=3, tiles_n=3),
     dict(wgrad3=True, tap=0, view=True, more_rows=True)] +
    # a view at an odd offset stays on the fp32 kernel
    [dict(wgrad3=False, tap=0, table='dense', view=True, vec=0, M=8192, C=128, N=256)] +
    # tap mode: the floor, F = 2, an 80- and a 68-wide last channel block, 4 columns in a second block, views
    [dict(wgrad3=True, tap=1, M=8192, C=128, F=15, N=256, view=False), dict(wgrad3=True, tap=1, F=2),
     dict(wgrad3=True, tap=1, c_tail=80), dict(wgrad3=True, tap=1, C=324, c_tail=68), dict(wgrad3=True, tap=1, n_tail=4, tiles_n=2),
     dict(wgrad3=True, tap=1, view=True, more_rows=True)] +
    # C = 132 with lists fails the tap rule and stays on the fp32 kernel
    [dict(wgrad3=False, taps=True, tap=0, C=132, M=8192, N=256)] +
    # the engineered lists
    [dict(wgrad3=True, tap=1, F=8, table='eng')]
)


def _w3_features(c):
    want = G.EXPECT_WGRAD3[c['name']]
    f = dict(want)
    f.update(M=c['M'], C=c['C'], F=c['F'], N=c['N'], table=c['table'], taps=c['taps'], wgrad3=want['family'] != G.FP32,
             c_tail=c['C'] % 128, n_tail=c['N'] % 256, view=bool(c['a_off'] or c['dy_off'] or c['a_ld'] or c['dy_ld']),
             more_rows=c['rows'] > c['M'])
    if not want['tap']:
        f['last_slab'] = c['M'] - (want['splits'] - 1) * want['m_per_split']
    return f


def test_every_required_wgrad3_form_is_reached_in_each_family():
    """Every form above is some case's pinned entry (pinned against the query by test_wgrad3_case_takes_its_form), and that case
    takes PAIRS with magnitudes and TRIPLES without in the default mode (there the query itself is asked again)."""
    for form in REQUIRED_WGRAD3:
        hits = [c for c in G.WGRAD3 if all(k in f and f[k] == v for f in [_w3_features(c)] for k, v in form.items())]
        assert hits, 'no WGRAD3 case reaches %r' % (form,)
        if form['wgrad3'] and MATH == '':
            assert any(_wgrad3_info(c, True)['family'] == G.PAIRS and _wgrad3_info(c, False)['family'] == G.TRIPLES for c in hits)
        if not form['wgrad3']:
            assert all(_wgrad3_info(c, s)['family'] == G.FP32 for c in hits for s in (True, False))


@pytest.mark.parametrize('cls', G.CLASSES)
@pytest.mark.parametrize('case', G.WGRAD3, ids=[c['name'] for c in G.WGRAD3])
def test_exact_operands_keep_every_partial_sum_exact(case, cls):
    """The property of the inputs that makes a bit-for-bit comparison legitimate: (|X|^T |dY|).max() < 2^24 in the common unit.
    Also: integer values, the classes' shapes (a full-width operand has its largest magnitude in the top binade)."""
    import torch
    args, _ = G.exact_wgrad_operands(case, cls, 'cpu')
    A, nbr, M, C, F, dY, N = args
    assert G.abs_product_max(args) < G.EXACT_LIMIT
    assert torch.equal(A, A.round()) and torch.equal(dY, dY.round())
    if cls == 'planes_a':
        assert (1 << 21) <= float(A.abs().max()) < (1 << 22) and int((dY != 0).sum(0).max()) <= 4 and float(dY.abs().max()) == 4
    if cls == 'planes_dy':
        assert (1 << 21) <= float(dY.abs().max()) < (1 << 22) and int((A != 0).sum(0).max()) <= 4 and float(A.abs().max()) == 4
    if nbr is not None:                                     # the table reads row 0 and the last row of A somewhere
        assert int(nbr.min()) == -1 and bool((nbr == 0).any()) and int(nbr.max()) < A.shape[0]
        if case['table'] == 'eng':
            assert [int((nbr[f] >= 0).sum()) for f in (0, 1, 2, 3, 4, 5, 7)] == [M, 0, 1, 16, 17, 40, 1]
            assert int(nbr[7, M - 1]) == A.shape[0] - 1


def test_queries_refuse_what_the_launch_refuses():
    """K = 32 772 > 32 768: the query returns the launch's error, with its message."""
    case = dict(G.FORWARD[0], name='k_too_long', C=32772, F=1, M=65, rows=65, N=32, table='dense')
    args, kw, _ = G.forward_operands(case, 'cpu', fill=False)
    with pytest.raises(_lib.HplError, match=r'contraction length F\*C = 32772 > 32768'):
        ops.gconv_launch_info(*args, **kw)
    info = _lib.WGradInfo()
    assert _lib.load().hpl_wgrad_launch_info(None, 4, 4, None, 0, 0, 4, 4, 1, None, 4, 4, None, 4, None, None, None, 0, None, None, None,
                                             ctypes.byref(info)) == -1
    assert b'null pointer' in _lib.load().hpl_last_error()


def test_empty_launch_reports_nothing():
    """M = 0: OK, and an all-zero struct.  (Through the C ABI: torch gives an empty tensor a null address.)"""
    lib = _lib.load()
    d = _lib.GConvDesc()
    d.A, d.lda, d.rows_a, d.M, d.C, d.F = 256, 8, 4, 0, 8, 1
    d.Wt, d.ldw, d.N, d.Y, d.ldy = 256, 32, 30, 256, 30
    info = _lib.GConvInfo(family=7, grid=7)
    assert lib.hpl_gconv_launch_info(ctypes.byref(d), ctypes.byref(info)) == 0
    assert not any(ops._info_dict(info).values())
    w = _lib.WGradInfo(family=7, tiles=7)
    assert lib.hpl_wgrad_launch_info(256, 8, 4, None, 0, 0, 0, 8, 1, 256, 32, 30, 256, 32, None, None, None, 0, 256, None, None,
                                     ctypes.byref(w)) == 0
    assert not any(ops._info_dict(w).values())
