"""The launch forms of the fp32 gather-GEMM (hpl_gconv_forward) and of the weight gradient (hpl_gconv_wgrad_scaled): one table
of cases shared by tests/test_gconv_forms_cpu.py (which instance does a case take: ops.gconv_launch_info / wgrad_launch_info
against the EXPECT_* entries below) and tests/test_gpu_gconv_forms.py (is that instance right: float64 on the device).

WGRAD3 is the table of the split-operand weight gradient (csrc/wgrad3.hip), with operands whose arithmetic is exact
(exact_wgrad_operands; tests/test_gpu_wgrad3_exact.py compares them bit for bit).

A case is a dict of shape parameters; its operands are built by forward_operands / wgrad_operands, with the same shapes,
strides and alignment on either device (the selection reads nothing else).  Shapes are the smallest that reach a form; the
thresholds they sit on are those of csrc/gconv.hip (plan_forward, plan_cfg, plan_wgrad) and csrc/wgrad3.hip (plan_wgrad3):

  tile     N <= 32: <128,32> from ceil(M/128) >= 512 (M >= 65 409), else <64,32>;  32 < N <= 64: <64,64>;
           N > 64: <64,128> from ceil(M/64) * ceil(N/128) >= 512 (N = 65: M >= 32 705; N = 129: M >= 16 321), else <64,64>
  avec     C % 4 == 0, lda % 4 == 0, A 16-byte aligned
  compact  <64,128>, avec, 2 <= F <= 8, ceil(K/32) <= 512, no split
  split-K  (a workspace, no scatter) small: <= 128 tiles and K >= 225;  mid: ceil(K/32) >= 32 and the scored choice > 1
  finish   vec4 when N % 4 == 0 and every row stride and pointer allows 16-byte accesses, else scalar
  order    under a row permutation without split-K: col_share = 8 / gcd(8, tiles_n)
  wgrad    BN 32 / 64 / 128 by N; vec: C, lda, lddy % 4 == 0 and aligned; tap: lists, table, vec, F > 1, c_tiles*128*4 <= 5*C;
           BN = 128 with vec: 512 threads, deep;  wgrad3: vec, (tap or dense without table), N >= 256, N % 4 == 0, C >= 128,
           M >= 8192
"""
import torch

FP32, PAIRS, TRIPLES = 0, 2, 3
FINISH_NONE, FINISH_SCALAR, FINISH_VEC4 = 0, 1, 2
WBIAS_NONE, WBIAS_KERNEL, WBIAS_COLSUM = 0, 1, 2


def _f(name, M, rows, C, F, N, table='rand', **kw):
    d = dict(name=name, M=M, rows=rows, C=C, F=F, N=N, table=table, bias=False, res_mod=0, act=False, a_off=0, a_ld=None,
             out_pad=(0, 0), out_ld=None, perm=False, tiles_bm=None, scat_c=0, srows=0, rows2=None, split_k=True)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


FORWARD = [
    # ---- every tile x vector / scalar A loads x F_LDS 1 / 15 (K < 225 or many tiles: no split)
    _f('t64x32_vec_f1', 129, 129, 8, 1, 30, 'dense', bias=True, act=True),
    _f('t64x32_sca_f1', 65, 65, 3, 1, 1, 'dense', bias=True),
    _f('t64x32_vec_f15', 64, 50, 4, 15, 3, bias=True, res_mod=60, act=True),
    _f('t64x32_sca_f15', 63, 70, 3, 15, 32),
    _f('t128x32_vec_f15', 65409, 500, 8, 15, 32, bias=True, act=True),
    _f('t128x32_sca_f15', 65409, 500, 8, 15, 30, a_off=1, a_ld=12, res_mod=97),      # A: a column view at an odd offset
    _f('t128x32_vec_f1', 65500, 65500, 12, 1, 32, 'dense', bias=True, res_mod=65500),
    _f('t128x32_sca_f1', 65409, 65409, 3, 1, 3, 'dense', bias=True, act=True),
    _f('t64x64_vec_f1', 1, 1, 36, 1, 33, 'dense'),
    _f('t64x64_sca_f1', 129, 129, 1, 1, 65, 'dense', bias=True, act=True),
    _f('t64x64_vec_f15', 129, 100, 12, 15, 64, bias=True, res_mod=1, act=True),
    _f('t64x64_sca_f15', 65, 65, 1, 15, 129),
    _f('t64x128_vec_f15', 32705, 400, 4, 15, 65, bias=True, act=True),
    _f('t64x128_sca_f15', 16321, 400, 3, 15, 129, res_mod=60),
    _f('t64x128_vec_f1', 32705, 32705, 36, 1, 65, 'dense', bias=True, act=True),
    _f('t64x128_sca_f1', 16321, 16321, 4, 1, 129, 'dense', a_ld=5),                   # A: an odd row stride
    # one row fewer: the narrower tile
    _f('below_t128x32', 65408, 500, 8, 15, 32),
    _f('below_t64x128_n65', 32704, 400, 4, 15, 65),
    _f('below_t64x128_n129', 16320, 400, 4, 15, 129),
    # ---- the COMPACT instance, at its limit ceil(K/32) = 512 and just past it
    _f('compact', 32705, 300, 4, 8, 65, bias=True, res_mod=97, act=True),
    _f('compact_f2', 16321, 300, 12, 2, 129, bias=True),
    _f('compact_nk512', 16321, 300, 2048, 8, 129, bias=True),
    _f('past_compact_nk513', 16321, 300, 2052, 8, 129, bias=True),
    _f('not_compact_f9', 16321, 300, 4, 9, 129),
    # ---- split-K, small and mid, each with both finish kernels
    _f('small_split_vec4', 129, 129, 36, 15, 64, bias=True, act=True),
    _f('small_split_scalar', 129, 129, 36, 15, 33, bias=True, res_mod=60),
    _f('small_split_dense', 65, 65, 256, 1, 32, 'dense', bias=True, res_mod=65, act=True),
    _f('below_small_split_k224', 65, 65, 224, 1, 32, 'dense'),
    _f('mid_split_vec4', 8320, 8320, 72, 15, 64, bias=True, act=True),
    _f('mid_split_scalar', 8320, 8320, 72, 15, 63, res_mod=97),
    _f('c100_f15', 64, 64, 100, 15, 33, bias=True),                                   # C % 8 = 4, slices straddle taps
    # ---- the contraction limit K = 32 768: 1024 slices, split 16 ways and in one workgroup
    _f('kmax_split', 65, 65, 32768, 1, 32, 'dense', bias=True),
    _f('kmax_one', 65, 65, 32768, 1, 32, 'dense', split_k=False),
    _f('kmax_stencil', 65, 40, 2184, 15, 33, split_k=False, act=True),                # 32 760 = 1023.75 slices
    # ---- XCD column order under a row permutation: col_share = 8 / gcd(8, tiles_n)
    _f('perm_share1', 700, 650, 4, 15, 500, perm=True, bias=True, act=True),
    _f('perm_share2', 700, 650, 4, 15, 250, perm=True, res_mod=97),
    _f('perm_share4', 700, 650, 4, 15, 100, perm=True, bias=True),
    _f('perm_share8', 700, 650, 4, 15, 40, perm=True, act=True),
    _f('perm_split', 700, 650, 36, 15, 40, perm=True, bias=True),                     # split-K: no column order
    # ---- tile index tables: used, and ignored because they were cut for another tile height
    _f('tiles_used_64', 700, 650, 12, 15, 64, perm=True, tiles_bm=64, bias=True, act=True),
    _f('tiles_ignored_128_on_64', 700, 650, 12, 15, 64, perm=True, tiles_bm=128, bias=True, act=True),
    _f('tiles_used_128', 65409, 500, 8, 15, 32, perm=True, tiles_bm=128, bias=True),
    _f('tiles_ignored_64_on_128', 65409, 500, 8, 15, 32, perm=True, tiles_bm=64, bias=True),
    # ---- scatter epilogue on a 64-row and on a 128-row tile
    _f('scatter_64', 400, 400, 32, 1, 240, 'dense', scat_c=16, srows=300),
    _f('scatter_128', 65409, 65409, 8, 1, 30, 'dense', scat_c=2, srows=500),
    # ---- the epilogue's 64-bit addressing, reached by shape: a row stride of 2^22 floats
    _f('epi_slow', 33, 40, 8, 15, 16, out_ld=1 << 22, bias=True, act=True),
    # ---- output as a column view between sentinel columns; second destination
    _f('outview', 65, 65, 4, 15, 33, out_pad=(1, 2), bias=True),
    _f('outview_split', 129, 129, 36, 15, 30, out_pad=(3, 5), bias=True, act=True),
    _f('outview_aligned_split', 129, 129, 36, 15, 32, out_pad=(4, 8), res_mod=60),
    _f('out2_rows0', 129, 100, 12, 15, 64, rows2=0, bias=True),
    _f('out2_mid_tile', 129, 100, 12, 15, 64, rows2=70, bias=True, act=True),
    _f('out2_all', 129, 100, 12, 15, 64, rows2=129, res_mod=97),
    _f('out2_split', 129, 100, 36, 15, 64, rows2=70, bias=True, act=True),
    _f('out2_split_scalar', 129, 100, 36, 15, 33, rows2=70, bias=True),
    # ---- the regular pattern (no table: tap f of row m reads row f*M + m)
    _f('regular_vec', 97, 15 * 97, 32, 15, 64, 'reg', bias=True, act=True, split_k=False),
    _f('regular_vec_split', 97, 15 * 97, 32, 15, 64, 'reg', bias=True, act=True),
    _f('regular_sca', 97, 15 * 97, 3, 15, 33, 'reg', bias=True),
]


def _w(name, M, rows, C, F, N, table='rand', **kw):
    d = dict(name=name, M=M, rows=rows, C=C, F=F, N=N, table=table, taps=False, bias=True, a_off=0, a_ld=None, dy_off=0, dy_ld=None)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


WGRAD = [
    # ---- BN 32 / 64 / 128, each scalar, vector and tap
    _w('w32_scalar_n3', 300, 300, 3, 1, 3, 'dense'),
    _w('w32_scalar_table', 333, 200, 5, 15, 32),                                      # scalar loads through a table, F > 1
    _w('w32_scalar_lddy3', 900, 900, 32, 1, 3, 'dense'),                              # C allows vectors, lddy = 3 does not
    _w('w32_vec', 1000, 800, 36, 15, 32),
    _w('w32_tap', 1000, 800, 128, 15, 32, taps=True),
    _w('w64_scalar', 500, 500, 7, 15, 33),
    _w('w64_vec', 777, 700, 68, 15, 64),
    _w('w64_tap', 1500, 1500, 104, 15, 40, taps=True),
    _w('w128_scalar', 400, 400, 3, 1, 65, 'dense'),
    _w('w128_vec_deep', 900, 900, 36, 15, 128),
    _w('w128_tap_deep', 2000, 1800, 256, 15, 96, taps=True),
    _w('w128_vec_nobias', 900, 900, 36, 15, 129, bias=False, dy_ld=132),
    # ---- the tap rule c_tiles * 128 * 4 <= 5 * C (lists given every time)
    _w('taprule_c100', 600, 600, 100, 15, 64, taps=True),
    _w('taprule_c104', 600, 600, 104, 15, 64, taps=True),
    _w('taprule_c132', 600, 600, 132, 15, 64, taps=True),
    _w('taprule_c260', 600, 600, 260, 15, 64, taps=True),
    _w('taprule_misaligned', 600, 600, 104, 15, 64, taps=True, a_off=1, a_ld=108),    # lists given, A not 16-byte aligned
    # ---- both sides of every threshold of the hand-off to wgrad3
    _w('w3_dense', 8192, 8192, 128, 1, 256, 'dense'),
    _w('w3_dense_n252', 8192, 8192, 128, 1, 252, 'dense'),
    _w('w3_dense_c124', 8192, 8192, 124, 1, 256, 'dense'),
    _w('w3_dense_m8191', 8191, 8191, 128, 1, 256, 'dense'),
    _w('w3_dense_n258', 8192, 8192, 128, 1, 258, 'dense', dy_ld=260),                 # N % 4
    _w('w3_tap', 8192, 8192, 128, 15, 256, taps=True),
    _w('w3_tap_n252', 8192, 8192, 128, 15, 252, taps=True),
    _w('w3_tap_m8191', 8191, 8191, 128, 15, 256, taps=True),
    _w('w3_table_no_taps', 8192, 8192, 128, 15, 256),                                 # a table without lists stays on fp32
    # ---- the regular pattern
    _w('wreg_c32', 97, 15 * 97, 32, 15, 64, 'reg'),
    _w('wreg_c3', 97, 15 * 97, 3, 15, 32, 'reg'),
    # ---- edges: fewer vertices than one step, operands as views of wider buffers
    _w('w_m5', 5, 9, 8, 15, 16),
    _w('w_m5_tap', 5, 9, 128, 15, 16, taps=True),
    _w('w_views', 1000, 800, 36, 15, 64, a_off=4, a_ld=48, dy_off=4, dy_ld=72),
    _w('w_views_tap', 1000, 800, 128, 15, 64, taps=True, a_off=4, a_ld=140, dy_off=8, dy_ld=80),
    _w('w_view_odd', 1000, 800, 36, 15, 64, a_off=1, a_ld=48),
]


# WGRAD3: the forms of the split-operand weight gradient (csrc/wgrad3.hip), each at the smallest shape that reaches it.  Their
# operands come from exact_wgrad_operands below: integers whose products and sums are exact, so a result has ONE right value.
# Dense slabs are m_per_split vertices (256 with one tile); a tap's list of L vertices is cut into slabs of
# ceil16(ceil(L / splits)).  table = 'eng': the engineered lists of _w3_table.
WGRAD3 = [
    # ---- dense 1x1 layers (F = 1, no table)
    _w('w3x_dense_floor', 8192, 8192, 128, 1, 256, 'dense'),                          # one tile, 32 full slabs
    _w('w3x_dense_m8193', 8193, 8193, 128, 1, 256, 'dense'),                          # a 33rd slab of one vertex
    _w('w3x_dense_m8208', 8208, 8208, 128, 1, 256, 'dense'),                          # last slab 16: one full step
    _w('w3x_dense_m8209', 8209, 8209, 128, 1, 256, 'dense'),                          # 17: two steps, the second of one row
    _w('w3x_dense_m8225', 8225, 8225, 128, 1, 256, 'dense'),                          # 33: three steps
    _w('w3x_dense_c132_n260', 8192, 8192, 132, 1, 260, 'dense'),                      # 4 channels / 4 columns in the second blocks
    _w('w3x_dense_c260_n516', 8192, 8192, 260, 1, 516, 'dense'),                      # 3 x 3 tiles
    _w('w3x_dense_views', 8192, 8192 + 53, 128, 1, 256, 'dense', a_off=4, a_ld=140, dy_off=8, dy_ld=268),
    _w('w3x_dense_view_odd', 8192, 8192, 128, 1, 256, 'dense', a_off=1, a_ld=140),    # not 16-byte aligned: the fp32 kernel
    # ---- tap mode (a table and its lists)
    _w('w3x_tap_floor', 8192, 8192, 128, 15, 256, taps=True),
    _w('w3x_tap_f2', 8192, 8192, 128, 2, 256, taps=True),
    _w('w3x_tap_c208', 8192, 8192, 208, 15, 256, taps=True),                          # an 80-wide last channel block
    _w('w3x_tap_c324', 8192, 8192, 324, 15, 256, taps=True),                          # 68-wide (the model's bcn2_)
    _w('w3x_tap_c132', 8192, 8192, 132, 15, 256, taps=True),                          # fails the tap rule: the fp32 kernel
    _w('w3x_tap_n260', 8192, 8192, 128, 15, 260, taps=True),
    _w('w3x_tap_views', 8192, 8192 + 53, 128, 15, 256, taps=True, a_off=4, a_ld=140, dy_off=8, dy_ld=268),
    _w('w3x_tap_lists', 8192, 8192, 128, 8, 256, 'eng', taps=True),
]


def _gi(family, bm, bn, threads, avec, f_lds, compact, splits, guard_sets, col_share, col_rows, tile_tables, epi_fast, finish,
        tiles_m, tiles_n, grid):
    return dict(family=family, bm=bm, bn=bn, threads=threads, avec=avec, f_lds=f_lds, compact=compact, splits=splits,
                guard_sets=guard_sets, col_share=col_share, col_rows=col_rows, tile_tables=tile_tables, epi_fast=epi_fast,
                finish=finish, tiles_m=tiles_m, tiles_n=tiles_n, grid=grid)


def _wi(family, bn, vec, tap, threads, deep, tiles_k, tiles_n, bias, tiles, splits, m_per_split):
    return dict(family=family, bn=bn, vec=vec, tap=tap, threads=threads, deep=deep, tiles_k=tiles_k, tiles_n=tiles_n, bias=bias,
                tiles=tiles, splits=splits, m_per_split=m_per_split)


# EXPECT_FORWARD / EXPECT_WGRAD: the instance every case is there to reach (all fields of hpl_gconv_info / hpl_wgrad_info), in the
# default math mode.  Cases whose family is not FP32 hand off to wgrad3.hip; under HPL_MATH=f32 they stay on the fp32 kernel.
EXPECT_FORWARD = {
    # name: _gi(family, bm, bn, threads, avec, f_lds, compact, splits, guard_sets, col_share, col_rows, tile_tables, epi_fast,
    #           finish, tiles_m, tiles_n, grid)
    't64x32_vec_f1': _gi(0, 64, 32, 128, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 3, 1, 3),
    't64x32_sca_f1': _gi(0, 64, 32, 128, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    't64x32_vec_f15': _gi(0, 64, 32, 128, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1),
    't64x32_sca_f15': _gi(0, 64, 32, 128, 0, 15, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1),
    't128x32_vec_f15': _gi(0, 128, 32, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't128x32_sca_f15': _gi(0, 128, 32, 256, 0, 15, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't128x32_vec_f1': _gi(0, 128, 32, 256, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't128x32_sca_f1': _gi(0, 128, 32, 256, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't64x64_vec_f1': _gi(0, 64, 64, 256, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1),
    't64x64_sca_f1': _gi(0, 64, 64, 256, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 3, 2, 6),
    't64x64_vec_f15': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 3, 1, 3),
    't64x64_sca_f15': _gi(0, 64, 64, 256, 0, 15, 0, 1, 1, 0, 0, 0, 1, 0, 2, 3, 6),
    't64x128_vec_f15': _gi(0, 64, 128, 512, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't64x128_sca_f15': _gi(0, 64, 128, 512, 0, 15, 0, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    't64x128_vec_f1': _gi(0, 64, 128, 512, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    't64x128_sca_f1': _gi(0, 64, 128, 512, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    'below_t128x32': _gi(0, 64, 32, 128, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 1022, 1, 1022),
    'below_t64x128_n65': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 511, 2, 1022),
    'below_t64x128_n129': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 255, 3, 765),
    'compact': _gi(0, 64, 128, 512, 1, 8, 1, 1, 1, 0, 0, 0, 1, 0, 512, 1, 512),
    'compact_f2': _gi(0, 64, 128, 512, 1, 8, 1, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    'compact_nk512': _gi(0, 64, 128, 512, 1, 8, 1, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    'past_compact_nk513': _gi(0, 64, 128, 512, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    'not_compact_f9': _gi(0, 64, 128, 512, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 256, 2, 512),
    'small_split_vec4': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 2, 3, 1, 12),
    'small_split_scalar': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 1, 3, 1, 12),
    'small_split_dense': _gi(0, 64, 32, 128, 1, 1, 0, 2, 1, 0, 0, 0, 1, 2, 2, 1, 4),
    'below_small_split_k224': _gi(0, 64, 32, 128, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    'mid_split_vec4': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 2, 130, 1, 520),
    'mid_split_scalar': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 1, 130, 1, 520),
    'c100_f15': _gi(0, 64, 64, 256, 1, 15, 0, 11, 1, 0, 0, 0, 1, 1, 1, 1, 11),
    'kmax_split': _gi(0, 64, 32, 128, 1, 1, 0, 16, 1, 0, 0, 0, 1, 2, 2, 1, 32),
    'kmax_one': _gi(0, 64, 32, 128, 1, 1, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    'kmax_stencil': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    'perm_share1': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 1, 11, 0, 1, 0, 11, 8, 88),
    'perm_share2': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 2, 8, 0, 1, 0, 11, 4, 64),
    'perm_share4': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 4, 4, 0, 1, 0, 11, 2, 32),
    'perm_share8': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 8, 4, 0, 1, 0, 11, 1, 32),
    'perm_split': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 2, 11, 1, 44),
    'tiles_used_64': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 8, 4, 1, 1, 0, 11, 1, 32),
    'tiles_ignored_128_on_64': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 8, 4, 0, 1, 0, 11, 1, 32),
    'tiles_used_128': _gi(0, 128, 32, 256, 1, 15, 0, 1, 1, 8, 64, 1, 1, 0, 512, 1, 512),
    'tiles_ignored_64_on_128': _gi(0, 128, 32, 256, 1, 15, 0, 1, 1, 8, 64, 0, 1, 0, 512, 1, 512),
    'scatter_64': _gi(0, 64, 64, 256, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 7, 4, 28),
    'scatter_128': _gi(0, 128, 32, 256, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 512, 1, 512),
    'epi_slow': _gi(0, 64, 32, 128, 1, 15, 0, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1),
    'outview': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    'outview_split': _gi(0, 64, 32, 128, 1, 15, 0, 4, 1, 0, 0, 0, 1, 1, 3, 1, 12),
    'outview_aligned_split': _gi(0, 64, 32, 128, 1, 15, 0, 4, 1, 0, 0, 0, 1, 2, 3, 1, 12),
    'out2_rows0': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 3, 1, 3),
    'out2_mid_tile': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 3, 1, 3),
    'out2_all': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 3, 1, 3),
    'out2_split': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 2, 3, 1, 12),
    'out2_split_scalar': _gi(0, 64, 64, 256, 1, 15, 0, 4, 1, 0, 0, 0, 1, 1, 3, 1, 12),
    'regular_vec': _gi(0, 64, 64, 256, 1, 15, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
    'regular_vec_split': _gi(0, 64, 64, 256, 1, 15, 0, 3, 1, 0, 0, 0, 1, 2, 2, 1, 6),
    'regular_sca': _gi(0, 64, 64, 256, 0, 15, 0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 2),
}

EXPECT_WGRAD = {
    # name: _wi(family, bn, vec, tap, threads, deep, tiles_k, tiles_n, bias, tiles, splits, m_per_split)
    'w32_scalar_n3': _wi(0, 32, 0, 0, 256, 0, 1, 1, 1, 1, 5, 64),
    'w32_scalar_table': _wi(0, 32, 0, 0, 256, 0, 1, 1, 1, 1, 6, 64),
    'w32_scalar_lddy3': _wi(0, 32, 0, 0, 256, 0, 1, 1, 1, 1, 15, 64),
    'w32_vec': _wi(0, 32, 1, 0, 256, 0, 5, 1, 1, 5, 16, 64),
    'w32_tap': _wi(0, 32, 1, 1, 256, 0, 15, 1, 2, 15, 1, 1024),
    'w64_scalar': _wi(0, 64, 0, 0, 256, 0, 1, 1, 1, 1, 8, 64),
    'w64_vec': _wi(0, 64, 1, 0, 256, 0, 8, 1, 1, 8, 13, 64),
    'w64_tap': _wi(0, 64, 1, 1, 256, 0, 15, 1, 2, 15, 2, 768),
    'w128_scalar': _wi(0, 128, 0, 0, 256, 0, 1, 1, 1, 1, 7, 64),
    'w128_vec_deep': _wi(0, 128, 1, 0, 512, 1, 5, 1, 1, 5, 15, 64),
    'w128_tap_deep': _wi(0, 128, 1, 1, 512, 1, 30, 1, 2, 30, 2, 1024),
    'w128_vec_nobias': _wi(0, 128, 1, 0, 512, 1, 5, 2, 0, 10, 15, 64),
    'taprule_c100': _wi(0, 64, 1, 0, 256, 0, 12, 1, 1, 12, 10, 64),
    'taprule_c104': _wi(0, 64, 1, 1, 256, 0, 15, 1, 2, 15, 1, 608),
    'taprule_c132': _wi(0, 64, 1, 0, 256, 0, 16, 1, 1, 16, 10, 64),
    'taprule_c260': _wi(0, 64, 1, 0, 256, 0, 31, 1, 1, 31, 10, 64),
    'taprule_misaligned': _wi(0, 64, 0, 0, 256, 0, 13, 1, 1, 13, 10, 64),
    'w3_dense': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 32, 256),
    'w3_dense_n252': _wi(0, 128, 1, 0, 512, 1, 1, 2, 1, 2, 128, 64),
    'w3_dense_c124': _wi(0, 128, 1, 0, 512, 1, 1, 2, 1, 2, 128, 64),
    'w3_dense_m8191': _wi(0, 128, 1, 0, 512, 1, 1, 2, 1, 2, 128, 64),
    'w3_dense_n258': _wi(0, 128, 1, 0, 512, 1, 1, 3, 1, 3, 128, 64),
    'w3_tap': _wi(2, 256, 1, 1, 512, 0, 15, 1, 2, 15, 8, 1024),
    'w3_tap_n252': _wi(0, 128, 1, 1, 512, 1, 15, 2, 2, 30, 8, 1024),
    'w3_tap_m8191': _wi(0, 128, 1, 1, 512, 1, 15, 2, 2, 30, 8, 1024),
    'w3_table_no_taps': _wi(0, 128, 1, 0, 512, 1, 15, 2, 1, 30, 16, 512),
    'wreg_c32': _wi(0, 64, 1, 0, 256, 0, 4, 1, 1, 4, 2, 64),
    'wreg_c3': _wi(0, 32, 0, 0, 256, 0, 1, 1, 1, 1, 2, 64),
    'w_m5': _wi(0, 32, 1, 0, 256, 0, 1, 1, 1, 1, 1, 32),
    'w_m5_tap': _wi(0, 32, 1, 1, 256, 0, 15, 1, 2, 15, 1, 32),
    'w_views': _wi(0, 64, 1, 0, 256, 0, 5, 1, 1, 5, 16, 64),
    'w_views_tap': _wi(0, 64, 1, 1, 256, 0, 15, 1, 2, 15, 1, 1024),
    'w_view_odd': _wi(0, 64, 0, 0, 256, 0, 5, 1, 1, 5, 16, 64),
}

# EXPECT_WGRAD3: as EXPECT_WGRAD, for the default mode with operand magnitudes (scales=True).  wgrad3_expect gives the entry of
# another selection.
EXPECT_WGRAD3 = {
    'w3x_dense_floor': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 32, 256),
    'w3x_dense_m8193': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 33, 256),
    'w3x_dense_m8208': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 33, 256),
    'w3x_dense_m8209': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 33, 256),
    'w3x_dense_m8225': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 33, 256),
    'w3x_dense_c132_n260': _wi(2, 256, 1, 0, 512, 0, 2, 2, 2, 4, 32, 256),
    'w3x_dense_c260_n516': _wi(2, 256, 1, 0, 512, 0, 3, 3, 2, 9, 27, 304),
    'w3x_dense_views': _wi(2, 256, 1, 0, 512, 0, 1, 1, 2, 1, 32, 256),
    'w3x_dense_view_odd': _wi(0, 128, 0, 0, 256, 0, 1, 2, 1, 2, 128, 64),
    'w3x_tap_floor': _wi(2, 256, 1, 1, 512, 0, 15, 1, 2, 15, 8, 1024),
    'w3x_tap_f2': _wi(2, 256, 1, 1, 512, 0, 2, 1, 2, 2, 8, 1024),
    'w3x_tap_c208': _wi(2, 256, 1, 1, 512, 0, 30, 1, 2, 30, 8, 1024),
    'w3x_tap_c324': _wi(2, 256, 1, 1, 512, 0, 45, 1, 2, 45, 8, 1024),
    'w3x_tap_c132': _wi(0, 128, 1, 0, 512, 1, 16, 2, 1, 32, 16, 512),
    'w3x_tap_n260': _wi(2, 256, 1, 1, 512, 0, 15, 2, 2, 30, 8, 1024),
    'w3x_tap_views': _wi(2, 256, 1, 1, 512, 0, 15, 1, 2, 15, 8, 1024),
    'w3x_tap_lists': _wi(2, 256, 1, 1, 512, 0, 8, 1, 2, 8, 8, 1024),
}


def wgrad3_expect(name, math='', scales=True):
    """The hpl_wgrad_info a WGRAD3 case must report under HPL_MATH = math, with (scales=True) or without operand magnitudes:
    the pinned entry with the family the selection leaves -- bf16 triples without magnitudes or under bf16x3.  None: under
    HPL_MATH=f32 a split-operand case stays on the fp32 kernel (family FP32, BN 128; its cut is that kernel's own)."""
    want = EXPECT_WGRAD3[name]
    if want['family'] == FP32:
        return want
    if math == 'f32':
        return None
    if math == 'bf16x3' or scales is False:
        return dict(want, family=TRIPLES)
    return want


# ------------------------------------------------------------------------------------------ operands
def _rand(shape, gen, device, fill):
    if not fill:
        return torch.empty(shape, dtype=torch.float32, device=device)
    return torch.randn(shape, generator=gen, dtype=torch.float32).to(device)


def _view(rows, cols, off, ld, gen, device, fill, pad_value=None):
    """A [rows, cols] matrix as the column view [off, off + cols) of a buffer with row stride ld (None: off + cols)."""
    ld = ld if ld is not None else off + cols
    if ld == cols and off == 0:
        return _rand((rows, cols), gen, device, fill)
    buf = _rand((rows, ld), gen, device, fill)
    return buf[:, off:off + cols]


def _table(case, gen, device, fill, density=0.7):
    F, M, rows = case['F'], case['M'], case['rows']
    if case['table'] in ('dense', 'reg'):
        return None
    assert case['table'] == 'rand' or not fill           # ('eng': filled by exact_wgrad_operands alone)
    if not fill:
        return torch.empty((F, M), dtype=torch.int32, device=device)
    nbr = torch.randint(0, rows, (F, M), generator=gen, dtype=torch.int32)
    nbr[torch.rand((F, M), generator=gen) >= density] = -1
    return nbr.to(device)


def forward_operands(case, device, fill=True):
    """Operands of ops.gconv_raw / ops.gconv_launch_info for a FORWARD case -> (args, kwargs, extras).  fill=False: same shapes,
    strides and alignment with unset contents (enough for the query, which reads none of it)."""
    gen = torch.Generator().manual_seed(sum(map(ord, case['name'])))
    M, rows, C, F, N = case['M'], case['rows'], case['C'], case['F'], case['N']
    K = F * C
    A = _view(rows, C, case['a_off'], case['a_ld'], gen, device, fill)
    nbr = _table(case, gen, device, fill)
    ldw = (N + 3) // 4 * 4
    Wt = torch.zeros(((K + 31) // 32 * 32, ldw), dtype=torch.float32, device=device) if fill else \
        torch.empty(((K + 31) // 32 * 32, ldw), dtype=torch.float32, device=device)
    if fill:
        Wt[:K, :N] = (torch.randn((K, N), generator=gen) / K ** 0.5).to(device)
    kw = dict(act=1 if case['act'] else 0, split_k=case['split_k'])
    if case['table'] == 'reg':
        kw['reg_stride'] = M
    if case['bias']:
        kw['bias'] = _rand((N,), gen, device, fill)
    if case['res_mod']:
        kw['res'] = _rand((case['res_mod'], N), gen, device, fill)
        kw['res_mod'] = case['res_mod']
    ex = {}
    if case['scat_c']:
        Fs = N // case['scat_c']
        if fill:
            scat = torch.randint(0, case['srows'], (Fs, M), generator=gen, dtype=torch.int32)
            scat[torch.rand((Fs, M), generator=gen) >= 0.7] = -1
            scat = scat.to(device)
        else:
            scat = torch.empty((Fs, M), dtype=torch.int32, device=device)
        kw.update(scat=scat, scat_c=case['scat_c'], out=torch.zeros((case['srows'], case['scat_c']), dtype=torch.float32, device=device))
    else:
        left, right = case['out_pad']
        ld = case['out_ld'] or (left + N + right)
        if ld != N:
            buf = torch.empty((M, ld), dtype=torch.float32, device=device)
            if fill:
                buf[:, :left + N + max(right, 8)] = SENTINEL
            ex['out_buf'] = buf
            kw['out'] = buf[:, left:left + N]
    if case['rows2'] is not None:
        buf2 = torch.full((M, N + 4), SENTINEL, dtype=torch.float32, device=device)
        ex['out2_buf'] = buf2
        kw.update(out2=buf2[:, :N], rows2=case['rows2'])
    if case['perm']:
        kw['row_perm'] = (torch.randperm(M, generator=gen).to(torch.int32) if fill else torch.empty(M, dtype=torch.int32)).to(device)
        if case['tiles_bm']:
            bm = case['tiles_bm']
            if fill:
                from hplflownet_amd import ops
                kw['tiles'] = ops.tile_index(nbr, kw['row_perm'], bm)
            else:
                t = (M + bm - 1) // bm
                kw['tiles'] = (torch.empty((t, F, bm), dtype=torch.int32, device=device),
                               torch.empty((t, 8), dtype=torch.int32, device=device))
    return (A, nbr, M, C, F, Wt, N), kw, ex


SENTINEL = -77.0


def wgrad_operands(case, device, fill=True):
    """Operands of ops.wgrad_raw / ops.wgrad_launch_info for a WGRAD case -> (args, kwargs)."""
    gen = torch.Generator().manual_seed(sum(map(ord, case['name'])))
    M, rows, C, F, N = case['M'], case['rows'], case['C'], case['F'], case['N']
    A = _view(rows, C, case['a_off'], case['a_ld'], gen, device, fill)
    dY = _view(M, N, case['dy_off'], case['dy_ld'], gen, device, fill)
    nbr = _table(case, gen, device, fill, density=0.5)
    kw = dict(want_bias=case['bias'])
    if case['table'] == 'reg':
        kw['reg_stride'] = M
    if case['taps']:
        if fill:
            nbr[0] = torch.arange(M, dtype=torch.int32, device=device) % rows      # the centre tap: always present
            nbr[3] = -1                                                            # a tap with an empty list
            from hplflownet_amd import ops
            kw['taps'] = ops.tap_lists(nbr)
        else:
            kw['taps'] = (torch.empty(F * M, dtype=torch.int32, device=device), torch.empty(F * M, dtype=torch.int32, device=device),
                          torch.empty(F + 1, dtype=torch.int32, device=device))
    return (A, nbr, M, C, F, dY, N), kw


# ------------------------------------------------------------------------------------------ exact operands (WGRAD3)
# Integer-valued operands whose weight gradient has one right value in every form and family:
#   * a power-of-two scale is exact, and an integer below 2^22 is exactly an fp16 pair once the largest magnitude of its matrix
#     sits in the top binade (14 + 7 bits below the scaled unit 2^-7 ... fp16's 11 + 11), and exactly a bf16 triple (3 x 8 bits);
#   * the kernel keeps hi*hi, hi*lo, lo*hi of pairs and the products with i + j <= 2 of triples: with one operand full width and
#     the other in its first plane alone, nothing that is dropped is non-zero;
#   * every partial sum is an integer of the common unit below 2^24, so fp32 accumulation is exact in any order.
# The last point is the precondition abs_product_max checks: (|X|^T |dY|).max() < EXACT_LIMIT.  The classes stay below
# 0.75 * 2^24 where a column has more than one term, so that the partial sums of a single plane (|hi| <= |x| (1 + 2^-8)) stay
# below 2^24 too; a lone term 4 * (2^22 - 1) is one exact product per plane.
EXACT_LIMIT = 1 << 24
CLASSES = ('small', 'planes_a', 'planes_dy', 'ramp')
_POW2_PATTERNS = ((4,), (2, 1), (1, 1, 1), (1, 1, 1))     # magnitudes of the non-zero entries of one column: sum <= 3, or 4 alone
PAD = 1234567.5                                           # what lies beside a view: reading it ruins a result


def _w3_table(case, gen):
    """The [F, M] table of a WGRAD3 case (None: dense).  Every tap reads distinct rows, so that a channel's magnitudes sum over
    a tap at most once each.  'rand': tap 0 is every vertex (reading row 0 .. M - 1), tap 3 is empty, the others a random half.
    'eng' (F = 8): every vertex / none / one / exactly 16 / 17 / 40 (fewer than 8 slabs x 16: trailing slabs are empty) / a
    random half / vertex M - 1 alone, reading the last row of A."""
    F, M, rows = case['F'], case['M'], case['rows']
    if case['table'] == 'dense':
        return None
    nbr = torch.full((F, M), -1, dtype=torch.int32)
    nbr[0] = torch.arange(M, dtype=torch.int32)
    for f in range(1, F):
        src = torch.randperm(rows, generator=gen)[:M].to(torch.int32)
        if case['table'] == 'eng':
            count = {1: 0, 2: 1, 3: 16, 4: 17, 5: 40, 6: None, 7: 0}[f]
        else:
            count = 0 if f == 3 else None
        if count is None:
            keep = torch.rand(M, generator=gen) < 0.5
        else:
            keep = torch.zeros(M, dtype=torch.bool)
            keep[torch.randperm(M, generator=gen)[:count]] = True
        nbr[f] = torch.where(keep, src, torch.full_like(src, -1))
    if case['table'] == 'eng':
        nbr[7, M - 1] = rows - 1
    return nbr


def _w3_marks(case, nbr):
    """[(tap, vertex)] the sparse classes place their non-zeros at: the first and last vertex of every slab of every tap's list
    (without tap mode: of the vertex range, which tap 0 reads whole), every position 0 .. 15 of a 16-vertex stage (tap 0), vertex 0 and
    vertex M - 1."""
    M, want = case['M'], EXPECT_WGRAD3[case['name']]
    marks = []
    for f in range(case['F'] if want['tap'] else 1):
        present = torch.nonzero(nbr[f] >= 0)[:, 0] if want['tap'] else torch.arange(M)
        L = present.numel()
        if L == 0:
            continue
        per = (-(-L // want['splits']) + 15) // 16 * 16 if want['tap'] else want['m_per_split']
        slabs = -(-L // per)
        pos = [0, L - 1]
        for s in range(slabs):
            pos += [s * per, min(L, (s + 1) * per) - 1]
        if f == 0:
            pos += [(i % slabs) * per + 16 * (i % 3) + i for i in range(16)]
        marks += [(f, int(present[j])) for j in dict.fromkeys(pos) if j < L]
    return marks


def _sparse_pow2(shape, lines_axis, targets, gen):
    """A zero matrix with, on every line (column of dY, channel of A: lines_axis = 1), the entries of one of _POW2_PATTERNS with
    random signs at consecutive rows of `targets` (cyclic: every target is used when the lines offer enough slots)."""
    X = torch.zeros(shape, dtype=torch.float32)
    n_lines, t = shape[lines_axis], 0
    assert len(targets) >= 3
    sign = torch.randint(0, 2, (n_lines, 3), generator=gen) * 2 - 1
    for n in range(n_lines):
        for k, mag in enumerate(_POW2_PATTERNS[n % len(_POW2_PATTERNS)]):
            X[targets[t % len(targets)], n] = float(mag * sign[n, k])
            t += 1
    assert t >= len(targets), 'more marked vertices (%d) than slots (%d)' % (len(targets), t)
    return X


def _full_width(shape, bits, gen):
    """Integers uniform in (-2^bits, 2^bits), with entry [0, 0] = -(2^bits - 1): the largest magnitude, and an odd one."""
    X = torch.randint(-(1 << bits) + 1, 1 << bits, shape, generator=gen).float()
    X[0, 0] = -float((1 << bits) - 1)
    return X


def _as_view(X, off, ld, device):
    """X on the device as the column view [off, off + cols) of a buffer with row stride ld (None: contiguous) filled with PAD."""
    rows, cols = X.shape
    if ld is None or (ld == cols and off == 0):
        return X.to(device)
    buf = torch.full((rows, ld), PAD, dtype=torch.float32)
    buf[:, off:off + cols] = X
    return buf.to(device)[:, off:off + cols]


def exact_wgrad_operands(case, cls, device, bits=22):
    """Operands of ops.wgrad_raw / ops.wgrad_launch_info for a WGRAD3 case in class cls -> (args, kwargs); the tap lists are built
    on a GPU only (the query and the precondition need none).  bits: the width of the full-width operand of the planes_ classes.
      small      A, dY dense integers in [-15, 15]: every vertex, tail and slab contributes
      planes_a   A integers in (-2^bits, 2^bits); dY zero but for +-2^p (p in 0..2) at the marked vertices (_w3_marks)
      planes_dy  the mirror image: dY full width, A zero but for +-2^p in the rows the marked vertices read
      ramp       A integers of 12-13 significant bits, dY in {-1, 0, 1} at 1/8 density"""
    gen = torch.Generator().manual_seed(sum(map(ord, case['name'])) + 1000 * CLASSES.index(cls))
    M, rows, C, F, N = case['M'], case['rows'], case['C'], case['F'], case['N']
    nbr = _w3_table(case, gen)
    if cls == 'small':
        A = torch.randint(-15, 16, (rows, C), generator=gen).float()
        dY = torch.randint(-15, 16, (M, N), generator=gen).float()
    elif cls == 'ramp':
        A = torch.randint(1 << 11, 1 << 13, (rows, C), generator=gen).float() * (torch.randint(0, 2, (rows, C), generator=gen) * 2 - 1)
        dY = torch.randint(-1, 2, (M, N), generator=gen).float() * (torch.rand((M, N), generator=gen) < 0.1875)     # (2/3 non-zero)
    elif cls == 'planes_a':
        A = _full_width((rows, C), bits, gen)
        dY = _sparse_pow2((M, N), 1, list(dict.fromkeys(m for _, m in _w3_marks(case, nbr))), gen)
    elif cls == 'planes_dy':
        marks = _w3_marks(case, nbr)
        A = _sparse_pow2((rows, C), 1, list(dict.fromkeys(m if nbr is None else int(nbr[f, m]) for f, m in marks)), gen)
        dY = _full_width((M, N), bits, gen)
    else:
        raise ValueError(cls)
    A, dY = _as_view(A, case['a_off'], case['a_ld'], device), _as_view(dY, case['dy_off'], case['dy_ld'], device)
    nbr = None if nbr is None else nbr.to(device)
    kw = dict(want_bias=case['bias'])
    if case['taps'] and A.is_cuda:
        from hplflownet_amd import ops
        kw['taps'] = ops.tap_lists(nbr)
    return (A, nbr, M, C, F, dY, N), kw


def wgrad_ref64(A, nbr, M, C, F, dY, N):
    """-> (dW, S) [F*C, N] in dtype float64 on a GPU: the weight gradient restated with index_select + matmul, and the sum of the
    magnitudes of its terms, (|X|^T |dY|).  On the CPU float32 serves: sums of non-negative integers are exact there until they
    reach 2^24 and never fall below it afterwards, which is all the precondition asks."""
    dt = torch.float64 if A.is_cuda else torch.float32
    Az = torch.cat([A.to(dt), torch.zeros((1, C), dtype=dt, device=A.device)])
    d = dY.to(dt)
    dW = torch.empty((F * C, N), dtype=dt, device=A.device)
    S = torch.empty_like(dW)
    for f in range(F):
        idx = torch.arange(M, device=A.device) if nbr is None else nbr[f].long()
        # (only vertices with something on both sides: the sparse classes leave a few hundred)
        live = torch.nonzero((idx >= 0) & d.ne(0).any(1))[:, 0]
        X = Az.index_select(0, idx[live])
        use = X.ne(0).any(1)
        X, D = X[use], d[live[use]]
        dW[f * C:(f + 1) * C] = X.t() @ D
        S[f * C:(f + 1) * C] = X.abs().t() @ D.abs()
    return dW, S


def abs_product_max(args):
    """(|X|^T |dY|).max() of a weight-gradient operand set: below EXACT_LIMIT, every fp32 partial sum is exact."""
    return float(wgrad_ref64(*args)[1].max())
