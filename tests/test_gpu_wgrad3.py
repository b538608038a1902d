"""The split-operand weight gradient (csrc/wgrad3.hip: both fp32 operands split while they are staged, MFMA fragments fetched
with the LDS transpose read) against float64 and against the fp32-MFMA kernel (HPL_WGRAD3=0 in a second interpreter).  Every
case here is handed its operands' magnitudes by ops.wgrad_raw, so what runs is what ops.wgrad_launch_info reports: scaled fp16
pairs on the fp16 matrix pipe in the default mode, three bf16 terms under HPL_MATH=bf16x3 (test_cases_take_the_mode_s_family).
Pinned here: its error against the exact result is of the fp32 rounding class on tap-list stencils and dense 1x1 layers,
including the tails (channels past the last 128-block, columns past the last 256-block, slabs that end inside a 16-vertex
stage, taps with empty lists) and the bias gradient of the same call.  tests/test_gpu_wgrad3_exact.py holds the same kernel
bit for bit on operands whose arithmetic is exact."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _table(M, rows_a, F, density, seed, empty_tap=None):
    g = torch.Generator(device='cpu').manual_seed(seed)
    nbr = torch.randint(0, rows_a, (F, M), generator=g, dtype=torch.int32)
    nbr[torch.rand((F, M), generator=g) > density] = -1
    if empty_tap is not None:
        nbr[empty_tap] = -1
    return nbr.to(DEV)


def _ref64(A, nbr, M, C, F, dY, N):
    A64, dY64 = A.double(), dY.double()
    out = torch.zeros(F * C, N, dtype=torch.float64, device=A.device)
    for f in range(F):
        if nbr is None:
            rows = A64[:M, :C]
        else:
            idx = nbr[f].long()
            rows = torch.where((idx >= 0)[:, None], A64[idx.clamp(min=0), :C], torch.zeros((), dtype=torch.float64, device=A.device))
        out[f * C:(f + 1) * C] = rows.t() @ dY64[:M, :N]
    return out


CASES = [
    # M, C, F, N, density, empty tap
    (9000, 580, 15, 1024, 0.42, None),        # bcn1_: 5 channel blocks (the last one 68 wide), 4 column blocks
    (8200, 324, 15, 512, 0.7, 3),             # bcn2_: 3 channel blocks (the last one 68 wide); one tap without neighbours
    (8195, 128, 2, 260, 0.9, None),           # N = 260: 4 columns in the second block; slabs end inside a stage
    (8192, 1024, 1, 1024, 1.0, None),         # dense 1x1 layer
    (9001, 512, 1, 512, 1.0, None),           # dense, odd vertex count
    (8192, 132, 1, 256, 1.0, None),           # dense, 4 channels in the second block
]


def test_cases_take_the_mode_s_family():
    """What the query reports for the cases of this file: fp16 pairs by default, bf16 triples under HPL_MATH=bf16x3 (and the
    fp32 kernel when HPL_MATH=f32 or HPL_WGRAD3=0 keep the hand-off away)."""
    from hplflownet_amd import ops
    math = os.environ.get('HPL_MATH', '')
    want = 0 if (math == 'f32' or os.environ.get('HPL_WGRAD3', '1') == '0') else (3 if math == 'bf16x3' else 2)
    for M, C, F, N, _density, _empty in CASES:
        rows_a = M if F == 1 else M + 53
        A, dY = torch.empty(rows_a, C, device=DEV), torch.empty(M, N, device=DEV)
        nbr = torch.empty((F, M), dtype=torch.int32, device=DEV) if F > 1 else None
        taps = tuple(torch.empty(n, dtype=torch.int32, device=DEV) for n in (F * M, F * M, F + 1)) if F > 1 else None
        assert ops.wgrad_launch_info(A, nbr, M, C, F, dY, N, taps=taps, want_bias=True)['family'] == want, (M, C, F, N)


def _run_case(M, C, F, N, density, empty_tap):
    from hplflownet_amd import ops
    torch.manual_seed(M + C + N)
    rows_a = M if F == 1 else M + 53
    A = torch.randn(rows_a, C, device=DEV) * torch.exp(torch.randn(rows_a, 1, device=DEV))       # rows of very different scale
    dY = torch.randn(M, N, device=DEV) * torch.exp(0.5 * torch.randn(M, 1, device=DEV))
    nbr = _table(M, rows_a, F, density, 5, empty_tap) if F > 1 else None
    taps = ops.tap_lists(nbr) if nbr is not None else None
    got, gb = ops.wgrad_raw(A, nbr, M, C, F, dY, N, taps=taps, want_bias=True)
    ref = _ref64(A, nbr, M, C, F, dY, N)
    err = float((got[:F * C, :N].double() - ref).abs().max() / ref.abs().max())
    # rows / columns of the image outside [F*C, N) stay zero (the kernel's tiles are cut there)
    assert float(got[F * C:].abs().max() if got.shape[0] > F * C else 0.0) == 0.0
    assert float(got[:, N:].abs().max() if got.shape[1] > N else 0.0) == 0.0
    gb_err = float((gb.double() - dY.double().sum(0)).abs().max() / dY.double().sum(0).abs().max())
    return err, gb_err


@pytest.mark.parametrize('M,C,F,N,density,empty_tap', CASES)
def test_wgrad3_matches_float64(M, C, F, N, density, empty_tap):
    err, gb_err = _run_case(M, C, F, N, density, empty_tap)
    assert err < 2e-5, err           # fp32 rounding class (the fp32-MFMA kernel: see the next test)
    assert gb_err < 1e-5, gb_err


def test_wgrad3_error_is_not_larger_than_the_fp32_kernels():
    """The same cases through the fp32-MFMA kernel (HPL_WGRAD3=0, its own interpreter: the switch is read once): the
    split-operand kernel's worst error against float64 stays within 1.5x of it."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import tests.test_gpu_wgrad3 as t\n"
            "print('ERRS', ' '.join('%%.3e' %% t._run_case(*c)[0] for c in t.CASES))\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    errs = {}
    for mode in ('1', '0'):
        r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, HPL_WGRAD3=mode), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        line = [l for l in r.stdout.splitlines() if l.startswith('ERRS')][0]
        errs[mode] = [float(x) for x in line.split()[1:]]
    print('split operands:', errs['1'])
    print('fp32 MFMA     :', errs['0'])
    for a, b in zip(errs['1'], errs['0']):
        assert a <= 1.5 * b + 1e-7, (errs['1'], errs['0'])


@pytest.mark.parametrize('tap', [True, False])
def test_concurrent_streams(tap):
    """The split-operand weight gradient on a side stream while memory-bound kernels of another stream saturate HBM (what the
    native training step does): the same result as alone.  (Round 5 found the hand-counted load waits of the kernel wrong under
    exactly this disturbance -- relative errors of 2-4 -- and replaced the wait in front of the LDS store by a full drain.)"""
    import torch
    from hplflownet_amd import ops
    g = torch.Generator().manual_seed(1)
    M, C, N, F = (18000, 324, 512, 15) if tap else (26000, 512, 512, 1)
    A, dY = torch.randn(M, C, generator=g).to('cuda'), torch.randn(M, N, generator=g).to('cuda')
    nbr = taps = None
    if tap:
        nbr = torch.randint(0, M, (F, M), generator=g).int()
        nbr[torch.rand(F, M, generator=g) < 0.4] = -1
        nbr[0] = torch.arange(M).int()
        nbr = nbr.to('cuda')
        taps = ops.tap_lists(nbr)
    ref = ops.wgrad_raw(A, nbr, M, C, F, dY, N, taps=taps).clone()
    torch.cuda.synchronize()
    X = torch.randn(30000, 1024, device='cuda')
    side = torch.cuda.Stream(priority=-1)
    worst = 0.0
    for _ in range(12):
        ev = torch.cuda.Event()
        ev.record()
        with torch.cuda.stream(side):
            side.wait_event(ev)
            out = ops.wgrad_raw(A, nbr, M, C, F, dY, N, taps=taps)
        for _ in range(4):
            Y = torch.relu(X) + 1
        torch.cuda.synchronize()
        worst = max(worst, float((out - ref).abs().max() / ref.abs().max()))
    assert worst < 1e-5, worst          # (fp32 atomics: the slabs of a tile arrive in any order)
