"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed -- the flow of the pair that step ran, the same as a
plain forward of that pair -- and the same bits on a second run with the same arguments."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, POOL, N = 3, 1, 4, 1024
PREWARM = 3          # bench.py's untimed steps ahead of --warmup


def _bench(out_dir):
    env = dict(os.environ, HPL_BENCH_NO_POWER='1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP),
                        '--points', str(N), '--pool', str(POOL), '--no-cpu-baseline', '--no-train-probe', '--detail', '',
                        '--dump-outputs', str(out_dir)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(os.path.join(str(out_dir), 'flow.npy'))


@pytest.mark.gpu
def test_dumped_flow_is_the_last_timed_step(tmp_path):
    import torch
    import hplflownet_amd as H
    from hplflownet_amd.synthetic import SCALES_FILTER_MAP, fill_module_, synthetic_pair
    got = _bench(tmp_path / 'a')
    assert got.dtype == np.float32 and got.shape == (1, 3, N) and np.isfinite(got).all()
    # the last timed step ran pair (PREWARM + WARMUP + STEPS - 1) % POOL of rank 0's seeds (parallel.sample_seeds: 0, 1, 2, ...)
    seed = (PREWARM + WARMUP + STEPS - 1) % POOL
    dev = torch.device('cuda:0')
    margs = types.SimpleNamespace(dim=3, scales_filter_map=SCALES_FILTER_MAP, evaluate=True, use_leaky=True,
                                  bcn_use_bias=True, bcn_use_norm=True, last_relu=False, DEVICE='cuda')
    model = H.HPLFlowNet(margs)
    fill_module_(model, 1.0, 'hash')
    model = model.to(dev).eval()
    gen = H.GenerateDataUnsymmetric(margs, device=dev, wide_up=model.lattice_hint())
    p1, p2, _ = synthetic_pair(N, seed)
    p1, p2 = (torch.from_numpy(p.T.copy()).to(dev) for p in (p1, p2))
    with torch.no_grad():
        want = model(p1[None], p2[None], gen.build(p1, p2)).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(_bench(tmp_path / 'b'), got)          # seeded inputs and weights: the same bits again
