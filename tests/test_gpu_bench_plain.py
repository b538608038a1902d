"""GPU: a plain `bench.py` run sets up, warms up, times its steps and prints the contract line -- nothing of what `--full` adds
(CPU baseline, training probe, the regions and passes behind the timed loop).  `--full` times the same steps: with the same
arguments both runs dump the same flow."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bench_cpu import check_contract_line  # noqa: E402

#: what every line carries, plain or full
CORE = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
        'dtype', 'data', 'config', 'roofline', 'ranks')
#: what only --full measures
EXTRAS = ('cpu_baseline', 'epe3d', 'speedup_vs_cpu_baseline', 'exact_bf16x3', 'train', 'steady', 'forward_only', 'power',
          'pipelined_output_check', 'single_pair_latency_ms')
STEPS, WARMUP, N = 3, 1, 1024


def _run(extra, out_dir):
    env = dict(os.environ, HPL_BENCH_NO_POWER='1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS), '--warmup', str(WARMUP),
                        '--points', str(N), '--detail', '', '--dump-outputs', str(out_dir)] + extra,
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith('{')]
    assert len(lines) == 1 and p.stdout.strip().splitlines()[-1] == lines[0]
    d = check_contract_line(lines[0], required=CORE)
    assert d['steps'] == STEPS and d['warmup'] == WARMUP and d['value'] > 0
    assert abs(d['value'] - 1e3 / d['ms_per_step']) < 1e-5 * d['value']
    return d, np.load(os.path.join(str(out_dir), 'flow.npy'))


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_times_the_same_steps(tmp_path):
    plain, flow = _run([], tmp_path / 'plain')
    for k in EXTRAS:
        assert k not in plain, k
    assert plain['kernels'] == {}
    assert all(plain['roofline'][k] is None for k in ('achieved', 'peak', 'frac'))
    assert plain['ranks']['ranks_seen'] == 1

    full, flow_full = _run(['--full', '--no-cpu-baseline'], tmp_path / 'full')
    assert full['pipelined_output_check']['max_abs_diff'] == 0.0
    assert full['steady']['steps'] >= STEPS and full['forward_only']['pairs_per_s'] > 0
    assert full['single_pair_latency_ms']['forward_ms'] > 0 and full['train']['ms_per_step'] > 0
    assert any(k.startswith('splat') for k in full['kernels']) and any(k.startswith('slice') for k in full['kernels'])
    assert full['roofline']['peak'] is not None
    assert np.array_equal(flow_full, flow)          # the same timed steps on the same seeded inputs: the same bits
